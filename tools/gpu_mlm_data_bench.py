#!/usr/bin/env python3
"""MLM corpus preparation: where the wall time of src.preprocessing.mlm_data goes, and the Python loops on the same box.

    python tools/gpu_mlm_data_bench.py [--docs 10000,1000000] [--cpu-docs 10000] [--dup 0.2] [--repeats 3]

Synthetic Korean-like documents (no reference and no network needed): two to five paragraphs of Hangul words with some
ASCII, blank runs and single line feeds inside, separated by two or three line feeds; a fraction ``--dup`` of the
paragraphs repeats an earlier one; one paragraph in ten is too short or holds no Hangul.  Per size the stages of
``prepare_mlm_corpus`` are timed apart, each closed by a device synchronisation:

  pack_s     documents to a CSR of code points on the host (snx.textprep.code_point_csr)
  device_s   copy to the device, segment, filter, gather, SHA-256 per batch; first_equal over all digests at the end
  back_s     the valid paragraphs' code points back to the host, the kept ones to ``str``
  write_s    shuffle, split, statistics, both files (src.preprocessing.mlm_data.finish_corpus, write_corpus)

and ``whole_s`` is ``prepare_mlm_corpus`` plus ``write_corpus`` as the CLI calls them.  ``--cpu-docs``: the plain-Python
restatement (tests/textprep_reference.py, the reference's algorithm: one hashlib call and one dict probe per paragraph)
over the first documents, run between the GPU repeats of that size.  Medians with min and max over ``--repeats`` runs after
one warm-up; one JSON line per measurement.  Nothing is asserted about speed."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def synth_documents(n: int, dup: float, seed: int = 0):
    r = random.Random(seed)
    syll = [chr(r.randint(0xAC00, 0xD7A3)) for _ in range(2000)]
    words = ["".join(r.choice(syll) for _ in range(r.randint(1, 5))) for _ in range(20000)]
    ascii_words = [f"w{i}" for i in range(500)]
    earlier, docs = [], []
    for _ in range(n):
        parts = []
        for _ in range(r.randint(2, 5)):
            kind = r.random()
            if earlier and kind < dup:
                parts.append(r.choice(earlier))
            elif kind > 0.95:
                parts.append(" ".join(r.choice(ascii_words) for _ in range(20)))      # no Hangul
            elif kind > 0.90:
                parts.append(r.choice(words))                                          # too short
            else:
                ws = [r.choice(words) if r.random() < 0.85 else r.choice(ascii_words) for _ in range(r.randint(12, 30))]
                text = r.choice([" ", " ", " ", "  ", "\n", " \t"]).join(ws)
                if len(earlier) < 50000:
                    earlier.append(text)
                parts.append(text)
        docs.append(r.choice(["", " "]) + r.choice(["\n\n", "\n\n\n"]).join(parts) + r.choice(["", "\n"]))
    return docs


def gpu_stages(docs, device, batch_code_points, out_dir):
    """The steps of mlm_data.batch_stage and prepare_mlm_corpus, with a clock between them."""
    import numpy as np
    import torch
    from snx import textprep as tx
    from src.preprocessing import mlm_data
    t = {"pack_s": 0.0, "device_s": 0.0, "back_s": 0.0, "write_s": 0.0}
    parts, digests = [], []
    for batch in mlm_data._batches([docs], batch_code_points):
        t0 = time.perf_counter()
        ptr, cps = tx.code_point_csr([x for _, _, x in batch])
        t1 = time.perf_counter()
        seg = tx.segment_csr(ptr, cps, device)
        keep = torch.nonzero(tx.valid_mask(seg.lengths, seg.par_hangul, 50, 0.3)).flatten()
        vptr, vcps = tx.gather_rows(seg.par_ptr, seg.par_cps, keep)
        digests.append(tx.sha256_rows(vptr, vcps))
        hangul, doc = seg.par_hangul[keep], seg.par_doc[keep]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        parts.append(mlm_data.ValidBatch(vptr.cpu().numpy(), vcps.cpu().numpy(), hangul.cpu().numpy(), doc.cpu().numpy(),
                                         None, digests[-1]))
        t3 = time.perf_counter()
        t["pack_s"] += t1 - t0
        t["device_s"] += t2 - t1
        t["back_s"] += t3 - t2
    t0 = time.perf_counter()
    first = mlm_data.dedup_stage(digests)
    t1 = time.perf_counter()
    t["device_s"] += t1 - t0
    unique, lengths, hangul = mlm_data.kept_paragraphs(parts, first == np.arange(first.size))
    t2 = time.perf_counter()
    t["back_s"] += t2 - t1
    corpus = mlm_data.finish_corpus(unique, lengths, hangul, 0.05, 42)
    mlm_data.write_corpus(corpus, out_dir)
    t["write_s"] += time.perf_counter() - t2
    return t, (first.size, len(unique))


def whole(docs, device, batch_code_points, out_dir):
    import torch
    from src.preprocessing import mlm_data
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    corpus = mlm_data.prepare_mlm_corpus([docs], batch_code_points=batch_code_points, device=device)
    mlm_data.write_corpus(corpus, out_dir)
    return time.perf_counter() - t0, corpus


def cpu_run(docs, out_dir):
    from tests import textprep_reference as R
    t0 = time.perf_counter()
    unique, train, val, tb, vb, stats = R.pipeline([docs], 50, 0.3, 0.05, 42)
    for name, data in (("train.txt", tb), ("val.txt", vb)):
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(data)
    return time.perf_counter() - t0, train, val


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=str, default="10000,1000000")
    ap.add_argument("--cpu-docs", type=int, default=10000)
    ap.add_argument("--dup", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch-code-points", type=int, default=1 << 24)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    sizes = [int(x) for x in args.docs.split(",") if x]
    t0 = time.perf_counter()
    docs = synth_documents(max(sizes + [args.cpu_docs]), args.dup)
    print(json.dumps({"bench": "mlm_data_synth", "documents": len(docs), "code_points": sum(len(d) for d in docs),
                      "seconds": round(time.perf_counter() - t0, 2)}), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for n in sizes:
            sub = docs[:n]
            stage_runs, whole_runs, cpu_runs, same = [], [], [], None
            for it in range(args.repeats + 1):
                t, counts = gpu_stages(sub, args.device, args.batch_code_points, tmp)
                w, corpus = whole(sub, args.device, args.batch_code_points, tmp)
                if it:                                       # the first pass warms up
                    stage_runs.append(t)
                    whole_runs.append(w)
                if it and n == args.cpu_docs:                # interleaved with the GPU repeats
                    c, train, val = cpu_run(sub, tmp)
                    cpu_runs.append(c)
                    same = train == corpus.train and val == corpus.val
            line = {"bench": "mlm_data_gpu", "documents": n, "code_points": sum(len(d) for d in sub), "valid": counts[0],
                    "unique": counts[1], "runs": args.repeats, "whole_s": spread(whole_runs)}
            for k in ("pack_s", "device_s", "back_s", "write_s"):
                line[k] = spread([t[k] for t in stage_runs])
            med = {k: line[k]["median"] for k in ("pack_s", "device_s", "back_s", "write_s")}
            line["host_share_of_stages"] = round(1 - med["device_s"] / max(sum(med.values()), 1e-9), 3)
            if cpu_runs:
                line["python_restatement_s"] = spread(cpu_runs)
                line["python_over_whole"] = round(statistics.median(cpu_runs) / statistics.median(whole_runs), 2)
                line["same_files"] = same
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Token retrieval of ``MultiVectorIndex`` (``search_tokens``) against the probed two-phase search on the same compressed
index, with recall.

    python tools/gpu_mv_token_bench.py [--corpora 20000x1024,200000x1024] [--doc-rows 128] [--batches 1,256]
                                       [--query-rows 16,64] [--ncentroids 4096] [--nbits 2] [--ncands 128,1024]
                                       [--nprobes 1,2,4,8] [--repeats 5] [--components 2000] [--doc-components 0]
                                       [--noise 0.5] [--sample-rows 262144]

Corpora and queries are drawn as in tools/gpu_mv_probe_bench.py (``--doc-components`` N > 0: the topical corpus).  The index
is compressed with ``keep_rows=True`` so that the exact ``search`` can give the truth; both timed searches read only the
packed form.  Per (batch, query length, nprobe): one untimed round, then ``--repeats`` rounds that time ``search_tokens`` and
``search_two_phase(ncand, nprobe)`` at every ``--ncands`` value one after the other (interleaved, so drift of the machine
hits all alike).  A time is a host clock around a call that ends in a device synchronise; median with the smallest and
the largest, in seconds.  recall@10: the mean share of the exact top 10 in each search's top 10.  One JSON line per
configuration; nothing is asserted."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gpu_dense2p_bench import spread  # noqa: E402
from gpu_ivf_bench import recall, timed  # noqa: E402
from gpu_mv_centroid_bench import noisy_unit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", type=str, default="20000x1024,200000x1024")
    ap.add_argument("--doc-rows", type=int, default=128)
    ap.add_argument("--batches", type=str, default="1,256")
    ap.add_argument("--query-rows", type=str, default="16,64")
    ap.add_argument("--ncentroids", type=int, default=4096)
    ap.add_argument("--nbits", type=int, default=2)
    ap.add_argument("--ncands", type=str, default="128,1024")
    ap.add_argument("--nprobes", type=str, default="1,2,4,8")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=2000)
    ap.add_argument("--doc-components", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--sample-rows", type=int, default=262144)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_mv_token_bench: needs a GPU")
    from snx.retrieval import MultiVectorIndex
    dev = torch.device(args.device)
    ncands = [int(v) for v in args.ncands.split(",")]
    for nd, dim in ((int(a), int(b)) for a, b in (c.split("x") for c in args.corpora.split(","))):
        gen = torch.Generator(device=dev).manual_seed(7)
        lo, hi = max(1, args.doc_rows * 3 // 4), args.doc_rows * 5 // 4
        dlen = torch.randint(lo, hi + 1, (nd,), generator=gen, device=dev)
        ptr = [0] + torch.cumsum(dlen, 0).cpu().tolist()
        doc_of = torch.repeat_interleave(torch.arange(nd, device=dev), dlen)
        topics = torch.randint(0, args.components, (nd, max(args.doc_components, 1)), generator=gen, device=dev)
        centres = torch.randn((args.components, dim), generator=gen, device=dev) / dim ** 0.5
        store = torch.empty((ptr[-1], dim), dtype=torch.bfloat16, device=dev)
        for s in range(0, ptr[-1], 1 << 17):
            m = min(1 << 17, ptr[-1] - s)
            pick = torch.randint(0, args.components, (m,), generator=gen, device=dev)
            if args.doc_components > 0:
                pick = topics[doc_of[s:s + m], pick % args.doc_components]
            store[s:s + m] = noisy_unit(centres[pick], args.noise / dim ** 0.5, gen).to(torch.bfloat16)
        index = MultiVectorIndex(dim, dev)
        index.add(store, ptr)
        index.build()
        shape = {"bench": "mv_token", "nd": nd, "doc_rows_total": ptr[-1], "dim": dim, "nbits": args.nbits,
                 "components": args.components, "doc_components": args.doc_components, "noise": args.noise}
        train_s, _ = timed(lambda: index.train_centroids(args.ncentroids, sample_rows=args.sample_rows))
        index.compress(args.nbits, keep_rows=True)
        lists_s, _ = timed(index._row_lists)
        index._lists()
        print(json.dumps({**shape, "ncentroids": int(index.centroids.shape[0]), "train_s": round(train_s, 3),
                          "row_lists_s": round(lists_s, 4)}), flush=True)
        for nq in (int(v) for v in args.batches.split(",")):
            for L in (int(v) for v in args.query_rows.split(",")):
                src = torch.randint(0, nd, (nq,), generator=gen, device=dev).cpu().tolist()
                take = torch.cat([ptr[d] + torch.randint(0, ptr[d + 1] - ptr[d], (L,), generator=gen, device=dev)
                                  for d in src])
                qmv = noisy_unit(store[take].float(), args.noise / dim ** 0.5, gen).to(torch.bfloat16)
                qptr = list(range(0, nq * L + 1, L))
                want = index.search(qmv, qptr, 10)[1]
                for nprobe in (int(v) for v in args.nprobes.split(",")):
                    runs = {"token": lambda: index.search_tokens(qmv, qptr, 10, nprobe)}
                    for ncand in ncands:
                        runs[f"two_phase_{ncand}"] = lambda ncand=ncand: index.search_two_phase(qmv, qptr, 10, ncand,
                                                                                               nprobe=nprobe)
                    rec = {name: round(recall(timed(f)[1][1], want, 10), 4) for name, f in runs.items()}   # untimed round
                    t = {name: [] for name in runs}
                    for _ in range(args.repeats):
                        for name, f in runs.items():
                            t[name].append(timed(f)[0])
                    s = {name: spread(v) for name, v in t.items()}
                    row = {**shape, "nq": nq, "query_rows": L, "nprobe": nprobe}
                    for name in runs:
                        row[name] = {**s[name], "recall@10": rec[name]}
                        if name != "token":
                            row[name]["over_token"] = round(s[name]["median_s"] / s["token"]["median_s"], 2)
                    print(json.dumps(row), flush=True)
        del index, store


if __name__ == "__main__":
    main()

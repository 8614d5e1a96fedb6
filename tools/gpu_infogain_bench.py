#!/usr/bin/env python3
"""Information-gain scores of synonym pairs: the GPU path at 2,000 pairs x 20,000 terms x 768 and at 100,000 pairs x
100,000 terms x 768 and x 1024, torch.cdist in float64 + topk on the same GPU at the first size, and the Python loop at the
first size -- the restatement's (tests/infogain_reference.py), or with ``--reference DIR`` the reference's own
compute_information_gain_batch (it needs scipy; the checkout is only read on the machine that has it, nothing here needs it
on a GPU machine).

    python tools/gpu_infogain_bench.py [--sizes 2000x20000x768,100000x100000x768,100000x100000x1024] [--repeats 5]
                                       [--cpu-size 2000x20000x768] [--reference DIR]

Synthetic embeddings: standard normal fp32 from a seed; a source is a corpus row, its target that row plus a tenth of
another normal vector.  Everything is normalised on the host first, outside the timed window, as is the upload of the
corpus (``upload_s``).  The GPU time is a host clock around snx.infogain.information_gain, which ends in copies to the host;
one untimed run warms up each size, then the median of ``--repeats`` runs with the smallest and the largest.  ``pair_rows``
is pairs x terms x 2, the (query, corpus row) distances the two searches form, and ``gfma_s`` that times D over the median:
the float64 fused multiply-adds per second of the whole call, not of a kernel.  One JSON line per measurement; nothing is
asserted about speed."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

K_ENTROPY, K_NEIGHBORHOOD = 10, 50


def parse_size(text: str):
    pairs, terms, dim = (int(x) for x in text.split("x"))
    return pairs, terms, dim


def synth(pairs: int, terms: int, dim: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    corpus = rng.standard_normal((terms, dim), dtype=np.float32)
    a, b = rng.integers(0, terms, size=pairs), rng.integers(0, terms, size=pairs)
    src = corpus[a]
    tgt = corpus[a] + np.float32(0.1) * corpus[b]
    return corpus, src, tgt


def normalize(x):
    return x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-10)


def spread(times):
    return {"median_s": round(statistics.median(times), 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4),
            "runs": len(times)}


def gpu_run(size, repeats: int, device: str, batch_size: int):
    import torch
    from snx.infogain import L2Index, information_gain
    pairs, terms, dim = size
    corpus, src, tgt = (normalize(x) for x in synth(*size))
    t0 = time.perf_counter()
    index = L2Index(corpus, device)
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0
    times = []
    for r in range(repeats + 1):                              # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ig, _, _ = information_gain(index, src, tgt, K_ENTROPY, K_NEIGHBORHOOD, batch_size)
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
    s = spread(times)
    rows = 2.0 * pairs * terms
    return {"upload_s": round(upload, 3), **s, "pair_rows": rows, "gfma_s": round(rows * dim / s["median_s"] / 1e9, 1),
            "ig_mean": float(ig.mean())}


def cdist_run(size, repeats: int, device: str):
    """float64 cdist + topk for both searches (the gather and the formulas left out): the off-the-shelf GPU form."""
    import torch
    pairs, terms, dim = size
    corpus, src, tgt = (torch.from_numpy(normalize(x)).to(device).double() for x in synth(*size))
    times = []
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = torch.cdist(tgt, corpus, compute_mode="donot_use_mm_for_euclid_dist").topk(K_ENTROPY + 1, largest=False)
        b = torch.cdist(src, corpus, compute_mode="donot_use_mm_for_euclid_dist").topk(K_NEIGHBORHOOD, largest=False)
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
        del a, b
    return spread(times)


def restatement_run(size):
    from tests import infogain_reference as R
    corpus, src, tgt = synth(*size)
    t0 = time.perf_counter()
    out = [R.information_gain(src[s:s + 100], tgt[s:s + 100], corpus, K_ENTROPY, K_NEIGHBORHOOD)
           for s in range(0, size[0], 100)]                   # 100 pairs at a time bound the float64 distance matrix
    return {"what": "the restatement's loop (tests/infogain_reference.py)", "seconds": round(time.perf_counter() - t0, 2),
            "ig_mean": float(np.concatenate([o[0] for o in out]).mean())}


def reference_run(size, root: str):
    spec = importlib.util.spec_from_file_location("ref_information_gain", os.path.join(root, "src", "information_gain.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    corpus, src, tgt = synth(*size)
    cfg = mod.InformationGainConfig(k_entropy=K_ENTROPY, k_neighborhood=K_NEIGHBORHOOD, use_faiss=False)
    t0 = time.perf_counter()
    ig, _, _ = mod.compute_information_gain_batch(src, tgt, corpus, cfg)
    return {"what": "the reference's compute_information_gain_batch", "seconds": round(time.perf_counter() - t0, 2),
            "ig_mean": float(ig.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="2000x20000x768,100000x100000x768,100000x100000x1024",
                    help="pairs x terms x dim of the GPU runs; empty: no GPU side")
    ap.add_argument("--cdist-size", type=str, default="2000x20000x768", help="empty: no torch.cdist row")
    ap.add_argument("--cpu-size", type=str, default="2000x20000x768", help="empty: no CPU side")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=10000, help="pairs per device batch")
    ap.add_argument("--reference", type=str, default=None, help="time the reference's own loop instead of the restatement's")
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    sizes = [parse_size(x) for x in args.sizes.split(",") if x]
    if sizes or args.cdist_size:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("gpu_infogain_bench: the GPU side needs a GPU (--sizes '' --cdist-size '' times the CPU side alone)")
    for size in sizes:
        print(json.dumps({"bench": "infogain_gpu", "pairs": size[0], "terms": size[1], "dim": size[2],
                          "batch_size": args.batch_size, **gpu_run(size, args.repeats, args.device, args.batch_size)}),
              flush=True)
    if args.cdist_size:
        size = parse_size(args.cdist_size)
        print(json.dumps({"bench": "infogain_torch_cdist_f64_topk", "pairs": size[0], "terms": size[1], "dim": size[2],
                          **cdist_run(size, args.repeats, args.device)}), flush=True)
    if args.cpu_size:
        size = parse_size(args.cpu_size)
        run = reference_run(size, args.reference) if args.reference else restatement_run(size)
        print(json.dumps({"bench": "infogain_cpu", "pairs": size[0], "terms": size[1], "dim": size[2], **run}), flush=True)


if __name__ == "__main__":
    main()

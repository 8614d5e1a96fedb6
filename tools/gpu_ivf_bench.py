#!/usr/bin/env python3
"""IVF-Flat against the exact dense search on one GPU: build seconds, search seconds and recall.

    python tools/gpu_ivf_bench.py [--nd 1000000] [--dim 1024] [--nq 4096] [--k 100] [--nlists 1000,4000]
                                  [--nprobes 1,8,32,0] [--repeats 5] [--components 2000] [--noise 1.0]

Corpus: a synthetic Gaussian mixture made on the device from a seed -- ``--components`` standard-normal centres, every doc
and every query a centre plus ``--noise`` times a standard-normal vector, L2-normalised.  Uniform random vectors would have
no cluster structure, and recall on them is about nprobe / nlist by construction.
Per ``nlist``: ``build_s`` is add + build() of an ``IvfFlatIndex`` (the index's own k-means over all docs, the assignment,
the sort and the row copy), one run.  Then ``--repeats`` rounds, each timing ``DenseIndex.search`` and the IVF search at every
``nprobe`` one after the other (interleaved, so drift of the machine hits both alike), after one untimed round that warms
every shape up; a time is a host clock around a call that ends in a device synchronise.  ``nprobe`` 0 stands for every list,
capped at the search's limit of 1024.  Reported: the median with the smallest and the largest, the ratio of the medians
to the exact search of the same rounds, and recall@10 / recall@100 of the IVF ids against the exact ids.  One JSON line
per measurement; nothing is asserted."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def mixture(n: int, dim: int, centres, noise: float, gen, chunk: int = 65536):
    import torch
    out = torch.empty((n, dim), dtype=torch.float32, device=centres.device)
    for s in range(0, n, chunk):
        m = min(chunk, n - s)
        pick = torch.randint(0, centres.shape[0], (m,), generator=gen, device=centres.device)
        x = centres[pick] + noise * torch.randn((m, dim), generator=gen, device=centres.device)
        out[s:s + m] = x / x.norm(dim=1, keepdim=True)
    return out


def spread(times):
    return {"median_s": round(statistics.median(times), 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4),
            "runs": len(times)}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def recall(got, want, r: int) -> float:
    """Mean share of the exact top r found among the IVF top r."""
    g, w = got[:, :r], want[:, :r]
    return float((g.unsqueeze(2) == w.unsqueeze(1)).any(dim=2).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nlists", type=str, default="1000,4000")
    ap.add_argument("--nprobes", type=str, default="1,8,32,0", help="0: every list (at most 1024)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=2000)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_ivf_bench: needs a GPU")
    from snx.retrieval import K_MAX, DenseIndex, IvfFlatIndex
    dev = torch.device(args.device)
    gen = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn((args.components, args.dim), generator=gen, device=dev)
    E = mixture(args.nd, args.dim, centres, args.noise, gen)
    Q = mixture(args.nq, args.dim, centres, args.noise, gen)
    shape = {"nd": args.nd, "dim": args.dim, "nq": args.nq, "k": args.k, "components": args.components, "noise": args.noise}
    flat = DenseIndex(args.dim, dev)
    flat.add(E)
    flat.build()
    _, exact = timed(lambda: flat.search(Q, args.k))          # warm-up, and the ids recall is measured against
    exact_docs = exact[1]
    for nlist in (int(x) for x in args.nlists.split(",") if x):
        ivf = IvfFlatIndex(args.dim, nlist, dev, niter=args.niter)

        def build():
            ivf.add(E)
            return ivf.build()
        build_s, _ = timed(build)
        sizes = (ivf.list_ptr[1:] - ivf.list_ptr[:-1]).double()
        print(json.dumps({"bench": "ivf_build", **shape, "nlist": nlist, "niter": args.niter, "build_s": round(build_s, 3),
                          "max_list": ivf.max_list, "mean_list": round(float(sizes.mean()), 1),
                          "empty_lists": int((sizes == 0).sum())}), flush=True)
        nprobes = sorted({min(nlist, K_MAX) if int(x) == 0 else int(x) for x in args.nprobes.split(",") if x})
        times = {"exact": [], **{p: [] for p in nprobes}}
        found = {}
        for r in range(args.repeats + 1):                    # round 0 warms every shape up
            t, _ = timed(lambda: flat.search(Q, args.k))
            if r:
                times["exact"].append(t)
            for p in nprobes:
                t, out = timed(lambda: ivf.search(Q, args.k, nprobe=p))
                if r:
                    times[p].append(t)
                found[p] = out[1]
        base = spread(times["exact"])
        print(json.dumps({"bench": "dense_exact_search", **shape, "beside_nlist": nlist, **base}), flush=True)
        for p in nprobes:
            s = spread(times[p])
            print(json.dumps({"bench": "ivf_search", **shape, "nlist": nlist, "nprobe": p, **s,
                              "exact_over_ivf": round(base["median_s"] / s["median_s"], 2),
                              "recall_at_10": round(recall(found[p], exact_docs, min(10, args.k)), 4),
                              "recall_at_k": round(recall(found[p], exact_docs, args.k), 4)}), flush=True)
        del ivf


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The centroid-interaction candidate search of ``MultiVectorIndex`` against its exact search, with recall.

    python tools/gpu_mv_centroid_bench.py [--nd 20000] [--doc-rows 128] [--dim 1024] [--nq 256] [--query-rows 16,64]
                                          [--ncentroids 1024,4096] [--ncands 128,512,1024] [--k 100] [--repeats 5]
                                          [--components 2000] [--noise 0.5] [--sample-rows 262144]

Corpus: bf16 rows drawn on the device from a Gaussian mixture (``--components`` standard-normal centres, a row is a centre
plus ``--noise`` times a standard-normal vector, L2-normalised, as tools/gpu_ivf_bench.py draws its vectors); documents of
``--doc-rows`` +- 25 % rows.  A query is ``query-rows`` rows of one document, each with fresh noise: uniform random rows
would have no centroid structure and would say nothing about recall.
Per number of centroids: ``train_s`` is ``train_centroids`` (k-means over ``--sample-rows`` evenly spaced rows, then the
codes of every row), ``assign_s`` the code assignment alone.  Per (query length, ncand): one untimed round, then
``--repeats`` rounds that time, one after the other (interleaved, so drift of the machine hits all alike), the exact
``search`` at ``--k``, the candidate pass (table + walk + select + merge), the rescore (rescore + order) over kept
candidates, and ``search_two_phase`` as a whole.  A time is a host clock around a call that ends in a device synchronise;
reported as the median with the smallest and the largest, in seconds.  recall@r: the mean share of the exact top r found
in the two-phase top r.  One JSON line per configuration; nothing is asserted."""
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


def noisy_unit(x, noise, gen):
    import torch
    x = x + noise * torch.randn(x.shape, generator=gen, device=x.device)
    return x / x.norm(dim=1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", type=int, default=20000)
    ap.add_argument("--doc-rows", type=int, default=128)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--query-rows", type=str, default="16,64")
    ap.add_argument("--ncentroids", type=str, default="1024,4096")
    ap.add_argument("--ncands", type=str, default="128,512,1024")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=2000)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--sample-rows", type=int, default=262144)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_mv_centroid_bench: needs a GPU")
    from snx.retrieval import MultiVectorIndex
    dev = torch.device(args.device)
    gen = torch.Generator(device=dev).manual_seed(7)
    lo, hi = max(1, args.doc_rows * 3 // 4), args.doc_rows * 5 // 4
    dlen = torch.randint(lo, hi + 1, (args.nd,), generator=gen, device=dev)
    ptr = [0] + torch.cumsum(dlen, 0).cpu().tolist()
    centres = torch.randn((args.components, args.dim), generator=gen, device=dev) / args.dim ** 0.5   # about unit length
    store = torch.empty((ptr[-1], args.dim), dtype=torch.bfloat16, device=dev)
    for s in range(0, ptr[-1], 1 << 17):
        m = min(1 << 17, ptr[-1] - s)
        pick = torch.randint(0, args.components, (m,), generator=gen, device=dev)
        store[s:s + m] = noisy_unit(centres[pick], args.noise / args.dim ** 0.5, gen).to(torch.bfloat16)
    index = MultiVectorIndex(args.dim, dev)
    index.add(store, ptr)
    index.build()
    shape = {"bench": "mv_centroid", "nd": args.nd, "doc_rows_total": ptr[-1], "dim": args.dim, "nq": args.nq,
             "components": args.components, "noise": args.noise}
    queries = {}
    for L in (int(v) for v in args.query_rows.split(",")):
        src = torch.randint(0, args.nd, (args.nq,), generator=gen, device=dev).cpu().tolist()
        take = torch.cat([ptr[d] + torch.randint(0, ptr[d + 1] - ptr[d], (L,), generator=gen, device=dev) for d in src])
        queries[L] = (noisy_unit(store[take].float(), args.noise / args.dim ** 0.5, gen).to(torch.bfloat16),
                      list(range(0, args.nq * L + 1, L)))
    for nc in (int(v) for v in args.ncentroids.split(",")):
        train_s, _ = timed(lambda: index.train_centroids(nc, sample_rows=args.sample_rows))
        assign_s, _ = timed(lambda: index.set_centroids(index.centroids.float()))
        print(json.dumps({**shape, "ncentroids": nc, "sample_rows": args.sample_rows, "train_s": round(train_s, 3),
                          "assign_s": round(assign_s, 3)}), flush=True)
        for L, (qmv, qptr) in queries.items():
            for ncand in (int(v) for v in args.ncands.split(",")):
                k = min(args.k, ncand)
                exact = lambda: index.search(qmv, qptr, k)
                cands = lambda: index.candidates(qmv, qptr, ncand)
                both = lambda: index.search_two_phase(qmv, qptr, k, ncand)
                (_, want), (_, (_, cd)), (_, got) = timed(exact), timed(cands), timed(both)     # the untimed round
                plist = index._queries("bench", qmv, qptr, 0, 0)[1]
                resc = lambda: index._rescore(qmv, plist, cd, 0, k, 0)
                timed(resc)
                t = {"search": [], "candidates": [], "rescore": [], "two_phase": []}
                for _ in range(args.repeats):
                    for name, f in (("search", exact), ("candidates", cands), ("rescore", resc), ("two_phase", both)):
                        t[name].append(timed(f)[0])
                s = {name: spread(v) for name, v in t.items()}
                print(json.dumps({**shape, "ncentroids": nc, "query_rows": L, "ncand": ncand, "k": k, **s,
                                  "search_over_two_phase": round(s["search"]["median_s"] / s["two_phase"]["median_s"], 2),
                                  "ranges_disjoint": s["two_phase"]["max_s"] < s["search"]["min_s"] or
                                  s["search"]["max_s"] < s["two_phase"]["min_s"],
                                  "recall@10": round(recall(got[1], want[1], min(10, k)), 4),
                                  f"recall@{k}": round(recall(got[1], want[1], k), 4)}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The exact multi-vector (MaxSim) search against the only other route to the same answer: snx_maxsim_pairs over all
nq x nd pairs, in slices of queries, followed by torch.topk.

    python tools/gpu_mv_search_bench.py [--nd 20000] [--doc-rows 128] [--dim 1024] [--nq 256] [--query-rows 16,64] [--k 100]
                                        [--repeats 5] [--pair-slice 16]

Synthetic unit rows in bf16, made on the device from a seed; documents of ``--doc-rows`` +- 25 % rows.  The documents and
the queries of every length live in ONE store, as the pair kernel needs it; ``MultiVectorIndex`` reads the documents as a
view of it.  The pair route calls the C entry point with index arrays made before the clock starts, so that the host loops
of ``snx.teacher.maxsim_pairs`` are not counted against it.  Per query length: one untimed round, then ``--repeats`` rounds
that time the two routes one after the other (interleaved, so drift of the machine hits both alike).  A time is a host
clock around a call that ends in a device synchronise.  Reported per route: the median with the smallest and the largest,
in seconds; the ratio of the medians and whether the ranges [min, max] are disjoint.  The two results are compared bit for
bit (scores) and id for id.  One JSON line per query length; nothing else is asserted."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gpu_dense2p_bench import spread  # noqa: E402
from gpu_ivf_bench import timed  # noqa: E402


def pair_route(store, ptr, nd, q0, nq, k, slices):
    """Top k per query from snx_maxsim_pairs over every (query, doc) pair; ``slices``: prebuilt (first query, queries,
    pair_q, pair_d, npairs) ctypes arrays."""
    import torch
    from snx._lib import call, fn
    from snx.ops import _p, _stream
    nseq, max_rows, dev = len(ptr) - 1, max(b - a for a, b in zip(ptr, ptr[1:])), store.device
    hptr = (C.c_int64 * (nseq + 1))(*ptr)
    scores = torch.empty((nq, nd), dtype=torch.float32, device=dev)   # this route's nq x nd matrix
    for s, m, hq, hd, n in slices:
        ws = torch.empty(int(fn("snx_maxsim_workspace_bytes")(nseq, n, max_rows)), dtype=torch.uint8, device=dev)
        call("snx_maxsim_pairs", _p(store), 0, int(store.shape[0]), int(store.shape[1]), hptr, nseq, hq, hd, n, max_rows,
             _p(scores[s:s + m]), _p(ws), ws.numel(), _stream())
    top = torch.topk(scores, k, dim=1)                                 # sorted; ties are not ordered by doc id
    return top.values, top.indices.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", type=int, default=20000)
    ap.add_argument("--doc-rows", type=int, default=128)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--query-rows", type=str, default="16,64")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pair-slice", type=int, default=16, help="queries per snx_maxsim_pairs call of the pair route")
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_mv_search_bench: needs a GPU")
    from snx.retrieval import MultiVectorIndex
    dev = torch.device(args.device)
    gen = torch.Generator(device=dev).manual_seed(7)
    qlens = [int(v) for v in args.query_rows.split(",")]
    lo, hi = max(1, args.doc_rows * 3 // 4), args.doc_rows * 5 // 4
    dlen = torch.randint(lo, hi + 1, (args.nd,), generator=gen, device=dev).cpu().tolist()
    lens = dlen + [L for L in qlens for _ in range(args.nq)]
    ptr = [0]
    for n in lens:
        ptr.append(ptr[-1] + n)
    store = torch.empty((ptr[-1], args.dim), dtype=torch.bfloat16, device=dev)
    for s in range(0, ptr[-1], 1 << 18):                               # unit rows, a block at a time
        x = torch.randn((min(1 << 18, ptr[-1] - s), args.dim), generator=gen, device=dev)
        store[s:s + x.shape[0]] = (x / x.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
    nd, drows = args.nd, ptr[args.nd]
    index = MultiVectorIndex(args.dim, dev)
    index.add(store[:drows], ptr[:nd + 1])
    index.build()
    for i, L in enumerate(qlens):
        q0 = nd + i * args.nq                                          # first query sequence of this length
        qmv = store[ptr[q0]:ptr[q0 + args.nq]]
        qptr = [v - ptr[q0] for v in ptr[q0:q0 + args.nq + 1]]
        slices = []
        for s in range(0, args.nq, args.pair_slice):
            m = min(args.pair_slice, args.nq - s)
            n = m * nd
            hq = (C.c_int32 * n)(*[q0 + s + j for j in range(m) for _ in range(nd)])
            hd = (C.c_int32 * n)(*(list(range(nd)) * m))
            slices.append((s, m, hq, hd, n))
        search = lambda: index.search(qmv, qptr, args.k)
        pairs = lambda: pair_route(store, ptr, nd, q0, args.nq, args.k, slices)
        (_, a), (_, b) = timed(search), timed(pairs)                   # the untimed round; and the two answers
        same_scores = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
        same_docs = float((a[1] == b[1]).float().mean())
        t_search, t_pairs = [], []
        for _ in range(args.repeats):
            t_search.append(timed(search)[0])
            t_pairs.append(timed(pairs)[0])
        s1, s2 = spread(t_search), spread(t_pairs)
        print(json.dumps({"bench": "mv_search", "nd": nd, "doc_rows_total": drows, "dim": args.dim, "nq": args.nq,
                          "query_rows": L, "k": args.k, "search": s1, "pairs_topk": s2,
                          "pairs_over_search": round(s2["median_s"] / s1["median_s"], 3),
                          "ranges_disjoint": s1["max_s"] < s2["min_s"] or s2["max_s"] < s1["min_s"],
                          "scores_bit_equal": same_scores, "docs_equal_fraction": same_docs}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The residual-compressed store of ``MultiVectorIndex`` against its bf16 rows: rescore time, bytes, recall.

    python tools/gpu_mv_residual_bench.py [--nd 20000] [--doc-rows 128] [--dim 1024] [--nq 256] [--query-rows 16,64]
                                          [--ncentroids 4096] [--ncands 128,1024] [--nbits 1,2,4] [--k 100]
                                          [--repeats 5] [--components 2000] [--noise 0.5] [--sample-rows 262144]

Corpus and queries: those of tools/gpu_mv_centroid_bench.py (a Gaussian mixture on the device; a query is rows of one
document with fresh noise).  One index holds the bf16 rows and the centroids; per ``nbits`` a second one shares its tensors
and is compressed with ``keep_rows=True``, so that both rescores run in one process over the same candidates.
``compress_s`` is one ``compress`` with the quantile defaults, after an untimed one.  ``bytes_rows`` is the bf16 store,
``bytes_packed`` the codes and the residuals that replace it.  Per (query length, ncand): the candidates are computed once;
one untimed round, then ``--repeats`` rounds that time, one after the other (interleaved, so drift of the machine hits all
alike), the rescore + order over the bf16 rows (``snx_mv_rescore``) and over each packed store (table + score + order,
``snx_mv_rescore_residual``).  A time is a host clock around a call that ends in a device synchronise; reported as the
median with the smallest and the largest, in seconds.  ``not_slower``: the packed rescore's fastest round is not above the
bf16 rescore's slowest (ranges disjoint in its favour or overlapping, never reversed).  recall@r: the mean share of the exact
``search``'s top r found in the two-phase top r, for the bf16 rows and for each packed store; it describes this synthetic
corpus only.  One JSON line per configuration; nothing is asserted."""
import argparse
import copy
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
    ap.add_argument("--nd", type=int, default=20000)
    ap.add_argument("--doc-rows", type=int, default=128)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--query-rows", type=str, default="16,64")
    ap.add_argument("--ncentroids", type=int, default=4096)
    ap.add_argument("--ncands", type=str, default="128,1024")
    ap.add_argument("--nbits", type=str, default="1,2,4")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=2000)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--sample-rows", type=int, default=262144)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_mv_residual_bench: needs a GPU")
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
    plain = MultiVectorIndex(args.dim, dev)
    plain.add(store, ptr)
    plain.build().train_centroids(args.ncentroids, sample_rows=args.sample_rows)
    nbits_all = [int(v) for v in args.nbits.split(",")]
    shape = {"bench": "mv_residual", "nd": args.nd, "doc_rows_total": ptr[-1], "dim": args.dim, "nq": args.nq,
             "ncentroids": int(plain.centroids.shape[0]), "components": args.components, "noise": args.noise}
    nbytes = lambda t: t.numel() * t.element_size()
    packed = {}
    for nb in nbits_all:
        packed[nb] = copy.copy(plain)                            # shares the rows, the codes and the centroids
        packed[nb].compress(nb, keep_rows=True)
        compress_s, _ = timed(lambda: packed[nb].compress(nb, keep_rows=True))
        print(json.dumps({**shape, "nbits": nb, "compress_s": round(compress_s, 3), "bytes_rows": nbytes(plain.rows),
                          "bytes_packed": nbytes(plain.codes) + nbytes(packed[nb].residuals),
                          "bytes_centroids": nbytes(plain.centroids)}), flush=True)
    for L in (int(v) for v in args.query_rows.split(",")):
        src = torch.randint(0, args.nd, (args.nq,), generator=gen, device=dev).cpu().tolist()
        take = torch.cat([ptr[d] + torch.randint(0, ptr[d + 1] - ptr[d], (L,), generator=gen, device=dev) for d in src])
        qmv = noisy_unit(store[take].float(), args.noise / args.dim ** 0.5, gen).to(torch.bfloat16)
        qptr = list(range(0, args.nq * L + 1, L))
        plist = plain._queries("bench", qmv, qptr, 0, 0)[1]
        exact = {}                                               # k -> the exact search's documents
        for ncand in (int(v) for v in args.ncands.split(",")):
            k = min(args.k, ncand)
            if k not in exact:
                exact[k] = plain.search(qmv, qptr, k)[1]
            want = exact[k]
            cd = plain.candidates(qmv, qptr, ncand)[1]
            legs = {"rows": lambda: plain._rescore(qmv, plist, cd, 0, k, 0)}
            for nb in nbits_all:
                legs[f"nbits{nb}"] = lambda nb=nb: packed[nb]._rescore(qmv, plist, cd, 0, k, 0)
            got = {name: timed(f)[1][1] for name, f in legs.items()}                     # the untimed round
            t = {name: [] for name in legs}
            for _ in range(args.repeats):
                for name, f in legs.items():
                    t[name].append(timed(f)[0])
            s = {name: spread(v) for name, v in t.items()}
            out = {**shape, "query_rows": L, "ncand": ncand, "k": k, "rescore_s": s}
            for name in legs:
                out[f"recall@10_{name}"] = round(recall(got[name], want, min(10, k)), 4)
                out[f"recall@{k}_{name}"] = round(recall(got[name], want, k), 4)
                if name != "rows":
                    out[f"rows_over_{name}"] = round(s["rows"]["median_s"] / s[name]["median_s"], 2)
                    out[f"not_slower_{name}"] = s[name]["min_s"] <= s["rows"]["max_s"]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

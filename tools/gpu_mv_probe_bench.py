#!/usr/bin/env python3
"""The probed candidate pass of ``MultiVectorIndex`` (``nprobe`` > 0) against the full walk (``nprobe`` = 0), with recall.

    python tools/gpu_mv_probe_bench.py [--corpora 20000x1024,200000x128] [--doc-rows 128] [--nq 256] [--query-rows 16,64]
                                       [--ncentroids 4096] [--ncands 128,1024] [--nprobes 1,2,4,8] [--k 100] [--repeats 5]
                                       [--components 2000] [--doc-components 0] [--noise 0.5] [--sample-rows 262144]

Corpora (``documents x dim``) and queries are drawn as in tools/gpu_mv_centroid_bench.py; with ``--doc-components`` N > 0
a document draws its rows from N of the mixture's centres, its own topics, and not from all of them.  Per corpus:
``train_s`` is ``train_centroids``, ``lists_s`` the build of the inverted lists (one run each).  Per (query length, ncand): one untimed
round, then ``--repeats`` rounds that time ``candidates`` at ``nprobe`` 0 (the full walk, this tree's parent's code path)
and at every ``--nprobes`` value one after the other (interleaved, so drift of the machine hits all alike).  A time is a
host clock around a call that ends in a device synchronise; median with the smallest and the largest, in seconds.
``probed``: the mean of |P(q)| / nd, the probe sets taken from fp32 products (not the table's bf16 keys: a mean, not a
check).  recall@r: the mean share of the exact top r (``search``, run once) in the top r of ``search_two_phase`` at that
``nprobe``.  One JSON line per configuration; nothing is asserted."""
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


def probed_fraction(index, qmv, qptr, nprobe):
    """Mean |P(q)| / nd: owns [nd, nc] marks the centroids a document owns a row of, hit [nq, nc] the centroids a query
    probes."""
    import torch
    nd, nc, dev = index.num_docs, int(index.centroids.shape[0]), index.device
    doc_of = torch.repeat_interleave(torch.arange(nd, device=dev), torch.tensor(index._ptr, device=dev).diff())
    owns = torch.zeros((nd, nc), dtype=torch.bfloat16, device=dev)
    owns[doc_of, index._codes_of(torch.arange(index.num_rows, device=dev))] = 1
    top = (qmv.float() @ index.centroids.float().T).topk(min(nprobe, nc), dim=1).indices
    hit = torch.zeros((len(qptr) - 1, nc), dtype=torch.bfloat16, device=dev)
    q_of = torch.repeat_interleave(torch.arange(len(qptr) - 1, device=dev), torch.tensor(qptr, device=dev).diff())
    hit[q_of[:, None].expand_as(top), top] = 1
    return float(((hit @ owns.T) > 0).float().sum(dim=1).mean()) / nd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", type=str, default="20000x1024,200000x128")
    ap.add_argument("--doc-rows", type=int, default=128)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--query-rows", type=str, default="16,64")
    ap.add_argument("--ncentroids", type=int, default=4096)
    ap.add_argument("--ncands", type=str, default="128,1024")
    ap.add_argument("--nprobes", type=str, default="1,2,4,8")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=2000)
    ap.add_argument("--doc-components", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--sample-rows", type=int, default=262144)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_mv_probe_bench: needs a GPU")
    from snx.retrieval import MultiVectorIndex
    dev = torch.device(args.device)
    nprobes = [0] + [int(v) for v in args.nprobes.split(",")]
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
        shape = {"bench": "mv_probe", "nd": nd, "doc_rows_total": ptr[-1], "dim": dim, "nq": args.nq,
                 "components": args.components, "doc_components": args.doc_components, "noise": args.noise}
        train_s, _ = timed(lambda: index.train_centroids(args.ncentroids, sample_rows=args.sample_rows))
        lists_s, _ = timed(index._lists)
        print(json.dumps({**shape, "ncentroids": int(index.centroids.shape[0]), "train_s": round(train_s, 3),
                          "lists_s": round(lists_s, 4), "list_entries": int(index.list_docs.numel())}), flush=True)
        for L in (int(v) for v in args.query_rows.split(",")):
            src = torch.randint(0, nd, (args.nq,), generator=gen, device=dev).cpu().tolist()
            take = torch.cat([ptr[d] + torch.randint(0, ptr[d + 1] - ptr[d], (L,), generator=gen, device=dev) for d in src])
            qmv = noisy_unit(store[take].float(), args.noise / dim ** 0.5, gen).to(torch.bfloat16)
            qptr = list(range(0, args.nq * L + 1, L))
            want = index.search(qmv, qptr, args.k)[1]
            frac = {n: round(probed_fraction(index, qmv, qptr, n), 4) for n in nprobes[1:]}
            for ncand in (int(v) for v in args.ncands.split(",")):
                k = min(args.k, ncand)
                runs = {n: (lambda n=n: index.candidates(qmv, qptr, ncand, nprobe=n)) for n in nprobes}
                rec = {}
                for n, f in runs.items():                     # the untimed round, and the recall of each setting
                    timed(f)
                    got = index.search_two_phase(qmv, qptr, k, ncand, nprobe=n)[1]
                    rec[n] = [round(recall(got, want, min(10, k)), 4), round(recall(got, want, k), 4)]
                t = {n: [] for n in nprobes}
                for _ in range(args.repeats):
                    for n, f in runs.items():
                        t[n].append(timed(f)[0])
                s = {n: spread(v) for n, v in t.items()}
                for n in nprobes:
                    print(json.dumps({**shape, "query_rows": L, "ncand": ncand, "k": k, "nprobe": n, "candidates": s[n],
                                      "probed": frac.get(n, 1.0), "recall@10": rec[n][0], f"recall@{k}": rec[n][1],
                                      "full_over_probed": round(s[0]["median_s"] / s[n]["median_s"], 2),
                                      "ranges_disjoint": s[n]["max_s"] < s[0]["min_s"] or s[0]["max_s"] < s[n]["min_s"]}),
                          flush=True)
        del index, store


if __name__ == "__main__":
    main()

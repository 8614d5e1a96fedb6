#!/usr/bin/env python3
"""Fixed-dimensional encodings (``FdeEncoder``, ``MultiVectorIndex.set_fde``) as the candidate pass of the two-phase MaxSim
search: encode time, recall, and end-to-end time against the centroid pass.

    python tools/gpu_mv_fde_bench.py [--corpora 20000x1024,200000x128] [--doc-rows 128] [--nq 256] [--query-rows 16,64]
                                     [--configs 4x8x16,4x16x16,5x4x32] [--ncands 128,1024] [--ncentroids 4096]
                                     [--nprobes 0,1] [--k 10] [--repeats 5] [--components 2000] [--doc-components 0]
                                     [--noise 0.5] [--sample-rows 262144]

Corpora and queries are drawn as in tools/gpu_mv_probe_bench.py (``--doc-components`` N > 0: the topical corpus).  A
config is ``k_sim x reps x d_proj``.  Per corpus and config, ``encode``: ``encoder.encode_documents`` over the whole store in
``set_fde``'s slices, one untimed round and ``--repeats`` timed ones, next to ``torch``: the sums alone restated in torch
(bf16 matmul of a slice of rows with the planes and with proj, the codes from the signs, ``index_add_`` of the fp32 products
into [nd reps B, d_proj]; no mean, no fill), and ``store_bytes`` for the HBM bound.  Per (query length, ncand):
``search_two_phase(fde=True)`` and, with ``--ncentroids`` > 0, ``search_two_phase`` at every ``--nprobes`` value, interleaved;
recall@k is the mean share of the exact top k (``search``, run once) in each.  A time is a host clock around a call that ends
in a device synchronise; median with the smallest and the largest, in seconds.  One JSON line per configuration; nothing is
asserted."""
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


def torch_sums(enc, store, ptr, slice_rows=1 << 16):
    """The bucket sums of every document by torch: what a version without the kernel would run."""
    import torch
    dev, nb, nd = store.device, 1 << enc.k_sim, len(ptr) - 1
    doc_of = torch.repeat_interleave(torch.arange(nd, device=dev), torch.tensor(ptr, device=dev).diff())
    out = torch.zeros((nd * enc.reps * nb, enc.d_proj), dtype=torch.float32, device=dev)
    planes, proj = enc.planes.reshape(-1, enc.dim), enc.proj.reshape(-1, enc.dim)
    weights = (1 << torch.arange(enc.k_sim, device=dev)).long()
    rep = torch.arange(enc.reps, device=dev)
    for s in range(0, store.shape[0], slice_rows):
        x = store[s:s + slice_rows]
        code = (((x @ planes.T).reshape(-1, enc.reps, enc.k_sim) > 0).long() * weights).sum(dim=2)
        y = (x @ proj.T).float().reshape(-1, enc.d_proj)
        out.index_add_(0, ((doc_of[s:s + slice_rows, None] * enc.reps + rep) * nb + code).reshape(-1), y)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", type=str, default="20000x1024,200000x128")
    ap.add_argument("--doc-rows", type=int, default=128)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--query-rows", type=str, default="16,64")
    ap.add_argument("--configs", type=str, default="4x8x16,4x16x16,5x4x32")
    ap.add_argument("--ncands", type=str, default="128,1024")
    ap.add_argument("--ncentroids", type=int, default=4096, help="0: no centroid pass to compare with")
    ap.add_argument("--nprobes", type=str, default="0,1")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=2000)
    ap.add_argument("--doc-components", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--sample-rows", type=int, default=262144)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_mv_fde_bench: needs a GPU")
    from snx.retrieval import FdeEncoder, MultiVectorIndex
    dev = torch.device(args.device)
    nprobes = [int(v) for v in args.nprobes.split(",")] if args.ncentroids > 0 else []
    configs = [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]
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
        shape = {"bench": "mv_fde", "nd": nd, "doc_rows_total": ptr[-1], "dim": dim, "nq": args.nq,
                 "components": args.components, "doc_components": args.doc_components, "noise": args.noise}
        if nprobes:
            train_s, _ = timed(lambda: index.train_centroids(args.ncentroids, sample_rows=args.sample_rows))
            print(json.dumps({**shape, "ncentroids": int(index.centroids.shape[0]), "train_s": round(train_s, 3)}), flush=True)
        queries = {}
        for L in (int(v) for v in args.query_rows.split(",")):
            src = torch.randint(0, nd, (args.nq,), generator=gen, device=dev).cpu().tolist()
            take = torch.cat([ptr[d] + torch.randint(0, ptr[d + 1] - ptr[d], (L,), generator=gen, device=dev) for d in src])
            qmv = noisy_unit(store[take].float(), args.noise / dim ** 0.5, gen).to(torch.bfloat16)
            qptr = list(range(0, args.nq * L + 1, L))
            queries[L] = (qmv, qptr, index.search(qmv, qptr, args.k)[1])
        for k_sim, reps, d_proj in configs:
            enc = FdeEncoder(dim, k_sim, reps, d_proj, dev)
            cfg = {**shape, "k_sim": k_sim, "reps": reps, "d_proj": d_proj, "fde_dim": enc.fde_dim}
            timed(lambda: index.set_fde(enc))
            timed(lambda: torch_sums(enc, store, ptr))
            t = {"kernel": [], "torch": []}
            for _ in range(args.repeats):
                t["kernel"].append(timed(lambda: index.set_fde(enc))[0])
                t["torch"].append(timed(lambda: torch_sums(enc, store, ptr))[0])
            s = {n: spread(v) for n, v in t.items()}
            print(json.dumps({**cfg, "encode": s["kernel"], "torch": s["torch"], "store_bytes": ptr[-1] * dim * 2,
                              "store_gb_per_s": round(ptr[-1] * dim * 2 / s["kernel"]["median_s"] / 1e9, 1),
                              "torch_over_kernel": round(s["torch"]["median_s"] / s["kernel"]["median_s"], 2)}), flush=True)
            for L, (qmv, qptr, want) in queries.items():
                for ncand in (int(v) for v in args.ncands.split(",")):
                    runs = {"fde": lambda: index.search_two_phase(qmv, qptr, args.k, ncand, fde=True)}
                    for n in nprobes:
                        runs[f"nprobe{n}"] = lambda n=n: index.search_two_phase(qmv, qptr, args.k, ncand, nprobe=n)
                    rec = {name: round(recall(timed(f)[1][1], want, args.k), 4) for name, f in runs.items()}
                    t = {name: [] for name in runs}
                    for _ in range(args.repeats):
                        for name, f in runs.items():
                            t[name].append(timed(f)[0])
                    print(json.dumps({**cfg, "query_rows": L, "ncand": ncand, "k": args.k,
                                      **{name: {**spread(v), f"recall@{args.k}": rec[name]} for name, v in t.items()}}),
                          flush=True)
        del index, store


if __name__ == "__main__":
    main()

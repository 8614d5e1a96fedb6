#!/usr/bin/env python3
"""The graph index against the exact dense search and IVF-Flat on one GPU: build seconds, search seconds and recall.

    python tools/gpu_graph_bench.py [--nd 200000] [--dim 256] [--nq 2048] [--k 100] [--degree 32] [--knn 64] [--width 4]
                                    [--nentry 0] [--efs 100,200,400] [--nlist 1000] [--nprobe 8] [--repeats 5] [--components 2000]
                                    [--noise 1.0]

Corpus: the synthetic Gaussian mixture of tools/gpu_ivf_bench.py, made on the device from a seed -- ``--components``
standard-normal centres, every doc and every query a centre plus ``--noise`` times a standard-normal vector, L2-normalised.
Build: ``neighbors_s`` is the exact neighbour lists (``DenseIndex``'s band search of every doc against every doc, nd^2
scores) and ``optimize_s`` the rest of ``GraphIndex.build()`` (detours, forward and reverse lists, interleave), one run each;
the second is measured by building again from the lists of the first.  Then ``--repeats`` rounds, each timing
``DenseIndex.search``, ``IvfFlatIndex.search`` at ``--nprobe`` of ``--nlist`` lists and the graph search at every ``ef`` one
after the other (interleaved, so drift of the machine hits all alike), after one untimed round that warms every shape up; a
time is a host clock around a call that ends in a device synchronise, and a graph time includes its seed search.
Reported: the median with the smallest and the largest, the ratio of the medians to the exact search of the same rounds,
recall@10 / recall@k against the exact ids and the mean iteration count.  One JSON line per measurement; nothing is
asserted."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gpu_ivf_bench import mixture, recall, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nq", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--knn", type=int, default=64)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--nentry", type=int, default=0, help="entry docs (0: the index's default, 4 * ceil(sqrt(nd)))")
    ap.add_argument("--efs", type=str, default="100,200,400")
    ap.add_argument("--nlist", type=int, default=1000)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=2000)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_graph_bench: needs a GPU")
    from snx.retrieval import DenseIndex, GraphIndex, IvfFlatIndex
    dev = torch.device(args.device)
    gen = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn((args.components, args.dim), generator=gen, device=dev)
    E = mixture(args.nd, args.dim, centres, args.noise, gen)
    Q = mixture(args.nq, args.dim, centres, args.noise, gen)
    shape = {"nd": args.nd, "dim": args.dim, "nq": args.nq, "k": args.k, "components": args.components, "noise": args.noise}
    efs = sorted({max(int(x), args.k) for x in args.efs.split(",") if x})
    flat = DenseIndex(args.dim, dev)
    flat.add(E)
    flat.build()
    _, exact = timed(lambda: flat.search(Q, args.k))          # warm-up, and the ids recall is measured against
    exact_docs = exact[1]
    graph = GraphIndex(args.dim, dev, degree=args.degree, knn=args.knn, ef=efs[0], width=args.width,
                       nentry=args.nentry or None)
    graph.add(E)
    neighbors_s, lists = timed(graph.exact_neighbors)
    optimize_s, _ = timed(lambda: graph.build(neighbors=lists))
    filled = (graph.graph >= 0).sum(1).double()
    print(json.dumps({"bench": "graph_build", **shape, "degree": args.degree, "knn": args.knn,
                      "neighbors_s": round(neighbors_s, 3), "optimize_s": round(optimize_s, 3),
                      "mean_links": round(float(filled.mean()), 2), "min_links": int(filled.min())}), flush=True)
    ivf = IvfFlatIndex(args.dim, args.nlist, dev, nprobe=min(args.nprobe, args.nlist))
    ivf.add(E)
    ivf_build_s, _ = timed(ivf.build)
    print(json.dumps({"bench": "ivf_build", **shape, "nlist": ivf.nlist, "build_s": round(ivf_build_s, 3)}), flush=True)
    times = {"exact": [], "ivf": [], **{ef: [] for ef in efs}}
    found, iters = {}, {}
    for r in range(args.repeats + 1):                        # round 0 warms every shape up
        t, _ = timed(lambda: flat.search(Q, args.k))
        if r:
            times["exact"].append(t)
        t, out = timed(lambda: ivf.search(Q, args.k))
        if r:
            times["ivf"].append(t)
        found["ivf"] = out[1]
        for ef in efs:
            t, out = timed(lambda: graph.search(Q, args.k, ef=ef))
            if r:
                times[ef].append(t)
            found[ef], iters[ef] = out[1], float(graph.last_iterations.double().mean())
    base = spread(times["exact"])
    print(json.dumps({"bench": "dense_exact_search", **shape, **base}), flush=True)

    def line(name, key, **more):
        s = spread(times[key])
        print(json.dumps({"bench": name, **shape, **more, **s, "exact_over_this": round(base["median_s"] / s["median_s"], 2),
                          "recall_at_10": round(recall(found[key], exact_docs, min(10, args.k)), 4),
                          "recall_at_k": round(recall(found[key], exact_docs, args.k), 4)}), flush=True)
    line("ivf_search", "ivf", nlist=ivf.nlist, nprobe=ivf.nprobe)
    for ef in efs:
        line("graph_search", ef, degree=args.degree, knn=args.knn, width=args.width, ef=ef, nentry=graph.entry_count(ef),
             mean_iterations=round(iters[ef], 2))


if __name__ == "__main__":
    main()

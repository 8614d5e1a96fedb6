#!/usr/bin/env python3
"""The two-phase dense search against the exact dense search on one GPU: seconds and the certified fraction.

    python tools/gpu_dense2p_bench.py [--nd 1000000] [--dim 1024] [--nq 4096] [--k 100] [--expansions 2,4,8]
                                      [--repeats 5] [--components 2000] [--noise 1.0]

Corpus: the synthetic L2-normalised Gaussian mixture of tools/gpu_ivf_bench.py, made on the device from a seed.  The
certified fraction it gives is a property of that mixture, not of real teacher embeddings.
``prepare_s`` is ``bf16_rows`` over all docs (the bf16 copy and the three norms), timed ``--repeats`` times after one
untimed run.  Then ``--repeats`` rounds after one untimed round that warms every shape up; a round times, one after the
other (interleaved, so drift of the machine hits all alike), ``DenseIndex.search`` and, per expansion, ``candidates`` (the
queries' prepare and phase 1), ``snx_dense2_rescore`` on the candidates just kept (phase 2 alone, called as
``search_two_phase`` calls it), ``search_two_phase`` (both phases) and ``search_two_phase(exact=True)`` (that and the
exact search of the uncertified rows).  A time is a host clock around a call that ends in a device synchronise.  Reported:
the median with the smallest and the largest, in seconds to the microsecond; the ratio of the exact search's median to
``exact=True``'s, and whether the two ranges [min, max] are disjoint.  Every ``exact=True`` result is compared with the
exact search's, bit for bit.  One JSON line per measurement; nothing else is asserted."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gpu_ivf_bench import mixture, timed  # noqa: E402


def spread(times):
    return {"median_s": round(statistics.median(times), 6), "min_s": round(min(times), 6), "max_s": round(max(times), 6),
            "runs": len(times)}


def rescore(index, Q, stats, approx, docs, k):
    """Phase 2 alone over kept candidates, as DenseIndex.search_two_phase calls it -> certified uint8 [nq]."""
    import torch
    from snx._lib import call
    from snx.ops import _p, _stream
    nq, k1, dev = int(Q.shape[0]), int(docs.shape[1]), Q.device
    out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.int32, device=dev)
    found = torch.empty(nq, dtype=torch.int32, device=dev)
    cert = torch.empty(nq, dtype=torch.uint8, device=dev)
    _, dn, dh, dr = index._two_phase_state()
    with torch.cuda.device(dev):
        call("snx_dense2_rescore", _p(Q), nq, _p(index.emb), index.num_docs, index.dim, _p(docs), _p(approx), k1,
             _p(stats[1]), _p(stats[2]), _p(stats[3]), dn, dh, dr, None, None, None, 0, k, _p(out_d), _p(out_s),
             _p(found), _p(cert), _stream())
    return cert


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--expansions", type=str, default="2,4,8")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=2000)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_dense2p_bench: needs a GPU")
    from snx.retrieval import K_MAX, DenseIndex
    dev = torch.device(args.device)
    gen = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn((args.components, args.dim), generator=gen, device=dev)
    E = mixture(args.nd, args.dim, centres, args.noise, gen)
    Q = mixture(args.nq, args.dim, centres, args.noise, gen)
    shape = {"nd": args.nd, "dim": args.dim, "nq": args.nq, "k": args.k, "components": args.components,
             "noise": args.noise, "corpus": "synthetic mixture"}
    index = DenseIndex(args.dim, dev)
    index.add(E)
    index.build()
    from snx.retrieval import bf16_rows
    prepare = [timed(lambda: bf16_rows(E))[0] for _ in range(args.repeats + 1)][1:]
    print(json.dumps({"bench": "dense2p_prepare", **shape, **spread(prepare)}), flush=True)
    index._two_phase_state()
    qstats = bf16_rows(Q)
    expansions = [float(x) for x in args.expansions.split(",") if x]
    k1 = {x: max(args.k, min(args.nd, K_MAX, math.ceil(args.k * x))) for x in expansions}
    names = ("scan", "rescore", "two_phase", "exact")
    times = {"search": [], **{(x, n): [] for x in expansions for n in names}}
    certified, equal = {}, {}
    for r in range(args.repeats + 1):                        # round 0 warms every shape up
        t, want = timed(lambda: index.search(Q, args.k))
        if r:
            times["search"].append(t)
        for x in expansions:
            kept = {}
            runs = (("scan", lambda: kept.setdefault("c", index.candidates(Q, k1[x]))),
                    ("rescore", lambda: rescore(index, Q, qstats, *kept["c"], args.k)),
                    ("two_phase", lambda: index.search_two_phase(Q, args.k, expansion=x)),
                    ("exact", lambda: index.search_two_phase(Q, args.k, expansion=x, exact=True)))
            for name, fn in runs:
                t, out = timed(fn)
                if r:
                    times[(x, name)].append(t)
            certified[x] = float(out[2].double().mean()) if args.nq else 0.0
            equal[x] = bool(torch.equal(out[1], want[1])) and bool(torch.equal(out[0].view(torch.int32),
                                                                               want[0].view(torch.int32)))
    base = spread(times["search"])
    print(json.dumps({"bench": "dense_exact_search", **shape, **base}), flush=True)
    for x in expansions:
        s = {n: spread(times[(x, n)]) for n in names}
        e = s["exact"]
        print(json.dumps({"bench": "dense2p_search", **shape, "expansion": x, "k1": k1[x],
                          "scan": s["scan"], "rescore": s["rescore"], "two_phase": s["two_phase"], "exact_true": e,
                          "certified_fraction": round(certified[x], 4), "equals_exact_search": equal[x],
                          "search_over_exact_true": round(base["median_s"] / e["median_s"], 2),
                          "ranges_disjoint": e["max_s"] < base["min_s"] or base["max_s"] < e["min_s"]}), flush=True)


if __name__ == "__main__":
    main()

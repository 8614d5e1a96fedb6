#!/usr/bin/env python3
"""Write tests/golden/g13_fusion.json by RUNNING the reference's fusion rules and its paired t-test.

    python tools/make_golden_fusion.py --reference <checkout of the reference project>

Loads ref:benchmark/score_fusion.py (numpy only) and ref:benchmark/metrics.py (scipy) by file path with importlib.  The
triple RRF exists only inside ref:benchmark/hybrid_searcher.py HybridTripleSearcher.search (:494-536), whose module
imports the OpenSearch client: the module is loaded with placeholder modules for `opensearchpy`, `benchmark.config` and
`benchmark.encoders`, the searcher object is made without its constructor and its three sub-searchers are objects that
return the case's lists, so the arithmetic that runs is the reference's own ("triple_source" in the JSON says so).

For a fixed set of cases the JSON records the input lists (doc ids as ints, scores fp32-representable) and, per method
and parameter set, the reference's fused {doc: score} map with scores as float64 hex (no decimal round trip) and its
total_hits; for the t-test cases the two rank lists (0 or above 10: not retrieved) and the reference's statistic and
p_value (hex, "nan" for nan).  Tests read only the JSON."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g13_fusion.json")
RETRIEVAL_SIZE = 10

PAIR_METHODS = [("rrf", {"k": 60}), ("rrf", {"k": 10}), ("weighted_rrf", {"k": 60, "weights": [0.4, 0.6]}),
                ("weighted_rrf", {"k": 60, "weights": [0.6, 0.4]}), ("linear", {"alpha": 0.3}), ("linear", {"alpha": 0.4}),
                ("linear", {"alpha": 0.5}), ("linear", {"alpha": 0.0}), ("linear", {"alpha": 1.0})]
LONG_METHODS = [("rrf", {"k": 60}), ("linear", {"alpha": 0.4})]

T_CASES = {
    "mixed": ([1, 2, 0, 5, 11, 3, 1, 0, 7, 10, 2, 4], [2, 1, 3, 0, 4, 3, 6, 0, 1, 12, 9, 1]),
    "identical": ([1, 3, 0, 2, 5], [1, 3, 0, 2, 5]),
    "one_pair": ([1], [3]),
    "all_misses": ([0, 0, 11, 0], [0, 12, 0, 0]),
    "strong": ([1] * 30 + [2] * 10, [5, 7, 0, 9, 4, 10, 6, 0, 8, 3] * 4),
}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _load_reference(ref):
    F = _load("benchmark.score_fusion", os.path.join(ref, "benchmark", "score_fusion.py"))
    M = _load("ref_benchmark_metrics", os.path.join(ref, "benchmark", "metrics.py"))
    for name, attrs in (("opensearchpy", ("OpenSearch",)), ("benchmark.config", ("BenchmarkConfig",)),
                        ("benchmark.encoders", ("BgeM3Encoder", "NeuralSparseEncoder"))):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, type(a, (), {}))
        sys.modules[name] = mod
    pkg = types.ModuleType("benchmark")
    pkg.__path__ = []
    sys.modules["benchmark"] = pkg
    S = _load("benchmark.searchers", os.path.join(ref, "benchmark", "searchers.py"))
    H = _load("benchmark.hybrid_searcher", os.path.join(ref, "benchmark", "hybrid_searcher.py"))
    return F, M, S, H


def _scores(rng, n):
    """n fp32-representable scores, descending (as a search returns them), with ties."""
    return np.sort(rng.integers(1, 400, n).astype(np.float64) / 16.0)[::-1].tolist()


def _cases():
    rng = np.random.default_rng(13)
    pick = lambda n, hi: rng.choice(hi, n, replace=False).tolist()              # noqa: E731
    a = pick(12, 30)
    cases = [
        ("unequal_lengths", [(pick(15, 40), _scores(rng, 15)), (pick(6, 40), _scores(rng, 6))], PAIR_METHODS),
        ("one_empty", [(pick(8, 20), _scores(rng, 8)), ([], [])], PAIR_METHODS),
        ("other_empty", [([], []), (pick(5, 20), _scores(rng, 5))], PAIR_METHODS),
        ("both_empty", [([], []), ([], [])], PAIR_METHODS),
        ("disjoint", [(list(range(0, 20, 2)), _scores(rng, 10)), (list(range(1, 15, 2)), _scores(rng, 7))], PAIR_METHODS),
        ("identical", [(a, _scores(rng, 12)), (a, _scores(rng, 12))], PAIR_METHODS),
        ("same_docs_reversed", [(a, _scores(rng, 12)), (a[::-1], _scores(rng, 12))], PAIR_METHODS),
        ("all_scores_equal", [(pick(9, 25), [2.5] * 9), (pick(7, 25), _scores(rng, 7))], PAIR_METHODS),
        ("both_all_equal", [(pick(6, 12), [1.0] * 6), (pick(6, 12), [0.25] * 6)], PAIR_METHODS),
        ("single_entries", [([3], [1.5]), ([3], [0.5])], PAIR_METHODS),
        ("longer_than_99", [(pick(105, 160), _scores(rng, 105)), (pick(40, 160), _scores(rng, 40))], LONG_METHODS),
        ("triple", [(pick(14, 30), _scores(rng, 14)), (pick(9, 30), _scores(rng, 9)), (pick(11, 30), _scores(rng, 11))],
         [("rrf", {"k": 60}), ("rrf", {"k": 1})]),
        ("triple_one_empty", [(pick(10, 20), _scores(rng, 10)), ([], []), (pick(10, 20), _scores(rng, 10))],
         [("rrf", {"k": 60})]),
        ("triple_long", [(pick(101, 130), _scores(rng, 101)), (pick(20, 130), _scores(rng, 20)),
                         (pick(30, 130), _scores(rng, 30))], [("rrf", {"k": 60})]),
    ]
    return cases


def _ranked(F, docs, scores):
    return [F.RankedResult(doc_id=str(d), score=float(s), rank=i + 1) for i, (d, s) in enumerate(zip(docs, scores))]


def _fuse_pair(F, lists, method, params):
    if method == "weighted_rrf":
        fusion = F.create_fusion_method(method, k=params["k"], sparse_weight=params["weights"][0],
                                        dense_weight=params["weights"][1])
    else:
        fusion = F.create_fusion_method(method, **params)
    out = fusion.fuse(*[_ranked(F, d, s) for d, s in lists])
    return {r.doc_id: float(r.score).hex() for r in out}, len(out)


class _Fixed:
    """A sub-searcher that returns one fixed list."""

    def __init__(self, S, docs, scores):
        self.response = S.SearchResponse(
            results=[S.SearchResult(doc_id=str(d), score=float(s), rank=i + 1) for i, (d, s) in enumerate(zip(docs, scores))],
            latency_ms=0.0, total_hits=len(docs))

    def search(self, query):
        return self.response


def _fuse_triple(S, H, lists, params):
    t = object.__new__(H.HybridTripleSearcher)
    t.top_k, t.rrf_k = 1 << 20, params["k"]
    # the reference's operand order is bm25, dense, sparse: list 0, 1, 2
    t._bm25_searcher, t._semantic_searcher, t._sparse_searcher = (_Fixed(S, d, s) for d, s in lists)
    resp = t.search("q")
    assert len(resp.results) == resp.total_hits
    return {r.doc_id: float(r.score).hex() for r in resp.results}, resp.total_hits


def _hex(x):
    x = float(x)
    return "nan" if x != x else x.hex()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project checkout")
    args = ap.parse_args()
    F, M, S, H = _load_reference(args.reference)
    fusion = []
    for name, lists, methods in _cases():
        for _, s in lists:
            assert all(float(np.float32(x)) == x for x in s)
        runs = []
        for method, params in methods:
            fused, total = _fuse_triple(S, H, lists, params) if len(lists) == 3 else _fuse_pair(F, lists, method, params)
            runs.append({"method": method, "params": params, "scores": fused, "total_hits": total})
        fusion.append({"name": name, "lists": [{"docs": [int(x) for x in d], "scores": s} for d, s in lists], "runs": runs})
    ttests = []
    for name, (ra, rb) in T_CASES.items():
        res = [[M.QueryResult(query=f"q{i}", target_doc_id="t", retrieved_doc_ids=[], latency_ms=0.0,
                              hit_rank=r if 1 <= r <= RETRIEVAL_SIZE else None) for i, r in enumerate(ranks)]
               for ranks in (ra, rb)]
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = M.paired_t_test(*res)
        ttests.append({"name": name, "ranks_a": ra, "ranks_b": rb, "statistic": _hex(out["statistic"]),
                       "p_value": _hex(out["p_value"]), "significant": bool(out["significant"])})
    doc = {"source": "ref:benchmark/score_fusion.py (RRFFusion, LinearFusion, WeightedRRFFusion), "
                     "ref:benchmark/hybrid_searcher.py:494-536, ref:benchmark/metrics.py:149-177",
           "triple_source": "HybridTripleSearcher.search run on fixed sub-searcher outputs (placeholder modules for the "
                            "OpenSearch client, config and encoders; no RRFFusion composition)",
           "retrieval_size": RETRIEVAL_SIZE, "fusion": fusion, "ttest": ttests}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {OUT} ({len(fusion)} fusion cases, {len(ttests)} t-test cases, {os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Write tests/golden/g12_retrieval_metrics.json by RUNNING the reference's metric functions.

    python tools/make_golden_retrieval.py --reference <checkout of the reference project>

Loads ref:benchmark/metrics.py by file path with importlib (not through benchmark/__init__, which pulls in the
OpenSearch client) and runs its compute_recall_at_k, compute_mrr and compute_ndcg_at_k over a fixed set of rank lists.
Each rank is the target's full 1-based rank in the scored corpus (0: score 0, nothing retrieved for it); a query's
QueryResult gets the top-10 retrieval (ref:benchmark/config.py:44) that rank implies, so its hit_rank comes from the
reference's own __post_init__.  Misses, ranks 1, 10 and 11, empty retrievals and an empty query set are covered.
Tests read only the JSON (src.train.eval.metrics_from_ranks must reproduce it exactly)."""
import argparse
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g12_retrieval_metrics.json")
RETRIEVAL_SIZE = 10

CASES = {
    "all_first": [1, 1, 1, 1],
    "mixed": [1, 2, 5, 6, 10, 11, 0, 3],
    "boundaries": [10, 11, 1, 0],
    "all_missed": [0, 0, 11, 250],
    "empty_retrievals": [0, 0, 0],
    "single_rank_10": [10],
    "single_rank_11": [11],
    "ladder": list(range(1, 21)) + [0] * 5,
    "no_queries": [],
}


def _load_metrics(ref: str):
    path = os.path.join(ref, "benchmark", "metrics.py")
    spec = importlib.util.spec_from_file_location("ref_benchmark_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _results(M, ranks):
    out = []
    for i, r in enumerate(ranks):
        target = f"d{i}"
        if r == 0:
            retrieved = []                                             # every score 0: nothing comes back
        elif r <= RETRIEVAL_SIZE:
            retrieved = [f"x{i}_{j}" for j in range(1, RETRIEVAL_SIZE + 1)]
            retrieved[r - 1] = target
        else:
            retrieved = [f"x{i}_{j}" for j in range(1, RETRIEVAL_SIZE + 1)]
        out.append(M.QueryResult(query=f"q{i}", target_doc_id=target, retrieved_doc_ids=retrieved, latency_ms=0.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project checkout")
    args = ap.parse_args()
    M = _load_metrics(args.reference)
    cases = []
    for name, ranks in CASES.items():
        res = _results(M, ranks)
        cases.append({"name": name, "ranks": ranks,
                      "hit_ranks": [r.hit_rank for r in res],
                      "metrics": {"recall@1": float(M.compute_recall_at_k(res, 1)),
                                  "recall@5": float(M.compute_recall_at_k(res, 5)),
                                  "recall@10": float(M.compute_recall_at_k(res, 10)),
                                  "mrr@10": float(M.compute_mrr(res)),
                                  "ndcg@10": float(M.compute_ndcg_at_k(res, 10))}})
    doc = {"source": "ref:benchmark/metrics.py:52-99 (compute_recall_at_k, compute_mrr, compute_ndcg_at_k)",
           "retrieval_size": RETRIEVAL_SIZE, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT} ({len(cases)} cases)")


if __name__ == "__main__":
    main()

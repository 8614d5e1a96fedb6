#!/usr/bin/env python3
"""Write tests/golden/g14_qrels.json and tests/golden/g14_benchmark_dir/ by RUNNING the reference's metrics.

    python tools/make_golden_qrels.py --reference <checkout of the reference project>

Loads ref:benchmark/metrics.py (numpy + scipy) by file path with importlib.  The any-relevant hit rule lives in
ref:benchmark/hf_runner.py:198-203, whose module needs an OpenSearch client: the four-line loop is restated here
(`_hit_rank`), everything that computes a recorded number is the reference's own code -- compute_metrics,
bootstrap_confidence_interval (n_bootstrap = 1000, its own seed 42) over compute_recall_at_k(k=1), compute_mrr and
compute_ndcg_at_k(k=10), and paired_t_test.

The JSON records, for two synthetic "methods" over the same queries: the ranked lists (doc ids as ints, -1 padded), the
qrels rows (several relevant docs per query, some rows empty, some ids outside the corpus), the hit ranks (0 = none), the
metrics, the three intervals and the t-test between the methods; floats as float64 hex (no decimal round trip).  It also
asserts what snx.retrieval.bootstrap_indices relies on: numpy.random.seed(42) followed by one numpy.random.choice(n,
size=n, replace=True) per resample is the stream of numpy.random.RandomState(42).randint(0, n, size=n) per resample, for
all 1000 draws.  The benchmark directory is three small JSONL files of synthetic text in the layout of
ref:benchmark/hf_data_loader.py:401-459, with a qrel of score 0, a relevant id absent from the corpus, a query with two
relevant docs and a query whose only qrel has score 0.  Tests read only these files."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g14_qrels.json")
OUT_DIR = os.path.join(ROOT, "tests", "golden", "g14_benchmark_dir")
NQ, ND, R, N_BOOTSTRAP = 150, 80, 10, 1000


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _hit_rank(retrieved, relevant):
    """ref:benchmark/hf_runner.py:198-203."""
    relevant = set(relevant)
    for rank, doc_id in enumerate(retrieved, 1):
        if doc_id in relevant:
            return rank
    return None


def _hex(x):
    x = float(x)
    return "nan" if x != x else x.hex()


def _fixture():
    rng = np.random.default_rng(14)
    rows, lists = [], {"a": [], "b": []}
    for q in range(NQ):
        nrel = 0 if q % 23 == 7 else int(rng.integers(1, 6))
        row = sorted(rng.choice(ND + 6, nrel, replace=False).tolist())          # ids >= ND: judged, not in the corpus
        rows.append([int(d) for d in row])
        for name, bias in (("a", 0.45), ("b", 0.25)):
            m = 0 if q % 31 == 5 else int(rng.integers(3, R + 1))
            lst = rng.choice(ND, m, replace=False).tolist()
            inside = [d for d in row if d < ND]
            if inside and m and rng.random() < bias:                              # plant a relevant doc near the top
                d = inside[int(rng.integers(len(inside)))]
                lst = [x for x in lst if x != d]
                lst.insert(int(rng.integers(0, min(3, len(lst) + 1))), d)
                lst = lst[:m]
            lists[name].append([int(d) for d in lst] + [-1] * (R - len(lst)))
    return rows, lists


def _benchmark_dir():
    os.makedirs(OUT_DIR, exist_ok=True)
    topics = ["red kettle", "blue bicycle", "green lantern", "wooden table", "steel bridge", "paper crane", "glass marble",
              "copper wire", "woollen scarf", "silver spoon", "stone garden", "leather boots"]
    corpus = [{"_id": f"d{i}", "title": f"{t} {i}", "text": f"{t} with {topics[(i + 3) % len(topics)]} number {i}"}
              for i, t in enumerate(topics)]
    queries = [{"_id": f"q{i}", "text": f"{topics[i]} number {i}"} for i in range(8)]
    qrels = [("q2", "d2", 1), ("q0", "d0", 1), ("q0", "d9", 2), ("q1", "d1", 0), ("q1", "d4", 1), ("q3", "d99", 1),
             ("q3", "d3", 1), ("q5", "d404", 1), ("q4", "d4", 0), ("q6", "d6", 1), ("q2", "d2", 1), ("q7", "d7", 1)]
    for name, items in (("corpus.jsonl", corpus), ("queries.jsonl", queries),
                        ("qrels.jsonl", [{"query-id": q, "corpus-id": d, "score": s} for q, d, s in qrels])):
        with open(os.path.join(OUT_DIR, name), "w", encoding="utf-8") as f:
            for x in items:
                f.write(json.dumps(x) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project checkout")
    args = ap.parse_args()
    M = _load("ref_benchmark_metrics", os.path.join(args.reference, "benchmark", "metrics.py"))
    rs = np.random.RandomState(42)
    np.random.seed(42)
    for _ in range(N_BOOTSTRAP):
        assert np.array_equal(np.random.choice(NQ, size=NQ, replace=True), rs.randint(0, NQ, size=NQ))
    rows, lists = _fixture()
    methods, results = {}, {}
    for name, ls in lists.items():
        res = []
        for q, lst in enumerate(ls):
            retrieved = [str(d) for d in lst if d >= 0]
            res.append(M.QueryResult(query=f"q{q}", target_doc_id=str(rows[q][0]) if rows[q] else "",
                                     retrieved_doc_ids=retrieved, latency_ms=0.0,
                                     hit_rank=_hit_rank(retrieved, [str(d) for d in rows[q]])))
        results[name] = res
        m = M.compute_metrics(name, res)
        ci = {"recall@1": M.bootstrap_confidence_interval(res, lambda s: M.compute_recall_at_k(s, k=1), N_BOOTSTRAP),
              "mrr": M.bootstrap_confidence_interval(res, M.compute_mrr, N_BOOTSTRAP),
              "ndcg@10": M.bootstrap_confidence_interval(res, lambda s: M.compute_ndcg_at_k(s, k=10), N_BOOTSTRAP)}
        methods[name] = {
            "lists": ls, "hit_ranks": [r.hit_rank or 0 for r in res],
            "metrics": {k: _hex(getattr(m, k)) for k in ("recall_at_1", "recall_at_5", "recall_at_10", "mrr", "ndcg_at_10")},
            "num_queries": m.num_queries,
            "ci": {k: {x: _hex(v[x]) for x in ("point_estimate", "lower", "upper")} for k, v in ci.items()}}
    t = M.paired_t_test(results["a"], results["b"])
    doc = {"source": "ref:benchmark/metrics.py (compute_metrics, bootstrap_confidence_interval, paired_t_test); hit ranks "
                     "by the any-relevant loop of ref:benchmark/hf_runner.py:198-203, restated in the tool",
           "num_docs": ND, "list_len": R, "n_bootstrap": N_BOOTSTRAP, "confidence": 0.95, "seed": 42, "relevant": rows,
           "methods": methods,
           "ttest": {"a": "a", "b": "b", "statistic": _hex(t["statistic"]), "p_value": _hex(t["p_value"]),
                     "significant": bool(t["significant"])}}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    _benchmark_dir()
    print(f"wrote {OUT} ({NQ} queries, 2 methods, {os.path.getsize(OUT)} bytes) and {OUT_DIR}")


if __name__ == "__main__":
    main()

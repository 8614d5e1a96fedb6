#!/usr/bin/env python3
"""Write tests/golden/g20_expansion/ by RUNNING the reference's src/evaluation/ranking_metrics.py (it needs torch, numpy,
scipy and an importable ``transformers``; no GPU).

    python tools/make_golden_expansion.py --reference <checkout of the reference project>

The inputs come from tests/expansion_reference.py (``build_rows``, ``build_queries``, the stub tokenizer and model), so the
fixture holds the cases and what the reference answered.  Data only:

  g20.json             the queries (dict order kept); ``single``: evaluate_single_query of every row with k_values
                       5 .. 150 and max_k = 100; ``single_aggregate``: _aggregate_metrics of those; ``evaluate_a`` /
                       ``evaluate_b``: evaluate() through the stubs (default k_values, two batches of 25 and 15) on the two
                       row sets; ``comparison``: compare_models of the two; ``pairs``: a from_synonym_pairs / save round
                       trip (the input, the saved text, statistics()); ``sample_statistics``.  Floats as float.hex.
  arrays.npz           rows_a, rows_b fp32 [40, 512]
  sample_dataset.json  create_korean_legal_medical_eval_dataset().save(): the judgment lists of the reference's sample,
                       which src/evaluation loads (they are data; none of them is written out in this repository's code)

Cases (tests/expansion_reference.build_queries): a query without judgments, one with only unresolved tokens, a judged
special id, two tokens sharing one id with grades 3 and 0 in both orders, a judged id of weight 0, a row with fewer
positives than max_k and one with none, the first relevant entry at positions 93 and 99, a judged id outside the
vocabulary, k_values above max_k, three domains and a query without one.

The tool refuses to write when a judged token with a positive weight shares that weight with another allowed entry of its
row: the only place where torch.topk's order among equal weights could reach a metric."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import expansion_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g20_expansion")
PAIRS = [
    {"source": "w100", "synonyms": {"exact": ["w101", "w102"], "partial": ["w103"], "related": ["w104", "w105"]},
     "domain": "legal"},
    {"source": "w200", "synonyms": {"exact": ["w201"], "related": ["w201", "w202"]}},
    {"source": "w300", "synonyms": {}, "domain": "general"},
    {"source": "w400"},
]


def load_reference(root: str):
    path = os.path.join(root, "src", "evaluation", "ranking_metrics.py")
    spec = importlib.util.spec_from_file_location("ref_ranking_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def enc(x):
    """JSON form: floats (numpy's too) as float.hex, ints and strings as they are."""
    if isinstance(x, dict):
        return {str(k): enc(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [enc(v) for v in x]
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    return x


def check_no_ties(rows, queries, resolve):
    ex = R.excluded_mask(R.SPECIAL_IDS, R.V)
    for i, q in enumerate(queries):
        for tok in q["relevance_judgments"]:
            t = resolve(tok)
            if t is None or not 0 <= t < R.V or not rows[i, t] > 0:
                continue
            same = [v for v in range(R.V) if v != t and not ex[v] and rows[i, v] == rows[i, t]]
            if same:
                raise SystemExit(f"query {i}: judged id {t} shares its weight with {same}: torch.topk's tie order would "
                                 "reach the metrics; nothing written")


def result_record(res):
    d = res.to_dict()
    return {"per_query_metrics": enc(d.pop("per_query_metrics")), "aggregate": enc(d), "summary": res.summary()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    import torch
    ref = load_reference(args.reference)
    tok = R.StubTokenizer()
    resolve = R.resolver(tok)
    rows_a, rows_b = R.build_rows(0), R.build_rows(1)
    queries = R.build_queries(rows_a)
    check_no_ties(rows_a, queries, resolve)
    check_no_ties(rows_b, queries, resolve)
    dataset = ref.EvaluationDataset(queries=[ref.GradedRelevance.from_dict(q) for q in queries], name="g20")
    wide = ref.RankingMetrics(tok, k_values=list(R.K_WIDE))
    assert sorted(wide.special_token_ids) == sorted(R.SPECIAL_IDS)
    single = [wide.evaluate_single_query(torch.from_numpy(rows_a[i]), dataset[i], max_k=R.MAX_K) for i in range(R.NQ)]
    mine = [R.single_query(rows_a[i], R.SPECIAL_IDS, resolve, queries[i], R.K_WIDE, R.MAX_K) for i in range(R.NQ)]
    print("restatement equals the reference per query:", mine == single)
    firsts = [s["first_relevant_rank"] for s in single]
    assert firsts[8] == 92 and firsts[9] == 98, firsts[:12]                    # positions 93 and 99 through int(1 / mrr)
    single_agg = wide._aggregate_metrics(single)
    plain = ref.RankingMetrics(tok)
    res_a = plain.evaluate(R.stub_model(rows_a), dataset, batch_size=R.BATCH_SIZE)
    res_b = plain.evaluate(R.stub_model(rows_b), dataset, batch_size=R.BATCH_SIZE)
    cmp_ = ref.ModelComparison.compare_models(res_a, res_b, "ckpt_a", "ckpt_b")
    assert all("error" not in v for v in cmp_.metrics_compared.values()), cmp_.metrics_compared
    pairs_ds = ref.EvaluationDataset.from_synonym_pairs(PAIRS, name="pairs")
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "pairs.json")
        pairs_ds.save(path)
        saved = open(path, encoding="utf-8").read()
        again = ref.EvaluationDataset.load(path)
        assert [q.to_dict() for q in again] == [q.to_dict() for q in pairs_ds]
    sample = ref.create_korean_legal_medical_eval_dataset()
    stats = sample.statistics()
    stats["domains"] = sorted(stats["domains"])
    pstats = pairs_ds.statistics()
    pstats["domains"] = sorted(pstats["domains"])
    os.makedirs(OUT, exist_ok=True)
    sample.save(os.path.join(OUT, "sample_dataset.json"))
    record = {"source": "ref:src/evaluation/ranking_metrics.py RankingMetrics, ModelComparison, EvaluationDataset",
              "numpy": np.__version__, "V": R.V, "max_k": R.MAX_K, "k_wide": R.K_WIDE, "k_default": R.K_DEFAULT,
              "batch_size": R.BATCH_SIZE, "special_ids": R.SPECIAL_IDS, "queries": queries,
              "single": enc(single), "single_aggregate": result_record(single_agg),
              "evaluate_a": result_record(res_a), "evaluate_b": result_record(res_b),
              "comparison": {"model_a_name": cmp_.model_a_name, "model_b_name": cmp_.model_b_name,
                             "metrics_compared": enc(cmp_.metrics_compared), "summary": cmp_.summary()},
              "pairs": {"input": PAIRS, "saved": saved, "statistics": enc(pstats),
                        "legal": [q.to_dict() for q in pairs_ds.filter_by_domain("legal")],
                        "legal_name": pairs_ds.filter_by_domain("legal").name},
              "sample_statistics": enc(stats), "sample_name": sample.name,
              "restatement_equal": mine == single}
    with open(os.path.join(OUT, "g20.json"), "w", encoding="utf-8") as f:
        json.dump(record, f, ensure_ascii=False, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(OUT, "arrays.npz"), rows_a=rows_a, rows_b=rows_b)
    print(f"wrote {OUT}: {R.NQ} queries")


if __name__ == "__main__":
    main()

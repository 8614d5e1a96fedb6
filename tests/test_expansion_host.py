"""Host checks of the term-expansion evaluation: the NumPy / Python restatement (tests/expansion_reference.py) against what
the reference project answered (tests/golden/g20_expansion, written by tools/make_golden_expansion.py), and the host
side of the mirror (src.evaluation) and of the binding (snx.expansion).  Every per-query number is compared with ==; the
aggregates are numpy means of identical inputs and are equal to the last bit as well.  The paired t-test is held to the
bounds tests/test_qrels_host.py applies to the same statistic against g14
(test_paired_t_test_over_first_relevant_ranks_equals_the_reference: 1e-10 relative on t, 1e-8 relative on p)."""
import json
import math
import os
import re

import numpy as np
import pytest

from tests import expansion_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g20_expansion")
HEADER = os.path.join(os.path.dirname(HERE), "include", "snx.h")
T_REL, P_REL = 1e-10, 1e-8                         # tests/test_qrels_host.py, the g14 t-test assertion


def golden():
    with open(os.path.join(GOLDEN, "g20.json"), encoding="utf-8") as f:
        return json.load(f)


def golden_rows():
    z = np.load(os.path.join(GOLDEN, "arrays.npz"))
    return z["rows_a"], z["rows_b"]


def dec(x):
    """The inverse of the golden tool's encoding: hex strings back to floats (names and domains are not hex)."""
    if isinstance(x, dict):
        return {k: (v if k in ("query", "domain", "domains", "error") else dec(v)) for k, v in x.items()}
    if isinstance(x, list):
        return [dec(v) for v in x]
    if isinstance(x, str):
        return float.fromhex(x)
    return x


def same(a, b):
    """== with the types that matter: a float is compared by value (inf included), an int stays an int."""
    assert type(a) is type(b) or {type(a), type(b)} <= {float, np.float64}, (a, b)
    return a == b


# ------------------------------------------------------------------------------------------------ the restatement
def test_case_builder_regenerates_the_golden_inputs():
    g = golden()
    rows_a, rows_b = golden_rows()
    assert np.array_equal(R.build_rows(0), rows_a) and np.array_equal(R.build_rows(1), rows_b)
    assert rows_a.dtype == np.float32 and rows_a.shape == (R.NQ, R.V) == (40, 512)
    q = R.build_queries(rows_a)
    assert q == g["queries"]
    assert [list(a["relevance_judgments"]) for a in q] == [list(b["relevance_judgments"]) for b in g["queries"]]   # order
    assert g["special_ids"] == R.SPECIAL_IDS and g["max_k"] == R.MAX_K and g["k_wide"] == R.K_WIDE
    assert g["restatement_equal"] is True


def test_cases_the_golden_must_hold():
    g = golden()
    rows_a, _ = golden_rows()
    q = g["queries"]
    resolve = R.resolver(R.StubTokenizer())
    single = dec(g["single"])
    assert q[0]["relevance_judgments"] == {}
    assert all(resolve(t) is None for t in q[1]["relevance_judgments"]) and len(q[1]["relevance_judgments"]) == 3
    assert resolve("w5") == 5 and "w5" in q[2]["relevance_judgments"] and rows_a[2, 5] > 0 and 5 in R.SPECIAL_IDS
    for i, grades in ((3, [3, 0]), (4, [0, 3])):                               # one id, two tokens, both orders
        toks = [t for t in q[i]["relevance_judgments"] if resolve(t) == resolve(list(q[i]["relevance_judgments"])[0])]
        assert len(toks) == 2 and [q[i]["relevance_judgments"][t] for t in toks] == grades
    assert single[3]["ndcg@5"] != single[4]["ndcg@5"] and single[3]["recall@5"] == single[4]["recall@5"]
    assert any(rows_a[5, resolve(t)] == 0 for t in q[5]["relevance_judgments"])
    assert 0 < single[6]["num_ranked_tokens"] < R.MAX_K and single[7]["num_ranked_tokens"] == 0
    assert single[8]["mrr"] == 1.0 / 93 and single[8]["first_relevant_rank"] == 92          # int(1 / (1 / 93))
    assert single[9]["mrr"] == 1.0 / 99 and single[9]["first_relevant_rank"] == 98
    assert any(resolve(t) is not None and resolve(t) >= R.V for t in q[10]["relevance_judgments"])
    assert max(R.K_WIDE) > R.MAX_K
    assert {x["domain"] for x in q} == set(R.DOMAINS) | {None} and q[R.NO_DOMAIN_QUERY]["domain"] is None
    assert [k for k in range(1, 200) if int(1 / (1.0 / k)) != k] == [93, 99, 105, 117, 123, 186, 198]


def test_restatement_equals_the_reference_per_query():
    g = golden()
    rows_a, rows_b = golden_rows()
    resolve = R.resolver(R.StubTokenizer())
    want = dec(g["single"])
    for i, q in enumerate(g["queries"]):
        got = R.single_query(rows_a[i], R.SPECIAL_IDS, resolve, q, R.K_WIDE, R.MAX_K)
        assert list(got) == list(want[i])
        for key in got:
            assert same(got[key], want[i][key]), (i, key, got[key], want[i][key])
    for rows, name in ((rows_a, "evaluate_a"), (rows_b, "evaluate_b")):
        want = dec(g[name]["per_query_metrics"])
        for i, q in enumerate(g["queries"]):
            got = R.single_query(rows[i], R.SPECIAL_IDS, resolve, q, R.K_DEFAULT, max(R.K_DEFAULT))
            assert got == want[i] and list(got) == list(want[i]), (name, i)


def test_abi_restatement_on_a_hand_worked_row():
    #        id:   0    1    2    3     4    5    6         7
    rep = np.array([[2.0, 3.0, 3.0, 0.0, -1.0, 3.0, 1.0, np.nan]], np.float32)
    ex = np.array([0, 0, 0, 0, 0, 1, 0, 0], np.uint8)                          # id 5 is excluded
    assert R.ranking(rep[0], ex, 10) == [1, 2, 0, 6] and R.ranking(rep[0], ex, 2) == [1, 2]
    ptr = np.array([0, 6])
    tok = np.array([2, 0, 5, 3, 6, 99])
    grade, rel = [3, 1, 3, 2, 0, 3], [1, 0, 1, 1, 1, 1]
    rank, nranked, first, hits, dcg = R.metrics(rep, ex, ptr, tok, grade, rel, 3, [1, 2, 5])
    assert rank.tolist() == [2, 3, 0, 0, 0, 0] and nranked.tolist() == [3] and first.tolist() == [2]
    assert hits.tolist() == [[0, 1, 1]]
    assert dcg[0].tolist() == [0.0, 0.0 + 7 / math.log2(3), (0.0 + 7 / math.log2(3)) + 1 / math.log2(4)]


# ------------------------------------------------------------------------------------------------ the mirror, host side
def _mirror_metrics(k_values=None):
    from src.evaluation import RankingMetrics
    return RankingMetrics(R.StubTokenizer(), k_values=k_values)


def test_mirror_interface_and_token_rules():
    import dataclasses
    import inspect
    from src import evaluation as E
    from src.evaluation import ranking_metrics as M
    assert sorted(E.__all__) == sorted(["RankingMetrics", "GradedRelevance", "EvaluationDataset", "EvaluationResult",
                                        "ModelComparison", "create_korean_legal_medical_eval_dataset"])
    assert [f.name for f in dataclasses.fields(E.EvaluationResult)] == [
        "per_query_metrics", "recall_at_k", "mrr", "ndcg_at_k", "mean_first_relevant_rank", "median_first_relevant_rank",
        "num_queries", "domain_metrics"]
    assert [(f.name, f.default) for f in dataclasses.fields(E.EvaluationDataset)][1:] == [
        ("name", "evaluation_dataset"), ("version", "1.0")]
    sig = inspect.signature(E.RankingMetrics.evaluate)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [
        ("model", inspect.Parameter.empty), ("eval_dataset", inspect.Parameter.empty), ("batch_size", 32), ("device", None)]
    sig = inspect.signature(E.ModelComparison.bootstrap_confidence_interval)
    assert {p.name: p.default for p in sig.parameters.values()} == {
        "scores_a": inspect.Parameter.empty, "scores_b": inspect.Parameter.empty, "n_bootstrap": 10000, "confidence": 0.95,
        "seed": 42}
    m = _mirror_metrics()
    assert m.k_values == [5, 10, 20, 50, 100] == E.RankingMetrics.DEFAULT_K_VALUES
    assert sorted(m.special_token_ids) == sorted(R.SPECIAL_IDS)
    assert sorted(E.RankingMetrics(R.StubTokenizer(), special_tokens={"w9+w11"}).special_token_ids) == sorted(
        R.SPECIAL_IDS + [9, 11])
    assert m._get_token_id("w7") == 7 and m._get_token_id("w7+w8") is None and m._get_token_id("") is None
    gt = E.GradedRelevance("q", {"w40": 3, "a40": 0, "w41+w42": 3, "w600": 1})
    assert m._relevant_ids(gt) == {40, 600} and m._grade_of(gt) == {40: 0, 600: 1}
    with pytest.raises(ValueError, match="Invalid relevance grade 4"):
        E.GradedRelevance("q", {"x": 4})
    assert gt.ideal_ranking(2) == [("w40", 3), ("w41+w42", 3)] and gt.get_tokens_by_grade(3) == {"w40", "w41+w42"}
    assert M.SAMPLE_DATASET.exists()


def test_mirror_list_metrics_equal_the_golden_on_the_restatements_ranking():
    """compute_* over a ranking list are plain Python: fed the restatement's ranking they give the golden numbers."""
    from src.evaluation import GradedRelevance
    g = golden()
    rows_a, _ = golden_rows()
    m = _mirror_metrics(list(R.K_WIDE))
    ex = R.excluded_mask(R.SPECIAL_IDS, R.V)
    want = dec(g["single"])
    for i, q in enumerate(g["queries"]):
        gt = GradedRelevance.from_dict(q)
        ranking = [(v, float(rows_a[i, v])) for v in R.ranking(rows_a[i], ex, R.MAX_K)]
        for k in R.K_WIDE:
            assert m.compute_recall_at_k(ranking, gt, k) == want[i][f"recall@{k}"]
            assert m.compute_ndcg(ranking, gt, k) == want[i][f"ndcg@{k}"]
        assert m.compute_mrr(ranking, gt) == want[i]["mrr"]


def test_mirror_aggregation_and_summary_equal_the_golden():
    g = golden()
    for name, ks in (("single_aggregate", R.K_WIDE), ("evaluate_a", R.K_DEFAULT), ("evaluate_b", R.K_DEFAULT)):
        per_query = dec(g["single"] if name == "single_aggregate" else g[name]["per_query_metrics"])
        res = _mirror_metrics(list(ks))._aggregate_metrics(per_query)
        want = dec(g[name]["aggregate"])
        got = res.to_dict()
        assert got.pop("per_query_metrics") is per_query
        got = json.loads(json.dumps(got, default=float))                       # int keys -> str, numpy floats -> float
        assert set(got["domain_metrics"]) == set(want["domain_metrics"]) == set(R.DOMAINS)
        assert got == want, name                                               # means of identical inputs: every bit
        assert res.summary().split("Per-Domain")[0] == g[name]["summary"].split("Per-Domain")[0]
        assert sorted(res.summary().splitlines()) == sorted(g[name]["summary"].splitlines())   # domains: set order
    from src.evaluation import EvaluationResult
    assert _mirror_metrics()._aggregate_metrics([]).to_dict() == EvaluationResult().to_dict()


def test_dataset_json_layout_and_statistics():
    from src.evaluation import EvaluationDataset, create_korean_legal_medical_eval_dataset
    g = golden()["pairs"]
    ds = EvaluationDataset.from_synonym_pairs(g["input"], name="pairs")
    assert ds.name == "pairs" and ds.version == "1.0" and len(ds) == 4 and ds[1].relevance_judgments == {"w201": 1, "w202": 1}
    stats = ds.statistics()
    stats["domains"] = sorted(stats["domains"])
    assert json.loads(json.dumps(stats)) == dec(g["statistics"])
    assert [q.to_dict() for q in ds.filter_by_domain("legal")] == g["legal"]
    assert ds.filter_by_domain("legal").name == g["legal_name"]
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "pairs.json")
        ds.save(path)
        assert open(path, encoding="utf-8").read() == g["saved"]              # the reference's file, byte for byte
        back = EvaluationDataset.load(path)
    assert [q.to_dict() for q in back] == [q.to_dict() for q in ds] and back.name == "pairs"
    sample = create_korean_legal_medical_eval_dataset()
    stats = sample.statistics()
    stats["domains"] = sorted(stats["domains"])
    assert json.loads(json.dumps(stats)) == dec(golden()["sample_statistics"])
    assert sample.name == golden()["sample_name"] and len(sample) == 15
    assert EvaluationDataset(queries=[]).statistics()["avg_judgments_per_query"] == 0


# ------------------------------------------------------------------------------------------------ comparison, host side
def test_bootstrap_stream_equals_the_references_for_the_goldens_n():
    from snx.retrieval import bootstrap_indices
    n, nb = R.NQ, 10000                                  # every draw of the default n_bootstrap
    ours = bootstrap_indices(n, nb, 42)
    np.random.seed(42)
    theirs = np.stack([np.random.choice(n, size=n, replace=True) for _ in range(nb)])
    assert np.array_equal(ours, theirs)


def test_paired_t_test_equals_the_golden_with_and_without_scipy(monkeypatch):
    from src.evaluation import ModelComparison
    from src.evaluation.ranking_metrics import _paired_t
    g = golden()
    a, b = dec(g["evaluate_a"]["per_query_metrics"]), dec(g["evaluate_b"]["per_query_metrics"])
    want = dec(g["comparison"]["metrics_compared"])
    assert list(want) == ["mrr", "ndcg@5", "ndcg@10", "ndcg@20"]
    for metric, w in want.items():
        sa, sb = [q[metric] for q in a], [q[metric] for q in b]
        t = ModelComparison.paired_t_test(sa, sb)
        assert list(t) == ["t_statistic", "p_value", "significant", "mean_diff", "std_diff"]
        wt = w["paired_t_test"]
        assert abs(t["t_statistic"] - wt["t_statistic"]) <= T_REL * abs(wt["t_statistic"])
        assert abs(t["p_value"] - wt["p_value"]) <= P_REL * abs(wt["p_value"])
        assert bool(t["significant"]) is wt["significant"]
        assert t["mean_diff"] == wt["mean_diff"] and t["std_diff"] == wt["std_diff"]        # np.mean / np.std (ddof 0)
        ft, fp = _paired_t(np.asarray(sa) - np.asarray(sb))                    # the path taken where scipy is absent
        assert abs(ft - wt["t_statistic"]) <= T_REL * abs(wt["t_statistic"])
        assert abs(fp - wt["p_value"]) <= P_REL * abs(wt["p_value"])
        assert w["model_a_mean"] == float(np.mean(sa)) and w["model_b_mean"] == float(np.mean(sb))
    few = ModelComparison.paired_t_test([0.5], [0.25])
    assert few == {"t_statistic": None, "p_value": None, "significant": False, "error": "Insufficient samples for t-test"}
    with pytest.raises(ValueError, match="same length"):
        ModelComparison.paired_t_test([1.0], [1.0, 2.0])


def test_comparison_summary_layout():
    from src.evaluation import ModelComparison
    g = golden()["comparison"]
    c = ModelComparison(g["model_a_name"], g["model_b_name"], dec(g["metrics_compared"]))
    assert c.summary() == g["summary"]
    c.metrics_compared["x"] = {"error": "boom"}
    assert "\nx: ERROR - boom" in c.summary()


# ------------------------------------------------------------------------------------------------ binding, CLI, C ABI
def test_gain_table_and_judgment_checks():
    from snx.expansion import gain_table, judgment_csr
    t = gain_table(150)
    assert t.shape == (3, 150) and t.dtype == np.float64
    assert all(t[g - 1, p - 1] == (2 ** g - 1) / math.log2(p + 1) == R.gain(g, p) for g in (1, 2, 3) for p in (1, 2, 93, 150))
    ptr, tok, grade, rel = judgment_csr([[(3, 2, True), (9, 0, False)], [], [(700, 3, 1)]], 3)
    assert ptr.tolist() == [0, 2, 2, 3] and tok.tolist() == [3, 9, 700] and tok.dtype == np.int32
    assert grade.tolist() == [2, 0, 3] and rel.tolist() == [1, 0, 1] and grade.dtype == rel.dtype == np.uint8
    again = judgment_csr((ptr, tok, grade, rel), 3)
    assert all(np.array_equal(x, y) for x, y in zip(again, (ptr, tok, grade, rel)))
    for bad, msg in (([[(3, 2, True), (3, 1, True)]], "repeated"), ([[(3, 4, True)]], "grades"), ([[(2 ** 31, 1, True)]], "int32"),
                     ([[(3, 1, True)], []], "rows for"), ([[(1.5, 1, True)]], "int ids")):
        with pytest.raises(ValueError, match=msg):
            judgment_csr(bad, 1)
    with pytest.raises(ValueError, match="j_ptr must start at 0"):
        judgment_csr((np.array([0, 2]), np.array([1]), np.array([1]), np.array([1])), 1)
    with pytest.raises(ValueError):
        gain_table(0)


def test_cli_parser_defaults():
    from src.train.cli import eval_expansion as E
    a = E.parse_args(["--sample"])
    assert a.k_values == [5, 10, 20, 50, 100] and a.batch_size == 32 and a.checkpoint is None and a.domain is None
    assert a.compare is None and a.report is None and a.sample is True and a.eval_set is None and a.synonym_pairs is None
    b = E.parse_args(["--eval-set", "x.json", "--k-values", "1,3", "--domain", "legal", "--compare", "b", "--report", "r.json"])
    assert b.k_values == [1, 3] and str(b.eval_set) == "x.json" and b.domain == "legal" and b.compare == "b"
    for argv in ([], ["--sample", "--eval-set", "x.json"], ["--sample", "--k-values", "0"], ["--sample", "--batch-size", "0"]):
        with pytest.raises(SystemExit):
            E.parse_args(argv)
    assert len(E.load_dataset(E.parse_args(["--sample", "--domain", "medical"]))) == 5
    from src.train.data.collator import HashTokenizer
    h = HashTokenizer(1000)
    assert h.encode("a b", add_special_tokens=False) == h(["a b"])["input_ids"][0, 1:3].tolist()


def test_header_declares_the_section_and_the_library_exports_it():
    import ctypes as C
    import snx
    from snx._lib import SIGNATURES
    from snx import asmcheck, fn
    text = open(HEADER).read()
    assert "---- term-expansion evaluation (csrc/expansion.hip)" in text and "ties lowest id first" in text
    names = ("snx_expansion_workspace_bytes", "snx_expansion_ranks", "snx_expansion_metrics")
    for n in names:
        assert re.search(r"\b%s\(" % n, text) and n in SIGNATURES, n
    assert not [n for n in snx.verify_exports() if n in names]
    assert set(asmcheck.GUARDED["expansion.hip"]) == {"ex_count_kernel"}
    assert fn("snx_expansion_workspace_bytes")(3, 10) >= 13 * 4 and fn("snx_expansion_workspace_bytes")(0, 10) == 0
    # argument errors are returned before anything is launched (no GPU is needed to see the code)
    one = C.c_void_p(256)
    cuts = (C.c_int32 * 3)(5, 10, 20)
    P = lambda a: C.cast(a, C.c_void_p)                                         # noqa: E731
    M = fn("snx_expansion_metrics")

    def call(B=2, V=64, max_k=10, cutoffs=P(cuts), ncut=3, G=10, slices=0, rep=one, ws=one, ws_bytes=4096):
        return M(rep, B, V, one, one, one, one, one, 4, max_k, cutoffs, ncut, one, G, slices, one, one, one, one, one, ws,
                 ws_bytes, None)
    assert call(cutoffs=None) == -3 and call(ncut=0) == -3 and call(ncut=9) == -3
    assert call(cutoffs=P((C.c_int32 * 3)(5, 5, 20))) == -3 and call(cutoffs=P((C.c_int32 * 3)(0, 5, 20))) == -3
    assert call(B=-1) == -2 and call(V=0) == -2 and call(V=2 ** 30 + 1) == -2 and call(max_k=0) == -2
    assert call(G=9) == -3 and call(slices=-1) == -3 and call(rep=None) == -3
    assert call(ws=None) == -3 and call(ws_bytes=8) == -3
    assert call(max_k=100, G=19) == -3 and call(max_k=7, G=6) == -3 and call(B=0) == 0
    Rk = fn("snx_expansion_ranks")
    assert Rk(one, 2, 0, one, one, one, 4, 10, 0, one, one, one, 4096, None) == -2
    assert Rk(None, 2, 64, one, one, one, 4, 10, 0, one, one, one, 4096, None) == -3
    assert Rk(one, 2, 64, one, one, one, 4, 10, 0, one, one, None, 0, None) == -3

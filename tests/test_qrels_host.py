"""CPU checks of scoring against qrels (include/snx.h "relevance judgments"): the benchmark-directory loader, the
relevance CSR, the metrics and the interval arithmetic against the reference project's own outputs
(tests/golden/g14_qrels.json and g14_benchmark_dir, written by tools/make_golden_qrels.py), the numpy restatement
(tests/qrels_reference.py) that the GPU suite (test_gpu_qrels.py) holds csrc/qrels.hip to, and the C ABI's presence and
argument checks."""
import json
import os
import re

import numpy as np
import pytest

from tests import qrels_reference as Q

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g14_qrels.json")
GOLDEN_DIR = os.path.join(HERE, "golden", "g14_benchmark_dir")
HEADER = os.path.join(os.path.dirname(HERE), "include", "snx.h")
REPORT = ("recall_at_1", "recall_at_5", "recall_at_10", "mrr", "ndcg_at_10")
OURS = ("recall@1", "recall@5", "recall@10", "mrr", "ndcg@10")


def golden_qrels():
    with open(GOLDEN) as f:
        return json.load(f)


def interval_bound(n):
    """Values in [0, 1]; both sides sum n float64 terms and divide by n, each carrying at most n * 2^-53: n * 2^-52."""
    return n * 2.0 ** -52


# ------------------------------------------------------------------------------------------------ loader
def test_load_benchmark_dir_follows_the_reference_rules():
    from src.train.eval import load_benchmark_dir
    d = load_benchmark_dir(GOLDEN_DIR)
    assert d.doc_ids == [f"d{i}" for i in range(12)] and len(d.docs) == len(d.titles) == 12
    assert d.docs[0].startswith("red kettle with") and d.titles[3] == "wooden table 3"
    # first appearance in qrels.jsonl; q4's only qrel has score 0: not a query; q5's only relevant doc is not in the corpus
    assert d.query_ids == ["q2", "q0", "q1", "q3", "q5", "q6", "q7"]
    assert d.queries[1] == "red kettle number 0"
    assert d.relevant == [[2], [0, 9], [4], [3], [], [6], [7]]        # d1 (score 0), d99 and d404 (absent) kept out
    assert d.judged == [2, 2, 1, 2, 1, 1, 1]
    cut = load_benchmark_dir(GOLDEN_DIR, max_queries=3)
    assert cut.query_ids == ["q2", "q0", "q1"] and cut.relevant == [[2], [0, 9], [4]] and cut.docs == d.docs
    assert load_benchmark_dir(GOLDEN_DIR, max_queries=0).query_ids == d.query_ids


def test_load_benchmark_dir_names_a_query_without_text(tmp_path):
    from src.train.eval import load_benchmark_dir
    for name in ("corpus.jsonl", "queries.jsonl"):
        (tmp_path / name).write_text(open(os.path.join(GOLDEN_DIR, name)).read())
    (tmp_path / "qrels.jsonl").write_text(json.dumps({"query-id": "nope", "corpus-id": "d1", "score": 1}) + "\n")
    with pytest.raises(ValueError, match="nope"):
        load_benchmark_dir(str(tmp_path))


# ------------------------------------------------------------------------------------------------ relevance rows
def test_relevance_csr_sorts_merges_and_keeps_ids_outside_the_corpus():
    import torch
    from snx.retrieval import relevance_csr
    ptr, docs = relevance_csr([[5, 2, 5], [], [40, -3, 0], [7]], 4, 10, "cpu")
    assert ptr.dtype == torch.long and docs.dtype == torch.int32
    assert ptr.tolist() == [0, 2, 2, 5, 6] and docs.tolist() == [2, 5, -3, 0, 40, 7]
    p2, d2 = relevance_csr((torch.tensor([0, 3, 3, 6, 7]), torch.tensor([5, 2, 5, 40, -3, 0, 7], dtype=torch.int32)), 4, 10,
                           "cpu")
    assert p2.tolist() == ptr.tolist() and d2.tolist() == docs.tolist()
    e_ptr, e_docs = relevance_csr([], 0, 10, "cpu")
    assert e_ptr.tolist() == [0] and e_docs.numel() == 0
    for bad in ([[1]], [[1], [2], [3], [4], [5]], [[1.5], [], [], []], [[True], [], [], []], [[2 ** 31], [], [], []], "abcd",
                (torch.tensor([0, 1]), torch.tensor([1])), (torch.tensor([1, 1, 1, 1, 1]), torch.tensor([1])),
                (torch.tensor([0, 1, 0, 1, 1]), torch.tensor([1])), (torch.tensor([0., 1, 1, 1, 1]), torch.tensor([1]))):
        with pytest.raises(ValueError):
            relevance_csr(bad, 4, 10, "cpu")


# ------------------------------------------------------------------------------------------------ metrics
def test_reference_restatement_gives_the_recorded_hit_ranks():
    g = golden_qrels()
    assert g["n_bootstrap"] == 1000 and len(g["relevant"]) == 150
    assert any(len(r) == 0 for r in g["relevant"]) and any(d >= g["num_docs"] for r in g["relevant"] for d in r)
    assert max(len(r) for r in g["relevant"]) >= 4
    for m in g["methods"].values():
        first, hits, dcg = Q.ranked_relevance(np.asarray(m["lists"], np.int32), g["relevant"], g["num_docs"], (1, 5, 10))
        assert first.tolist() == m["hit_ranks"]
        assert (hits[:, 0] <= hits[:, 1]).all() and (hits[:, 1] <= hits[:, 2]).all() and int(hits.max()) >= 2
        assert ((first == 0) == (hits[:, 2] == 0)).all()


def test_qrels_metrics_equal_the_reference_values():
    from src.train.eval import REPORT_KEYS, first_relevant_values, qrels_metrics
    g = golden_qrels()
    nd = g["num_docs"]
    nrel = np.asarray([sum(1 for d in r if 0 <= d < nd) for r in g["relevant"]])
    assert tuple(REPORT_KEYS) == OURS and tuple(REPORT_KEYS.values()) == REPORT
    for name, m in g["methods"].items():
        first, hits, dcg = Q.ranked_relevance(np.asarray(m["lists"], np.int32), g["relevant"], nd, (1, 5, 10))
        out = qrels_metrics(m["hit_ranks"], hits, dcg, nrel, (1, 5, 10))
        for ours, ref in zip(OURS, REPORT):
            print(name, ours, out[ours], float.fromhex(m["metrics"][ref]))
            assert out[ours] == float.fromhex(m["metrics"][ref]), (name, ours)
        assert out["num_queries"] == m["num_queries"] == 150
        # the multi-relevant numbers, against their definitions written out
        disc = Q.discount_table(10)
        for j, c in enumerate((1, 5, 10)):
            frac = [h / n if n else 0.0 for h, n in zip(hits[:, j].tolist(), nrel.tolist())]
            assert out[f"recall_frac@{c}"] == float(np.mean(frac))
            nd_multi = []
            for q in range(150):
                idcg = 0.0
                for p in range(min(int(nrel[q]), c)):
                    idcg = idcg + disc[p]
                nd_multi.append(dcg[q, j] / idcg if idcg > 0 else 0.0)
            assert out[f"ndcg_multi@{c}"] == float(np.mean(nd_multi))
        assert 0 < out["recall_frac@10"] <= out["recall@10"] and 0 < out["ndcg_multi@10"] <= 1
        # a rank beyond the list depth is a miss
        deep = [r + 7 if r else 0 for r in m["hit_ranks"]]
        v = first_relevant_values(deep, k=10)
        assert ((v[:, 3] > 0) == np.asarray([1 <= r <= 10 for r in deep])).all()
        assert qrels_metrics(deep, hits, dcg, nrel, (1, 5, 10), k=8)["recall@10"] == float(np.mean([1 <= r <= 8 for r in deep]))
    with pytest.raises(ValueError):
        qrels_metrics([1, 2], np.zeros((3, 3)), np.zeros((3, 3)), [1, 1, 1])


def test_bootstrap_indices_are_the_reference_stream_for_every_draw():
    from snx.retrieval import bootstrap_indices
    for n in (150, 7):
        idx = bootstrap_indices(n, 1000, 42)
        assert idx.shape == (1000, n) and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < n
        np.random.seed(42)                                     # ref:benchmark/metrics.py:198-204, draw by draw
        for b in range(1000):
            assert np.array_equal(np.random.choice(n, size=n, replace=True), idx[b]), (n, b)
    assert not np.array_equal(bootstrap_indices(150, 2, 42), bootstrap_indices(150, 2, 43))
    with pytest.raises(ValueError):
        bootstrap_indices(0)


def test_interval_arithmetic_equals_the_reference_intervals():
    """The restated fixed summation order in place of the kernel: the same bound as the GPU test, derived from n."""
    from snx.retrieval import bootstrap_indices
    from src.train.eval import first_relevant_values, interval_from_means
    g = golden_qrels()
    idx = bootstrap_indices(150, g["n_bootstrap"], g["seed"])
    for name, m in g["methods"].items():
        vals = first_relevant_values(m["hit_ranks"], k=10)
        n = vals.shape[0]
        assert vals.min() >= 0.0 and vals.max() <= 1.0
        means = Q.bootstrap_means(vals, idx)
        for col, key in ((0, "recall@1"), (3, "mrr"), (4, "ndcg@10")):
            got = interval_from_means(vals[:, col], means[:, col], g["confidence"])
            for x in ("point_estimate", "lower", "upper"):
                want = float.fromhex(m["ci"][key][x])
                print(name, key, x, got[x], want, abs(got[x] - want))
                assert abs(got[x] - want) <= interval_bound(n), (name, key, x)
            assert got["lower"] < got["point_estimate"] < got["upper"]


def test_bootstrap_reference_order_is_the_documented_one():
    # n = 130: segments [0, 64), [64, 128), [128, 130); values chosen so that the order of the adds shows
    rng = np.random.default_rng(3)
    v = rng.random((130, 2)) * np.array([1.0, 1e-9]) + np.array([0.0, 1.0])
    idx = rng.integers(0, 130, (5, 130))
    got = Q.bootstrap_means(v, idx)
    for b in range(5):
        for m in range(2):
            segs = []
            for s0 in (0, 64, 128):
                acc = 0.0
                for i in range(s0, min(130, s0 + 64)):
                    acc = acc + float(v[idx[b, i], m])
                segs.append(acc)
            assert got[b, m] == ((0.0 + segs[0]) + segs[1] + segs[2]) / 130.0


def test_paired_t_test_over_first_relevant_ranks_equals_the_reference():
    from src.train.eval import paired_t_test
    g = golden_qrels()
    t = paired_t_test(g["methods"]["a"]["hit_ranks"], g["methods"]["b"]["hit_ranks"])
    want_t, want_p = float.fromhex(g["ttest"]["statistic"]), float.fromhex(g["ttest"]["p_value"])
    assert abs(t["statistic"] - want_t) <= 1e-10 * abs(want_t) and abs(t["p_value"] - want_p) <= 1e-8 * abs(want_p)
    assert t["significant"] is g["ttest"]["significant"] is True


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_section_and_the_library_exports_it():
    import snx
    from snx._lib import SIGNATURES
    text = open(HEADER).read()
    assert "---- relevance judgments (csrc/qrels.hip)" in text
    assert re.search(r"#define SNX_BOOTSTRAP_SEGMENT 64\b", text) and "ascending segment order" in text
    names = ("snx_sparse_first_relevant_workspace_bytes", "snx_sparse_first_relevant", "snx_ranked_relevance",
             "snx_bootstrap_means")
    for n in names:
        assert re.search(r"\b%s\(" % n, text) and n in SIGNATURES, n
    assert not [n for n in snx.verify_exports() if n in names]
    from snx.retrieval import BOOTSTRAP_SEGMENT
    assert BOOTSTRAP_SEGMENT == Q.SEGMENT == 64
    from snx import asmcheck
    assert set(asmcheck.GUARDED["qrels.hip"]) == {"qr_best_kernel", "qr_count_kernel", "qr_boot_kernel"}


def test_qrels_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes as C
    from snx import fn
    one = C.c_void_p(16)
    ws_bytes = fn("snx_sparse_first_relevant_workspace_bytes")
    assert ws_bytes(0, 10, 0) == 0 and ws_bytes(3, -1, 0) == 0 and ws_bytes(3, 10, -1) == 0
    assert ws_bytes(3, 100000, 0) >= 3 * 7 * 4 and ws_bytes(3, 100000, 1000) >= 3 * 100 * 4
    first = fn("snx_sparse_first_relevant")
    # q_ptr q_term q_w nq term_ptr post_doc post_w doc_ptr doc_term doc_w nd V rel_ptr rel_doc chunk out_doc out_score
    # out_rank out_nrel workspace ws_bytes stream
    args = [one, one, one, 4, one, one, one, one, one, one, 100, 50, one, one, 0, one, one, one, one, one, 1 << 20, None]
    for i, v, rc in ((0, None, -3), (4, None, -3), (7, None, -3), (12, None, -3), (15, None, -3), (16, None, -3),
                     (17, None, -3), (18, None, -3), (3, -1, -2), (10, -1, -2), (11, 0, -2), (14, -1, -2), (14, 32769, -2),
                     (19, None, -3), (20, 8, -3)):
        bad = list(args)
        bad[i] = v
        assert first(*bad) == rc, (i, v)
    ok = list(args)
    ok[3] = 0                                                                # nothing to launch
    assert first(*ok) == 0
    ranked = fn("snx_ranked_relevance")
    cut = lambda *c: C.cast((C.c_int32 * len(c))(*c), C.c_void_p)            # noqa: E731
    # docs nq R nd rel_ptr rel_doc cutoffs ncut disc out_first out_hits out_dcg stream
    args = [one, 4, 100, 50, one, one, cut(1, 5, 10), 3, one, one, one, one, None]
    for i, v, rc in ((2, 0, -2), (2, 4097, -2), (1, -1, -2), (3, -1, -2), (6, None, -3), (7, 0, -3), (7, 9, -3),
                     (6, cut(0, 5, 10), -3), (6, cut(1, 5, 101), -3), (6, cut(1, 5, 5), -3), (6, cut(5, 1, 10), -3),
                     (0, None, -3), (4, None, -3), (8, None, -3), (9, None, -3), (10, None, -3), (11, None, -3)):
        bad = list(args)
        bad[i] = v
        assert ranked(*bad) == rc, (i, v)
    ok = list(args)
    ok[1] = 0
    assert ranked(*ok) == 0
    boot = fn("snx_bootstrap_means")
    # values n M idx nboot out stream
    args = [one, 100, 3, one, 1000, one, None]
    for i, v, rc in ((1, 0, -2), (2, 0, -2), (2, 17, -2), (4, -1, -2), (0, None, -3), (3, None, -3), (5, None, -3)):
        bad = list(args)
        bad[i] = v
        assert boot(*bad) == rc, (i, v)
    ok = list(args)
    ok[4] = 0
    assert boot(*ok) == 0


def test_python_layer_rejects_bad_arguments_without_a_gpu():
    import torch
    from snx.retrieval import bootstrap_means, ranked_relevance
    with pytest.raises(ValueError):
        ranked_relevance(torch.zeros((2, 10), dtype=torch.int32), [[], []], 5)            # not on a GPU
    with pytest.raises(ValueError):
        ranked_relevance(torch.zeros((2, 10), dtype=torch.int64), [[], []], 5)
    for bad in (np.zeros((0, 2)), np.zeros((3, 17)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            bootstrap_means(bad)
    from snx._lib import SnxError
    for idx in ([[0, 1, 3]], [[-1, 0, 0]]):
        with pytest.raises(SnxError, match="SNX_E_ARG"):
            bootstrap_means(np.zeros(3), indices=np.asarray(idx))
    with pytest.raises(ValueError):
        bootstrap_means(np.zeros(3), indices=np.zeros((2, 4), np.int64))


def test_cli_arguments():
    from src.train.cli import eval_benchmark as E
    a = E.parse_args(["--benchmark-dir", "x"])
    assert a.methods == list(E.METHODS) == ["sparse", "bm25", "bm25_sparse_rrf", "two_phase", "seismic"]
    assert a.top_k == 10 and a.bootstrap == 1000 and a.max_queries is None and a.report is None
    assert E.parse_args(["--benchmark-dir", "x", "--methods", "bm25,sparse"]).methods == ["bm25", "sparse"]
    for bad in (["--methods", "sparse,dense"], ["--methods", "sparse,sparse"], ["--methods", ""], ["--top-k", "9"],
                ["--top-k", "101"], ["--bootstrap", "-1"]):
        with pytest.raises(SystemExit):
            E.parse_args(["--benchmark-dir", "x"] + bad)
    with pytest.raises(SystemExit):
        E.parse_args([])

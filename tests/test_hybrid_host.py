"""CPU checks of the BM25 baseline and rank fusion (include/snx.h "BM25 baseline and rank fusion"): the numpy references
(tests/fusion_reference.py, tests/bm25_reference.py) that the GPU suite (test_gpu_hybrid.py) holds csrc/hybrid.hip to are
pinned here -- against the reference project's own fused scores (tests/golden/g13_fusion.json, written by
tools/make_golden_fusion.py) bit for bit, and by hand-worked examples; then src.train.eval.paired_t_test against the
reference's scipy values, the C ABI's argument checks, the evaluator's parameters, the CLI's rows and the
benchmark.score_fusion mirror."""
import json
import math
import os

import numpy as np
import pytest

from tests import bm25_reference as B
from tests import fusion_reference as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_fusion.json")


def golden_fusion():
    with open(GOLDEN) as f:
        return json.load(f)


def runs_of(case):
    """[(run, {doc: fused score})] of one fixture case, scores decoded from their float64 hex."""
    return [(run, {int(d): float.fromhex(h) for d, h in run["scores"].items()}) for run in case["runs"]]


# ------------------------------------------------------------------------------------------------ fusion
def test_reference_reproduces_the_golden_scores_bit_for_bit():
    g = golden_fusion()
    names = {c["name"] for c in g["fusion"]}
    assert {"unequal_lengths", "one_empty", "both_empty", "disjoint", "identical", "all_scores_equal", "longer_than_99",
            "triple"} <= names and "HybridTripleSearcher.search" in g["triple_source"]
    checked = 0
    for case in g["fusion"]:
        lists = [(c["docs"], c["scores"]) for c in case["lists"]]
        assert all(np.float32(s) == s for _, ss in lists for s in ss)
        for run, want in runs_of(case):
            docs, scores = F.fuse(lists, run["method"], **run["params"])
            assert len(docs) == run["total_hits"] == len(want), case["name"]
            got = dict(zip(docs.tolist(), scores.tolist()))
            assert {d: s.hex() for d, s in got.items()} == {d: s.hex() for d, s in want.items()}, (case["name"], run)
            # the order: only strictly different reference scores constrain it; ties go by doc id
            assert docs.tolist() == sorted(want, key=lambda d: (-want[d], d)), (case["name"], run)
            checked += 1
    assert checked > 80
    long = next(c for c in g["fusion"] if c["name"] == "longer_than_99")
    assert max(len(c["docs"]) for c in long["lists"]) + 1 > 100             # len + 1 beats the default penalty rank


def test_reference_reproduces_the_hand_worked_fusions():
    # RRF, k = 60.  A = [d7, d3, d9], B = [d3, d5].  max_rank = max(4, 3, 100) = 100: an absent doc adds 1 / 160.
    #   d3: 1/62 + 1/61   d7: 1/61 + 1/160   d5: 1/160 + 1/62   d9: 1/63 + 1/160
    # 1/61 + 1/160 > 1/62 + 1/160 = 1/160 + 1/62 (addition commutes, also in floating point) > 1/63 + 1/160: no tie yet.
    docs, scores = F.fuse([([7, 3, 9], [3.0, 2.0, 1.0]), ([3, 5], [4.0, 1.0])], "rrf", k=60)
    assert docs.tolist() == [3, 7, 5, 9]
    assert scores.tolist() == [1 / 62 + 1 / 61, 1 / 61 + 1 / 160, 1 / 160 + 1 / 62, 1 / 63 + 1 / 160]
    # a tie: A = [d8, d2, d4], B = [d2, d8] -> d8: 1/61 + 1/62, d2: 1/62 + 1/61: equal, so d2 (the lower id) comes first;
    # d4 is absent from B (whose third slot is unused): 1/63 + 1/160.
    docs, scores = F.fuse([([8, 2, 4], [1.0, 1.0, 1.0]), ([2, 8, -1], [1.0, 1.0, 0.0])], "rrf", k=60)
    assert docs.tolist() == [2, 8, 4] and scores[0] == scores[1] == 1 / 61 + 1 / 62 and scores[2] == 1 / 63 + 1 / 160
    # entries behind the first negative id are not part of the list
    assert F.fuse([([1, -1, 5], [1.0, 0.0, 9.0])], "rrf")[0].tolist() == [1]
    # weighted RRF: the same fold with w_l / (k + rank)
    docs, scores = F.fuse([([7, 3], [2.0, 1.0]), ([3], [1.0])], "weighted_rrf", k=60, weights=(0.4, 0.6))
    assert docs.tolist() == [3, 7] and scores.tolist() == [0.4 / 62 + 0.6 / 61, 0.4 / 61 + 0.6 / 160]
    # linear, alpha = 0.25.  A's scores are all 2.5: every entry of A normalises to 1.0.  B = [d1: 8, d6: 6, d0: 4]:
    # min 4, max 8 -> 1.0, 0.5, 0.0.  With A = [d0, d1]:
    #   d1: .25 * 1 + .75 * 1 = 1     d0: .25 * 1 + .75 * 0 = .25     d6: .25 * 0 + .75 * .5 = .375
    docs, scores = F.fuse([([0, 1], [2.5, 2.5]), ([1, 6, 0], [8.0, 6.0, 4.0])], "linear", alpha=0.25)
    assert docs.tolist() == [1, 6, 0] and scores.tolist() == [1.0, 0.375, 0.25]
    # one list empty: its docs are all absent (0.0); both empty: nothing
    docs, scores = F.fuse([([], []), ([4, 2], [3.0, 1.0])], "linear", alpha=0.25)
    assert docs.tolist() == [4, 2] and scores.tolist() == [0.75, 0.0]
    assert F.fuse([([], []), ([-1], [0.0])], "rrf")[0].tolist() == []
    s, d, r, t = F.fuse_batch(np.array([[[7, 3, 9]], [[3, 5, -1]]]), np.ones((2, 1, 3), np.float32), "rrf", 2, [9])
    assert d.tolist() == [[3, 7]] and r.tolist() == [4] and t.tolist() == [4]


# ------------------------------------------------------------------------------------------------ BM25
# V = 6; id 4 is not allowed.  Four docs of S = 6 positions (mask 0: not counted):
#   d0: 1 1 2 (4) [5]     -> terms {1: 2, 2: 1}, dl 3     (4 disallowed, the 5 is masked)
#   d1: 2 3 3 3 0 0       -> terms {0: 2, 2: 1, 3: 3}, dl 6
#   d2: everything masked -> empty, dl 0
#   d3: 1 (7) (-1) 5      -> terms {1: 1, 5: 1}, dl 2     (7 and -1 are outside [0, V))
# df = [1, 2, 2, 1, 0, 1], N = 4, total length 11, avgdl = 2.75.
HAND_IDS = [[1, 1, 2, 4, 5, 0], [2, 3, 3, 3, 0, 0], [1, 2, 3, 0, 0, 0], [1, 7, -1, 5, 0, 0]]
HAND_MASK = [[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0]]
HAND_ALLOWED = [1, 1, 1, 1, 0, 1]


def test_reference_reproduces_the_hand_worked_bm25_corpus():
    term, tf, cnt, length = B.term_counts(HAND_IDS, HAND_MASK, HAND_ALLOWED)
    assert term.tolist() == [[1, 2, -1, -1, -1, -1], [0, 2, 3, -1, -1, -1], [-1] * 6, [1, 5, -1, -1, -1, -1]]
    assert tf.tolist() == [[2, 1, 0, 0, 0, 0], [2, 1, 3, 0, 0, 0], [0] * 6, [1, 1, 0, 0, 0, 0]]
    assert cnt.tolist() == [2, 3, 0, 2] and length.tolist() == [3, 6, 0, 2]
    rows, df, dl, idf, avg = B.bm25_rows(HAND_IDS, HAND_MASK, HAND_ALLOWED)
    assert df.tolist() == [1, 2, 2, 1, 0, 1] and dl.tolist() == [3, 6, 0, 2] and avg == 2.75
    assert idf.tolist() == [math.log1p(3.5 / 1.5), math.log1p(2.5 / 2.5), math.log1p(2.5 / 2.5), math.log1p(3.5 / 1.5),
                            math.log1p(4.5 / 0.5), math.log1p(3.5 / 1.5)]
    # d0, term 1: tf 2, norm = 1.2 * (0.25 + 0.75 * (3 / 2.75)); w = log(2) * 2 / (2 + norm)
    norm0 = 1.2 * ((1.0 - 0.75) + 0.75 * (3 / 2.75))
    assert rows[0][0].tolist() == [1, 2] and rows[0][1].dtype == np.float32
    assert rows[0][1].tolist() == [float(np.float32(math.log1p(1.0) * (2 / (2 + norm0)))),
                                   float(np.float32(math.log1p(1.0) * (1 / (1 + norm0))))]
    assert len(rows[2][0]) == 0 and len(rows[2][1]) == 0                       # the empty doc is a row of length 0
    # b = 0: no length normalisation, norm = k1; k1 = 0: every weight is the idf
    flat = B.bm25_rows(HAND_IDS, HAND_MASK, HAND_ALLOWED, k1=1.2, b=0.0)[0]
    assert flat[1][1].tolist() == [float(np.float32(idf[0] * (2 / 3.2))), float(np.float32(idf[2] * (1 / 2.2))),
                                   float(np.float32(idf[3] * (3 / 4.2)))]
    binary = B.bm25_rows(HAND_IDS, HAND_MASK, HAND_ALLOWED, k1=0.0)[0]
    assert binary[3][1].tolist() == [float(np.float32(idf[1])), float(np.float32(idf[5]))]
    q = B.query_rows([[5, 5, 4, 1]], [[1, 1, 1, 0]], HAND_ALLOWED)
    assert q[0][0].tolist() == [5] and q[0][1].tolist() == [2.0]               # a repeated query term counts twice


# ------------------------------------------------------------------------------------------------ t-test
def _close(got, want, rel):
    if want != want:
        return got != got
    return got == want or abs(got - want) <= rel * abs(want)


def test_paired_t_test_against_the_reference():
    from src.train.eval import betainc, paired_t_test
    cases = {c["name"]: c for c in golden_fusion()["ttest"]}
    assert set(cases) == {"mixed", "identical", "one_pair", "all_misses", "strong"}
    for name, c in cases.items():
        got = paired_t_test(c["ranks_a"], c["ranks_b"])
        want_t = float("nan") if c["statistic"] == "nan" else float.fromhex(c["statistic"])
        want_p = float("nan") if c["p_value"] == "nan" else float.fromhex(c["p_value"])
        print(name, got, want_t, want_p)
        assert _close(got["statistic"], want_t, 1e-10), (name, got, want_t)
        assert _close(got["p_value"], want_p, 1e-8), (name, got, want_p)
        assert got["significant"] is c["significant"], name
    for name in ("identical", "one_pair", "all_misses"):
        assert cases[name]["p_value"] == "nan" and not cases[name]["significant"]
    assert cases["strong"]["significant"] and float.fromhex(cases["strong"]["p_value"]) < 1e-6
    with pytest.raises(ValueError):
        paired_t_test([1, 2], [1])
    # a rank above k is a miss: at k = 3 the 5 counts 0.0
    assert paired_t_test([1, 5, 2], [2, 0, 2], k=3) == paired_t_test([1, 0, 2], [2, 0, 2], k=3)
    assert betainc(2.0, 3.0, 0.0) == 0.0 and betainc(2.0, 3.0, 1.0) == 1.0
    assert abs(betainc(1.0, 1.0, 0.3) - 0.3) < 1e-15 and abs(betainc(2.0, 1.0, 0.5) - 0.25) < 1e-15


# ------------------------------------------------------------------------------------------------ C ABI
def test_hybrid_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes as C
    from snx import fn
    one = C.c_void_p(16)
    prm = (C.c_double * 5)(60.0, 0.4, 0.6, 1.0, 1.0)
    p = C.cast(prm, C.c_void_p)
    fuse = fn("snx_fuse_ranked")
    # docs scores L nq R method params target top_k out_doc out_score out_total out_rank stream
    args = [one, one, 2, 8, 100, 0, p, one, 10, one, one, one, one, None]
    for i, v, rc in ((2, 0, -3), (2, 5, -3), (5, 3, -3), (5, -1, -3), (4, 1025, -2), (4, 0, -2), (8, 0, -2), (8, 4097, -2),
                     (3, -1, -2), (6, None, -3), (0, None, -3), (9, None, -3), (10, None, -3), (11, None, -3),
                     (12, None, -3)):
        bad = list(args)
        bad[i] = v
        assert fuse(*bad) == rc, (i, v)
    lin = list(args)
    lin[5] = 2
    lin[2] = 3
    assert fuse(*lin) == -3                                                  # linear takes exactly two lists
    lin[2] = 2
    for alpha in (-0.1, 1.5, float("nan")):
        prm2 = (C.c_double * 1)(alpha)
        lin[6] = C.cast(prm2, C.c_void_p)
        assert fuse(*lin) == -3, alpha
    for k in (-1.0, float("inf"), float("nan")):
        prm3 = (C.c_double * 3)(k, 1.0, 1.0)
        bad = list(args)
        bad[6] = C.cast(prm3, C.c_void_p)
        assert fuse(*bad) == -3, k
    ok = list(args)
    ok[3] = 0                                                                # nothing to launch
    assert fuse(*ok) == 0
    counts = fn("snx_term_counts")
    smax = fn("snx_term_counts_max_len")()
    assert smax >= 8192
    # input_ids attention_mask allowed n S V out_term out_tf out_cnt out_len stream
    args = [one, one, one, 4, 64, 1000, one, one, one, one, None]
    for i, v, rc in ((4, smax + 1, -2), (4, 0, -2), (3, -1, -2), (5, 0, -2), (0, None, -3), (1, None, -3), (2, None, -3),
                     (6, None, -3), (7, None, -3), (8, None, -3), (9, None, -3)):
        bad = list(args)
        bad[i] = v
        assert counts(*bad) == rc, (i, v)
    ok = list(args)
    ok[3] = 0
    assert counts(*ok) == 0
    weights = fn("snx_bm25_weights")
    # ptr term tf dl idf n nnz V avgdl k1 b w stream
    args = [one, one, one, one, one, 4, 100, 1000, 2.5, 1.2, 0.75, one, None]
    for i, v, rc in ((9, -1.0, -3), (9, float("nan"), -3), (10, 1.5, -3), (10, -0.1, -3), (8, 0.0, -3), (8, -1.0, -3),
                     (5, -1, -2), (6, -1, -2), (7, 0, -2), (0, None, -3), (4, None, -3), (11, None, -3)):
        bad = list(args)
        bad[i] = v
        assert weights(*bad) == rc, (i, v)
    ok = list(args)
    ok[6], ok[8] = 0, 0.0                                                    # every doc empty: nothing to weigh
    assert weights(*ok) == 0
    df = fn("snx_bm25_doc_freq")
    assert df(one, -1, 10, one, None) == -2 and df(one, 5, 0, one, None) == -2 and df(None, 5, 10, one, None) == -3
    assert df(one, 0, 10, one, None) == 0


# ------------------------------------------------------------------------------------------------ Python surface
def test_hybrid_parameters_the_cli_rows_and_host_validation():
    import torch
    from snx.retrieval import Bm25Index, fuse_ranked
    from src.train.cli.eval_hybrid import parse_args, rows
    from src.train.eval import HYBRID_DEFAULTS, hybrid_params
    assert HYBRID_DEFAULTS == {"method": "rrf", "k": 60, "alpha": 0.4, "retrieval_k": 100, "k1": 1.2, "b": 0.75}
    assert hybrid_params({}) == HYBRID_DEFAULTS and hybrid_params({"alpha": 0.5}) == dict(HYBRID_DEFAULTS, alpha=0.5)
    for bad in ({"rrf_k": 60}, {"method": "nope"}, {"retrieval_k": 0}, {"retrieval_k": 2000}):
        with pytest.raises(ValueError):
            hybrid_params(bad)
    assert [r[0] for r in rows(parse_args([]))] == ["sparse", "bm25", "bm25_sparse_rrf"]
    grid = rows(parse_args(["--sweep"]))[3:]
    assert [(r[1], r[2]) for r in grid] == [("linear", {"alpha": 0.3}), ("linear", {"alpha": 0.4}),
                                           ("linear", {"alpha": 0.5}),
                                           ("weighted_rrf", {"k": 60, "weights": (0.4, 0.6)})]
    assert all(r[3] == ("bm25", "sparse") for r in grid)
    seven = rows(parse_args(["--dense-run", "x.npz"]))
    assert [r[0] for r in seven] == ["sparse", "bm25", "bm25_sparse_rrf", "dense", "bm25_dense_rrf", "dense_sparse_rrf",
                                     "triple_rrf"]
    assert seven[-1][3] == ("bm25", "dense", "sparse") and len(rows(parse_args(["--sweep", "--dense-run", "x"]))) == 11
    for bad in (["--retrieval-k", "0"], ["--retrieval-k", "1025"], ["--b", "1.5"], ["--k1", "-1"], ["--rrf-k", "x"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    for kw in ({"k1": -1.0}, {"b": 1.5}, {"k1": float("nan")}):
        with pytest.raises(ValueError):
            Bm25Index(16, "cpu", **kw)
    with pytest.raises(ValueError):
        Bm25Index(0, "cpu")
    with pytest.raises(RuntimeError):
        Bm25Index(16, "cpu").search_tokens(None, None, None, 10)
    pair = (torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 4)))
    for lists, method, kw in (([pair, pair], "nope", {}), ([], "rrf", {}), ([pair] * 5, "rrf", {}),
                              ([pair] * 3, "linear", {}), ([pair, pair], "linear", {"alpha": 1.5}),
                              ([pair, pair], "rrf", {"alpha": 0.4}), ([pair, pair], "rrf", {"k": -1}),
                              ([pair] * 3, "weighted_rrf", {}), ([pair, pair], "weighted_rrf", {"weights": (1.0,)}),
                              ([pair, pair], "rrf", {})):                       # the last: lists must live on a GPU
        with pytest.raises(ValueError):
            fuse_ranked(lists, method, 10, **kw)


def test_score_fusion_mirror_keeps_the_reference_interface():
    import inspect
    from benchmark import score_fusion as S
    assert S.RRFFusion().k == 60 and S.LinearFusion().alpha == 0.4
    w = S.WeightedRRFFusion()
    assert (w.k, w.sparse_weight, w.dense_weight) == (60, 0.4, 0.6)
    assert list(inspect.signature(S.WeightedRRFFusion.__init__).parameters) == ["self", "k", "sparse_weight", "dense_weight"]
    assert list(inspect.signature(S.ScoreFusion.fuse).parameters) == ["self", "sparse_results", "dense_results"]
    assert isinstance(S.create_fusion_method("rrf", k=10), S.RRFFusion) and S.create_fusion_method("rrf", k=10).k == 10
    assert isinstance(S.create_fusion_method("linear", alpha=0.3), S.LinearFusion)
    assert isinstance(S.create_fusion_method("weighted_rrf"), S.WeightedRRFFusion)
    with pytest.raises(ValueError):
        S.create_fusion_method("nope")
    with pytest.raises(ValueError):
        S.LinearFusion(alpha=1.5)
    r = S.RankedResult(doc_id="a", score=1.5, rank=1)
    assert (r.doc_id, r.score, r.rank) == ("a", 1.5, 1)


def test_evaluator_keys_are_unchanged_without_hybrid(monkeypatch):
    from src.train.data.collator import create_tokenizer
    from src.train.eval import HYBRID_KEYS, MidTrainingEvaluator
    plain_keys = ["recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10", "num_queries", "num_docs", "avg_nnz_q",
                  "avg_nnz_d"]
    assert HYBRID_KEYS == tuple(f"{p}_{k}" for p in ("bm25", "hybrid") for k in
                                ("recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10")) + \
        ("hybrid_total", "sparse_vs_bm25_p", "hybrid_vs_sparse_p")
    tok = create_tokenizer("hash:1000")
    monkeypatch.setattr(MidTrainingEvaluator, "encode", lambda self, model: (None, None))
    kw = dict(tokenizer=tok, val_file="synthetic:20:2", max_queries=5, max_docs=12, device="cpu")
    assert list(MidTrainingEvaluator(**kw).evaluate(None)) == plain_keys
    assert list(MidTrainingEvaluator(**kw, hybrid=None).evaluate(None)) == plain_keys
    out = MidTrainingEvaluator(**kw, hybrid={}).evaluate(None)
    assert list(out) == plain_keys + list(HYBRID_KEYS) and all(out[k] == 0.0 for k in HYBRID_KEYS)
    with pytest.raises(ValueError):
        MidTrainingEvaluator(**kw, hybrid={"ratio": 0.4})

"""CPU checks of pruning and two-phase search (include/snx.h "pruning and two-phase search"): a hand-worked example pins
the numpy reference (tests/two_phase_reference.py) that the GPU suite (test_gpu_two_phase.py) holds csrc/two_phase.hip
to; the C ABI's argument checks, the window arithmetic, the evaluator's parameters and the grid of the CLI
src.train.cli.eval_pruning."""
import numpy as np
import pytest

from tests import two_phase_reference as R

# One row, V = 5, dyadic weights.  Order by (weight desc, term asc): t1 1, t0 .5, t2 .5, t3 .25, t4 .125.
HAND_ROW = ([0, 1, 2, 3, 4], [0.5, 1.0, 0.5, 0.25, 0.125])
HAND_PRUNE = [
    ("max_ratio", 0.5, [1, 1, 1, 0, 0]),       # threshold .5 * 1: the entries at .5 stay (>=)
    ("max_ratio", 0.0, [1, 1, 1, 1, 1]),
    ("max_ratio", 1.0, [0, 1, 0, 0, 0]),       # the maximum always stays
    ("abs_value", 0.3, [1, 1, 1, 0, 0]),
    ("abs_value", 2.0, [0, 0, 0, 0, 0]),       # a row may become empty
    ("top_k", 2, [1, 1, 0, 0, 0]),             # t0 and t2 tie at .5: the lower term wins
    ("top_k", 3, [1, 1, 1, 0, 0]),
    ("top_k", 9, [1, 1, 1, 1, 1]),
    ("alpha_mass", 0.5, [1, 1, 0, 0, 0]),      # total 2.375, goal 1.1875: 1 < goal <= 1.5
    ("alpha_mass", 0.01, [0, 1, 0, 0, 0]),     # goal .02375 is passed by the first entry: at least one is kept
    ("alpha_mass", 1.0, [1, 1, 1, 1, 1]),
]

# V = 6.  Posting lists: t0 {d0, d1, d4}, t1 {d0, d2, d4}, t2 {d1, d4, d5}, t3 {d2, d3}, t4 {d5}, t5 {}.
HAND_V = 6
HAND_DOCS = [([0, 1], [1.0, 0.5]),
             ([0, 2], [0.5, 1.0]),
             ([1, 3], [1.0, 0.5]),
             ([3], [1.0]),
             ([0, 1, 2], [0.25, 0.25, 0.25]),
             ([2, 4], [0.5, 1.0])]
HAND_QUERIES = [([0, 2, 3], [1.0, 0.625, 0.25]), ([3, 4], [0.5, 1.0]), ([0, 2, 3], [1.0, 0.625, 0.25]), ([], [])]
HAND_TARGETS = [0, 3, 4, 0]
HAND_K, HAND_TYPE, HAND_VALUE, HAND_RATE, HAND_MAXW = 2, "max_ratio", 0.75, 1.5, 10000        # W = floor(2 * 1.5) = 3
# q0: threshold .75 * 1 keeps t0 alone.  Phase 1 over t0: d0 1, d1 .5, d4 .25 -> window d0, d1, d4.  Full scores: d0 1,
# d1 .5 + .625 * 1 = 1.125, d4 .25 + .625 * .25 = .40625: the dropped t2 puts d1 in front of d0.  Target d0 is second.
# q1: threshold .75 keeps t4.  Phase 1: d5 alone.  Exact search would return d5 1, d3 .5 (d3 holds t3 only): d3 is
# reachable through the dropped token alone and is missed; its score is still reported (target outside the window).
# q2 = q0 with target d4: inside the window at position 3 > k, so absent from the output.  q3 is empty.
HAND_DOCS_OUT = [[1, 0], [5, -1], [1, 0], [-1, -1]]
HAND_SCORES_OUT = [[1.125, 1.0], [1.0, 0.0], [1.125, 1.0], [0.0, 0.0]]
HAND_RANK = [2, 0, 0, 0]
HAND_TSCORE = [1.0, 0.5, 0.40625, 0.0]
HAND_STATS = [[3, 8, 3], [1, 3, 1], [3, 8, 3], [0, 0, 0]]
HAND_EXACT_DOCS = [[1, 0], [5, 3], [1, 0], [-1, -1]]


def test_reference_reproduces_the_hand_worked_prunes():
    for ptype, value, want in HAND_PRUNE:
        assert R.keep_mask(HAND_ROW[1], ptype, value).astype(int).tolist() == want, (ptype, value)
        assert R.keep_mask([], ptype, value).tolist() == []                     # empty rows stay empty
        assert R.keep_mask([0.25], ptype, value).tolist() == [not (ptype == "abs_value" and value > 0.25)]
    kept, rest = R.prune([HAND_ROW], "top_k", 2)
    assert kept[0][0].tolist() == [0, 1] and rest[0][0].tolist() == [2, 3, 4]
    assert kept[0][1].tolist() == [0.5, 1.0] and rest[0][1].tolist() == [0.5, 0.25, 0.125]


def test_reference_reproduces_the_hand_worked_two_phase_search():
    sc, dc, rk, ts, stats = R.two_phase(HAND_DOCS, HAND_QUERIES, HAND_V, HAND_K, HAND_TYPE, HAND_VALUE, HAND_RATE,
                                        HAND_MAXW, HAND_TARGETS)
    assert dc.tolist() == HAND_DOCS_OUT and sc.tolist() == HAND_SCORES_OUT
    assert rk.tolist() == HAND_RANK and ts.tolist() == HAND_TSCORE and stats.tolist() == HAND_STATS
    assert R.search(R.scores(HAND_QUERIES, HAND_DOCS, HAND_V), HAND_K)[1].tolist() == HAND_EXACT_DOCS
    # rescore on its own: unused slots, a doc given twice, a candidate that scores 0 (d3 for q1 would score; d0 does not)
    S = R.scores(HAND_QUERIES, HAND_DOCS, HAND_V)
    cand = np.array([[4, -1, 1, 1], [0, 5, 5, -1], [-1, -1, -1, -1], [1, 2, 3, 4]])
    sc, dc, rk, ts = R.rescore(S, cand, 3, [1, 5, 0, 2])
    assert dc.tolist() == [[1, 4, -1], [5, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    assert sc.tolist() == [[1.125, 0.40625, 0.0], [1.0, 0.0, 0.0], [0.0] * 3, [0.0] * 3]
    assert rk.tolist() == [1, 1, 0, 0] and ts.tolist() == [1.125, 1.0, 1.0, 0.0]


def test_reference_max_ratio_zero_is_exact_search():
    rng = np.random.default_rng(0)
    V, levels = 12, np.array([16, 32, 64]) / 64.0
    docs = [np.sort(rng.choice(V, int(rng.integers(1, 5)), replace=False)) for _ in range(60)]
    docs = [(t, rng.choice(levels, len(t))) for t in docs]
    queries = [(np.sort(rng.choice(V, 3, replace=False)), rng.choice(levels, 3)) for _ in range(8)]
    es, ed = R.search(R.scores(queries, docs, V), 10)
    for rate in (1.0, 2.5, 100.0):
        sc, dc, _, _, stats = R.two_phase(docs, queries, V, 10, "max_ratio", 0.0, rate, 10000)
        assert np.array_equal(dc, ed) and np.array_equal(sc.view(np.int32), es.view(np.int32))
        assert np.array_equal(stats[:, 0], stats[:, 1])                    # nothing was dropped


def test_two_phase_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes as C
    from snx import fn
    one = C.c_void_p(16)
    resc = fn("snx_sparse_rescore")
    # q_ptr q_term q_w nq cand_doc W doc_ptr doc_term doc_w nd target k out_doc out_score out_rank out_tscore stream
    args = [one, one, one, 4, one, 50, one, one, one, 100, one, 10, one, one, one, one, None]
    for i, v, rc in ((5, 0, -2), (5, 1025, -2), (11, 51, -2), (11, 0, -2), (3, -1, -2), (9, -1, -2), (12, None, -3),
                     (13, None, -3), (14, None, -3), (15, None, -3), (4, None, -3), (0, None, -3), (6, None, -3)):
        bad = list(args)
        bad[i] = v
        assert resc(*bad) == rc, (i, v)
    ok = list(args)
    ok[3] = 0                                                              # nothing to launch
    assert resc(*ok) == 0
    prune = fn("snx_sparse_prune_rows")
    need = fn("snx_sparse_prune_workspace_bytes")
    # ptr w n nnz max_row_nnz prune_type value keep kept_cnt workspace ws_bytes stream
    args = [one, one, 4, 100, 50, 0, 0.4, one, one, None, 0, None]
    for t, v in ((7, 0.4), (-1, 0.4), (0, -0.1), (0, float("nan")), (0, 1.5), (1, -1.0), (1, float("nan")), (2, 0.0),
                 (2, 2.5), (2, float("nan")), (3, 0.0), (3, 1.5), (3, -0.5), (3, float("nan"))):
        bad = list(args)
        bad[5], bad[6] = t, v
        assert prune(*bad) == -3, (t, v)
    for i, v, rc in ((2, -1, -2), (3, -1, -2), (4, -1, -2), (7, None, -3), (8, None, -3), (0, None, -3), (1, None, -3)):
        bad = list(args)
        bad[i] = v
        assert prune(*bad) == rc, (i, v)
    assert need(3, 10, 4096) == 0 and need(0, 10, 50000) == 0 and need(3, 0, 50000) == 0
    assert need(3, 10, 50000) == 10 * 65536 * 8 and need(3, 1000, 5000) == 128 * 8192 * 8
    long_rows = [one, one, 4, 100000, 50000, 3, 0.4, one, one, None, 0, None]  # alpha_mass needs its workspace
    assert prune(*long_rows) == -3
    long_rows[9], long_rows[10] = one, need(3, 4, 50000) - 1
    assert prune(*long_rows) == -3
    ok = list(args)
    ok[2] = 0
    assert prune(*ok) == 0


def test_window_arithmetic_and_host_validation():
    import torch
    from snx.retrieval import SparseIndex, prune_rows, two_phase_window
    assert two_phase_window(10, 5, 10000) == 50                            # the reference's settings at retrieval size 10
    assert two_phase_window(10, 5, 30) == 30 and two_phase_window(3, 2.5, 10000) == 7
    assert two_phase_window(10, 1, 10000) == 10 and two_phase_window(10, 102.4, 10000) == 1024
    for k, rate, cap in ((10, 0.5, 10000), (10, 5, 9), (10, 102.5, 10000), (10, 200, 10000), (0, 5, 10000),
                         (1025, 1, 10000), (10, float("nan"), 10000), (10, 0, 10000), (10, float("inf"), 10000)):
        with pytest.raises(ValueError):
            two_phase_window(k, rate, cap)                                 # never clamped
    idx = SparseIndex(16, "cpu")
    q = (torch.zeros(1, 1), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    for kw in ({"expansion_rate": 0.5}, {"expansion_rate": 200.0}, {"max_window_size": 5}, {"prune_type": "ratio"},
               {"prune_value": 1.5}, {"prune_value": float("nan")}, {"prune_type": "alpha_mass", "prune_value": 0.0},
               {"prune_type": "top_k", "prune_value": 2.5}, {"prune_type": "abs_value", "prune_value": -1.0}):
        with pytest.raises(ValueError):
            idx.search_two_phase(*q, 10, **kw)
    with pytest.raises(ValueError):
        idx.pruned("top_k", 0)
    rows = (torch.tensor([2]), torch.tensor([0, 1], dtype=torch.int32), torch.tensor([1.0, 0.5]))
    for ptype, value in (("max_ratio", -0.1), ("nope", 0.5), ("alpha_mass", 1.5), ("top_k", True), ("top_k", "3")):
        with pytest.raises(ValueError):
            prune_rows(*rows, ptype, value)
    with pytest.raises(ValueError):
        prune_rows(*rows, "max_ratio", 0.5)                                # the rows must live on a GPU


def test_two_phase_parameters_and_the_cli_grid():
    from src.train.cli.eval_pruning import parse_args, settings
    from src.train.eval import TWO_PHASE_DEFAULTS, two_phase_params
    assert TWO_PHASE_DEFAULTS == {"prune_type": "max_ratio", "prune_value": 0.4, "expansion_rate": 5.0,
                                  "max_window_size": 10000}
    assert two_phase_params({"expansion_rate": 2.0}) == dict(TWO_PHASE_DEFAULTS, expansion_rate=2.0)
    with pytest.raises(ValueError):
        two_phase_params({"prune_ratio": 0.4})
    assert settings(parse_args([])) == [(("max_ratio", 0.4, 5.0), None)]
    assert settings(parse_args(["--prune-ratio", "0.2", "--expansion-rate", "3"])) == [(("max_ratio", 0.2, 3.0), None)]
    grid = settings(parse_args(["--sweep"]))
    exact = ("max_ratio", 0.0, 1.0)
    want = [(("max_ratio", r, 5.0), None) for r in (0.1, 0.2, 0.4, 0.6, 0.8)] + \
           [(("max_ratio", 0.4, e), None) for e in (1.0, 2.0, 5.0, 10.0, 20.0)] + \
           [(exact, ("max_ratio", v)) for v in (0.05, 0.1, 0.2)] + [(exact, ("top_k", v)) for v in (32, 64, 128)] + \
           [(exact, ("alpha_mass", v)) for v in (0.8, 0.9, 0.95)]
    assert grid == want and len(grid) == 19
    for bad in (["--prune-ratio", "1.5"], ["--expansion-rate", "0"], ["--max-window-size", "0"], ["--prune-ratio", "x"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_evaluator_keys_are_unchanged_without_two_phase(monkeypatch):
    """two_phase=None leaves evaluate()'s dict as it was, key for key; with the option and no GPU result (no queries to
    search) the two_phase_* keys are present and 0.0, as for SEISMIC."""
    from src.train.data.collator import create_tokenizer
    from src.train.eval import MidTrainingEvaluator
    plain_keys = ["recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10", "num_queries", "num_docs", "avg_nnz_q",
                  "avg_nnz_d"]
    tp_keys = [f"two_phase_{k}" for k in ("recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10", "overlap@5",
                                          "postings_frac")]
    tok = create_tokenizer("hash:1000")
    monkeypatch.setattr(MidTrainingEvaluator, "encode", lambda self, model: (None, None))
    kw = dict(tokenizer=tok, val_file="synthetic:20:2", max_queries=5, max_docs=12, device="cpu")
    assert list(MidTrainingEvaluator(**kw).evaluate(None)) == plain_keys
    assert list(MidTrainingEvaluator(**kw, two_phase=None).evaluate(None)) == plain_keys
    out = MidTrainingEvaluator(**kw, two_phase={}).evaluate(None)
    assert list(out) == plain_keys + tp_keys and all(out[k] == 0.0 for k in tp_keys)
    both = MidTrainingEvaluator(**kw, seismic={}, two_phase={"prune_value": 0.2}).evaluate(None)
    assert list(both)[:9] == plain_keys and set(tp_keys) < set(both) and len(both) == 9 + 7 + 7
    with pytest.raises(ValueError):
        MidTrainingEvaluator(**kw, two_phase={"ratio": 0.4})

"""CPU checks of SEISMIC (include/snx.h "SEISMIC"): a hand-worked example pins the numpy reference
(tests/seismic_reference.py) that the GPU suite (test_gpu_seismic.py) holds csrc/seismic.hip to, the C ABI's argument
checks, and the grid of the CLI src.train.cli.eval_seismic."""
import numpy as np
import pytest

from tests import seismic_reference as R

# V = 5 terms; dyadic weights, so every score below is exact
HAND_DOCS = [([0, 1], [1.0, 0.5]),
             ([0, 2], [0.5, 1.0]),
             ([0, 1, 3], [2.0, 0.25, 0.5]),
             ([1, 2], [1.0, 0.5]),
             ([0, 3], [1.0, 1.0]),
             ([2, 4], [0.25, 0.5])]
HAND_V, HAND_NP, HAND_R, HAND_ALPHA = 5, 3, 0.5, 0.75
HAND_QUERIES = [([1, 2, 3], [1.0, 0.5, 0.25]), ([0, 4], [0.5, 1.0]), ([], [])]
HAND_TARGETS = [1, 2, 0]
HAND_K, HAND_TOP_N, HAND_HF = 2, 2, 0.5

# Worked by hand.  t0: list d0 1, d1 .5, d2 2, d4 1 -> P = d2, d0, d4 (n_postings 3); c = ceil(1.5) = 2, centroids at
# positions 0, 1: d2, d0; s(d0, d2) = 2.125 > s(d0, d0) = 1.25, s(d4, d2) = 2.5 > 1: all three join d2, so centroid d0's
# block is empty and dropped.  t1: P = d3, d0, d2; centroids d3, d0; d0 and d2 prefer d0, d3 itself.  t2: P = d1, d3, d5;
# centroids d1, d3.  t3: P = d4, d2, one centroid.  t4: d5 alone.  Summaries (alpha .75): t0's block {0: 2, 3: 1, 1: .5},
# total 3.5, goal 2.625 -> 2 + 1 reaches it: {0: 2, 3: 1}; and so on.
HAND_STRUCT = {
    "prune_ptr": [0, 3, 6, 9, 11, 12],
    "prune_doc": [0, 2, 4, 0, 2, 3, 1, 3, 5, 2, 4, 5],
    "prune_w": [1, 2, 1, .5, .25, 1, 1, .5, .25, .5, 1, .5],
    "cent_ptr": [0, 2, 4, 6, 7, 8],
    "cent_doc": [2, 0, 3, 0, 1, 3, 4, 5],
    "term_blk_ptr": [0, 1, 3, 5, 6, 7],
    "blk_cent": [0, 0, 1, 0, 1, 0, 0],
    "blk_ptr": [0, 3, 4, 6, 8, 9, 11, 12],
    "blk_doc": [0, 2, 4, 3, 0, 2, 1, 5, 3, 2, 4, 5],
    "sum_ptr": [0, 2, 4, 6, 8, 10, 12, 14],
    "sum_term": [0, 3, 1, 2, 0, 1, 0, 2, 1, 2, 0, 3, 2, 4],
    "sum_w": [2, 1, 1, .5, 2, .5, .5, 1, 1, .5, 2, 1, .25, .5],
}
# q0 (k 2, top_n 2: terms 1 then 2, hf .5): block t1/d3 (summary score 1.25) scores d3 1.25; t1/{d0, d2} (.5) while H is
# not full: d0 .5, d2 .375 -> H = d3, d0, s_k = .5; t2/{d1, d5}: .5 * .5 < .5, skipped; t2/d3: .5 * 1.25 >= .5, scored,
# d3 already held.  q1 (terms 4 then 0): t4/d5 -> d5 .5; t0/{d0, d2, d4} (H not full): d2 1, then d0, d4, d5 tie at .5 ->
# d0 (lowest id).  q2 is empty.
HAND_DOCS_OUT = [[3, 0], [2, 0], [-1, -1]]
HAND_SCORES_OUT = [[1.25, 0.5], [1.0, 0.5], [0.0, 0.0]]
HAND_RANK = [0, 1, 0]
HAND_TSCORE = [0.5, 1.0, 0.0]
HAND_STATS = [[4, 3, 4], [2, 2, 4], [0, 0, 0]]


def test_reference_reproduces_the_hand_worked_example():
    st = R.build(HAND_DOCS, HAND_V, HAND_NP, HAND_R, HAND_ALPHA)
    for key, want in HAND_STRUCT.items():
        assert st[key].tolist() == want, key
    sc, dc, rk, ts, stats = R.search(st, HAND_DOCS, HAND_QUERIES, HAND_K, HAND_TOP_N, HAND_HF, HAND_TARGETS)
    assert dc.tolist() == HAND_DOCS_OUT and sc.tolist() == HAND_SCORES_OUT
    assert rk.tolist() == HAND_RANK and ts.tolist() == HAND_TSCORE and stats.tolist() == HAND_STATS


def test_reference_degenerate_setting_is_exact_search():
    rng = np.random.default_rng(0)
    V, levels = 12, np.array([16, 32, 64]) / 64.0
    docs = [(np.sort(rng.choice(V, int(rng.integers(1, 5)), replace=False)), None) for _ in range(60)]
    docs = [(t, rng.choice(levels, len(t))) for t, _ in docs]
    queries = [(np.sort(rng.choice(V, 3, replace=False)), rng.choice(levels, 3)) for _ in range(8)]
    st = R.build(docs, V, 10 ** 6, 0.3, 0.4)
    sc, dc, _, _, stats = R.search(st, docs, queries, 10, 100, np.inf)
    D = np.array([[sum(w1 * w2 for t1, w1 in zip(*q) for t2, w2 in zip(*d) if t1 == t2) for d in docs] for q in queries])
    for q in range(len(queries)):
        order = np.lexsort((np.arange(len(docs)), -D[q]))
        order = order[D[q, order] > 0][:10]
        assert dc[q, :len(order)].tolist() == order.tolist() and (dc[q, len(order):] == -1).all()
        assert stats[q, 0] == stats[q, 1]                          # hf = inf skips nothing


def test_seismic_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes as C
    from snx import fn
    one = C.c_void_p(16)
    srch = fn("snx_seismic_search")
    # q_ptr q_term q_w nq max_nnz term_blk_ptr blk_ptr blk_doc sum_ptr sum_term sum_w doc_ptr doc_term doc_w nd V target
    # k top_n hf out_doc out_score out_rank out_tscore out_stats stream
    args = [one, one, one, 4, 64, one, one, one, one, one, one, one, one, one, 100, 50, one, 10, 10, 1.0, one, one, one,
            one, one, None]
    for i, v, rc in ((17, 0, -2), (17, 1025, -2), (18, 0, -2), (4, 1025, -2), (4, -1, -2), (19, 0.0, -2),
                     (19, -1.0, -2), (19, float("nan"), -2), (3, -1, -2), (0, None, -3), (5, None, -3), (24, None, -3),
                     (22, None, -3), (23, None, -3), (20, None, -3)):
        bad = list(args)
        bad[i] = v
        assert srch(*bad) == rc, (i, v)
    ok = list(args)
    ok[3], ok[19] = 0, float("inf")                                # nothing to launch; +inf is a valid heap factor
    assert srch(*ok) == 0
    summ = fn("snx_seismic_build_summaries")
    # doc_ptr doc_term doc_w nd V blk_ptr blk_doc nblocks alpha sum_ptr sum_cnt sum_term sum_w ws ws_bytes stream
    need = fn("snx_seismic_build_workspace_bytes")(50, 10)
    assert need > 0 and fn("snx_seismic_build_workspace_bytes")(50, 0) == 0
    args = [one, one, one, 100, 50, one, one, 10, 0.4, None, one, None, None, one, need, None]
    for i, v, rc in ((8, 0.0, -2), (8, 1.5, -2), (8, float("nan"), -2), (7, -1, -2), (14, need - 1, -3),
                     (13, None, -3), (10, None, -3), (0, None, -3)):
        bad = list(args)
        bad[i] = v
        assert summ(*bad) == rc, (i, v)
    bad = list(args)
    bad[9] = one                                                   # the fill pass needs sum_term / sum_w
    assert summ(*bad) == -3
    clus = fn("snx_seismic_build_clusters")
    # term_ptr post_doc post_w doc_ptr doc_term doc_w nd V n_postings prune_ptr cent_cnt cent_ptr npruned ncent
    # prune_doc prune_w cent_doc assign cent_size stream
    args = [one] * 6 + [100, 50, 300, one, one, one, 40, 10] + [one] * 5 + [None]
    for i, v, rc in ((8, 0, -2), (13, 41, -2), (7, 0, -2), (14, None, -3), (18, None, -3), (0, None, -3)):
        bad = list(args)
        bad[i] = v
        assert clus(*bad) == rc, (i, v)
    blocks = fn("snx_seismic_build_blocks")
    assert blocks(one, one, one, one, 50, 40, None, one, None) == -3
    assert blocks(one, one, one, one, 0, 40, one, one, None) == -2


def test_seismic_index_validates_on_the_host():
    from snx.retrieval import SeismicIndex, SparseIndex
    idx = SparseIndex(16, "cpu")
    with pytest.raises(ValueError):
        SeismicIndex(idx)                                          # not built
    with pytest.raises(ValueError):
        SeismicIndex("index")


def test_cli_reference_sweep_grid_matches_the_reference_order():
    from src.train.cli.eval_seismic import parse_args, settings
    flat = [(i, q) for i, qs in settings(parse_args(["--reference-sweep"])) for q in qs]
    want_index = [(n, 0.1, 0.4) for n in (10, 50, 100, 300, 500, 1000)] + \
                 [(300, r, 0.4) for r in (0.01, 0.05, 0.2, 0.5)] + [(300, 0.1, a) for a in (0.1, 0.2, 0.6, 0.8)]
    want = [(i, (10, 1.0)) for i in want_index] + \
           [((300, 0.1, 0.4), q) for q in [(10, 1.0), (10, 0.5), (10, 1.0), (10, 2.0), (5, 1.0), (10, 1.0), (20, 1.0)]]
    assert flat == want and len(flat) == 21
    groups = settings(parse_args(["--n-postings", "10,20", "--cluster-ratio", "0.1", "--top-n", "5,10",
                                  "--heap-factor", "1,2"]))
    assert [g[0] for g in groups] == [(10, 0.1, 0.4), (20, 0.1, 0.4)]
    assert groups[0][1] == [(5, 1.0), (5, 2.0), (10, 1.0), (10, 2.0)]
    for bad in (["--n-postings", "0"], ["--cluster-ratio", "0"], ["--summary-prune-ratio", "1.5"],
                ["--heap-factor", "0"], ["--top-n", "x"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_overlap_and_seismic_parameters():
    from src.train.eval import overlap_at, seismic_params
    assert overlap_at([[1, 2, 3, 4, 5]], [[5, 6, 7, 8, 9]]) == 0.2
    assert overlap_at([[1, -1, -1, -1, -1], [3, 4, -1, -1, -1]], [[-1] * 5, [4, 9, -1, -1, -1]]) == 0.25
    assert seismic_params({"top_n": 5})["n_postings"] == 300
    with pytest.raises(ValueError):
        seismic_params({"k": 3})

"""CPU checks of the exact dense retrieval (include/snx.h "exact dense retrieval"): hand-worked cases pin the numpy
reference tests/dense_reference.py, and the teacher pipeline (src.train.mining.dense) runs on the numpy stand-in index --
the score writer against the reference project's own output (tests/golden/g15_teacher_scores.json, written by
tools/make_golden_dense.py), the miner against hand-built expectations."""
import json
import os
import re

import numpy as np
import pytest

from tests import dense_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "g15_teacher_scores.json")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the reference by hand
def test_chain_is_the_float64_matmul_for_dyadic_values_at_d_1024():
    rng = np.random.default_rng(0)
    Q = (rng.integers(-8, 9, size=(7, 1024)) / 8).astype(np.float32)
    E = (rng.integers(-8, 9, size=(33, 1024)) / 8).astype(np.float32)
    assert np.array_equal(_bits(R.chain_scores(Q, E)), _bits(R.exact_scores(Q, E)))
    # and it is a chain, not a sum in another order: 2^24 + 1 - 2^24 is 0 from the left and 1 in exact arithmetic
    Q1 = np.array([[1.0, 1.0, 1.0]], np.float32)
    E1 = np.array([[2.0 ** 24, 1.0, -(2.0 ** 24)]], np.float32)
    assert R.chain_scores(Q1, E1)[0, 0] == 0.0 and (Q1.astype(np.float64) @ E1.astype(np.float64).T)[0, 0] == 1.0


def test_order_ties_negative_scores_and_k_beyond_nd():
    # scores of the one query: [0.5, -1, 0.5, -0.25, 0.5]
    E = np.array([[0.5], [-1.0], [0.5], [-0.25], [0.5]], np.float32)
    Q = np.array([[1.0]], np.float32)
    S = R.chain_scores(Q, E)
    sc, dc, rk, ts = R.search(S, 7, targets=[4])
    assert dc.tolist() == [[0, 2, 4, 3, 1, -1, -1]]
    assert sc.tolist() == [[0.5, 0.5, 0.5, -0.25, -1.0, 0.0, 0.0]]
    assert rk.tolist() == [3] and ts.tolist() == [0.5]            # two equal scores with lower ids in front
    assert R.search(S, 2, targets=[1])[2].tolist() == [5]           # the rank does not stop at k
    # all scores negative: still a full ranking, best (closest to zero) first
    sc, dc, _, _ = R.search(R.chain_scores(-Q, np.abs(E)), 3)
    assert dc.tolist() == [[3, 0, 2]] and sc.tolist() == [[-0.25, -0.5, -0.5]]


def test_negative_underflow_reads_plus_zero_and_ranks_among_the_zeros():
    E = np.array([[0.0], [-(2.0 ** -100)], [0.0], [2.0 ** -40]], np.float32)
    Q = np.array([[2.0 ** -100]], np.float32)
    S = R.chain_scores(Q, E)
    assert _bits(S).tolist() == [[0, 0, 0, _bits(np.float32(2.0 ** -140))[()]]]     # -0 became +0; a subnormal stays
    sc, dc, rk, _ = R.search(S, 4, targets=[1])
    assert dc.tolist() == [[3, 0, 1, 2]] and rk.tolist() == [3]


def test_band_with_exclusion_and_ceiling():
    E = np.array([[0.5], [-1.0], [0.5], [-0.25], [0.75], [0.25]], np.float32)
    S = R.chain_scores(np.array([[1.0], [1.0], [1.0], [1.0]], np.float32), E)
    # order of all docs: 4 (0.75), 0, 2 (0.5), 5 (0.25), 3 (-0.25), 1 (-1)
    sc, dc, fd = R.search_band(S, 1, 4, exclude=[[], [0, 4], list(range(6)), []],
                               ceiling=[np.inf, np.inf, np.inf, 0.5])
    assert dc.tolist() == [[0, 2, 5], [5, 3, 1], [-1, -1, -1], [3, 1, -1]]       # 0.5 itself is not below the ceiling 0.5
    assert fd.tolist() == [3, 3, 0, 2]
    assert sc.tolist() == [[0.5, 0.5, 0.25], [0.25, -0.25, -1.0], [0.0, 0.0, 0.0], [-0.25, -1.0, 0.0]]
    assert R.search_band(S, 0, 2, ceiling=[-np.inf, np.nan, np.inf, 0.75])[2].tolist() == [0, 0, 2, 2]


# ------------------------------------------------------------------------------------------------ header, ABI, CLI
def test_header_and_ctypes_table_name_the_dense_entry_points():
    from snx._lib import SIGNATURES
    text = open(os.path.join(ROOT, "include", "snx.h")).read()
    names = ["snx_dense_search_workspace_bytes", "snx_dense_search", "snx_dense_search_band_workspace_bytes",
             "snx_dense_search_band", "snx_dense_pair_scores"]
    for n in names:
        assert re.search(r"\b%s\(" % n, text) and n in SIGNATURES, n
    import snx
    assert not [n for n in snx.verify_exports() if n in names]
    from snx import asmcheck
    assert set(asmcheck.GUARDED["dense.hip"]) == {"dn_search_kernel", "dn_merge_kernel"}


def test_workspace_grows_with_queries_times_k_not_with_docs():
    from snx import fn
    size = fn("snx_dense_search_workspace_bytes")
    band = fn("snx_dense_search_band_workspace_bytes")
    big = size(4096, 1 << 22, 100, 0)
    assert 0 < big < 4096 * (1 << 22) * 4 // 50                   # far below the [nq, nd] fp32 matrix
    assert size(4096, 1 << 24, 100, 0) == big                      # more docs: the default split count is capped
    assert size(8192, 1 << 22, 100, 0) <= 2 * big + 4096
    assert band(4096, 1 << 22, 100, 0) == big
    for bad in ((0, 10, 10, 0), (10, -1, 10, 0), (10, 10, 0, 0), (10, 10, 1025, 0), (10, 10, 10, 127), (10, 10, 10, -1)):
        assert size(*bad) == 0 and band(*bad) == 0


def test_shape_errors_come_from_the_host():
    import ctypes as C
    from snx import fn
    buf = (C.c_float * 64)()
    ibuf = (C.c_int32 * 64)()
    p, ip = C.cast(buf, C.c_void_p), C.cast(ibuf, C.c_void_p)
    search, band, pairs = fn("snx_dense_search"), fn("snx_dense_search_band"), fn("snx_dense_pair_scores")
    for D, k, chunk in ((0, 1, 0), (4097, 1, 0), (8, 0, 0), (8, 1025, 0), (8, 1, 64), (8, 1, -1)):
        assert search(p, 2, p, 2, D, None, k, chunk, ip, p, None, None, p, 1 << 20, None) == -2, (D, k, chunk)
    for lo, hi in ((-1, 1), (3, 3), (0, 1025)):
        assert band(p, 2, p, 2, 8, None, None, None, lo, hi, 0, ip, p, ip, p, 1 << 20, None) == -2
    assert search(p, 2, p, 2, 8, None, 1, 0, None, p, None, None, p, 1 << 20, None) == -3          # no out_doc
    assert search(p, 2, p, 2, 8, ip, 1, 0, ip, p, None, None, p, 1 << 20, None) == -3             # target without out_rank
    assert search(p, 2, p, 2, 8, None, 1, 0, ip, p, None, None, p, 16, None) == -3                # workspace too small
    assert band(p, 2, p, 2, 8, ip, None, None, 0, 1, 0, ip, p, ip, p, 1 << 20, None) == -3         # ex_ptr without ex_doc
    assert pairs(p, 2, p, 2, 0, ip, ip, 1, p, None) == -2 and pairs(p, 2, p, 2, 8, None, ip, 1, p, None) == -3
    assert search(p, 0, p, 2, 8, None, 1, 0, ip, p, None, None, None, 0, None) == 0                # no queries: nothing to do
    assert pairs(p, 2, p, 2, 8, ip, ip, 0, p, None) == 0


def test_dense_index_validates_dim_without_a_gpu():
    from snx.retrieval import DenseIndex
    for dim in (0, 4097, -3, 1.5, True, "8"):
        with pytest.raises(ValueError):
            DenseIndex(dim, "cpu")
    idx = DenseIndex(4096, "cpu")
    with pytest.raises(RuntimeError):
        idx.search(None, 1)


def test_cli_arguments():
    from src.train.cli import eval_hybrid, teacher_scores
    a = teacher_scores.parse_args(["mine", "--embeddings", "e.npy", "--text-index", "t.json"])
    assert (a.k, a.rank_start, a.rank_end, a.sample) == (7, 10, 50, "first")
    a = teacher_scores.parse_args(["score", "--embeddings", "e.npy", "--text-index", "t.json"])
    assert a.command == "score" and a.output_dir == "data/v29.0_kd"
    for bad in (["mine", "--embeddings", "e", "--text-index", "t", "--rank-start", "50"], ["score"], []):
        with pytest.raises(SystemExit):
            teacher_scores.parse_args(bad)
    with pytest.raises(SystemExit):
        eval_hybrid.parse_args(["--dense-run", "a.npz", "--dense-embeddings", "b.npz"])
    a = eval_hybrid.parse_args(["--dense-embeddings", "b.npz"])
    assert [r[0] for r in eval_hybrid.rows(a)][-4:] == ["dense", "bm25_dense_rrf", "dense_sparse_rrf", "triple_rrf"]


# ------------------------------------------------------------------------------------------------ the score writer
def golden_cache(tmp_path):
    """The golden's cache and shards as files -> (golden, embeddings .npy path, text index path, input dir)."""
    from src.train.mining.dense import text_hash
    g = json.load(open(GOLDEN, encoding="utf-8"))
    emb = (np.asarray(g["embeddings_times_8"], np.float64) / 8).astype(np.float32)
    np.save(tmp_path / "embeddings.npy", emb)                   # written by the test, not committed
    (tmp_path / "text_index.json").write_text(json.dumps({text_hash(t): i for i, t in enumerate(g["texts"])}))
    src = tmp_path / "in"
    src.mkdir()
    for name, lines in g["shards"].items():
        (src / name).write_text("".join(x + "\n" for x in lines), encoding="utf-8")
    return g, str(tmp_path / "embeddings.npy"), str(tmp_path / "text_index.json"), src


def test_score_writer_reproduces_the_reference_files(tmp_path):
    from src.train.mining.dense import load_teacher_cache, write_teacher_scores
    g, npy, tix, src = golden_cache(tmp_path)
    emb, text_to_idx = load_teacher_cache(npy, tix)
    assert emb.shape == (len(g["texts"]), g["dim"]) and len(text_to_idx) == len(g["texts"])
    files = sorted(str(p) for p in src.iterdir())
    total = write_teacher_scores(files, str(tmp_path / "out"), emb, text_to_idx, R.NumpyDenseIndex(g["dim"]))
    assert total == g["total"] == 8
    for name, want in g["expected"].items():
        assert (tmp_path / "out" / name).read_text(encoding="utf-8").splitlines() == want, name
    # the unscored records of the golden are there unchanged, the line that is no JSON is gone
    assert sum(len(v) for v in g["expected"].values()) == 10
    assert sum("teacher_pos_score" not in json.loads(x) for v in g["expected"].values() for x in v) == 2


def test_score_writer_extension_scores_a_negatives_list(tmp_path):
    from src.train.mining.dense import text_hash, write_teacher_scores
    texts = ["q", "p", "n0", "n1"]
    emb = np.array([[1, 0.5], [0.5, 0.25], [-1, 0], [0.125, 1]], np.float32)
    tix = {text_hash(t): i for i, t in enumerate(texts)}
    f = tmp_path / "train_0.jsonl"
    f.write_text(json.dumps({"query": "q", "positive": "p", "negatives": ["n1", "unknown", "n0"]}) + "\n")
    assert write_teacher_scores([str(f)], str(tmp_path / "out"), emb, tix, R.NumpyDenseIndex(2)) == 1
    assert json.loads((tmp_path / "out" / "train_0.jsonl").read_text()) == {
        "query": "q", "positive": "p", "negatives": ["n1", "unknown", "n0"], "teacher_pos_score": 0.625,
        "teacher_neg_score": 0.0, "teacher_neg_scores": [0.625, 0.0, -1.0]}


# ------------------------------------------------------------------------------------------------ the miner
MINE_TEXTS = {"qa": [1, 0], "qb": [0, 1], "qd": [1, 1], "P0": [1, 1], "N0": [0.5, -0.5], "P1": [0.875, 0],
              "N1": [0.25, 0.25], "N2": [0.5, 0.75], "P2": [-1, -1]}                       # qc and N3: not in the cache
MINE_RECORDS = [{"query": "qa", "positive": "P0", "negative": "N0"},
                {"query": "qa", "positive": "P1", "negative": "N1", "source": "s", "teacher_pos_score": 0.5},
                {"query": "qb", "positive": "P0", "negative": "N2"},
                {"query": "qc", "positive": "P1", "negative": "N0"},
                {"query": "qd", "positive": "P2", "negative": "N3"}]


def mine_case(tmp_path):
    from src.train.mining.dense import text_hash
    names = sorted(MINE_TEXTS, reverse=True)                     # cache order differs from corpus order
    emb = np.array([MINE_TEXTS[n] for n in names], np.float32)
    tix = {text_hash(n): i for i, n in enumerate(names)}
    src = tmp_path / "in"
    src.mkdir(parents=True, exist_ok=True)
    (src / "train_0.jsonl").write_text("".join(json.dumps(r) + "\n" for r in MINE_RECORDS[:3]))
    (src / "train_1.jsonl").write_text("".join(json.dumps(r) + "\n" for r in MINE_RECORDS[3:]))
    return emb, tix, sorted(str(p) for p in src.iterdir())


def _mined(tmp_path, name, **kw):
    from src.train.mining.dense import mine_dense_negatives
    emb, tix, files = mine_case(tmp_path)
    summary = mine_dense_negatives(files, str(tmp_path / name), emb, tix, R.NumpyDenseIndex(2), k=2, **kw)
    out = [json.loads(x) for f in ("train_0.jsonl", "train_1.jsonl") for x in open(tmp_path / name / f)]
    return summary, out


def test_miner_full_bands_and_a_query_without_embedding(tmp_path):
    # corpus docs: P0 N0 P1 N1 N2 P2 (N3 has no embedding).  qa scores the first component, its positives P0 and P1 leave
    # before ranking: N0 .5, N2 .5, N1 .25, P2 -1 -> ranks [1, 3) = N2, N1.  qb scores the second, P0 leaves: N2 .75,
    # N1 .25, P1 0, N0 -.5, P2 -1 -> N1, P1.  qd sums both, P2 leaves: P0 2, N2 1.25, P1 .875, N1 .5, N0 0 -> N2, P1.
    summary, out = _mined(tmp_path, "a", rank_start=1, rank_end=3)
    assert out == [
        {"query": "qa", "positive": "P0", "negatives": ["N2", "N1"], "teacher_pos_score": 1.0,
         "teacher_neg_scores": [0.5, 0.25]},
        {"query": "qa", "positive": "P1", "negatives": ["N2", "N1"], "teacher_pos_score": 0.875,
         "teacher_neg_scores": [0.5, 0.25], "source": "s"},
        {"query": "qb", "positive": "P0", "negatives": ["N1", "P1"], "teacher_pos_score": 1.0,
         "teacher_neg_scores": [0.25, 0.0]},
        MINE_RECORDS[3],                                         # qc is not in the cache: unchanged
        {"query": "qd", "positive": "P2", "negatives": ["N2", "P1"], "teacher_pos_score": -2.0,
         "teacher_neg_scores": [1.25, 0.875]}]
    assert summary == {"records": 5, "queries": 4, "docs": 7, "indexed_docs": 6, "band_fill": 1.0, "padded": 0,
                       "fallback": 0, "unchanged": 1}
    assert list(out[1]) == ["query", "positive", "negatives", "teacher_pos_score", "teacher_neg_scores", "source"]


def test_miner_pads_a_short_band(tmp_path):
    # ranks [3, 5): qa has four admissible docs -> P2 alone, repeated; qb and qd have five -> N0, P2 and N1, N0
    summary, out = _mined(tmp_path, "b", rank_start=3, rank_end=5)
    assert (out[0]["negatives"], out[0]["teacher_neg_scores"]) == (["P2", "P2"], [-1.0, -1.0])
    assert (out[1]["negatives"], out[1]["teacher_neg_scores"]) == (["P2", "P2"], [-1.0, -1.0])
    assert (out[2]["negatives"], out[2]["teacher_neg_scores"]) == (["N0", "P2"], [-0.5, -1.0])
    assert (out[4]["negatives"], out[4]["teacher_neg_scores"]) == (["N1", "N0"], [0.5, 0.0])
    assert summary["padded"] == 2 and summary["fallback"] == 0 and summary["unchanged"] == 1
    assert summary["band_fill"] == 5 / 6


def test_miner_falls_back_on_an_empty_band(tmp_path):
    # ranks [5, 6): every band is empty -> the record's own negative, scored by the teacher (0.0 without an embedding)
    summary, out = _mined(tmp_path, "c", rank_start=5, rank_end=6)
    assert (out[0]["negatives"], out[0]["teacher_neg_scores"]) == (["N0", "N0"], [0.5, 0.5])
    assert (out[1]["negatives"], out[1]["teacher_neg_scores"]) == (["N1", "N1"], [0.25, 0.25])
    assert (out[2]["negatives"], out[2]["teacher_neg_scores"]) == (["N2", "N2"], [0.75, 0.75])
    assert out[3] == MINE_RECORDS[3]
    assert (out[4]["negatives"], out[4]["teacher_neg_scores"]) == (["N3", "N3"], [0.0, 0.0])
    assert summary["fallback"] == 4 and summary["padded"] == 0 and summary["band_fill"] == 0.0
    with pytest.raises(ValueError):
        _mined(tmp_path, "d", rank_start=5, rank_end=5)

"""GPU checks of the exact dense retrieval (csrc/dense.hip, include/snx.h "exact dense retrieval"): snx.retrieval.DenseIndex,
the teacher pipeline on it (src.train.mining.dense) and the dense rows of src.train.cli.eval_hybrid.

Everything is compared exactly -- int32 ids and fp32 BITS -- against tests/dense_reference.py.  The dyadic cases (integers
in [-8, 8] divided by 8) make every partial sum of the score chain exact, so the reference is the ABI's chain bit for bit
there; the non-dyadic case checks the MFMA chain against the serial chain of pair_scores (bit for bit) and against a
float64 dot under the first-order bound of a length-D fp32 chain."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dense_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 128                             # query rows of a workgroup, and docs of the smallest chunk


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _dyadic(rng, n, D):
    return (rng.integers(-8, 9, size=(n, D)) / 8.0).astype(np.float32)


def _index(E, dev):
    from snx.retrieval import DenseIndex
    idx = DenseIndex(E.shape[1], dev)
    half = E.shape[0] // 2                                   # two batches: doc ids are the order of addition
    if half:
        idx.add(torch.from_numpy(E[:half]).to(dev))
    idx.add(torch.from_numpy(E[half:]).to(dev))
    return idx.build()


def _same_search(got, want):
    sc, dc, rk, ts = got
    rs, rd, rr, rt = want
    assert np.array_equal(dc.cpu().numpy(), rd)
    assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs))
    if rr is not None:
        assert np.array_equal(rk.cpu().numpy(), rr)
        assert np.array_equal(_bits(ts.cpu().numpy()), _bits(rt))


# ------------------------------------------------------------------------------------------------ 1. exact sweep
# (D, nd, nq, k, chunk_docs): D ragged against the K tile (16) and the 16-byte loads; nd around one chunk of 128 and three
# chunks plus a tail; nq around the query tile; k > nd; splits of many tiles, where the running threshold and the list
# compaction do the work (k = 100: lists of 512 compact from the fourth tile on; k = 1024: lists of 2048 from the 16th)
SWEEP = [
    (1, 1, 1, 1, 0),
    (2, 31, TILE - 1, 10, 0),
    (33, 33, TILE + 1, 100, 0),
    (64, TILE - 1, 1, 1024, TILE),
    (384, TILE + 1, TILE - 1, 10, TILE),
    (1024, 3 * TILE + 37, TILE + 1, 100, TILE),
    (33, 3 * TILE + 37, 1, 1024, TILE),
    (64, 5000, TILE + 1, 100, 2560),
    (2, 5000, TILE - 1, 1024, 5000),
    (1, 4000, 3, 10, 0),
    (1024, 1500, 300, 10, 640),
    (384, 5000, 2, 1, 0),
]


@pytest.mark.parametrize("D,nd,nq,k,chunk", SWEEP)
def test_exact_sweep_dyadic(dev, D, nd, nq, k, chunk):
    rng = np.random.default_rng(1000 * D + nd + nq + k)
    E, Q = _dyadic(rng, nd, D), _dyadic(rng, nq, D)
    S = R.exact_scores(Q, E)
    targets = rng.integers(0, nd, size=nq)
    idx = _index(E, dev)
    got = idx.search(torch.from_numpy(Q).to(dev), k, targets=torch.from_numpy(targets).to(dev), chunk_docs=chunk)
    _same_search(got, R.search(S, k, targets))
    assert int(got[2].min()) >= 1                            # a valid target always has a rank


# ------------------------------------------------------------------------------------------------ 2. tie order
@pytest.mark.parametrize("chunk", [0, 3000])
def test_thousands_of_ties_resolve_by_doc_id(dev, chunk):
    rng = np.random.default_rng(2)
    E = rng.integers(-1, 2, size=(3000, 4)).astype(np.float32)
    Q = rng.integers(-1, 2, size=(40, 4)).astype(np.float32)
    S = R.exact_scores(Q, E)
    assert len(np.unique(S)) <= 9
    targets = rng.integers(0, 3000, size=40)
    idx = _index(E, dev)
    got = idx.search(torch.from_numpy(Q).to(dev), 1024, targets=torch.from_numpy(targets).to(dev), chunk_docs=chunk)
    _same_search(got, R.search(S, 1024, targets))


# ------------------------------------------------------------------------------------------------ 3. invariance
def test_chunking_and_query_slicing_change_no_bit(dev):
    rng = np.random.default_rng(3)
    E = rng.standard_normal((2500, 200)).astype(np.float32)
    Q = rng.standard_normal((150, 200)).astype(np.float32)
    idx = _index(E, dev)
    q = torch.from_numpy(Q).to(dev)
    t = torch.from_numpy(rng.integers(0, 2500, size=150)).to(dev)
    base = idx.search(q, 100, targets=t)
    for kw in ({"chunk_docs": TILE}, {"query_slice": 50}, {"chunk_docs": 1000, "query_slice": 1}):
        other = idx.search(q, 100, targets=t, **kw)
        for a, b in zip(base, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), kw
    band = idx.search_band(q, 10, 50, exclude=[[int(x)] for x in t.tolist()])
    other = idx.search_band(q, 10, 50, exclude=[[int(x)] for x in t.tolist()], chunk_docs=TILE, query_slice=64)
    for a, b in zip(band, other):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # nor does the alignment of the operands: D % 4 == 0 with both bases one float off a 16-byte boundary
    from snx.retrieval import DenseIndex
    D, nd, nq, k = 20, 300, 130, 10
    E = rng.standard_normal((nd, D)).astype(np.float32)
    Q = rng.standard_normal((nq, D)).astype(np.float32)
    e, q = torch.from_numpy(E).to(dev), torch.from_numpy(Q).to(dev)
    e1, q1 = _one_float_off(e), _one_float_off(q)
    t = torch.from_numpy(rng.integers(0, nd, size=nq)).to(dev)
    excl = [rng.choice(nd, size=40, replace=False).tolist() for _ in range(nq)]
    results = []
    for emb, qq in ((e, q), (e1, q1)):
        idx = DenseIndex(D, dev)
        idx.add(emb)                                         # one batch: build() keeps the tensor, and so its base
        idx.build()
        assert idx.emb.data_ptr() == emb.data_ptr()
        results.append(list(idx.search(qq, k, targets=t)) + list(idx.search_band(qq, 2, k, exclude=excl)))
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _one_float_off(x):
    """The same values in a contiguous view that starts one float into a larger buffer."""
    flat = torch.empty(x.numel() + 8, dtype=x.dtype, device=x.device)
    view = flat[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and torch.equal(view, x)
    return view


# ------------------------------------------------------------------------------------------------ 4. non-dyadic
def test_mfma_chain_equals_serial_chain_and_float64_bound(dev):
    rng = np.random.default_rng(4)
    D, nd, nq, k = 1024, 2000, 64, 100
    E = rng.standard_normal((nd, D))
    Q = rng.standard_normal((nq, D))
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    idx = _index(E, dev)
    q = torch.from_numpy(Q).to(dev)
    pairs = torch.stack(torch.meshgrid(torch.arange(nq), torch.arange(nd), indexing="ij"), -1).reshape(-1, 2).to(dev)
    P = idx.pair_scores(q, pairs).cpu().numpy().reshape(nq, nd)
    # (a) the search (MFMA) ranks the values of the serial chain, bit for bit
    sc, dc, _, _ = idx.search(q, k)
    rs, rd, _, _ = R.search(P, k)
    assert np.array_equal(dc.cpu().numpy(), rd)
    assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs))
    # (b) |s - float64 dot| <= D * 2^-24 * sum_j |q_j e_j|: the first-order bound of a length-D fp32 chain (each of the
    # D roundings is at most half an ulp, 2^-24 relative, of a partial sum that sum_j |q_j e_j| bounds)
    Q64, E64 = Q.astype(np.float64), E.astype(np.float64)
    exact = Q64 @ E64.T
    bound = D * 2.0 ** -24 * (np.abs(Q64) @ np.abs(E64).T)
    err = np.abs(P.astype(np.float64) - exact)
    print(f"max err {err.max():.3e}, min bound {bound.min():.3e}, max err / bound {(err / bound).max():.3e}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ 5. band
@pytest.mark.parametrize("lo,hi", [(0, 1), (10, 50), (1000, 1024)])
def test_band_exclusions_and_ceilings(dev, lo, hi):
    rng = np.random.default_rng(5)
    nd, D = 1500, 33
    E, Q = _dyadic(rng, nd, D), _dyadic(rng, 9, D)
    S = R.exact_scores(Q, E)
    some = sorted(rng.choice(nd, size=700, replace=False).tolist())
    top = [int(d) for d in R.ranked(S[4])[:30]]              # the best 30 docs of query 4 leave its ranking
    excl = [[], some, list(range(nd)), [], top, [], some, [], []]
    mid = [float(np.sort(S[q])[::-1][200]) for q in range(9)]   # an existing score: strictly below it only
    ceil = [np.inf, np.inf, np.inf, mid[3], mid[4], -np.inf, mid[6], float(S[7].max()), float(S[8].min())]
    idx = _index(E, dev)
    q = torch.from_numpy(Q).to(dev)
    for ex, ce in ((excl, None), (None, ceil), (excl, ceil)):
        ct = None if ce is None else torch.tensor(ce, dtype=torch.float32, device=dev)
        sc, dc, fd = idx.search_band(q, lo, hi, exclude=ex, ceiling=ct)
        rs, rd, rf = R.search_band(S, lo, hi, ex, ce)
        assert np.array_equal(fd.cpu().numpy(), rf)
        assert np.array_equal(dc.cpu().numpy(), rd)
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs))
    # the unused slots of the last run: doc -1, score +0; the fully excluded and the -inf query found nothing
    f = fd.cpu().numpy()
    assert f[2] == 0 and f[5] == 0 and f[8] == 0
    d, s = dc.cpu().numpy(), _bits(sc.cpu().numpy())
    for r in range(9):
        assert (d[r, f[r]:] == -1).all() and (s[r, f[r]:] == 0).all()


# ------------------------------------------------------------------------------------------------ 6. signs
def test_negative_zero_and_underflow_scores(dev):
    from snx.retrieval import DenseIndex
    rng = np.random.default_rng(6)
    # all scores negative
    E = -np.maximum(np.abs(_dyadic(rng, 300, 8)), np.float32(0.125))
    Q = np.maximum(np.abs(_dyadic(rng, 5, 8)), np.float32(0.125))
    S = R.exact_scores(Q, E)
    assert (S < 0).all()
    t = rng.integers(0, 300, size=5)
    _same_search(_index(E, dev).search(torch.from_numpy(Q).to(dev), 10, targets=torch.from_numpy(t).to(dev)),
                 R.search(S, 10, t))
    # all-zero docs tie at +0 by id
    Z = np.zeros((200, 5), np.float32)
    sc, dc, rk, ts = _index(Z, dev).search(torch.from_numpy(Q[:, :5].copy()).to(dev), 10,
                                           targets=torch.full((5,), 150, device=dev))
    assert np.array_equal(dc.cpu().numpy(), np.tile(np.arange(10, dtype=np.int32), (5, 1)))
    assert (_bits(sc.cpu().numpy()) == 0).all() and (rk.cpu().numpy() == 151).all() and (_bits(ts.cpu().numpy()) == 0).all()
    # 2^-100 * -2^-100 underflows to -0: that doc ranks among the zeros by doc id, and its score reads +0
    E1 = np.zeros((6, 1), np.float32)
    E1[2, 0] = -2.0 ** -100
    E1[4, 0] = 2.0 ** -60                                    # 2^-160: below the subnormals, +0
    E1[5, 0] = 2.0 ** -40                                    # 2^-140: a subnormal, the only positive score
    Q1 = np.full((1, 1), 2.0 ** -100, np.float32)
    S1 = R.chain_scores(Q1, E1)
    assert _bits(S1)[0, 2] == 0 and S1[0, 5] > 0
    idx = DenseIndex(1, dev)
    idx.add(torch.from_numpy(E1).to(dev))
    idx.build()
    q1 = torch.from_numpy(Q1).to(dev)
    got = idx.search(q1, 6, targets=torch.tensor([2], device=dev))
    _same_search(got, R.search(S1, 6, np.array([2])))
    assert got[1].cpu().numpy().tolist() == [[5, 0, 1, 2, 3, 4]] and int(got[2][0]) == 4
    ps = idx.pair_scores(q1, torch.tensor([[0, 2], [0, 5]], device=dev)).cpu().numpy()
    assert _bits(ps)[0] == 0 and _bits(ps)[1] == _bits(S1)[0, 5]


# ------------------------------------------------------------------------------------------------ 7. errors
def test_argument_errors(dev):
    from snx.retrieval import DenseIndex
    for dim in (0, 4097, -1, 2.5, True):
        with pytest.raises(ValueError):
            DenseIndex(dim, dev)
    idx = DenseIndex(8, dev)
    good = torch.zeros((4, 8), device=dev)
    q = torch.ones((2, 8), device=dev)
    for bad in (torch.zeros((4, 8), dtype=torch.float64, device=dev), torch.zeros((4, 7), device=dev),
                torch.zeros(8, device=dev), torch.zeros((4, 8)), torch.full((4, 8), float("nan"), device=dev),
                torch.full((4, 8), float("inf"), device=dev), np.zeros((4, 8), np.float32)):
        with pytest.raises(ValueError):
            idx.add(bad)
    idx.add(good)
    for call in (lambda: idx.search(q, 1), lambda: idx.search_band(q, 0, 1),
                 lambda: idx.pair_scores(q, torch.zeros((1, 2), dtype=torch.long, device=dev))):
        with pytest.raises(RuntimeError):
            call()
    idx.build()
    bad_q = (q.double(), q[:, :7], q.cpu(), torch.full((2, 8), float("-inf"), device=dev))
    for b in bad_q:
        with pytest.raises(ValueError):
            idx.search(b, 1)
        with pytest.raises(ValueError):
            idx.search_band(b, 0, 1)
        with pytest.raises(ValueError):
            idx.pair_scores(b, torch.zeros((1, 2), dtype=torch.long, device=dev))
    for k in (0, 1025, -1):
        with pytest.raises(ValueError):
            idx.search(q, k)
    for lo, hi in ((-1, 1), (0, 0), (5, 5), (6, 5), (0, 1025)):
        with pytest.raises(ValueError):
            idx.search_band(q, lo, hi)
    for chunk in (-1, 1, TILE - 1):
        with pytest.raises(ValueError):
            idx.search(q, 1, chunk_docs=chunk)
        with pytest.raises(ValueError):
            idx.search_band(q, 0, 1, chunk_docs=chunk)
    for t in (torch.tensor([0, 4], device=dev), torch.tensor([0], device=dev), torch.tensor([0.0, 1.0], device=dev),
              torch.tensor([0, 1])):
        with pytest.raises(ValueError):
            idx.search(q, 1, targets=t)
    with pytest.raises(ValueError):
        idx.search_band(q, 0, 1, ceiling=torch.tensor([float("nan"), 0.0], device=dev))
    with pytest.raises(ValueError):
        idx.search_band(q, 0, 1, exclude=[[4], []])
    for p in (torch.tensor([[0, 4]], device=dev), torch.tensor([[2, 0]], device=dev), torch.tensor([0, 1], device=dev),
              torch.tensor([[0.0, 1.0]], device=dev)):
        with pytest.raises(ValueError):
            idx.pair_scores(q, p)
    # and what is valid at the edges runs: an empty query set, k > nd
    sc, dc, _, _ = idx.search(q[:0], 3)
    assert sc.shape == (0, 3) and dc.shape == (0, 3)
    sc, dc, _, _ = idx.search(q, 6)
    assert dc.cpu().numpy().tolist() == [[0, 1, 2, 3, -1, -1]] * 2


# ------------------------------------------------------------------------------------------------ 8. end to end, tiny
def _tree(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path))}


def test_teacher_pipeline_on_the_gpu_equals_the_stand_in_byte_for_byte(dev, tmp_path):
    from snx.retrieval import DenseIndex
    from src.train.mining.dense import load_teacher_cache, mine_dense_negatives, write_teacher_scores
    from tests.test_dense_host import golden_cache, mine_case
    g, npy, tix, src = golden_cache(tmp_path)
    emb, text_to_idx = load_teacher_cache(npy, tix)
    files = sorted(str(p) for p in src.iterdir())
    n_gpu = write_teacher_scores(files, str(tmp_path / "score_gpu"), emb, text_to_idx, DenseIndex(g["dim"], dev))
    n_cpu = write_teacher_scores(files, str(tmp_path / "score_cpu"), emb, text_to_idx, R.NumpyDenseIndex(g["dim"]))
    assert n_gpu == n_cpu == g["total"]
    assert _tree(tmp_path / "score_gpu") == _tree(tmp_path / "score_cpu")
    memb, mtix, mfiles = mine_case(tmp_path / "mine")
    for lo, hi in ((1, 3), (3, 5), (5, 6)):                      # full bands, a padded band, the fallback
        kw = dict(k=2, rank_start=lo, rank_end=hi)
        s_gpu = mine_dense_negatives(mfiles, str(tmp_path / f"gpu{lo}"), memb, mtix, DenseIndex(2, dev), **kw)
        s_cpu = mine_dense_negatives(mfiles, str(tmp_path / f"cpu{lo}"), memb, mtix, R.NumpyDenseIndex(2), **kw)
        assert s_gpu == s_cpu
        assert _tree(tmp_path / f"gpu{lo}") == _tree(tmp_path / f"cpu{lo}")


def test_teacher_scores_cli_writes_the_reference_files(dev, tmp_path):
    from src.train.cli import teacher_scores
    from tests.test_dense_host import golden_cache
    g, npy, tix, src = golden_cache(tmp_path)
    total = teacher_scores.main(["score", "--embeddings", npy, "--text-index", tix, "--input-pattern",
                                 str(src / "train_*.jsonl"), "--val-pattern", str(src / "val.jsonl"), "--output-dir",
                                 str(tmp_path / "out")])
    assert total == g["total"]
    for name, want in g["expected"].items():
        assert (tmp_path / "out" / name).read_text(encoding="utf-8").splitlines() == want, name


def test_eval_hybrid_dense_embeddings_equal_the_dense_run_of_the_reference_lists(dev, tmp_path):
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.cli import eval_hybrid
    from tests.test_gpu_retrieval import _val_file
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(dict(
        vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
        local_attention=16, pad_token_id=999)))
    torch.manual_seed(5)
    (tmp_path / "ckpt").mkdir()
    torch.save(SPLADEModernBERT(model_name=str(mdir)).state_dict(), tmp_path / "ckpt" / "model.pt")
    argv = ["--checkpoint", str(tmp_path / "ckpt" / "model.pt"), "--model-name", str(mdir), "--tokenizer", "hash:1000",
            "--val-file", _val_file(tmp_path, 80), "--max-queries", "40", "--max-docs", "120", "--query-max-length", "16",
            "--doc-max-length", "32", "--batch-size", "16"]
    base = eval_hybrid.main(argv)
    nq, nd = base[0]["num_queries"], base[0]["num_docs"]
    rng = np.random.default_rng(8)
    E, Q = _dyadic(rng, nd, 24), _dyadic(rng, nq, 24)
    np.savez(tmp_path / "emb.npz", docs=E, queries=Q)
    scores, docs, _, _ = R.search(R.exact_scores(Q, E), 100)
    np.savez(tmp_path / "run.npz", docs=docs, scores=scores)
    from_run = eval_hybrid.main(argv + ["--dense-run", str(tmp_path / "run.npz")])
    from_emb = eval_hybrid.main(argv + ["--dense-embeddings", str(tmp_path / "emb.npz")])
    assert [x["method"] for x in from_emb] == ["sparse", "bm25", "bm25_sparse_rrf", "dense", "bm25_dense_rrf",
                                               "dense_sparse_rrf", "triple_rrf"]
    assert from_emb == from_run and from_emb[:3] == base
    with pytest.raises(ValueError):
        np.savez(tmp_path / "bad.npz", docs=E[:-1], queries=Q)
        eval_hybrid.main(argv + ["--dense-embeddings", str(tmp_path / "bad.npz")])

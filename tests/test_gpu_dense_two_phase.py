"""GPU checks of the two-phase dense retrieval (csrc/dense_two_phase.hip, include/snx.h "two-phase dense retrieval"):
snx.retrieval.bf16_rows and DenseIndex.candidates / search_two_phase / search_band_two_phase, and the flat2 index of
src.train.cli.teacher_scores.

Everything is compared exactly -- int32 ids and fp32 / float64 BITS.  The prepare step and, on the grid fixture (where no
sum rounds in any order), phase 1 are held to tests/dense_two_phase_reference.py; phase 2 is held to the card's own exact
search (search, search_band, pair_scores), which tests/test_gpu_dense.py holds to its reference."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dense_reference as DR
from tests import dense_two_phase_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _np(x):
    return x.cpu().numpy()


def _index(E, dev):
    from snx.retrieval import DenseIndex
    idx = DenseIndex(E.shape[1], dev)
    idx.add(torch.from_numpy(np.ascontiguousarray(E)).to(dev))
    return idx.build()


def _same(got, want):
    """(scores, docs[, found]) tensors, bit for bit."""
    assert np.array_equal(_np(got[1]), _np(want[1]))
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    if len(want) > 2:
        assert np.array_equal(_np(got[2]), _np(want[2]))


# ------------------------------------------------------------------------------------------------ 1. prepare
@pytest.mark.parametrize("D", (1, 31, 32, 100, 1024))
def test_prepare_equals_the_reference_bit_for_bit(dev, D):
    from snx.retrieval import bf16_rows
    rng = np.random.default_rng(D)
    n = 300
    X = (rng.standard_normal((n, D)) * np.exp2(rng.integers(-20, 21, size=(n, 1)))).astype(np.float32)
    flat = X.reshape(-1)
    m = min(flat.size, 64)
    # rounding ties (both parities), values that round up into the next binade, subnormals, and an overflow to infinity
    special = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 2.0 - 2.0 ** -9, 1e-40, -3e-39, 3.4e38,
                        0.0, -0.0, 2.0 ** -126], np.float32)
    flat[:m] = np.resize(special, m)
    bits, n2, h2, r2 = (_np(t) for t in bf16_rows(torch.from_numpy(X).to(dev)))
    wb, wn, wh, wr = R.prepare(X)
    assert bits.shape == (n, R.dp(D)) and np.array_equal(bits.view(np.uint16), wb)
    for got, want in ((n2, wn), (h2, wh), (r2, wr)):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ------------------------------------------------------------------------------------------------ 2. grid fixture
@pytest.mark.parametrize("D", (32, 100))
@pytest.mark.parametrize("nq", (1, 130))
@pytest.mark.parametrize("k", (1, 10, 100))
def test_grid_fixture_is_the_reference_and_certified(dev, D, nq, k):
    nd = 1000
    Q, E = R.grid_fixture(nd, D, nq, k, seed=7 * D + k)
    idx, q = _index(E, dev), torch.from_numpy(Q).to(dev)
    k1 = R.search_k1(nd, k, 2)
    S = DR.exact_scores(Q, E)                                  # no sum rounds: this is a(q, d) and s(q, d) in any order
    wd, wa = R.candidates(S, k1)
    approx, docs = idx.candidates(q, k1)
    assert np.array_equal(_np(docs), wd) and np.array_equal(_bits(approx), _bits(wa))     # ties: lowest doc id first
    sc, dc, cert = idx.search_two_phase(q, k, expansion=2)
    assert bool(cert.all())
    _same((sc, dc), idx.search(q, k)[:2])
    ws, wdoc, _, _ = DR.search(S, k)
    assert np.array_equal(_np(dc), wdoc) and np.array_equal(_bits(sc), _bits(ws))


# ------------------------------------------------------------------------------------------------ 3. random operands
_CACHE = {}


def _random_case(dev, D):
    """nd = 5000 normalised docs, 130 queries (a second query tile, a ragged last doc tile), built once per D."""
    if D not in _CACHE:
        rng = np.random.default_rng(100 + D)
        E = rng.standard_normal((5000, D)).astype(np.float32)
        Q = rng.standard_normal((130, D)).astype(np.float32)
        E /= np.linalg.norm(E, axis=1, keepdims=True)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        _CACHE[D] = (_index(E, dev), torch.from_numpy(Q).to(dev), {})
    return _CACHE[D]


@pytest.mark.parametrize("D", (64, 100, 1024))
@pytest.mark.parametrize("k", (10, 100))
@pytest.mark.parametrize("expansion", (1, 4))
def test_random_operands(dev, D, k, expansion):
    idx, q, exact = _random_case(dev, D)
    if k not in exact:
        exact[k] = idx.search(q, k)[:2]
    want = exact[k]
    sc, dc, cert = idx.search_two_phase(q, k, expansion=expansion)
    nq = q.shape[0]
    # every returned score is the ABI's chain
    pairs = torch.stack([torch.arange(nq, device=dev).repeat_interleave(k), dc.reshape(-1).long()], 1)
    assert np.array_equal(_bits(idx.pair_scores(q, pairs)), _bits(sc).reshape(-1))
    s, d = _np(sc).astype(np.float64), _np(dc)
    assert ((s[:, :-1] > s[:, 1:]) | ((s[:, :-1] == s[:, 1:]) & (d[:, :-1] < d[:, 1:]))).all()
    # a certified row is the exact search's
    c = _np(cert)
    print(f"D={D} k={k} expansion={expansion}: certified {int(c.sum())} of {nq}")
    assert np.array_equal(d[c], _np(want[1])[c]) and np.array_equal(_bits(sc)[c], _bits(want[0])[c])
    if expansion == 4:
        assert c.any()
    _same(idx.search_two_phase(q, k, expansion=expansion, exact=True)[:2], want)
    # several splits and their merge, one tile per split, a second launch: no bit of any output moves
    k1 = R.search_k1(5000, k, expansion)
    ca, cd = idx.candidates(q, k1)
    for chunk_docs in (0, 128, 1024):
        for query_slice in (0, 64):
            if chunk_docs == 0 and query_slice == 0:
                continue
            s2, d2, c2 = idx.search_two_phase(q, k, expansion=expansion, chunk_docs=chunk_docs, query_slice=query_slice)
            _same((s2, d2), (sc, dc))
            assert np.array_equal(_np(c2), c)
            a2, e2 = idx.candidates(q, k1, chunk_docs=chunk_docs, query_slice=query_slice)
            assert np.array_equal(_np(e2), _np(cd)) and np.array_equal(_bits(a2), _bits(ca))


# ------------------------------------------------------------------------------------------------ 4. small shapes
def test_all_docs_are_candidates(dev):
    rng = np.random.default_rng(5)
    E, Q = rng.standard_normal((50, 48)).astype(np.float32), rng.standard_normal((9, 48)).astype(np.float32)
    idx, q = _index(E, dev), torch.from_numpy(Q).to(dev)
    sc, dc, cert = idx.search_two_phase(q, 100)
    assert bool(cert.all()) and bool((dc[:, 50:] == -1).all()) and not bool(sc[:, 50:].any())
    _same((sc, dc), idx.search(q, 100)[:2])
    sc, dc, cert = idx.search_two_phase(q[:0], 3)
    assert sc.shape == (0, 3) and dc.shape == (0, 3) and cert.shape == (0,)


def test_band_with_exclusions_and_ceiling(dev):
    rng = np.random.default_rng(6)
    nd, nq, D, lo, hi = 3000, 70, 96, 10, 50
    E, Q = rng.standard_normal((nd, D)).astype(np.float32), rng.standard_normal((nq, D)).astype(np.float32)
    idx, q = _index(E, dev), torch.from_numpy(Q).to(dev)
    top_s, top_d, _, _ = idx.search(q, 64)
    top_s, top_d = _np(top_s), _np(top_d)
    exclude = [sorted(rng.choice(top_d[i], size=i % 9, replace=False).tolist()) for i in range(nq)]
    # the ceiling cuts the best five docs of every other query; +inf cuts none
    ceiling = torch.from_numpy(np.array([top_s[i, 4] if i % 2 else np.inf for i in range(nq)], np.float32)).to(dev)
    want = idx.search_band(q, lo, hi, exclude=exclude, ceiling=ceiling)
    sc, dc, fd, cert = idx.search_band_two_phase(q, lo, hi, exclude=exclude, ceiling=ceiling)
    c = _np(cert)
    print(f"band: certified {int(c.sum())} of {nq}")
    assert c.any()
    for got, ref in ((dc, want[1]), (fd, want[2])):
        assert np.array_equal(_np(got)[c], _np(ref)[c])
    assert np.array_equal(_bits(sc)[c], _bits(want[0])[c])
    for expansion in (1, 4):                                   # expansion 1 leaves rows uncertified: the fallback runs
        got = idx.search_band_two_phase(q, lo, hi, exclude=exclude, ceiling=ceiling, expansion=expansion, exact=True,
                                        query_slice=32)
        _same(got[:3], want)
    assert not bool(idx.search_band_two_phase(q, lo, hi, exclude=exclude, ceiling=ceiling, expansion=1)[3].all())


def test_adversarial_twins_on_the_card(dev):
    Q, E, ids = R.adversarial_fixture()
    idx, q = _index(E, dev), torch.from_numpy(Q).to(dev)
    approx, docs = idx.candidates(q, 20)
    assert _np(docs)[0].tolist() == ids[:20].tolist() and (_np(approx) == 32.0).all()
    sc, dc, cert = idx.search_two_phase(q, 10, expansion=2)
    assert not bool(cert[0]) and _np(dc)[0].tolist() == ids[19:9:-1].tolist()
    sc, dc, cert = idx.search_two_phase(q, 10, expansion=2, exact=True)
    assert not bool(cert[0]) and _np(dc)[0].tolist() == ids[:-11:-1].tolist()
    _same((sc, dc), idx.search(q, 10)[:2])


def test_operands_that_could_overflow_fp32_are_never_certified(dev):
    Q = np.zeros((2, 4), np.float32)
    Q[0, 0], Q[1, 1] = 2.0 ** 64, 1.0
    E = np.zeros((40, 4), np.float32)
    E[:, 1] = np.arange(40, dtype=np.float32)
    E[3, 2] = 2.0 ** 64
    idx, q = _index(E, dev), torch.from_numpy(Q).to(dev)
    # k1 = 6, and every doc a candidate: there the second query, small enough (2^64 <= 2^127), is certified
    for k, expansion, want in ((3, 2, [False, False]), (3, 40, [False, True])):
        sc, dc, cert = idx.search_two_phase(q, k, expansion=expansion)
        assert _np(cert).tolist() == want
        _same(idx.search_two_phase(q, k, expansion=expansion, exact=True)[:2], idx.search(q, k)[:2])


def test_add_drops_the_bf16_copy(dev):
    rng = np.random.default_rng(8)
    E, Q = rng.standard_normal((300, 40)).astype(np.float32), rng.standard_normal((4, 40)).astype(np.float32)
    idx, q = _index(E[:200], dev), torch.from_numpy(Q).to(dev)
    idx.search_two_phase(q, 5)
    idx.add(torch.from_numpy(E[200:]).to(dev))
    idx.build()
    _same(idx.search_two_phase(q, 5, exact=True)[:2], _index(E, dev).search(q, 5)[:2])


def test_argument_errors_raise_before_any_launch(dev):
    from snx._lib import SnxError, call
    from snx.ops import _p
    from snx.retrieval import DenseIndex, bf16_rows
    idx = DenseIndex(8, dev)
    q = torch.zeros((2, 8), device=dev)
    idx.add(torch.zeros((40, 8), device=dev))
    for run in (lambda: idx.search_two_phase(q, 1), lambda: idx.search_band_two_phase(q, 0, 1),
                lambda: idx.candidates(q, 1)):
        with pytest.raises(RuntimeError):
            run()
    idx.build()
    for k in (0, 1025, -1):
        with pytest.raises(ValueError):
            idx.search_two_phase(q, k)
        with pytest.raises(ValueError):
            idx.candidates(q, k)
    for expansion in (0.5, 0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            idx.search_two_phase(q, 1, expansion=expansion)
        with pytest.raises(ValueError):
            idx.search_band_two_phase(q, 0, 1, expansion=expansion)
    for lo, hi in ((-1, 1), (0, 0), (6, 5), (0, 1025)):
        with pytest.raises(ValueError):
            idx.search_band_two_phase(q, lo, hi)
    for bad in (q.double(), q[:, :7], q.cpu(), torch.full((2, 8), float("inf"), device=dev)):
        with pytest.raises(ValueError):
            idx.search_two_phase(bad, 1)
    with pytest.raises(ValueError):
        idx.search_two_phase(q, 1, chunk_docs=127)
    with pytest.raises(ValueError):
        idx.search_two_phase(q, 1, query_slice=-1)
    with pytest.raises(ValueError, match="search_band"):
        idx.search_band_two_phase(q, 0, 1020, exclude=[list(range(5)), []])
    with pytest.raises(ValueError):
        bf16_rows(torch.zeros((2, 4097), device=dev))
    # the C ABI checks shapes and arguments on the host
    qb, n2, h2, r2 = bf16_rows(q)
    eb = bf16_rows(idx.emb)[0]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    cd = torch.full((2, 4), -1, dtype=torch.int32, device=dev)
    ca = torch.zeros((2, 4), device=dev)
    out_f, out_c = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.uint8, device=dev)
    for D, k1 in ((0, 4), (4097, 4), (8, 0), (8, 1025)):
        with pytest.raises(SnxError, match="SNX_E_SHAPE"):
            call("snx_dense2_scan", _p(qb), 2, _p(eb), 40, D, k1, 0, _p(cd), _p(ca), _p(ws), ws.numel(), None)
    with pytest.raises(SnxError, match="SNX_E_ARG"):
        call("snx_dense2_scan", _p(qb), 2, _p(eb), 40, 8, 4, 0, _p(cd), _p(ca), _p(ws), 16, None)
    with pytest.raises(SnxError, match="SNX_E_ARG"):
        call("snx_dense2_scan", None, 2, _p(eb), 40, 8, 4, 0, _p(cd), _p(ca), _p(ws), ws.numel(), None)
    for lo, hi in ((-1, 2), (2, 2), (0, 5)):
        with pytest.raises(SnxError, match="SNX_E_SHAPE"):
            call("snx_dense2_rescore", _p(q), 2, _p(idx.emb), 40, 8, _p(cd), _p(ca), 4, _p(n2), _p(h2), _p(r2), 0.0, 0.0,
                 0.0, None, None, None, lo, hi, _p(cd), _p(ca), _p(out_f), _p(out_c), None)
    with pytest.raises(SnxError, match="SNX_E_ARG"):
        call("snx_dense2_rescore", _p(q), 2, _p(idx.emb), 40, 8, _p(cd), _p(ca), 4, _p(n2), _p(h2), _p(r2), 0.0, 0.0,
             0.0, None, None, None, 0, 4, _p(cd), _p(ca), _p(out_f), None, None)
    with pytest.raises(SnxError, match="SNX_E_SHAPE"):
        call("snx_dense2_prepare", _p(q), 2, 0, _p(qb), _p(n2), _p(h2), _p(r2), None)
    assert not bool(out_f.any()) and not bool(out_c.any()) and bool((cd == -1).all())        # nothing ran


# ------------------------------------------------------------------------------------------------ 5. the CLI
def test_mine_flat2_writes_the_files_of_flat(dev, tmp_path):
    from src.train.cli import teacher_scores
    from src.train.mining.dense import text_hash
    rng = np.random.default_rng(9)
    nq, nd, D = 12, 400, 64
    texts = [f"query {i}" for i in range(nq)] + [f"doc {i}" for i in range(nd)]
    emb = rng.standard_normal((len(texts), D)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    np.save(tmp_path / "embeddings.npy", emb)
    (tmp_path / "text_index.json").write_text(json.dumps({text_hash(t): i for i, t in enumerate(texts)}))
    os.makedirs(tmp_path / "in")
    for shard in range(2):
        with open(tmp_path / "in" / f"train_{shard}.jsonl", "w") as f:
            for i in range(shard, nq, 2):
                negs = [f"doc {(7 * i + j) % nd}" for j in range(1, 4)]
                f.write(json.dumps({"query": f"query {i}", "positive": f"doc {i}", "negatives": negs}) + "\n")
            for d in range(shard, nd, 2):                        # the rest of the corpus, as records of its own
                f.write(json.dumps({"query": f"query {d % nq}", "positive": f"doc {d}", "negatives": []}) + "\n")
    base = ["mine", "--embeddings", str(tmp_path / "embeddings.npy"), "--text-index", str(tmp_path / "text_index.json"),
            "--input-pattern", str(tmp_path / "in" / "train_*.jsonl"), "--val-pattern", str(tmp_path / "none.jsonl"),
            "--k", "5", "--rank-start", "3", "--rank-end", "20", "--device", str(dev)]
    outs = {}
    for name, extra in (("flat", []), ("flat2", ["--index", "flat2"]),
                        ("flat2x1", ["--index", "flat2", "--expansion", "1"])):
        outs[name] = teacher_scores.main(base + ["--output-dir", str(tmp_path / name)] + extra)
    for shard in range(2):
        want = (tmp_path / "flat" / f"train_{shard}.jsonl").read_bytes()
        assert want and (tmp_path / "flat2" / f"train_{shard}.jsonl").read_bytes() == want
        assert (tmp_path / "flat2x1" / f"train_{shard}.jsonl").read_bytes() == want
    assert "certified_fraction" not in outs["flat"]
    assert 0.0 < outs["flat2"]["certified_fraction"] <= 1.0
    assert outs["flat2x1"]["certified_fraction"] <= outs["flat2"]["certified_fraction"]
    assert {k: v for k, v in outs["flat2"].items() if k != "certified_fraction"} == outs["flat"]


def test_eval_hybrid_flat2_returns_the_lists_of_flat(dev, tmp_path):
    from src.train.cli.eval_hybrid import search_dense_embeddings
    rng = np.random.default_rng(10)
    nq, nd, D, depth = 33, 700, 72, 100
    E, Q = rng.standard_normal((nd, D)).astype(np.float32), rng.standard_normal((nq, D)).astype(np.float32)
    np.savez(tmp_path / "emb.npz", docs=E, queries=Q)
    d1, s1, x1 = search_dense_embeddings(str(tmp_path / "emb.npz"), nq, nd, depth, dev)
    d2, s2, x2 = search_dense_embeddings(str(tmp_path / "emb.npz"), nq, nd, depth, dev, "flat2")
    _same((s2, d2), (s1, d1))
    assert x1 == {} and x2["dense_index"] == "flat2" and 0.0 <= x2["certified_fraction"] <= 1.0

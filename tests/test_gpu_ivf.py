"""GPU checks of the IVF-Flat dense retrieval (csrc/ivf.hip, include/snx.h "IVF-Flat dense retrieval"):
snx.retrieval.IvfFlatIndex, the miner on it (src.preprocessing.miners) and ``teacher_scores mine --index ivf``.

Everything is compared exactly -- int32 ids and fp32 BITS.  On dyadic data (integers in [-8, 8] divided by 8: every
partial sum of the score chain is exact) the reference is the numpy stand-in tests/ivf_reference.py; on random fp32 data it
is the composition the definition states: ``DenseIndex.search`` when every list is probed, ``DenseIndex.search_band`` with
the docs of the other lists excluded otherwise, ``DenseIndex.pair_scores`` for the scores.

Shapes: D 20 (ragged against the K tile and the 16-byte loads) and 64; 1000 docs in 7 lists set by hand -- list 2 holds 600
(five doc tiles, five splits at 128 docs per split), list 6 is empty (its centroid repeats list 0's), the rest hold fewer
than 128; 130 queries (two query tiles when they all probe one list); nprobe 1, 3 and 7; k 1, 10 and 1024 (more than the
probed lists hold)."""
import json

import numpy as np
import pytest
import torch

from tests import dense_reference as DR
from tests import ivf_reference as R

pytestmark = pytest.mark.gpu

NLIST, ND, NQ = 7, 1000, 130


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _centroids(D):
    c = np.zeros((NLIST, D), np.float32)
    c[np.arange(6), np.arange(6)] = 1.0
    c[6] = c[0]                                              # a duplicate: every tie goes to list 0, list 6 stays empty
    return c


def _dyadic_case(D):
    """Docs whose coordinate `want` alone is 1.0, the largest value there is: list(d) = want[d], 600 docs in list 2."""
    rng = np.random.default_rng(D)
    E = (rng.integers(-8, 9, size=(ND, D)) / 8.0).astype(np.float32)
    E[:, :6] = np.minimum(E[:, :6], np.float32(0.875))       # no second 1.0 among the coordinates the centroids read
    want = np.concatenate([np.full(600, 2), np.repeat([0, 1, 3, 4, 5], 80)])
    want = want[rng.permutation(ND)]
    E[np.arange(ND), want] = 1.0
    Q = (rng.integers(-8, 9, size=(NQ, D)) / 8.0).astype(np.float32)
    Q[:100, 2] = 1.0                                         # most queries probe the long list first: a full query tile
    return E, Q, _centroids(D)


def _gpu_index(E, Cn, dev, batches=3, **kw):
    from snx.retrieval import IvfFlatIndex
    idx = IvfFlatIndex(E.shape[1], Cn.shape[0], dev, **kw).set_centroids(_t(Cn, dev))
    for part in np.array_split(E, batches):
        idx.add(_t(part, dev))
    return idx.build()


_CACHE = {}


def _dyadic_pair(D, dev):
    """(case, GPU index, stand-in), built once per D."""
    if D not in _CACHE:
        E, Q, Cn = _dyadic_case(D)
        ref = R.NumpyIvfFlatIndex(D, NLIST).set_centroids(Cn)
        ref.add(E)
        _CACHE[D] = ((E, Q, Cn), _gpu_index(E, Cn, dev), ref.build())
    return _CACHE[D]


@pytest.fixture
def split128(monkeypatch):
    from snx.retrieval import ivf
    monkeypatch.setattr(ivf, "_IVF_SPLIT_DOCS", 128)


# ------------------------------------------------------------------------------------------------ 1. dyadic data
@pytest.mark.parametrize("D", [20, 64])
def test_structure_and_probe_equal_the_stand_in(dev, D):
    (E, Q, Cn), idx, ref = _dyadic_pair(D, dev)
    st, rs = idx.structure(), ref.structure()
    sizes = np.diff(rs["list_ptr"])
    assert sizes[6] == 0 and sizes[2] > 4 * 128 and (sizes[[0, 1, 3, 4, 5]] < 128).all() and sizes.sum() == ND
    assert np.array_equal(st["list_ptr"].cpu().numpy(), rs["list_ptr"])
    assert np.array_equal(st["list_doc"].cpu().numpy(), rs["list_doc"])
    assert np.array_equal(_bits(st["centroids"].cpu().numpy()), _bits(Cn))
    assert idx.max_list == sizes.max()
    for nprobe in (1, 3, NLIST):
        sc, ls = idx.probe(_t(Q, dev), nprobe)
        rsc, rls = ref.probe(Q, nprobe)
        assert np.array_equal(ls.cpu().numpy(), rls) and np.array_equal(_bits(sc.cpu().numpy()), _bits(rsc))


@pytest.mark.parametrize("k", [1, 10, 1024])
@pytest.mark.parametrize("nprobe", [1, 3, NLIST])
@pytest.mark.parametrize("D", [20, 64])
def test_search_equals_the_stand_in_on_dyadic_data(dev, D, nprobe, k, monkeypatch):
    from snx.retrieval import ivf
    monkeypatch.setattr(ivf, "_IVF_SPLIT_DOCS", 128 if D == 20 else 0)       # the long list in five splits, and in one
    (E, Q, Cn), idx, ref = _dyadic_pair(D, dev)
    sc, dc = idx.search(_t(Q, dev), k, nprobe=nprobe)
    rs, rd = ref.search(Q, k, nprobe=nprobe)
    assert np.array_equal(dc.cpu().numpy(), rd)
    assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs))
    if k == 1024 and nprobe == 1:
        assert (rd == -1).any()                              # more slots than the probed list holds


@pytest.mark.parametrize("lo,hi", [(0, 1), (10, 50), (100, 612)])
def test_band_equals_the_stand_in_on_dyadic_data(dev, lo, hi, split128):
    (E, Q, Cn), idx, ref = _dyadic_pair(20, dev)
    rng = np.random.default_rng(7)
    excl = [sorted(rng.choice(ND, size=int(n), replace=False).tolist()) for n in rng.choice([0, 5, 400, ND], size=NQ)]
    S = DR.exact_scores(Q, E)
    ceil = np.where(rng.random(NQ) < 0.5, np.inf, np.sort(S, axis=1)[:, ::-1][:, 30]).astype(np.float32)
    ceil[7] = -np.inf
    for ex, ce in ((excl, None), (None, ceil), (excl, ceil)):
        ct = None if ce is None else _t(ce, dev)
        sc, dc, fd = idx.search_band(_t(Q, dev), lo, hi, exclude=ex, ceiling=ct, nprobe=3)
        rs, rd, rf = ref.search_band(Q, lo, hi, exclude=ex, ceiling=ce, nprobe=3)
        assert np.array_equal(fd.cpu().numpy(), rf)
        assert np.array_equal(dc.cpu().numpy(), rd)
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs))


# ------------------------------------------------------------------------------------------------ 2. random fp32 data
def _random_case(D, nd=ND, seed=0):
    rng = np.random.default_rng(100 * D + seed)
    E = rng.standard_normal((nd, D))
    E[:600] += 3.0 * rng.standard_normal((1, D))             # a clump: one list much longer than the others
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    Q = rng.standard_normal((NQ, D))
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    Cn = E[[0, 700, 750, 800, 850, 900, 700]].copy()         # centroid 6 repeats centroid 1: an empty list
    return E, Q, Cn


def _complement(idx, q, nprobe):
    """Per query, the docs of the lists it does NOT probe, as exclusion rows."""
    st = idx.structure()
    ptr, doc = st["list_ptr"].cpu().numpy(), st["list_doc"].cpu().numpy()
    doc_list = np.empty(len(doc), np.int64)
    doc_list[doc] = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    probed = idx.probe(q, nprobe)[1].cpu().numpy()
    return [np.flatnonzero(~np.isin(doc_list, row)).tolist() for row in probed]


@pytest.mark.parametrize("D", [20, 64])
def test_random_data_equals_the_dense_index_composition(dev, D, split128):
    from snx.retrieval import DenseIndex
    E, Q, Cn = _random_case(D)
    idx = _gpu_index(E, Cn, dev)
    sizes = np.diff(idx.structure()["list_ptr"].cpu().numpy())
    assert sizes.max() > 2 * 128 and sizes[6] == 0
    flat = DenseIndex(D, dev)
    flat.add(_t(E, dev))
    flat.build()
    q = _t(Q, dev)
    # the two list rules are the dense search over the centroids
    cents = DenseIndex(D, dev)
    cents.add(_t(Cn, dev))
    cents.build()
    want_list = cents.search(_t(E, dev), 1)[1].cpu().numpy()[:, 0]
    st = idx.structure()
    got_list = np.empty(ND, np.int64)
    got_list[st["list_doc"].cpu().numpy()] = np.repeat(np.arange(NLIST), sizes)
    assert np.array_equal(got_list, want_list)
    assert _same(idx.probe(q, 3), cents.search(q, 3)[:2])
    for k in (1, 10, 1024):
        assert _same(idx.search(q, k, nprobe=NLIST), flat.search(q, k)[:2]), k
        for nprobe in (1, 3):
            want = flat.search_band(q, 0, k, exclude=_complement(idx, q, nprobe))
            assert _same(idx.search(q, k, nprobe=nprobe), want[:2]), (k, nprobe)
    pairs = torch.stack(torch.meshgrid(torch.arange(NQ), torch.arange(ND), indexing="ij"), -1).reshape(-1, 2).to(dev)
    P = idx.pair_scores(q, pairs)
    assert torch.equal(P.view(torch.int32), flat.pair_scores(q, pairs).view(torch.int32))
    sc, dc = idx.search(q, 10, nprobe=3)                     # the ranked scores are the pair scores
    assert torch.equal(sc.view(torch.int32), P.reshape(NQ, ND).gather(1, dc.long()).view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. ties
def test_thousands_of_ties_over_several_lists_resolve_by_doc_id(dev, split128):
    rng = np.random.default_rng(3)
    E = rng.integers(-1, 2, size=(3000, 4)).astype(np.float32)
    Q = rng.integers(-1, 2, size=(40, 4)).astype(np.float32)
    Cn = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, -1, 0, 0]], np.float32)
    assert len(np.unique(DR.exact_scores(Q, E))) <= 9
    idx = _gpu_index(E, Cn, dev)
    ref = R.NumpyIvfFlatIndex(4, 4).set_centroids(Cn)
    ref.add(E)
    ref.build()
    assert (np.diff(ref.list_ptr) > 200).all()
    for nprobe, k in ((4, 1024), (3, 1024), (2, 100)):
        sc, dc = idx.search(_t(Q, dev), k, nprobe=nprobe)
        rs, rd = ref.search(Q, k, nprobe=nprobe)
        assert np.array_equal(dc.cpu().numpy(), rd), (nprobe, k)
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs))


# ------------------------------------------------------------------------------------------------ 4. invariance
def test_slicing_batches_budget_and_splits_change_no_bit(dev, monkeypatch):
    from snx.retrieval import ivf
    E, Q, Cn = _random_case(20, seed=4)
    idx = _gpu_index(E, Cn, dev, batches=1)
    q = _t(Q, dev)
    rng = np.random.default_rng(4)
    excl = [rng.choice(ND, size=50, replace=False).tolist() for _ in range(NQ)]
    base = idx.search(q, 100, nprobe=3)
    band = idx.search_band(q, 10, 50, exclude=excl, nprobe=3)
    assert _same(base, idx.search(q, 100, nprobe=3))
    for qs in (1, 37):
        assert _same(base, idx.search(q, 100, nprobe=3, query_slice=qs)), qs
        assert _same(band, idx.search_band(q, 10, 50, exclude=excl, nprobe=3, query_slice=qs)), qs
    three = _gpu_index(E, Cn, dev, batches=3)
    assert _same(list(idx.structure().values()), list(three.structure().values()))
    assert _same(base, three.search(q, 100, nprobe=3))
    # nor does the alignment of the queries: D % 4 == 0, their base one float off a 16-byte boundary, the sorted rows on one
    from tests.test_gpu_dense import _one_float_off
    small = _gpu_index(E[:300], E[[0, 100, 200, 299]].copy(), dev, batches=1)
    q1 = _one_float_off(q)
    ex = [rng.choice(300, size=40, replace=False).tolist() for _ in range(NQ)]
    assert small.nlist == 4 and small.list_emb.data_ptr() % 16 == 0
    assert _same(small.search(q, 10, nprobe=2), small.search(q1, 10, nprobe=2))
    assert _same(small.search_band(q, 2, 10, exclude=ex, nprobe=2), small.search_band(q1, 2, 10, exclude=ex, nprobe=2))
    monkeypatch.setattr(ivf, "_IVF_SPLIT_DOCS", 128)
    assert _same(base, idx.search(q, 100, nprobe=3)) and _same(band, idx.search_band(q, 10, 50, exclude=excl, nprobe=3))
    monkeypatch.setattr(ivf, "_IVF_WS_BUDGET", 1 << 20)      # a few queries per launch, in the coarse step too
    assert _same(base, idx.search(q, 100, nprobe=3)) and _same(band, idx.search_band(q, 10, 50, exclude=excl, nprobe=3))
    tiny = _gpu_index(E, Cn, dev, batches=2)
    assert _same(list(idx.structure().values()), list(tiny.structure().values()))


# ------------------------------------------------------------------------------------------------ 5. train
def test_train_equals_the_stand_in_on_separated_clusters(dev):
    from snx.retrieval import IvfFlatIndex
    rng = np.random.default_rng(5)
    D, sizes = 20, (1100, 300, 300, 300, 300)          # one cluster beyond a segment of the centroid sum
    X = np.concatenate([8 * np.eye(D)[c] + rng.integers(-1, 2, size=(n, D)) for c, n in enumerate(sizes)])
    X = X[rng.permutation(len(X))].astype(np.float32)
    seed = next(s for s in range(2000)                       # a seed whose first rows come from five different clusters
                if len({int(np.argmax(X[r])) for r in np.random.RandomState(s).permutation(len(X))[:5]}) == 5)
    for niter in (0, 1, 4):
        want = R.kmeans(X, 5, niter, seed)
        got = IvfFlatIndex(D, 5, dev, niter=niter, seed=seed).train(_t(X, dev)).centroids
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), niter
    assert sorted(np.argmax(want, axis=1).tolist()) == [0, 1, 2, 3, 4]
    # build() trains by itself when no centroids were given, and clamps nlist to the doc count
    idx = IvfFlatIndex(D, 5, dev, niter=4, seed=seed)
    idx.add(_t(X, dev))
    idx.build()
    assert np.array_equal(_bits(idx.centroids.cpu().numpy()), _bits(want))
    assert sorted(np.diff(idx.list_ptr.cpu().numpy()).tolist()) == [300, 300, 300, 300, 1100]
    few = IvfFlatIndex(D, 100, dev, nprobe=100)
    few.add(_t(X[:3], dev))
    few.build()
    assert few.nlist == 3 and few.nprobe == 3 and int(few.list_ptr[-1]) == 3
    with pytest.raises(ValueError):
        IvfFlatIndex(D, 5, dev).train(_t(X[:4], dev))


def test_train_on_random_data_is_reproducible(dev):
    from snx.retrieval import IvfFlatIndex
    E, _, _ = _random_case(64, seed=5)
    runs = []
    for _ in range(2):
        idx = IvfFlatIndex(64, 16, dev, niter=3, seed=1)
        idx.add(_t(E, dev))
        runs.append(list(idx.build().structure().values()))
    assert _same(runs[0], runs[1])
    assert int(runs[0][1][-1]) == ND and sorted(runs[0][2].cpu().tolist()) == list(range(ND))
    norms = runs[0][0].double().norm(dim=1)
    assert bool(((norms - 1).abs() < 1e-6).all())


# ------------------------------------------------------------------------------------------------ 6. band
@pytest.mark.parametrize("lo,hi", [(0, 1), (10, 50), (1000, 1024)])
def test_band_exclusions_and_ceilings_equal_the_dense_composition(dev, lo, hi):
    from snx.retrieval import DenseIndex
    nd, D = 1500, 20
    E, Q, Cn = _random_case(D, nd=nd, seed=6)
    Q = Q[:9]
    idx = _gpu_index(E, Cn, dev)
    flat = DenseIndex(D, dev)
    flat.add(_t(E, dev))
    flat.build()
    q = _t(Q, dev)
    rng = np.random.default_rng(6)
    S = flat.pair_scores(q, torch.stack(torch.meshgrid(torch.arange(9), torch.arange(nd), indexing="ij"), -1)
                         .reshape(-1, 2).to(dev)).cpu().numpy().reshape(9, nd)
    some = sorted(rng.choice(nd, size=300, replace=False).tolist())
    top = [int(d) for d in DR.ranked(S[4])[:30]]
    excl = [[], some, list(range(nd)), [], top, [], some, [], []]
    mid = [float(np.sort(S[r])[::-1][100]) for r in range(9)]
    ceil = [np.inf, np.inf, np.inf, mid[3], mid[4], -np.inf, mid[6], float(S[7].max()), float(S[8].min())]
    for nprobe in (3, NLIST):
        comp = _complement(idx, q, nprobe)
        for ex, ce in ((excl, None), (None, ceil), (excl, ceil)):
            ct = None if ce is None else torch.tensor(ce, dtype=torch.float32, device=dev)
            both = [sorted(set(a) | set(b)) for a, b in zip(comp, ex if ex is not None else [[]] * 9)]
            got = idx.search_band(q, lo, hi, exclude=ex, ceiling=ct, nprobe=nprobe)
            want = flat.search_band(q, lo, hi, exclude=both, ceiling=ct)
            assert _same(got, want), (nprobe, ex is not None, ce is not None)
    f = got[2].cpu().numpy()
    assert f[2] == 0 and f[5] == 0 and f[8] == 0
    d, s = got[1].cpu().numpy(), _bits(got[0].cpu().numpy())
    for r in range(9):
        assert (d[r, f[r]:] == -1).all() and (s[r, f[r]:] == 0).all()


# ------------------------------------------------------------------------------------------------ 7. the miner
def _gpu_miner(encode, index_type, dev, **kw):
    from src.preprocessing.miners import BGEM3HardNegativeMiner
    from tests.test_ivf_host import golden
    miner = BGEM3HardNegativeMiner(device=str(dev), encode=encode)
    miner.build_index(list(golden()[0]["documents"]), index_type=index_type, **kw)
    return miner


def test_miner_on_the_gpu_reproduces_the_reference_results(dev):
    from snx.retrieval import DenseIndex, IvfFlatIndex
    from tests.test_ivf_host import golden, run_golden_cases
    made = []

    def make(index_type, **kw):
        def f(encode):
            made.append(_gpu_miner(encode, index_type, dev, **kw))
            return made[-1]
        return f
    run_golden_cases(make("flat"))
    run_golden_cases(make("ivf", nlist=4, nprobe=4))         # every list probed: the flat index's results
    assert isinstance(made[0]._index, DenseIndex) and isinstance(made[1]._index, IvfFlatIndex)
    g, encode = golden()
    miner = _gpu_miner(encode, "ivf", dev, nlist=4)          # nprobe 1, FAISS's default
    idx = miner._index
    assert idx.nprobe == 1 and idx.nlist == 4
    queries, positives = g["cases"][0]["queries"], g["cases"][0]["positives"]
    res = miner.mine_negatives(queries, positives, num_negatives=5, min_score=0.2, max_score=0.9)
    ptr, doc = idx.list_ptr.cpu().numpy(), idx.list_doc.cpu().numpy()
    assert np.diff(ptr).max() < len(g["documents"])          # fewer docs in a list than slots asked for
    probed = idx.probe(_t(encode(queries), dev), 1)[1].cpu().numpy()[:, 0]
    for r, c in zip(res, probed):
        inside = {g["documents"][d] for d in doc[ptr[c]:ptr[c + 1]]}
        assert set(r.negatives) <= inside and not set(r.negatives) & set(positives) and r.query not in r.negatives
        assert all(0.2 <= s <= 0.9 for s in r.negative_scores) and len(r.negatives) == len(r.negative_scores)
    assert any(r.negatives for r in res)


# ------------------------------------------------------------------------------------------------ 8. errors
def test_argument_errors(dev):
    from snx.retrieval import IvfFlatIndex
    idx = IvfFlatIndex(8, 2, dev, nprobe=2)
    good = torch.zeros((4, 8), device=dev)
    q = torch.ones((2, 8), device=dev)
    for bad in (torch.zeros((4, 8), dtype=torch.float64, device=dev), torch.zeros((4, 7), device=dev),
                torch.zeros(8, device=dev), torch.zeros((4, 8)), torch.full((4, 8), float("nan"), device=dev),
                torch.full((4, 8), float("inf"), device=dev), np.zeros((4, 8), np.float32)):
        with pytest.raises(ValueError):
            idx.add(bad)
        with pytest.raises(ValueError):
            idx.train(bad)
        with pytest.raises(ValueError):
            idx.set_centroids(bad)
    with pytest.raises(ValueError):
        idx.train(good[:1])                                  # fewer rows than lists
    idx.add(good)
    idx.set_centroids(torch.eye(8, device=dev)[:2])
    for call in (lambda: idx.search(q, 1), lambda: idx.search_band(q, 0, 1),
                 lambda: idx.pair_scores(q, torch.zeros((1, 2), dtype=torch.long, device=dev))):
        with pytest.raises(RuntimeError):
            call()
    idx.build()
    for b in (q.double(), q[:, :7], q.cpu(), torch.full((2, 8), float("-inf"), device=dev)):
        with pytest.raises(ValueError):
            idx.search(b, 1)
        with pytest.raises(ValueError):
            idx.search_band(b, 0, 1)
        with pytest.raises(ValueError):
            idx.probe(b)
        with pytest.raises(ValueError):
            idx.pair_scores(b, torch.zeros((1, 2), dtype=torch.long, device=dev))
    for k in (0, 1025, -1):
        with pytest.raises(ValueError):
            idx.search(q, k)
    for lo, hi in ((-1, 1), (0, 0), (5, 5), (6, 5), (0, 1025)):
        with pytest.raises(ValueError):
            idx.search_band(q, lo, hi)
    for nprobe in (0, 3, True, 1.5):
        with pytest.raises(ValueError):
            idx.search(q, 1, nprobe=nprobe)
        with pytest.raises(ValueError):
            idx.probe(q, nprobe)
    with pytest.raises(ValueError):
        idx.search(q, 1, query_slice=-1)
    with pytest.raises(ValueError):
        idx.search_band(q, 0, 1, ceiling=torch.tensor([float("nan"), 0.0], device=dev))
    with pytest.raises(ValueError):
        idx.search_band(q, 0, 1, exclude=[[4], []])
    for p in (torch.tensor([[0, 4]], device=dev), torch.tensor([[2, 0]], device=dev), torch.tensor([0, 1], device=dev),
              torch.tensor([[0.0, 1.0]], device=dev)):
        with pytest.raises(ValueError):
            idx.pair_scores(q, p)
    # and what is valid at the edges runs: an empty query set, k > nd, chunk_docs accepted and ignored, a new batch
    sc, dc = idx.search(q[:0], 3)
    assert sc.shape == (0, 3) and dc.shape == (0, 3)
    sc, dc = idx.search(q, 6)                                # all docs are zero rows: list 0, tied, by id
    assert dc.cpu().numpy().tolist() == [[0, 1, 2, 3, -1, -1]] * 2
    assert idx.search_band(q, 0, 6, chunk_docs=4096)[2].cpu().tolist() == [4, 4]
    idx.add(good)
    with pytest.raises(RuntimeError):
        idx.search(q, 1)
    assert idx.build().search(q, 8)[1].cpu().numpy().tolist() == [[0, 1, 2, 3, 4, 5, 6, 7]] * 2


# ------------------------------------------------------------------------------------------------ 9. CLI
def test_mine_cli_with_every_list_probed_writes_the_flat_files(dev, tmp_path):
    from src.train.cli import teacher_scores
    from tests.test_dense_host import mine_case
    emb, tix, files = mine_case(tmp_path)
    np.save(tmp_path / "emb.npy", emb)
    (tmp_path / "tix.json").write_text(json.dumps(tix))
    base = ["mine", "--embeddings", str(tmp_path / "emb.npy"), "--text-index", str(tmp_path / "tix.json"),
            "--input-pattern", str(tmp_path / "in" / "train_*.jsonl"), "--val-pattern", str(tmp_path / "in" / "none.jsonl"),
            "--k", "2", "--rank-start", "1", "--rank-end", "3", "--device", str(dev)]
    a = teacher_scores.main(base + ["--output-dir", str(tmp_path / "flat")])
    b = teacher_scores.main(base + ["--output-dir", str(tmp_path / "ivf"), "--index", "ivf", "--nlist", "3", "--nprobe", "3"])
    assert a == b
    for name in ("train_0.jsonl", "train_1.jsonl"):
        assert (tmp_path / "flat" / name).read_bytes() == (tmp_path / "ivf" / name).read_bytes()

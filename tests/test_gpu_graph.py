"""GPU checks of the graph dense retrieval (csrc/graph.hip, include/snx.h "graph dense retrieval"):
snx.retrieval.GraphIndex, ``teacher_scores mine --index graph`` and ``eval_hybrid --dense-index graph``.

Everything is compared exactly -- int32 ids, iteration counts and fp32 BITS -- with the plain-Python stand-in
tests/graph_reference.py, which keeps the exact set of scored docs.  On dyadic data (integers in [-8, 8] divided by 8: every
partial sum of the score chain is exact) the stand-in scores in numpy; on random fp32 data it reads the bits of
``GraphIndex.pair_scores`` and takes the neighbour lists from the GPU, which are held to ``DenseIndex`` separately.

Shapes: 1500 docs (six workgroups' worth of a 256-row launch, not a multiple of it), D 20 (no multiple of the 16-wide K
tile of the exact search) and 64, D 22 where the 16-byte row loads do not apply; ef 16, 100 and 1024 (the whole pool
buffer), width 1, 4 and 8; (degree, knn) from (8, 16) to the caps (64, 128)."""
import json

import numpy as np
import pytest
import torch

from tests import graph_reference as R

pytestmark = pytest.mark.gpu

ND, NQ = 1500, 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(x):
    return x.cpu().numpy()


def _dyadic(rng, n, D):
    return (rng.integers(-8, 9, size=(n, D)) / 8.0).astype(np.float32)


def _gpu_index(E, dev, batches=3, neighbors=None, **kw):
    from snx.retrieval import GraphIndex
    idx = GraphIndex(E.shape[1], dev, **kw)
    for part in np.array_split(E, batches):
        idx.add(_t(part, dev))
    return idx.build(neighbors=None if neighbors is None else _t(neighbors, dev))


def _standin(E, neighbors=None, score=None, **kw):
    ref = R.NumpyGraphIndex(E.shape[1], score=score, **kw)
    ref.add(E)
    return ref.build(neighbors=neighbors)


def _gpu_scores(idx, Q, dev):
    """score(q_row, ids) of the stand-in on the bits of GraphIndex.pair_scores: the whole [nq, nd] table, read once."""
    nq, nd = Q.shape[0], idx.num_docs
    pairs = torch.stack([torch.arange(nq, device=dev).repeat_interleave(nd), torch.arange(nd, device=dev).repeat(nq)], 1)
    S = _n(idx.pair_scores(_t(Q, dev), pairs)).reshape(nq, nd)
    rows = {Q[i].tobytes(): i for i in range(nq)}
    return lambda q_row, ids: S[rows[q_row.tobytes()], np.asarray(ids, np.int64)]


def _equal_search(idx, ref, Q, dev, k, **kw):
    s, d = idx.search(_t(Q, dev), k, **kw)
    rs, rd = ref.search(Q, k, **kw)
    assert np.array_equal(_n(d), rd)
    assert np.array_equal(_bits(_n(s)), _bits(rs))
    assert np.array_equal(_n(idx.last_iterations), ref.last_iterations)


_CACHE = {}


def _dyadic_pair(D, dev, degree=8, knn=16):
    """(E, Q, GPU index, stand-in) on dyadic data, built once per shape."""
    key = (D, degree, knn)
    if key not in _CACHE:
        rng = np.random.default_rng(D)
        E, Q = _dyadic(rng, ND, D), _dyadic(rng, NQ, D)
        _CACHE[key] = (E, Q, _gpu_index(E, dev, degree=degree, knn=knn), _standin(E, degree=degree, knn=knn))
    return _CACHE[key]


def _same_structure(idx, ref):
    st, rs = idx.structure(), ref.structure()
    for name in ("neighbors", "forward", "graph", "entry"):
        assert st[name].dtype == torch.int32 and np.array_equal(_n(st[name]), rs[name]), name


# ------------------------------------------------------------------------------------------------ 1. structure
@pytest.mark.parametrize("D,degree,knn", [(20, 8, 16), (64, 32, 64)])
def test_structure_equals_the_stand_in_on_dyadic_data(dev, D, degree, knn):
    E, Q, idx, ref = _dyadic_pair(D, dev, degree, knn)
    _same_structure(idx, ref)
    g = _n(idx.graph)
    assert (g >= 0).all() and (g != np.arange(ND)[:, None]).all()
    assert all(len(set(row)) == degree for row in g[::97])
    assert not np.array_equal(_n(idx.forward), g)            # the reverse edges took slots


def test_structure_at_the_caps_on_random_data(dev):
    from snx.retrieval import DenseIndex
    rng = np.random.default_rng(3)
    E = rng.standard_normal((ND, 20)).astype(np.float32)
    idx = _gpu_index(E, dev, degree=64, knn=128)
    N = _n(idx.neighbors)
    # the lists are the exact band search with the row's own doc excluded
    dense = DenseIndex(20, dev)
    dense.add(_t(E, dev))
    dense.build()
    rows = [0, 1, 255, 256, 777, ND - 1]
    _, want, found = dense.search_band(_t(E[rows], dev), 0, 128, exclude=[[r] for r in rows])
    assert np.array_equal(N[rows], _n(want)) and (_n(found) == 128).all()
    assert (N != np.arange(ND)[:, None]).all() and (N >= 0).all()
    ref = _standin(E, neighbors=N, degree=64, knn=128)
    assert np.array_equal(_n(idx.forward), ref.forward) and np.array_equal(_n(idx.graph), ref.graph)


def test_fewer_docs_than_knn_gives_padded_rows(dev):
    rng = np.random.default_rng(4)
    E, Q = _dyadic(rng, 10, 20), _dyadic(rng, 3, 20)
    idx, ref = _gpu_index(E, dev, batches=2, degree=8, knn=16), _standin(E, degree=8, knn=16)
    _same_structure(idx, ref)
    assert (_n(idx.neighbors)[:, 9:] == -1).all() and (_n(idx.neighbors)[:, :9] >= 0).all()
    assert (_n(idx.graph) >= 0).all()                        # nine neighbours each: every row is full
    _equal_search(idx, ref, Q, dev, 12, ef=16)
    s, d = idx.search(_t(Q, dev), 12, ef=16)
    assert (_n(d)[:, 10:] == -1).all() and (_n(s)[:, 10:] == 0).all() and (np.sort(_n(d)[:, :10], 1) == np.arange(10)).all()
    one = _gpu_index(E[:1], dev, batches=1, degree=2, knn=2)
    assert _n(one.graph).tolist() == [[-1, -1]] and _n(one.search(_t(Q, dev), 2)[1]).tolist() == [[0, -1]] * 3


def test_crafted_neighbors_full_of_detour_ties(dev):
    nd, knn = 301, 16
    rng = np.random.default_rng(5)
    E, Q = _dyadic(rng, nd, 20), _dyadic(rng, NQ, 20)
    rings = np.array([[(u + s) % nd for s in range(1, knn + 1)] for u in range(nd)], np.int32)     # detour(u, j) = j
    # odd offsets: the difference of two of them is even, so no neighbour lists another and every detour count is 0
    spread = np.array([[(u + 2 * s - 1) % nd for s in range(1, knn + 1)] for u in range(nd)], np.int32)
    short = rings.copy()
    short[::3, 5:] = -1                                      # rows of five ids among full ones
    for N in (rings, spread, short):
        idx, ref = _gpu_index(E, dev, neighbors=N, degree=8, knn=knn), _standin(E, neighbors=N, degree=8, knn=knn)
        _same_structure(idx, ref)
        _equal_search(idx, ref, Q, dev, 10, ef=32, width=4)
    assert R.detours(spread, 0) == [0] * knn and R.detours(rings, 0) == list(range(knn))


# ------------------------------------------------------------------------------------------------ 2. search
@pytest.mark.parametrize("width", [1, 4, 8])
@pytest.mark.parametrize("ef", [16, 100, 1024])
@pytest.mark.parametrize("D", [20, 64])
def test_search_equals_the_stand_in_on_dyadic_data(dev, D, ef, width):
    E, Q, idx, ref = _dyadic_pair(D, dev)
    q = Q[:4] if ef == 1024 else Q                           # the stand-in sorts a pool of 1024 per iteration
    s, d = idx.search(_t(q, dev), ef, ef=ef, width=width)
    pools = ref.pools(q, ef, width)
    assert np.array_equal(_n(idx.last_iterations), ref.last_iterations)
    for k in (1, 10, ef):
        rows = [R.band(p, 0, k) for p in pools]
        assert np.array_equal(_n(d)[:, :k], np.stack([r[1] for r in rows]))
        assert np.array_equal(_bits(_n(s)[:, :k]), _bits(np.stack([r[0] for r in rows])))
    sk, dk = idx.search(_t(q, dev), 10, ef=ef, width=width)
    assert torch.equal(dk, d[:, :10]) and torch.equal(sk.view(torch.int32), s[:, :10].contiguous().view(torch.int32))


@pytest.mark.parametrize("D", [20, 22, 64])
def test_search_on_random_data_equals_the_stand_in_on_pair_score_bits(dev, D):
    rng = np.random.default_rng(10 + D)
    E, Q = rng.standard_normal((ND, D)).astype(np.float32), rng.standard_normal((NQ, D)).astype(np.float32)
    idx = _gpu_index(E, dev, degree=16, knn=32)
    ref = _standin(E, neighbors=_n(idx.neighbors), score=_gpu_scores(idx, Q, dev), degree=16, knn=32)
    assert np.array_equal(_n(idx.graph), ref.graph)
    for ef, width in ((16, 1), (100, 4), (200, 8)):
        _equal_search(idx, ref, Q, dev, min(ef, 50), ef=ef, width=width)
    _equal_search(idx, ref, Q, dev, 10, ef=100, width=4, max_iter=3)
    assert (_n(idx.last_iterations) == 3).all()
    s, d = idx.search(_t(Q, dev), 10)                        # every returned score is pair_scores'
    pairs = torch.stack([torch.arange(NQ, device=dev).repeat_interleave(10), d.reshape(-1).long()], 1)
    assert torch.equal(idx.pair_scores(_t(Q, dev), pairs).view(torch.int32), s.reshape(-1).view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. identity
@pytest.mark.parametrize("D", [20, 22, 64])
def test_every_doc_a_seed_is_the_dense_index_bit_for_bit(dev, D):
    from snx.retrieval import DenseIndex
    nd, nq = 700, 33
    rng = np.random.default_rng(D)
    E, Q = rng.standard_normal((nd, D)).astype(np.float32), rng.standard_normal((nq, D)).astype(np.float32)
    E[100:140] = E[7]                                        # forty docs tied for every query
    idx = _gpu_index(E, dev, degree=8, knn=16)
    dense = DenseIndex(D, dev)
    dense.add(_t(E, dev))
    dense.build()
    q = _t(Q, dev)
    for k in (1, 10, 700, 1024):
        s, d = idx.search(q, k, ef=1024)
        ws, wd, _, _ = dense.search(q, k)
        assert torch.equal(d, wd) and torch.equal(s.view(torch.int32), ws.view(torch.int32))
    top = _n(dense.search(q, 30)[1])
    exclude = [sorted(set(top[i, ::2].tolist()) | {int(rng.integers(nd))}) for i in range(nq)]
    exclude[5] = []
    ceiling = dense.search(q, 30)[0][:, 12].clone()
    ceiling[3], ceiling[4] = float("inf"), -1e30
    for lo, hi in ((0, 1), (10, 50), (600, 1024)):
        for ex, cl in ((exclude, None), (None, ceiling), (exclude, ceiling)):
            got = idx.search_band(q, lo, hi, exclude=ex, ceiling=cl, ef=1024)
            want = dense.search_band(q, lo, hi, exclude=ex, ceiling=cl)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want)), (lo, hi)


# ------------------------------------------------------------------------------------------------ 4. ties
def test_hundreds_of_equal_rows_resolve_by_doc_id(dev):
    rng = np.random.default_rng(6)
    E, Q = _dyadic(rng, ND, 20), _dyadic(rng, NQ, 20)
    same = rng.permutation(ND)[:400]
    E[same] = E[same[0]]                                     # 400 copies of one row, spread over the ids
    Q[0] = E[same[0]]
    idx, ref = _gpu_index(E, dev, degree=8, knn=16), _standin(E, degree=8, knn=16)
    _same_structure(idx, ref)
    for ef, width in ((16, 1), (100, 4), (1024, 8)):
        _equal_search(idx, ref, Q[:4], dev, min(ef, 500), ef=ef, width=width)
    s, d = idx.search(_t(Q[:1], dev), 300, ef=1024)
    d, s = _n(d)[0], _n(s)[0]
    assert max(np.sum(_bits(s) == b) for b in np.unique(_bits(s))) >= 100
    assert all((np.diff(d[np.flatnonzero(_bits(s) == b)]) > 0).all() for b in np.unique(_bits(s)))


def test_a_doc_under_several_parents_of_one_iteration_is_scored_once(dev):
    nd, knn = 400, 16
    rng = np.random.default_rng(7)
    E, Q = _dyadic(rng, nd, 20), _dyadic(rng, NQ, 20)
    # every node lists the same sixteen hubs (the hubs list each other and one outsider): all parents share their rows
    N = np.tile(np.arange(knn, dtype=np.int32), (nd, 1))
    for u in range(knn):
        N[u] = [x for x in range(knn + 1) if x != u]
    idx, ref = _gpu_index(E, dev, neighbors=N, degree=8, knn=knn), _standin(E, neighbors=N, degree=8, knn=knn)
    _same_structure(idx, ref)
    for width in (1, 4, 8):
        _equal_search(idx, ref, Q, dev, 30, ef=64, width=width)
        d = _n(idx.search(_t(Q, dev), 64, ef=64, width=width)[1])
        assert all(len(set(row[row >= 0])) == (row >= 0).sum() for row in d)


def test_a_walk_far_larger_than_the_visited_table(dev):
    nd, D, nq = 20000, 20, 3
    rng = np.random.default_rng(8)
    E, Q = rng.standard_normal((nd, D)).astype(np.float32), rng.standard_normal((nq, D)).astype(np.float32)
    idx = _gpu_index(E, dev, degree=64, knn=64)
    ref = R.NumpyGraphIndex(D, degree=64, knn=64, score=_gpu_scores(idx, Q, dev))
    ref.num_docs, ref.graph = nd, _n(idx.graph)              # the walk alone: the structure has its own tests
    _equal_search(idx, ref, Q, dev, 1024, ef=1024, width=8)
    scored = 1024 + 512 * int(ref.last_iterations.min())
    print("iterations", ref.last_iterations.tolist(), "ids met per query, at most", scored)
    assert ref.last_iterations.min() * 8 >= 1024             # every pool entry was expanded: far more than 4096 ids met


# ------------------------------------------------------------------------------------------------ 5. independence
def test_slicing_budget_and_batches_change_no_bit(dev, monkeypatch):
    from snx.retrieval import graph
    E, Q, idx, _ = _dyadic_pair(64, dev)
    rng = np.random.default_rng(9)
    Q = _dyadic(rng, 70, 64)
    q = _t(Q, dev)
    want = idx.search(q, 50, ef=100)
    iters = idx.last_iterations.clone()
    top = _n(want[1])
    exclude = [top[i, :7].tolist() for i in range(70)]
    ceiling = want[0][:, 3].clone()
    band = idx.search_band(q, 2, 40, exclude=exclude, ceiling=ceiling, ef=100)
    st = {k: v.clone() for k, v in idx.structure().items()}

    def same(a, b):
        return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    for qs in (1, 7, 64):
        assert same(idx.search(q, 50, ef=100, query_slice=qs), want) and torch.equal(idx.last_iterations, iters)
        assert same(idx.search_band(q, 2, 40, exclude=exclude, ceiling=ceiling, ef=100, query_slice=qs), band)
    monkeypatch.setattr(graph, "_GRAPH_WS_BUDGET", 1 << 12)  # a few queries per launch; the build's lists in many slices
    assert same(idx.search(q, 50, ef=100), want) and same(idx.search_band(q, 2, 40, exclude=exclude, ceiling=ceiling, ef=100),
                                                          band)
    for batches in (1, 7):
        other = _gpu_index(E, dev, batches=batches, degree=8, knn=16)
        assert all(torch.equal(other.structure()[k], st[k]) for k in st)
        assert same(other.search(q, 50, ef=100), want)


# ------------------------------------------------------------------------------------------------ 6. band
@pytest.mark.parametrize("lo,hi", [(0, 1), (10, 50), (900, 1024)])
def test_band_equals_the_stand_in(dev, lo, hi):
    E, Q, idx, ref = _dyadic_pair(20, dev)
    Q = Q[:5]
    ef = 1024 if hi > 100 else 100
    pools = ref.pools(Q, ef, 4)
    plain = ref.last_iterations.copy()
    rng = np.random.default_rng(hi)
    exclude = [sorted({d for _, d in p[::3]} | {int(rng.integers(ND))}) for p in pools]
    exclude[1] = [d for _, d in pools[1]]                    # the whole pool: nothing is left
    exclude[2] = []
    ceiling = np.array([p[min(len(p) - 1, 20)][0] for p in pools], np.float32)
    ceiling[3] = np.nan                                      # admits nothing
    ceiling[4] = np.inf
    for ex, cl in ((exclude, None), (None, ceiling), (exclude, ceiling)):
        s, d, f = idx.search_band(_t(Q, dev), lo, hi, exclude=ex, ceiling=None if cl is None else _t(cl, dev), ef=ef)
        rs, rd, rf = ref.search_band(Q, lo, hi, exclude=ex, ceiling=cl, ef=ef)
        assert np.array_equal(_n(d), rd) and np.array_equal(_bits(_n(s)), _bits(rs)) and np.array_equal(_n(f), rf)
        assert np.array_equal(_n(idx.last_iterations), plain)               # the filter does not touch the walk
        if ex is not None:
            assert rf[1] == 0 and (_n(d)[1] == -1).all()
        if cl is not None:
            assert rf[3] == 0 and (_n(s)[3] == 0).all()


# ------------------------------------------------------------------------------------------------ 7. recall
def test_recall_of_the_definition_on_a_gaussian_mixture(dev):
    """The stand-in's own CPU run on this corpus gave recall@10 = 0.98 at ef 16, 32, 64, 100 and 128 (default nentry, 312
    entry docs; mean iterations 5.0 at ef 16 and 32.9 at ef 128): the floor is 0.05 under it.  The corpus is too small for
    any claim about speed."""
    rng = np.random.RandomState(1234)
    centres = rng.randn(150, 32)

    def draw(n):
        x = centres[rng.randint(0, 150, n)] + 0.5 * rng.randn(n, 32)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    E, Q = draw(6000), draw(50)
    idx = _gpu_index(E, dev, degree=16, knn=32, width=4)
    ref = _standin(E, neighbors=_n(idx.neighbors), score=_gpu_scores(idx, Q, dev), degree=16, knn=32, width=4)
    assert np.array_equal(_n(idx.graph), ref.graph)
    S = R.scores64(Q, E)
    ids = np.arange(6000)
    exact = [set(ids[np.lexsort((ids, -S[i].astype(np.float64)))][:10].tolist()) for i in range(50)]
    for ef in (16, 128):
        _equal_search(idx, ref, Q, dev, 10, ef=ef)
        rd = ref.search(Q, 10, ef=ef)[1]
        recall = float(np.mean([len(exact[i] & set(rd[i].tolist())) / 10 for i in range(50)]))
        print("ef", ef, "recall@10", recall, "mean iterations", float(ref.last_iterations.mean()))
        assert recall >= 0.93


# ------------------------------------------------------------------------------------------------ 8. errors, CLI
def test_argument_errors(dev):
    from snx.retrieval import GraphIndex
    E, Q, idx, _ = _dyadic_pair(20, dev)
    q = _t(Q, dev)
    bad_calls = [lambda: idx.search(q, 0), lambda: idx.search(q, 1025), lambda: idx.search(q, 101),        # k > ef = 100
                 lambda: idx.search(q, 10, ef=9), lambda: idx.search(q, 1, ef=0), lambda: idx.search(q, 1, ef=1025),
                 lambda: idx.search(q, 1, ef=16.0), lambda: idx.search(q, 1, width=0), lambda: idx.search(q, 1, width=9),
                 lambda: idx.search(q, 1, width=True), lambda: idx.search(q, 1, max_iter=-1),
                 lambda: idx.search(q, 1, max_iter=1.5), lambda: idx.search(q, 1, query_slice=-1),
                 lambda: idx.search(q.double(), 1), lambda: idx.search(q[:, :19], 1), lambda: idx.search(q.cpu(), 1),
                 lambda: idx.search(torch.full_like(q, float("inf")), 1),
                 lambda: idx.search_band(q, 5, 5), lambda: idx.search_band(q, 0, 101), lambda: idx.search_band(q, -1, 4),
                 lambda: idx.search_band(q, 0, 4, exclude=[[0]]), lambda: idx.search_band(q, 0, 4, exclude=[[ND]] * NQ),
                 lambda: idx.search_band(q, 0, 4, ceiling=torch.zeros(NQ + 1, device=dev)),
                 lambda: idx.search_band(q, 0, 4, ceiling=torch.zeros(NQ, dtype=torch.float64, device=dev)),
                 lambda: idx.pair_scores(q, torch.tensor([[0, ND]], device=dev)),
                 lambda: idx.pair_scores(q, torch.zeros((1, 3), dtype=torch.long, device=dev))]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    small = GraphIndex(20, dev, degree=4, knn=6)
    small.add(_t(E[:50], dev))
    N = _n(_gpu_index(E[:50], dev, degree=4, knn=6).neighbors)
    twice, own, late, far = N.copy(), N.copy(), N.copy(), N.copy()
    twice[3, 1] = twice[3, 0]
    own[4, 2] = 4
    late[5, 1] = -1
    far[6, 0] = 50
    for bad in (twice, own, late, far, N[:49], N[:, :5], N.astype(np.int64)):
        with pytest.raises(ValueError):
            small.build(neighbors=_t(bad, dev))
    with pytest.raises(ValueError):
        small.build(neighbors=torch.from_numpy(N))           # on the host
    with pytest.raises(RuntimeError):
        small.search(q, 1)
    ok = late.copy()
    ok[5, 1:] = -1
    assert small.build(neighbors=_t(ok, dev)).built and _n(small.search(q, 4)[1]).shape == (NQ, 4)
    small.add(_t(E[50:60], dev))
    with pytest.raises(RuntimeError):                        # a new batch invalidates the built index
        small.search(q, 1)


def test_mine_cli_with_every_doc_a_seed_writes_the_flat_files(dev, tmp_path):
    from src.train.cli import teacher_scores
    from tests.test_dense_host import mine_case
    emb, tix, files = mine_case(tmp_path)
    np.save(tmp_path / "emb.npy", emb)
    (tmp_path / "tix.json").write_text(json.dumps(tix))
    base = ["mine", "--embeddings", str(tmp_path / "emb.npy"), "--text-index", str(tmp_path / "tix.json"),
            "--input-pattern", str(tmp_path / "in" / "train_*.jsonl"), "--val-pattern", str(tmp_path / "in" / "none.jsonl"),
            "--k", "2", "--rank-start", "1", "--rank-end", "3", "--device", str(dev)]
    assert len(emb) <= 100                                   # the default ef covers every doc
    a = teacher_scores.main(base + ["--output-dir", str(tmp_path / "flat")])
    b = teacher_scores.main(base + ["--output-dir", str(tmp_path / "graph"), "--index", "graph", "--degree", "4"])
    assert a == b
    for name in ("train_0.jsonl", "train_1.jsonl"):
        assert (tmp_path / "flat" / name).read_bytes() == (tmp_path / "graph" / name).read_bytes()


def test_eval_hybrid_graph_dense_index_emits_the_extra_fields(dev, tmp_path):
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
            "--doc-max-length", "32", "--batch-size", "16", "--retrieval-k", "20"]
    probe = eval_hybrid.main(argv)
    nq, nd = probe[0]["num_queries"], probe[0]["num_docs"]
    rng = np.random.default_rng(8)
    np.savez(tmp_path / "emb.npz", docs=_dyadic(rng, nd, 24), queries=_dyadic(rng, nq, 24))
    dense = ["--dense-embeddings", str(tmp_path / "emb.npz")]
    flat = eval_hybrid.main(argv + dense)
    assert nd <= 1024
    whole = eval_hybrid.main(argv + dense + ["--dense-index", "graph", "--ef", "1024", "--degree", "8"])
    extra = {"dense_index": "graph", "ef": 1024, "degree": 8, "recall_vs_exact@10": 1.0, "recall_vs_exact@20": 1.0}
    line = next(x for x in whole if x["method"] == "dense")
    assert {k: line[k] for k in extra} == extra and line["mean_iterations"] > 0
    strip = [{k: v for k, v in x.items() if k not in extra and k != "mean_iterations"} for x in whole]
    assert strip == flat                                     # every doc a seed: the flat run's lines
    part = eval_hybrid.main(argv + dense + ["--dense-index", "graph", "--degree", "8"])
    line = next(x for x in part if x["method"] == "dense")
    assert line["ef"] == 100 and 0.0 < line["recall_vs_exact@10"] <= 1.0 and 0.0 < line["recall_vs_exact@20"] <= 1.0
    assert all("recall_vs_exact@10" not in x for x in part if x["method"] != "dense")

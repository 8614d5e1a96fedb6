"""CPU checks of the graph dense retrieval (include/snx.h "graph dense retrieval"): the plain-Python stand-in
tests/graph_reference.py against hand-worked cases of the definition, the argument checks of snx.retrieval.GraphIndex and
of the C entry points that need no GPU, and the command lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import graph_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# six nodes, knn = 4: every row written by hand
SIX = np.array([[1, 2, 3, 4], [2, 0, 3, 5], [3, 1, 0, 4], [2, 4, 1, 0], [3, 5, 2, 0], [4, 3, 1, 2]], np.int32)


def _dyadic(rng, n, D):
    return (rng.integers(-8, 9, size=(n, D)) / 8.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ structure
def test_detours_of_six_nodes_by_hand():
    # node 0, neighbours 1 2 3 4.  column 1 (doc 2): 1 lists 2 at column 0 < 1 -> 1.  column 2 (doc 3): 1 lists 3 at
    # column 2, not < 2; 2 lists 3 at column 0 -> 1.  column 3 (doc 4): 1 does not list 4; 2 lists it at column 3, not
    # < 3; 3 lists it at column 1 -> 1.
    assert R.detours(SIX, 0) == [0, 1, 1, 1]
    # node 1, neighbours 2 0 3 5.  doc 0: 2 lists 0 at column 2, not < 1.  doc 3: 2 lists 3 at column 0 -> 1; 0 lists 3 at
    # column 2, not < 2.  doc 5: nobody in front lists it.
    assert R.detours(SIX, 1) == [0, 0, 1, 0]
    assert R.detours(SIX, 2) == [0, 0, 1, 1]
    # node 3, neighbours 2 4 1 0.  doc 0: 2 lists 0 at column 2 < 3, 4 lists 0 at column 3 (not < 3), 1 lists 0 at 1 -> 2
    assert R.detours(SIX, 3) == [0, 0, 1, 2]
    assert R.detours(SIX, 4) == [0, 0, 1, 1]
    # node 5, neighbours 4 3 1 2.  doc 3: 4 lists 3 first -> 1.  doc 1: 4 does not list 1, 3 lists 1 at column 2, not < 2
    # -> 0.  doc 2: 4 lists 2 at column 2, 3 and 1 list 2 first -> 3
    assert R.detours(SIX, 5) == [0, 1, 0, 3]
    F, G = R.optimize(SIX, 2)
    # (detour, column) ascending: node 0 keeps columns 0, 1; node 1 columns 0, 1; node 5 columns 0 and 2 (doc 1 passes doc 3)
    assert F.tolist() == [[1, 2], [2, 0], [3, 1], [2, 4], [3, 5], [4, 1]]
    # column 0 of F names 1 2 3 2 3 4 for u = 0 .. 5, column 1 names 2 0 1 4 5 1
    assert R.reverse_lists(F) == [[1], [0, 2], [1, 3], [2, 4], [5, 3], [4]]
    assert G.tolist() == [[1, 2], [2, 0], [3, 1], [2, 4], [3, 5], [4, 1]]     # F[v][0], then R[v][0] or, if taken, F[v][1]
    F4, G4 = R.optimize(SIX, 4)
    assert F4[5].tolist() == [4, 1, 3, 2] and F4[3].tolist() == [2, 4, 1, 0]
    assert R.reverse_lists(F4)[5] == [4, 1] and G4[5].tolist() == [4, 1, 3, 2]


def test_a_row_shorter_than_knn():
    E = np.array([[1, 0], [0.5, 0.5], [0, 1]], np.float32)
    N = R.neighbor_lists(R.scores64(E, E), 4)
    assert N.tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]]    # row 1 ties 0 and 2: lowest id first
    # node 0: 1 lists 2 at column 1, not < 1.  node 2, neighbours 1 0: 1 lists 0 first -> 1
    assert R.detours(N, 0) == [0, 0] and R.detours(N, 1) == [0, 0] and R.detours(N, 2) == [0, 1]
    F, G = R.optimize(N, 4)
    assert F.tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]]
    assert G.tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]]
    one = R.neighbor_lists(np.zeros((1, 1), np.float32), 2)
    assert one.tolist() == [[-1, -1]] and R.optimize(one, 2)[1].tolist() == [[-1, -1]]


def test_interleave():
    assert R.interleave([1, 2, 3], [2, 9], 4) == [1, 2, 9, 3]               # R's 2 is taken already; R runs out, F goes on
    assert R.interleave([1, 2, 3, 4], [7], 3) == [1, 7, 2]
    assert R.interleave([1], [5, 6, 7], 4) == [1, 5, 6, 7]                   # F runs out, R goes on
    assert R.interleave([1, 2], [1, 2], 4) == [1, 2]
    assert R.interleave([], [], 2) == []
    # a hub: every node points at 0 first, R[0] keeps the first `degree` of them in (column, node) order
    F = np.array([[1, 2], [0, 2], [0, 1], [0, 1], [0, 2]], np.int32)
    assert R.reverse_lists(F)[0] == [1, 2] and R.reverse_lists(F)[1] == [0, 2] and R.reverse_lists(F)[2] == [0, 1]


def test_forward_ties_resolve_by_column():
    # a ring of cliques in which every detour count is equal: the forward list is the row's first `degree` columns
    nd, knn = 12, 4
    N = np.array([[(u + s) % nd for s in (1, 2, 3, 4)] for u in range(nd)], np.int32)
    det = [R.detours(N, u) for u in range(nd)]
    assert all(d == det[0] for d in det) and det[0] == [0, 1, 2, 3]
    N2 = np.array([[(u + s) % nd for s in (1, 5, 9, 3)] for u in range(nd)], np.int32)   # no two-hop routes in front
    assert R.detours(N2, 0) == [0, 0, 0, 0] and R.optimize(N2, 2)[0][0].tolist() == [1, 5]


def test_entry_sample():
    assert R.entry_sample(10, 4).tolist() == [0, 2, 5, 7]
    assert R.entry_sample(7, 7).tolist() == list(range(7))
    assert R.default_nentry(1500) == 4 * 39 and R.default_nentry(1600) == 160 and R.default_nentry(1) == 4
    assert R.clamp_nentry(None, 100, 1500) == 156 and R.clamp_nentry(None, 1024, 1500) == 1024
    assert R.clamp_nentry(None, 1024, 700) == 700 and R.clamp_nentry(5000, 16, 700) == 700 and R.clamp_nentry(3, 16, 700) == 16
    from snx.retrieval import entry_sample
    assert entry_sample(2 ** 31 - 1, 5).tolist() == [(i * (2 ** 31 - 1)) // 5 for i in range(5)]


# ------------------------------------------------------------------------------------------------ walk
def _index(nd=300, D=6, seed=0, **kw):
    rng = np.random.default_rng(seed)
    E, Q = _dyadic(rng, nd, D), _dyadic(rng, 9, D)
    idx = R.NumpyGraphIndex(D, **kw)
    idx.add(E[:100])
    idx.add(E[100:])
    return idx.build(), E, Q


def _exact(S, k):
    ids = np.arange(S.shape[1])
    return np.stack([ids[np.lexsort((ids, -row.astype(np.float64)))][:k] for row in S])


def test_every_doc_a_seed_is_the_exact_search():
    idx, E, Q = _index(degree=8, knn=16)
    S = R.scores64(Q, E)
    s, d = idx.search(Q, 300, ef=300)
    want = _exact(S, 300)
    assert np.array_equal(d, want) and np.array_equal(s, np.take_along_axis(S, want, 1))
    s, d = idx.search(Q, 320, ef=1024)                       # more slots than docs
    assert np.array_equal(d[:, :300], want) and (d[:, 300:] == -1).all() and (s[:, 300:] == 0).all()


def test_walk_finds_neighbours_and_max_iter_cuts_it():
    idx, E, Q = _index(degree=8, knn=16)
    S = R.scores64(Q, E)
    s, d = idx.search(Q, 10, ef=64, width=2)
    free = idx.last_iterations.copy()
    assert (free > 2).all()
    recall = np.mean([len(set(d[i]) & set(_exact(S, 10)[i])) / 10 for i in range(len(Q))])
    assert recall >= 0.9
    assert np.array_equal(s, np.take_along_axis(S, d.astype(np.int64), 1))
    for i in range(len(Q)):                                  # in order, no doc twice
        keys = [(-float(a), int(b)) for a, b in zip(s[i], d[i])]
        assert keys == sorted(keys) and len(set(d[i])) == 10
    idx.search(Q, 10, ef=64, width=2, max_iter=2)
    assert (idx.last_iterations == 2).all()
    s0, d0 = idx.search(Q, 10, ef=64, width=2, max_iter=1)
    # one iteration: the seeds and the rows of the two best seeds, nothing else
    entry = idx.entry(64)
    for i in range(len(Q)):
        seeds = R.ordered(S[i][entry], entry)[:64]
        seen = {x for _, x in seeds} | {int(x) for _, p in seeds[:2] for x in idx.graph[p] if x >= 0}
        cand = np.array(sorted(seen))
        assert np.array_equal(d0[i], cand[_exact(S[i:i + 1, cand], 10)[0]])


def test_band_filter_leaves_the_walk_alone():
    idx, E, Q = _index(degree=8, knn=16)
    pools = idx.pools(Q, 40, 2)
    plain = idx.last_iterations.copy()
    exclude = [[d for _, d in p[:5]] for p in pools]         # the five best of every pool
    ceiling = np.array([p[2][0] for p in pools], np.float32)
    ceiling[3] = np.nan
    s, d, found = idx.search_band(Q, 0, 40, exclude=exclude, ceiling=ceiling, ef=40, width=2)
    assert np.array_equal(idx.last_iterations, plain)
    for i, p in enumerate(pools):
        want = [(a, b) for a, b in p if b not in exclude[i] and np.float32(a) < ceiling[i]]
        assert found[i] == len(want) and d[i, :found[i]].tolist() == [b for _, b in want]
        assert (d[i, found[i]:] == -1).all() and (s[i, found[i]:] == 0).all()
    assert found[3] == 0 and (found[[0, 1, 2]] > 0).all() and (found < 40).all()
    s2, d2, f2 = idx.search_band(Q, 3, 7, exclude=exclude, ef=40, width=2)
    assert all(d2[i].tolist() == [b for _, b in pools[i][5:]][3:7] for i in range(len(Q))) and (f2 == 4).all()


# ------------------------------------------------------------------------------------------------ header, ABI, CLI
NAMES = ["snx_graph_optimize_workspace_bytes", "snx_graph_optimize", "snx_graph_search_workspace_bytes",
         "snx_graph_search"]


def test_header_and_ctypes_table_name_the_graph_entry_points():
    import snx
    from snx import asmcheck
    from snx._lib import SIGNATURES
    text = open(os.path.join(ROOT, "include", "snx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, text) and n in SIGNATURES, n
    assert "graph dense retrieval (csrc/graph.hip)" in text and "ref:benchmark/index_manager.py:98-110" in text
    assert not [n for n in snx.verify_exports() if n in NAMES]
    assert set(asmcheck.GUARDED["graph.hip"]) == {"gr_forward_kernel", "gr_walk_kernel", "gr_output_kernel"}


def test_workspace_and_shape_errors_come_from_the_host():
    from snx import fn
    osize, ssize = fn("snx_graph_optimize_workspace_bytes"), fn("snx_graph_search_workspace_bytes")
    assert osize(1000, 64, 32) >= 1000 * 32 * 12 and osize(2000, 64, 32) > osize(1000, 64, 32)
    for bad in ((0, 64, 32), (-1, 64, 32), (10, 129, 32), (10, 16, 32), (10, 64, 0), (10, 128, 65)):
        assert osize(*bad) == 0, bad
    assert ssize(8, 100, 4, 32) == ssize(8, 100, 8, 64) > 0 and ssize(16, 100, 4, 32) > ssize(8, 100, 4, 32)
    for bad in ((0, 100, 4, 32), (8, 0, 4, 32), (8, 1025, 4, 32), (8, 100, 0, 32), (8, 100, 9, 32), (8, 100, 4, 0),
                (8, 100, 4, 65)):
        assert ssize(*bad) == 0, bad
    buf, ibuf = (C.c_float * 64)(), (C.c_int32 * 64)()
    p, ip = C.cast(buf, C.c_void_p), C.cast(ibuf, C.c_void_p)
    optimize, search = fn("snx_graph_optimize"), fn("snx_graph_search")
    assert optimize(ip, 4, 129, 2, ip, None, p, 1 << 20, None) == -2 and optimize(ip, 4, 2, 4, ip, None, p, 1 << 20, None) == -2
    assert optimize(ip, -1, 4, 2, ip, None, p, 1 << 20, None) == -2 and optimize(ip, 4, 4, 65, ip, None, p, 1 << 20, None) == -2
    assert optimize(None, 4, 4, 2, ip, None, p, 1 << 20, None) == -3 and optimize(ip, 4, 4, 2, None, None, p, 1 << 20, None) == -3
    assert optimize(ip, 4, 4, 2, ip, None, p, 16, None) == -3 and optimize(ip, 4, 4, 2, ip, None, None, 1 << 20, None) == -3
    assert optimize(None, 0, 4, 2, None, None, None, 0, None) == 0           # no docs: nothing to do

    def s(nq=2, D=8, nd=4, degree=2, nseed=1, ef=4, width=1, max_iter=0, lo=0, hi=1, q=p, out=ip, ws=p, ws_bytes=1 << 20,
          ex=None):
        return search(q, nq, D, p, nd, ip, degree, ip, nseed, ef, width, max_iter, ex, None, None, lo, hi, out, p, None,
                      None, ws, ws_bytes, None)
    for kw in (dict(D=0), dict(D=4097), dict(nd=-1), dict(degree=0), dict(degree=65), dict(nseed=-1), dict(nseed=5),
               dict(ef=0), dict(ef=1025), dict(width=0), dict(width=9), dict(max_iter=-1), dict(lo=-1), dict(lo=1, hi=1),
               dict(hi=5), dict(nq=-1)):
        assert s(**kw) == -2, kw
    for kw in (dict(q=None), dict(out=None), dict(ws=None), dict(ws_bytes=16), dict(ex=ip)):
        assert s(**kw) == -3, kw
    assert s(nq=0, ws=None, ws_bytes=0) == 0                 # no queries: nothing to do


def test_graph_index_validates_its_arguments_without_a_gpu():
    from snx.retrieval import GRAPH_DEGREE_MAX, GRAPH_EF_MAX, GRAPH_KNN_MAX, GRAPH_WIDTH_MAX, GraphIndex
    assert (GRAPH_DEGREE_MAX, GRAPH_KNN_MAX, GRAPH_EF_MAX, GRAPH_WIDTH_MAX) == (64, 128, 1024, 8)
    for dim in (0, 4097, 1.5, True, "8"):
        with pytest.raises(ValueError):
            GraphIndex(dim, "cpu")
    for kw in (dict(degree=0), dict(degree=1), dict(degree=7), dict(degree=66), dict(degree=8.0), dict(degree=True),
               dict(knn=16), dict(knn=129), dict(knn=64.0), dict(degree=8, knn=7), dict(ef=0), dict(ef=1025), dict(ef=10.0),
               dict(ef=True), dict(width=0), dict(width=9), dict(width=2.0), dict(nentry=0), dict(nentry=1.5),
               dict(nentry=True)):
        with pytest.raises(ValueError):
            GraphIndex(8, "cpu", **kw)
    idx = GraphIndex(8, "cpu")
    assert (idx.degree, idx.knn, idx.ef, idx.width, idx.nentry) == (32, 64, 100, 4, None)    # m 16, ef_construction 128
    assert GraphIndex(8, "cpu", degree=64, knn=128, ef=1024, width=8, nentry=7).nentry == 7
    for call in (lambda: idx.search(None, 1), lambda: idx.search_band(None, 0, 1), lambda: idx.pair_scores(None, None),
                 lambda: idx.structure()):
        with pytest.raises(RuntimeError):
            call()
    for k in (0, 1025, 1.0, True):
        with pytest.raises(ValueError):
            idx.search(None, k)
    for lo, hi in ((-1, 1), (1, 1), (0, 1025), (0.0, 1), (0, True)):
        with pytest.raises(ValueError):
            idx.search_band(None, lo, hi)
    import torch
    for bad in (np.zeros((2, 8), np.float32), torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 7), torch.zeros(8),
                torch.full((2, 8), float("nan"))):
        with pytest.raises(ValueError):
            idx.add(bad)


def test_cli_arguments():
    from src.train.cli import eval_hybrid, teacher_scores
    base = ["mine", "--embeddings", "e.npy", "--text-index", "t.json"]
    a = teacher_scores.parse_args(base)
    assert (a.index, a.degree, a.ef) == ("flat", 32, 0)
    a = teacher_scores.parse_args(base + ["--index", "graph", "--degree", "16", "--ef", "200"])
    assert (a.index, a.degree, a.ef) == ("graph", 16, 200)
    for bad in (["--index", "hnsw"], ["--index", "graph", "--degree", "7"], ["--index", "graph", "--degree", "66"],
                ["--index", "graph", "--ef", "49"], ["--index", "graph", "--ef", "1025"]):
        with pytest.raises(SystemExit):
            teacher_scores.parse_args(base + bad)
    a = eval_hybrid.parse_args([])
    assert (a.dense_index, a.ef, a.degree) == ("flat", 0, 32)
    a = eval_hybrid.parse_args(["--dense-embeddings", "e.npz", "--dense-index", "graph", "--ef", "128", "--degree", "16"])
    assert (a.dense_index, a.ef, a.degree) == ("graph", 128, 16)
    for bad in (["--dense-index", "graph"], ["--dense-embeddings", "e.npz", "--dense-index", "hnsw"],
                ["--dense-embeddings", "e.npz", "--dense-index", "graph", "--ef", "99"],
                ["--dense-embeddings", "e.npz", "--dense-index", "graph", "--degree", "3"],
                ["--dense-run", "r.npz", "--dense-index", "graph"]):
        with pytest.raises(SystemExit):
            eval_hybrid.parse_args(bad)
    from src.preprocessing.miners import BGEM3HardNegativeMiner
    miner = BGEM3HardNegativeMiner(device="cpu", encode=lambda texts: np.zeros((len(texts), 4), np.float32))
    for index_type in ("hnsw", "graph"):                     # the miner stays at the reference's flat | ivf
        with pytest.raises(ValueError):
            miner.build_index(["a"], index_type=index_type)


def test_list_recall_of_eval_hybrid():
    import torch
    from src.train.cli.eval_hybrid import list_recall
    exact = torch.tensor([[0, 1, 2, 3], [4, 5, -1, -1], [-1, -1, -1, -1]], dtype=torch.int32)
    got = torch.tensor([[3, 9, 0, 8], [5, 4, 7, -1], [2, -1, -1, -1]], dtype=torch.int32)
    assert list_recall(got, exact, 4) == pytest.approx((0.5 + 1.0 + 1.0) / 3)
    assert list_recall(got, exact, 1) == pytest.approx((0.0 + 0.0 + 1.0) / 3)
    assert list_recall(exact, exact, 4) == 1.0 and list_recall(got[:0], exact[:0], 4) == 1.0

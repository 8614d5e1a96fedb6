"""Budget-driven query slicing of SparseIndex.search / search_band / first_relevant (snx/retrieval/sparse.py over the
shared slice iterator): every other case of the suite fits in one launch.  With the budgets shrunk, five queries go as
2 + 2 + 1; every sliced argument (query rows, targets, exclusion rows whose values index the unsliced doc array,
ceilings, relevance rows, every output) must land where the one-launch call puts it.  Dyadic weights: every score is
exact in fp32, so the results equal the numpy restatements BIT for BIT, and the unsliced call as well."""
import numpy as np
import pytest
import torch

from tests import qrels_reference as Q
from tests.test_gpu_mining import _ref_band
from tests.test_gpu_retrieval import _dense, _index, _ref_rank, _rows, _to_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_sliced_launches_equal_the_references_and_the_unsliced_calls(dev, monkeypatch):
    from snx import fn
    from snx.retrieval import sparse
    rng = np.random.default_rng(31)
    V, nd, k, lo, hi, chunk = 40, 300, 7, 2, 9, 128            # three chunks, the last partial
    levels = np.array([16, 32, 64])
    docs = _rows(rng, nd, V, 6, levels, common=7, empty_every=17)
    queries = _rows(rng, 5, V, 5, levels)
    queries[3] = (np.zeros(0, np.int64), np.zeros(0, np.float64))               # an empty query in the last full slice
    idx = _index(docs, V, dev)
    q = _to_device(queries, dev, np.random.default_rng(5))
    S = _dense(queries, V) @ _dense(docs, V).T
    order = [np.lexsort((np.arange(nd), -S[i])) for i in range(5)]
    targets = [int(order[0][3]), 0, int(order[2][0]), 150, int(order[4][11])]    # doc 0 is empty: a miss
    excl = [[int(d) for d in order[0][:3]] + [250, 251], [], [int(order[2][4])], [1, 2],
            [int(d) for d in order[4][1:9]] + [int(order[4][1])]]               # lengths 5, 0, 1, 2, 9
    ceil = [np.float32(S[0, order[0][1]]), np.inf, np.float32(S[2, order[2][5]]), np.float32(1.0),
            np.float32(S[4, order[4][0]])]
    relevant = [[int(order[0][5]), int(order[0][1]), nd + 5], [0, int(order[1][3])], [], [3, 4],
                [int(order[4][2]), 1000, int(order[4][6])]]                     # multi-doc rows, ids outside the corpus
    tg = torch.tensor(targets, dtype=torch.int32, device=dev)
    ct = torch.tensor(ceil, dtype=torch.float32, device=dev)

    def calls():
        return (idx.search(*q, k, targets=tg, chunk_docs=chunk),
                idx.search_band(*q, lo, hi, exclude=excl, ceiling=ct, chunk_docs=chunk),
                idx.first_relevant(*q, relevant, chunk_docs=chunk))

    launches = []

    def counting_fn(name):
        f = fn(name)
        if name.endswith("_bytes"):
            return f
        return lambda *a: (launches.append((name, a[3])), f(*a))[1]             # a[3]: the queries of the launch

    monkeypatch.setattr(sparse, "fn", counting_fn)
    whole = calls()
    assert launches == [("snx_sparse_search", 5), ("snx_sparse_search_band", 5), ("snx_sparse_first_relevant", 5)]
    del launches[:]
    monkeypatch.setattr(sparse, "_FIRST_RELEVANT_BLOCKS", 6)                    # 6 workgroups / 3 chunks: 2 queries
    monkeypatch.setattr(sparse, "_SEARCH_WS_BUDGET", 2 * int(fn("snx_sparse_search_workspace_bytes")(1, nd, k, chunk)))
    search = idx.search(*q, k, targets=tg, chunk_docs=chunk)
    monkeypatch.setattr(sparse, "_SEARCH_WS_BUDGET",
                        2 * int(fn("snx_sparse_search_band_workspace_bytes")(1, nd, hi, chunk)))
    band = idx.search_band(*q, lo, hi, exclude=excl, ceiling=ct, chunk_docs=chunk)
    first = idx.first_relevant(*q, relevant, chunk_docs=chunk)
    assert launches == [(name, m) for name in ("snx_sparse_search", "snx_sparse_search_band",
                                               "snx_sparse_first_relevant") for m in (2, 2, 1)]
    for got, want in zip((search, band, first), whole):                         # the slicing changes no bit
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g, w)

    sc, dc, rk, ts = (x.cpu().numpy() for x in search)
    rd, rs, rr = _ref_rank(S, k, np.asarray(targets))
    assert np.array_equal(dc, rd) and np.array_equal(sc.astype(np.float64), rs) and np.array_equal(rk, rr)
    assert np.array_equal(ts.astype(np.float64), S[np.arange(5), targets])
    assert rr[1] == 0 and rr[3] == 0 and (rr[[0, 2, 4]] > 0).all()
    sc, dc, fd = (x.cpu().numpy() for x in band)
    rd, rs, rf = _ref_band(S, lo, hi, excl, np.asarray(ceil, np.float64))
    assert np.array_equal(dc, rd) and np.array_equal(sc.astype(np.float64), rs) and np.array_equal(fd, rf)
    assert rf[3] == 0 and (rf[[0, 1, 2, 4]] > 0).all()
    want = Q.first_relevant(Q.scores(queries, docs, V), relevant)
    for g, w in zip(first, want):
        assert g.cpu().numpy().dtype == w.dtype and np.array_equal(g.cpu().numpy(), w)
    assert want[3].tolist() == [2, 2, 0, 2, 2] and want[0][2] == -1 and want[0][3] == -1 and (want[2][[0, 1, 4]] > 0).all()

"""Exact multi-vector (MaxSim) search on the GPU (csrc/mv_search.hip, snx.retrieval.MultiVectorIndex) against
snx.teacher.maxsim_pairs over all pairs, bit for bit, and against float64 torch within the bound that
tests/test_gpu_maxsim.py derives: (1.01 D + Lq + 2) 2^-24 over rows already rounded to the store's type."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
QROWS = (1, 2, 31, 33, 63, 64, 65, 130)        # blocks of several queries, one across a block edge, one over three blocks
CASES = [(p, D) for p in ("bf16", "fp32") for D in (64, 1024)]


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


@functools.lru_cache(maxsize=None)
def _store(D):
    """Float64 unit rows: (query rows, q_ptr, doc rows, doc_ptr, twins).  Documents: the row counts of the tile's edges, forty
    of 1 to 3 rows, a group whose ends fall one before, one behind and on a 64-row edge, one without rows, random ones, two
    copies of earlier documents (equal bits, a tie) and, per query, a document of -centre + noise (every similarity
    negative: a zero or padding row would win its max).  Three documents per query carry near-matches of the query's
    centres at their first row, their last row and wherever they touch a tile edge."""
    gen = torch.Generator().manual_seed(4000 + D)

    def rand(n):
        return _unit(torch.randn(n, D, generator=gen, dtype=torch.float64))

    centres = [rand(3) for _ in QROWS]
    queries = [_unit(c[torch.arange(L) % 3] + 0.05 * rand(L)) for c, L in zip(centres, QROWS)]
    lens = [1, 2, 63, 64, 65, 129, 200] + [1 + i % 3 for i in range(40)]
    lens += [64 - sum(lens) % 64, 63, 2, 63, 0] + [int(v) for v in torch.randint(1, 90, (230,), generator=gen)]
    docs = [rand(n) for n in lens]
    start = 0
    for i, d in enumerate(docs):
        for q in range(len(QROWS)):
            if i in (q, 60 + 3 * q, 120 + 5 * q):
                rows = sorted({0, len(d) - 1} | {r for r in range(len(d)) if (start + r) % 64 in (0, 63)})
                d[rows] = _unit(0.9 * centres[q][torch.arange(len(rows)) % 3] + 0.436 * rand(len(rows)))
        start += len(d)
    twins = [(60, len(docs)), (5, len(docs) + 1)]
    docs += [docs[60].clone(), docs[5].clone()] + [_unit(-c[:1] + 0.3 * rand(1 + q % 3)) for q, c in enumerate(centres)]
    ptr = lambda seqs: torch.tensor([0] + [len(s) for s in seqs]).cumsum(0).tolist()
    return torch.cat(queries), ptr(queries), torch.cat(docs), ptr(docs), twins


@functools.lru_cache(maxsize=None)
def _case(precision, D):
    """The built index, the queries, maxsim_pairs over all nq x nd pairs (the empty document aside) as [nq, nd] fp32 on the
    CPU with NaN at the empty document, float64 torch over the same rounded rows, and the expected ranking per query."""
    from snx.retrieval import MultiVectorIndex
    from snx.teacher import maxsim_pairs
    q64, qp, d64, dp, twins = _store(D)
    qmv, dmv = q64.to(DTYPES[precision]).to(DEV), d64.to(DTYPES[precision]).to(DEV)
    index = MultiVectorIndex(D, DEV)
    half = len(dp) // 2                                            # two batches: doc ids = order of addition
    index.add(dmv[:dp[half]], dp[:half + 1])
    index.add(dmv[dp[half]:], [v - dp[half] for v in dp[half:]])
    index.build()
    nq, nd = len(qp) - 1, len(dp) - 1
    live = [d for d in range(nd) if dp[d + 1] > dp[d]]
    assert len(live) == nd - 1
    pq = torch.tensor([q for q in range(nq) for _ in live])
    pd = torch.tensor([nq + d for _ in range(nq) for d in live])
    joint_ptr = qp + [qp[-1] + v for v in dp[1:]]
    pairs = maxsim_pairs(torch.cat([qmv, dmv]), joint_ptr, pq, pd).cpu().view(nq, len(live))
    ref = torch.full((nq, nd), float("nan"))
    ref[:, live] = pairs
    xq, xd = qmv.double().cpu(), dmv.double().cpu()
    ref64 = torch.full((nq, nd), float("nan"), dtype=torch.float64)
    for q in range(nq):
        S = xq[qp[q]:qp[q + 1]] @ xd.t()
        for d in live:
            ref64[q, d] = S[:, dp[d]:dp[d + 1]].amax(dim=1).sum() / (qp[q + 1] - qp[q])
    rank = [sorted(live, key=lambda d: (-float(ref[q, d]), d)) for q in range(nq)]
    return index, qmv, qp, ref, ref64, rank, twins


def _expect(rank, ref, k):
    """Rows of (scores, docs) of width k: the ranking's first k, then 0 / -1."""
    docs = torch.tensor([r[:k] + [-1] * (k - len(r[:k])) for r in rank], dtype=torch.int32)
    scores = torch.stack([torch.where(d >= 0, ref[q, d.clamp_min(0).long()], torch.zeros(())) for q, d in enumerate(docs)])
    return scores, docs


@pytest.mark.parametrize("precision,D", CASES)
def test_scores_and_order(precision, D):
    index, qmv, qp, ref, ref64, rank, twins = _case(precision, D)
    nq, nd = ref.shape
    for a, b in twins:                                             # equal rows, equal bits: the lower id first
        assert torch.equal(ref[:, a], ref[:, b]) and all(r.index(a) + 1 == r.index(b) for r in rank)
    lq = torch.tensor([qp[q + 1] - qp[q] for q in range(nq)], dtype=torch.float64)
    bound = ((1.01 * D + lq + 2.0) * 2.0 ** -24)[:, None]
    for k in (1, 10, nd + 5):
        scores, docs = index.search(qmv, qp, k)
        scores, docs = scores.cpu(), docs.cpu()
        want_s, want_d = _expect(rank, ref, k)
        assert torch.equal(docs, want_d)                           # the whole ranking, ties and unused slots; no empty doc
        assert torch.equal(scores.view(torch.int32), want_s.view(torch.int32))     # maxsim_pairs, bit for bit
        used = docs >= 0
        err = (scores.double() - torch.gather(ref64, 1, docs.clamp_min(0).long())).abs()
        print(f"mv_search {precision} D={D} k={k}: max err / bound {float((err / bound)[used].max()):.3f}")
        assert bool((err <= bound)[used].all())


@pytest.mark.parametrize("precision,D", CASES)
def test_independent_of_chunks_slices_and_query_order(precision, D):
    index, qmv, qp, ref, _, rank, _ = _case(precision, D)
    nq, k = ref.shape[0], ref.shape[1] + 5
    base = index.search(qmv, qp, k)
    for kw in ({"chunk_docs": 64}, {"query_slice": 1}, {"chunk_docs": 64, "query_slice": 3}):
        got = index.search(qmv, qp, k, **kw)
        assert torch.equal(got[0].view(torch.int32), base[0].view(torch.int32)) and torch.equal(got[1], base[1]), kw
    rev = torch.cat([qmv[qp[q]:qp[q + 1]] for q in reversed(range(nq))])
    rptr = torch.tensor([0] + [qp[q + 1] - qp[q] for q in reversed(range(nq))]).cumsum(0).tolist()
    got = index.search(rev, rptr, k)
    assert torch.equal(got[0].flip(0).view(torch.int32), base[0].view(torch.int32)) and torch.equal(got[1].flip(0), base[1])


@pytest.mark.parametrize("precision,D", CASES)
def test_band_with_exclusions(precision, D):
    index, qmv, qp, ref, _, rank, twins = _case(precision, D)
    nq, nd = ref.shape
    exclude = [[rank[q][0], twins[q % 2][1]] + ([twins[0][0]] if q == 0 else []) for q in range(nq)]
    left = [[d for d in rank[q] if d not in exclude[q]] for q in range(nq)]
    for lo, hi in ((0, 7), (3, 40), (nd - 12, nd + 3)):
        scores, docs, found = index.search_band(qmv, qp, lo, hi, exclude=exclude, chunk_docs=64 if lo else 0)
        want_s, want_d = _expect([r[lo:hi] for r in left], ref, hi - lo)
        assert torch.equal(docs.cpu(), want_d)
        assert torch.equal(scores.cpu().view(torch.int32), want_s.view(torch.int32))
        assert found.cpu().tolist() == [max(0, min(hi, len(r)) - lo) for r in left]

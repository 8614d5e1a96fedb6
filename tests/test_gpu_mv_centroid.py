"""The centroid-interaction candidate search of MultiVectorIndex (csrc/mv_centroid.hip) on the GPU: the candidate scores
against float64, the codes, and the exact rescore against ``search`` / ``search_band`` / ``pair_scores`` bit for bit."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

Q_LENS = [1, 2, 15, 16, 17, 33, 63, 64, 65, 130]               # cross the 16-, 32- and 64-row group edges and a 64-row run
NCS = (8, 1500, 4096)                                          # R = 64 / 32 / 16 query rows per table group
CASES = [(dt, D) for dt in (torch.bfloat16, torch.float32) for D in (64, 1024)]


def _unit(n, D, seed):
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=-1, keepdim=True)


@functools.lru_cache(maxsize=None)
def _store(dtype, D):
    """About 300 documents: 1 to 3 rows, 63 / 64 / 65 / 129 / 200 rows, a run whose ends fall on and beside the 8-code
    pieces the walk loads, one document without rows, two bit-equal twins of earlier documents; and the queries."""
    g = torch.Generator().manual_seed(7)
    lens = [1, 2, 3, 63, 64, 65, 129, 200, 2, 8, 8, 7, 9, 16, 1, 15, 17, 8, 24, 3] + [0]
    lens += torch.randint(1, 41, (277,), generator=g).tolist()
    twins = {len(lens): 5, len(lens) + 1: 33}                    # new id -> the earlier document it copies
    lens += [lens[5], lens[33]]
    ptr = [0]
    for n in lens:
        ptr.append(ptr[-1] + n)
    rows = _unit(ptr[-1], D, 1).to(dtype)
    for new, old in twins.items():
        rows[ptr[new]:ptr[new + 1]] = rows[ptr[old]:ptr[old + 1]]
    q_ptr = [0]
    for n in Q_LENS:
        q_ptr.append(q_ptr[-1] + n)
    # queries near documents, so that scores spread: a query row is a document row plus noise
    pick = torch.randint(0, ptr[-1], (q_ptr[-1],), generator=g)
    q = rows[pick].float() + 0.5 * _unit(q_ptr[-1], D, 2)
    q = (q / q.norm(dim=-1, keepdim=True)).to(dtype)
    return rows.cuda(), ptr, q.cuda(), q_ptr, twins


@functools.lru_cache(maxsize=None)
def _index(dtype, D, nc):
    from snx.retrieval import MultiVectorIndex
    rows, ptr, q, q_ptr, twins = _store(dtype, D)
    index = MultiVectorIndex(D, "cuda")
    index.add(rows[:ptr[150]], ptr[:151])
    index.add(rows[ptr[150]:], [v - ptr[150] for v in ptr[150:]])
    index.build().set_centroids(_unit(nc, D, 3).cuda())
    return index


def _a64(index, q, q_ptr, ptr):
    """a64 [nq, nd]: the mean over the query's rows of the best float64 product with a centroid of the document; -inf for
    a document without rows."""
    S = q.double() @ index.centroids.double().T
    M = S[:, index.codes.long()]
    per_doc = torch.stack([M[:, a:b].amax(dim=1) if b > a else torch.full_like(M[:, 0], float("-inf"))
                           for a, b in zip(ptr, ptr[1:])], dim=1)
    return torch.stack([per_doc[a:b].mean(dim=0) for a, b in zip(q_ptr, q_ptr[1:])])


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("dtype,D", CASES)
def test_candidate_scores_and_codes(dtype, D, nc):
    rows, ptr, q, q_ptr, _ = _store(dtype, D)
    index, nd, ncand = _index(dtype, D, nc), len(ptr) - 1, 20
    # 2. the codes: a row's code is its best centroid up to the fp32 dot's error
    codes = index.codes.long()
    assert index.codes.dtype == torch.uint16 and codes.numel() == ptr[-1] and int(codes.max()) < nc
    P = rows.double() @ index.centroids.double().T
    gap = P.amax(dim=1) - P.gather(1, codes[:, None])[:, 0]
    assert float(gap.max()) <= (1.01 * D + 2) * 2.0 ** -24
    # 1. the candidate scores against float64, and the set as a valid top ncand
    a64 = _a64(index, q, q_ptr, ptr)
    exclude = [[3, 7, 40 + i] for i in range(len(Q_LENS))]
    worst = 0.0
    for ex in (None, exclude):
        for n in (ncand, 1024):
            a, docs = index.candidates(q, q_ptr, n, exclude=ex)
            for i, lq in enumerate(Q_LENS):
                B = 2.0 ** -8 + (1.01 * D + lq + 2) * 2.0 ** -24
                got = docs[i][docs[i] >= 0].long()
                live = [d for d in range(nd) if ptr[d + 1] > ptr[d] and not (ex and d in ex[i])]
                assert got.numel() == min(n, len(live)) and set(got.tolist()) <= set(live)   # no rowless, excluded, outside id
                err = (a[i, :got.numel()].double() - a64[i, got]).abs().max()
                worst = max(worst, float(err) / B)
                assert float(err) <= B
                if n == ncand:
                    ref = a64[i, live].sort(descending=True).values
                    assert float(a64[i, got].min()) >= float(ref[n - 1]) - 2 * B
                    rest = sorted(set(live) - set(got.tolist()))
                    assert float(a64[i, rest].max()) <= float(a64[i, got].min()) + 2 * B
    print(f"candidate scores {dtype} D={D} nc={nc}: max err / B = {worst:.3f}")


@pytest.mark.parametrize("dtype,D", CASES)
def test_all_candidates_give_the_exact_search(dtype, D):
    rows, ptr, q, q_ptr, twins = _store(dtype, D)
    index, nd = _index(dtype, D, 1500), len(ptr) - 1
    for k in (1, 10, nd + 5):
        s, d = index.search(q, q_ptr, k)
        s2, d2 = index.search_two_phase(q, q_ptr, k, 1024)
        assert torch.equal(d, d2) and torch.equal(_bits(s), _bits(s2))
    exclude = [[3, 7, 40 + i] for i in range(len(Q_LENS))]
    for lo, hi in ((0, 7), (3, 40)):
        want = index.search_band(q, q_ptr, lo, hi, exclude=exclude)
        got = index.search_band_two_phase(q, q_ptr, lo, hi, 1024, exclude=exclude)
        assert torch.equal(want[1], got[1]) and torch.equal(_bits(want[0]), _bits(got[0])) and torch.equal(want[2], got[2])
    s2, d2 = s2.cpu(), d2.cpu().tolist()
    for new, old in twins.items():
        for i in range(len(Q_LENS)):
            a, b = d2[i].index(old), d2[i].index(new)
            assert a < b and _bits(s2[i, a:a + 1]).item() == _bits(s2[i, b:b + 1]).item()


@pytest.mark.parametrize("dtype,D", CASES)
def test_independent_of_chunks_slices_and_query_order(dtype, D):
    _, _, q, q_ptr, _ = _store(dtype, D)
    index = _index(dtype, D, 1500)
    a, docs = index.candidates(q, q_ptr, 20)
    s, d = index.search_two_phase(q, q_ptr, 10, 20)
    for kw in ({"chunk_docs": 64}, {"query_slice": 1}, {"chunk_docs": 64, "query_slice": 1}):
        a2, docs2 = index.candidates(q, q_ptr, 20, **kw)
        s2, d2 = index.search_two_phase(q, q_ptr, 10, 20, **kw)
        assert torch.equal(docs, docs2) and torch.equal(_bits(a), _bits(a2)), kw
        assert torch.equal(d, d2) and torch.equal(_bits(s), _bits(s2)), kw
    rq = torch.cat([q[a0:b0] for a0, b0 in reversed(list(zip(q_ptr, q_ptr[1:])))])
    rptr = [0]
    for n in reversed(Q_LENS):
        rptr.append(rptr[-1] + n)
    a2, docs2 = index.candidates(rq, rptr, 20)
    s2, d2 = index.search_two_phase(rq, rptr, 10, 20)
    assert torch.equal(docs, docs2.flip(0)) and torch.equal(_bits(a), _bits(a2.flip(0)))
    assert torch.equal(d, d2.flip(0)) and torch.equal(_bits(s), _bits(s2.flip(0)))


@pytest.mark.parametrize("dtype,D", CASES)
def test_rescored_scores_are_pair_scores(dtype, D):
    _, _, q, q_ptr, _ = _store(dtype, D)
    index, ncand = _index(dtype, D, 1500), 20
    _, cand = index.candidates(q, q_ptr, ncand)
    s, d = index.search_two_phase(q, q_ptr, ncand, ncand)
    assert torch.equal(cand.sort(dim=1).values, d.sort(dim=1).values) and int(d.min()) >= 0
    pairs = torch.stack([torch.arange(len(Q_LENS), device="cuda").repeat_interleave(ncand), d.reshape(-1).long()], dim=1)
    want = index.pair_scores(q, q_ptr, pairs).view(-1, ncand)
    assert torch.equal(_bits(s), _bits(want))
    s, d = s.cpu().tolist(), d.cpu().tolist()
    for i in range(len(Q_LENS)):
        order = sorted(range(ncand), key=lambda j: (-s[i][j], d[i][j]))
        assert order == list(range(ncand))

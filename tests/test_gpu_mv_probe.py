"""The probed candidate pass of MultiVectorIndex (csrc/mv_centroid.hip, the mvp_ kernels) on the GPU: the inverted lists
against a torch restatement, and the probed candidates against the unprobed pass with the complement of P(q) excluded, bit
for bit.  The probe sets come from the unprobed pass itself, over an auxiliary index whose documents are the centroids."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 64
Q_LENS = [1, 7, 16, 17, 33, 64, 70]                            # on and beside the 8-row pieces and the 16 / 32 / 64-row groups
DTYPES = (torch.bfloat16, torch.float32)
STORES = [("small", 48), ("small", 1500), ("small", 4096), ("large", 48)]      # R = 64 / 32 / 16; "large" crosses a block
EXCLUDE = [[3, 7, 40 + i] for i in range(len(Q_LENS))]


def _unit(n, seed):
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=-1, keepdim=True)


@functools.lru_cache(maxsize=None)
def _store(dtype, kind):
    """small: about 300 documents of 0 to 200 rows, rows starting on and beside the 8-code pieces, one document without
    rows.  large: 2,500 documents of 1 to 12 rows, so that a query probes more than 1,024 of them.  And the queries, the
    first of which probes an empty list at nc = 4096, nprobe = 1."""
    g = torch.Generator().manual_seed(7)
    if kind == "small":
        lens = [1, 2, 3, 63, 64, 65, 129, 200, 2, 8, 8, 7, 9, 16, 1, 15, 17, 8, 24, 3, 0]
        lens += torch.randint(1, 41, (279,), generator=g).tolist()
    else:
        lens = torch.randint(1, 13, (2500,), generator=g).tolist()
    ptr = [0]
    for n in lens:
        ptr.append(ptr[-1] + n)
    rows = _unit(ptr[-1], 1).to(dtype)
    q_ptr = [0]
    for n in Q_LENS:
        q_ptr.append(q_ptr[-1] + n)
    pick = torch.randint(0, ptr[-1], (q_ptr[-1],), generator=g)
    q = rows[pick].float() + 0.5 * _unit(q_ptr[-1], 2)         # a query row is a document row plus noise
    q = (q / q.norm(dim=-1, keepdim=True)).to(dtype)
    if kind == "small":                                        # query 0 is the centroid (of 4,096) farthest from every row:
        c = _unit(4096, 3)                                     # its own best centroid, and one that owns no row
        q[0] = c[(rows.float() @ c.T).amax(dim=0).argmin()].to(dtype)
    return rows.cuda(), ptr, q.cuda(), q_ptr


def _build(dtype, kind, nc):
    from snx.retrieval import MultiVectorIndex
    rows, ptr, _, _ = _store(dtype, kind)
    index = MultiVectorIndex(D, "cuda")
    index.add(rows, ptr)
    return index.build().set_centroids(_unit(nc, 3).cuda())


_index = functools.lru_cache(maxsize=None)(_build)


@functools.lru_cache(maxsize=None)
def _top(dtype, kind, nc):
    """top(i) [qrows, 4] by the unprobed pass: the centroids are the one-row documents of an auxiliary index, every query
    row a one-row query, so its candidates are the row's best centroids under the table's keys and tie rule."""
    from snx.retrieval import MultiVectorIndex
    index, (_, _, q, q_ptr) = _index(dtype, kind, nc), _store(dtype, kind)
    aux = MultiVectorIndex(D, "cuda")
    aux.add(index.centroids, list(range(nc + 1)))
    aux.build().set_centroids(_unit(nc, 3).cuda())
    assert torch.equal(aux.codes.to(torch.int32).cpu(), torch.arange(nc, dtype=torch.int32))
    return aux.candidates(q, list(range(q_ptr[-1] + 1)), 4)[1].long().cpu()


def _probed_sets(dtype, kind, nc, nprobe):
    """P(q) before the exclusion, as sets of doc ids."""
    index, (_, ptr, _, q_ptr) = _index(dtype, kind, nc), _store(dtype, kind)
    doc_of = torch.repeat_interleave(torch.arange(len(ptr) - 1), torch.tensor(ptr).diff())
    codes = index.codes.to(torch.int32).cpu().long()
    top = _top(dtype, kind, nc)[:, :nprobe]
    return [set(doc_of[torch.isin(codes, top[a:b].reshape(-1))].tolist()) for a, b in zip(q_ptr, q_ptr[1:])]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(got, want):
    return torch.equal(got[1], want[1]) and torch.equal(_bits(got[0]), _bits(want[0]))


@pytest.mark.parametrize("kind,nc", STORES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lists_are_the_sorted_unique_code_doc_pairs(dtype, kind, nc):
    index, (_, ptr, q, q_ptr) = _index(dtype, kind, nc), _store(dtype, kind)
    index.candidates(q, q_ptr, 1, nprobe=1)                   # the first probed call builds the lists
    doc_of = torch.repeat_interleave(torch.arange(len(ptr) - 1), torch.tensor(ptr).diff())
    pairs = torch.unique(index.codes.to(torch.int32).cpu().long() * len(ptr) + doc_of)      # sorted: by code, then doc
    want_ptr = torch.zeros(nc + 1, dtype=torch.long)
    want_ptr[1:] = torch.bincount(pairs // len(ptr), minlength=nc).cumsum(0)
    assert index.list_ptr.dtype == torch.int64 and index.list_docs.dtype == torch.int32
    assert torch.equal(index.list_ptr.cpu(), want_ptr) and torch.equal(index.list_docs.cpu().long(), pairs % len(ptr))


@pytest.mark.parametrize("dtype", DTYPES)
def test_probing_every_centroid_is_the_unprobed_pass(dtype):
    index, (_, _, q, q_ptr) = _index(dtype, "small", 48), _store(dtype, "small")
    for ex in (None, EXCLUDE):
        for ncand in (20, 1024):
            assert _same(index.candidates(q, q_ptr, ncand, exclude=ex, nprobe=64), index.candidates(q, q_ptr, ncand, exclude=ex))


@pytest.mark.parametrize("kind,nc", STORES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_probed_candidates_are_the_unprobed_pass_over_the_probed_set(dtype, kind, nc):
    index, (_, ptr, q, q_ptr) = _index(dtype, kind, nc), _store(dtype, kind)
    everything, crossed, empty = set(range(len(ptr) - 1)), 0, 0
    for nprobe in (1, 4):
        probed = _probed_sets(dtype, kind, nc, nprobe)
        crossed += sum(len(p) > 1024 for p in probed)
        empty += sum(len(p - set(e)) == 0 for p, e in zip(probed, EXCLUDE))
        for ex in (None, EXCLUDE):
            outside = [sorted((everything - p) | set(e if ex else ())) for p, e in zip(probed, EXCLUDE)]
            for ncand in (20, 1024):
                got = index.candidates(q, q_ptr, ncand, exclude=ex, nprobe=nprobe)
                assert _same(got, index.candidates(q, q_ptr, ncand, exclude=outside)), (nprobe, ncand, ex is not None)
                # 4. neither the block size, the slices nor the order of the queries change a bit
                rq = torch.cat([q[a:b] for a, b in reversed(list(zip(q_ptr, q_ptr[1:])))])
                rptr = [0]
                for n in reversed(Q_LENS):
                    rptr.append(rptr[-1] + n)
                rex = None if ex is None else ex[::-1]
                back = index.candidates(rq, rptr, ncand, exclude=rex, chunk_docs=64, query_slice=2, nprobe=nprobe)
                assert _same((back[0].flip(0), back[1].flip(0)), got), (nprobe, ncand, ex is not None)
    assert crossed > 0 or kind != "large"                      # a query walked more than one block of 1,024
    assert empty > 0 or nc != 4096                             # a query probed nothing at all
    print(f"{kind} nc={nc}: queries past one block {crossed}, queries with nothing probed {empty}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_phase_over_probed_candidates(dtype):
    index, (_, _, q, q_ptr) = _index(dtype, "small", 1500), _store(dtype, "small")
    ncand, nq = 20, len(Q_LENS)
    _, cand = index.candidates(q, q_ptr, ncand, nprobe=4)
    s, d = index.search_two_phase(q, q_ptr, ncand, ncand, nprobe=4)
    assert torch.equal(cand.sort(dim=1).values, d.sort(dim=1).values)
    live = d >= 0
    pairs = torch.stack([torch.arange(nq, device="cuda").repeat_interleave(ncand)[live.reshape(-1)], d[live].long()], dim=1)
    assert torch.equal(_bits(s[live]), _bits(index.pair_scores(q, q_ptr, pairs)))
    assert bool((s[~live] == 0).all())
    sl, dl = s.cpu().tolist(), d.cpu().tolist()
    for i in range(nq):
        n = int(live[i].sum())
        assert all(v >= 0 for v in dl[i][:n]) and sorted(range(n), key=lambda j: (-sl[i][j], dl[i][j])) == list(range(n))
    # 6. the band agrees on found
    _, cand = index.candidates(q, q_ptr, ncand, exclude=EXCLUDE, nprobe=4)
    bs, bd, found = index.search_band_two_phase(q, q_ptr, 3, 12, ncand, exclude=EXCLUDE, nprobe=4)
    want = ((cand >= 0).sum(dim=1).clamp(max=12) - 3).clamp(min=0)
    assert torch.equal(found.long(), want) and torch.equal((bd >= 0).sum(dim=1), want)


def test_a_compressed_index_returns_the_same_candidates():
    _, _, q, q_ptr = _store(torch.bfloat16, "small")
    index = _build(torch.bfloat16, "small", 1500)
    want = index.candidates(q, q_ptr, 20, exclude=EXCLUDE, nprobe=4)
    index.compress(2)
    assert index.rows is None and index.list_ptr is not None   # the lists need codes, not rows
    assert _same(index.candidates(q, q_ptr, 20, exclude=EXCLUDE, nprobe=4), want)

"""The residual-compressed store of MultiVectorIndex (csrc/mv_centroid.hip, the mvr_ kernels) on the GPU: the codec against
its torch definition bit for bit, the scores from the packed form against float64, their invariances, and the released
rows."""
import functools

import pytest
import torch

from tests.test_gpu_mv_centroid import Q_LENS, _bits, _store, _unit

pytestmark = pytest.mark.gpu

CASES = [(nbits, D, 1500) for nbits in (1, 2, 4) for D in (64, 1024)] + [(2, 64, 8)]
BF16 = torch.bfloat16


def _codebook(nbits, D):
    """Given cutoffs and weights on the scale of a residual's entries, 1 / sqrt(D)."""
    n = 1 << nbits
    return torch.linspace(-1.5, 1.5, n + 1)[1:-1] / D ** 0.5, torch.linspace(-2.0, 2.0, n) / D ** 0.5


def _build(nbits, D, nc, keep_rows):
    from snx.retrieval import MultiVectorIndex
    rows, ptr, _, _, _ = _store(BF16, D)
    index = MultiVectorIndex(D, "cuda")
    index.add(rows, ptr)
    index.build().set_centroids(_unit(nc, D, 3).cuda())
    return index.compress(nbits, *_codebook(nbits, D), keep_rows=keep_rows)


@functools.lru_cache(maxsize=None)
def _index(nbits, D, nc, keep_rows=False):
    return _build(nbits, D, nc, keep_rows)


def _residuals(index, rows):
    return rows.float() - index.centroids[index.codes.long()].float()


@pytest.mark.parametrize("nbits,D,nc", CASES)
def test_codec_is_its_torch_definition(nbits, D, nc):
    rows = _store(BF16, D)[0]
    index = _build(nbits, D, nc, True)                            # its own: it is compressed again below
    res, every = _residuals(index, rows), torch.arange(rows.shape[0])
    cut, w = _codebook(nbits, D)
    m = cut.numel() // 2                                          # one cutoff moves onto a residual of the store
    inside = res[(res > (cut[m - 1] if m else -1.0)) & (res < (cut[m + 1] if m + 1 < cut.numel() else 1.0))]
    cut[m] = float(inside[0])
    index.compress(nbits, cut, w, keep_rows=True)
    assert index.residuals.dtype == torch.uint8 and tuple(index.residuals.shape) == (rows.shape[0], D * nbits // 8)
    buckets = torch.bucketize(res, cut.cuda())                    # #{m : cutoffs[m] < r}
    assert bool((buckets[res == cut[m]] == m).all())
    want = index.centroids[index.codes.long()].float() + w.to(BF16).float().cuda()[buckets]
    assert torch.equal(_bits(index.decompress(every)), _bits(want))
    index.compress(nbits, keep_rows=True)                         # the quantile defaults
    c, w = index.cutoffs, index.weights
    assert c.shape == ((1 << nbits) - 1,) and w.shape == (1 << nbits,) and c.dtype == w.dtype == torch.float32
    assert bool((c[1:] > c[:-1]).all()) and torch.equal(w, w.to(BF16).float()) and torch.equal(w, index.weights_bf16.float())
    tol = 2.0 ** -8 * float(w.abs().max())                       # the bf16 rounding of a weight
    assert bool((w[:-1] <= c + tol).all()) and bool((c <= w[1:] + tol).all())


@pytest.mark.parametrize("nbits,D,nc", CASES)
def test_scores_against_float64(nbits, D, nc):
    rows, ptr, q, q_ptr, twins = _store(BF16, D)
    index, nd = _index(nbits, D, nc), len(ptr) - 1
    wrow = index.weights.double()[torch.bucketize(_residuals(index, rows), index.cutoffs)]
    rho = float(wrow.norm(dim=1).max())
    M = q.double() @ (index.centroids.double()[index.codes.long()] + wrow).T
    per_doc = torch.stack([M[:, a:b].amax(dim=1) if b > a else torch.full_like(M[:, 0], float("-inf"))
                           for a, b in zip(ptr, ptr[1:])], dim=1)
    s64 = torch.stack([per_doc[a:b].mean(dim=0) for a, b in zip(q_ptr, q_ptr[1:])])
    s, d = index.search_two_phase(q, q_ptr, 1024, 1024)
    live = [j for j in range(nd) if ptr[j + 1] > ptr[j]]
    worst = 0.0
    for i, lq in enumerate(Q_LENS):
        B = (1.01 * D + lq + 5) * 1.02 * (1 + rho) * 2.0 ** -24
        got = d[i][d[i] >= 0].long()
        assert sorted(got.tolist()) == live                       # every document with rows, exactly once
        err = float((s[i, :got.numel()].double() - s64[i, got]).abs().max())
        worst = max(worst, err / B)
        assert err <= B
        si, di = s[i, :got.numel()].tolist(), got.tolist()
        assert all((-si[j], di[j]) < (-si[j + 1], di[j + 1]) for j in range(len(di) - 1))
        for new, old in twins.items():
            a, b = di.index(old), di.index(new)
            assert a < b and _bits(s[i, a:a + 1]).item() == _bits(s[i, b:b + 1]).item()
    print(f"residual scores nbits={nbits} D={D} nc={nc}: max err / B = {worst:.3f}")


@pytest.mark.parametrize("nbits,D,nc", CASES)
def test_independent_of_chunks_slices_and_query_order(nbits, D, nc):
    _, _, q, q_ptr, _ = _store(BF16, D)
    index, nq = _index(nbits, D, nc), len(Q_LENS)
    s, d = index.search_two_phase(q, q_ptr, 10, 20)
    for kw in ({"query_slice": 1}, {"chunk_docs": 64}):
        s2, d2 = index.search_two_phase(q, q_ptr, 10, 20, **kw)
        assert torch.equal(d, d2) and torch.equal(_bits(s), _bits(s2)), kw
    rq = torch.cat([q[a:b] for a, b in reversed(list(zip(q_ptr, q_ptr[1:])))])
    rptr = [0]
    for n in reversed(Q_LENS):
        rptr.append(rptr[-1] + n)
    s2, d2 = index.search_two_phase(rq, rptr, 10, 20)
    assert torch.equal(d, d2.flip(0)) and torch.equal(_bits(s), _bits(s2.flip(0)))
    pairs = torch.stack([torch.arange(nq, device="cuda").repeat_interleave(10), d.reshape(-1).long()], dim=1)
    assert torch.equal(_bits(index.pair_scores(q, q_ptr, pairs).view(nq, 10)), _bits(s))
    exclude = [[3, 7, 40 + i] for i in range(nq)]
    full_s, full_d = index.search_two_phase(q, q_ptr, 1024, 1024)
    bs, bd, found = index.search_band_two_phase(q, q_ptr, 3, 40, 1024, exclude=exclude)
    for i in range(nq):
        keep = torch.tensor([j for j, doc in enumerate(full_d[i].tolist()) if doc >= 0 and doc not in exclude[i]][3:40])
        assert int(found[i]) == 37 and torch.equal(bd[i], full_d[i][keep]) and torch.equal(_bits(bs[i]), _bits(full_s[i][keep]))


def test_table_groups_do_not_change_a_bit():
    """nc = 4096 holds 128 table blocks per launch group: 127 one-row queries and one of three runs put a query's runs on
    both sides of a group's end."""
    _, _, q, _, _ = _store(BF16, 64)
    index = _index(2, 64, 4096)
    qptr = list(range(128)) + [127 + 130]
    s, d = index.search_two_phase(q[:qptr[-1]], qptr, 10, 20)
    s2, d2 = index.search_two_phase(q[:qptr[-1]], qptr, 10, 20, query_slice=1)
    assert torch.equal(d, d2) and torch.equal(_bits(s), _bits(s2))


@pytest.mark.parametrize("nbits,D,nc", CASES)
def test_released_rows_change_no_bit(nbits, D, nc):
    _, ptr, q, q_ptr, _ = _store(BF16, D)
    kept, index = _index(nbits, D, nc, True), _index(nbits, D, nc)
    assert kept.rows is not None and index.rows is None
    held = [v for v in list(vars(index).values()) + index._parts if isinstance(v, torch.Tensor)]
    assert not any(v.dtype == BF16 and v.numel() >= ptr[-1] * D for v in held)
    a, b = kept.search_two_phase(q, q_ptr, 10, 20), index.search_two_phase(q, q_ptr, 10, 20)
    assert torch.equal(a[1], b[1]) and torch.equal(_bits(a[0]), _bits(b[0]))
    with pytest.raises(RuntimeError, match="keep_rows"):
        index.search(q, q_ptr, 5)
    assert kept.search(q, q_ptr, 5)[1].shape == (len(Q_LENS), 5)

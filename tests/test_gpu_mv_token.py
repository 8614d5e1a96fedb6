"""Token retrieval over the compressed store of MultiVectorIndex (csrc/mv_centroid.hip, the mvt_ kernels) on the GPU: with
every centroid probed it is the residual rescore bit for bit; below that, the definition of include/snx.h against float64,
the probe sets taken from the library's own keys; and its invariances."""
import functools

import pytest
import torch

from tests import test_gpu_mv_probe as probe
from tests.test_gpu_mv_centroid import _bits, _store, _unit
from tests.test_gpu_mv_residual import BF16, _codebook, _index

pytestmark = pytest.mark.gpu

FORMS = [(nbits, D) for nbits in (1, 2, 4) for D in (64, 1024)]


def _exclude(nq):
    return [[3, 7, 40 + i] for i in range(nq)]


def _same(got, want):
    return all(torch.equal(g, w) if g.dtype != torch.float32 else torch.equal(_bits(g), _bits(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("nbits,D", FORMS)
def test_every_centroid_probed_is_the_residual_rescore(nbits, D):
    _, _, q, q_ptr, _ = _store(BF16, D)
    index, ex = _index(nbits, D, 48), _exclude(len(q_ptr) - 1)
    assert _same(index.search_tokens(q, q_ptr, 1024, 64), index.search_two_phase(q, q_ptr, 1024, 1024))
    assert _same(index.search_band_tokens(q, q_ptr, 3, 40, 64, exclude=ex),
                 index.search_band_two_phase(q, q_ptr, 3, 40, 1024, exclude=ex))
    assert index.row_list_ptr.dtype == torch.int64 and index.row_list.dtype == torch.int32
    assert torch.equal(index.row_list.long(), torch.sort(index.codes.long(), stable=True).indices)


@functools.lru_cache(maxsize=None)
def _case(nbits, D, nc, kind):
    """(index, ptr, q, q_ptr, t64 [qrows, drows], S64 [qrows, nc], rho, top [qrows, 4]): the float64 row scores of the
    packed form, the float64 centroid products, and the library's own centroid order per query row (``probe._top``'s
    auxiliary index, whose documents are the centroids)."""
    from snx.retrieval import MultiVectorIndex
    if kind == "probe":                                          # D = 64; query 0 probes a centroid that owns no row
        rows, ptr, q, q_ptr = probe._store(BF16, "small")
        index = probe._build(BF16, "small", nc).compress(nbits, *_codebook(nbits, D))
    else:
        rows, ptr, q, q_ptr, _ = _store(BF16, D)
        index = _index(nbits, D, nc)
    cent = index.centroids.double()
    res = rows.float() - index.centroids[index.codes.long()].float()
    wrow = index.weights.double()[torch.bucketize(res, index.cutoffs)]
    t64 = q.double() @ (cent[index.codes.long()] + wrow).T
    aux = MultiVectorIndex(D, "cuda")
    aux.add(index.centroids, list(range(nc + 1)))
    aux.build().set_centroids(_unit(nc, D, 3).cuda())
    assert torch.equal(aux.codes.to(torch.int32).cpu(), torch.arange(nc, dtype=torch.int32))
    top = aux.candidates(q, list(range(q_ptr[-1] + 1)), 4)[1].long()
    return index, ptr, q, q_ptr, t64, q.double() @ cent.T, float(wrow.norm(dim=1).max()), top


@pytest.mark.parametrize("nprobe", (1, 3))
@pytest.mark.parametrize("nbits,D,nc,kind", [(b, D, nc, "plain") for b, D in FORMS for nc in (48, 1500)] + [(2, 64, 4096, "probe")])
def test_definition_against_float64(nbits, D, nc, kind, nprobe):
    index, ptr, q, q_ptr, t64, S64, rho, top = _case(nbits, D, nc, kind)
    nq, nd = len(q_ptr) - 1, len(ptr) - 1
    ex = _exclude(nq)
    codes = index.codes.long()
    hit_row = (codes[None, :, None] == top[:, None, :nprobe]).any(dim=2)          # [qrows, drows]: codes[j] in top(i)
    miss = S64.gather(1, top[:, nprobe:nprobe + 1])                               # S[i, c*(i)]
    masked = torch.where(hit_row, t64, torch.full_like(t64, float("-inf")))
    best = torch.stack([masked[:, a:b].amax(dim=1) if b > a else torch.full_like(miss[:, 0], float("-inf"))
                        for a, b in zip(ptr, ptr[1:])], dim=1)                    # [qrows, nd]
    m = torch.where(best > float("-inf"), best, miss)
    s, d, found = index.search_band_tokens(q, q_ptr, 0, 1024, nprobe, exclude=ex)
    worst, empty_list = 0.0, False
    for i, (a, b) in enumerate(zip(q_ptr, q_ptr[1:])):
        want = set(torch.nonzero((best[a:b] > float("-inf")).any(dim=0)).flatten().tolist()) - set(ex[i])
        got = d[i][d[i] >= 0].long()
        assert int(found[i]) == got.numel() == len(want) and set(got.tolist()) == want     # P(q), each document once
        assert bool((d[i, got.numel():] == -1).all()) and bool((s[i, got.numel():] == 0).all())
        B = (1.01 * D + (b - a) + 5) * 1.02 * (1 + rho) * 2.0 ** -24
        if got.numel():
            err = float((s[i, :got.numel()].double() - m[a:b].mean(dim=0)[got]).abs().max())
            worst = max(worst, err / B)
            assert err <= B, (i, err, B)
        si, di = s[i, :got.numel()].tolist(), got.tolist()
        assert all((-si[j], di[j]) < (-si[j + 1], di[j + 1]) for j in range(len(di) - 1))
        empty_list |= bool((index.row_list_ptr.diff()[top[a:b, :nprobe]] == 0).any())
    assert empty_list or kind != "probe"                          # a probed centroid that owns no row
    print(f"token retrieval nbits={nbits} D={D} nc={nc} nprobe={nprobe}: max err / B = {worst:.3f}")


@pytest.mark.parametrize("nbits,D", FORMS)
def test_independent_of_slices_query_order_and_released_rows(nbits, D):
    _, _, q, q_ptr, _ = _store(BF16, D)
    index, ex = _index(nbits, D, 1500), _exclude(len(q_ptr) - 1)
    want = index.search_band_tokens(q, q_ptr, 0, 50, 3, exclude=ex)
    assert int(want[2].min()) > 0
    for query_slice in (1, 3):
        assert _same(index.search_band_tokens(q, q_ptr, 0, 50, 3, exclude=ex, query_slice=query_slice), want)
    spans = list(zip(q_ptr, q_ptr[1:]))
    rq, rptr = torch.cat([q[a:b] for a, b in reversed(spans)]), [0]
    for a, b in reversed(spans):
        rptr.append(rptr[-1] + b - a)
    back = index.search_band_tokens(rq, rptr, 0, 50, 3, exclude=ex[::-1])
    assert _same([x.flip(0) for x in back], want)
    kept = _index(nbits, D, 1500, True)
    assert kept.rows is not None and index.rows is None
    assert _same(kept.search_band_tokens(q, q_ptr, 0, 50, 3, exclude=ex), want)

"""The fixed-dimensional encodings of snx.retrieval.FdeEncoder (csrc/mv_fde.hip) on the GPU against a float64 restatement of
include/snx.h "multi-vector fixed-dimensional encodings", and the fde=True candidate path of MultiVectorIndex."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 63, 64, 65, 129, 200, 8, 7, 9]                 # across the 64-row tile, sharing tiles, most buckets empty
# (k_sim, reps, d_proj).  (6, 3, 64) has fde_dim = 12,288, past the contract's 4,096: it is held to the refusal, and what it
# stands for (64 buckets, 64-wide projections, three passes) is covered inside the contract by the three cases after it
CONFIGS = [(0, 1, 16), (3, 2, 32), (6, 3, 64), (4, 5, 16), (6, 1, 64), (6, 3, 16), (2, 3, 64)]


def _ptr(total=None):
    lens = LENS + torch.randint(1, 41, (40,), generator=torch.Generator().manual_seed(11)).tolist()
    ptr = [0]
    for n in lens:
        if total is None or ptr[-1] + n <= total:
            ptr.append(ptr[-1] + n)
    return ptr


def _pm1(shape, seed):
    return (2 * torch.randint(0, 2, shape, generator=torch.Generator().manual_seed(seed)) - 1).to(torch.bfloat16)


def _reference(rows, ptr, planes, proj, query):
    """(FDEs, A) in float64: section 1 of the header as written, and the same expression with every product replaced by its
    absolute value."""
    reps, k_sim, _ = planes.shape
    dp, nb, x = proj.shape[1], 1 << k_sim, rows.double()
    scale = float(torch.tensor(1 / math.sqrt(dp), dtype=torch.float32))
    out = torch.zeros(len(ptr) - 1, reps * nb * dp, dtype=torch.float64)
    bound = torch.zeros_like(out)
    pop = torch.tensor([bin(v).count("1") for v in range(64)])
    for r in range(reps):
        code = ((x @ planes[r].double().T > 0).long() << torch.arange(k_sim)).sum(dim=1)
        y, ya = x @ proj[r].double().T, x.abs() @ proj[r].double().abs().T
        for s, (a, e) in enumerate(zip(ptr, ptr[1:])):
            for b in range(nb if e > a else 0):
                hit = code[a:e] == b
                if hit.any():
                    div = 1 if query else int(hit.sum())
                    v, va = y[a:e][hit].sum(dim=0) / div, ya[a:e][hit].sum(dim=0) / div
                elif query:
                    continue
                else:
                    dist = pop[code[a:e] ^ b]
                    j = a + int(torch.nonzero(dist == dist.min())[0])          # ties: the lowest row
                    v, va = y[j], ya[j]
                at = (r * nb + b) * dp
                out[s, at:at + dp], bound[s, at:at + dp] = v * scale, va * scale
    return out, bound


def _encode(rows, ptr, planes, proj):
    from snx.retrieval import FdeEncoder
    enc = FdeEncoder(rows.shape[1], planes.shape[1], planes.shape[0], proj.shape[1], "cuda", planes=planes, proj=proj)
    return enc, enc.encode_documents(rows.cuda(), ptr).cpu(), enc.encode_queries(rows.cuda(), ptr).cpu()


@pytest.mark.parametrize("k_sim,reps,dp", CONFIGS)
@pytest.mark.parametrize("dim", [64, 192])
def test_exact_arithmetic(dim, k_sim, reps, dp):
    """Small integers: every sum is exact in fp32 in any order, zero projections test the > 0 rule, and codes, fills and
    ties are exact; a query FDE has one rounding, a document FDE two."""
    g, ptr = torch.Generator().manual_seed(dim + k_sim), _ptr()
    rows = torch.randint(-2, 3, (ptr[-1], dim), generator=g).to(torch.bfloat16)
    planes = torch.randint(-1, 2, (reps, k_sim, dim), generator=g).to(torch.bfloat16)
    proj = _pm1((reps, dp, dim), 5)
    if reps * (1 << k_sim) * dp > 4096:
        with pytest.raises(ValueError, match="fde_dim"):
            _encode(rows, ptr, planes, proj)
        return
    _, docs, queries = _encode(rows, ptr, planes, proj)
    for got, query in ((docs, False), (queries, True)):
        want, _ = _reference(rows, ptr, planes, proj, query)
        err = (got.double() - want).abs()
        print(f"query={query}: max relative error {float((err / want.abs().clamp(min=1e-30)).max()):.3e}")
        assert bool((err <= 2.0 ** -22 * want.abs()).all())
    assert bool((docs[0] == 0).all()) and docs.dtype == torch.float32 and docs.shape == (len(ptr) - 1, reps * (1 << k_sim) * dp)


@functools.lru_cache(maxsize=None)
def _real():
    rows = torch.randn(700, 128, generator=torch.Generator().manual_seed(6))
    rows = (rows / rows.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
    planes = torch.randn(16, 128, generator=torch.Generator().manual_seed(106)).to(torch.bfloat16).reshape(4, 4, 128)
    return rows, _ptr(700), planes, _pm1((4, 16, 128), 7)


def test_real_data_within_the_accumulation_bound():
    rows, ptr, planes, proj = _real()
    margin = float((rows.double() @ planes.double().reshape(16, 128).T).abs().min())
    assert margin >= 1e-4, margin                              # no fp32 accumulation order can flip a code
    _, docs, queries = _encode(rows, ptr, planes, proj)
    lens = torch.tensor(ptr).diff().double()[:, None]
    for got, query in ((docs, False), (queries, True)):
        want, bound = _reference(rows, ptr, planes, proj, query)
        err, tol = (got.double() - want).abs(), (128 + lens + 2) * 2.0 ** -24 * bound
        print(f"query={query}: max error {float(err.max()):.3e}, largest error / bound {float((err / tol)[tol > 0].max()):.3f}")
        assert bool((err <= tol).all())


def test_an_fde_depends_on_its_own_sequence_alone():
    rows, ptr, planes, proj = _real()
    enc, docs, queries = _encode(rows, ptr, planes, proj)
    order = list(range(len(ptr) - 1))[::-1]
    back, bptr = torch.cat([rows[ptr[s]:ptr[s + 1]] for s in order]).cuda(), [0]
    for s in order:
        bptr.append(bptr[-1] + ptr[s + 1] - ptr[s])
    assert torch.equal(enc.encode_documents(back, bptr).cpu().flip(0).view(torch.int32), docs.view(torch.int32))
    assert torch.equal(enc.encode_queries(back, bptr).cpu().flip(0).view(torch.int32), queries.view(torch.int32))
    for s in (1, 4, 5, 7, 9, 20):                              # alone: 1, 64, 65, 200, 7 rows and a random length
        one = rows[ptr[s]:ptr[s + 1]].cuda()
        assert torch.equal(enc.encode_documents(one, [0, one.shape[0]]).cpu()[0].view(torch.int32), docs[s].view(torch.int32))
        assert torch.equal(enc.encode_queries(one, [0, one.shape[0]]).cpu()[0].view(torch.int32), queries[s].view(torch.int32))


def test_search_with_fde_candidates():
    from snx.retrieval import DenseIndex, MultiVectorIndex
    rows, ptr, planes, proj = _real()
    enc, docs, _ = _encode(rows, ptr, planes, proj)
    index = MultiVectorIndex(128, "cuda")
    index.add(rows.cuda(), ptr)
    index.build().set_fde(enc)
    assert torch.equal(index.fde.cpu().view(torch.int32), docs.view(torch.int32))
    q_ptr = [0, 5, 37, 38]
    q = rows[torch.randint(0, 700, (38,), generator=torch.Generator().manual_seed(3))].cuda()
    nd, exclude = len(ptr) - 1, [[3, 7], [], [4, 12, 20]]
    dense = DenseIndex(enc.fde_dim, "cuda")
    dense.add(docs.cuda())
    dense.build()
    for ncand in (20, 64):                                     # 64: more than the documents with rows, so unused slots
        got = index.candidates(q, q_ptr, ncand, exclude=exclude, fde=True)
        want = dense.search_band(enc.encode_queries(q, q_ptr), 0, ncand, exclude=[e + [0] for e in exclude])   # 0: no rows
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert int((got[1] >= 0).sum(dim=1).max()) < 64 and not bool((got[1] == 0).any())
    got, want = index.search_two_phase(q, q_ptr, 10, nd, fde=True), index.search(q, q_ptr, 10)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    s, d, found = index.search_band_two_phase(q, q_ptr, 2, 8, 20, exclude=exclude, fde=True)
    assert found.tolist() == [6, 6, 6] and not any(int(x) in e for row, e in zip(d.tolist(), exclude) for x in row)

"""Multi-vector teacher scores on the GPU (csrc/maxsim.hip, the head in csrc/teacher.hip, snx.teacher): the MaxSim kernel,
the head's row kernel and the whole path from token ids to scores, each against float64 torch computed here from the same
inputs.

Bound of a MaxSim score over rows already rounded to the store's type: (1.01 D + Lq + 2) 2^-24 -- an fp32 accumulation of D
products of rows with norms <= 1 + 2^-8, which the max inherits, the fp32 sum of Lq values <= 1 and its division, and the
final rounding."""
import ctypes as C
import functools

import pytest
import torch

from tests import teacher_helpers as TH

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = (1, 2, 63, 64, 65, 129, 200)            # the edges of the 64-row query block and the 64-row document tile
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _ref_scores(mv, ptr, pairs):
    x = mv.double()
    return torch.stack([(x[ptr[a]:ptr[a + 1]] @ x[ptr[b]:ptr[b + 1]].t()).amax(dim=1).sum() / (ptr[a + 1] - ptr[a])
                        for a, b in pairs])


@functools.lru_cache(maxsize=None)
def _store(D):
    """One ragged store (float64 unit rows) and its pair list.  Every (Lq, Ld) of ROWS x ROWS is a family of three
    sequences stored one behind the other: the query (its rows within cosine 0.999 of one of a few centres), the document
    (per centre one planted row of cosine ~0.9 -- at the first row, the last row and the tile edges in turn -- and
    otherwise random rows), and a trap holding the centres themselves, so that a read past the document's end meets a
    cosine of 0.999.  Seven more families have documents of -centre + noise: every similarity is negative there and a zero
    or padding row would win the max.  Sequences of equal row counts are also paired with themselves."""
    gen = torch.Generator().manual_seed(1000 + D)
    seqs, pairs = [], []

    def rand(n):
        return _unit(torch.randn(n, D, generator=gen, dtype=torch.float64))

    for negative in (False, True):
        for iq, Lq in enumerate(ROWS):
            for Ld in (ROWS if not negative else (ROWS[(iq + 3) % len(ROWS)],)):
                plant = [0] if negative else sorted({p for p in (0, Ld - 1, 63, 64, 127, 128) if p < Ld})
                centres = rand(len(plant))
                q = _unit(centres[torch.arange(Lq) % len(plant)] + 0.05 * rand(Lq))
                if negative:
                    d = _unit(-centres[0] + 0.3 * rand(Ld))
                else:
                    d = rand(Ld)
                    d[plant] = _unit(0.9 * centres + 0.436 * rand(len(plant)))
                pairs.append((len(seqs), len(seqs) + 1))
                if Lq == Ld:
                    pairs.append((len(seqs) + 1, len(seqs) + 1))
                seqs += [q, d, centres]
    ptr = [0]
    for s in seqs:
        ptr.append(ptr[-1] + s.shape[0])
    return torch.cat(seqs), ptr, pairs


@pytest.mark.parametrize("D", (64, 256, 1024))
@pytest.mark.parametrize("precision", ("bf16", "fp32"))
def test_maxsim_pairs_against_float64(precision, D):
    from snx.teacher import maxsim_pairs
    rows64, ptr, pairs = _store(D)
    mv = rows64.to(DTYPES[precision])                              # rounded once to the store's type
    ref = _ref_scores(mv, ptr, pairs)
    pq, pd = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    dmv, dptr = mv.to(DEV), torch.tensor(ptr)
    got = maxsim_pairs(dmv, dptr, pq, pd)
    err = (got.double().cpu() - ref).abs()
    lq = torch.tensor([ptr[a + 1] - ptr[a] for a, _ in pairs], dtype=torch.float64)
    bound = (1.01 * D + lq + 2.0) * 2.0 ** -24
    print(f"maxsim {precision} D={D}: {len(pairs)} pairs, max err {float(err.max()):.3e}, max err / bound "
          f"{float((err / bound).max()):.3f}, scores in [{float(ref.min()):.3f}, {float(ref.max()):.3f}]")
    assert bool((err <= bound).all())
    assert torch.equal(got, maxsim_pairs(dmv, dptr, pq, pd))       # the same bits from call to call ...
    h = len(pairs) // 2                                            # ... and whatever else is in the pair list
    assert torch.equal(got, torch.cat([maxsim_pairs(dmv, dptr, pq[:h], pd[:h]), maxsim_pairs(dmv, dptr, pq[h:], pd[h:])]))


@pytest.mark.parametrize("H", (256, 768, 1024))
@pytest.mark.parametrize("y_f32", (0, 1))
def test_mv_rows_against_float64(y_f32, H):
    from snx import fn
    from snx._lib import check
    gen = torch.Generator().manual_seed(2000 + H)
    lens = [1, 2, 3, 65, 257]                                      # the one-token sequence owns no row
    T, n = sum(lens), len(lens)
    cu = torch.tensor([0] + lens).cumsum(0)
    dtype = torch.float32 if y_f32 else torch.bfloat16
    y = (1.5 * torch.randn(T, H, generator=gen)).to(dtype)
    y[5] = 0.0                                                     # with the zero bias: the 1e-12 floor, no NaN
    for bias in (0.1 * torch.randn(H, generator=gen), torch.zeros(H)):
        x = y.double() + bias.double()
        x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        ref = torch.empty(T - n, H, dtype=torch.float64)
        for s in range(n):                                         # sequence s owns store rows mv_ptr[s] = cu[s] - s onward:
            for i in range(lens[s] - 1):                           # its tokens behind the first
                ref[int(cu[s]) - s + i] = x[int(cu[s]) + 1 + i]
        mv = torch.full((T - n + 4, H), 7.0, dtype=dtype, device=DEV)
        dy, db, dcu = y.to(DEV), bias.to(DEV), cu.to(torch.int32).to(DEV)
        check(fn("snx_teacher_mv_rows")(C.c_void_p(dy.data_ptr()), y_f32, C.c_void_p(db.data_ptr()),
                                        C.c_void_p(dcu.data_ptr()), C.c_void_p(mv.data_ptr()), T, n, H,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "snx_teacher_mv_rows")
        got = mv.cpu().double()
        assert bool((got[T - n:] == 7.0).all())                    # T - n rows: no CLS row, nothing behind the store
        if y_f32:
            err = (got[:T - n] - ref).abs()
            print(f"mv_rows fp32 H={H}: max abs err {float(err.max()):.3e}")
            assert bool((err <= 1e-5).all())
        else:
            ref_b = ref.float().to(torch.bfloat16).double()
            _, e = torch.frexp(ref_b.abs().clamp_min(2.0 ** -120))
            steps = (got[:T - n] - ref_b).abs() / torch.ldexp(torch.ones_like(ref_b), e - 8)
            print(f"mv_rows bf16 H={H}: max bf16 steps off {float(steps.max()):.3f}")
            assert bool((steps <= 1.0).all())
        if not bool(bias.any()):
            assert bool((got[5 - 2 - 1] == 0).all())               # token row 5 is the last of sequence 2


@functools.lru_cache(maxsize=None)
def _end_to_end_reference():
    """The golden batch through forward_torch and the head in fp32, with emulated bf16 and in float64 -> the pairs, their
    Lq and the three score vectors (float64), all on the CPU."""
    from snx.teacher import forward_torch, maxsim_pairs_torch, multivector_torch, random_colbert_head
    _, cfg, sd = TH.golden()
    head = random_colbert_head(cfg, 77)
    ids, mask = TH.golden_reference("batch")[:2]
    n = int(ids.shape[0])
    pq = torch.tensor([0] * n + list(range(n)))
    pd = torch.tensor(list(range(n)) * 2)
    out = []
    for params, hd, emul in ((sd, head, False), (sd, head, True),
                             ({k: v.double() for k, v in sd.items()}, {k: v.double() for k, v in head.items()}, False)):
        _, _, h = forward_torch(cfg, params, ids, mask, emulate_bf16=emul, return_hidden=True)
        ptr, mv = multivector_torch(hd, h, mask, emulate_bf16=emul)
        out.append(maxsim_pairs_torch(mv, ptr, pq, pd))
    lq = (mask.sum(dim=1) - 1)[pq].double()
    return head, ids, mask, pq, pd, lq, out


@pytest.mark.parametrize("precision", ("bf16", "fp32"))
def test_encode_multivector_end_to_end(precision):
    from snx.teacher import TeacherEncoder, maxsim_pairs
    _, cfg, sd = TH.golden()
    head, ids, mask, pq, pd, lq, (s32, s16, s64) = _end_to_end_reference()
    assert sorted(mask.sum(dim=1).tolist()) == [2, 3, 17, 64, 65, 130, 257]
    enc = TeacherEncoder(cfg, sd, DEV, precision, colbert_head=head)
    emb, mv_ptr, mv = enc.encode_tokens_multivector(ids, mask)
    assert torch.equal(emb, enc.encode_tokens(ids, mask))          # the dense output of the same forward, bit for bit
    assert mv_ptr.tolist() == [0] + torch.cumsum(mask.sum(dim=1) - 1, 0).tolist() and mv.shape[0] == int(mv_ptr[-1])
    got = maxsim_pairs(mv, mv_ptr, pq, pd).double().cpu()
    e_ref = float((s16 - s32).abs().max())
    e32 = float((s32 - s64).abs().max())
    if precision == "bf16":
        to_emul, to_f32 = float((got - s16).abs().max()), float((got - s32).abs().max())
        print(f"end to end bf16: e_ref {e_ref:.3e}  |gpu - emulated| / e_ref = {to_emul / e_ref:.3f}  "
              f"|gpu - fp32 reference| / e_ref = {to_f32 / e_ref:.3f}")
        assert to_emul <= e_ref and to_f32 <= 2.0 * e_ref
    else:
        err = (got - s64).abs()
        bound = 4.0 * e32 + (1.01 * cfg.hidden_size + lq + 2.0) * 2.0 ** -24
        print(f"end to end fp32: e32 {e32:.3e}  max |gpu - float64| {float(err.max()):.3e}  max err / bound "
              f"{float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())

"""Dense teacher encoder on the GPU (csrc/teacher.hip, snx.teacher): every row kernel alone against float64 torch, the fp32
attention against float64 SDPA, the whole forward in both precisions against the transformers golden
(tests/golden/g21_teacher) and against ``forward_torch``, determinism, batching, and the reference API on top of it.

Tolerances.  fp32 outputs: 1e-5 of the row's largest magnitude (the project's fp32 figure).  bf16 outputs of a kernel: one
bf16 step of the float64 value rounded to bf16.  The bf16 forward: e_ref = max |forward_torch(emulate_bf16) -
forward_torch(fp32)|, the comparator's own number computed on the CPU; the GPU must lie within e_ref of the emulated run and
within 2 e_ref of the fp32 reference (accumulation order, the device exp / erf and single bf16 rounding flips, each worth
one bf16 step)."""
import ctypes as C

import pytest
import torch

from tests import teacher_helpers as TH

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HS = (256, 768, 1024)
TS = (1, 63, 130)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _call(name, *args):
    from snx import fn
    from snx._lib import check
    check(fn(name)(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
    torch.cuda.synchronize()


def _bf16_step(ref_b: torch.Tensor) -> torch.Tensor:
    """One bf16 step at the magnitude of ``ref_b`` (float64 values that are bf16 numbers)."""
    _, e = torch.frexp(ref_b.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(ref_b), e - 8)


def _assert_f32(got, ref64, what):
    err = (got.double().cpu() - ref64).abs().amax(dim=-1)
    bound = 1e-5 * ref64.abs().amax(dim=-1)
    print(f"{what}: max err / row max = {float((err / ref64.abs().amax(dim=-1).clamp_min(1e-30)).max()):.3e}")
    assert bool((err <= bound).all()), what


def _assert_bf16(got, ref64, what):
    ref_b = ref64.float().to(torch.bfloat16).double()
    d = (got.double().cpu() - ref_b).abs()
    steps = d / _bf16_step(ref_b)
    print(f"{what}: max bf16 steps off = {float(steps.max()):.3f}")
    assert bool((steps <= 1.0).all()), what


def _ln64(x, w, b, eps=1e-5):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w.double(), b.double(), eps)


def _ln_params(H, gen):
    return 1.0 + 0.2 * torch.randn(H, generator=gen), 0.1 * torch.randn(H, generator=gen)


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("T", TS)
def test_embed_ln(H, T):
    gen = torch.Generator().manual_seed(100 + H + T)
    V, P = 300, 300
    word, pos, typ = (0.1 * torch.randn(n, H, generator=gen) for n in (V, P, 1))
    w, b = _ln_params(H, gen)
    ids = torch.randint(0, V, (T,), generator=gen)
    pid = torch.randint(2, P, (T,), generator=gen, dtype=torch.int32)
    ids[0], pid[-1] = V - 1, P - 1                                # the last rows of both tables
    ref = _ln64((word[ids].double() + typ[0].double()) + pos[pid.long()].double(), w, b)
    d = [t.to(DEV) for t in (ids, pid, word, pos, typ, w, b)]
    h = torch.empty(T, H, device=DEV)
    x = torch.empty(T, H, dtype=torch.bfloat16, device=DEV)
    _call("snx_teacher_embed_ln", *map(_p, d), _p(h), _p(x), T, H, V, P, 1e-5)
    _assert_f32(h, ref, "embed_ln h")
    _assert_bf16(x, ref, "embed_ln bf16(h)")
    h2 = torch.empty(T, H, device=DEV)
    _call("snx_teacher_embed_ln", *map(_p, d), _p(h2), _p(None), T, H, V, P, 1e-5)      # fp32 form: no bf16 copy
    assert torch.equal(h, h2)


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("y_f32", (0, 1))
def test_bias_resid_ln(H, T, y_f32):
    gen = torch.Generator().manual_seed(200 + H + T)
    h = torch.randn(T, H, generator=gen)
    y = torch.randn(T, H, generator=gen)
    y = y if y_f32 else y.to(torch.bfloat16)
    bias = 0.1 * torch.randn(H, generator=gen)
    w, b = _ln_params(H, gen)
    ref = _ln64((y.double() + bias.double()) + h.double(), w, b)
    dh, dy, dbias, dw, db = (t.to(DEV) for t in (h, y, bias, w, b))
    out = torch.empty(T, H, device=DEV)
    x = torch.empty(T, H, dtype=torch.bfloat16, device=DEV)
    _call("snx_teacher_bias_resid_ln", _p(dh), _p(dy), y_f32, _p(dbias), _p(dw), _p(db), _p(out), _p(x), T, H, 1e-5)
    _assert_f32(out, ref, "bias_resid_ln h_out")
    _assert_bf16(x, ref, "bias_resid_ln bf16(h_out)")
    _call("snx_teacher_bias_resid_ln", _p(dh), _p(dy), y_f32, _p(dbias), _p(dw), _p(db), _p(dh), _p(None), T, H, 1e-5)
    assert torch.equal(dh, out)                                   # in place on h, without the bf16 copy: the same bits


@pytest.mark.parametrize("N", (8, 512, 4096))
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("gelu", (False, True))
def test_bias_rows_and_bias_gelu(N, T, gelu):
    gen = torch.Generator().manual_seed(300 + N + T)
    y = 1.5 * torch.randn(T, N, generator=gen)                    # the scale of a Linear's output in this model
    bias = 0.1 * torch.randn(N, generator=gen)
    name = "snx_teacher_bias_gelu" if gelu else "snx_teacher_bias_rows"

    def ref(y64):
        s = y64 + bias.double()
        return torch.nn.functional.gelu(s) if gelu else s

    a, dbias = y.to(DEV), bias.to(DEV)
    _call(name, _p(a), 1, _p(dbias), T, N)
    _assert_f32(a, ref(y.double()), name + " fp32")
    yb = y.to(torch.bfloat16)
    a = yb.to(DEV)
    _call(name, _p(a), 0, _p(dbias), T, N)
    _assert_bf16(a, ref(yb.double()), name + " bf16")


@pytest.mark.parametrize("H", HS)
def test_cls_normalize(H):
    gen = torch.Generator().manual_seed(400 + H)
    lens = [1, 63, 2, 64]
    T = sum(lens)
    h = torch.randn(T, H, generator=gen)
    h[1] = 0.0                                                    # the CLS row of sequence 1 is all zero: no NaN
    cu = torch.tensor([0, 1, 64, 66, 130], dtype=torch.int32)
    cls = torch.empty(4, H, device=DEV)
    emb = torch.empty(4, H, device=DEV)
    dh, dcu = h.to(DEV), cu.to(DEV)
    _call("snx_teacher_cls_normalize", _p(dh), _p(dcu), _p(cls), _p(emb), T, 4, H)
    rows = h[cu[:-1].long()]
    assert torch.equal(cls.cpu(), rows)
    ref = rows.double() / rows.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    assert bool(torch.isfinite(emb).all()) and bool((emb[1] == 0).all())
    keep = torch.tensor([0, 2, 3])
    _assert_f32(emb.cpu()[keep], ref[keep], "cls_normalize emb")


# the edges of the tiled forward this entry point runs (csrc/f32_path.hip): 128-query blocks, 64-key tiles, a grid whose third
# dimension follows the MEAN sequence length
@pytest.mark.parametrize("lens,heads", [([1, 2, 65, 257], 4),            # more than one block and tile, nothing a multiple
                                        ([1], 1),                        # T = 1: one block, one key
                                        ([128, 129, 64, 63], 4),         # exact and off-by-one query blocks and key tiles
                                        ([3] * 40, 4)],                  # mean length far below one query block
                         ids=["ragged", "one_token", "block_edges", "forty_short"])
def test_attn_f32_against_float64_sdpa(lens, heads):
    gen = torch.Generator().manual_seed(500)
    T = sum(lens)
    qkv = torch.randn(T, 3, heads, 64, generator=gen)
    cu = torch.tensor([0] + lens, dtype=torch.int32).cumsum(0, dtype=torch.int32)
    out = torch.empty(T, heads, 64, device=DEV)
    dqkv, dcu = qkv.to(DEV), cu.to(DEV)
    _call("snx_teacher_attn_f32", _p(dqkv), _p(dcu), _p(out), T, len(lens), heads)
    ref = torch.empty(T, heads, 64, dtype=torch.float64)
    for s in range(len(lens)):
        a, b = int(cu[s]), int(cu[s + 1])
        q, k, v = (qkv[a:b, j].double().transpose(0, 1) for j in range(3))            # [heads, len, 64]
        ref[a:b] = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(0, 1)
    _assert_f32(out.reshape(T, heads * 64), ref.reshape(T, heads * 64), "attn_f32")


def _encoder(cfg, sd, precision):
    from snx.teacher import TeacherEncoder
    return TeacherEncoder(cfg, sd, DEV, precision)


def _check_forward(cfg, sd, ids, mask, e32, e16, e_ref, what, golden_emb=None):
    """The two rules of the module docstring, on unit embeddings."""
    g32 = _encoder(cfg, sd, "fp32").encode_tokens(ids, mask).cpu()
    err32 = float((g32 - (e32 if golden_emb is None else golden_emb)).abs().max())
    print(f"{what}: fp32 max abs err {err32:.3e}")
    assert err32 <= 1e-5
    g16 = _encoder(cfg, sd, "bf16").encode_tokens(ids, mask).cpu()
    to_emul, to_f32 = float((g16 - e16).abs().max()), float((g16 - (e32 if golden_emb is None else golden_emb)).abs().max())
    print(f"{what}: e_ref {e_ref:.3e}  |gpu bf16 - emulated| / e_ref = {to_emul / e_ref:.3f}  "
          f"|gpu bf16 - fp32 reference| / e_ref = {to_f32 / e_ref:.3f}")
    assert to_emul <= e_ref and to_f32 <= 2.0 * e_ref


@pytest.mark.parametrize("call", ("batch", "single"))
def test_forward_against_the_transformers_golden(call):
    _, cfg, sd = TH.golden()
    ids, mask, gcls, gemb, e32, e16, e_ref = TH.golden_reference(call)
    _check_forward(cfg, sd, ids, mask, e32, e16, e_ref, f"golden {call}", golden_emb=gemb)
    cls = _encoder(cfg, sd, "fp32").encode_tokens(ids, mask, normalize=False).cpu()
    assert bool(((cls - gcls).abs().amax(dim=1) <= 1e-5 * gcls.abs().amax(dim=1)).all())


@pytest.mark.parametrize("hidden", (768, 1024))
def test_one_layer_wide_models(hidden):
    from snx.teacher import forward_torch, normalize_state_dict, random_state_dict
    cfg = TH.one_layer_config(hidden)
    sd = normalize_state_dict(cfg, random_state_dict(cfg, 30 + hidden))
    ids, mask = TH.pad_batch(TH.ragged_sequences([2, 64, 65, 130]))
    _, e32 = forward_torch(cfg, sd, ids, mask)
    _, e16 = forward_torch(cfg, sd, ids, mask, emulate_bf16=True)
    _check_forward(cfg, sd, ids, mask, e32, e16, float((e16 - e32).abs().max()), f"one layer, hidden {hidden}")


@pytest.mark.parametrize("precision", ("bf16", "fp32"))
def test_determinism_batching_and_order(precision):
    _, cfg, sd = TH.golden()
    ids, mask, _, _, e32, e16, e_ref = TH.golden_reference("batch")
    enc = _encoder(cfg, sd, precision)
    a, b = enc.encode_tokens(ids, mask), enc.encode_tokens(ids, mask)
    assert torch.equal(a, b)
    tok = TH.ToyTokenizer(cfg.vocab_size)
    small = enc.encode(TH.TEXTS, tok, max_length=256, batch_tokens=130).cpu()
    large = enc.encode(TH.TEXTS, tok, max_length=256, batch_tokens=16384).cpu()
    bound = 1e-5 if precision == "fp32" else e_ref
    print(f"{precision}: |budget 130 - budget 16384| = {float((small - large).abs().max()):.3e} (bound {bound:.3e})")
    assert float((small - large).abs().max()) <= bound
    for i, t in enumerate(TH.TEXTS):                               # row i is text i, whatever the sorted packing did
        one = enc.encode([t], tok, max_length=256).cpu()
        assert float((one[0] - large[i]).abs().max()) <= bound, i


def test_ranking_scores_equal_dense_index_pair_scores():
    from snx.retrieval import DenseIndex
    from src.model.teachers import BGEM3Teacher
    _, cfg, sd = TH.golden()
    teacher = BGEM3Teacher(_encoder(cfg, sd, "bf16"), device=DEV, max_length=64, tokenizer=TH.ToyTokenizer(cfg.vocab_size))
    queries, docs = TH.TEXTS[:6], TH.TEXTS[6:]
    scores = teacher.get_ranking_scores(queries, docs)
    q, d = teacher.encode(queries), teacher.encode(docs)
    index = DenseIndex(cfg.hidden_size, DEV)
    index.add(d)
    index.build()
    pairs = torch.arange(6, device=DEV).repeat(2, 1).t().contiguous()
    ps = index.pair_scores(q, pairs)
    assert float((scores - ps).abs().max()) <= 1e-5               # one fp32 dot product of unit vectors, two summation orders

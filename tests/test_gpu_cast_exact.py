"""The weight-cache casts (csrc/elementwise.hip: snx_cast_bf16, snx_cast_transpose_bf16, snx_cast_geglu_interleave), bit
for bit against x.to(torch.bfloat16) on the CPU (round to nearest even), into guarded outputs.  They produce the operands
of the weight-gradient GEMM family and define the interleaved GeGLU order its `interleaved` problems undo.

Inputs: randn over several binades, exact ties (low half 0x8000 above an even and above an odd bf16 mantissa, both signs),
the largest fp32 (rounds to infinity), both zeros, both infinities and NaN (NaN-ness compared, not the payload).  fp32
subnormals stay out: nothing states the conversion's denormal mode.
Shapes: every tail of the 4-wide cast and its grid clamp at 4096 blocks; transposes with partial 64 x 64 tiles in either
direction; the interleave with `out` only, `out_t` only and both.  The round trip feeds snx_gemm_tn_accum_interleaved a dY
whose columns snx_cast_geglu_interleave itself ordered: the gradient lands in the rows of the natural Wi, exactly.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tn_reference as T

pytestmark = pytest.mark.gpu
GR = T.GUARD_ROWS
SENT = 0x7FA5                                        # gemm_reference.SENT_BF16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(n, seed):
    """n fp32 values (CPU): randn x 2^(-20..20), then the special values dealt over the front and the back"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 21, (n,), generator=g).float())
    ties = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F7F8000, 0x00808000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,
            0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x3F800001, 0x3F807FFF, 0x3F808001]
    sp = torch.from_numpy(np.array(ties, dtype=np.uint32).view(np.float32).copy())
    k = min(n, len(sp))
    x[:k] = sp[:k]
    if n >= 2 * len(sp):
        x[n - len(sp):] = sp.flip(0)
    a = x.abs()
    assert not bool(((a > 0) & (a < 2.0 ** -126)).any())
    return x


def _equal_bf16(got, want, what):
    """bit for bit, NaN for NaN"""
    gb, wb = got.view(torch.int16), want.view(torch.int16)
    nan_g, nan_w = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(nan_g, nan_w), f"{what}: NaN in other places"
    bad = ((gb != wb) & ~nan_w).nonzero()
    assert bad.numel() == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}"


def _guards_1d(buf, n, what):
    raw = buf.view(torch.int16)
    assert bool((raw[:1024] == SENT).all()) and bool((raw[1024 + n:] == SENT).all()), f"{what}: guard written"


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 4096 * 1024 + 5])
def test_cast_bf16(dev, n):
    from snx._lib import call
    from snx.ops import _p, _stream
    x = _inputs(n, n)
    xd = x.to(dev)
    buf = torch.full((n + 2048,), SENT, dtype=torch.int16, device=dev).view(T.BF16)
    out = buf[1024:1024 + n]
    call("snx_cast_bf16", _p(xd), _p(out), n, _stream())
    torch.cuda.synchronize()
    _guards_1d(buf, n, f"cast_bf16 n={n}")
    _equal_bf16(out.cpu(), x.to(T.BF16), f"cast_bf16 n={n}")


def test_cast_bf16_refuses_misaligned_pointers(dev):
    from snx._lib import fn
    from snx.ops import _stream
    x = torch.zeros(64, device=dev)
    out = torch.zeros(64, dtype=T.BF16, device=dev)
    f = fn("snx_cast_bf16")
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 8 == 0
    assert f(C.c_void_p(x.data_ptr() + 4), C.c_void_p(out.data_ptr()), 8, _stream()) == -3
    assert f(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr() + 2), 8, _stream()) == -3
    assert f(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 8, _stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("R,Cc", [(1, 1), (63, 65), (64, 64), (200, 130), (768, 1152)])
def test_cast_transpose_bf16(dev, R, Cc):
    from snx._lib import call
    from snx.ops import _p, _stream
    x = _inputs(R * Cc, R + Cc).view(R, Cc)
    buf, out = T.guarded(Cc, R, T.BF16, dev)
    call("snx_cast_transpose_bf16", _p(x.to(dev)), _p(out), R, Cc, _stream())
    torch.cuda.synchronize()
    T.check_guards(buf, Cc, f"cast_transpose {R}x{Cc}")
    _equal_bf16(out.cpu(), x.to(T.BF16).t().contiguous(), f"cast_transpose {R}x{Cc}")


@pytest.mark.parametrize("which", ["out", "out_t", "both"])
@pytest.mark.parametrize("I,Cc", [(32, 64), (96, 130), (1152, 768)])
def test_cast_geglu_interleave(dev, I, Cc, which):
    from snx._lib import call
    from snx.ops import _p, _stream
    x = _inputs(2 * I * Cc, I + Cc).view(2 * I, Cc)
    want = x[torch.from_numpy(T.src_rows(2 * I))].to(T.BF16)                    # out rows = bf16(in[geglu_src_row])
    (b0, o0), (b1, o1) = T.guarded(2 * I, Cc, T.BF16, dev), T.guarded(Cc, 2 * I, T.BF16, dev)
    call("snx_cast_geglu_interleave", _p(x.to(dev)), _p(o0) if which != "out_t" else C.c_void_p(0),
         _p(o1) if which != "out" else C.c_void_p(0), I, Cc, _stream())
    torch.cuda.synchronize()
    T.check_guards(b0, 2 * I, f"interleave {I}x{Cc} out")
    T.check_guards(b1, Cc, f"interleave {I}x{Cc} out_t")
    if which != "out_t":
        _equal_bf16(o0.cpu(), want, f"interleave {I}x{Cc} out")
    else:
        assert bool((o0.view(torch.int16) == SENT).all()), "out written though it was not asked for"
    if which != "out":
        _equal_bf16(o1.cpu(), want.t().contiguous(), f"interleave {I}x{Cc} out_t")
    else:
        assert bool((o1.view(torch.int16) == SENT).all()), "out_t written though it was not asked for"


@pytest.mark.parametrize("tn256", [0, 1])
def test_interleave_round_trip_through_the_weight_gradient(dev, tn256):
    """dY's columns ordered by snx_cast_geglu_interleave itself (the transposed output of the cast of dY_natural^T), then
    snx_gemm_tn_accum_interleaved: dW = dW0 + dY_natural^T X in the rows of the natural Wi -- exact family, as bits"""
    import snx
    from snx._lib import call, fn
    from snx.ops import TnProblem, _p, _stream
    M, I, K = 200, 192, 256
    N = 2 * I
    c = T.build_case("exact", ((N, K, 0),), M)                                   # dY in natural order
    dy_nat, x = T.operands(c, 0)
    src = dy_nat.float().t().contiguous().to(dev)                               # [2I, M] fp32, bf16-exact values
    dyb, dy = T.guarded(M, N, T.BF16, dev)
    call("snx_cast_geglu_interleave", _p(src), C.c_void_p(0), _p(dy), I, M, _stream())
    torch.cuda.synchronize()
    assert torch.equal(dy.cpu(), dy_nat[:, torch.from_numpy(T.src_rows(N))])
    saved = {k: snx.config(k) for k in ("tn256", "tn256_min_m")}
    try:
        snx.configure(tn256=tn256, tn256_min_m=1)
        sizes = (TnProblem * 1)(TnProblem(0, 0, 0, N, K, 1, 0))
        nbytes = int(fn("snx_gemm_tn_workspace_bytes")(sizes, 1, M))
        ws = T.workspace(nbytes, dev)
        buf, dw = T.guarded_dw(c.dW0[0], dev)
        xd = c.X[0].to(dev)
        call("snx_gemm_tn_accum_interleaved", _p(dy), _p(xd[GR:GR + M]), _p(dw), M, N, K, _p(ws) if nbytes else C.c_void_p(0),
             nbytes, _stream())
        torch.cuda.synchronize()
    finally:
        snx.configure(**saved)
    T.check_workspace(ws, nbytes, "round trip")
    st = T.check_guarded(buf.cpu(), T.expected(c, None)[0], "round trip")
    assert st.single == 1.0
    assert torch.equal(T._raw(dw.cpu()), T._raw(c.want[0]))

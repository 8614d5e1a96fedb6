"""Float64 restatement of the NT GEMM family (csrc/gemm.hip, gemm_nt256.hip, gemm_nt_pipe.hip, gemm_core.h, gemm_epi.h),
the case tables, a restatement of the two persistent kernels' launch arithmetic, and a per-element check whose acceptance
SETS follow from the kernels' documented cast points.  Plain torch / numpy on the CPU; sibling of
tests/attention_reference.py and tests/splade_fwd_reference.py.

The operation.  All six entry points form acc = sum_k A[m,k] B[n,k] from bf16 operands, accumulated in fp32 by the MFMA,
and the Linear's output is c = bf16(acc), round to nearest even.  Epilogues, cast points as in gemm.hip's accumulator ->
staging-image block and csrc/common.h (rbf, mul_rn, gelu_f, gelu_grad_f); fl32 = one fp32 operation:
    snx_gemm_nt_bf16          c
    snx_gemm_nt_resid         fl32(Hin + float(c))
    snx_gemm_nt_rope, _rows   columns < rope_cols, per 64-column head, pairs (d, d + 32), x = float(c):
                              lo = bf16(fl32(fl32(x1 cos) - fl32(x2 sin))), hi = bf16(fl32(fl32(x2 cos) + fl32(x1 sin))),
                              (cos, sin) = tab[pos[row]][d]; the four products rounded separately.  Other columns: c.
    snx_gemm_nt_geglu_fwd     u = c in the interleaved column order (per 64 columns: 32 of a, then 32 of g);
                              y = bf16(G(a) g), G(a) = bf16(gelu_f(a))            (the product of two bf16 is exact in fp32)
    snx_gemm_nt_geglu_bwd     dy = c; a, g from the saved u [M, 2N]; dg = bf16(dy G(a)); da = bf16(fl32(bf16(dy g) gelu'(a)))
                              with gelu' in fp32; du in the interleaved order of u.

Acceptance set, not a tolerance.  Every step above is a rounding or an fp32 operation that is monotone in each argument,
so the reference carries per element an interval [lo, hi] of admissible results and a result passes iff lo <= x <= hi.
  start     S = float64 sum of the exact products, Abs = sum_k |a_k| |b_k|, delta = gamma_n Abs with
            gamma_n = n 2^-24 / (1 - n 2^-24), n = K + 8 -- the convention of _tn_check in tests/test_gpu_ops.py (Higham,
            Accuracy and Stability, 4.2) -- plus K 2^-52 Abs for the float64 sum itself.
            ASSUMPTION (MFMA-ADD): each of the MFMA's additions errs by at most 2^-24 of its result, in whatever order
            it adds; the products of two bf16 values are exact.  The guides do not state the MFMA's internal order or
            rounding; nothing else about the hardware's sum is assumed.
            c in [bf16(S - delta), bf16(S + delta)]        (bf16() below: bf16_round, exact integer arithmetic on the bits)
  epilogue  evaluated exactly at the corners of the incoming intervals, min and max taken.  numpy's float32 multiply and
            add are the IEEE operations v_mul_f32 / v_add_f32 perform; the inputs keep clear of subnormals (asserted
            where a rounding is taken).  GELU is not monotone (minimum near -0.75): G over an interval of a is the
            union over EVERY bf16 value in it, not its corners.

gelu_f and gelu_grad_f use v_rcp_f32, v_exp_f32 and a degree-6 fit (csrc/common.h, gelu_cdf_exp) and cannot be
reproduced bit for bit on the CPU.  Their argument is a bf16 value, so gelu_table() tabulates, over all finite bf16 x, an
interval around the float64 x Phi(x) and Phi(x) + x phi(x).  Half-width, DERIVED from the source, u = 2^-24:
    t = rcp(fma(|x|, c1, 1))           relative error eps_t = u (the fma) + ULP_RCP 2u
                                       ASSUMPTION (RCP-EXP): v_rcp_f32 and v_exp_f32 are accurate to 1 ulp (<= 2u
                                       relative); the guides give no figure.
    P(t), six fmas                     running error bound of Horner's rule (Higham 5.1): err <- err t + u |p| per step
    Q = P t                            err_Q = err_P t + u |Q| + |Q'(t)| t eps_t, Q' = P + t P' evaluated in float64
    e = exp2(fl32(x x c2))             x x is exact (bf16 x bf16); the product with c2 is one rounding of an exponent y:
                                       eps_e = ULP_EXP 2u + 2u ln2 |y| (rounding of the product and of the constant c2)
    h = 0.5 Q e = erfc(|x|/sqrt2)/2    err_h = 0.5 e err_Q + h (eps_e + 2u) + fit(x) + 2^-125.  fit(x) = |formula - truth|, the
                                       formula of gelu_cdf_exp evaluated in float64 WITH its fp32-rounded constants against
                                       erfc: the fit error and the rounding of the nine constants, per input, from the
                                       source alone.  (The header states "3.5e-9 absolute" for the fit: measured in float64
                                       that is the error of h = erfc / 2 with the decimal constants, 3.6e-9; rounding the
                                       constants to fp32 raises it to 2.2e-8 at x = 0, where the coefficients no longer
                                       sum to 1 -- tests/test_gemm_reference_host.py prints both.)  2^-125: a flushed e or h
    cdf = 1 - h (x >= 0) or h          err_cdf = err_h + u cdf for x >= 0 (the subtraction)
    gelu_f = x cdf                     err = |x| err_cdf + u |x cdf|
    gelu_grad_f = fma(x, c3 e, cdf)    err = |x| phi (eps_e + 2u) + err_cdf + u |gelu'|     (c3 e: a rounding; c3 rounded)
  each times 1.01 for the products of two of the terms.  G(a) = bf16(gelu_f(a)) is then in [bf16(gelu - err),
  bf16(gelu + err)]; gelu' in the fp32 values that enclose [gelu' - err, gelu' + err].  No half-width was fitted to a kernel.

Two input families.
  exact     A and B are multiples of 2^-3 with |.| <= 1/2 (rows alternate between symmetric, non-negative and large-only
            value sets so that the sums cover several binades), the saved u and the residual are bf16-exact values in
            GELU's interesting range.  Every product and partial sum is a multiple of 2^-6 below 2^18: exact in fp32 in
            any order, delta = 0 (the sum is formed as an integer matrix product, exact in float32 on the CPU as well),
            c is pinned to ONE bf16 value, round-to-even ties included.  Store, residual, RoPE and the u half of the GeGLU
            forward are then pinned to one value with no assumption at all; y, da and dg up to the gelu table.  Any K.
  random    randn for A, 0.05 randn for B (what tests/test_gpu_ops.py uses), K <= 1152: delta stays below an eighth of
            a mean term (8 K^2 2^-24 <= 1), the acceptance set cannot swallow a dropped or doubled product.

The residual epilogue is checked against the SET inside its fp32 interval: a result must be fl32(Hin + v) for a bf16 v of
c's set (ep_resid).  Exact requirements besides the interval (check_guarded): the outputs live inside larger buffers pre-filled with a NaN
sentinel bit pattern, GUARD_ROWS = 128 guard rows before and after; the guards are untouched, every element is written
and finite.  Columns >= rope_cols equal c (their interval is c's), rope and rope_rows return the same bits, two runs
return the same bits (tests/test_gpu_gemm_per_element.py).

Launch arithmetic restated: nt256_plan (gemm_nt256.hip launch() and next_tile: tile grid, column-group cost model,
per-XCD whole rounds, leftover 64-row units, column-run or tile-order dealing) and pipe_plan (gemm_nt_pipe.hip: workgroup
count, tiles per workgroup, empty workgroups).  The case tables ASSERT the class of every shape through them.

Measured on an MI355X with the kernels of commit f602ce6 (the change that adds this file touches no kernel), against
this reference, over all cases of tests/test_gpu_gemm_per_element.py.  Nothing fell outside its acceptance set.  "one" =
share of the checked elements whose set is a single value (each met it: bit for bit), "two" = share with two adjacent
admissible values, "low" = share of those at the lower end (the rest at the upper end); the remainder has wider sets:
    form       family  epilogue    elements      one        two       low
    128x128    exact   store           838,476   100 %      -
                       resid           838,476   100 %      -
                       rope (+rows)  5,586,688   100 %      -
                       geglu_fwd     1,063,392   99.830 %   0.079 %   47.8 %     (u: 100 %; y up to the gelu table)
                       geglu_bwd     1,539,136   99.923 %   0.077 %   42.4 %
               random  store           842,572   59.964 %   28.632 %  50.1 %
                       resid           842,572   59.964 %   28.632 %  50.1 %
                       rope (+rows)  5,603,072   56.728 %   28.352 %  50.0 %
                       geglu_fwd     1,069,536   51.175 %   28.549 %  50.1 %
                       geglu_bwd     1,547,328   62.143 %   22.461 %  50.0 %
    256x256    exact   store        72,147,712   100 %      -
                       resid        72,147,712   100 %      -
                       rope (+rows) 150,516,224  100 %      -
                       geglu_fwd   108,221,568   100.000 %  0.000 %              (rounded; u: 100 %)
                       geglu_bwd   144,295,424   99.923 %   0.077 %   42.5 %
               random  store        72,147,712   93.011 %   6.018 %   50.0 %
                       resid        72,147,712   93.011 %   6.018 %   50.0 %
                       rope (+rows) 150,516,224  94.980 %   3.692 %   50.0 %
                       geglu_fwd   108,221,568   91.405 %   6.737 %   50.0 %
                       geglu_bwd   144,295,424   93.783 %   4.466 %   50.0 %
    pipelined  exact   geglu_bwd    99,418,112   99.921 %   0.079 %   42.7 %     (nt_pipe 2 and 1: same bits)
               random  geglu_bwd     2,686,976   51.122 %   28.434 %  50.1 %
    chain of a layer, both forms       588,800   81.312 %   13.683 %  50.1 %
(The random 128x128 cases reach K = 1152, the 256x256 cases K <= 256: gamma_n grows with K and so do the sets.)
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

BF16 = torch.bfloat16
U32 = 2.0 ** -24
GUARD_ROWS = 128
ULP_RCP = 1
ULP_EXP = 1
FIT = 3.5e-9                # what csrc/common.h states for the erfc fit (see the docstring)
SENT_BF16 = 0x7FA5          # a NaN: an element never written fails the finiteness check
SENT_F32 = 0x7FA5A5A5
ENTRIES = ("store", "resid", "rope", "rope_rows", "geglu_fwd", "geglu_bwd")
MAX_POS = 512

_MASK45 = np.uint64((1 << 45) - 1)
_SIGN = np.uint64(1 << 63)
BF16_MAX = float.fromhex("0x1.fep127")
BF16_MIN = 2.0 ** -126


# ----------------------------------------------------------------------------- roundings
def _check_range(out):
    a = np.abs(out)
    assert bool(np.all((a == 0) | ((a >= BF16_MIN) & (a <= BF16_MAX)))), "value outside the normal bf16 range"


def bf16_round(x, check=True):
    """float64 -> nearest bf16 (ties to even), returned as float64.  Integer arithmetic on the float64 bits: the 45 low
    significand bits are rounded away in one step -- no detour through fp32 (no double rounding)."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    sign, mag = b & _SIGN, b & ~_SIGN
    r = (mag + np.uint64((1 << 44) - 1) + ((mag >> np.uint64(45)) & np.uint64(1))) & ~_MASK45
    out = (r | sign).view(np.float64)
    if check:
        _check_range(out)
    return out


def bf16_trunc(x):
    """float64 -> bf16 by dropping the low bits (a planted fault, never the reference)."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return (b & ~_MASK45).view(np.float64)


def bf16_ord(v):
    """bf16 values held in float64 -> a signed integer that is monotone in the value (+-0 -> 0)."""
    bits = (np.ascontiguousarray(v, dtype=np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.int64)
    return np.where(bits & 0x8000, -(bits & 0x7FFF), bits)


def f32_down(x):
    r = x.astype(np.float32)
    return np.where(r.astype(np.float64) > x, np.nextafter(r, np.float32(-np.inf)), r).astype(np.float64)


def f32_up(x):
    r = x.astype(np.float32)
    return np.where(r.astype(np.float64) < x, np.nextafter(r, np.float32(np.inf)), r).astype(np.float64)


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def to_np(t):
    """torch tensor (bf16 / fp32) -> float64 numpy, exactly."""
    return t.detach().cpu().to(torch.float64).numpy()


# ----------------------------------------------------------------------------- the gelu table
C1, C2, C3 = (float(np.float32(v)) for v in (0.23164189, -0.72134752, 0.39894228040143268))
POLY_DEC = (-0.29844744, 1.50480362, -2.08551838, 2.04007077, -0.74904709, 0.43109737, 0.15704115)
POLY = tuple(float(np.float32(v)) for v in POLY_DEC)


def all_bf16():
    """every finite bf16 value, as float64, in bit order of the 65,536 patterns (Inf / NaN patterns dropped)."""
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return bits, (bits << 16).view(np.float32).astype(np.float64)


def gelu_fit_f64(x, poly=POLY, c1=C1, c2=C2):
    """the formula of gelu_cdf_exp in float64 with its fp32 constants: (h = erfc(|x|/sqrt2)/2, e, t, P, Q')."""
    t = 1.0 / (1.0 + np.abs(x) * c1)
    e = np.exp2(x * x * c2)
    p, dp = np.full_like(x, poly[0]), np.zeros_like(x)
    for c in poly[1:]:
        dp = dp * t + p
        p = p * t + c
    return 0.5 * (p * t) * e, e, t, p, p + t * dp


@functools.lru_cache(maxsize=1)
def gelu_table():
    """ord-indexed (bf16_ord + 0x7F7F) arrays: g_lo, g_hi (bf16 values G(a) may take), d_lo, d_hi (fp32 values gelu_grad_f
    may take).  Derivation: the module docstring."""
    from scipy.special import erfc
    bits, x = all_bf16()
    ax = np.abs(x)
    phi_cdf = 0.5 * erfc(-x / math.sqrt(2.0))
    pdf = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    gelu, grad = x * phi_cdf, phi_cdf + x * pdf
    h, e, t, p, dq = gelu_fit_f64(x)
    eps_t = U32 + ULP_RCP * 2 * U32
    pp, err_p = np.full_like(x, POLY[0]), np.zeros_like(x)
    for c in POLY[1:]:
        pp = pp * t + c
        err_p = err_p * t + U32 * np.abs(pp)
    q = p * t
    err_q = err_p * t + U32 * np.abs(q) + np.abs(dq) * t * eps_t
    y = np.minimum(x * x * -C2, 1e6)
    eps_e = ULP_EXP * 2 * U32 + 2 * U32 * math.log(2.0) * y
    fit = np.abs(h - 0.5 * erfc(ax / math.sqrt(2.0))) + 1e-16
    err_h = 0.5 * e * err_q + h * (eps_e + 2 * U32) + fit + 2.0 ** -125
    cdf = np.where(x >= 0, 1.0 - h, h)
    err_cdf = err_h + np.where(x >= 0, U32 * cdf, 0.0)
    err_g = 1.01 * (ax * err_cdf + U32 * np.abs(gelu))
    err_d = 1.01 * (ax * pdf * (eps_e + 2 * U32) + err_cdf + U32 * np.abs(grad))

    def flush(v):                                   # below the normal range the result may be flushed or kept
        return np.where(np.abs(v) < BF16_MIN, 0.0, v)
    g_lo, g_hi = bf16_round(flush(gelu - err_g)), bf16_round(flush(gelu + err_g))
    d_lo, d_hi = f32_down(grad - err_d), f32_up(grad + err_d)
    o = bf16_ord(x) + 0x7F7F
    tab = SimpleNamespace(x=np.zeros(2 * 0x7F7F + 1))
    for name, v in (("x", x), ("g_lo", g_lo), ("g_hi", g_hi), ("d_lo", d_lo), ("d_hi", d_hi), ("gelu", gelu),
                    ("grad", grad), ("err_g", err_g), ("err_d", err_d)):
        a = np.zeros(2 * 0x7F7F + 1)
        a[o] = v                                    # +0 and -0 share ord 0 and carry the same (zero) entries
        setattr(tab, name, a)
    return tab


def gelu_emul(x, drcp=0, dexp=0):
    """float32 emulation of gelu_cdf_exp / gelu_f / gelu_grad_f (csrc/common.h) for bf16 values x (float64 array): every
    operation rounded to fp32 where the kernel rounds, an fma as the float64 result rounded once more (the product of
    two fp32 values is exact in float64), the reciprocal and the exponential correctly rounded and then moved by drcp /
    dexp ulp.  Returns (gelu_f, gelu_grad_f) as float64."""
    f = np.float32
    x32 = _f32(x)
    x64 = x32.astype(np.float64)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(f)

    def bump(v, d):
        for _ in range(abs(d)):
            v = np.nextafter(v, f(np.inf) if d > 0 else f(-np.inf))
        return v
    t = bump((1.0 / fma(np.abs(x32), np.full_like(x32, f(C1)), 1.0).astype(np.float64)).astype(f), drcp)
    with np.errstate(over="ignore", under="ignore"):
        arg = ((x32 * x32) * f(C2)).astype(f)
        e = np.exp2(arg.astype(np.float64)).astype(f)
    e = np.where(np.abs(e) < f(BF16_MIN), f(0), bump(e, dexp)).astype(f)
    p = np.full_like(x32, f(POLY[0]))
    for c in POLY[1:]:
        p = fma(p, t, c)
    with np.errstate(under="ignore"):
        h = ((f(0.5) * (p * t).astype(f)).astype(f) * e).astype(f)
    cdf = np.where(x32 >= 0, (f(1.0) - h).astype(f), h).astype(f)
    gelu = (x32 * cdf).astype(f)
    grad = (x64 * (f(C3) * e).astype(f).astype(np.float64) + cdf.astype(np.float64)).astype(f)
    return gelu.astype(np.float64), grad.astype(np.float64)


def _g_interval(a_lo, a_hi):
    """[min, max] of the table's G over every bf16 value in [a_lo, a_hi]."""
    tab = gelu_table()
    o_lo, o_hi = bf16_ord(a_lo) + 0x7F7F, bf16_ord(a_hi) + 0x7F7F
    lo, hi = tab.g_lo[o_lo].copy(), tab.g_hi[o_lo].copy()
    w = o_hi - o_lo
    for k in range(1, int(min(w.max(initial=0), 16)) + 1):
        idx = np.minimum(o_lo + k, o_hi)
        lo, hi = np.minimum(lo, tab.g_lo[idx]), np.maximum(hi, tab.g_hi[idx])
    for i in zip(*np.nonzero(w > 16)):              # an interval across zero: every small bf16 value lies in it
        lo[i], hi[i] = tab.g_lo[o_lo[i]:o_hi[i] + 1].min(), tab.g_hi[o_lo[i]:o_hi[i] + 1].max()
    return lo, hi


# ----------------------------------------------------------------------------- cases
def rope_table(theta, max_pos=MAX_POS):
    """[max_pos, 32, 2] fp32 (cos, sin), as snx.ops.rope_table computes it (head_dim 64)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, 64, 2, dtype=torch.float) / 64))
    freqs = torch.arange(max_pos, dtype=torch.float)[:, None] * inv_freq[None, :]
    return torch.stack((freqs.cos(), freqs.sin()), dim=-1).contiguous()


def legal_entries(N, form="128"):
    """entries whose shape conditions N meets (launch_nt of gemm.hip; the 256x256 form takes N % 64 == 0 only)."""
    if form != "128" and N % 64:
        return ()
    out = ["store", "resid"]
    if N % 64 == 0:
        out += ["rope", "rope_rows", "geglu_fwd"]
    if N % 32 == 0:
        out.append("geglu_bwd")
    return tuple(e for e in ENTRIES if e in out)


def _exact_matrix(g, rows, K):
    """multiples of 1/8, |.| <= 1/2; row r draws from -4..4, 0..4 or 2..4 eighths by r % 3"""
    lo = torch.tensor([-4, 0, 2])[torch.arange(rows) % 3][:, None]
    v = torch.randint(0, 9, (rows, K), generator=g)
    return (lo + v % (5 - lo)).to(torch.float32) / 8.0


@functools.lru_cache(maxsize=4)
def build_case(family, M, N, K, theta=10000.0):
    """inputs of one (family, shape): A [M,K], B [N,K] bf16, Hin [M,N] fp32, U [M,2N] bf16 (the saved u of the GeGLU
    backward), pos [M] int32 (shuffled, repeats, contains MAX_POS - 1 and, from two rows on, 0), tab; and the interval of c."""
    assert family in ("exact", "random") and K % 64 == 0 and N % 4 == 0
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + (7 if family == "exact" else 0))
    if family == "exact":
        A, B = _exact_matrix(g, M, K), _exact_matrix(g, N, K)
        Hin = (2.0 * torch.randn(M, N, generator=g)).to(BF16).float()
        U = (1.5 * torch.randn(M, 2 * N, generator=g)).to(BF16)
        ai, bi = (A * 8).contiguous(), (B * 8).contiguous()
        assert 16 * K < 2 ** 24                                 # integer sums below 2^24: exact in float32, any order
        S = (ai @ bi.t()).double().numpy() / 64.0
        delta = np.zeros_like(S)
    else:
        assert K <= 1152, "random family: 8 K^2 2^-24 <= 1"
        A, B = torch.randn(M, K, generator=g), 0.05 * torch.randn(N, K, generator=g)
        Hin = torch.randn(M, N, generator=g)
        U = torch.randn(M, 2 * N, generator=g).to(BF16)
        a64, b64 = A.to(BF16).double(), B.to(BF16).double()
        S = (a64 @ b64.t()).numpy()
        mag = (a64.abs() @ b64.abs().t()).numpy()
        n = K + 8
        delta = (n * U32 / (1 - n * U32) + K * 2.0 ** -52) * mag
    A, B = A.to(BF16), B.to(BF16)
    pos = torch.randint(0, MAX_POS, (M,), generator=g, dtype=torch.int32)
    pos[0] = MAX_POS - 1
    if M >= 2:
        pos[M // 2] = 0
    if M >= 4:
        pos[M - 1] = pos[1]                                       # a repeat for certain
    c = SimpleNamespace(family=family, M=M, N=N, K=K, A=A, B=B, Hin=Hin, U=U, pos=pos, theta=theta, tab=rope_table(theta),
                        S=S, delta=delta, c_lo=bf16_round(S - delta), c_hi=bf16_round(S + delta))
    return c


# ----------------------------------------------------------------------------- epilogues on intervals
def case_of(A, B, Hin=None, U=None, pos=None, theta=10000.0):
    """the interval of c for given bf16 operands (the chain test: a stage's inputs are the previous kernel's outputs);
    delta as in the random family"""
    M, K = A.shape
    N = B.shape[0]
    assert A.dtype == BF16 and B.dtype == BF16 and K <= 1152
    a64, b64 = A.double(), B.double()
    S = (a64 @ b64.t()).numpy()
    n = K + 8
    delta = (n * U32 / (1 - n * U32) + K * 2.0 ** -52) * (a64.abs() @ b64.abs().t()).numpy()
    return SimpleNamespace(family="random", M=M, N=N, K=K, A=A, B=B, Hin=Hin, U=U, pos=pos, theta=theta, tab=rope_table(theta),
                           S=S, delta=delta, c_lo=bf16_round(S - delta), c_hi=bf16_round(S + delta))


def _corners(f, *ivs):
    """min and max of f over the corners of the intervals ivs = ((lo, hi), ...)"""
    lo = hi = None
    if all(iv[0] is iv[1] or np.array_equal(iv[0], iv[1]) for iv in ivs):      # every interval one value: one corner
        v = f(*[iv[0] for iv in ivs])
        return v, v
    for m in range(1 << len(ivs)):
        v = f(*[iv[(m >> i) & 1] for i, iv in enumerate(ivs)])
        lo, hi = (v, v) if lo is None else (np.minimum(lo, v), np.maximum(hi, v))
    return lo, hi


def ep_resid(c_lo, c_hi, Hin):
    """the fp32 interval, and the SET inside it: a result is admissible iff it is fl32(Hin + v) for a bf16 v in c's interval
    (a two-value set of c leaves two fp32 values, not the thousands between them)"""
    h = _f32(Hin)

    def member(got):
        v = bf16_round(got - h.astype(np.float64), check=False)       # the only bf16 value that can have produced `got`
        return (v >= c_lo) & (v <= c_hi) & ((h + _f32(v)).astype(np.float64) == got)
    return (h + _f32(c_lo)).astype(np.float64), (h + _f32(c_hi)).astype(np.float64), dict(member=member, nvals=widths(c_lo, c_hi))


def ep_rope(c_lo, c_hi, tab, pos, rope_cols):
    M, N = c_lo.shape
    lo, hi = c_lo.copy(), c_hi.copy()
    if rope_cols == 0:
        return lo, hi
    cs = tab.numpy()[pos.numpy().astype(np.int64)]               # [M, 32, 2] fp32
    cos, sin = cs[:, None, :, 0], cs[:, None, :, 1]
    vl, vh = (v[:, :rope_cols].reshape(M, rope_cols // 64, 2, 32) for v in (c_lo, c_hi))
    x1, x2 = (vl[:, :, 0], vh[:, :, 0]), (vl[:, :, 1], vh[:, :, 1])
    r_lo = _corners(lambda a, b: bf16_round(((_f32(a) * cos) - (_f32(b) * sin)).astype(np.float64)), x1, x2)
    r_hi = _corners(lambda a, b: bf16_round(((_f32(b) * cos) + (_f32(a) * sin)).astype(np.float64)), x1, x2)
    for out, k in ((lo, 0), (hi, 1)):
        out[:, :rope_cols] = np.stack((r_lo[k], r_hi[k]), axis=2).reshape(M, rope_cols)
    return lo, hi


def ep_geglu_fwd(c_lo, c_hi):
    """-> (u interval, y interval); y [M, N / 2], column 32 q + d from a = u[64 q + d], g = u[64 q + 32 + d]"""
    M, N = c_lo.shape
    vl, vh = c_lo.reshape(M, N // 64, 2, 32), c_hi.reshape(M, N // 64, 2, 32)
    G = _g_interval(vl[:, :, 0], vh[:, :, 0])
    y = _corners(lambda a, b: bf16_round(a * b), G, (vl[:, :, 1], vh[:, :, 1]))
    return (c_lo, c_hi), (y[0].reshape(M, N // 2), y[1].reshape(M, N // 2))


def ep_geglu_bwd(c_lo, c_hi, U):
    """dy = c [M, N], saved u [M, 2N] -> du interval [M, 2N]"""
    M, N = c_lo.shape
    tab = gelu_table()
    u = to_np(U).reshape(M, N // 32, 2, 32)
    a, g = u[:, :, 0], u[:, :, 1]
    o = bf16_ord(a) + 0x7F7F
    dy = (c_lo.reshape(M, N // 32, 32), c_hi.reshape(M, N // 32, 32))
    dg = _corners(lambda d, G: bf16_round(d * G), dy, (tab.g_lo[o], tab.g_hi[o]))
    t = _corners(lambda d: bf16_round(d * g), dy)
    da = _corners(lambda tt, D: bf16_round((tt * D).astype(np.float32).astype(np.float64)), t, (tab.d_lo[o], tab.d_hi[o]))
    return tuple(np.stack((da[k], dg[k]), axis=2).reshape(M, 2 * N) for k in (0, 1))


def expected(c, entry, rope_cols=None):
    """{output name: (lo, hi)} of one entry point at case c"""
    if entry == "store":
        return {"C": (c.c_lo, c.c_hi)}
    if entry == "resid":
        return {"Hout": ep_resid(c.c_lo, c.c_hi, c.Hin.numpy())}
    if entry in ("rope", "rope_rows"):
        return {"C": ep_rope(c.c_lo, c.c_hi, c.tab, c.pos, rope_cols)}
    if entry == "geglu_fwd":
        u, y = ep_geglu_fwd(c.c_lo, c.c_hi)
        return {"U": u, "Y": y}
    assert entry == "geglu_bwd"
    return {"dU": ep_geglu_bwd(c.c_lo, c.c_hi, c.U)}


def subcase(c, rows):
    """the case restricted to some rows (every row's results depend on that row of A, Hin, U and pos alone)"""
    r = torch.as_tensor(rows)
    d = dict(vars(c))
    d.update(M=len(rows), A=c.A[r], Hin=c.Hin[r], U=c.U[r], pos=c.pos[r], **{k: getattr(c, k)[np.asarray(rows)] for k in
                                                                          ("S", "delta", "c_lo", "c_hi")})
    return SimpleNamespace(**d)


def rope_cols_of(N):
    return sorted({0, 64, N - 64, N})


# ----------------------------------------------------------------------------- guarded buffers and the check
def guarded(rows, cols, dtype, device="cpu"):
    """(buffer [GUARD_ROWS + rows + GUARD_ROWS, cols] filled with the sentinel, view of the middle rows)"""
    if dtype == BF16:
        buf = torch.full((rows + 2 * GUARD_ROWS, cols), SENT_BF16, dtype=torch.int16, device=device).view(BF16)
    else:
        buf = torch.full((rows + 2 * GUARD_ROWS, cols), SENT_F32, dtype=torch.int32, device=device).view(torch.float32)
    return buf, buf[GUARD_ROWS:GUARD_ROWS + rows]


def _raw(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def check_guards(buf, rows, what):
    """the guard rows before and behind the `rows` middle rows of a guarded buffer are untouched (a scratch buffer, whose
    contents nobody checks, is held to this alone); returns the sentinel"""
    raw = _raw(buf)
    sent = SENT_BF16 if buf.dtype == BF16 else SENT_F32
    for name, part in (("before", raw[:GUARD_ROWS]), ("behind", raw[GUARD_ROWS + rows:])):
        bad = (part != sent).nonzero()
        assert bad.numel() == 0, f"{what}: guard rows {name} the output written at (row, col) {bad[0].tolist()} ({len(bad)} elements)"
    return sent


def check_guarded(buf, iv, what):
    """buf: a guarded buffer (on the CPU) after the run; iv = (lo, hi) of its middle rows.  Guards untouched, every element
    written and finite and inside its interval.  Returns the shares the docstrings record."""
    lo, hi, *extra = iv
    extra = extra[0] if extra else {}
    rows = lo.shape[0]
    sent = check_guards(buf, rows, what)
    mid = buf[GUARD_ROWS:GUARD_ROWS + rows]
    unwritten = (_raw(mid) == sent).nonzero()
    assert unwritten.numel() == 0, f"{what}: {len(unwritten)} elements never written, first {unwritten[0].tolist()}"
    got = to_np(mid)
    assert bool(np.isfinite(got).all()), f"{what}: non-finite result"
    ok = (got >= lo) & (got <= hi)
    if "member" in extra:
        ok &= extra["member"](got)
    bad = np.argwhere(~ok)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements outside their acceptance set, first at {i}: got "
                             f"{got[i]!r}, admissible [{lo[i]!r}, {hi[i]!r}]")
    single = lo == hi
    if "nvals" in extra:
        two = extra["nvals"] == 2
    elif buf.dtype == BF16:
        two = (bf16_ord(hi) - bf16_ord(lo)) == 1
    else:
        two = ~single & (np.nextafter(lo.astype(np.float32), np.float32(np.inf)).astype(np.float64) >= hi)
    at_lo = two & (got == lo)
    return SimpleNamespace(n=got.size, single=float(single.mean()), two=float(two.mean()),
                           two_lo=float(at_lo.sum() / max(1, two.sum())), wide=float((~single & ~two).mean()))


def widths(lo, hi):
    """number of admissible bf16 values per element"""
    return bf16_ord(hi) - bf16_ord(lo) + 1


# ----------------------------------------------------------------------------- launch arithmetic, restated
def cdiv(a, b):
    return -(-a // b)


def column_group(M, N, K, bn, cap):
    """the column-group width of the tile order (launch_nt / launch): among splitting the tn column tiles into 1..4 groups,
    the cheapest by `activation bytes x groups + 8 x weight bytes x (1 if a group's weights fit cap else 4)`, first wins"""
    tn = cdiv(N, bn)
    best, cg = None, tn
    for parts in (1, 2, 3, 4):
        c = cdiv(tn, parts)
        cost = 2.0 * M * K * cdiv(tn, c) + 8.0 * 2.0 * N * K * (1.0 if 2.0 * c * bn * K <= cap else 4.0)
        if best is None or cost < best:
            best, cg = cost, c
    return cg


def tile_of(order, pos):
    """gemm_core.h: position of the tile sequence -> (row panel, column tile); super-blocks of sb_rows row panels, inside
    them column groups of cg tiles, inside a group row panel by row panel"""
    tm, tn, sb_rows, cg = order
    per_sb = sb_rows * tn
    sb = pos // per_sb
    rows = min(sb_rows, tm - sb * sb_rows)
    p = pos - sb * per_sb
    g = p // (rows * cg)
    cols = min(cg, tn - g * cg)
    p -= g * rows * cg
    r = p // cols
    return sb * sb_rows + r, g * cg + (p - r * cols)


def nt256_plan(M, N, K, reserved_cus=0):
    """What gemm_nt256.hip's launch() and next_tile make of a shape.  256 x 256 tiles, tm x tn of them, ordered by tile_of
    with the column group of column_group(cap 2.2 MB).  256 - reserved (rounded up to 8) workgroups, `per` of them on
    each of the 8 XCDs; XCD x owns positions [ntiles x / 8, ntiles (x + 1) / 8) of the sequence: nround whole rounds of
    `per` tiles (workgroup j takes position j of every round, 4 units high) and nleft < per tiles left over, cut into
    4 nleft units of 64 rows of which workgroup j takes units [4 nleft j / per, 4 nleft (j + 1) / per).  Column-run dealing
    (one column group and, for every XCD, all leftover tiles in one super-block): the units are listed column by column
    and a workgroup's piece is cut at column ends and at 4 units; tile-order dealing: listed tile by tile and cut at tile
    ends.  Returns the per-workgroup tile lists [(first row, first column, units)] and the classes a case table asks for."""
    res = cdiv(reserved_cus, 8) * 8
    tm, tn = cdiv(M, 256), cdiv(N, 256)
    cg = column_group(M, N, K, 256, 2.2e6)
    order = (tm, tn, cdiv(tm, 8), cg)
    nwg = 256 - res
    per = nwg >> 3
    ntiles, per_sb = tm * tn, order[2] * tn
    xcds, coldeal = [], cg == tn and per > 0
    for x in range(8):
        P0, P1 = ntiles * x // 8, ntiles * (x + 1) // 8
        nround = (P1 - P0) // per
        Pl = P0 + nround * per
        xcds.append((P0, P1, nround, P1 - Pl))
        if P1 > Pl and Pl // per_sb != (P1 - 1) // per_sb:
            coldeal = False
    tiles = {}
    for x, (P0, P1, nround, nleft) in enumerate(xcds):
        Pl = P0 + nround * per
        for j in range(per):
            mine = []
            for k in range(nround):
                pm, pn = tile_of(order, P0 + k * per + j)
                mine.append((pm * 256, pn * 256, 4))
            y, ye = 4 * nleft * j // per, 4 * nleft * (j + 1) // per
            while y < ye:
                if coldeal:
                    sb = Pl // per_sb
                    pa = Pl - sb * per_sb
                    pb, cum = pa + nleft, 0
                    for col in range(tn):
                        first = (pa - col + tn - 1) // tn if pa > col else 0
                        last = (pb - 1 - col) // tn if pb - 1 >= col else -1
                        cnt = max(0, last - first + 1)
                        if y < cum + 4 * cnt:
                            o = y - cum
                            uu = min(ye - y, 4, 4 * cnt - o)
                            mine.append(((sb * order[2] + first) * 256 + 64 * o, col * 256, uu))
                            break
                        cum += 4 * cnt
                    else:
                        raise AssertionError("unit outside every column run")
                else:
                    xg = 4 * Pl + y
                    uu = min(4 - (xg & 3), ye - y)
                    pm, pn = tile_of(order, xg >> 2)
                    mine.append((pm * 256 + (xg & 3) * 64, pn * 256, uu))
                y += uu
            tiles[8 * j + x] = mine                                   # blockIdx = 8 j + x
    flat = [t for v in tiles.values() for t in v]
    any_left = any(x[3] for x in xcds)
    classes = set()
    if ntiles == 1 and M % 256:
        classes.add("single ragged tile")
    if ntiles < nwg and not coldeal:
        classes.add("fewer tiles than workgroups, tile order")
    if any_left:
        classes.add("column runs" if coldeal else "tile order")
    if all(x[2] == 1 and x[3] == 0 for x in xcds):
        classes.add("one round, nothing left")
    if any(x[2] >= 1 and x[3] > 0 for x in xcds):
        classes.add("rounds plus leftovers")
    if max(x[2] for x in xcds) >= 2:
        classes.add("two rounds")
    if any(len(v) > 1 for v in tiles.values()):
        classes.add("tile after tile")
    classes.add(f"nk {min(K // 64, 3)}")
    if N % 256:
        classes.add(f"N % 256 = {N % 256}")
    for u in {t[2] for t in flat}:
        classes.add(f"u {u}")
    return SimpleNamespace(tm=tm, tn=tn, cg=cg, nwg=nwg, per=per, xcds=xcds, coldeal=coldeal, tiles=tiles, classes=classes)


def pipe_plan(M, N, K, reserved_cus=0):
    """gemm_nt_pipe.hip: None where the shape is not taken (M, N % 128, K != 768).  Two workgroups per unreserved CU, no
    more than tiles rounded up to 8, at least 8; workgroup j of XCD x takes positions P0 + j, P0 + j + per, ... below P1 of
    the XCD's run.  n tiles = one FIRST period, n - 1 MIDDLE periods, one DRAIN period; none = the workgroup returns."""
    if M % 128 or N % 128 or K != 768:
        return None
    res = cdiv(reserved_cus, 8) * 8
    ntiles = (M // 128) * (N // 128)
    nwg = 2 * (256 - res)
    if nwg > ntiles:
        nwg = (ntiles + 7) & ~7
    nwg = max(nwg, 8)
    per = nwg >> 3
    counts = []
    for x in range(8):
        P0, P1 = ntiles * x // 8, ntiles * (x + 1) // 8
        counts += [len(range(P0 + j, P1, per)) for j in range(per)]
    return SimpleNamespace(nwg=nwg, ntiles=ntiles, counts=sorted(counts), empty=counts.count(0), most=max(counts),
                           cg=column_group(M, N, K, 128, 1.8e6))


# ----------------------------------------------------------------------------- case tables
# 128x128 kernel (nt256 off, nt_pipe 0): (M, N, K, families).  M: wave-tile and workgroup-tile seams, clamped rows; N: narrow
# path (4, 12, 68, 132), wide with a partial 64-column span (8, 72, 200), GeGLU-backward-only widths (32, 96, 160), whole
# spans; K: nk = 1, 2 (mainloop's short forms), 3, 4, 5 (the mainloop_mid switch), 6, 12, and the long sums 1152 / 2304.
B_ = ("exact", "random")
CASES_128 = (
    (1, 4, 64, B_), (65, 12, 128, B_), (129, 68, 320, B_), (200, 132, 192, B_), (200, 4, 384, B_),
    (200, 8, 256, B_), (65, 72, 384, B_), (129, 200, 320, B_), (1, 72, 64, B_),
    (129, 32, 64, B_), (200, 96, 320, B_), (65, 160, 256, B_), (1, 32, 128, B_), (65, 96, 192, B_), (129, 160, 384, B_),
    (1, 64, 128, B_), (65, 192, 64, B_), (200, 192, 320, B_), (129, 384, 256, B_), (65, 64, 192, B_), (200, 384, 384, B_),
    (129, 192, 768, B_), (200, 64, 64, B_), (65, 384, 128, B_),
    (200, 2304, 768, B_), (129, 64, 1152, ("random",)), (65, 64, 2304, ("exact",)),
)
# 256x256 kernel (snx_nt256_configure(2, 1)): (M, N, K, reserved CUs, classes nt256_plan must report)
CASES_256 = (
    (200, 192, 128, 0, ("single ragged tile", "u 1", "N % 256 = 192", "nk 2")),
    (4100, 320, 256, 0, ("fewer tiles than workgroups, tile order", "tile order", "N % 256 = 64", "nk 3")),
    (2100, 1280, 64, 0, ("fewer tiles than workgroups, tile order", "tile order", "nk 1")),
    (6000, 768, 64, 0, ("column runs", "u 1", "u 2", "nk 1")),
    (4096, 2048, 128, 0, ("column runs", "u 2", "nk 2")),
    (4096, 2048, 128, 128, ("one round, nothing left", "u 4", "nk 2")),
    (4160, 2048, 128, 128, ("rounds plus leftovers", "tile after tile", "nk 2")),
    (5000, 2048, 128, 128, ("rounds plus leftovers", "tile after tile", "nk 2")),
    (5900, 768, 128, 128, ("column runs", "u 1", "u 2", "u 3", "nk 2")),
    (4900, 1280, 128, 128, ("tile order", "u 1", "u 2", "u 3", "u 4", "nk 2")),
    (8192, 2048, 64, 128, ("two rounds", "tile after tile", "nk 1")),
    (1000, 384, 64, 0, ("N % 256 = 128", "nk 1")),
)
# pipelined GeGLU backward (nt_pipe 2 and 1, nt_pipe_min_m 1, K = 768): (M, N, reserved CUs, workgroups, empty, most tiles)
CASES_PIPE = (
    (128, 128, 0, 8, 7, 1), (384, 384, 0, 16, 7, 1), (4224, 384, 0, 104, 5, 1),
    (2048, 2048, 128, 256, 0, 1), (4096, 2048, 128, 256, 0, 2), (5120, 2048, 128, 256, 0, 3),
)

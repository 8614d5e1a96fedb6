"""Float64 restatement of the kernels of the fp32 path (csrc/f32_path.hip), their case tables, and per-element acceptance
SETS derived from the kernels' arithmetic.  Plain numpy / torch on the CPU; sibling of tests/rows_reference.py (whose
LayerNorm statistics and any-order bounds it calls), tests/attention_reference.py (mask recipes and visibility rule),
tests/splade_fwd_reference.py / splade_bwd_reference.py (the routing rule) and tests/loss_reference.py (ULP_EXPF, ULP_LOGF).
Conventions.  fl32 = one fp32 operation, u = 2^-24, gamma_n = n u / (1 - n u): a sum of n operands in ANY order, fused or
not, errs by at most gamma_(n-1) sum|operand| (Higham 3.1 / 4.2, as in rows_reference).  Every cast point is fp32: the
bf16 terms of the sibling references do not occur.  An output passes iff it is finite and v - B <= got <= v + B for the
float64 value v and the bound B below; B = 0 pins the element to v (zeros of either sign compare equal).  Every B is
multiplied by 1 + 2^-20 for the float64 evaluation of v and B themselves.  The only number that is not derived is
SLACK = 1.01 of attention_reference, for products of two error terms.

ASSUMPTIONS (libm).  expf, logf, erff and log1pf are library calls.  Neither the guides nor the headers and documents of
the ROCm installation state their accuracy: ULP_EXPF = ULP_LOGF = 2 (loss_reference) and, of the same kind,
ULP_ERFF = ULP_LOG1PF = 2 are ASSUMED.  lib(ulp) = (1 + 2 ulp) u is the relative error of a call: the rounding of the
exact result (u) plus ulp ulps of at most 2u each.  Every check is also made with all four set to 0 (the call taken as
exact before its rounding); an element inside at 2 and outside at 0 is one the assumptions DECIDED, and is counted.
rsqrtf: ASSUMPTION (RSQ) of rows_reference.  A division and sqrtf are one rounding each (no fast-math flag).

GEMM (gemm_f32_kernel, gemm_f32_deepk_kernel, gemm_f32_128_kernel; EPI 0 / 1).  One value per element, no tolerance:
v_mfma_f32_32x32x2_f32 is a k-ascending fmaf chain, acc_0 = +0, acc_(k+1) = fl32(acc_k + a_k b_k) with ONE rounding;
EPI 0: C = fl32(R + acc) (acc when R is NULL); EPI 1: C = fl32(C0 + acc).  chain() emulates it: the product of two fp32
values is exact in float64, the float64 sum carries its exact TwoSum residual, and round_f32 consults the residual where
the float64 sum lies exactly half way between two fp32 neighbours (no double rounding; proven against Fraction arithmetic
in tests/test_f32_reference_host.py).  Operands: random signs, magnitudes log-uniform over [2^-10, 2^4).  The 128-tile
form needs M N >= 4,194,304: gemm_subset checks all elements of the edge tiles and a stride sample of >= 200,000 on the
CPU; the GPU file compares the rest as bits with the 64-tile form.

Decoder tail forward (EPI 2 of the three kernels, tail_finalize_kernel).  logit = fl32(chain + bias): ONE value
(tail_logits).  "exact" family: Hd, E in eighths below 2, bias in eighths, so every product is a multiple of 1/64 and
every partial sum is exact whatever the form (asserted); distinct logits differ by >= 1/64 and their log1pf sets are
disjoint (asserted in the host file), so the routing has one right answer.  value in [v - B, v + B], v = log1p(relu(logit)),
B = lib(ULP_LOG1PF) v, and never the sign bit; a masked token has weight +0.  Routing (_route_check): the stored candidate
must be the FIRST position (keys) / FIRST column (twkeys) of the maximal effective logit relu(logit) mask; a candidate
below the maximum is admitted only where its log1pf set reaches the set of the maximum (log1pf may map neighbouring
logits to one value) -- never in the exact family, counted apart in the random one.  The values are also held to
the set of 0 ulp; those inside at ULP_LOG1PF and outside at 0 are the elements ASSUMPTION (LOG1PF) decided.  The EPI-2
path never stores a logit: what the device shows of its logits are these routed maxima (which candidate won, and its
value); a logit below its maximum is held only through not having won.  sparse and token_weights
equal the high words bit for bit.

Row kernels.  LayerNorm forward and backward: rows_reference.ln_forward / ln_backward term by term (mean, centring,
squares, division, var + eps, rsqrt under RSQ, xhat, weight, g, s1, s2, dx, dw = dw0 + sum_t dy xhat with
gamma_(T+1), gradE = gE0 + sum of n rows with gamma_n; the accumulate mode is fl32(dh0 + dx) at the corners of dx).
GELU modes (src 2): the kernel normalises x^ = gelu_exact(in) with |x^_j - G_j| <= EG_j (below).  Its own rounding
error is that of rows_reference at G without the exact-sum shortcut (exact=False); the input perturbation adds, to
first order and times SLACK, D_j = r (dc_j + |xhat_j| mean(|xhat| dc)), dc_j = EG_j + mean(EG), to xhat, r^2 mean(|xhat| dc)
to rstd, and through them |w| D to the output, Dr |z| + r (D |s2| + |xhat| mean(|g| D)) to dx and |dy| D to every term
of dw (_perturbed); dst = fl32(dx gelu'(in)): |dx| Ed + Edx (|gelu'| + Ed) + u |v|.
gelu_exact(a) = fl(fl(0.5 a) fl(1 + erff(fl(a c1)))), c1 = fl32(1 / sqrt 2): the argument errs by 3u |x| (c1, the
product), erf' = 2 / sqrt(pi) exp(-x^2) <= its value at |x| (1 - 3u); Eerf = that + lib(ULP_ERFF) |erf|;
Es = Eerf + u |1 + erf|; 0.5 a is exact; EG = |h| Es + u |G|.  For a << 0 the sum 1 + erf cancels: EG is then the
absolute error of erff, which is what fp32 gives.  gelu_exact_grad(a) = fl(fl(0.5 s) + fl(fl(a c2) expf(fl(fl(-0.5 a) a)))):
the exponent errs by u |arg|, expf by lib(ULP_EXPF), c2 = fl32(1 / sqrt(2 pi)) and the two products by 3u;
Ed = 0.5 Es + Eq + u |d| (a contracted fma has one rounding fewer: covered); a flushed expf: TINY |a c2|.
GeGLU: y = fl(G g): |g| EG + u |y|; du_a = fl(fl(d g) gelu'): u |d g| (|gelu'| + Ed) + |d g| Ed + u |du_a|;
du_g = fl(d G): |d| EG + u |du_g|.
RoPE: bit for bit.  The kernel rounds the two products separately (mul_rn) and adds once: numpy float32 arithmetic
gives the same bits (one rounding per operation, proven against Fraction arithmetic in the host file); the v third keeps
its bits.

Attention (attn_f32_fwd_tiled_kernel, attn_f32_fwd_kernel, attn_f32_bwd_kernel), as attention_reference in fp32 terms.
n = keys of the sequence, NT = ceil(n / 64) + 1 key tiles (the first tile of a window need not be aligned),
scale = 1 / sqrt(hd), A_ij = sum_d |q_id| |k_jd|, B_ij = sum_d |dO_id| |v_jd|, D_i = sum_d |dO_id| |out_id|, z the score.
  score      ez_ij = gamma_(hd+4) scale A_ij: the hd-term chain in any order, scale = fl(1 / sqrtf(hd)) (2u), the product (u)
  forward    the online soft-max is the exact soft-max of the computed scores: every P_ij moves by at most
             e^(2 max_j ez) - 1.  Roundings per accumulated term, numerator and denominator alike:
             Rl_i = 4u Z_i (fl(s - m) and the sum of |m_old - m_new|, each at most 2 Z_i, Z_i = max_j |z_ij|)
                    + lib(ULP_EXPF) (1 + NT) (expf of the term and of every rescale) + 2u NT (o alpha, l alpha + psum)
                    + gamma_(n + NT) (the accumulation of l, terms of one sign).
             out: SLACK ((2 max ez + 2 Rl + gamma_(n + NT)) (P |v|) + 2u |O| + TINY sum_j |v_j|)
             lse: SLACK (max ez + Rl + lib(ULP_LOGF) (ln l + Rl + 2 max ez) + u |lse|), l = exp(lse - max z)
  backward   from out_in / lse_in as given: rho_ij = expm1(ez_ij + u |z_ij - lse_i|) + lib(ULP_EXPF) (relative error of P);
             Se_ij = |dS_ij| (rho_ij + 5u) + scale P_ij (1 + rho_ij) (gamma_hd + u) (B_ij + D_i): two products, the
             rounded scale, and the CANCELLATION term of fl(dp - delta) from two hd-term chains, which does not shrink
             with dS; accumulation over keys (dq, one wave) or queries (dk, dv: float atomics) gamma_(n+1) sum|term|:
             dq: SLACK (Se |k| + gamma_(n+1) |dS| |k|), dk: with q and the transpose, dv: SLACK (P rho + TINY)^T |dO| + ...
  exact      a query without a visible key has out = 0 and lse = 0 (the kernels define it: no element is left out);
             dk / dv of a masked key and dq of a row without a visible key have B = 0: exactly 0; everything finite.

Routed tail backward (tail_f32_bwd_kernel, tail_f32_tw_bwd_kernel).  From the keys / twkeys handed over (the device's
own, read back, or tail_ref_keys): per routed (b, v) with y > 0 and g != 0, c = fl(g expf(-y)), Ec = |c| ((1 + lib) (1 + u) - 1);
dHd, gradE, gradb are sums of fl(c x) by float atomics: B = sum Ec |x| + gamma_(n+1) (|initial| + sum (|c| + Ec) |x|), n the
contributions of the element; n = 0: the initial bits exactly (dHd: +0), i.e. no contribution where y <= 0 or g == 0.

Measured.  On an MI355X with the kernels of commit 86d3b44 (the change that adds this file moves launches into
entry points and touches no kernel), over all cases of tests/test_gpu_f32_per_element.py: 167 tests, 9.6 s for the file,
the slowest test 0.8 s (attention backward, head_dim 16, the full recipe table).  Nothing fell outside its set, no guard
or gap element was touched.  ASSUMPTIONS (EXPF, LOGF, ERFF) decided 0 elements (every element inside at 2 ulp was
inside at 0); for LOG1PF see the tail forward below.  The four constants stay at their assumed value 2.  Elements checked / pinned to one value / worst
err / bound:
    GEMM 64-tile / deepk / 128-tile  103,743 / 122,088 / 1,396,518 on the CPU chain, all pinned, all met bit for bit in the
                                     three layouts; deepk and 128-tile against the 64-tile form on the device: 122,088 and
                                     25,270,350 elements, the same bits
    tail forward                     537,384 routed maxima (per (sequence, v) and per token) against reference logits that
                                     are ONE value each (chain or exact): every route the first of its maximum, none
                                     admitted through overlapping log1pf sets, every value inside its log1pf set at
                                     2 ulp, 0 of them outside it at 0 ulp; the deepk and 128-tile forms give the
                                     keys of the 64-tile form bit for bit
    tail backward                    dHd 487,056 / 134,204 / 0.347    gradE 674,880 / 10,392 / 0.649    gradb 11,160 / 384 / 0.462
    LayerNorm forward src 0 / 1 / 2  341,736 each / 106,656, 82,042, 51,804 / 0.218, 0.165, 0.258
    LayerNorm backward               ow dx 341,736 / 0 / 0.302    acc (corners of fl32(dh0 + dx)) 341,736    gelu 341,736 / 0 / 0.187
                                     embed gradE 982,000 / 794,376 (pad row, idle ids, zero rows) / 0.869    dw 0.171 .. 0.237
    RoPE                             179,520, all pinned, the bits of numpy float32, forward and inverse
    GeGLU                            y 84,932 / 12 / 0.760    du 169,864 / 13,081 / 0.782
    attention forward  tiled         out 1,742,400 / 302,288 / 0.048    lse 75,900 / 13,538 / 0.137
                       wave-per-row  out 708,400 / 128,740 / 0.041      lse 64,900 / 12,176 / 0.174
    attention backward               dq 1,944,800 / 358,136 / 0.452    dk 1,944,800 / 893,656 / 0.271    dv 1,944,800 / 893,656 / 0.246
                                     (from the reference's out / lse and as the chain kernel forward -> kernel backward)
tests/test_f32_reference_host.py (46 tests, 20 s on the CPU): the chain emulation equals Fraction arithmetic on 4,036
triples (36 planted half-way cases) and a 50 x 37 chain; fp32 emulations in three orders reach at most 0.78 (GeGLU), 0.87
(gradE), 0.56 (tail backward), 0.45 (attention) of B; all 44 planted faults (GEMM 9, tail forward 7, tail backward 2, LayerNorm 7, RoPE 4, GeGLU 3, attention 12) are
rejected by a case of the tables.
"""
import functools
import math
from types import SimpleNamespace  # noqa: F401  (re-exported)

import numpy as np
import torch

from tests import attention_reference as AR
from tests import rows_reference as R
from tests.gemm_reference import SENT_F32, U32, f32_down, f32_up, to_np  # noqa: F401
from tests.loss_reference import ULP_EXPF, ULP_LOGF
from tests.rows_reference import F64, gamma

f32 = np.float32
f64 = np.float64
ULP_ERFF = 2                 # ASSUMPTION (ERFF), see the docstring
ULP_LOG1PF = 2               # ASSUMPTION (LOG1PF)
TINY = 2.0 ** -120           # a result below this may be flushed or rounded as a subnormal (attention_reference.TINY)
SLACK = 1.01                 # products of two error terms (attention_reference)
U = U32


def cdiv(a, b):
    return -(-a // b)


def lib(ulp):
    """relative error of a libm call accurate to `ulp` ulp: the rounding of the exact result (u) plus ulp ulps of 2u"""
    return (1 + 2 * ulp) * U


def ulps(**kw):
    """the four libm assumptions as one namespace; ulps(all=0) takes every call as exact before its rounding"""
    d = dict(expf=ULP_EXPF, logf=ULP_LOGF, erff=ULP_ERFF, log1pf=ULP_LOG1PF)
    if "all" in kw:
        d = {k: kw["all"] for k in d}
    d.update({k: v for k, v in kw.items() if k != "all"})
    return SimpleNamespace(**d)


# ----------------------------------------------------------------------------- checking
class Tally:
    """per output: elements checked, pinned to one value, outside at ulp 0 (decided by a libm assumption), worst err / bound"""

    def __init__(self):
        self.rows = {}

    def add(self, name, n, pinned, worst, decided=0):
        r = self.rows.setdefault(name, [0, 0, 0.0, 0])
        r[0] += n
        r[1] += pinned
        r[2] = max(r[2], worst)
        r[3] += decided

    def merge(self, other):
        for k, (n, p, w, d) in other.rows.items():
            self.add(k, n, p, w, d)

    def __str__(self):
        return "; ".join(f"{k}: {n} elements, {p} pinned, worst err/bound {w:.3f}, decided by libm assumption {d}"
                         for k, (n, p, w, d) in sorted(self.rows.items()))


def check_interval(what, got, lo, hi, tally=None, name=None, lo0=None, hi0=None):
    """every element of got finite and inside [lo, hi] (lo == hi: that one value; zeros compare equal whatever their sign).
    lo0 / hi0: the set with every libm call taken as exact, for the count of elements the assumptions decided."""
    got = np.asarray(got, dtype=f64)
    lo, hi = np.broadcast_to(lo, got.shape), np.broadcast_to(hi, got.shape)
    ok = np.isfinite(got) & (got >= lo) & (got <= hi)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements outside their acceptance set, first at {i}: got "
                             f"{got[i]!r}, admissible [{lo[i]!r}, {hi[i]!r}]")
    if tally is not None:
        half = (hi - lo) / 2
        err = np.abs(got - (lo + hi) / 2)
        worst = float((err[half > 0] / half[half > 0]).max(initial=0.0))
        decided = 0 if lo0 is None else int((~((got >= lo0) & (got <= hi0))).sum())
        tally.add(name or what, got.size, int((half == 0).sum()), worst, decided)
    return ok


def check_bits(what, got, want, tally=None, name=None):
    """bit for bit (fp32)"""
    g = np.ascontiguousarray(got, dtype=f32).view(np.uint32)
    w = np.ascontiguousarray(want, dtype=f32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ from their one value, first at {i}: got "
                             f"{np.asarray(got, dtype=f32)[i]!r}, want {np.asarray(want, dtype=f32)[i]!r}")
    if tally is not None:
        tally.add(name or what, g.size, g.size, 0.0)


# ----------------------------------------------------------------------------- the fma chain
def round_f32(s, err):
    """float64 s with the exact residual err of the sum that produced it -> fl32(s + err), one rounding: the cast of s
    alone is wrong only where s lies exactly half way between two fp32 neighbours and err != 0"""
    s = np.ascontiguousarray(s, dtype=f64)
    assert bool(np.all((np.abs(s) >= 2.0 ** -126) | (s == 0))) and bool(np.all(np.abs(s) < 2.0 ** 127)), "fp32 range left"
    r = s.astype(f32)
    tie = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (err != 0)
    if tie.any():
        r64 = r.astype(f64)
        up = np.where(r64 < s, np.nextafter(r, f32(np.inf)), r)
        dn = np.where(r64 > s, np.nextafter(r, f32(-np.inf)), r)
        r = np.where(tie, np.where(err > 0, up, dn), r).astype(f32)
    return r


def fma32(a, b, c):
    """fl32(a b + c) for fp32 arrays: the product is exact in float64, the sum carries its TwoSum residual"""
    p = np.asarray(a, dtype=f32).astype(f64) * np.asarray(b, dtype=f32).astype(f64)
    x = np.asarray(c, dtype=f32).astype(f64)
    s = x + p
    bb = s - x
    err = (x - (s - bb)) + (p - bb)
    return round_f32(s, err)


def chain(A, B, acc0=None, order=None, fused=True):
    """acc_0 = +0 (or acc0), acc_{k+1} = fl32(acc_k + a_k b_k) for k ascending; A [..., K] and B [..., K] broadcast.
    order / fused = False are for planted faults (another k order; the product rounded before the add)."""
    A, B = np.asarray(A, dtype=f32), np.asarray(B, dtype=f32)
    K = A.shape[-1]
    shape = np.broadcast_shapes(A.shape[:-1], B.shape[:-1])
    acc = np.zeros(shape, dtype=f32) if acc0 is None else np.broadcast_to(np.asarray(acc0, dtype=f32), shape).copy()
    for k in (range(K) if order is None else order):
        if fused:
            acc = fma32(A[..., k], B[..., k], acc)
        else:
            acc = (acc + (A[..., k] * B[..., k]).astype(f32)).astype(f32)
    return acc


# ----------------------------------------------------------------------------- GEMM
def gemm_form(M, N, K, gemm64=False):
    """launch_gemm restated: which of the three kernels a problem takes"""
    if not gemm64 and M * N >= 128 * 128 * 256 and K >= 32:
        return "128"
    if not gemm64 and K >= 128 and cdiv(M, 64) * cdiv(N, 64) <= 512:
        return "deepk"
    return "64"


def vec_ok(offset, s_row, s_k):
    """launch_gemm's vec_ok for a 16-byte aligned base and an offset in floats"""
    if offset % 4:
        return 0
    if s_k == 1:
        return int(s_row % 4 == 0)
    if s_row == 1:
        return int(s_k % 4 == 0)
    return 0


LAYOUTS = ("nt", "nn", "tn")      # forward NT + residual, dX NN, dW TN accumulating
# (name, M, N, K, form, extra): extra = offsets (floats) and paddings of the leading dimensions
GEMM_CASES = (
    ("one", 1, 1, 1, "64", {}),
    ("ragged15", 65, 63, 15, "64", {}),
    ("ragged50", 130, 70, 50, "64", {}),
    ("novec", 65, 63, 15, "64", dict(a_off=1, b_off=1, a_pad=2, b_pad=3)),      # 4-byte offsets, strides % 4 != 0
    ("vec15", 65, 63, 15, "64", dict(a_pad=1, b_pad=1)),                       # 16-byte loads with a K tail of 3
    ("mixedvec", 130, 70, 50, "64", dict(b_off=1, a_pad=2, b_pad=1)),          # a_vec = 1, b_vec = 0
    ("ldc", 65, 63, 15, "64", dict(c_pad=3, r_pad=5)),
    ("deepk130", 33, 100, 130, "deepk", {}),
    ("deepk130v", 33, 100, 130, "deepk", dict(a_pad=2, b_pad=2)),
    ("deepk128", 64, 64, 128, "deepk", {}),
    ("deepk200", 100, 300, 200, "deepk", dict(c_pad=3, r_pad=5)),
    ("big33", 2049, 2050, 33, "128", {}),
    ("big70", 4100, 1030, 70, "128", dict(a_pad=2, b_pad=2, c_pad=3, r_pad=5)),
)
GEMM_SAMPLE = 200_003            # elements of a 128-form case checked on the CPU beside its edge tiles (>= 200,000)


def operand_values(rng, shape):
    """random signs, magnitudes log-uniform over [2^-10, 2^4): clear of subnormals and overflow for every K here"""
    return (np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-10, 4, shape)) * rng.choice([-1.0, 1.0], shape)).astype(f32)


@functools.lru_cache(maxsize=4)
def gemm_case(name, layout):
    """logical A [M, K], B [N, K], R / C0 [M, N] and the storage of each: (offset, row stride, k stride), ldc, ldr"""
    spec = {c[0]: c for c in GEMM_CASES}[name]
    _, M, N, K, form, ex = spec
    assert gemm_form(M, N, K) == form
    rng = np.random.default_rng(GEMM_CASES.index(spec) * 7 + LAYOUTS.index(layout))
    A, B, R0 = operand_values(rng, (M, K)), operand_values(rng, (N, K)), operand_values(rng, (M, N))
    ap, bp_ = ex.get("a_pad", 0), ex.get("b_pad", 0)
    if layout == "nt":
        a_st, b_st = (K + ap, 1), (K + bp_, 1)
    elif layout == "nn":
        a_st, b_st = (K + ap, 1), (1, N + bp_)
    else:
        a_st, b_st = (1, M + ap), (1, N + bp_)
    c = SimpleNamespace(name=name, layout=layout, M=M, N=N, K=K, form=form, A=A, B=B, R0=R0, epi=1 if layout == "tn" else 0,
                        a_off=ex.get("a_off", 0), b_off=ex.get("b_off", 0), a_st=a_st, b_st=b_st, ldc=N + ex.get("c_pad", 0),
                        ldr=N + ex.get("r_pad", 0), has_r=layout == "nt")
    c.a_vec, c.b_vec = vec_ok(c.a_off, *a_st), vec_ok(c.b_off, *b_st)
    return c


def gemm_subset(c):
    """(rows, cols) index arrays of the elements checked on the CPU: everything, or for the 128-tile form all elements of
    the edge tiles (last 128-row and 128-column band, first tile) and a fixed stride sample of GEMM_SAMPLE elements"""
    M, N = c.M, c.N
    if c.form != "128":
        r, q = np.divmod(np.arange(M * N), N)
        return r, q
    flat = np.arange(0, M * N, max(1, (M * N) // GEMM_SAMPLE))
    sel = np.zeros((M, N), dtype=bool)
    sel.reshape(-1)[flat] = True
    sel[(M - 1) // 128 * 128:, :] = True
    sel[:, (N - 1) // 128 * 128:] = True
    sel[:128, :128] = True
    r, q = np.nonzero(sel)
    assert len(flat) >= 200_000
    return r, q


def gemm_expected(c, rows, cols, fault=None):
    """the ONE value of C[rows, cols].  fault: a planted fault of tests/test_f32_reference_host.py"""
    A, B, K = c.A[rows], c.B[cols], c.K
    order, fused, acc0 = None, True, None
    if fault in ("drop_k4", "drop_k16", "drop_k64"):
        if K % int(fault[6:]) != 0:
            order = range(K - 1)
    elif fault == "reversed":
        order = range(K - 1, -1, -1)
    elif fault == "mul_add":
        fused = False
    elif fault == "r_first" and c.epi == 0 and c.has_r:
        acc0 = c.R0[rows, cols]
    acc = chain(A, B, acc0=acc0, order=order, fused=fused)
    if fault == "r_first" and c.epi == 0 and c.has_r:
        out = acc
    elif c.epi == 1:
        out = acc if fault == "overwrite" else (c.R0[rows, cols] + acc).astype(f32)
    else:
        out = ((c.R0[rows, cols] if c.has_r else f32(0)) + acc).astype(f32)
    if fault == "edge_row":
        m = rows == c.M - 1
        if c.M > 1:
            out = out.copy()
            out[m] = gemm_expected(c, np.maximum(rows[m] - 1, 0), cols[m])
    if fault == "edge_col":
        m = cols == c.N - 1
        if c.N > 1:
            out = out.copy()
            out[m] = gemm_expected(c, rows[m], np.maximum(cols[m] - 1, 0))
    return out


GEMM_FAULTS = ("drop_k4", "drop_k16", "drop_k64", "reversed", "mul_add", "r_first", "edge_row", "edge_col", "overwrite")


# ----------------------------------------------------------------------------- GELU in fp32
C1 = float(f32(0.70710678118654752))
C2 = float(f32(0.39894228040143268))


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=f64))).numpy()


def gelu_iv(a, ul):
    """gelu_exact(a) = fl(fl(0.5 a) fl(1 + erff(fl(a c1)))): (G, EG), G = a Phi(a) in float64"""
    a = np.asarray(a, dtype=f64)
    x = a / math.sqrt(2.0)
    ax = np.abs(x)
    er = _erf(x)
    # argument: c1 is 1/sqrt 2 rounded (u), the product is rounded (u): |x^ - x| <= 3u |x|; erf' = 2/sqrt(pi) exp(-x^2)
    d_arg = 2.0 / math.sqrt(math.pi) * np.exp(-(ax * (1 - 3 * U)) ** 2) * 3 * U * ax
    Eerf = d_arg + lib(ul.erff) * (np.abs(er) + d_arg)
    s0 = 1.0 + er
    Es = Eerf + U * (np.abs(s0) + Eerf)
    h = 0.5 * a                                                  # exact: a power of two
    G = h * s0
    EG = np.abs(h) * Es + U * (np.abs(G) + np.abs(h) * Es)
    return G, F64 * EG, (s0, Es)


def gelu_grad_iv(a, ul):
    """gelu_exact_grad(a) = fl(fl(0.5 s) + fl(fl(a c2) expf(fl(fl(-0.5 a) a)))), s as above (an fma has one rounding fewer)"""
    a = np.asarray(a, dtype=f64)
    _, _, (s0, Es) = gelu_iv(a, ul)
    arg = -0.5 * a * a
    ex = np.exp(arg)
    rE = np.expm1(U * np.abs(arg))
    rE = rE + lib(ul.expf) * (1 + rE)
    t0 = a / math.sqrt(2.0 * math.pi)
    q0 = t0 * ex
    rq = (1 + U) ** 3 * (1 + rE) - 1                             # c2 rounded, a c2 rounded, the product with expf rounded
    Eq = np.abs(q0) * rq + np.abs(t0) * (1 + 3 * U) * TINY
    d0 = 0.5 * s0 + q0
    Ed = 0.5 * Es + Eq + U * (np.abs(d0) + 0.5 * Es + Eq)
    return d0, F64 * Ed


GEGLU_I = (1, 96, 1152)
GEGLU_T = (1, 67)
SPECIALS = (0.0, 10.0, -10.0, 1e-6, -1e-6)


@functools.lru_cache(maxsize=8)
def geglu_case(T, I):
    g = torch.Generator().manual_seed(77 * T + I)
    u = (2.0 * torch.randn(T, 2 * I, generator=g)).numpy().astype(f32)
    flat = u.reshape(-1)
    for i, s in enumerate(SPECIALS * 2):                          # specials in the gelu half and in the gate half
        flat[(i * 7919) % flat.size] = s
    if I >= 96:
        u[0, :5] = SPECIALS
        u[T - 1, I:I + 5] = SPECIALS
    dy = torch.randn(T, I, generator=g).numpy().astype(f32)
    dy.reshape(-1)[:: 13] = 0.0
    return SimpleNamespace(T=T, I=I, u=u, dy=dy)


def geglu_expected(c, ul):
    """{name: (lo, hi)} for y [T, I] and du [T, 2 I]"""
    a, g, d = c.u[:, :c.I].astype(f64), c.u[:, c.I:].astype(f64), c.dy.astype(f64)
    G, EG, _ = gelu_iv(a, ul)
    y0 = G * g
    Ey = np.abs(g) * EG + U * (np.abs(y0) + np.abs(g) * EG)
    gp, Ed = gelu_grad_iv(a, ul)
    m = np.abs(d * g)
    da0 = d * g * gp
    Et = m * U                                                   # fl(d g)
    Ea = Et * (np.abs(gp) + Ed) + m * Ed
    Ea = Ea + U * (np.abs(da0) + Ea)
    dg0 = d * G
    Eg = np.abs(d) * EG
    Eg = Eg + U * (np.abs(dg0) + Eg)
    du, Edu = np.concatenate([da0, dg0], axis=1), F64 * np.concatenate([Ea, Eg], axis=1)
    Ey = F64 * Ey
    return {"y": (y0 - Ey, y0 + Ey), "du": (du - Edu, du + Edu)}


def geglu_emul(c, fault=None, tanh=False):
    """the kernel's arithmetic in fp32 (erf / exp from float64, rounded once) with an optional planted fault"""
    a, g, d = c.u[:, :c.I], c.u[:, c.I:], c.dy
    if fault == "swapped":
        a, g = g, a

    def gelu(x):
        if fault == "tanh":
            x64 = x.astype(f64)
            return (0.5 * x64 * (1 + np.tanh(math.sqrt(2 / math.pi) * (x64 + 0.044715 * x64 ** 3)))).astype(f32)
        e = _erf((x * f32(C1)).astype(f32).astype(f64)).astype(f32)
        return ((f32(0.5) * x).astype(f32) * (f32(1) + e).astype(f32)).astype(f32)

    def grad(x):
        e = _erf((x * f32(C1)).astype(f32).astype(f64)).astype(f32)
        ex = np.exp(((f32(-0.5) * x).astype(f32) * x).astype(f32).astype(f64)).astype(f32)
        return ((f32(0.5) * (f32(1) + e).astype(f32)).astype(f32) + ((x * f32(C2)).astype(f32) * ex).astype(f32)).astype(f32)

    y = (gelu(a) * g).astype(f32)
    da = ((d * g).astype(f32) * grad(a)).astype(f32)
    dg = d if fault == "gate_without_gelu" else (d * gelu(a)).astype(f32)
    return {"y": y, "du": np.concatenate([da, dg], axis=1)}


GEGLU_FAULTS = ("swapped", "tanh", "gate_without_gelu")


# ----------------------------------------------------------------------------- RoPE
ROPE_HD = (2, 6, 16, 64)
ROPE_HEADS = (1, 4)
ROPE_T = (1, 67)
ROPE_MAXPOS = 96


@functools.lru_cache(maxsize=8)
def rope_case(T, heads, hd):
    g = torch.Generator().manual_seed(31 * T + 7 * heads + hd)
    qkv = torch.randn(T, 3, heads, hd, generator=g).numpy().astype(f32)
    pos = torch.randint(0, ROPE_MAXPOS, (T,), generator=g).numpy().astype(np.int32)     # non-monotone
    if T > 4:
        pos[3] = pos[1]                                                               # repeated
        pos[T - 1] = ROPE_MAXPOS - 1
        pos[2] = 0
    half = hd // 2
    ang = np.arange(ROPE_MAXPOS, dtype=f64)[:, None] * (10000.0 ** (-np.arange(half, dtype=f64) / half))[None, :]
    tab = np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(f32)                   # [max_pos, half, 2]
    return SimpleNamespace(T=T, heads=heads, hd=hd, qkv=qkv, pos=pos, tab=tab)


def rope_expected(c, inverse, fault=None):
    """numpy float32 arithmetic: two rounded products, one rounded sum -- the bits of the kernel; the v third untouched"""
    half = c.hd // 2
    out = c.qkv.copy()
    pos = c.pos
    if fault == "prev_pos":
        pos = np.concatenate([pos[:1], pos[:-1]])
    cs = c.tab[pos]                                              # [T, half, 2]
    co = cs[:, None, None, :, 0]
    si = cs[:, None, None, :, 1]
    if inverse and fault != "same_sign":
        si = -si
    thirds = 3 if fault == "v_rotated" else 2
    x1, x2 = c.qkv[:, :thirds, :, :half], c.qkv[:, :thirds, :, half:]
    if fault == "fma":
        o1 = ((x1.astype(f64) * co) - (x2 * si).astype(f32).astype(f64)).astype(f32)
        o2 = ((x2.astype(f64) * co) + (x1 * si).astype(f32).astype(f64)).astype(f32)
    else:
        o1 = ((x1 * co).astype(f32) - (x2 * si).astype(f32)).astype(f32)
        o2 = ((x2 * co).astype(f32) + (x1 * si).astype(f32)).astype(f32)
    out[:, :thirds, :, :half], out[:, :thirds, :, half:] = o1, o2
    return out


ROPE_FAULTS = ("same_sign", "prev_pos", "v_rotated", "fma")


# ----------------------------------------------------------------------------- LayerNorm rows
LN_H = (8, 64, 100, 768, 1024)
LN_T = (1, 5, 6, 8, 67)
LN_EPS = (1e-5, 1e-3)
LN_FWD_MODES = (0, 1, 2)
LN_BWD_MODES = ("acc", "ow", "embed", "gelu")


@functools.lru_cache(maxsize=4)
def ln_case(T, H, eps):
    g = torch.Generator().manual_seed(1000003 * T + 1009 * H)
    x = R.mixed_rows(T, H, g)
    a = R.mixed_rows(T, H, g).clamp(min=-6.0, max=50.0)          # pre-GELU rows of the GELU modes (gelu' stays normal)
    E = R.mixed_rows(R.V, H, g)
    return SimpleNamespace(T=T, H=H, eps=eps, V=R.V, pad=R.V - 1, x=x.numpy(), a=a.numpy(), E=E.numpy(),
                           ids=R.ids_for(T, g).numpy(), w=R.weights(H, g).numpy(), dy=torch.randn(T, H, generator=g).numpy(),
                           dh0=torch.randn(T, H, generator=g).numpy(), dw0=(0.5 * torch.randn(H, generator=g)).numpy(),
                           gE0=(0.5 * torch.randn(R.V, H, generator=g)).numpy())


def _perturbed(st, e):
    """first-order bounds of what an input perturbation |dx_j| <= e_j does to xhat (D) and to rstd (Dr):
    d xhat_j = r (dc_j - xhat_j mean(xhat dc)), dc_j = dx_j - mean(dx); d rstd = -r^2 mean(xhat dc)"""
    H = e.shape[-1]
    dc = e + e.sum(-1, keepdims=True) / H
    mx = (np.abs(st.xh) * dc).sum(-1, keepdims=True) / H
    r = st.r[:, None]
    return SLACK * r * (dc + np.abs(st.xh) * mx), SLACK * r * r * mx


def ln_fwd_expected(c, src, ul):
    """(lo, hi) of out [T, H]"""
    w = c.w.astype(f64)
    if src == 2:
        G, EG, _ = gelu_iv(c.a, ul)
        v, B, st = R.ln_forward(G, w, c.eps, exact=False)
        D, _ = _perturbed(st, EG)
        B = B + F64 * np.abs(w)[None, :] * D * (1 + U)
    else:
        x = (c.E[c.ids] if src == 1 else c.x).astype(f64)
        v, B, _ = R.ln_forward(x, w, c.eps)
    return v - B, v + B


def ln_bwd_expected(c, mode, ul):
    """{name: (lo, hi)}: dst and dw; mode acc / ow (src 0), embed (src 1: dst = gradE [V, H]), gelu (src 2)"""
    w, dy = c.w.astype(f64), c.dy.astype(f64)
    T = c.T
    if mode == "gelu":
        G, EG, _ = gelu_iv(c.a, ul)
        bw = R.ln_backward(G, w, c.eps, dy, exact=False)
        st = bw.st
        D, Dr = _perturbed(st, EG)
        H = c.H
        g = dy * w[None, :]
        s2 = (g * st.xh).sum(-1, keepdims=True) / H
        z = bw.dx / st.r[:, None]
        Edx = bw.Edx + F64 * SLACK * (Dr * np.abs(z) + st.r[:, None] * (D * np.abs(s2) + np.abs(st.xh) * (np.abs(g) * D).sum(-1, keepdims=True) / H))
        gp, Ed = gelu_grad_iv(c.a, ul)
        v = bw.dx * gp
        B = Edx * (np.abs(gp) + Ed) + np.abs(bw.dx) * Ed
        B = F64 * (B + U * (np.abs(v) + B))
        Ep, Ap = bw.Ep + np.abs(dy) * D, bw.Ap + np.abs(dy) * D
        dst = (v - B, v + B)
    else:
        x = (c.E[c.ids] if mode == "embed" else c.x).astype(f64)
        bw = R.ln_backward(x, w, c.eps, dy)
        Ep, Ap = bw.Ep, bw.Ap
        lo, hi = bw.dx - bw.Edx, bw.dx + bw.Edx
        if mode == "ow":
            dst = (lo, hi)
        elif mode == "acc":
            dh0 = c.dh0.astype(f64)
            dst = ((dh0 + f32_up(lo)).astype(f32).astype(f64), (dh0 + f32_down(hi)).astype(f32).astype(f64))
        else:
            gE0 = c.gE0.astype(f64)
            glo, ghi = gE0.copy(), gE0.copy()
            for v_ in np.unique(c.ids):
                if v_ == c.pad:
                    continue
                rows = np.nonzero(c.ids == v_)[0]
                s = gE0[v_] + bw.dx[rows].sum(0)
                B = F64 * (bw.Edx[rows].sum(0) + gamma(len(rows)) * (np.abs(gE0[v_]) + (np.abs(bw.dx[rows]) + bw.Edx[rows]).sum(0)))
                glo[v_], ghi[v_] = s - B, s + B
            dst = (glo, ghi)
    dw0 = c.dw0.astype(f64)
    v = dw0 + bw.p.sum(0)
    B = F64 * (Ep.sum(0) + gamma(T + 1) * (np.abs(dw0) + Ap.sum(0)))
    return {"dst": dst, "dw": ((v - B)[None, :], (v + B)[None, :])}


def _sum32(x, order):
    """fp32 sum along the last axis: 'asc' sequential, 'pair' pairwise (a butterfly), 'perm' a fixed permutation"""
    x = np.asarray(x, dtype=f32)
    if order == "pair":
        while x.shape[-1] > 1:
            if x.shape[-1] % 2:
                x = np.concatenate([x, np.zeros(x.shape[:-1] + (1,), dtype=f32)], axis=-1)
            x = (x[..., 0::2] + x[..., 1::2]).astype(f32)
        return x[..., 0]
    idx = np.arange(x.shape[-1]) if order == "asc" else np.random.default_rng(5).permutation(x.shape[-1])
    s = np.zeros(x.shape[:-1], dtype=f32)
    for i in idx:
        s = (s + x[..., i]).astype(f32)
    return s


def _gelu32(x):
    e = _erf((x * f32(C1)).astype(f32).astype(f64)).astype(f32)
    return ((f32(0.5) * x).astype(f32) * (f32(1) + e).astype(f32)).astype(f32)


def _gelu_grad32(x):
    e = _erf((x * f32(C1)).astype(f32).astype(f64)).astype(f32)
    ex = np.exp(((f32(-0.5) * x).astype(f32) * x).astype(f32).astype(f64)).astype(f32)
    return ((f32(0.5) * (f32(1) + e).astype(f32)).astype(f32) + ((x * f32(C2)).astype(f32) * ex).astype(f32)).astype(f32)


def ln_emul(c, src, mode=None, order="asc", fault=None):
    """the kernels' arithmetic in fp32 in a chosen summation order, with an optional planted fault.  mode None: forward ->
    out; else backward -> {dst, dw}"""
    H, eps = c.H, f32(c.eps)
    x = c.E[c.ids] if src == 1 else _gelu32(c.a) if src == 2 else c.x
    x = x.astype(f32)
    keep = H - H % 64 if fault == "last_stride" and H % 64 and H > 64 else H      # columns the three row sums see
    mean = (_sum32(x[:, :keep], order) / f32(H)).astype(f32)[:, None]
    dv = (x if fault == "no_mean" else (x - mean).astype(f32))[:, :keep]
    var = (_sum32((dv * dv).astype(f32), order) / f32(H)).astype(f32)
    if fault == "eps_outside":
        rstd = (1.0 / (np.sqrt(var.astype(f64)) + float(eps))).astype(f32)[:, None]
    else:
        rstd = (1.0 / np.sqrt((var + eps).astype(f32).astype(f64))).astype(f32)[:, None]
    dc = (x - mean).astype(f32)
    xh = (dc * rstd).astype(f32)
    if mode is None:
        return (xh * c.w[None, :]).astype(f32)
    g, w = c.dy.astype(f32), c.w.astype(f32)[None, :]
    gw = (g * w).astype(f32)
    s1 = (_sum32(gw, order) / f32(H)).astype(f32)[:, None]
    s2 = (_sum32((gw * xh).astype(f32), order) / f32(H)).astype(f32)[:, None]
    dx = (rstd * ((gw - s1).astype(f32) - (xh * s2).astype(f32)).astype(f32)).astype(f32)
    p = ((gw if fault == "dw_with_w" else g) * xh).astype(f32)
    rows = np.arange(c.T) if order == "asc" else np.random.default_rng(9).permutation(c.T) if order == "perm" else np.arange(c.T)[::-1]
    dw = c.dw0.astype(f32).copy()
    for t in rows:
        dw = (dw + p[t]).astype(f32)
    if mode == "embed":
        dst = c.gE0.astype(f32).copy()
        for t in rows:
            if c.ids[t] != c.pad or fault == "pad_row":
                dst[c.ids[t]] = (dst[c.ids[t]] + dx[t]).astype(f32)
    elif mode == "gelu":
        dst = (dx * _gelu_grad32(xh if fault == "gelu_of_xhat" else c.a.astype(f32))).astype(f32)
    elif mode == "acc":
        dst = dx if fault == "acc_overwrites" else (c.dh0.astype(f32) + dx).astype(f32)
    else:
        dst = dx
    return {"dst": dst, "dw": dw[None, :]}


LN_FAULTS = ("no_mean", "eps_outside", "dw_with_w", "pad_row", "acc_overwrites", "gelu_of_xhat", "last_stride")


# ----------------------------------------------------------------------------- attention
ATTN_LENS = ((1,), (1, 2, 65, 257), (128, 129, 64, 63), (3,) * 30 + (300,))
ATTN_WINDOWS = (-1, 0, 8, 64, 1000)
ATTN_RECIPES = AR.RECIPES + ("novis",)
ATTN_HD_TILED = (8, 16, 24, 40, 64)
ATTN_HD_ROWS = (2, 6, 10, 64)
ATTN_HD_BWD = (2, 16, 64)


def attn_table(hd, salt=0):
    """(lens index, window, recipe) triples of one head_dim: every lens x window once with the recipes in rotation, and
    every recipe at every lens for windows 8 and -1 when salt == 0 (one head_dim per form carries the full recipe table)"""
    out = []
    for li in range(len(ATTN_LENS)):
        for wi, w in enumerate(ATTN_WINDOWS):
            out.append((li, w, ATTN_RECIPES[(li * len(ATTN_WINDOWS) + wi + hd) % len(ATTN_RECIPES)]))
    if salt == 0:
        for li in range(len(ATTN_LENS)):
            for rec in ATTN_RECIPES:
                for w in (8, -1):
                    if (li, w, rec) not in out:
                        out.append((li, w, rec))
    return out


@functools.lru_cache(maxsize=4)
def attn_case(li, heads, hd, window, recipe):
    lens = ATTN_LENS[li]
    gen = torch.Generator().manual_seed(1009 * li + 31 * hd + 7 * heads + (window + 2) * 131 + ATTN_RECIPES.index(recipe))
    B, T = len(lens), sum(lens)
    cu = np.zeros(B + 1, dtype=np.int32)
    cu[1:] = np.cumsum(lens)
    qkv = torch.randn(T, 3, heads, hd, generator=gen)
    qkv[:, :2] *= 1.1 * (64.0 / hd) ** 0.25                       # scores of the same spread at every head_dim
    dout = 0.5 * torch.randn(T, heads, hd, generator=gen)
    masks = []
    for b, n in enumerate(lens):
        if recipe == "novis":
            masks.append(torch.zeros(n, dtype=torch.int64) if b == (1 if B > 1 else 0) else AR.seq_mask("mix", n, b))
        else:
            masks.append(AR.seq_mask(recipe, n, b))
    mask = torch.cat(masks)
    seqid = np.repeat(np.arange(B, dtype=np.int32), lens)
    return SimpleNamespace(lens=lens, B=B, T=T, heads=heads, hd=hd, window=int(window), recipe=recipe, cu=cu, seqid=seqid,
                           mask=mask.numpy(), qkv=qkv.numpy().astype(f32), dout=dout.numpy().astype(f32))


def _attn_units(c):
    x = torch.from_numpy(c.qkv.astype(f64))
    m = torch.from_numpy(c.mask)
    for b in range(c.B):
        sl = slice(int(c.cu[b]), int(c.cu[b + 1]))
        vis = AR.visibility(c.lens[b], m[sl], c.window)
        for h in range(c.heads):
            yield sl, h, x[sl, 0, h], x[sl, 1, h], x[sl, 2, h], vis


def attn_fwd_expected(c, ul):
    """out [T, heads, hd], lse [heads, T] (float64) and their bounds; rows without a visible key: 0, bound 0.  ul: one
    ulps() namespace, or a tuple of them (-> a tuple of results from one pass)"""
    uls = ul if isinstance(ul, tuple) else (ul,)
    T, Hn, hd = c.T, c.heads, c.hd
    z64 = lambda *sh: torch.zeros(*sh, dtype=torch.float64)   # noqa: E731
    out, lse = z64(T, Hn, hd), z64(Hn, T)
    out_b, lse_b = [z64(T, Hn, hd) for _ in uls], [z64(Hn, T) for _ in uls]
    scale = 1.0 / math.sqrt(hd)
    for sl, h, q, k, v, vis in _attn_units(c):
        n = q.shape[0]
        NT = cdiv(n, 64) + 1
        anyv = vis.any(dim=1)
        z = scale * (q @ k.t())
        zm = torch.where(vis, z, torch.full_like(z, -math.inf))
        mx = torch.where(anyv, zm.max(dim=1).values, z64(n))
        l_ = torch.where(anyv, torch.logsumexp(zm, dim=1), z64(n))
        P = torch.where(vis, torch.exp(z - l_[:, None]), torch.zeros_like(z))
        O = P @ v
        A = torch.where(vis, q.abs() @ k.abs().t(), torch.zeros_like(z))
        Z = torch.where(vis, z.abs(), torch.zeros_like(z)).max(dim=1).values
        ez = gamma(hd + 4) * scale * A.max(dim=1).values
        Pv = P @ v.abs()
        out[sl, h], lse[h, sl] = O, l_
        lnl = l_ - mx
        for i, u_ in enumerate(uls):
            Rl = 4 * U * Z + lib(u_.expf) * (1 + NT) + 2 * U * NT + gamma(n + NT)
            Rtot = 2 * ez + 2 * Rl
            out_b[i][sl, h] = torch.where(anyv[:, None], SLACK * ((Rtot[:, None] + gamma(n + NT)) * Pv + 2 * U * O.abs()
                                                                  + TINY * v.abs().sum(dim=0)[None, :]), torch.zeros_like(O))
            lse_b[i][h, sl] = torch.where(anyv, SLACK * (ez + Rl + lib(u_.logf) * (lnl + Rl + 2 * ez) + U * l_.abs()), z64(n))
    res = tuple(SimpleNamespace(out=out.numpy(), out_b=F64 * out_b[i].numpy(), lse=lse.numpy(), lse_b=F64 * lse_b[i].numpy())
                for i in range(len(uls)))
    return res if isinstance(ul, tuple) else res[0]


def attn_bwd_expected(c, out_in, lse_in, ul):
    """dqkv [T, 3, heads, hd] and its bound from out_in [T, heads, hd] / lse_in [heads, T] fp32, used as the kernel uses
    them.  ul: one ulps() namespace or a tuple of them, as in attn_fwd_expected"""
    uls = ul if isinstance(ul, tuple) else (ul,)
    T, Hn, hd = c.T, c.heads, c.hd
    d = torch.zeros(T, 3, Hn, hd, dtype=torch.float64)
    db = [torch.zeros(T, 3, Hn, hd, dtype=torch.float64) for _ in uls]
    dO_all = torch.from_numpy(c.dout.astype(f64))
    o_all = torch.from_numpy(np.asarray(out_in, dtype=f64).reshape(T, Hn, hd))
    lse_all = torch.from_numpy(np.asarray(lse_in, dtype=f64))
    scale = 1.0 / math.sqrt(hd)
    for sl, h, q, k, v, vis in _attn_units(c):
        n = q.shape[0]
        dO, o, l_ = dO_all[sl, h], o_all[sl, h], lse_all[h, sl]
        zero = torch.zeros(n, n, dtype=torch.float64)
        z = scale * (q @ k.t())
        P = torch.where(vis, torch.exp(z - l_[:, None]), zero)
        delta = (dO * o).sum(dim=1)
        dS = scale * P * (dO @ v.t() - delta[:, None])
        d[sl, 0, h], d[sl, 1, h], d[sl, 2, h] = dS @ k, dS.t() @ q, P.t() @ dO
        A, Bm, D = q.abs() @ k.abs().t(), dO.abs() @ v.abs().t(), (dO.abs() * o.abs()).sum(dim=1)
        ez = gamma(hd + 4) * scale * A
        tiny = torch.where(vis, torch.full_like(z, TINY), zero)
        acc = gamma(n + 1)
        accV, accQ, accK = acc * (P.t() @ dO.abs()), acc * (dS.abs() @ k.abs()), acc * (dS.abs().t() @ q.abs())
        for i, u_ in enumerate(uls):
            rho = torch.expm1(ez + U * (z - l_[:, None]).abs()) + lib(u_.expf)
            Pe = P * rho + tiny
            Se = dS.abs() * (rho + 5 * U) + scale * (P * (1 + rho) + tiny) * (gamma(hd) + U) * (Bm + D[:, None])
            db[i][sl, 0, h] = SLACK * (Se @ k.abs() + accQ)
            db[i][sl, 1, h] = SLACK * (Se.t() @ q.abs() + accK)
            db[i][sl, 2, h] = SLACK * (Pe.t() @ dO.abs() + accV)
    res = tuple(SimpleNamespace(dqkv=d.numpy(), dqkv_b=F64 * db[i].numpy()) for i in range(len(uls)))
    return res if isinstance(ul, tuple) else res[0]


def attn_emul(c, order="asc", fault=None, out_lse=None):
    """the attention in fp32 arithmetic (float32 matmuls in a chosen key order, expf / logf from float64 rounded once),
    with an optional planted fault.  -> out, lse, dqkv (the backward from its own out / lse, or from out_lse)"""
    T, Hn, hd = c.T, c.heads, c.hd
    scale = f32(1.0) / np.sqrt(f32(hd))
    if fault == "scale_8th":
        scale = f32(0.125)
    out, lse = np.zeros((T, Hn, hd), dtype=f32), np.zeros((Hn, T), dtype=f32)
    dqkv = np.zeros((T, 3, Hn, hd), dtype=f32)
    rng = np.random.default_rng(3)
    for b in range(c.B):
        s0, n = int(c.cu[b]), c.lens[b]
        sl = slice(s0, s0 + n)
        vis = AR.visibility(n, torch.from_numpy(c.mask[sl]), c.window).numpy().copy()
        if fault == "window_strict" and c.window >= 0:
            i = np.arange(n)
            vis &= np.abs(i[:, None] - i[None, :]) < c.window
        if fault == "drop_visible":
            j = np.argmax(vis.any(axis=0)) if vis.any() else 0
            vis[:, j] = False
        if fault == "include_masked" and (c.mask[sl] == 0).any():
            j = int(np.argmax(c.mask[sl] == 0))
            vis[:, j] = True if c.window < 0 else (np.abs(np.arange(n) - j) <= c.window)
        if fault == "key65":
            vis[:, 64::64] = False
        perm = np.arange(n) if order == "asc" else rng.permutation(n) if order == "perm" else np.arange(n)[::-1]
        for h in range(Hn):
            q, k, v = c.qkv[sl, 0, h], c.qkv[sl, 1, h], c.qkv[sl, 2, h]
            s = (np.matmul(q, k.T).astype(f32) * scale).astype(f32)
            sm = np.where(vis, s, -np.inf).astype(f32)
            anyv = vis.any(axis=1)
            m = np.where(anyv, sm.max(axis=1), 0).astype(f32)
            p = np.where(vis, np.exp((s - m[:, None]).astype(f32).astype(f64)), 0).astype(f32)
            l_ = _sum32(p[:, perm], "asc" if order != "pair" else "pair")
            o = np.zeros((n, hd), dtype=f32)
            for j in perm:
                o = (o + (p[:, j:j + 1] * v[j][None, :]).astype(f32)).astype(f32)
            safe = np.where(anyv, l_, 1).astype(f32)
            o = np.where(anyv[:, None], (o / safe[:, None]).astype(f32), 0).astype(f32)
            ls = np.where(anyv, (m + np.log(safe.astype(f64)).astype(f32)).astype(f32), 0).astype(f32)
            if fault == "lse_no_max":
                ls = np.where(anyv, np.log(safe.astype(f64)).astype(f32), 0).astype(f32)
            if fault == "novis_mean_v":
                o = np.where(anyv[:, None], o, v.mean(axis=0, keepdims=True)).astype(f32)
            if fault == "query129" and n > 128:
                o[128] = o[127]
                ls[128] = ls[127]
            if fault == "skip_q0_stride" and n > 128 and len(c.lens) > 8:
                o[128:256] = 0
                ls[128:256] = 0
            out[sl, h], lse[h, sl] = o, ls
            oi, li_ = (o, ls) if out_lse is None else (np.asarray(out_lse[0], dtype=f32)[sl, h], np.asarray(out_lse[1], dtype=f32)[h, sl])
            dO = c.dout[sl, h]
            delta = np.zeros(n, dtype=f32) if fault == "no_delta" else _sum32((dO * oi).astype(f32), "asc")
            pb = np.where(vis, np.exp((s - li_[:, None]).astype(f32).astype(f64)), 0).astype(f32)
            dp = np.matmul(dO, v.T).astype(f32)
            ds = ((pb * (dp - delta[:, None]).astype(f32)).astype(f32) * scale).astype(f32)
            dq, dk, dv = np.zeros((n, hd), dtype=f32), np.zeros((n, hd), dtype=f32), np.zeros((n, hd), dtype=f32)
            for j in perm:
                dq = (dq + (ds[:, j:j + 1] * k[j][None, :]).astype(f32)).astype(f32)
            for i in perm:
                dk = (dk + (ds[i][:, None] * q[i][None, :]).astype(f32)).astype(f32)
                dv = (dv + ((ds if fault == "dv_from_ds" else pb)[i][:, None] * dO[i][None, :]).astype(f32)).astype(f32)
            if fault == "dk_no_scale":
                dk = (dk / scale).astype(f32)
            dqkv[sl, 0, h], dqkv[sl, 1, h], dqkv[sl, 2, h] = dq, dk, dv
    return out, lse, dqkv


ATTN_FAULTS = ("drop_visible", "include_masked", "window_strict", "scale_8th", "key65", "query129", "skip_q0_stride",
               "lse_no_max", "no_delta", "dk_no_scale", "dv_from_ds", "novis_mean_v")


# ----------------------------------------------------------------------------- decoder tail
TAIL_LENS = (1, 3, 60, 5, 70)
TAIL_V = (1, 63, 64, 65, 200)
TAIL_MASKS = ("ones", "holes", "seq_masked")
TAIL_FAMILIES = ("exact", "random")
# (name, lens, V, H, form of the EPI-2 GEMM)
TAIL_CASES = tuple((f"v{V}", TAIL_LENS, V, 8, "64") for V in TAIL_V) + (
    ("deepk", TAIL_LENS, 200, 130, "deepk"),
    ("big", TAIL_LENS * 15 + (15,), 2000, 32, "128"),
)


@functools.lru_cache(maxsize=3)
def tail_case(name, family, maskkind):
    _, lens, V, H, form = {c[0]: c for c in TAIL_CASES}[name]
    T, B = sum(lens), len(lens)
    assert gemm_form(T, V, H) == form
    rng = np.random.default_rng(TAIL_FAMILIES.index(family) * 100 + TAIL_MASKS.index(maskkind) * 10 + V + H)
    if family == "exact":
        # multiples of 1/8 below 2 in magnitude: every product a multiple of 1/64, every partial sum below 2^18 / 64
        Hd = (rng.integers(-12, 13, (T, H)) / 8.0).astype(f32)
        E = (rng.integers(-12, 13, (V, H)) / 8.0).astype(f32)
        bias = (rng.integers(-8, 9, V) / 8.0).astype(f32)
    else:
        Hd, E = operand_values(rng, (T, H)), operand_values(rng, (V, H))
        Hd, E = (Hd * f32(0.25)).astype(f32), (E * f32(0.25)).astype(f32)      # exact scalings: logits of a few units
        bias = operand_values(rng, (V,))
    cu = np.zeros(B + 1, dtype=np.int32)
    cu[1:] = np.cumsum(lens)
    # planted ties: duplicated Hd rows inside a sequence (the later copy must lose), duplicated E rows with equal bias
    for b in range(B):
        if lens[b] >= 5:
            Hd[cu[b] + lens[b] - 2] = Hd[cu[b] + 1]
            Hd[cu[b] + 3] = Hd[cu[b] + 1]
    if V >= 63:
        E[V - 3], bias[V - 3] = E[2], bias[2]
        E[40], bias[40] = E[2], bias[2]
    if V >= 2:
        E[V - 1] = 0                                              # a column whose logits are all < 0: its value is +0
        bias[V - 1] = -max(abs(bias[V - 1]), f32(0.125))
    mask = np.ones(T, dtype=np.int64)
    if maskkind != "ones":
        for b in range(B):
            m = AR.seq_mask("holes", lens[b], b).numpy()
            mask[cu[b]:cu[b + 1]] = m
        if lens[0] == 1 and B > 1:
            mask[cu[1] + 1] = 0
    if maskkind == "seq_masked":
        mask[cu[2]:cu[3]] = 0
    seqid = np.repeat(np.arange(B, dtype=np.int32), lens)
    pos = (np.arange(T) - cu[seqid]).astype(np.int32)
    c = SimpleNamespace(name=name, family=family, maskkind=maskkind, lens=lens, T=T, B=B, V=V, H=H, form=form, Hd=Hd, E=E,
                        bias=bias, cu=cu, seqid=seqid, pos=pos, mask=mask)
    return c


def tail_logits(c, rows=None, cols=None):
    """fp32 logits fl32(chain + bias) of the given rows x cols: ONE value each (exact family: also the exact value)"""
    rows = np.arange(c.T) if rows is None else np.asarray(rows)
    cols = np.arange(c.V) if cols is None else np.asarray(cols)
    if c.family == "exact":
        x = c.Hd[rows].astype(f64) @ c.E[cols].astype(f64).T + c.bias[cols].astype(f64)[None, :]
        assert bool(np.all(x == x.astype(f32).astype(f64))) and float(np.abs(x).max(initial=0)) * 64 < 2 ** 24
        return x.astype(f32)
    acc = chain(c.Hd[rows][:, None, :], c.E[cols][None, :, :])
    return (acc + c.bias[cols][None, :]).astype(f32)


def log1p_set(x, ulp):
    """[lo, hi] of log1pf(relu(x)) for fp32 logits x"""
    v = np.log1p(np.maximum(np.asarray(x, dtype=f64), 0.0))
    B = F64 * lib(ulp) * v
    return v - B, v + B


def split_keys(keys):
    keys = np.asarray(keys, dtype=np.uint64)
    return (keys >> np.uint64(32)).astype(np.uint32).view(f32), (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)


def tail_fwd_emul(c, x, fault=None):
    """keys [B, V], twkeys [T] from logits x [T, V] the way the kernel forms them (log1p from float64, rounded once)"""
    T, V = x.shape
    xx = x.astype(f64)
    if fault == "unclamped":
        w = np.log1p(np.maximum(xx, -0.999)).astype(f32)
    else:
        w = np.log1p(np.maximum(xx, 0.0)).astype(f32)
    if fault != "mask_not_zeroed":
        w = np.where(c.mask[:, None] != 0, w, f32(0)).astype(f32)
    wb = w.view(np.uint32).astype(np.uint64) << np.uint64(32)
    tagp = (np.arange(T) if fault == "flat_pos" else c.pos).astype(np.uint64)
    if fault == "last_pos_tie":
        kk = wb | tagp[:, None]
    else:
        kk = wb | (np.uint64(0xFFFFFFFF) - tagp)[:, None]
    keys = np.zeros((c.B, V), dtype=np.uint64)
    for b in range(c.B):
        lo, hi = int(c.cu[b]), int(c.cu[b + 1])
        if fault == "seq_leak" and b > 0 and lo % 16:
            lo = lo // 16 * 16
        keys[b] = kk[lo:hi].max(axis=0)
    if fault == "last_pos_tie":
        keys = (keys & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF)))
    tagv = np.arange(V, dtype=np.uint64)
    kv = wb | (tagv if fault == "last_col_tie" else np.uint64(0xFFFFFFFF) - tagv)[None, :]
    if fault == "lose_last_col" and V % 32:
        kv = kv[:, :V - 1]
        keys[:, V - 1] = 0
    tw = kv.max(axis=1, initial=0)
    if fault == "last_col_tie":
        tw = (tw & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - (tw & np.uint64(0xFFFFFFFF)))
    return keys, tw


TAIL_FAULTS = ("last_pos_tie", "last_col_tie", "mask_not_zeroed", "seq_leak", "flat_pos", "lose_last_col", "unclamped")


def _route_check(what, xr, val, idx, valid_n, ulp, strict):
    """one routed maximum per column of xr [n, m] (n candidates in tie order): val [m] the stored value, idx [m] the stored
    candidate.  The candidate must be the FIRST of the maximum; a candidate below the maximum is admissible only where
    the log1pf sets of the two overlap (never in the exact family: strict).  -> (routes admitted through such an
    overlap, values inside their set at `ulp` and outside it at 0 ulp: the elements ASSUMPTION (LOG1PF) decided)"""
    n, m = xr.shape
    assert bool(np.all((idx >= 0) & (idx < valid_n))), f"{what}: a routed index outside its range"
    first = xr.argmax(axis=0)                                    # numpy: the first of the maximum
    cols = np.arange(m)
    lo, hi = log1p_set(xr[idx, cols], ulp)
    bits = np.asarray(val, dtype=f32).view(np.uint32)
    inside = (val.astype(f64) >= lo) & (val.astype(f64) <= hi) & ((bits >> 31) == 0)
    bad = np.argwhere(~inside)
    assert len(bad) == 0, (f"{what}: {len(bad)} values outside the log1pf set of their logit, first at column {bad[0][0]}: "
                           f"got {val[bad[0][0]]!r}, set [{lo[bad[0][0]]!r}, {hi[bad[0][0]]!r}]")
    lo0, hi0 = log1p_set(xr[idx, cols], 0)
    decided = int((~((val.astype(f64) >= lo0) & (val.astype(f64) <= hi0))).sum())
    same = idx == first
    lo_f, _ = log1p_set(xr[first, cols], ulp)
    overlap = ~same & (xr[idx, cols] < xr[first, cols]) & (hi >= lo_f)
    wrong = ~same & ~overlap
    if strict:
        wrong = ~same
    bad = np.argwhere(wrong)
    assert len(bad) == 0, (f"{what}: {len(bad)} wrong routes, first at column {bad[0][0]}: stored candidate {idx[bad[0][0]]}, "
                           f"the first of the maximum is {first[bad[0][0]]}")
    return int(overlap.sum()), decided


def tail_fwd_check(c, keys, twkeys, sparse, tw, ulp=ULP_LOG1PF, cols=None, rows=None, x_cols=None, x_rows=None, tally=None):
    """keys [B, V] / twkeys [T] (uint64) and the decoded sparse / tw against the logits: x_cols [T, len(cols)] for the
    per-(sequence, v) maxima, x_rows [len(rows), V] for the per-token maxima"""
    cols = np.arange(c.V) if cols is None else np.asarray(cols)
    rows = np.arange(c.T) if rows is None else np.asarray(rows)
    x_cols = tail_logits(c, None, cols) if x_cols is None else x_cols
    x_rows = tail_logits(c, rows, None) if x_rows is None else x_rows
    strict = c.family == "exact"
    kval, kpos = split_keys(keys)
    check_bits(f"{c.name} sparse == high words", np.asarray(sparse).reshape(c.B, c.V), kval)
    tval, tcol = split_keys(twkeys)
    check_bits(f"{c.name} token_weights == high words", np.asarray(tw), tval)
    counts = np.zeros(2, dtype=np.int64)                         # overlap-admitted routes, values decided by LOG1PF
    live = c.mask != 0
    for b in range(c.B):
        lo, hi = int(c.cu[b]), int(c.cu[b + 1])
        xr = np.where(live[lo:hi, None], np.maximum(x_cols[lo:hi], f32(0)), f32(0)).astype(f32)
        assert bool(np.array_equal(c.pos[lo:hi], np.arange(hi - lo)))
        counts += _route_check(f"{c.name} {c.family} {c.maskkind} keys of sequence {b}", xr, kval[b, cols], kpos[b, cols], hi - lo, ulp, strict)
    xr = np.where(live[rows, None], np.maximum(x_rows, f32(0)), f32(0)).astype(f32)
    counts += _route_check(f"{c.name} {c.family} {c.maskkind} twkeys", xr.T, tval[rows], tcol[rows], c.V, ulp, strict)
    assert bool(np.all(tval[~live].view(np.uint32) == 0)), "a masked token carries weight"
    if tally is not None:
        n = c.B * len(cols) + len(rows)                          # the routed maxima: all the device shows of its logits
        tally.add("tail values of the routed maxima", n, 0, 0.0, int(counts[1]))
        tally.add("tail routes (pinned: the first of the maximum; the rest admitted through overlapping log1pf sets)", n,
                  n - int(counts[0]), 0.0)


def tail_ref_keys(c):
    """the reference's own keys / twkeys (values: log1p from float64, rounded once)"""
    return tail_fwd_emul(c, tail_logits(c))


def tail_bwd_expected(c, keys, twkeys, g, g_tw, gE0, gb0, ul):
    """dHd [T, H], gradE [V, H], gradb [V] as (lo, hi) from the given keys / twkeys (uint64) and upstream gradients"""
    T, V, H = c.T, c.V, c.H
    Hd, E = c.Hd.astype(f64), c.E.astype(f64)
    val = {k: np.zeros(s) for k, s in (("dHd", (T, H)), ("gE", (V, H)), ("gb", (V,)))}
    err = {k: np.zeros_like(v) for k, v in val.items()}
    mag = {k: np.zeros_like(v) for k, v in val.items()}
    cnt = {k: np.zeros(v.shape[:1] if k != "gb" else v.shape, dtype=np.int64) for k, v in val.items()}

    def route(y, gv, tok, v):
        sel = (y > 0) & (gv != 0)
        y, gv, tok, v = y[sel].astype(f64), gv[sel].astype(f64), tok[sel], v[sel]
        c0 = gv * np.exp(-y)
        Ec = np.abs(c0) * ((1 + lib(ul.expf)) * (1 + U) - 1)
        for name, idx, other in (("dHd", tok, E[v]), ("gE", v, Hd[tok])):
            np.add.at(val[name], idx, c0[:, None] * other)
            np.add.at(err[name], idx, Ec[:, None] * np.abs(other))
            np.add.at(mag[name], idx, (np.abs(c0) + Ec)[:, None] * np.abs(other))
            np.add.at(cnt[name], idx, 1)
        np.add.at(val["gb"], v, c0)
        np.add.at(err["gb"], v, Ec)
        np.add.at(mag["gb"], v, np.abs(c0) + Ec)
        np.add.at(cnt["gb"], v, 1)

    kval, kpos = split_keys(keys)
    bb, vv = np.divmod(np.arange(c.B * V), V)
    route(kval.reshape(-1), np.asarray(g, dtype=f32).reshape(-1), c.cu[bb] + kpos.reshape(-1), vv)
    if g_tw is not None:
        tval, tcol = split_keys(twkeys)
        route(tval, np.asarray(g_tw, dtype=f32), np.arange(T), tcol)
    out = {}
    for name, init in (("dHd", np.zeros((T, H))), ("gE", gE0.astype(f64)), ("gb", gb0.astype(f64))):
        n = cnt[name] if name == "gb" else cnt[name][:, None]
        v = init + val[name]
        B = F64 * (err[name] + gamma(n + 1) * (np.abs(init) + mag[name]))
        B = np.where(n == 0, 0.0, B)
        out[name] = (v - B, v + B)
    return out


def tail_bwd_emul(c, keys, twkeys, g, g_tw, gE0, gb0, order="asc", fault=None):
    """the routed backward in fp32, contributions added in a chosen arrival order"""
    T, V, H = c.T, c.V, c.H
    dHd, gE, gb = np.zeros((T, H), dtype=f32), gE0.astype(f32).copy(), gb0.astype(f32).copy()
    kval, kpos = split_keys(keys)
    items = [(kval[b, v], g[b, v], int(c.cu[b] + kpos[b, v]), v) for b in range(c.B) for v in range(V)]
    if g_tw is not None:
        tval, tcol = split_keys(twkeys)
        items += [(tval[t], g_tw[t], t, int(tcol[t])) for t in range(T)]
    idx = np.arange(len(items)) if order == "asc" else np.random.default_rng(11).permutation(len(items)) if order == "perm" else np.arange(len(items))[::-1]
    for i in idx:
        y, gv, tok, v = items[i]
        if (not (y > 0) or gv == 0) and fault != "no_skip":
            continue
        cc = f32(gv) * f32(np.exp(-float(y)))
        if fault == "no_exp":
            cc = f32(gv)
        dHd[tok] = (dHd[tok] + (cc * c.E[v]).astype(f32)).astype(f32)
        gE[v] = (gE[v] + (cc * c.Hd[tok]).astype(f32)).astype(f32)
        gb[v] = f32(gb[v] + cc)
    return {"dHd": dHd, "gE": gE, "gb": gb}


def tail_grads(c, seed=0):
    """upstream gradients with exact zeros, and the non-zero contents gradE / gradb are accumulated into"""
    rng = np.random.default_rng(1000 + seed + c.V)
    g = rng.standard_normal((c.B, c.V)).astype(f32)
    g[rng.random((c.B, c.V)) < 0.2] = 0
    g_tw = rng.standard_normal(c.T).astype(f32)
    g_tw[::5] = 0
    return g, g_tw, rng.standard_normal((c.V, c.H)).astype(f32), rng.standard_normal(c.V).astype(f32)


# ----------------------------------------------------------------------------- checks shared by the host and the GPU file
def check_sets(what, got, exp, tally=None, exp0=None, prefix=""):
    """got {name: array}, exp {name: (lo, hi)}; exp0: the same sets with every libm call taken as exact"""
    assert set(got) == set(exp), (what, sorted(got), sorted(exp))
    for k in sorted(got):
        lo0, hi0 = exp0[k] if exp0 is not None else (None, None)
        check_interval(f"{what} {k}", got[k], exp[k][0], exp[k][1], tally, prefix + k, lo0, hi0)


def attn_fwd_check(what, c, out, lse, tally=None, prefix="attn fwd "):
    sets = [{"out": (r.out - r.out_b, r.out + r.out_b), "lse": (r.lse - r.lse_b, r.lse + r.lse_b)}
            for r in attn_fwd_expected(c, (ulps(), ulps(all=0)))]
    got = {"out": np.asarray(out).reshape(c.T, c.heads, c.hd)}
    if lse is not None:
        got["lse"] = np.asarray(lse)
    else:
        sets = [{"out": e["out"]} for e in sets]
    check_sets(what, got, sets[0], tally, sets[1], prefix)


def attn_bwd_check(what, c, dqkv, out_in, lse_in, tally=None, prefix="attn bwd "):
    got = np.asarray(dqkv).reshape(c.T, 3, c.heads, c.hd)
    sets = [{n: (r.dqkv[:, i] - r.dqkv_b[:, i], r.dqkv[:, i] + r.dqkv_b[:, i]) for i, n in enumerate(("dq", "dk", "dv"))}
            for r in attn_bwd_expected(c, out_in, lse_in, (ulps(), ulps(all=0)))]
    check_sets(what, {n: got[:, i] for i, n in enumerate(("dq", "dk", "dv"))}, sets[0], tally, sets[1], prefix)

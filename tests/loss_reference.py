"""Float64 restatement of csrc/loss.hip (loss_partial_kernel, loss_sum_partials_kernel, loss_reduce_kernel behind
snx_loss_fwd; loss_bwd_kernel behind snx_loss_bwd), written from its cast points and not from its loops; the case table; a
restatement of pick_ch, the dynamic-LDS sizes and the workspace size; per-element acceptance SETS.  Sibling of
tests/rows_reference.py and tests/adamw_reference.py, whose roundings, guarded buffers and fp32 intervals it reuses.

Contracts (fl32 = one fp32 operation, bf16() = round to nearest even; mode bf16 = `bf16_mm`; off = label_off;
q [B, V], p [Bp, V], n [B k, V]; hp = {tau, lam_q, lam_d, lam_neg, lam_mm, lam_kd, T_kd}; inv_tau = fl32(1 / tau)):
    in-batch   D_ij = sum_c a_ic b_jc, fp32 accumulation; a = bf16(q), b = bf16(p) in bf16 mode, a = q, b = p otherwise
               s_ij = fl32(bf16(D_ij) inv_tau) in bf16 mode -- rounded BEFORE the scaling, one fp32 multiply --,
               fl32(D_ij inv_tau) otherwise
    hard, q.p  H_ik = sum_c q_ic n_(ik)c and P_i = sum_c q_ic p_(off+i)c: operands and sums never rounded to bf16;
               s_(i, Bp+kk) = fl32(H_ik inv_tau)
    soft-max   row i = [s_i0 .. s_i,Bp-1 | s_i,Bp .. s_i,Bp+k-1], label off + i; mx = max; lse = fl32(mx + logf(sum_j
               expf(fl32(s_ij - mx)))); ce_i = fl32(lse - s_i,lab); infonce = fl32(sum_i ce_i / B)
    G          G_ij = fl32(fl32(expf(fl32(s_ij - lse)) - [j = lab]) gs), gs = fl32(inv_tau / B); bf16(.) in bf16 mode
    Gh         Gh_ik = fl32(expf(fl32(s_i,Bp+kk - lse)) gs) [- dsm_ik]: the hard negatives' coefficients carry the
               MarginMSE term: df = fl32(fl32(P_i - H_ik) - fl32(tpos_i - tneg_ik)), mm = sum df^2,
               dsm = fl32(fl32(fl32(lam_mm 2) df) / (B k)); margin_mse = fl32(mm / (B k)); never rounded to bf16
    dpos       dpos_i = sum_kk dsm_ik
    KD         student sv_ij = fl32(x inv_tkd), x = bf16(D_i,off+j) in bf16 mode (the SAME dots), teacher tv_ij =
               fl32(t_ij inv_tkd), j over the B own positives; lse_s, lse_t as above; ls = fl32(sv - lse_s), lt =
               fl32(tv - lse_t), pt = expf(lt); kd = sum over pt > 0 of fl32(pt fl32(lt - ls)) (xlogy: a zero teacher
               probability contributes nothing); kd_loss = fl32(kd / B);
               Gkd_ij = fl32(fl32(expf(ls) - pt) gk), gk = fl32(fl32(lam_kd inv_tkd) / B); bf16(.) in bf16 mode
    means      mq_c = fl32(sum_r q_rc / B), mp_c = fl32(sum_r p_(off+r)c / B), mn_c = fl32(sum over the B k rows of n / (B k))
    FLOPS      flops_q = sum_c fl32(mq_c^2), flops_d, flops_neg alike
    counts     nonzero_q = fl32(#{q_rc > 0} / B), nonzero_d = fl32(#{p_(off+r)c > 0} / B): exact integers below 2^24
    out[9]     {loss, infonce, flops_q, flops_d, flops_neg, margin_mse, nonzero_q, nonzero_d, kd}; loss adds its terms left
               to right: infonce + lam_q flops_q + lam_d flops_d + lam_neg flops_neg + [lam_kd kd_loss] + [lam_mm margin_mse]
    dq_ic      go fl32(R + [K] + sum_kk Gh_ik n_(ik)c + (dpos_i p_(off+i)c + fq mq_c)); R = sum_j G_ij b_jc, rounded to bf16
               in bf16 mode; K = sum_j Gkd_ij b_(off+j)c, a SECOND product rounded to bf16 on its own; fq = fl32(fl32(2
               lam_q) / B); go = gout[0]
    dp_jc      go fl32(R' + [K'] + [dpos_il q_il,c + fd mp_c]), R' = sum_i G_ij a_ic, K' = sum_i Gkd_i,il a_ic, il = j -
               off: the bracketed terms only for the B local rows; remote rows receive the in-batch term alone
    dn_rc      go fl32(Gh_r q_ic + fn mn_c), i = r / k, fn = fl32(fl32(2 lam_neg) / (B k))

Acceptance sets, not tolerances.  Every quantity is an interval [lo, hi] of fp32 values (adamw_reference.Iv): the real
result of an operation over the corners of its operands, rounded outward to fp32 -- one rounding per fp32 operation, a
correctly rounded division, a contracted fma inside the same interval.  What is not a single operation:
    sums       n operands in ANY order, fused or not: gamma_(n-1) sum|operand|, gamma_n when the operands are products
               formed inside the sum; u = 2^-24; times 1 + 2^-20 for the float64 evaluation.  Nothing knows the chunk
               width, the 4-way split of loss_sum_partials_kernel or the wave layout.  Where all operands are multiples
               of one power of two g and sum|operand| <= 2^24 g, every partial sum is an fp32 value: the sum is exact.
    bf16       a bf16-rounded quantity passes iff it lies between the bf16 roundings of the interval's corners
    lse        log-sum-exp is monotone in every logit with slopes that add up to 1: logits known to within delta give
               lse to within delta -- [LSE(lo), LSE(hi)] --, widened by the evaluation's own error: rho / (1 - rho) +
               2u ULP_LOGF (ln NS + 1) + u (|lse| + 1), rho = expm1(104 u + 2u ULP_EXPF + gamma_NS) + NS 2^-148 (a
               term below e^-104 is zero or the smallest subnormal).  Each probability is then known to within
               e^(+-2 delta): the interval of fl32(s_ij - lse) carries exactly that.
    ASSUMPTION (EXPF, LOGF): expf and logf are library calls.  Neither the guides nor the headers and documents of the
               ROCm installation state their accuracy: ULP_EXPF = ULP_LOGF = 2 ulp (4u relative) are ASSUMED, of the
               same kind as RCP-EXP of gemm_reference and RSQ of rows_reference.
    No constant was fitted to a kernel's output.

Input families (build_case):
    exact_a   multiples of 0.25, sparse, non-negative, positives that resemble their anchors: scores of 5e3 .. 2e4, every
              partial sum an fp32 value, so a score is known exactly and its bf16 rounding (ulp 32 .. 128) is a fact.  At
              tau = 1 the soft-max is one-hot except where planted: positive row Bp - 1 (or 1) is a near copy of row off
              whose exact score against anchor 0 differs by less than a bf16 ulp and rounds to the SAME bf16 value -- in
              bf16 mode the two probabilities tie exactly, in fp32 mode they do not --, and the label of the last anchor
              is not the arg-max.
    exact_b   multiples of 2^-9 below 1.25 (nine significant bits: NOT bf16 values), sparse: scores below 8 about 1 apart,
              a spread soft-max, G not one-hot.  exact_a alone is blind to soft-max errors, exact_b sees the operand rounding.
    random    relu(s (randn - c)) rows of mixed density, one all-zero row each in q, p, n (from three rows on), one column
              that is zero everywhere, values that are not bf16 values, s such that scores stay below ~4: the bf16 ulp of
              a score is <= 2^-6, so a probability whose score interval straddles a rounding boundary is known to
              e^(+-2^-5) = 3.2 %, every other one to ~1e-6 (worst relative half-width, from the reference alone:
              tests/test_loss_reference_host.py prints it)
    teachers  MarginMSE scores 3 randn (both signs); KD scores 2 randn with row 0 peaked at 400 (T_kd = 2: every other
              teacher probability of that row underflows to 0: the pt > 0 branch)

Width of the sets, from the reference alone (tests/test_loss_reference_host.py): in the random family in bf16 mode the
worst relative half-width of a probability is 3.5 % (a score interval that straddles a bf16 rounding boundary, 2^-6, and
lse moved by as much); in exact_a at tau = 1 the label's coefficient is known to u |lse| ~ 2e-3 of gs only, because
fl32(mx + logf(se)) is rounded at a magnitude of 2e4: that is fp32 at the production temperature, not a loose bound.

Measured on an MI355X with the kernels of commit 9db777b (the change that adds this file touches no kernel), over all
cases of tests/test_gpu_loss_per_element.py: 38 tests, 5.7 s for the file, the slowest test 0.5 s (B = 16, Bp = 768,
V = 4,117).  Nothing fell outside its acceptance set in either mode, family or launch form; no guard was touched and no
sentinel read; the three shapes above 64 KiB of dynamic LDS (83,200 / 131,840 / 135,296 B) launched and passed without
an opt-in.  The same outputs were also held to the sets of ULP_EXPF = ULP_LOGF = 1 and of 0 (expf and logf taken as
exact before the outward rounding): 0 elements outside in both, so ASSUMPTION (EXPF, LOGF) never decided an element; the
constants stay at their assumed value 2.  The bf16-rounded coefficients G the forward leaves in its workspace, bf16 mode,
300,328 elements over all cases and families: 15.0 % zero or below 2^-120, 81.3 % one admissible value (met bit for
bit), 3.2 % two adjacent values, 0.41 % more (the labels of exact_a, see above).
tests/test_loss_reference_host.py: 78 tests, 42 s on the CPU.
"""
import functools
from types import SimpleNamespace

import numpy as np

from tests.adamw_reference import Iv, _c
from tests.gemm_reference import U32, bf16_round
from tests.rows_reference import F64, gamma

f32 = np.float32
ULP_EXPF = 2                 # ASSUMPTION (EXPF), see the docstring
ULP_LOGF = 2                 # ASSUMPTION (LOGF)
FAMILIES = ("exact_a", "exact_b", "random")
OUT_NAMES = ("loss", "infonce", "flops_q", "flops_d", "flops_neg", "margin_mse", "nonzero_q", "nonzero_d", "kd")
LAMBDAS = dict(lam_q=0.013, lam_d=0.007, lam_neg=0.003, lam_mm=0.11, lam_kd=0.23, T_kd=2.0)
BF16_TINY = 2.0 ** -120


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- launch arithmetic, restated
def pick_ch(B, Bp):
    ch = 128
    while ch > 16 and (B + Bp) * ch * 4 > 96 * 1024:
        ch >>= 1
    return ch


def lds_bytes(B, Bp, k):
    """(loss_partial_kernel and loss_bwd_kernel, loss_reduce_kernel)"""
    return (B + Bp) * (pick_ch(B, Bp) + 1) * 4, (B * (Bp + k) + B * k + B) * 4


def dims_ok(B, Bp, k, V, off):
    if B <= 0 or Bp < B or k <= 0 or V <= 0 or off < 0 or off + B > Bp:
        return False
    if B > 256 or Bp > 1024 or k > 16:
        return False
    return lds_bytes(B, Bp, k)[1] <= 150 * 1024


def workspace_bytes(B, Bp, k, V):
    if B <= 0 or Bp < B or k <= 0 or V <= 0:
        return 0
    nchunk = cdiv(V, pick_ch(B, Bp))
    return 4 * (nchunk * (B * Bp + B * k + B + 8) + 3 * V + 2 * (B * Bp + B * k + B) + B * B)


def case_classes(c):
    ch = pick_ch(c["B"], c["Bp"])
    nchunk = cdiv(c["V"], ch)
    cl = {f"CH {ch}", f"nchunk % 4 = {nchunk % 4}" if nchunk >= 4 else "nchunk < 4"}
    if c["V"] < ch:
        cl.add("V below one chunk")
    if c["V"] == ch:
        cl.add("V exactly one chunk")
    if c["V"] % ch and nchunk > 1:
        cl.add("ragged last chunk")
    if nchunk > 256:
        cl.add(f"nchunk > 256 at CH {ch}")
    if c["B"] % 4 or c["Bp"] % 4:
        cl.add("clamped 4x4 block")
    if c["B"] > 16:
        cl.add("second dq round")
    if max(lds_bytes(c["B"], c["Bp"], c["k"])) > 64 * 1024:
        cl.add("LDS above 64 KiB")
    return cl


# ----------------------------------------------------------------------------- interval helpers
def iv_exp(x, ulp=None):
    ulp = ULP_EXPF if ulp is None else ulp
    r, sub = 2 * U32 * ulp, ulp * 2.0 ** -149                   # ulps of the result; the subnormal spacing near zero
    with np.errstate(under="ignore"):
        return Iv._out(np.maximum(np.exp(x.lo) * (1 - r) - sub, 0.0), np.exp(x.hi) * (1 + r) + sub)


def iv_bf16(x):
    def rnd(v, up):
        r = bf16_round(v, check=False)
        small = np.abs(v) < BF16_TINY
        return np.where(small, np.where(v > 0, BF16_TINY if up else 0.0, np.where(v < 0, 0.0 if up else -BF16_TINY, 0.0)), r)
    return Iv(rnd(x.lo, False), rnd(x.hi, True))


def sum_any(x, axis, products=False):
    n = x.lo.shape[axis]
    A = np.maximum(np.abs(x.lo), np.abs(x.hi)).sum(axis)
    e = F64 * gamma(n if products else n - 1) * A
    return Iv._out(x.lo.sum(axis) - e, x.hi.sum(axis) + e)


def real_mul(a, b):
    """the real products of two intervals, NOT rounded (operands of a sum whose bound counts the product's rounding)"""
    c = [x * y for x in (a.lo, a.hi) for y in (b.lo, b.hi)]
    return Iv(np.minimum.reduce(c), np.maximum.reduce(c))


def dots(a, b, grid):
    """sum_c a_ic b_jc of point matrices in any order -> Iv; exact where every partial sum is an fp32 value"""
    S, A = a @ b.T, np.abs(a) @ np.abs(b).T
    e = F64 * gamma(a.shape[1]) * A
    if grid:
        e = np.where(A <= 2.0 ** 24 * grid * grid, 0.0, e)
    return Iv._out(S - e, S + e)


def iv_matmul(G, P):
    """sum_j G_ij P_jc, G an interval matrix, P a point matrix, any order"""
    Pp, Pn = np.maximum(P, 0.0), np.minimum(P, 0.0)
    lo, hi = G.lo @ Pp + G.hi @ Pn, G.hi @ Pp + G.lo @ Pn
    e = F64 * gamma(P.shape[0]) * (np.maximum(np.abs(G.lo), np.abs(G.hi)) @ np.abs(P))
    return Iv._out(lo - e, hi + e)


def col_mean(x, grid):
    n = x.shape[0]
    S, A = x.sum(0), np.abs(x).sum(0)
    e = F64 * gamma(n - 1) * A
    if grid:
        e = np.where(A <= 2.0 ** 24 * grid, 0.0, e)
    return Iv._out(S - e, S + e) / _c(n)


def lse_any(row, ulp_e=None, ulp_l=None):
    ulp_e, ulp_l = ULP_EXPF if ulp_e is None else ulp_e, ULP_LOGF if ulp_l is None else ulp_l

    def L(x):
        m = x.max(-1)
        return m + np.log(np.exp(x - m[:, None]).sum(-1))
    l_lo, l_hi = L(row.lo), L(row.hi)
    NS = row.lo.shape[-1]
    rho = np.expm1(104 * U32 + 2 * U32 * ulp_e + gamma(NS)) + NS * 2.0 ** -148
    E = F64 * (rho / (1 - rho) + 2 * U32 * ulp_l * (np.log(NS) + 1) + U32 * (np.maximum(np.abs(l_lo), np.abs(l_hi)) + 1))
    return Iv._out(l_lo - E, l_hi + E)


def col(x):
    return Iv(x.lo[:, None], x.hi[:, None])


def hull0(x, cond):
    """where cond, the value may also be exactly 0"""
    return Iv(np.where(cond, np.minimum(x.lo, 0.0), x.lo), np.where(cond, np.maximum(x.hi, 0.0), x.hi))


# ----------------------------------------------------------------------------- the contract
def expected(c, bf16_mm, ulp_e=None, ulp_l=None):
    """-> {"out9": (lo, hi) [1, 9], "dq", "dp", "dn": (lo, hi)} and, under "mid", the intermediate intervals"""
    B, Bp, k, V, off = c.B, c.Bp, c.k, c.V, c.off
    q, p, n = (np.asarray(x, dtype=np.float64) for x in (c.q, c.p, c.n))
    grid = c.grid
    tau, lam_q, lam_d, lam_neg, lam_mm, lam_kd, T_kd = (float(x) for x in c.hp)
    use_mm = lam_mm > 0 and c.tpos is not None
    use_kd = lam_kd > 0 and c.tsc is not None
    one = _c(1.0)
    inv_tau = one / _c(tau)
    inv_tkd = one / _c(T_kd) if T_kd > 0 else one
    a, b = (bf16_round(q, check=False), bf16_round(p, check=False)) if bf16_mm else (q, p)
    D = dots(a, b, grid)
    Db = iv_bf16(D) if bf16_mm else D
    s_in = Db * inv_tau
    own = p[off:off + B]
    H = dots(q, n, grid)
    H = Iv(H.lo[np.arange(B * k) // k, np.arange(B * k)].reshape(B, k), H.hi[np.arange(B * k) // k, np.arange(B * k)].reshape(B, k))
    Pd = sum_any(Iv(q * own), 1, products=True)
    if grid:
        A = (np.abs(q) * np.abs(own)).sum(1)
        Pd = Iv(np.where(A <= 2.0 ** 24 * grid * grid, (q * own).sum(1), Pd.lo), np.where(A <= 2.0 ** 24 * grid * grid, (q * own).sum(1), Pd.hi))
    s_h = H * inv_tau
    row = Iv(np.concatenate([s_in.lo, s_h.lo], 1), np.concatenate([s_in.hi, s_h.hi], 1))
    lse = lse_any(row, ulp_e, ulp_l)
    lab = off + np.arange(B)
    ce = lse - Iv(s_in.lo[np.arange(B), lab], s_in.hi[np.arange(B), lab])
    infonce = sum_any(ce, 0) / _c(B)
    gs = inv_tau / _c(B)
    onehot = np.zeros((B, Bp))
    onehot[np.arange(B), lab] = 1.0
    G = (iv_exp(s_in - col(lse), ulp_e) - Iv(onehot)) * gs
    if bf16_mm:
        G = iv_bf16(G)
    Gh = iv_exp(s_h - col(lse), ulp_e) * gs
    mid = SimpleNamespace(D=D, s_in=s_in, H=H, lse=lse, G=G)
    zero = Iv(np.zeros(()))
    mmse, dpos = zero, Iv(np.zeros(B))
    if use_mm:
        tp, tn = np.asarray(c.tpos, np.float64), np.asarray(c.tneg, np.float64).reshape(B, k)
        df = (col(Pd) - H) - (Iv(tp[:, None]) - Iv(tn))
        mm = sum_any(Iv(real_mul(df, df).lo.reshape(-1), real_mul(df, df).hi.reshape(-1)), 0, products=True)
        mm = Iv(np.maximum(mm.lo, 0.0), mm.hi)
        mmse = mm / _c(B * k)
        dsm = ((_c(lam_mm) * _c(2.0)) * df) / _c(B * k)
        dpos = sum_any(dsm, 1)
        Gh = Gh - dsm
    kdl, Gkd = zero, None
    if use_kd:
        x = Iv(Db.lo[:, off:off + B], Db.hi[:, off:off + B])
        sv = x * inv_tkd
        tv = Iv(np.asarray(c.tsc, np.float64)) * inv_tkd
        ls = sv - col(lse_any(sv, ulp_e, ulp_l))
        lt = tv - col(lse_any(tv, ulp_e, ulp_l))
        pt = iv_exp(lt, ulp_e)
        term = hull0(pt * (lt - ls), pt.lo <= 0)
        term = Iv(np.where(pt.hi <= 0, 0.0, term.lo), np.where(pt.hi <= 0, 0.0, term.hi))
        kdl = sum_any(Iv(term.lo.reshape(-1), term.hi.reshape(-1)), 0) / _c(B)
        gk = (_c(lam_kd) * inv_tkd) / _c(B)
        Gkd = (iv_exp(ls, ulp_e) - pt) * gk
        if bf16_mm:
            Gkd = iv_bf16(Gkd)
        mid.Gkd = Gkd
    mq, mp, mn = col_mean(q, grid), col_mean(own, grid), col_mean(n, grid)
    fl = [sum_any(real_mul(m, m), 0, products=True) for m in (mq, mp, mn)]
    fl = [Iv(np.maximum(f.lo, 0.0), f.hi) for f in fl]
    nzq, nzd = _c(f32((q > 0).sum()) / f32(B)), _c(f32((own > 0).sum()) / f32(B))      # one correctly rounded division each
    loss = infonce + _c(lam_q) * fl[0] + _c(lam_d) * fl[1] + _c(lam_neg) * fl[2]
    loss = loss + (_c(lam_kd) * kdl if use_kd else zero)
    loss = loss + (_c(lam_mm) * mmse if use_mm else zero)
    out = [loss, infonce, fl[0], fl[1], fl[2], mmse, nzq, nzd, kdl]
    exp = {"out9": (np.array([[float(o.lo) for o in out]]), np.array([[float(o.hi) for o in out]]))}
    # ---- backward
    go = _c(c.gout)
    fq, fd, fn = (_c(2.0) * _c(lam_q)) / _c(B), (_c(2.0) * _c(lam_d)) / _c(B), (_c(2.0) * _c(lam_neg)) / _c(B * k)
    R = iv_matmul(G, b)
    r = iv_bf16(R) if bf16_mm else R
    if use_kd:
        K = iv_matmul(Gkd, b[off:off + B])
        r = r + (iv_bf16(K) if bf16_mm else K)
    n3 = n.reshape(B, k, V)
    for kk in range(k):
        r = r + Iv(Gh.lo[:, kk:kk + 1], Gh.hi[:, kk:kk + 1]) * Iv(n3[:, kk])
    r = r + (col(dpos) * Iv(own) + fq * Iv(mq.lo[None, :], mq.hi[None, :]))
    dq = go * r
    Rp = iv_matmul(Iv(G.lo.T, G.hi.T), a)
    rp = iv_bf16(Rp) if bf16_mm else Rp
    loc = Iv(rp.lo[off:off + B], rp.hi[off:off + B])
    if use_kd:
        Kp = iv_matmul(Iv(Gkd.lo.T, Gkd.hi.T), a)
        loc = loc + (iv_bf16(Kp) if bf16_mm else Kp)
    loc = loc + (col(dpos) * Iv(q) + fd * Iv(mp.lo[None, :], mp.hi[None, :]))
    rp.lo[off:off + B], rp.hi[off:off + B] = loc.lo, loc.hi
    dp = go * rp
    qr = q[np.arange(B * k) // k]
    dn = go * (Iv(Gh.lo.reshape(-1, 1), Gh.hi.reshape(-1, 1)) * Iv(qr) + fn * Iv(mn.lo[None, :], mn.hi[None, :]))
    for name, iv in (("dq", dq), ("dp", dp), ("dn", dn)):
        exp[name] = (iv.lo, iv.hi)
    exp["mid"] = mid
    return exp


# ----------------------------------------------------------------------------- inputs
def _exact_a(B, Bp, k, V, off, rng):
    M = float(np.clip(np.sqrt(6.25e4 / V), 4, 64))              # label scores ~ 0.8 dens V M^2 / 3 ~ 1e4
    dens = min(0.6, 3.75e4 / (M * M * V))

    def rows(r):
        x = np.floor(rng.random((r, V)) * (4 * M) + 1) / 4
        return (x * (rng.random((r, V)) < dens)).astype(f32)
    q, p, n = rows(B), rows(Bp), rows(B * k)
    keep = rng.random((B, V)) < 0.8
    p[off:off + B] = np.where(keep, q, p[off:off + B])        # positives that resemble their anchors
    last = off + B - 1
    if B > 1:
        p[last] = np.floor(rows(1)[0])  / 4                     # unlike its anchor and small: this label is not the arg-max
    tie = None
    if Bp >= 2 and B >= 2:
        j2 = Bp - 1 if Bp - 1 >= off + B else (off + 1 if B > 2 else None)
        if j2 is not None:
            p[j2] = p[off]
            cands = np.nonzero((q[0] > 0) & (q[0] <= 2.0))[0]
            cc = cands[0] if len(cands) else int(np.argmin(np.where(q[0] > 0, q[0], np.inf)))
            p[j2, cc] += f32(0.25)
            tie = (off, j2)
    return q, p, n, 0.25, tie


def _exact_b(B, Bp, k, V, off, rng):
    dens = min(0.5, np.sqrt(5.4 / V))

    def rows(r):
        x = (128 + rng.integers(0, 513, (r, V))) / 512.0       # multiples of 2^-9 in [0.25, 1.25]
        return (x * (rng.random((r, V)) < dens)).astype(f32)
    return rows(B), rows(Bp), rows(B * k), 2.0 ** -9, None


def _random(B, Bp, k, V, off, rng):
    s = np.sqrt(50.0 / V)

    def rows(r):
        cut = rng.choice([0.0, 0.5, 1.0, 1.5], (r, 1))
        x = np.maximum(s * (rng.standard_normal((r, V)) - cut), 0.0)
        x[:, V // 2] = 0.0                                      # one column that is zero in every row
        if r >= 3:
            x[r // 2] = 0.0                                     # one all-zero row
        return x.astype(f32)
    return rows(B), rows(Bp), rows(B * k), None, None


CASES = {
    # name: B, Bp, k, V, off, tau, mm, kd, gout                 which seam
    "b1": dict(B=1, Bp=1, k=1, V=40, off=0, tau=1.0, mm=False, kd=False, gout=1.0),           # one row; V below one chunk
    "b3_one_chunk": dict(B=3, Bp=4, k=3, V=128, off=1, tau=20.0, mm=True, kd=False, gout=0.25),   # Bp - B = 1, label_off last
    "b4_258_chunks": dict(B=4, Bp=4, k=1, V=128 * 257 + 5, off=0, tau=1.0, mm=True, kd=True, gout=1.0),   # nchunk > 256 at CH 128
    "b13_5_chunks": dict(B=13, Bp=52, k=3, V=128 * 4 + 9, off=13, tau=1.0, mm=True, kd=True, gout=0.3),    # 3 B remote rows, middle
    "b17_7_chunks": dict(B=17, Bp=17, k=16, V=128 * 6 + 1, off=0, tau=20.0, mm=False, kd=True, gout=1.0),  # k = 16; second dq round
    "b64_8_chunks": dict(B=64, Bp=64, k=1, V=128 * 7 + 100, off=0, tau=1.0, mm=True, kd=False, gout=0.25),
    "b13_6_chunks": dict(B=13, Bp=14, k=3, V=128 * 5 + 64, off=0, tau=20.0, mm=True, kd=True, gout=0.3),   # label_off first of a wider P
    "ch64": dict(B=40, Bp=160, k=3, V=64 * 2 + 5, off=120, tau=1.0, mm=False, kd=True, gout=1.0),          # KD, Bp > B, label_off last
    "ch32": dict(B=64, Bp=336, k=1, V=32 * 5 + 3, off=100, tau=1.0, mm=True, kd=True, gout=0.3),
    "ch16_258_chunks": dict(B=16, Bp=768, k=1, V=16 * 257 + 5, off=368, tau=1.0, mm=False, kd=False, gout=1.0),
    "zero_lambda": dict(B=4, Bp=8, k=1, V=130, off=4, tau=1.0, mm=False, kd=False, gout=1.0, zero=True),   # out[0] == out[1]
}
# dynamic LDS above 64 KiB: a test function of their own, collected last
LDS_CASES = {
    "cfg4_256": dict(B=64, Bp=256, k=1, V=200, off=64, tau=1.0, mm=False, kd=False, gout=1.0),    # 83,200 / 66,304 B
    "cfg4_512": dict(B=64, Bp=512, k=1, V=200, off=192, tau=1.0, mm=True, kd=True, gout=1.0),     # 76,032 / 131,840 B
    "near_150k": dict(B=32, Bp=1024, k=16, V=50, off=992, tau=20.0, mm=True, kd=False, gout=0.25),   # 71,808 / 135,296 B
}
ALL_CASES = dict(CASES, **LDS_CASES)
REFUSED = (  # (B, Bp, k, V, off): SNX_E_SHAPE
    (0, 4, 1, 8, 0), (5, 4, 1, 8, 0), (4, 4, 0, 8, 0), (4, 4, 1, 0, 0), (4, 4, 1, 8, -1), (4, 6, 1, 8, 3), (257, 257, 1, 8, 0),
    (4, 1025, 1, 8, 0), (4, 4, 17, 8, 0), (256, 256, 1, 8, 0), (64, 1024, 16, 8, 0),
)
REQUIRED_CLASSES = {"CH 128", "CH 64", "CH 32", "CH 16", "nchunk % 4 = 0", "nchunk % 4 = 1", "nchunk % 4 = 2", "nchunk % 4 = 3",
                    "nchunk < 4", "V below one chunk", "V exactly one chunk", "ragged last chunk", "nchunk > 256 at CH 128",
                    "nchunk > 256 at CH 16", "clamped 4x4 block", "second dq round", "LDS above 64 KiB"}


@functools.lru_cache(maxsize=8)
def build_case(name, family):
    d = ALL_CASES[name]
    B, Bp, k, V, off = d["B"], d["Bp"], d["k"], d["V"], d["off"]
    assert dims_ok(B, Bp, k, V, off)
    rng = np.random.default_rng(10007 * B + 101 * Bp + 13 * V + FAMILIES.index(family))
    q, p, n, grid, tie = {"exact_a": _exact_a, "exact_b": _exact_b, "random": _random}[family](B, Bp, k, V, off, rng)
    lam = {kk: 0.0 for kk in LAMBDAS} if d.get("zero") else dict(LAMBDAS)
    if not d["mm"]:
        lam["lam_mm"] = 0.0
    if not d["kd"]:
        lam["lam_kd"] = 0.0
    hp = np.array([d["tau"], lam["lam_q"], lam["lam_d"], lam["lam_neg"], lam["lam_mm"], lam["lam_kd"], LAMBDAS["T_kd"]], f32)
    tpos = (3 * rng.standard_normal(B)).astype(f32) if d["mm"] else None
    tneg = (3 * rng.standard_normal(B * k)).astype(f32) if d["mm"] else None
    tsc = None
    if d["kd"]:
        tsc = (2 * rng.standard_normal((B, B))).astype(f32)
        tsc[0, 0] = 400.0
    c = SimpleNamespace(name=name, family=family, B=B, Bp=Bp, k=k, V=V, off=off, q=q, p=p, n=n, grid=grid, tie=tie, hp=hp,
                        tpos=tpos, tneg=tneg, tsc=tsc, gout=float(f32(d["gout"])), CH=pick_ch(B, Bp))
    if grid:
        for x in (q, p, n):
            assert bool(np.all(x / grid == np.floor(x / grid))) and bool(np.all(x >= 0))
    return c

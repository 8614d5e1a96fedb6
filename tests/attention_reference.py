"""Float64 restatement of the attention kernels (csrc/attention.hip, attention_unit.hip, attention_1p.hip), a case
builder, and a per-element check whose bounds are DERIVED from the kernels' documented cast points.  Plain torch on the
CPU; sibling of tests/splade_bwd_reference.py.

The operation.  qkv [T, 3, heads, 64] bf16 (RoPE already applied), sequences are the row ranges cu[s] .. cu[s + 1].  Key j
is visible to query i of the same sequence iff mask[j] != 0 and (window < 0 or |i - j| <= window); the query's own mask
bit is not consulted.  Per (sequence, head), with scale = 0.125 and sums over the visible keys only:
    forward    s = scale q k^T,  lse_i = logsumexp_j s_ij,  P = exp(s - lse),  O = P v
    backward   takes out_in (bf16) and lse_in (fp32) as the kernels do:  delta_i = sum_d dO_id out_in_id,
               P = exp(s - lse_in),  dS = P o (dO v^T - delta),  dV = P^T dO,  dQ = scale dS k,  dK = scale dS^T q
    rope       with a (cos, sin) table and positions, dQ and dK leave through the transposed rotation that
               store_grad_rows (csrc/attention_common.h) applies to the pair (d, d + 32), d < 32:
               lo = g_d cos + g_{d+32} sin,  hi = g_{d+32} cos - g_d sin.

Cast points (headers of the three sources): fp32 scores from bf16 x bf16 MFMAs; P (forward: the not yet normalised
p~ = 2^(t - m), t the score in the log2 domain, m the running maximum) and dS rounded to bf16 as MFMA operands; fp32
accumulation; bf16 results; lse in fp32.

Bounds.  u = 2^-8 (bf16 unit roundoff: 8 significand bits, round to nearest), e = 2^-24 (fp32).  n = keys (or queries)
of the sequence, NT = ceil(n / 64) its tiles.  |.| is the element-wise absolute value, A_ij = sum_d |q_id| |k_jd|,
B_ij = sum_d |dO_id| |v_jd|, D_i = sum_d |dO_id| |out_in_id|, z_ij = s_ij (natural-log domain).

First order: the bf16 rounding of every P (dS) operand and of the result -- rigorous sums of absolute values:
    out  u (P |v|) + u |O|                    dV  u (P^T |dO|) + u |dV|
    dQ   scale u (|dS| |k|) + u |dQ|          dK  scale u (|dS|^T |q|) + u |dK|
(forward: sum_j bf16(p~_j) v_j / l with l the fp32 sum of the UNROUNDED p~: the relative rounding of p~_j is that of P_j.)

Second order, each with its derivation:
  C = 64 + 3      fp32 sums of 64 exact bf16 x bf16 products: 63 additions, and a 64th for the row constant that the one-pass
                  kernel carries as the initial accumulator, each ASSUMED to err by at most e of its result whatever the
                  order in which the MFMA adds (its internal order is not stated in the guides): 64 e times the sum of
                  magnitudes.  + 3: the rounded constant scale log2(e), the product (or fma) with it, and the product
                  lse_in log2(e) of the two-pass kernels.
  rho_ij          relative error of the backward's P_ij = 2^(c2 s - lse_in log2 e) (two-pass) or 2^(c2 (s - lse_in / scale))
                  with -lse_in / scale as the MFMA's initial accumulator (one-pass):
                      C e (scale A_ij + |lse_in_i|)      score and row constant summed in fp32
                    + e |z_ij - lse_in_i|                rounding of the exponent itself
                    + 4 e                                v_exp_f32, ASSUMED accurate to 2 fp32 ulp (= 4 e; not stated in the guides)
  E_i (forward)   relative error of every p~_ij after all rescales, and of l_i:
                      C e scale max_j A_ij               scores
                    + 5 e Z_i, Z_i = max_j |z_ij|        t = fl(s c2), t - m and the m_old - m_new of the rescales, whose
                                                         magnitudes add up to at most 5 Z_i
                    + e (4 + 5 NT + n + 8)               v_exp (4 e), per rescale v_exp of alpha + the product (5 e), fp32
                                                         accumulation of n terms of one sign (n e) and 1 / l, o * inv, shuffles
                  out: the numerator and l both carry it -> 2 E_i (P |v|).
  lse             E_i (relative error of l = absolute error of ln l; the error of m is the score term of E_i)
                  + e (3 |lse| + 26): v_log_f32 ASSUMED 2 ulp: 4 e |ln l| <= 4 e ln 513 < 26 e; m + log2 l, the product
                  with ln 2 and that constant: 3 e |lse|.
  dS              |dS_ij| (rho_ij + 2 e)  +  P_ij C e (B_ij + 2 D_i): dP - delta is formed in fp32 from a 64-term sum
                  (C e B_ij), a 64-term sum for delta (64 e D_i) and their difference, or with -delta as the initial
                  accumulator (C e (B_ij + D_i)): the CANCELLATION term -- it does not shrink with dS, and is all that is
                  left when dS = 0 exactly (one visible key).
  accumulation    over keys (dQ) or queries (dK, dV) in fp32: (n + 2) e times the sum of magnitudes; scale is a power of 2.
  total           bound = 1.01 (first order + second order): 1 + u < 1.01 is the rounding of an inexact fp32 result to
                  bf16 (u |computed| <= u |exact| + u err) and the products of two of the terms above.
  rope epilogue   y = bf16(acc scale) is the plain result (bound b); lo = bf16(fl(y1 cos + y2 sin)), hi likewise: the two
                  extra roundings are the fp32 arithmetic (2 e (|y1 cos| + |y2 sin|), covering a product and a sum or an
                  fma) and the second bf16 rounding (u |lo|); b passes through the rotation as |cos| b1 + |sin| b2.
  underflow       a P below 2^-120 may be flushed or rounded as a subnormal: 2^-120 per term, times the other operand.
Exact requirements: where a bound is 0 the result is 0 -- dK and dV of a masked key, dQ of a row without a visible key;
every output is finite.  Forward rows without a visible key (masked tokens only): out and lse only finite (the oracle's
note in oracle/splade_oracle.py, sdpa: such rows are don't-care).  No number here is tuned: nothing beyond the 1.01.

Measured worst err / bound on an MI355X, over all cases of tests/test_gpu_attention_per_element.py, with the kernels of
commit 8f9e9ca (the change that adds this file touches no kernel); the float64 simulation of the cast points in
tests/test_attention_reference_host.py has the same worst figures (out 0.825, dQ 0.887, dK 0.904, dV 0.890; lse 0.010):
    forward   resident            out 0.825   lse 0.031        (sequence groups: out 0.660, lse 0.029)
              streaming           out 0.825   lse 0.031
    backward  one-pass            dQ 0.887    dK 0.904    dV 0.869     (sequence groups: 0.750, 0.791, 0.737)
              resident two-pass   dQ 0.887    dK 0.904    dV 0.869     (sequence groups: 0.750, 0.791, 0.737)
              streaming two-pass  dQ 0.887    dK 0.904    dV 0.890
    chain (kernel forward, then kernel backward)      out 0.738, lse 0.031, dQ 0.770, dK 0.744, dV 0.788
    fused inverse rope, all three backward forms      dQ 0.530, dK 0.576, dV 0.542
The worst elements stand in the window-1 cases (two or three keys per row: the least averaging of the roundings).
"""
import math
from types import SimpleNamespace

import torch

U = 2.0 ** -8
E = 2.0 ** -24
C = 64 + 3
TINY = 2.0 ** -120
SCALE = 0.125
BF16 = torch.bfloat16
F64 = torch.float64

RECIPES = ("ones", "right", "left", "holes", "alternate", "mix")


# ----------------------------------------------------------------------------- cases
def seq_mask(recipe, n, b):
    """mask of sequence number b (n tokens); every recipe leaves at least one valid token.
      ones       all valid
      right      a valid prefix of 1, n // 3 or n - 1 tokens (b % 3): one valid token, wholly masked trailing tiles
      left       the first 64 + 3 b tokens masked where at least two stay valid (the first key tile is wholly masked),
                 else the first n // 2
      holes      single masked tokens at n // 5, n // 2 and n - 2 - (b % 2) (interior: first and last stay valid)
      alternate  every other key masked, starting with token b % 2
      mix        right, left, holes, alternate, ones by b % 5"""
    m = torch.ones(n, dtype=torch.int64)
    if recipe == "mix":
        recipe = ("right", "left", "holes", "alternate", "ones")[b % 5]
    if recipe == "right":
        m[(1, max(1, n // 3), max(1, n - 1))[b % 3]:] = 0
    elif recipe == "left":
        m[:64 + 3 * b if n >= 66 + 3 * b else n // 2] = 0
    elif recipe == "holes":
        for p in (n // 5, n // 2, n - 2 - (b % 2)):
            if 0 < p < n - 1:
                m[p] = 0
    elif recipe == "alternate":
        m[(b % 2)::2] = 0
        if n == 1:
            m[0] = 1
    elif recipe != "ones":
        raise ValueError(recipe)
    assert int(m.sum()) >= 1
    return m


def make_case(lens, heads, window, recipe="ones", seed=0, qk_scale=1.1, v_scale=1.0, do_scale=0.5, peaked=None):
    """qkv [T, 3 heads 64] bf16, dout [T, heads 64] bf16 (zero at masked tokens), mask int64 [T], cu int32.
    peaked = "up" / "down": q_i = 2 w + noise, k_j = 3 (j + 1) / n w + noise for one direction w per head (|w|^2 ~ 64), so
    the scores of a row climb by ~48 over the sequence (softmax sharp, running maximum rising up to the last tile);
    "down" reverses k along the sequence."""
    gen = torch.Generator().manual_seed(seed)
    lens = [int(x) for x in lens]
    B, T = len(lens), sum(lens)
    cu = torch.zeros(B + 1, dtype=torch.int64)
    cu[1:] = torch.tensor(lens).cumsum(0)
    qkv = torch.randn(T, 3, heads, 64, generator=gen)
    qkv[:, :2] *= qk_scale
    qkv[:, 2] *= v_scale
    if peaked:
        w = torch.randn(heads, 64, generator=gen)
        for b, n in enumerate(lens):
            ramp = torch.arange(1, n + 1, dtype=torch.float32) / n
            if peaked == "down":
                ramp = ramp.flip(0)
            s = slice(int(cu[b]), int(cu[b + 1]))
            qkv[s, 0] = 2.0 * w + 0.3 * qkv[s, 0]
            qkv[s, 1] = 3.0 * ramp[:, None, None] * w + 0.3 * qkv[s, 1]
    mask = torch.cat([seq_mask(recipe, n, b) for b, n in enumerate(lens)])
    dout = torch.randn(T, heads, 64, generator=gen) * do_scale
    dout[mask == 0] = 0
    return SimpleNamespace(lens=lens, B=B, T=T, heads=heads, window=int(window), recipe=recipe, max_len=max(lens),
                           cu=cu.to(torch.int32), mask=mask, qkv=qkv.reshape(T, 3 * heads * 64).to(BF16),
                           dout=dout.reshape(T, heads * 64).to(BF16))


def visibility(n, mask_seq, window):
    """[n queries, n keys] bool"""
    vis = (mask_seq != 0)[None, :].expand(n, n)
    if window >= 0:
        i = torch.arange(n)
        vis = vis & ((i[:, None] - i[None, :]).abs() <= window)
    return vis


def _units(case):
    """(slice of the sequence, head, q, k, v [n, 64] float64, visibility [n, n]) per (sequence, head)"""
    x = case.qkv.to(F64).view(case.T, 3, case.heads, 64)
    cu = case.cu.tolist()
    for b in range(case.B):
        sl = slice(cu[b], cu[b + 1])
        vis = visibility(cu[b + 1] - cu[b], case.mask[sl], case.window)
        for h in range(case.heads):
            yield sl, h, x[sl, 0, h], x[sl, 1, h], x[sl, 2, h], vis


def no_visible_key(case):
    """[T] bool: rows without a visible key (they can only be masked tokens)"""
    cu = case.cu.tolist()
    r = torch.cat([~visibility(cu[b + 1] - cu[b], case.mask[cu[b]:cu[b + 1]], case.window).any(dim=1)
                   for b in range(case.B)])
    assert not (r & (case.mask != 0)).any()
    return r


# ----------------------------------------------------------------------------- forward
def forward_reference(case):
    """-> namespace: out [T, heads 64], lse [heads, T] (float64; rows without a visible key: 0), their bounds out_b,
    lse_b, and novis [T]."""
    T, H = case.T, case.heads
    out, out_b = torch.zeros(T, H, 64, dtype=F64), torch.zeros(T, H, 64, dtype=F64)
    lse, lse_b = torch.zeros(H, T, dtype=F64), torch.zeros(H, T, dtype=F64)
    for sl, h, q, k, v, vis in _units(case):
        n = q.shape[0]
        any_vis = vis.any(dim=1)
        z = SCALE * (q @ k.t())
        zm = torch.where(vis, z, torch.full_like(z, -math.inf))
        l_ = torch.where(any_vis, torch.logsumexp(zm, dim=1), torch.zeros(n, dtype=F64))
        P = torch.where(vis, torch.exp(z - l_[:, None]), torch.zeros_like(z))
        O = P @ v
        A = torch.where(vis, q.abs() @ k.abs().t(), torch.zeros_like(z))
        Z = torch.where(vis, z.abs(), torch.zeros_like(z)).max(dim=1).values
        NT = (n + 63) // 64
        Ei = C * E * SCALE * A.max(dim=1).values + 5 * E * Z + E * (4 + 5 * NT + n + 8)
        Pv = P @ v.abs()
        out[sl, h] = O
        out_b[sl, h] = 1.01 * (U * Pv + U * O.abs() + 2 * Ei[:, None] * Pv + TINY * v.abs().sum(dim=0)[None, :])
        lse[h, sl] = l_
        lse_b[h, sl] = 1.01 * (Ei + E * (3 * l_.abs() + 26))
    return SimpleNamespace(out=out.view(T, H * 64), out_b=out_b.view(T, H * 64), lse=lse, lse_b=lse_b,
                           novis=no_visible_key(case))


def backward_inputs(ref):
    """the reference forward rounded the way the kernels' forward hands it on: out bf16, lse fp32, both 0 at rows
    without a visible key"""
    return ref.out.to(torch.float32).to(BF16), ref.lse.to(torch.float32)


def rope_pairs(g, gb, cos, sin):
    """transposed rotation of g [n, 64] with its bound gb; cos, sin [n, 32] float64 -> (rotated, bound)"""
    g1, g2, b1, b2 = g[:, :32], g[:, 32:], gb[:, :32], gb[:, 32:]
    lo, hi = g1 * cos + g2 * sin, g2 * cos - g1 * sin
    m = g1.abs() * cos.abs() + g2.abs() * sin.abs(), g2.abs() * cos.abs() + g1.abs() * sin.abs()
    lo_b = 1.01 * (cos.abs() * b1 + sin.abs() * b2 + 2 * E * m[0] + U * lo.abs())
    hi_b = 1.01 * (cos.abs() * b2 + sin.abs() * b1 + 2 * E * m[1] + U * hi.abs())
    return torch.cat([lo, hi], dim=1), torch.cat([lo_b, hi_b], dim=1)


def backward_reference(case, out_in, lse_in, rope_table=None, pos=None):
    """out_in [T, heads 64] bf16 and lse_in [heads, T] fp32 are used exactly as the kernels use them.  -> namespace: dqkv
    [T, 3 heads 64] float64 and its bound dqkv_b.  rope_table [P, 32, 2] fp32 (cos, sin), pos [T]: dQ and dK rotated."""
    T, H = case.T, case.heads
    d = torch.zeros(T, 3, H, 64, dtype=F64)
    db = torch.zeros(T, 3, H, 64, dtype=F64)
    dO_all = case.dout.to(F64).view(T, H, 64)
    o_all = out_in.to(F64).view(T, H, 64)
    lse_all = lse_in.to(F64)
    if rope_table is not None:
        cs = rope_table.to(F64)[pos.to(torch.int64)]          # [T, 32, 2]
    for sl, h, q, k, v, vis in _units(case):
        n = q.shape[0]
        dO, o, l_ = dO_all[sl, h], o_all[sl, h], lse_all[h, sl]
        zero = torch.zeros(n, n, dtype=F64)
        z = SCALE * (q @ k.t())
        P = torch.where(vis, torch.exp(z - l_[:, None]), zero)
        delta = (dO * o).sum(dim=1)
        dS = P * (dO @ v.t() - delta[:, None])
        dV, dQ, dK = P.t() @ dO, SCALE * (dS @ k), SCALE * (dS.t() @ q)
        A, Bm, D = q.abs() @ k.abs().t(), dO.abs() @ v.abs().t(), (dO.abs() * o.abs()).sum(dim=1)
        rho = C * E * (SCALE * A + l_.abs()[:, None]) + E * (z - l_[:, None]).abs() + 4 * E
        acc = (n + 2) * E
        Pe = P * (U + rho + acc) + torch.where(vis, torch.full_like(z, TINY), zero)          # |error of P_ij| as an operand
        Se = dS.abs() * (U + rho + 2 * E + acc) + P * C * E * (Bm + 2 * D[:, None]) \
            + torch.where(vis, TINY * (Bm + D[:, None]), zero)                               # |error of dS_ij|
        dV_b = 1.01 * (Pe.t() @ dO.abs() + U * dV.abs())
        dQ_b = 1.01 * (SCALE * (Se @ k.abs()) + U * dQ.abs())
        dK_b = 1.01 * (SCALE * (Se.t() @ q.abs()) + U * dK.abs())
        if rope_table is not None:
            dQ, dQ_b = rope_pairs(dQ, dQ_b, cs[sl, :, 0], cs[sl, :, 1])
            dK, dK_b = rope_pairs(dK, dK_b, cs[sl, :, 0], cs[sl, :, 1])
        d[sl, 0, h], d[sl, 1, h], d[sl, 2, h] = dQ, dK, dV
        db[sl, 0, h], db[sl, 1, h], db[sl, 2, h] = dQ_b, dK_b, dV_b
    return SimpleNamespace(dqkv=d.view(T, 3 * H * 64), dqkv_b=db.view(T, 3 * H * 64), heads=H)


# ----------------------------------------------------------------------------- checks
def _ratio(got, want, bound):
    """worst |got - want| / bound over all elements: 0 where the error is 0, inf where a bound of 0 is missed or the
    result is not finite"""
    err = torch.nan_to_num((got - want).abs(), nan=math.inf, posinf=math.inf)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    return float(r.max()) if r.numel() else 0.0


def _verdict(what, ratios, bad):
    for name, r in ratios.items():
        if not r <= 1.0:
            bad.append(f"{name}: bound violated, worst err / bound ratio {r:.3g}")
    msg = f"{what}: worst err / bound ratio " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items())
    print(msg)
    assert not bad, msg + " -- " + "; ".join(bad)
    return ratios


def forward_ratios(out, lse, ref):
    out, lse = out.detach().cpu().to(F64), lse.detach().cpu().to(F64)
    rows = ~ref.novis
    return {"out": _ratio(out[rows], ref.out[rows], ref.out_b[rows]),
            "lse": _ratio(lse[:, rows], ref.lse[:, rows], ref.lse_b[:, rows])}


def check_forward(out, lse, ref, what=""):
    """every element of out and lse within its bound; rows without a visible key: finite.  Returns and prints the worst
    err / bound ratio per tensor."""
    bad = []
    if not (torch.isfinite(out.detach().cpu().float()).all() and torch.isfinite(lse.detach().cpu()).all()):
        bad.append("a non-finite value in out or lse")
    return _verdict(what, forward_ratios(out, lse, ref), bad)


def backward_ratios(dqkv, ref):
    T = dqkv.shape[0]
    g = dqkv.detach().cpu().to(F64).view(T, 3, -1)
    want, bound = ref.dqkv.view(T, 3, -1), ref.dqkv_b.view(T, 3, -1)
    return {n: _ratio(g[:, i], want[:, i], bound[:, i]) for i, n in enumerate(("dQ", "dK", "dV"))}


def check_backward(dqkv, ref, what=""):
    """every element of dQ, dK and dV within its bound; a bound of 0 (masked key, row without a visible key) demands an
    exact 0.  Returns and prints the worst err / bound ratio per tensor."""
    bad = []
    if not torch.isfinite(dqkv.detach().cpu().float()).all():
        bad.append("a non-finite value in dqkv")
    return _verdict(what, backward_ratios(dqkv, ref), bad)

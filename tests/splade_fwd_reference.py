"""Host restatement of the fused decoder GEMM + SPLADE tail forward (snx_decoder_splade_fwd*, csrc/splade_head.hip and
csrc/decoder256.hip), an input builder whose arithmetic is ORDER-INDEPENDENT, and a per-element checker.  No GPU, no snx.

The operation, for Hd [T, K] bf16, W [V, K] bf16, bias [V] fp32, cu_seqlens [B + 1], mask [T]:
    x[t, v]          = bf16( fp32(Hd[t] . W[v]) + fp32(bf16(bias[v])) )       one fp32 add, one round-to-nearest-even
    value[t, v]      = max(x, 0)                                              its 16 bits order like the values
    keys[b, v]       = bits(max over the VALID rows of sequence b) << 16 | 0xFFFF - (lowest sequence position attaining it)
                       0x0000FFFF when that value is 0 (no valid row, or no positive logit)
    sparse[b, v]     = log1p(that value)
    token_keys[t]    = bits(max over v < V) << 16 | 0xFFFF - (lowest column attaining it); 0x0000FFFF for a masked token,
                       a token outside [cu[0], cu[B]) and a token whose every logit is <= 0
    token_weights[t] = log1p(that value); 0 for a masked token
A row is valid when it lies inside its sequence and mask != 0.  Rows of the token buffer behind cu[B] must be masked.

The exact class (build_case, kind "exact").  Hd holds integers in [-4, 4], W integers / 16 in [-4, 4] / 16.  Every partial
sum of the K loop is then a multiple of 2^-4 below 2^20 in magnitude: exact in fp32 in ANY order and in either MFMA
shape (the builder asserts  sum_k |h| |w| 2^4 < 2^24  per logit).  What follows the accumulation -- the fp32 add of
bf16(bias), the rounding to bf16, relu, two maxima with tie rules -- is deterministic IEEE arithmetic, so keys and
token_keys are known to the BIT and both kernel forms must reproduce them; only log1pf is left to a bound.  The builder
plants what random data does not contain: duplicated Hd rows inside a sequence (ties between two valid rows; the pairs
straddle the 32-row sub-tile seams in list position and the 64 / 128-row chunk seams in sequence position, the copy
before and behind the original), duplicated W rows with equal bias (ties between two columns, across the 32-, 96-,
128- and 192-column seams), bias values on the bf16 grid, off it (the rounding of the bias matters) and of the form
+-2^-s (1 +- 2^-9) that put x exactly halfway between two bf16 values once rounded and off the tie when not, a fifth of
the columns dead (<= 0 on every row), and column V - 1 strong enough to be a token's arg-max.  Its conditions (asserted,
not measured; a case names the ones its shape cannot meet in `waive`): >= 10 % of the (b, v) entries zero and >= 10 %
positive; >= 5 % of the positive entries with their maximum tied between two valid rows; >= 5 % of the live tokens with
their maximum tied between two columns; at least one logit an exact rounding tie.

The generic class (kind "generic"): random normal bf16 inputs at the scales of tests/test_gpu_ops.py.  Per logit the
fp32 result lies in x +- e,  e = gamma_(K+2) (sum |h||w| + |b|) + u |x|  (u = 2^-24, gamma_n = n u / (1 - n u), Higham 4.2:
K products exact in fp32, K - 1 additions in any order, the bias add; + 2^-40 of the magnitude for the float64 product
of this file).  Rounding is monotone, so the bf16 value lies between the roundings L and H of the interval's ends: one or
two candidates.  A reported maximum must lie in [max L, max H]; the reported row (column) must be valid, its own [L, H]
must contain the value, and no earlier valid row (lower column) may have L >= the value.  An entry with max L != max H is
AMBIGUOUS; at most 5 % of the (b, v) entries and 5 % of the live tokens of a case may be (AMBIGUOUS_CAP; the checker
fails the case otherwise).  With S = 300, V = 777 the share is 0.6 / 0.3 % at K = 64, 0.9 / 0.7 % at 128, 2.7 / 3.3 % at
256 and 12 % at 768: the generic class stops at K = 256, larger K belongs to the exact class.

log1p.  sparse and token_weights are compared with the float64 log1p of the REPORTED value bits: exactly 0 for bits 0,
else within LOG1P_ULPS = 2 fp32 ulp: 1 ulp is the maximum error the HIP math API reference of the ROCm documentation
lists for log1pf (table "Single precision floating-point functions"; the installed headers -- __clang_hip_math.h maps
log1pf to __ocml_log1p_f32 -- state no figure), half an ulp is the rounding of the float64 reference to fp32, rounded up.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests.splade_bwd_reference import U, gamma

BF16 = torch.bfloat16
F64 = torch.float64
EMPTY_KEY = 0xFFFF
AMBIGUOUS_CAP = 0.05
LOG1P_ULPS = 2.0


# ----------------------------------------------------------------------------------------------- bit helpers
def value_bits_f32(x32, truncate=False):
    """fp32 logits -> bf16 bits after relu (int64).  truncate: the planted fault 'chop instead of round-to-nearest-even'."""
    if truncate:
        bits = (x32.contiguous().view(torch.int32).to(torch.int64) >> 16) & 0xFFFF
    else:
        bits = x32.to(BF16).view(torch.int16).to(torch.int64) & 0xFFFF
    return torch.where(bits >= 0x8000, torch.zeros_like(bits), bits)


def raw_bits_f32(x32):
    """fp32 logits -> bf16 bits, sign bit kept (for the planted fault 'relu missing')"""
    return x32.to(BF16).view(torch.int16).to(torch.int64) & 0xFFFF


def bits_value(bits):
    """bf16 bits (any integer tensor) -> float64 values"""
    return (bits.to(torch.int32) << 16).view(torch.float32).to(F64)


def _rne_bf16_value(x):
    """float64 -> nearest bf16 VALUE (ties to even) in ONE rounding, as float64.  (torch rounds float64 -> bf16 through
    fp32: two roundings.)  bf16 subnormals are not modelled: no logit of a case lies below 2^-100."""
    m, e = np.frexp(x)                                     # x = m 2^e, 0.5 <= |m| < 1
    return np.ldexp(np.rint(m * 256.0), e - 8)             # 8 significant bits; rint is round-half-even


def _value_bits_f64(x):
    """float64 logits -> bf16 bits after relu of their correctly rounded bf16 value (int64 tensor)"""
    v = torch.from_numpy(_rne_bf16_value(x.numpy())).to(torch.float32)      # exact: a bf16 value
    return value_bits_f32(v)


def rbf_bias(bias):
    return bias.to(torch.float32).to(BF16).to(torch.float32)


# ----------------------------------------------------------------------------------------------- the reference
def sequence_rows(cu, mask):
    """-> list over the sequences of (s0, length, valid sequence positions [n] int64)"""
    cu = [int(c) for c in cu]
    m = mask != 0
    out = []
    for b in range(len(cu) - 1):
        s0, ln = cu[b], cu[b + 1] - cu[b]
        out.append((s0, ln, torch.nonzero(m[s0:s0 + ln]).flatten()))
    return out


def forward_reference(Hd, W, bias, cu, mask, exact):
    """CPU tensors in.  Returns a namespace with, per logit, the candidate value bits L <= H [T, V] (equal in the exact
    class), `rows` (sequence_rows), `live` [T] (inside a sequence and mask != 0), and the exact routing of L:
    keys [B, V], tkeys [T] (int64, unsigned 32-bit values), sparse [B, V], tw [T] (float64).  In the exact class these
    ARE the operation's outputs; in the generic class they are one admissible answer."""
    T, K = Hd.shape
    V = W.shape[0]
    h, w = Hd.to(F64), W.to(F64)
    acc = h @ w.t()
    b32 = rbf_bias(bias)
    r = SimpleNamespace(T=T, V=V, K=K, exact=exact)
    if exact:
        a32 = acc.to(torch.float32)
        assert (a32.to(F64) == acc).all(), "not an exact-class input: a logit's sum has no fp32 form"
        x32 = a32 + b32[None, :]                            # the kernels' one fp32 add
        r.x32 = x32
        r.L = r.H = value_bits_f32(x32)
    else:
        x = acc + b32.to(F64)[None, :]
        mag = h.abs() @ w.abs().t() + b32.to(F64).abs()[None, :]
        e = (gamma(K + 2) + 2.0 ** -40) * mag + U * x.abs()
        r.L, r.H = _value_bits_f64(x - e), _value_bits_f64(x + e)
        assert (r.L <= r.H).all()
    r.rows = sequence_rows(cu, mask)
    B = len(r.rows)
    r.B = B
    live = torch.zeros(T, dtype=torch.bool)
    keys = torch.full((B, V), EMPTY_KEY, dtype=torch.int64)
    for b, (s0, ln, vp) in enumerate(r.rows):
        if vp.numel() == 0:
            continue
        live[s0 + vp] = True
        vals = r.L[s0 + vp].numpy()                         # [n, V]
        first = torch.from_numpy(vals.argmax(0))            # numpy: the FIRST maximum
        m = torch.from_numpy(vals.max(0))
        keys[b] = torch.where(m > 0, (m << 16) | (0xFFFF - vp[first]), torch.full_like(m, EMPTY_KEY))
    r.live = live
    Ln = r.L.numpy()
    m = torch.from_numpy(Ln.max(1))
    c = torch.from_numpy(Ln.argmax(1))
    # (the column tag has 16 bits: no token keys above 65,535 columns, as in the kernels)
    r.tkeys = torch.where(live & (m > 0), (m << 16) | (0xFFFF - c), torch.full_like(m, EMPTY_KEY)) if V <= 65535 else None
    r.keys = keys
    r.sparse = torch.log1p(bits_value(keys >> 16))
    r.tw = torch.log1p(bits_value(torch.where(live, m, torch.zeros_like(m))))
    return r


# ----------------------------------------------------------------------------------------------- the checker
def _u32(t):
    return t.detach().cpu().to(torch.int64) & 0xFFFFFFFF


def _log1p_ratio(got, bits):
    """|got - log1p(value(bits))| in units of LOG1P_ULPS fp32 ulp of the reference, per element (float64); inf where
    bits = 0 and got is not an exact zero, and where got is NaN"""
    ref = torch.log1p(bits_value(bits))
    ulp = torch.from_numpy(np.spacing(ref.to(torch.float32).numpy()).astype(np.float64))
    g = got.detach().cpu().to(F64)
    ratio = (g - ref).abs() / (LOG1P_ULPS * ulp)
    ratio = torch.where(bits == 0, torch.where(g == 0, torch.zeros_like(ratio), torch.full_like(ratio, float("inf"))), ratio)
    return torch.nan_to_num(ratio, nan=float("inf"))


def check_forward(ref, keys, sparse, tw=None, tkeys=None, what=""):
    """Per-element check of one forward's outputs (tensors of any device; tw = None: the token half was not asked for;
    tkeys = None: no token keys) against forward_reference.  Raises AssertionError naming every violated requirement;
    returns a namespace of counts: checked (elements), sparse_ratio / tw_ratio (worst error over the log1p bound),
    amb_cols / amb_toks (ambiguous shares)."""
    bad = []
    B, V, T = ref.B, ref.V, ref.T
    kk = _u32(keys).view(B, V)
    r, low = kk >> 16, kk & 0xFFFF
    p = 0xFFFF - low
    n_amb = n_ent = 0
    cnt = dict(range=0, empty=0, row=0, own=0, first=0)
    for b, (s0, ln, vp) in enumerate(ref.rows):
        rb, pb = r[b], p[b]
        if vp.numel() == 0:
            cnt["empty"] += int((kk[b] != EMPTY_KEY).sum())
            continue
        Lb, Hb = ref.L[s0 + vp], ref.H[s0 + vp]
        lo, hi = Lb.max(0).values, Hb.max(0).values
        n_ent += V
        n_amb += int((lo != hi).sum())
        cnt["range"] += int(((rb < lo) | (rb > hi)).sum())
        zero = rb == 0
        cnt["empty"] += int((zero & (kk[b] != EMPTY_KEY)).sum())
        idx_of = torch.full((max(ln, 1) + 1,), -1, dtype=torch.int64)
        idx_of[vp] = torch.arange(vp.numel())
        i = idx_of[pb.clamp(max=ln)]                       # -1: not a valid row of this sequence
        badrow = ~zero & (i < 0)
        cnt["row"] += int(badrow.sum())
        ok = ~zero & (i >= 0)
        ii = i.clamp(min=0)
        col = torch.arange(V)
        own = ok & ((Lb[ii, col] > rb) | (Hb[ii, col] < rb))
        cnt["own"] += int(own.sum())
        ge = torch.from_numpy((Lb >= rb[None, :]).numpy().argmax(0))      # first valid row whose value is surely >= r
        has = (Lb >= rb[None, :]).any(0)
        cnt["first"] += int((ok & has & (ge < ii)).sum())
    if cnt["range"]:
        bad.append(f"keys: {cnt['range']} values outside [max L, max H]")
    if cnt["empty"]:
        bad.append(f"keys: {cnt['empty']} entries of value 0 are not 0x0000FFFF")
    if cnt["row"]:
        bad.append(f"keys: {cnt['row']} entries name a row that is masked or outside the sequence")
    if cnt["own"]:
        bad.append(f"keys: {cnt['own']} entries name a row whose logit is not the value")
    if cnt["first"]:
        bad.append(f"keys: {cnt['first']} entries name a row behind an earlier valid row with the same or a larger value")
    sr = _log1p_ratio(sparse.view(B, V), r)
    out = SimpleNamespace(checked=2 * B * V, sparse_ratio=float(sr.max()), tw_ratio=0.0,
                          amb_cols=n_amb / max(n_ent, 1), amb_toks=0.0)
    if not out.sparse_ratio <= 1.0:
        bad.append(f"sparse: log1p bound violated (or a zero / unwritten element), worst ratio {out.sparse_ratio:.3g}")
    if tw is not None:
        live = ref.live
        lo, hi = ref.L.max(1).values, ref.H.max(1).values
        out.amb_toks = float((lo != hi)[live].sum()) / max(int(live.sum()), 1)
        g = tw.detach().cpu().to(F64)
        dead_bad = int(((g != 0) | torch.isnan(g))[~live].sum())
        if dead_bad:
            bad.append(f"token_weights: {dead_bad} masked tokens are not exact zeros")
        out.checked += T
        if tkeys is not None:
            tk = _u32(tkeys)
            out.checked += T
            rt, ct = tk >> 16, 0xFFFF - (tk & 0xFFFF)
            n = int((tk[~live] != EMPTY_KEY).sum())
            if n:
                bad.append(f"token_keys: {n} masked tokens are not 0x0000FFFF")
            n = int((live & ((rt < lo) | (rt > hi))).sum())
            if n:
                bad.append(f"token_keys: {n} values outside [max L, max H]")
            zero = rt == 0
            n = int((live & zero & (tk != EMPTY_KEY)).sum())
            if n:
                bad.append(f"token_keys: {n} tokens of value 0 are not 0x0000FFFF")
            ok = live & ~zero
            n = int((ok & (ct >= V)).sum())
            if n:
                bad.append(f"token_keys: {n} tokens name a column outside the vocabulary")
            ok &= ct < V
            cc = ct.clamp(max=V - 1)
            t = torch.arange(T)
            n = int((ok & ((ref.L[t, cc] > rt) | (ref.H[t, cc] < rt))).sum())
            if n:
                bad.append(f"token_keys: {n} tokens name a column whose logit is not the value")
            gem = ref.L >= rt[:, None]
            ge = torch.from_numpy(gem.numpy().argmax(1))
            n = int((ok & gem.any(1) & (ge < cc)).sum())
            if n:
                bad.append(f"token_keys: {n} tokens name a column behind a lower column with the same or a larger value")
            twr = _log1p_ratio(g, torch.where(live, rt, torch.zeros_like(rt)))
            out.tw_ratio = float(twr.max())
        else:                                               # value bits unknown: log1p of [max L, max H], widened by the bound
            rlo = torch.where(live, lo, torch.zeros_like(lo))
            rhi = torch.where(live, hi, torch.zeros_like(hi))
            a, b_ = _log1p_ratio(g, rlo), _log1p_ratio(g, rhi)
            flo, fhi = torch.log1p(bits_value(rlo)), torch.log1p(bits_value(rhi))
            inside = (g >= flo) & (g <= fhi) & ((rhi > 0) | (g == 0))
            twr = torch.where(inside, torch.zeros_like(a), torch.minimum(a, b_))
            out.tw_ratio = float(twr.max())
        if not out.tw_ratio <= 1.0:
            bad.append(f"token_weights: log1p bound violated (or a zero / unwritten element), worst ratio {out.tw_ratio:.3g}")
    if ref.exact:
        if not torch.equal(kk, ref.keys):
            bad.append(f"keys: {int((kk != ref.keys).sum())} entries differ from the exact reference")
        if tkeys is not None and not torch.equal(_u32(tkeys), ref.tkeys):
            bad.append(f"token_keys: {int((_u32(tkeys) != ref.tkeys).sum())} entries differ from the exact reference")
    if out.amb_cols > AMBIGUOUS_CAP or out.amb_toks > AMBIGUOUS_CAP:
        bad.append(f"ambiguous share above the cap: columns {out.amb_cols:.3%}, tokens {out.amb_toks:.3%}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return out


# ----------------------------------------------------------------------------------------------- case builder
def _mask_of(spec, gen):
    """(kind, length[, valid]) -> mask [length].  kinds: ones, right (padding behind), left (padding in front), holes
    (valid rows scattered, first and last row masked where the length allows), mid (one valid row in the middle), none"""
    kind, ln = spec[0], spec[1]
    m = torch.zeros(ln, dtype=torch.int64)
    if kind == "ones":
        m[:] = 1
    elif kind == "right":
        m[:spec[2]] = 1
    elif kind == "left":
        m[ln - spec[2]:] = 1
    elif kind == "holes":
        n = spec[2]
        assert n + 2 <= ln
        m[1 + torch.randperm(ln - 2, generator=gen)[:n]] = 1
    elif kind == "mid":
        m[ln // 2] = 1
    elif kind != "none":
        raise ValueError(kind)
    return m


def _acc_std(K):
    return (K * (60.0 / 9.0) ** 2 / 256.0) ** 0.5          # h, 16 w uniform integers in [-4, 4]: variance 60 / 9 each


def _exact_bias(V, K, gen, allneg):
    std = _acc_std(K)
    cls = torch.rand(V, generator=gen)
    s = torch.randint(4, 8, (V,), generator=gen).to(F64)
    sign = torch.randint(0, 2, (V,), generator=gen).to(F64) * 2 - 1
    res = torch.randint(0, 2, (V,), generator=gen).to(F64) * 2 - 1
    tie = sign * 2.0 ** -s * (1.0 + res * 2.0 ** -9)        # bf16 -> +-2^-s; unrounded: just off the tie
    grid = torch.randint(-8, 9, (V,), generator=gen).to(F64) / 8.0
    rnd = torch.randn(V, generator=gen).to(F64) * 0.3
    midneg = -(1.5 * std) + rnd
    dead = -(float(K) + 8.0) + rnd
    b = torch.where(cls < 0.20, dead, torch.where(cls < 0.30, midneg, torch.where(cls < 0.45, grid,
                                                                                 torch.where(cls < 0.70, tie, rnd))))
    if allneg:
        b = -b.abs() - 2.0 ** -7
    return b


def build_case(name):
    """-> namespace of CPU tensors Hd, W, bias, cu (int32), mask (int64) + T, V, K, B, lens, nvalid, longest, spec, ref
    (forward_reference), stats (what the builder's conditions measured)"""
    return _build(name)


@functools.lru_cache(maxsize=None)
def _build(name):
    spec = CASES[name]
    gen = torch.Generator().manual_seed(spec.get("seed", 1) * 7919 + len(name))
    exact = spec["kind"] == "exact"
    V, K = spec["V"], spec["K"]
    masks = [_mask_of(s, gen) for s in spec["seqs"]]
    lens = [int(m.numel()) for m in masks]
    tail = spec.get("tail", 0)
    T = sum(lens) + tail
    mask = torch.cat(masks + [torch.zeros(tail, dtype=torch.int64)])
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    c = SimpleNamespace(name=name, spec=spec, T=T, V=V, K=K, B=len(lens), lens=lens, cu=cu, mask=mask,
                        nvalid=[int(m.sum()) for m in masks], longest=max(lens), exact=exact)
    if not exact:
        c.Hd = torch.randn(T, K, generator=gen).to(BF16)
        c.W = (torch.randn(V, K, generator=gen) * 0.05).to(BF16)
        c.bias = (torch.randn(V, generator=gen) * 0.3).to(torch.float32)
        c.ref = forward_reference(c.Hd, c.W, c.bias, cu, mask, exact=False)
        c.stats = {}
        return c
    allneg = spec.get("allneg", False)
    h = torch.randint(-4, 5, (T, K), generator=gen).to(F64)
    w = torch.randint(-4, 5, (V, K), generator=gen).to(F64) / 16.0
    b = _exact_bias(V, K, gen, allneg)
    # column V - 1: strong enough to be some token's arg-max (allneg: alive, just below zero; one column: 3 / 128 rounds
    # up between 4 and 8 where chopping rounds down)
    res = 1.0 + 2.0 ** -9
    b[V - 1] = -2.0 ** -7 * res if allneg else 3 * 2.0 ** -7 * res if V == 1 else float(int(2.5 * _acc_std(K)) + 1) + 2.0 ** -5 * res
    if allneg and T > 0:                                    # a zero row: x = bias < 0 in every column
        live_rows = torch.nonzero(mask).flatten()
        if live_rows.numel():
            h[live_rows[live_rows.numel() // 2]] = 0.0
    # ties between two columns: W rows (and bias) duplicated across the column seams and at random; V - 1 stays out
    pairs = [(d, d - 1) for d in (32, 96, 128, 192) if d < V - 1]
    free = torch.randperm(max(V - 1, 0), generator=gen).tolist()
    pairs += [(free[2 * i], free[2 * i + 1]) for i in range((V - 1) // 4)]
    for d, s in pairs:
        w[d], b[d] = w[s], b[s]
    # ties between two valid rows of a sequence: Hd rows duplicated across the sub-tile seams (list position) and the
    # chunk seams (sequence position), the copy behind (j <- j - 1) and before (j - 2 <- j + 1) the original, and at random
    s0 = 0
    for m, ln in zip(masks, lens):
        vp = torch.nonzero(m).flatten().tolist()
        n = len(vp)
        rp = []
        for j in (32, 64, 128, 256):
            if n > j:
                rp.append((vp[j], vp[j - 1]))
            if n > j + 1 and j >= 2:
                rp.append((vp[j - 2], vp[j + 1]))
            if j < ln and m[j] and m[j - 1]:
                rp.append((j, j - 1))
        if n >= 2:
            for _ in range(max(1, n // 3)):
                a, d = torch.randperm(n, generator=gen)[:2].tolist()
                rp.append((vp[d], vp[a]))
        for d, s in rp:                                     # (the last valid row stays single: the 256x192 form pads with it,
            if n < 3 or vp[-1] not in (d, s):               # and a padded copy that won a tie would show nowhere else)
                h[s0 + d] = h[s0 + s]
        s0 += ln
    mag = h.abs() @ w.abs().t()
    assert float(mag.max()) * 16.0 < 2.0 ** 24, "exactness precondition: sum |h||w| 2^4 < 2^24"
    assert (h == h.round()).all() and (w * 16 == (w * 16).round()).all() and h.abs().max() <= 4 and w.abs().max() <= 0.25
    c.Hd, c.W, c.bias = h.to(BF16), w.to(BF16), b.to(torch.float32)
    assert (c.Hd.to(F64) == h).all() and (c.W.to(F64) == w).all()
    c.ref = forward_reference(c.Hd, c.W, c.bias, cu, mask, exact=True)
    c.stats = _conditions(c)
    return c


def _conditions(c):
    """the builder's conditions (module docstring); `waive` names the ones the case's shape cannot meet"""
    ref, waive = c.ref, set(c.spec.get("waive", ()))
    vals = ref.keys >> 16
    st = {"zero": float((vals == 0).float().mean()), "positive": float((vals > 0).float().mean())}
    tied = pos = 0
    for b, (s0, ln, vp) in enumerate(ref.rows):
        if vp.numel() == 0:
            continue
        Lb = ref.L[s0 + vp]
        m = Lb.max(0).values
        tied += int(((Lb == m[None, :]).sum(0) >= 2)[m > 0].sum())
        pos += int((m > 0).sum())
    st["row_ties"] = tied / max(pos, 1)
    lv = ref.live
    m = ref.L.max(1).values
    st["col_ties"] = float((((ref.L == m[:, None]).sum(1) >= 2) & (m > 0))[lv].sum()) / max(int(lv.sum()), 1)
    st["rounding_ties"] = int(((ref.x32.contiguous().view(torch.int32) & 0xFFFF) == 0x8000).sum())
    st["dead_tokens"] = int((lv & (m == 0)).sum())
    need = {"zero": 0.10, "positive": 0.10, "row_ties": 0.05, "col_ties": 0.05, "rounding_ties": 1}
    for k, v in need.items():
        if k in waive:
            continue
        assert st[k] >= v, f"case {c.name}: builder condition {k} = {st[k]:.4g} < {v}"
    return st


# ----------------------------------------------------------------------------------------------- the case table
# seqs: (kind, length[, valid rows]) per sequence (_mask_of); tail: rows of the token buffer behind cu[B] (masked);
# msl: the max_seqlen values a GPU run is given (the 128x128 kernel takes 64-row chunks up to 64, 128-row chunks above);
# rec: False where V > 65535 (no token keys); split: first sequence of the second group of a two-call run; waive: builder
# conditions the shape cannot meet.  tests/test_gpu_splade_fwd_per_element.py says which seam each case is there for.
_S1 = [("holes", 40, 33)]
_S7 = [("ones", 33), ("none", 4), ("left", 20, 7), ("mid", 9), ("right", 66, 40), ("holes", 64, 20), ("ones", 1)]
_S9 = _S7 + [("none", 2), ("ones", 65)]
_NOROWS = ("zero", "positive", "row_ties", "col_ties", "rounding_ties")
CASES = {
    "counts": dict(kind="exact", V=385, K=128, tail=5, msl=(300, 400), seqs=[
        ("none", 5), ("mid", 7), ("right", 40, 31), ("ones", 32), ("holes", 50, 33), ("left", 70, 63), ("ones", 64),
        ("holes", 90, 65), ("none", 3), ("right", 130, 127), ("ones", 128), ("left", 140, 129), ("holes", 300, 257),
        ("ones", 300), ("none", 0), ("none", 9)]),
    "one_row_x20": dict(kind="exact", V=192, K=128, msl=(3, 65), seqs=[("mid", 3)] * 20, waive=("row_ties",)),
    "two_tiles": dict(kind="exact", V=3100, K=64, msl=(320,), seqs=[
        ("ones", 300), ("right", 310, 300), ("holes", 320, 300), ("left", 305, 300)] + [("ones", 300)] * 4),
    "no_valid": dict(kind="exact", V=200, K=64, msl=(40,), tail=2, seqs=[("none", 5), ("none", 40), ("none", 0)],
                     waive=_NOROWS),
    "nseq65": dict(kind="exact", V=129, K=64, msl=(5, 100), tail=1, seqs=[
        (("ones", 1), ("right", 2, 1), ("left", 3, 2), ("mid", 4), ("none", 5), ("ones", 5), ("holes", 5, 2))[i % 7]
        for i in range(65)]),
    # (one column and one sequence of 33 valid rows: its maximum is positive)
    "v1": dict(kind="exact", V=1, K=64, msl=(40, 128), seqs=_S1, waive=("col_ties", "row_ties", "zero")),
    "v95": dict(kind="exact", V=95, K=128, msl=(66,), seqs=_S7, allneg=True),
    "v96": dict(kind="exact", V=96, K=256, msl=(66,), seqs=_S9),
    "v97": dict(kind="exact", V=97, K=64, msl=(66,), tail=3, seqs=_S7),
    "v127": dict(kind="exact", V=127, K=128, msl=(40,), seqs=_S1, seed=2),
    "v128": dict(kind="exact", V=128, K=256, msl=(66,), seqs=_S9, allneg=True),
    "v191": dict(kind="exact", V=191, K=64, msl=(66,), seqs=_S7),
    "v193": dict(kind="exact", V=193, K=1152, msl=(66,), seqs=_S9),
    "v777": dict(kind="exact", V=777, K=768, msl=(66, 67), tail=3, seqs=_S7),
    "v65600": dict(kind="exact", V=65600, K=64, msl=(4,), rec=False, seqs=[("ones", 3), ("right", 4, 2)]),
    "groups": dict(kind="exact", V=200, K=256, msl=(140,), split=5, tail=2, seqs=[
        ("ones", 33), ("holes", 40, 20), ("none", 6), ("left", 30, 9), ("mid", 5),
        ("ones", 129), ("right", 140, 100), ("none", 10), ("holes", 70, 65)]),
    "gen64": dict(kind="generic", V=777, K=64, msl=(300,), tail=3, seqs=[
        ("holes", 300, 200), ("left", 129, 100), ("none", 7), ("mid", 9), ("right", 70, 33), ("ones", 65)]),
    "gen128": dict(kind="generic", V=777, K=128, msl=(300,), seqs=[
        ("left", 300, 257), ("holes", 129, 64), ("ones", 31), ("none", 7), ("holes", 70, 33)]),
    "gen256": dict(kind="generic", V=385, K=256, msl=(140,), tail=1, seqs=[
        ("holes", 140, 129), ("none", 3), ("right", 64, 63), ("left", 66, 65), ("mid", 5), ("ones", 32)]),
}

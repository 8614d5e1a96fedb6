"""Float64 restatement of the LayerNorm kernel family (csrc/elementwise.hip on csrc/rows.h: ln_fwd_kernel, ln_bwd_kernel,
ln_dw_reduce_kernel, the ordered embedding scatter), the case tables, a restatement of the backward's launch arithmetic,
and per-element acceptance SETS that follow from the kernels' cast points.  Plain numpy / torch on the CPU; sibling of
tests/gemm_reference.py, whose roundings, gelu table, guarded buffers and check it reuses.

Contracts (fl32 = one fp32 operation, bf16() = round to nearest even, H in {256, 512, 768, 1024}, LayerNorm without bias):
    LN(src)[j]        = fl32(fl32(c_j rstd) w_j), c_j = fl32(src_j - mean), mean = fl32(sum src / H),
                        var = fl32(sum c_j^2 / H), rstd = rsqrtf(fl32(var + eps))        (ln_normalize; eps as fp32)
    snx_ln_fwd        x = bf16(LN(h)), h fp32
    snx_ln_fwd_add    h_out = fl32(h + float(y)), y bf16: ONE value; x = bf16(LN(h_out))
    snx_embed_ln_fwd  h_out = LN(E[ids[t]]) stored as fp32; x0 = bf16(h_out): the bits of the stored value
    snx_gelu_ln_fwd   x = bf16(LN(G(d))), G(d) = bf16(gelu_f(d)), d bf16 (rbf(gelu_f) of csrc/common.h)
    backward          xhat_j = fl32(c_j rstd) as above; g_j = fl32(dy_j w_j); s1 = fl32(sum g / H);
                      s2 = fl32(sum g_j xhat_j / H); dx_j = fl32(rstd fl32(fl32(g_j - s1) - fl32(xhat_j s2)));
                      dw_j += sum_t dy_tj xhat_tj in fp32 (registers, 4 waves, one partial row per block, partial rows in
                      block order -- or one float atomic per block with "det_reduce" = 0)
    snx_ln_bwd        accumulate: dh = fl32(dh0 + dx); overwrite: dh = dx; dh_bf16 (optional) = bf16(dh as stored)
    snx_gelu_ln_bwd   dd = bf16(fl32(bf16(dx) gelu'(d))), gelu' = gelu_grad_f(d) in fp32
    snx_embed_ln_bwd  dy is the fp32 dh stream; gradE[id] += sum of dx[t] over the tokens with ids[t] = id, ascending t
                      (light ids: one sequential sum; more than 64 tokens: 32-token chunks, then the chunks in order; float
                      atomics with "det_reduce" = 0); the pad id takes no part; dw as above

Acceptance set, not a tolerance.  Per element the reference carries the float64 value v and a running bound B of
|computed - v|; an fp32 output passes iff v - B <= got <= v + B, a bf16 output iff bf16(v - B) <= got <= bf16(v + B).  B
is derived term by term from the source in the convention of gemm_reference and _tn_check (Higham, Accuracy and
Stability, 3.1 / 4.2): u = 2^-24, gamma_n = n u / (1 - n u), a sum of n operands in ANY order, fused or not, errs by at
most gamma_(n-1) sum|operand|.  A division is one rounding (snx/build.py sets no fast-math flag: hipcc's default is the
correctly rounded fp32 division).  Nothing below knows the lane layout or the butterfly:
    mean      Em = gamma_(H+1) sum|x| / H                     (H - 1 additions, one division, any order)
              If every partial sum of the row is exact in fp32 -- all elements multiples of one power of two g with
              sum|x| / g <= 2^24 -- the sum is exact in any order: Em = u |mean|, and 0 if sum / H is an fp32 value.
              (The constant row of 0.5 and the zero row: xhat = 0 exactly, the forward output is pinned to zero.)
    centring  c^ = (c - e)(1 + d), |e| <= Em: Ec_j = Em (1 + u) + u |c_j|
    squares   sum (c_j - e)^2 = sum c_j^2 + H e^2 because sum c_j = 0: the mean's error enters in second order only.
              Eq = H Em^2 + (gamma_H + 3u) sum (|c_j| + Em)^2  (2u + u^2 for the rounded c^, gamma_H for product + sum)
    division  Ev = Eq (1 + u) / H + u var
    var+eps   Ea = Ev (1 + u) + u (var + eps)
    rsqrt     a^-1/2 is convex and decreasing: Er = ((a - Ea)^-1/2 - a^-1/2) + RSQ 2u (a - Ea)^-1/2
              ASSUMPTION (RSQ): rsqrtf is accurate to ULP_RSQ = 1 ulp (<= 2u relative), of the same kind as RCP-EXP in
              gemm_reference.  Neither the guides nor the headers and documents of the ROCm installation state a figure
              for rsqrtf or v_rsq_f32: it is ASSUMED, not cited.  Nothing else about the hardware is assumed.
    xhat      Exh_j = Ec_j (r + Er) + |c_j| Er + u (|c_j| + Ec_j)(r + Er)
    weight    Ey_j = |w_j| (Exh_j + u (|xhat_j| + Exh_j))
    g, s1     g^ = g (1 + d);  E1 = gamma_(H+1) sum|g| / H      (product, H - 1 additions, division)
    s2        E2 = (sum |g_j| Exh_j + gamma_(H+2) sum |g_j| (|xhat_j| + Exh_j)) / H
    dx        z = g - s1 - xhat s2.  P = u |g| + E1 + |xhat| E2 + Exh (|s2| + E2) + u (|g| (1 + u) + |s1| + E1)
              + u (|xhat| + Exh)(|s2| + E2);  Ez = P + u (|z| + P);  Edx = Ez (r + Er) + |z| Er + u (|z| + Ez)(r + Er)
              (a contracted fma has one rounding fewer: covered)
    dh        accumulate: [fl32(dh0 + lo), fl32(dh0 + hi)] for the fp32 corners lo, hi of dx's interval: fl32 is
              monotone, corners suffice.  overwrite: dx's interval
    dd        bf16(fl32(b gelu')) at the corners of b in [bf16(dx - Edx), bf16(dx + Edx)] and gelu' in [d_lo, d_hi]
    dw        dw0 + sum_t dy xhat: T + 1 operands, each product rounded once: Edw = sum_t |dy| Exh + gamma_(T+1)
              (|dw0| + sum_t |dy| (|xhat| + Exh)) -- for the ordered reduce and for the atomics alike
    gradE     gE0 + sum of n rows: EgE = sum Edx + gamma_n (|gE0| + sum (|dx| + Edx)); n = 0: the initial bits
  Every B is multiplied by 1 + 2^-20 for the float64 evaluation of v and of B itself (n 2^-53 against gamma_n).  No
  constant was fitted to a kernel's output.

GELU modes.  gelu_f cannot be reproduced bit for bit on the CPU; gemm_reference.gelu_table() gives G(a) in [g_lo, g_hi] and
gelu' in [d_lo, d_hi].  The row statistics need ONE input: build_case replaces every drawn d whose table entry has
g_lo != g_hi by the nearest bf16 value with a single G and asserts that this touched at most 1 % of the elements; d is
clamped at -6 (gelu' stays a normal number).

Exact relations (bit equalities, tests/test_gpu_rows_per_element.py): h_out of the add mode; x0 == bf16(h_out);
dh_bf16 == bf16(dh as stored) in both modes; overwrite ignores the NaN sentinel dh held before; the pad row and every
gradE row whose id does not occur keep their initial bits (their set is that one value); dw and gradE start non-zero.

Input families, mixed row by row inside every tensor (row t is FAMILIES[t % 6]: random, small, const, spike, offset, zero):
  random  3 randn + 0.5        small  0.01 randn (variance ~ 10 eps: epsilon decides)      offset  OFFSET_MEAN + randn
  spike   1 + 0.25 randn with one element ~ 1e4       const  0.5 everywhere      zero  0 everywhere
weights with an exact zero, a quarter negative, magnitudes in [1/8, 2); upstream gradients of mixed sign (the column sums
of dw cancel).  All values keep clear of subnormals (asserted by bf16_round where a rounding is taken).

Launch arithmetic restated: ln_bwd_plan (ln_bwd_rows_per_block, block count, rows of the last block, workspace rows) and
reduce_split (ln_dw_reduce_kernel: per wave the 16-wide trips and the tail).  The case table asserts the class of every
large case through them; tests/test_rows_reference_host.py proves blocks <= workspace rows for T = 1..70,000.

Width of the sets, from the reference alone (tests/test_rows_reference_host.py asserts the floors 0.85 / 0.4): share of
the elements of bf16(LN(h)) with ONE admissible value at H = 256 / 512 / 768 / 1024, eps = 1e-5:
    family    256      512      768      1024        (two adjacent values: most of the rest; wider: at most 3.8 %)
    random    0.974    0.952    0.934    0.916
    small     0.973    0.954    0.935    0.916
    spike     0.991    0.981    0.973    0.961
    offset    0.928    0.874    0.830    0.786       (OFFSET_MEAN = 3; mean 8 would give 0.847 .. 0.593)
  B of the fp32 outputs stays below 2^-12 = 2.4e-4 of the row's largest magnitude: worst row of the 67-row cases, both
  eps, per width: h_out of the embedding forward 4.1e-5 / 6.8e-5 / 9.0e-5 / 1.2e-4, dx 4.5e-5 / 8.0e-5 / 1.3e-4 / 1.7e-4.

Measured on an MI355X with the kernels of commit 0431e50 (the change that adds this file touches no kernel), over all
cases of tests/test_gpu_rows_per_element.py: 74 tests, 9 s for the file, the slowest test 1.7 s (T = 8,193, H = 768).
Nothing fell outside its acceptance set at any width, mode or launch form, so ASSUMPTION (RSQ) was never what decided
an element: ULP_RSQ stays at its assumed value 1.  bf16 outputs: shares of elements with one / two adjacent / more
admissible values, all families mixed (every element that had one value met it bit for bit); fp32 outputs: the worst
|got - v| / B.  Small cases (T <= 67, both eps) at H = 256 / 512 / 768 / 1024:
    entry             output    one %                          two %                        worst |got - v| / B
    snx_ln_fwd        x         97.8   96.0   94.5   93.0      1.9    3.4    4.8    6.1
    snx_ln_fwd_add    x         97.8   95.3   92.9   90.9      1.9    4.2    6.2    8.0     h_out: one value, bit for bit
    snx_embed_ln_fwd  x0        97.6   96.0   93.7   92.5      2.2    3.5    5.4    6.4     h_out 0.024 0.013 0.009 0.008
    snx_gelu_ln_fwd   x         99.4   98.4   97.5   95.2      0.6    1.5    2.3    4.2
    snx_ln_bwd acc    dh_bf16   97.9   96.4   95.1   93.9      1.8    3.0    4.1    5.1     dw 0.252 0.201 0.164 0.390
    snx_ln_bwd ow     dh_bf16   93.8   89.4   85.4   82.1      5.2    8.8   11.8   14.1     dh, dw 0.252 0.201 0.164 0.390
    snx_gelu_ln_bwd   dd        94.8   91.1   87.6   84.0      4.2    7.1    9.6   12.1     dw 0.167 0.161 0.189 0.231
  Large cases (T, H): dh_bf16 overwrite / accumulate / dd one-value shares, worst |got - v| / B of the overwritten dh:
    (4096, 1024)  81.7 % / 92.3 % / 84.0 %, 0.023     (4101, 256)  93.4 % / 97.4 % / 94.8 %, 0.081
    (8193, 768)   85.5 % / 93.9 % / 87.6 %, 0.031     (dw at these T: below 0.001 of its bound, gamma_(T+1) is a worst case)
  snx_embed_ln_bwd (gradE and dw, fp32), worst |got - v| / B, the same with "det_reduce" 1 and 0:
    T = 1: 0.170 0.268 0.367 0.339     T = 131: 0.106 0.061 0.049 0.052     T = 4,101 at H = 512: 0.125
tests/test_rows_reference_host.py (37 tests, 13 s on the CPU): the fp32 emulations reach at most 0.46 of B.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests.gemm_reference import (BF16, GUARD_ROWS, U32, _corners, _raw, bf16_ord, bf16_round, check_guarded,  # noqa: F401
                                  check_guards, f32_down, f32_up, gelu_table, guarded, to_np, widths)

ULP_RSQ = 1                  # ASSUMPTION (RSQ), see the docstring
F64 = 1.0 + 2.0 ** -20
FAMILIES = ("random", "small", "const", "spike", "offset", "zero")   # five rows end on `offset`: a last row that counts in dw
OFFSET_MEAN = 3.0            # "a few standard deviations from zero"; the single-value floor of the host test holds at every width
WIDTHS = (256, 512, 768, 1024)
EPS = (1e-5, 1e-3)
V = 50
ROWS_PER_BLOCK = 4
EMBED_HEAVY = 64


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- launch arithmetic, restated
def ln_bwd_plan(T):
    """(rows per block, blocks, rows in the last block, workspace rows) of one LayerNorm backward over T rows"""
    rpb = cdiv(cdiv(T, 1024), ROWS_PER_BLOCK) * ROWS_PER_BLOCK
    rpb = max(rpb, ROWS_PER_BLOCK)
    blocks = cdiv(T, rpb)
    return rpb, blocks, T - (blocks - 1) * rpb, min(cdiv(T, ROWS_PER_BLOCK), 1024)


def reduce_split(blocks):
    """ln_dw_reduce_kernel: wave g of 16 sums partial rows [g nb / 16, (g + 1) nb / 16) -> [(first row, 16-wide trips, tail)]"""
    out = []
    for g in range(16):
        b0, b1 = g * blocks // 16, (g + 1) * blocks // 16
        out.append((b0, (b1 - b0) // 16, (b1 - b0) % 16))
    return out


def plan_classes(T):
    """the classes a case table asks for, read off ln_bwd_plan / reduce_split"""
    rpb, blocks, last, _ = ln_bwd_plan(T)
    cl = {f"trips {rpb // ROWS_PER_BLOCK}", f"fwd live waves {(T - 1) % ROWS_PER_BLOCK + 1}"}
    if last < ROWS_PER_BLOCK:
        cl.add("last block: fewer rows than waves")
    if ROWS_PER_BLOCK < last < 2 * ROWS_PER_BLOCK:
        cl.add("last block: partial second trip")
    for _, trips, tail in reduce_split(blocks):
        cl.add("reduce wave: no rows" if trips == 0 and tail == 0 else "reduce wave: tail only" if trips == 0 else
               "reduce wave: whole trips" if tail == 0 else "reduce wave: trips plus tail")
    return cl


# ----------------------------------------------------------------------------- the derivation
def exact_sum_rows(x):
    """rows of fp32 values all of whose partial sums, in any order, are exact in fp32: every element a multiple of one
    power of two g and sum|x| / g <= 2^24"""
    b = np.ascontiguousarray(x, dtype=np.float64).astype(np.float32).view(np.uint32)
    e = ((b >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    nz = (b & np.uint32(0x7FFFFFFF)) != 0
    assert bool(np.all(e[nz] > 0)), "subnormal input"
    m = ((b & np.uint32(0x7FFFFF)) | np.uint32(0x800000)).astype(np.int64)
    low = np.where(nz, e - 150 + np.log2((m & -m).astype(np.float64)).astype(np.int64), 10 ** 6)
    gexp = low.min(axis=-1)
    tot = np.abs(x).sum(axis=-1)
    return (gexp == 10 ** 6) | (tot <= np.ldexp(1.0, np.where(gexp == 10 ** 6, 0, gexp) + 24))


def ln_stats(x, eps, rsq=ULP_RSQ, exact=True):
    """x [T, H] float64 holding fp32 values -> xhat, rstd and their bounds (the module docstring, line by line).
    exact=False: without the exact-sum shortcut of the mean (rows that are not known to the bit: tests/f32_reference.py)"""
    u = U32
    H = x.shape[-1]
    eps = float(np.float32(eps))
    ax = np.abs(x).sum(-1)
    mean = x.sum(-1) / H
    exact = exact_sum_rows(x) if exact else np.zeros(x.shape[0], dtype=bool)
    Em = np.where(exact, np.where(mean.astype(np.float32).astype(np.float64) == mean, 0.0, u * np.abs(mean)), gamma(H + 1) * ax / H)
    c = x - mean[:, None]
    Em_ = Em[:, None]
    Ec = Em_ * (1 + u) + u * np.abs(c)
    var = (c * c).sum(-1) / H
    Eq = H * Em ** 2 + (gamma(H) + 3 * u) * ((np.abs(c) + Em_) ** 2).sum(-1)
    Ev = Eq * (1 + u) / H + u * var
    a = var + eps
    Ea = Ev * (1 + u) + u * a
    assert bool(np.all(a - Ea > 0))
    r = a ** -0.5
    r_hi = (a - Ea) ** -0.5
    Er = (r_hi - r) + rsq * 2 * u * r_hi
    rr = (r + Er)[:, None]
    xh = c * r[:, None]
    Exh = Ec * rr + np.abs(c) * Er[:, None] + u * (np.abs(c) + Ec) * rr
    return SimpleNamespace(xh=xh, Exh=Exh, r=r, Er=Er, mean=mean, var=var, Em=Em, c=c)


def ln_forward(x, w, eps, rsq=ULP_RSQ, exact=True):
    """-> (v, B) of LN(x) before the output cast, and the statistics"""
    st = ln_stats(x, eps, rsq, exact)
    aw = np.abs(w)[None, :]
    return st.xh * w[None, :], F64 * aw * (st.Exh + U32 * (np.abs(st.xh) + st.Exh)), st


def ln_backward(x, w, eps, dy, rsq=ULP_RSQ, exact=True):
    """-> dx, Edx [T, H] and the per-row terms of dw: p = dy xhat, Ep = |dy| Exh, Ap = |dy| (|xhat| + Exh)"""
    u = U32
    H = x.shape[-1]
    st = ln_stats(x, eps, rsq, exact)
    xh, Exh, axh = st.xh, st.Exh, np.abs(st.xh)
    g = dy * w[None, :]
    ag = np.abs(g)
    s1 = (g.sum(-1) / H)[:, None]
    E1 = (gamma(H + 1) * ag.sum(-1) / H)[:, None]
    s2 = ((g * xh).sum(-1) / H)[:, None]
    E2 = (((ag * Exh).sum(-1) + gamma(H + 2) * (ag * (axh + Exh)).sum(-1)) / H)[:, None]
    z = g - s1 - xh * s2
    P = (u * ag + E1 + axh * E2 + Exh * (np.abs(s2) + E2) + u * (ag * (1 + u) + np.abs(s1) + E1)
         + u * (axh + Exh) * (np.abs(s2) + E2))
    Ez = P + u * (np.abs(z) + P)
    r, Er = st.r[:, None], st.Er[:, None]
    dx = r * z
    Edx = F64 * (Ez * (r + Er) + np.abs(z) * Er + u * (np.abs(z) + Ez) * (r + Er))
    ady = np.abs(dy)
    return SimpleNamespace(dx=dx, Edx=Edx, p=dy * xh, Ep=ady * Exh, Ap=ady * (axh + Exh), st=st)


def dw_interval(dw0, bw):
    T = bw.p.shape[0]
    v = dw0 + bw.p.sum(0)
    B = F64 * (bw.Ep.sum(0) + gamma(T + 1) * (np.abs(dw0) + bw.Ap.sum(0)))
    return (v - B)[None, :], (v + B)[None, :]


def bf16_interval(v, B):
    return bf16_round(v - B), bf16_round(v + B)


def g_of(d):
    """the single admissible G(d) of bf16 values d (float64); asserts that the table entry IS single"""
    tab = gelu_table()
    o = bf16_ord(d) + 0x7F7F
    assert bool(np.all(tab.g_lo[o] == tab.g_hi[o])), "ambiguous G(d) in a case"
    return tab.g_lo[o]


# ----------------------------------------------------------------------------- cases
def family_rows(fam, n, H, g):
    if fam == "random":
        return 3.0 * torch.randn(n, H, generator=g) + 0.5
    if fam == "small":
        return 0.01 * torch.randn(n, H, generator=g)
    if fam == "offset":
        return OFFSET_MEAN + torch.randn(n, H, generator=g)
    if fam == "spike":
        r = 1.0 + 0.25 * torch.randn(n, H, generator=g)
        r[torch.arange(n), torch.randint(0, H, (n,), generator=g)] = 1e4 * (1.0 + 0.1 * torch.randn(n, generator=g))
        return r
    return torch.full((n, H), 0.5 if fam == "const" else 0.0)


def mixed_rows(T, H, g):
    """row t is of family FAMILIES[t % 6]: a one-row tensor is `random`, five rows hold every family but `zero` and end on `offset`"""
    out = torch.empty(T, H)
    for i, fam in enumerate(FAMILIES):
        if i < T:
            idx = torch.arange(i, T, len(FAMILIES))
            out[idx] = family_rows(fam, len(idx), H, g)
    return out


def weights(H, g):
    """an exact zero, a quarter negative, magnitudes over [1/8, 2)"""
    w = (0.5 + 0.5 * torch.rand(H, generator=g)) * 2.0 ** torch.randint(-2, 2, (H,), generator=g).float()
    w = torch.where(torch.rand(H, generator=g) < 0.25, -w, w)
    w[H // 3] = 0.0
    return w


def single_g(d):
    """bf16 tensor d -> (d with every element of ambiguous G(d) replaced by the nearest bf16 value of single G, share replaced)"""
    tab = gelu_table()
    single = tab.g_lo == tab.g_hi
    o = bf16_ord(to_np(d.clamp(min=-6.0))) + 0x7F7F
    bad = ~single[o]
    ob = o[bad]
    new, done = ob.copy(), np.zeros(ob.shape, dtype=bool)
    for k in range(1, 64):
        for s in (k, -k):
            cand = np.clip(ob + s, 0, len(single) - 1)
            fix = ~done & single[cand]
            new[fix] = cand[fix]
            done |= fix
    o2 = o.copy()
    o2[bad] = new
    assert bool(np.all(single[o2]))
    return torch.from_numpy(tab.x[o2]).to(BF16), float(bad.mean())


def ids_for(T, g, kind="fwd"):
    """fwd: contains 0, V - 1 and repeats (from two tokens on).  bwd131: T = 131 with id 3 on exactly 64 tokens (the last
    light size), id 7 on exactly 65 (the first heavy size), one pad token, one token of id 0, everything else never occurs.
    skew: id 5 on ~40 % of the rows, id 9 on ~3 %, the rest uniform over all ids (light ones, a few just past 64, pads)."""
    pad = V - 1
    if kind == "bwd131":
        assert T == 131
        ids = torch.tensor([3] * 64 + [7] * 65 + [pad, 0])
        return ids[torch.randperm(T, generator=g)]
    if kind == "skew":
        ids = torch.randint(0, V, (T,), generator=g)
        r = torch.rand(T, generator=g)
        ids[r < 0.4] = 5
        ids[(r >= 0.4) & (r < 0.43)] = 9
        return ids
    ids = torch.randint(0, V, (T,), generator=g)
    ids[0] = pad
    if T >= 2:
        ids[T // 2] = 0
    if T >= 4:
        ids[T - 1], ids[1] = 7, 7
    return ids


@functools.lru_cache(maxsize=3)
def build_case(T, H, eps=1e-5, ids_kind="fwd"):
    """every input of every entry point at one (T, H): h, y (bf16), d (bf16, single G), E, ids, w, dy (bf16), dyf, dh0,
    dw0, gE0.  Rows (and the rows of E) are the families in turn."""
    g = torch.Generator().manual_seed(1000003 * T + 1009 * H + {"fwd": 0, "bwd131": 1, "skew": 2}[ids_kind])
    h = mixed_rows(T, H, g)
    y = torch.randn(T, H, generator=g).to(BF16)
    d, replaced = single_g(mixed_rows(T, H, g).to(BF16))
    assert replaced <= 0.01, f"{replaced:.3%} of the drawn d replaced"
    E = mixed_rows(V, H, g)
    c = SimpleNamespace(T=T, H=H, eps=eps, V=V, pad=V - 1, h=h, y=y, d=d, E=E, ids=ids_for(T, g, ids_kind), w=weights(H, g),
                        dy=(0.1 * torch.randn(T, H, generator=g)).to(BF16), dyf=torch.randn(T, H, generator=g),
                        dh0=torch.randn(T, H, generator=g), dw0=0.5 * torch.randn(H, generator=g),
                        gE0=0.5 * torch.randn(V, H, generator=g), replaced=replaced)
    return c


def reversed_case(c):
    """the same launch with the rows reversed (E, w, dw0, gE0 stay)"""
    d = {k: v for k, v in vars(c).items() if k != "_bw"}
    for k in ("h", "y", "d", "ids", "dy", "dyf", "dh0"):
        d[k] = torch.flip(d[k], dims=(0,)).contiguous()
    return SimpleNamespace(**d)


# ----------------------------------------------------------------------------- expected sets per entry point
FWD_ENTRIES = ("ln_fwd", "ln_fwd_add", "embed_ln_fwd", "gelu_ln_fwd")
BWD_ENTRIES = ("ln_bwd_acc", "ln_bwd_acc_bf16", "ln_bwd_ow", "ln_bwd_ow_bf16", "gelu_ln_bwd", "embed_ln_bwd")


def source_rows(c, entry):
    """the fp32 rows the statistics are taken of, as float64"""
    if entry.startswith("ln_fwd_add"):
        return (c.h.numpy() + c.y.float().numpy()).astype(np.float64)          # fl32(h + float(y)): one value
    if entry.startswith("embed"):
        return to_np(c.E)[c.ids.numpy()]
    if entry.startswith("gelu"):
        return g_of(to_np(c.d))
    return to_np(c.h)


def expected_fwd(c, entry, rsq=ULP_RSQ):
    """{output name: (lo, hi)}"""
    x = source_rows(c, entry)
    v, B, _ = ln_forward(x, to_np(c.w), c.eps, rsq)
    if entry == "embed_ln_fwd":
        return {"h_out": (v - B, v + B), "x0": bf16_interval(v, B)}
    out = {"x": bf16_interval(v, B)}
    if entry == "ln_fwd_add":
        out["h_out"] = (x, x)
    return out


def _gradE_interval(c, bw):
    ids = c.ids.numpy()
    gE0 = to_np(c.gE0)
    lo, hi = gE0.copy(), gE0.copy()
    for v in np.unique(ids):
        if v == c.pad:
            continue
        rows = np.nonzero(ids == v)[0]
        s = gE0[v] + bw.dx[rows].sum(0)
        B = F64 * (bw.Edx[rows].sum(0) + gamma(len(rows)) * (np.abs(gE0[v]) + (np.abs(bw.dx[rows]) + bw.Edx[rows]).sum(0)))
        lo[v], hi[v] = s - B, s + B
    return lo, hi


def expected_bwd(c, entry, rsq=ULP_RSQ):
    """{output name: (lo, hi)}; dh_bf16 is the interval of bf16(dh) (the test also asks for the bits of the stored dh)"""
    src = "embed" if entry == "embed_ln_bwd" else "gelu" if entry == "gelu_ln_bwd" else "ln_fwd"
    memo = c.__dict__.setdefault("_bw", {})                      # the four snx_ln_bwd forms share one derivation
    if (src, rsq) not in memo:
        memo.clear()
        bw = ln_backward(source_rows(c, src), to_np(c.w), c.eps, to_np(c.dyf if src == "embed" else c.dy), rsq)
        memo[src, rsq] = SimpleNamespace(dx=bw.dx, Edx=bw.Edx, dw=dw_interval(to_np(c.dw0), bw))
    bw = memo[src, rsq]
    if entry == "embed_ln_bwd":
        return {"gradE": _gradE_interval(c, bw), "dw": bw.dw}
    out = {"dw": bw.dw}
    lo, hi = bw.dx - bw.Edx, bw.dx + bw.Edx
    if entry == "gelu_ln_bwd":
        tab = gelu_table()
        o = bf16_ord(to_np(c.d)) + 0x7F7F
        b = (bf16_round(lo), bf16_round(hi))
        out["dd"] = _corners(lambda bb, D: bf16_round((bb * D).astype(np.float32).astype(np.float64)), b, (tab.d_lo[o], tab.d_hi[o]))
        return out
    if entry.startswith("ln_bwd_acc"):
        dh0 = to_np(c.dh0)
        lo, hi = (dh0 + f32_up(lo)).astype(np.float32).astype(np.float64), (dh0 + f32_down(hi)).astype(np.float32).astype(np.float64)
    out["dh"] = (lo, hi)
    if entry.endswith("_bf16"):
        out["dh_bf16"] = (bf16_round(lo), bf16_round(hi))
    return out


def fp32_bound_ratio(c, entry):
    """max over the rows of B / (the row's largest magnitude) for the fp32 outputs h_out (embedding forward) and dh (overwrite)"""
    if entry == "embed_ln_fwd":
        v, B, _ = ln_forward(source_rows(c, entry), to_np(c.w), c.eps)
    else:
        bw = ln_backward(to_np(c.h), to_np(c.w), c.eps, to_np(c.dy))
        v, B = bw.dx, bw.Edx
    top = np.abs(v).max(-1)
    return np.where(top > 0, B.max(-1) / np.where(top > 0, top, 1.0), 0.0)


# ----------------------------------------------------------------------------- case tables
FWD_T = (1, 5, 6, 8, 67)     # last block with 1, 1, 2, 4 and 3 live waves (the issue's 1, 5, 67 and the two classes they miss)
BWD_T = (1, 5, 67)           # one block of one row; two blocks, the last with one row; 17 blocks, the last with three
# (T, H, classes plan_classes must report, (rows per block, blocks, rows in the last block))
BWD_LARGE = (
    (4096, 1024, ("trips 1", "reduce wave: whole trips"), (4, 1024, 4)),             # 1,024 blocks: the workspace ceiling
    (4101, 256, ("trips 2", "last block: partial second trip", "reduce wave: trips plus tail"), (8, 513, 5)),
    (8193, 768, ("trips 3", "reduce wave: trips plus tail"), (12, 683, 9)),
)
# snx_embed_ln_bwd: (T, H, ids kind).  T = 1; 131 tokens around the 64 / 65 light / heavy boundary with pads and ids that
# never occur, at every width; 4,101 rows with one id on ~40 % of them (a heavy id of ~1,640 tokens = 52 chunks) at one width
EMBED_BWD = tuple((1, H, "fwd") for H in WIDTHS) + tuple((131, H, "bwd131") for H in WIDTHS) + ((4101, 512, "skew"),)

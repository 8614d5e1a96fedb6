"""Float64 restatement of the routed SPLADE-head backward (snx_splade_bwd / snx_splade_bwd_tw, csrc/splade_head.hip),
with no autograd, an exact-coefficient input builder and a per-element check whose bounds are DERIVED.

The operation.  `keys[b, v] = bf16_bits(x) << 16 | (0xFFFF - row)` names, per (sequence, term), the bf16 logit x at the
arg-max row and that row (position inside the sequence).  With c[b, v] = bf16(g[b, v] / (1 + x)) for x > 0, else 0:
    dW[v, :]             = dW0[v, :] + sum_b c[b, v] Hd[cu[b] + row(b, v), :]
    db[v]                = db0[v]    + sum_b c[b, v]
    dHd[cu[b] + s, :]    = bf16( sum_{v: row(b, v) = s} c[b, v] W[v, :] )
The token direction (comment block above splade_tw_coef_kernel) adds, per token t with tkeys[t] = bf16_bits(x_t) << 16 |
(0xFFFF - v*), x_t > 0 and g_tw[t] != 0, the coefficient
    c_t = bf16((g_s + g_tw[t]) / (1 + x_t)) - bf16(g_s / (1 + x_t)),
g_s = g[seq(t), v*] where the sparse key of (seq(t), v*) routes to that very row, else 0.  c_t W[v*] joins the row's sum
of dHd before its single rounding; c_t Hd[t] and c_t join column v* of dW and db.

Why a per-element bound exists.  When every coefficient is an exact bf16 value (build_exact_g / build_exact_g_tw make
g = c* (1 + x) an exact fp32 product, so the quotient is c* whatever the division's last bits), every product c Hd and
c W is the product of two bf16 values: 16 significant bits, exact in fp32.  What is left is fp32 summation and, for dHd,
one rounding to bf16.  With u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, 4.2), for ANY
summation order -- sequential, tree, first-come buckets:
    dW, db:  |err| <= gamma_n magnitude,                       n = number of sequences + 8
    dHd:     |err| <= 2^-8 |ref| + 1.01 gamma_n magnitude,     n = entries of that row + 2
magnitude = |dW0| + sum |c| |Hd|  (|db0| + sum |c|;  sum |c| |W| for dHd).  For dW / db the + 8 covers the initial value,
the token-direction terms of that column (check_routed refuses a case with more than 6 of them in one column unless the
caller states that those sums are exact in fp32) and the shuffle tree of db.  For dHd the + 2 covers the token entry;
2^-8 |s| is half a bf16 ulp of the rounded fp32 sum s, and |s| <= |ref| + gamma_n magnitude gives the factor
1 + 2^-8 < 1.01.  Required exactly: rows without an entry are zeros (and written: the caller pre-fills dHd with NaN),
columns without an active entry keep dW0 / db0 bit for bit.  None of these numbers is tuned.
"""
from types import SimpleNamespace

import torch

U = 2.0 ** -24
BF16 = torch.bfloat16


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-24; n a number or a tensor"""
    return n * U / (1 - n * U)


def rbf64(a):
    """float64 -> nearest bf16 value (through fp32; for the exact inputs of the builder both steps are exact), as float64"""
    return a.to(torch.float32).to(BF16).to(torch.float64)


def decode_keys(keys):
    """packed int32 keys -> (value of the high 16 bits as bf16, float64; 0xFFFF - low 16 bits, int64)"""
    kk = keys.to(torch.int64) & 0xFFFFFFFF
    x = ((kk >> 16).to(torch.int32) << 16).view(torch.float32).to(torch.float64)
    return x, 0xFFFF - (kk & 0xFFFF)


def encode_keys(x, tag):
    """bf16-valued x >= 0 and a row (or column) index -> packed int32 keys"""
    bits = x.to(BF16).view(torch.int16).to(torch.int64) & 0xFFFF
    assert (x.to(BF16).to(torch.float64) == x.to(torch.float64)).all() and (x >= 0).all()
    k = (bits << 16) | (0xFFFF - tag.to(torch.int64))
    return torch.where(k >= 2 ** 31, k - 2 ** 32, k).to(torch.int32)


def _lens(cu):
    cu = cu.to(torch.int64)
    return cu, cu[1:] - cu[:-1]


def token_routing(g, keys, tkeys, cu):
    """Per token t: x_t, v*, its sequence and row, `live` (x_t > 0 and inside the packed buffer) and g_s (float64): the
    sparse gradient of (seq(t), v*) where that sparse key routes to row t, else 0."""
    cu, _ = _lens(cu)
    T, (B, V) = tkeys.numel(), g.shape
    xt, vt = decode_keys(tkeys)
    t = torch.arange(T)
    seq = (torch.searchsorted(cu, t, right=True) - 1).clamp(0, B - 1)
    live = (xt > 0) & (t < cu[-1])
    if (vt[live] >= V).any():
        raise ValueError("token key names a column outside the vocabulary")
    vs = torch.where(live, vt, torch.zeros_like(vt))
    xs, rs = decode_keys(keys)
    same = live & (rs[seq, vs] == t - cu[seq]) & (xs[seq, vs] > 0)
    if (xs[seq, vs][same] != xt[same]).any():
        raise ValueError("inconsistent keys: one logit with two values")
    gs = torch.where(same, g.to(torch.float64)[seq, vs], torch.zeros(T, dtype=torch.float64))
    return SimpleNamespace(x=xt, v=vs, seq=seq, live=live, same=same, gs=gs)


def splade_bwd_reference(g, keys, g_tw, tkeys, Hd, W, cu_seqlens, dW0, db0):
    """CPU tensors in, float64 out (g_tw = tkeys = None: the sparse direction alone).  Returns a namespace with
    dW, db, dHd (values), dW_mag, db_mag, dHd_mag (magnitudes), n_w (terms of a dW / db element: sequences + 8),
    dHd_n (terms of a dHd row: its entries + 2), row_entries [T], col_entries [V] (active entries, both directions),
    tok_col_entries [V] (token-direction entries of a column)."""
    cu, lens = _lens(cu_seqlens)
    B, V = g.shape
    T, H = Hd.shape
    f64 = torch.float64
    x, row = decode_keys(keys)
    c = torch.where(x > 0, rbf64(g.to(f64) / (1.0 + x)), torch.zeros((), dtype=f64))
    act = c != 0
    if (row[act] >= lens[:, None].expand(B, V)[act]).any():
        raise ValueError("an active key routes outside its own sequence")
    bi, vi = torch.nonzero(act, as_tuple=True)
    ti, ci = cu[bi] + row[bi, vi], c[bi, vi]
    tok_v = torch.zeros(0, dtype=torch.int64)
    if g_tw is not None:
        r = token_routing(g, keys, tkeys, cu)
        gt = g_tw.to(f64)
        ct = rbf64((r.gs + gt) / (1.0 + r.x)) - rbf64(r.gs / (1.0 + r.x))
        ct = torch.where(r.live & (gt != 0), ct, torch.zeros((), dtype=f64))
        tt = torch.nonzero(ct != 0, as_tuple=True)[0]
        tok_v = r.v[tt]
        ti, vi, ci = torch.cat([ti, tt]), torch.cat([vi, tok_v]), torch.cat([ci, ct[tt]])
    idx = torch.stack([ti, vi])
    A = torch.sparse_coo_tensor(idx, ci, (T, V)).coalesce()
    Aabs = torch.sparse_coo_tensor(idx, ci.abs(), (T, V)).coalesce()
    At, Aabst = A.t().coalesce(), Aabs.t().coalesce()
    Hd64, W64 = Hd.to(f64), W.to(f64)
    out = SimpleNamespace()
    out.dHd = torch.sparse.mm(A, W64)
    out.dHd_mag = torch.sparse.mm(Aabs, W64.abs())
    out.dW = dW0.to(f64) + torch.sparse.mm(At, Hd64)
    out.dW_mag = dW0.to(f64).abs() + torch.sparse.mm(Aabst, Hd64.abs())
    out.db = db0.to(f64) + torch.zeros(V, dtype=f64).index_add_(0, vi, ci)
    out.db_mag = db0.to(f64).abs() + torch.zeros(V, dtype=f64).index_add_(0, vi, ci.abs())
    out.row_entries = torch.bincount(ti, minlength=T)
    out.col_entries = torch.bincount(vi, minlength=V)
    out.tok_col_entries = torch.bincount(tok_v, minlength=V)
    out.n_w = B + 8
    out.dHd_n = out.row_entries + 2
    out.in_seq = torch.arange(T) < cu[-1]
    return out


def _ratio(err, bound):
    return torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))


def check_routed(dHd, dW, db, ref, dW0, db0, what="", token_sums_exact=False):
    """Per-element check of a backward's outputs against splade_bwd_reference (bounds: module docstring).  Returns the
    worst err / bound ratio per tensor; raises AssertionError naming every violated requirement with its worst ratio."""
    f64 = torch.float64
    if not token_sums_exact and int(ref.tok_col_entries.max()) > 6:
        raise ValueError("more than 6 token entries in a column: n = sequences + 8 does not cover them")
    dHd, dW, db = dHd.detach().cpu().to(f64), dW.detach().cpu().to(f64), db.detach().cpu().to(f64)
    dW0, db0 = dW0.detach().cpu().to(f64), db0.detach().cpu().to(f64)
    bad, ratios = [], {}
    rows = ref.in_seq
    nan_rows = int(torch.isnan(dHd[rows]).any(dim=1).sum())
    if nan_rows:
        bad.append(f"dHd: {nan_rows} rows not written (NaN)")
    empty = rows & (ref.row_entries == 0)
    nz = int((dHd[empty] != 0).any(dim=1).sum())          # NaN != 0 as well
    if nz:
        bad.append(f"dHd: {nz} rows without an entry are not exact zeros")
    b_h = 2.0 ** -8 * ref.dHd.abs() + 1.01 * gamma(ref.dHd_n.to(f64))[:, None] * ref.dHd_mag
    e_h = torch.nan_to_num((dHd - ref.dHd).abs(), nan=float("inf"))[rows]
    ratios["dHd"] = float(_ratio(e_h, b_h[rows]).max()) if e_h.numel() else 0.0
    idle = ref.col_entries == 0
    for name, got, init, val, mag in (("dW", dW, dW0, ref.dW, ref.dW_mag), ("db", db, db0, ref.db, ref.db_mag)):
        ch = int((got[idle] != init[idle]).sum())
        if ch:
            bad.append(f"{name}: {ch} elements of columns without an active entry differ from their initial values")
        e = torch.nan_to_num((got - val).abs(), nan=float("inf"))
        ratios[name] = float(_ratio(e, gamma(ref.n_w) * mag).max())
    for name, r in ratios.items():
        if not r <= 1.0:
            bad.append(f"{name}: bound violated, worst err / bound ratio {r:.3g}")
    msg = f"{what}: worst err / bound ratio " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items())
    assert not bad, msg + " -- " + "; ".join(bad)
    return ratios


# ----------------------------------------------------------------------------- exact-coefficient builder
def pick_x(shape, gen):
    """bf16 values in [2^-6, 16), as float64"""
    e = torch.randint(-6, 4, shape, generator=gen).to(torch.float64)
    m = torch.randint(0, 128, shape, generator=gen).to(torch.float64)
    return (1.0 + m / 128.0) * 2.0 ** e


def exact_coefs(shape, gen, emin=-3, emax=0):
    """+- (8..15) / 8 * 2^e, e in [emin, emax]: at most 4 significant bits, a small common exponent range (float64)"""
    m = torch.randint(8, 16, shape, generator=gen).to(torch.float64)
    e = torch.randint(emin, emax + 1, shape, generator=gen).to(torch.float64)
    s = torch.randint(0, 2, shape, generator=gen).to(torch.float64) * 2 - 1
    return s * m / 8.0 * 2.0 ** e


def build_exact_g(x, gen, zero_frac=0.1):
    """g (fp32) = c* (1 + x) for the decoded logits x (float64, bf16-valued): a fraction zero_frac of zeros, both signs;
    where x = 0, g is non-zero and the coefficient is 0 by definition.  Where the product has no exact fp32 form (x below
    about 2^-13, possible only for keys of a real forward) g = 0.  Returns (g, c) with c the exact coefficient (float64).
    Asserts in float64 that g IS the product, and that an fp32 quotient rounds to c*."""
    cs = exact_coefs(x.shape, gen)
    cs = torch.where(torch.rand(x.shape, generator=gen) < zero_frac, torch.zeros_like(cs), cs)
    p = cs * (1.0 + x)                                  # 4 x 24 bits at the most: exact in float64
    ok = (p.to(torch.float32).to(torch.float64) == p) & ((1.0 + x).to(torch.float32).to(torch.float64) == 1.0 + x)
    cs = torch.where(ok, cs, torch.zeros_like(cs))
    g = (cs * (1.0 + x)).to(torch.float32)
    assert (g.to(torch.float64) == cs * (1.0 + x)).all()
    q = g / (1.0 + x).to(torch.float32)
    assert (q.to(BF16).to(torch.float64) == cs).all()
    for ulps in (-3, 3):                                # a quotient a few fp32 ulps off rounds to c* as well
        assert ((q * (1.0 + ulps * 2.0 ** -23)).to(BF16).to(torch.float64) == cs).all()
    return g, torch.where(x > 0, cs, torch.zeros_like(cs))


def build_exact_g_tw(g, keys, tkeys, cu, gen, zero_frac=0.1):
    """g_tw (fp32) with g_s + g_tw = c2* (1 + x_t) exactly, in float64 AND as the fp32 sum the kernel forms; tokens whose
    sum has no exact form get 0; masked tokens (x_t = 0) get a non-zero g_tw that must contribute nothing."""
    r = token_routing(g, keys, tkeys, cu)
    c2 = exact_coefs(r.x.shape, gen)
    c2 = torch.where(torch.rand(r.x.shape, generator=gen) < zero_frac, torch.zeros_like(c2), c2)
    p2 = c2 * (1.0 + r.x)
    gt = p2 - r.gs                                      # both a few bits at nearby exponents: exact in float64
    gt32, gs32 = gt.to(torch.float32), r.gs.to(torch.float32)
    ok = (gt32.to(torch.float64) == gt) & ((gs32 + gt32).to(torch.float64) == p2) & (c2 != 0)
    g_tw = torch.where(ok, gt32, torch.zeros_like(gt32))
    g_tw = torch.where(r.live, g_tw, torch.ones_like(g_tw))
    chk = r.live & (g_tw != 0)
    assert ((gs32 + g_tw).to(torch.float64)[chk] == p2[chk]).all()
    q = (gs32 + g_tw) / (1.0 + r.x).to(torch.float32)
    assert (q.to(BF16).to(torch.float64)[chk] == c2[chk]).all()
    return g_tw


# ----------------------------------------------------------------------------- synthetic cases
def make_case(lens, V, H, seed, routing="random", tokens=None, coincide=0.3, hd_dyadic=False):
    """A synthetic backward problem with exact coefficients (CPU tensors in a namespace).  `routing`: one name, or one per
    sequence --
      random       rows drawn at random; a fifth of the terms inactive the way the forward writes them (value 0, row 0)
      one_row      every term of the sequence routed to one row
      round_robin  term v to row v % length
      counts       rows 0..3 get exactly 63, 64, 65 and 128 entries (columns scattered); every other term has x > 0, g = 0
      masked       key 0 exactly (value 0 at row 65,535; the forward writes 0x0000FFFF for a fully masked sequence, and the
                   backward must ignore any key of value 0), g != 0
      gzero        x > 0 everywhere, g = 0 everywhere
    Active keys carry only rows inside their own sequence.  `tokens`: None (no token direction), "spread" (token t takes
    column perm[t % V]: at most ceil(T / V) tokens per column; a fifth masked with 0xFFFF; in `random` sequences a
    fraction `coincide` of the tokens has the sparse key of its column routed to its own row) or "one_col" (every token
    takes one column).  hd_dyadic: Hd = k / 4, |k| <= 16, so that a column's token sum  sum_t c_t Hd[t]  (multiples of
    2^-8 below 8, a few thousand of them) is exact in fp32 in any order."""
    gen = torch.Generator().manual_seed(seed)
    lens = torch.as_tensor(lens, dtype=torch.int64)
    B, T = lens.numel(), int(lens.sum())
    cu = torch.zeros(B + 1, dtype=torch.int64)
    cu[1:] = lens.cumsum(0)
    routing = [routing] * B if isinstance(routing, str) else list(routing)
    assert len(routing) == B
    x = pick_x((B, V), gen)
    row = torch.zeros((B, V), dtype=torch.int64)
    gmask = torch.ones((B, V), dtype=torch.bool)
    gforce = torch.zeros((B, V), dtype=torch.bool)
    for b, kind in enumerate(routing):
        L = int(lens[b])
        if kind == "random":
            row[b] = torch.randint(0, L, (V,), generator=gen)
            off = torch.rand(V, generator=gen) < 0.2
            x[b, off], row[b, off] = 0.0, 0
        elif kind == "one_row":
            row[b] = int(torch.randint(0, L, (1,), generator=gen))
        elif kind == "round_robin":
            row[b] = torch.arange(V) % L
        elif kind == "counts":
            assert L >= 4 and V >= 320
            perm = torch.randperm(V, generator=gen)
            row[b] = torch.randint(0, 4, (V,), generator=gen)
            gmask[b] = False
            beg = 0
            for r, n in enumerate((63, 64, 65, 128)):
                row[b, perm[beg:beg + n]] = r
                gmask[b, perm[beg:beg + n]] = gforce[b, perm[beg:beg + n]] = True
                beg += n
        elif kind == "masked":
            x[b], row[b] = 0.0, 0xFFFF
        elif kind == "gzero":
            row[b] = torch.randint(0, L, (V,), generator=gen)
            gmask[b] = False
        else:
            raise ValueError(kind)
    tkeys = None
    if tokens is not None:
        t = torch.arange(T)
        seq = torch.searchsorted(cu, t, right=True) - 1
        pos = t - cu[seq]
        if tokens == "one_col":
            vt = torch.full((T,), int(torch.randint(0, V, (1,), generator=gen)))
        else:
            vt = torch.randperm(V, generator=gen)[t % V]
            force = (torch.rand(T, generator=gen) < coincide) & torch.tensor([routing[int(s)] == "random" for s in seq])
            for i in torch.nonzero(force).flatten().tolist():
                b, v = int(seq[i]), int(vt[i])
                row[b, v] = pos[i]
                if x[b, v] == 0:
                    x[b, v] = pick_x((1,), gen)[0]
        xt = pick_x((T,), gen)
        same = (row[seq, vt] == pos) & (x[seq, vt] > 0)
        xt = torch.where(same, x[seq, vt], xt)
        if tokens != "one_col":
            xt = torch.where(torch.rand(T, generator=gen) < 0.2, torch.zeros_like(xt), xt)
        tkeys = torch.where(xt > 0, encode_keys(xt, vt), torch.full((T,), 0xFFFF, dtype=torch.int32))
    keys = encode_keys(x, row)
    g, _ = build_exact_g(x, gen)
    g = torch.where(gforce & (g == 0), (1.0 + x).to(torch.float32), g)   # c* = 1: the counted entries are all active
    g = torch.where(gmask, g, torch.zeros_like(g))
    g_tw = build_exact_g_tw(g, keys, tkeys, cu, gen) if tokens is not None else None
    if hd_dyadic:
        Hd = (torch.randint(-16, 17, (T, H), generator=gen).to(torch.float32) / 4).to(BF16)
    else:
        Hd = torch.randn(T, H, generator=gen).to(BF16)
    W = (torch.randn(V, H, generator=gen) * 0.05).to(BF16)
    return SimpleNamespace(lens=lens, cu=cu.to(torch.int32), B=B, T=T, V=V, H=H, max_len=int(lens.max()), g=g, keys=keys,
                           g_tw=g_tw, tkeys=tkeys, Hd=Hd, W=W, dW0=torch.randn(V, H, generator=gen),
                           db0=torch.randn(V, generator=gen))


def reference_of(case):
    return splade_bwd_reference(case.g, case.keys, case.g_tw, case.tkeys, case.Hd, case.W, case.cu, case.dW0, case.db0)

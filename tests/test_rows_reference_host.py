"""Host-side proof of tests/rows_reference.py (no GPU): the reference admits what the LayerNorm kernels' cast points can
produce and rejects what they cannot.

a. Conformance.  emulate() restates every entry point in numpy float32 in three summation orders -- sequential, pairwise
   and the kernel's own (groups of four per lane, NV vectors per lane, the 64-lane xor butterfly; the multiply-adds of the
   in-lane loops contracted to fmas; dw through the blocks, waves and the 16-way reduce of ln_bwd_plan / reduce_split;
   gradE through the light walk and the heavy 32-token chunks) -- with rsqrt correctly rounded and moved by -1, 0, +1
   ulp.  Every result must lie inside its acceptance set for every family (each case mixes all six) at every width, and
   the worst |got - ref| / B per entry point, printed, is <= 1.  torch's CPU fp32 layer_norm, forward and autograd backward
   (Welford moments, its own order), must lie inside as an implementation nobody here wrote.
b. Planted faults.  FAULTS names, per fault, the entry point, the output and the case (the smallest of the GPU table that
   can show it: T = 5 rows of the families random, small, const, spike, offset; T = 131 for the 64 / 65 boundary).  One
   element outside its set is a rejection.  Which family exposes which fault: the `rows` column -- `small` (variance
   ~ 10 eps) is the only family that sees a dropped, misplaced or changed eps; every family but zero sees the H - 1
   divisor; the weight shift, truncation, neighbour statistics and the backward faults show on `random` alone already.
c. The conditions that keep a set from hiding a failure: single-value shares per family and width, B of the fp32
   outputs below 2^-12 of the row's largest magnitude.
d. The launch arithmetic: ln_bwd_plan against snx_ln_bwd_workspace_bytes (a host function), blocks <= workspace rows and
   a monotone workspace for T = 1..70,000, the 16-way split dealing every partial row once, and the case tables reaching
   every class.
"""
import numpy as np
import pytest
import torch

from tests import rows_reference as R
from tests.gemm_reference import gelu_emul

f32 = np.float32
ORDERS = ("seq", "pair", "kernel")


# ----------------------------------------------------------------------------- fp32 sums in three orders
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _seq(t):
    return np.cumsum(t, axis=-1, dtype=f32)[..., -1]


def _pair(t):
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = np.concatenate([t[..., :-2], (t[..., -2:-1] + t[..., -1:]).astype(f32)], axis=-1)
        else:
            t = (t[..., ::2] + t[..., 1::2]).astype(f32)
    return t[..., 0]


def _butterfly(v):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., idx ^ o]).astype(f32)
    return v[..., 0]


def _lanes(a):
    """[..., H] -> [..., 64, NV, 4]: what lane l holds, vector by vector (rows.h: element (i * 64 + l) * 4 + e)"""
    return np.swapaxes(a.reshape(*a.shape[:-1], a.shape[-1] // 256, 64, 4), -3, -2)


def row_sum(a, order):
    """RowVec::sum"""
    if order == "seq":
        return _seq(a)
    if order == "pair":
        return _pair(a)
    v = _lanes(a)
    q = ((v[..., 0] + v[..., 1]).astype(f32) + (v[..., 2] + v[..., 3]).astype(f32)).astype(f32)      # [..., 64, NV]
    return _butterfly(_seq(q))


def row_dot(a, b, order):
    """sum a_j b_j as the in-lane loops of ln_normalize / ln_bwd_kernel form it (b None: sum a_j)"""
    if order != "kernel":
        t = a if b is None else (a * b).astype(f32)
        return _seq(t) if order == "seq" else _pair(t)
    va = _lanes(a).reshape(*a.shape[:-1], 64, -1)
    vb = None if b is None else _lanes(b).reshape(*a.shape[:-1], 64, -1)
    s = np.zeros(va.shape[:-1], f32)
    for k in range(va.shape[-1]):
        s = (s + va[..., k]).astype(f32) if vb is None else _fma(va[..., k], vb[..., k], s)
    return _butterfly(s)


def _bump(v, d):
    for _ in range(abs(d)):
        v = np.nextafter(v, f32(np.inf) if d > 0 else f32(-np.inf))
    return v


def _bf16(a):
    """fp32 -> bf16 by torch's own cast (independent of bf16_round), as float64"""
    return R.to_np(torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(R.BF16))


def _trunc(a):
    return (np.ascontiguousarray(a, dtype=f32).view(np.uint32) & np.uint32(0xFFFF0000)).view(f32).astype(np.float64)


# ----------------------------------------------------------------------------- the emulation
def emu_normalize(x, eps, order, bump=0, fault=None):
    H = x.shape[-1]
    eps32 = f32(eps * 0.1) if fault == "other_eps" else f32(eps)
    mean = (row_sum(x, order) / f32(H)).astype(f32)
    c = (x - mean[:, None]).astype(f32)
    var = (row_dot(c, c, order) / f32(H - 1 if fault == "var_hm1" else H)).astype(f32)
    a = var if fault in ("no_eps", "eps_after_sqrt") else (var + eps32).astype(f32)
    with np.errstate(divide="ignore"):
        if fault == "eps_after_sqrt":
            r = (f32(1) / (np.sqrt(a.astype(np.float64)).astype(f32) + eps32)).astype(f32)
        else:
            r = _bump((1.0 / np.sqrt(a.astype(np.float64))).astype(f32), bump)
    if fault == "neighbour_stats" and len(x) > 1:
        swap = np.arange(len(x)) ^ 1
        swap[swap >= len(x)] = len(x) - 1
        c, r = (x - mean[swap][:, None]).astype(f32), r[swap]
    with np.errstate(invalid="ignore"):
        xh = np.nan_to_num((c * r[:, None]).astype(f32), nan=0.0, posinf=3e38, neginf=-3e38)
    return xh, r


def _inputs(c, entry):
    if entry.startswith("ln_fwd_add"):
        return (c.h.numpy() + c.y.float().numpy()).astype(f32)
    if entry.startswith("embed"):
        return c.E.numpy()[c.ids.numpy()]
    if entry.startswith("gelu"):
        return R.g_of(R.to_np(c.d)).astype(f32)
    return c.h.numpy()


def emulate_fwd(c, entry, order, bump=0, fault=None):
    """-> ({output name: values as float64}, y before the output cast)"""
    x = _inputs(c, entry)
    w = c.w.numpy()
    xh, _ = emu_normalize(x, c.eps, order, bump, fault)
    y = (xh * (np.roll(w, 4) if fault == "weight_shift" else w)[None, :]).astype(f32)
    cast = _trunc if fault == "truncate" else _bf16
    if entry == "embed_ln_fwd":
        return {"h_out": y.astype(np.float64), "x0": cast(xh if fault == "x0_before_weight" else y)}, y
    out = {"x": cast(y)}
    if entry == "ln_fwd_add":
        out["h_out"] = (c.h.numpy() if fault == "hout_is_h" else x).astype(np.float64)
    return out, y


def emu_dw(dy, xh, dw0, order, fault=None):
    T, H = dy.shape
    rpb, blocks, _, _ = R.ln_bwd_plan(T)
    if order != "kernel":                                       # the rows a faulty launch would add, in this order's sum
        rows = list(range(T)) + ([T - 1] if fault == "rows_past_T" else [])
        if fault == "dw_last_block":
            rows = [t for t in rows if t // rpb != blocks - 1]
        if fault == "dw_one_wave":
            b0, trips, tail = R.reduce_split(blocks)[7]
            rows = [t for t in rows if not b0 <= t // rpb < b0 + 16 * trips + tail]
        if order == "pair":
            return (dw0 + _pair(np.ascontiguousarray((dy[rows] * xh[rows]).astype(f32).T))).astype(f32)
        acc = dw0.copy()
        for t in rows:
            acc = (acc + (dy[t] * xh[t]).astype(f32)).astype(f32)
        return acc
    part = np.zeros((blocks, H), f32)
    for b in range(blocks):
        end = min(T, (b + 1) * rpb) + (1 if fault == "rows_past_T" and b == blocks - 1 else 0)
        acc = np.zeros((R.ROWS_PER_BLOCK, H), f32)
        for wave in range(R.ROWS_PER_BLOCK):
            for t in range(b * rpb + wave, end, R.ROWS_PER_BLOCK):
                tt = min(t, T - 1)                               # the planted row past T re-reads the last row's data
                acc[wave] = _fma(dy[tt], xh[tt], acc[wave])
        part[b] = ((acc[0] + acc[1]).astype(f32) + (acc[2] + acc[3]).astype(f32)).astype(f32)
    if fault == "dw_last_block":
        part[blocks - 1] = 0
    tot = None
    for g, (b0, trips, tail) in enumerate(R.reduce_split(blocks)):
        s = np.zeros(H, f32)
        for b in range(b0, b0 + 16 * trips + tail):
            s = (s + part[b]).astype(f32)
        if fault == "dw_one_wave" and g == 7:
            s[:] = 0
        tot = s if tot is None else (tot + s).astype(f32)
    return (dw0 + tot).astype(f32)


def emu_gradE(c, dx, order, fault=None):
    ids = c.ids.numpy()
    gE = c.gE0.numpy().copy()
    for v in np.unique(ids):
        if v == c.pad and fault != "pad_gets_grad":
            continue
        rows = np.nonzero(ids == v)[0]
        if fault == "token_dropped" and len(rows) >= R.EMBED_HEAVY:
            rows = rows[:-1]
        if order == "pair":
            gE[v] = (gE[v] + _pair(np.ascontiguousarray(dx[rows].T))).astype(f32)
            continue
        acc = gE[v].copy()
        if order == "seq" or len(rows) <= R.EMBED_HEAVY:
            for t in rows:
                acc = (acc + dx[t]).astype(f32)
        else:
            for k in range(0, len(rows), 32):
                p = np.zeros_like(acc)
                for t in rows[k:k + 32]:
                    p = (p + dx[t]).astype(f32)
                acc = (acc + p).astype(f32)
        gE[v] = acc
    return gE.astype(np.float64)


def emulate_bwd(c, entry, order, bump=0, fault=None):
    """-> ({output name: values as float64}, dx in fp32)"""
    embed, gelu = entry == "embed_ln_bwd", entry == "gelu_ln_bwd"
    x = _inputs(c, "embed" if embed else "gelu" if gelu else "ln_fwd")
    w, H = c.w.numpy(), c.H
    dy = c.dyf.numpy() if embed else c.dy.float().numpy()
    xh, r = emu_normalize(x, c.eps, order, bump)
    g = (dy * w[None, :]).astype(f32)
    s1 = (row_dot(g, None, order) / f32(H)).astype(f32)
    if fault == "no_mean_g":
        s1 = np.zeros_like(s1)
    s2 = (row_dot(dy if fault == "s2_from_dy" else g, xh, order) / f32(H)).astype(f32)
    if order == "kernel":                                       # contracted: fma(-xhat, s2, g - s1)
        z = _fma(-xh, np.broadcast_to(s2[:, None], xh.shape), (g - s1[:, None]).astype(f32))
    else:
        z = ((g - s1[:, None]).astype(f32) - (xh * s2[:, None]).astype(f32)).astype(f32)
    dx = (r[:, None] * z).astype(f32)
    out = {"dw": emu_dw(g if fault == "dw_from_g" else dy, xh, c.dw0.numpy(), order, fault)[None, :].astype(np.float64)}
    if embed:
        out["gradE"] = emu_gradE(c, dx, order, fault)
    elif gelu:
        out["dd"] = _bf16((_bf16(dx).astype(f32) * gelu_emul(R.to_np(c.d))[1].astype(f32)).astype(f32))
    else:
        acc = entry.startswith("ln_bwd_acc") != (fault == "acc_ow_swapped")
        dh = (c.dh0.numpy() + dx).astype(f32) if acc else dx
        out["dh"] = dh.astype(np.float64)
        if entry.endswith("_bf16"):
            out["dh_bf16"] = _bf16(dx if fault == "dhbf16_from_dx" else dh)
    return out, dx


def n_outside(got, iv):
    return int((~((got >= iv[0]) & (got <= iv[1]))).sum())


def _ratio(got, v, B):
    err = np.abs(got.astype(np.float64) - v)
    assert bool(np.all(err[B == 0] == 0))
    return float((err[B > 0] / B[B > 0]).max(initial=0.0))


# ----------------------------------------------------------------------------- a. conformance
@pytest.mark.parametrize("H", R.WIDTHS)
def test_emulations_lie_inside_their_sets(H):
    worst = {}
    for T, eps, kind in ((67, 1e-5, "fwd"), (5, 1e-3, "fwd"), (131, 1e-5, "bwd131")):
        c = R.build_case(T, H, eps, kind)
        w = R.to_np(c.w)
        for order in ORDERS:
            for bump in (-1, 0, 1):
                for e in R.FWD_ENTRIES:
                    got, y = emulate_fwd(c, e, order, bump)
                    exp = R.expected_fwd(c, e)
                    assert set(got) == set(exp)
                    for k in got:
                        assert n_outside(got[k], exp[k]) == 0, (T, eps, order, bump, e, k)
                    v, B, _ = R.ln_forward(R.source_rows(c, e), w, eps)
                    worst[e] = max(worst.get(e, 0.0), _ratio(y, v, B))
                for e in R.BWD_ENTRIES:
                    got, dx = emulate_bwd(c, e, order, bump)
                    exp = R.expected_bwd(c, e)
                    assert set(got) == set(exp)
                    for k in got:
                        assert n_outside(got[k], exp[k]) == 0, (T, eps, order, bump, e, k)
                    src = "embed" if e == "embed_ln_bwd" else "gelu" if e == "gelu_ln_bwd" else "ln_fwd"
                    bw = R.ln_backward(R.source_rows(c, src), w, eps, R.to_np(c.dyf if src == "embed" else c.dy))
                    worst[e] = max(worst.get(e, 0.0), _ratio(dx, bw.dx, bw.Edx))
                    lo, hi = exp["dw"]
                    worst[e + " dw"] = max(worst.get(e + " dw", 0.0), _ratio(got["dw"], (lo + hi) / 2, (hi - lo) / 2 * (1 + 1e-9) + 1e-300))
    for k, v in sorted(worst.items()):
        print(f"H {H} {k}: worst |got - ref| / B = {v:.3f}")
        assert v <= 1.0


@pytest.mark.parametrize("H", R.WIDTHS)
def test_torch_cpu_layer_norm_lies_inside(H):
    """an independent fp32 implementation: forward, autograd backward, embedding backward with padding_idx"""
    F = torch.nn.functional
    for T, kind in ((67, "fwd"), (131, "bwd131")):
        c = R.build_case(T, H, 1e-5, kind)
        hl, wl = c.h.clone().requires_grad_(True), c.w.clone().requires_grad_(True)
        y = F.layer_norm(hl, (H,), wl, None, c.eps)
        v, B, _ = R.ln_forward(R.to_np(c.h), R.to_np(c.w), c.eps)
        assert n_outside(R.to_np(y), (v - B, v + B)) == 0
        assert n_outside(R.to_np(y.detach().to(R.BF16)), R.expected_fwd(c, "ln_fwd")["x"]) == 0
        y.backward(c.dy.float())
        exp = R.expected_bwd(c, "ln_bwd_ow_bf16")
        assert n_outside(R.to_np(hl.grad), exp["dh"]) == 0
        assert n_outside(R.to_np(hl.grad.to(R.BF16)), exp["dh_bf16"]) == 0
        assert n_outside(R.to_np(c.dh0 + hl.grad), R.expected_bwd(c, "ln_bwd_acc")["dh"]) == 0
        assert n_outside(R.to_np(c.dw0 + wl.grad)[None, :], exp["dw"]) == 0
        El, wl = c.E.clone().requires_grad_(True), c.w.clone().requires_grad_(True)
        F.layer_norm(F.embedding(c.ids, El, padding_idx=c.pad), (H,), wl, None, c.eps).backward(c.dyf)
        exp = R.expected_bwd(c, "embed_ln_bwd")
        assert n_outside(R.to_np(c.gE0 + El.grad), exp["gradE"]) == 0
        assert n_outside(R.to_np(c.dw0 + wl.grad)[None, :], exp["dw"]) == 0


# ----------------------------------------------------------------------------- b. planted faults
# fault: (entry, output, (T, ids kind), rows whose families must expose it -- None: any element anywhere)
SMALL, RANDOM = (1,), (0,)
FAULTS = {
    "var_hm1": ("ln_fwd", "x", (5, "fwd"), (0, 1, 3, 4)),                 # every family with a variance
    "no_eps": ("ln_fwd", "x", (5, "fwd"), SMALL),
    "eps_after_sqrt": ("ln_fwd", "x", (5, "fwd"), SMALL),
    "other_eps": ("ln_fwd", "x", (5, "fwd"), SMALL),
    "weight_shift": ("ln_fwd", "x", (5, "fwd"), RANDOM),
    "truncate": ("ln_fwd", "x", (5, "fwd"), RANDOM),
    "neighbour_stats": ("ln_fwd", "x", (5, "fwd"), RANDOM),
    "hout_is_h": ("ln_fwd_add", "h_out", (1, "fwd"), RANDOM),
    "x0_before_weight": ("embed_ln_fwd", "x0", (1, "fwd"), None),
    "no_mean_g": ("ln_bwd_ow", "dh", (1, "fwd"), RANDOM),
    "s2_from_dy": ("ln_bwd_ow", "dh", (1, "fwd"), RANDOM),
    "dw_from_g": ("ln_bwd_ow", "dw", (1, "fwd"), None),
    "dw_last_block": ("ln_bwd_ow", "dw", (5, "fwd"), None),               # two blocks, the last holds row 4 (offset) alone
    "dw_one_wave": ("gelu_ln_bwd", "dw", (5, "fwd"), None),               # reduce wave 7 owns partial row 0
    "rows_past_T": ("ln_bwd_acc", "dw", (5, "fwd"), None),
    "acc_ow_swapped": ("ln_bwd_acc", "dh", (1, "fwd"), RANDOM),
    "dhbf16_from_dx": ("ln_bwd_acc_bf16", "dh_bf16", (1, "fwd"), RANDOM),
    "pad_gets_grad": ("embed_ln_bwd", "gradE", (131, "bwd131"), None),
    "token_dropped": ("embed_ln_bwd", "gradE", (131, "bwd131"), None),    # ids 3 (64 tokens, light) and 7 (65, heavy)
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_rejected(fault):
    entry, name, (T, kind), rows = FAULTS[fault]
    c = R.build_case(T, 256, 1e-5, kind)
    fwd = entry in R.FWD_ENTRIES
    exp = (R.expected_fwd if fwd else R.expected_bwd)(c, entry)[name]
    for order in ORDERS:
        clean = (emulate_fwd if fwd else emulate_bwd)(c, entry, order)[0][name]
        assert n_outside(clean, exp) == 0
        got = (emulate_fwd if fwd else emulate_bwd)(c, entry, order, fault=fault)[0][name]
        bad = ~((got >= exp[0]) & (got <= exp[1]))
        assert bad.any(), f"{fault} ({order}) passes"
        for r in rows or ():
            if r < T:
                assert bad[r].any(), f"{fault} ({order}): row {r} ({R.FAMILIES[r]}) does not expose it"
        if fault == "token_dropped":
            assert bad[3].any() and bad[7].any()                          # on both sides of the light / heavy boundary
        if fault == "pad_gets_grad":
            assert bad[c.pad].any() and not np.delete(bad, c.pad, axis=0).any()


def test_second_eps_is_told_apart_only_by_small_rows():
    """what the families are there for: eps / 10 moves rstd of a `random` row by 5e-8 (inside its set) and of a `small`
    row by 4 % (outside)"""
    c = R.build_case(5, 256, 1e-5)
    exp = R.expected_fwd(c, "ln_fwd")["x"]
    got = emulate_fwd(c, "ln_fwd", "kernel", fault="other_eps")[0]["x"]
    bad = ~((got >= exp[0]) & (got <= exp[1]))
    assert not bad[0].any() and bad[1].mean() > 0.5


# ----------------------------------------------------------------------------- c. the sets are narrow
@pytest.mark.parametrize("H", R.WIDTHS)
def test_sets_are_narrow(H):
    g = torch.Generator().manual_seed(H)
    w = R.to_np(R.weights(H, g))
    for eps in R.EPS:
        for fam, floor in (("random", 0.85), ("small", 0.85), ("spike", 0.85), ("offset", 0.4)):
            x = R.to_np(R.family_rows(fam, 96, H, g))
            v, B, _ = R.ln_forward(x, w, eps)
            n = R.widths(*R.bf16_interval(v, B))
            one, two = float((n == 1).mean()), float((n == 2).mean())
            print(f"H {H} eps {eps} {fam}: one {one:.3f} two {two:.3f} wider {1 - one - two:.4f}")
            assert one >= floor
            assert float((B.max(-1) / np.abs(v).max(-1)).max()) < 2.0 ** -12
    for T in (67,):
        c = R.build_case(T, H)
        for e in ("embed_ln_fwd", "ln_bwd_ow"):
            assert float(R.fp32_bound_ratio(c, e).max()) < 2.0 ** -12, e
    # the constant and the zero row: pinned to zero, no assumption (the RSQ constant does not enter)
    x = np.stack([np.full(H, 0.5), np.zeros(H)])
    for rsq in (1, 1000):
        v, B, st = R.ln_forward(x, w, 1e-5, rsq)
        assert not v.any() and not B.any() and not st.xh.any()


def test_gelu_inputs_are_single_valued():
    for H in R.WIDTHS:
        c = R.build_case(67, H)
        assert c.replaced <= 0.01
        R.g_of(R.to_np(c.d))                                     # asserts a single G for every element
        assert float(c.d.float().min()) >= -6.0


# ----------------------------------------------------------------------------- d. launch arithmetic and coverage
def test_plan_equals_the_library():
    from snx import fn
    for T in list(range(1, 4200)) + [8192, 8193, 9000, 36864, 69999, 70000]:
        rpb, blocks, last, ws_rows = R.ln_bwd_plan(T)
        for H in R.WIDTHS:
            assert fn("snx_ln_bwd_workspace_bytes")(T, H) == ws_rows * H * 4
        assert 1 <= last <= rpb and (blocks - 1) * rpb + last == T and rpb % R.ROWS_PER_BLOCK == 0
    assert R.ln_bwd_plan(8192)[1] == 1024 and R.ln_bwd_plan(9000)[1] == 750       # the comment's own example: not monotone
    assert fn("snx_embed_ln_bwd_workspace_bytes")(131, 256, R.V) % 256 == 0


def test_workspace_bound_holds_for_every_T():
    """the claim of the comment above snx_ln_bwd_workspace_bytes, proved for T = 1..70,000: every launch's block count fits
    the advertised rows, and a workspace planned for T rows serves every smaller launch"""
    prev = most = 0
    for T in range(1, 70001):
        _, blocks, _, ws_rows = R.ln_bwd_plan(T)
        assert blocks <= ws_rows, T
        assert ws_rows >= prev, T
        prev = ws_rows
        most = max(most, blocks)
        assert most <= ws_rows, T                                # every T' <= T fits the workspace of T
    assert most == 1024


def test_reduce_split_deals_every_partial_row_once():
    for blocks in range(1, 1025):
        seen = []
        for b0, trips, tail in R.reduce_split(blocks):
            seen += list(range(b0, b0 + 16 * trips + tail))
        assert seen == list(range(blocks))


def test_case_tables_reach_every_class():
    assert set(R.WIDTHS) == {256, 512, 768, 1024}
    fwd = set().union(*(R.plan_classes(T) for T in R.FWD_T))
    assert {f"fwd live waves {k}" for k in (1, 2, 3, 4)} <= fwd
    bwd_T = list(R.BWD_T) + [T for T, *_ in R.BWD_LARGE]
    bwd = set().union(*(R.plan_classes(T) for T in bwd_T))
    assert {"trips 1", "trips 2", "trips 3", "last block: fewer rows than waves", "last block: partial second trip",
            "reduce wave: no rows", "reduce wave: tail only", "reduce wave: trips plus tail", "reduce wave: whole trips"} <= bwd
    for T, H, classes, plan in R.BWD_LARGE:
        assert set(classes) <= R.plan_classes(T) and R.ln_bwd_plan(T)[:3] == plan
    assert R.ln_bwd_plan(4096)[3] == 1024 == R.ln_bwd_plan(4096)[1]               # exactly the ceiling
    kinds = {k for _, _, k in R.EMBED_BWD}
    assert kinds == {"fwd", "bwd131", "skew"}
    c = R.build_case(131, 256, 1e-5, "bwd131")
    n = np.bincount(c.ids.numpy(), minlength=R.V)
    assert n[3] == 64 and n[7] == 65 and n[c.pad] == 1 and (n == 0).sum() == R.V - 4
    ids = R.build_case(67, 256).ids
    assert 0 in ids and R.V - 1 in ids and len(set(ids.tolist())) < 67
    sk = np.bincount(R.build_case(4101, 512, 1e-5, "skew").ids.numpy(), minlength=R.V)
    assert 0.35 < sk[5] / 4101 < 0.45 and sk[R.V - 1] > 0 and (sk > R.EMBED_HEAVY).sum() >= 2 and (sk <= R.EMBED_HEAVY).sum() >= 2

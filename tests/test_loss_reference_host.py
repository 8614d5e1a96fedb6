"""Host-side proof of tests/loss_reference.py (no GPU): the reference admits what the cast points of csrc/loss.hip can
produce and rejects what they cannot.

a. Conformance.  emulate() restates snx_loss_fwd / snx_loss_bwd in numpy float32 with the kernel's cast points, every sum
   in three orders -- the kernel's (chunks of CH columns left to right, the chunks dealt to four accumulators, (s0 + s1) +
   (s2 + s3)), plain left to right, a pairwise tree -- and expf / logf correctly rounded and moved by -ULP, 0, +ULP ulps.
   Every output lies inside its acceptance set at every case, in all three families and both modes.
b. Planted faults.  FAULTS names per fault where it must be rejected (case, family, mode); the bf16-mode faults are
   rejected in an exact family as well.  One element outside its set is a rejection.
c. The planted structure of the exact families: the tie (two exact scores less than a bf16 ulp apart with one bf16 value;
   equal expected G in bf16 mode, different in fp32 mode), the label that is not the arg-max, the underflowing teacher row;
   the worst relative half-width of a probability in the random family, printed.
d. The reference's temperature division: torch bf16 arithmetic on the CPU against the contract.
e. The launch arithmetic: the case table reaches every pick_ch, nchunk, ragged, clamp and LDS class.
"""
import numpy as np
import pytest
import torch

from tests import loss_reference as L
from tests.gemm_reference import BF16, bf16_round

f32 = np.float32
ORDERS = ("kernel", "seq", "pair")
MODES = (0, 1)


def _bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(BF16).float().numpy()


def _seq(t):
    return np.cumsum(t, axis=-1, dtype=f32)[..., -1] if t.shape[-1] else np.zeros(t.shape[:-1], f32)


def _pair(t):
    t = t.astype(f32)
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = np.concatenate([t[..., :-2], (t[..., -2:-1] + t[..., -1:]).astype(f32)], axis=-1)
        t = (t[..., ::2] + t[..., 1::2]).astype(f32)
    return t[..., 0]


def fsum(t, order, ch=None, fault=None):
    """sum over the last axis"""
    if fault == "ragged_dropped" and ch and t.shape[-1] % ch and t.shape[-1] > ch:
        t = t[..., :t.shape[-1] // ch * ch]
    if fault == "chunk_twice" and ch:
        t = np.concatenate([t, t[..., :ch]], axis=-1)
    if order == "seq" or (order == "kernel" and not ch):
        return _seq(t)
    if order == "pair":
        return _pair(t)
    n = t.shape[-1]
    nchunk = L.cdiv(n, ch)
    pad = np.zeros(t.shape[:-1] + (nchunk * ch - n,), f32)
    parts = _seq(np.concatenate([t, pad], axis=-1).reshape(t.shape[:-1] + (nchunk, ch)))     # [..., nchunk]
    full = nchunk // 4 * 4
    acc = [_seq(parts[..., i:full:4]) for i in range(4)]
    if nchunk > full:
        acc[0] = _seq(np.concatenate([acc[0][..., None], parts[..., full:]], axis=-1))
    return ((acc[0] + acc[1]).astype(f32) + (acc[2] + acc[3]).astype(f32)).astype(f32)


def dot_rows(a, b, order, ch, fault=None):
    return np.stack([fsum((a[i][None, :] * b).astype(f32), order, ch, fault) for i in range(a.shape[0])])


def _bump(v, d):
    for _ in range(abs(d)):
        v = np.nextafter(v, f32(np.inf) if d > 0 else f32(-np.inf))
    return v.astype(f32)


def emulate(c, bf16_mm, order="kernel", bump=0, fault=None):
    B, Bp, k, V, off, CH = c.B, c.Bp, c.k, c.V, c.off, c.CH
    q, p, n = c.q, c.p, c.n
    tau, lam_q, lam_d, lam_neg, lam_mm, lam_kd, T_kd = c.hp
    one = f32(1)
    inv_tau, inv_tkd = f32(one / tau), f32(one / T_kd)
    use_mm, use_kd = lam_mm > 0 and c.tpos is not None, lam_kd > 0 and c.tsc is not None
    rb = (lambda x: _bf(x)) if bf16_mm else (lambda x: x)

    def ex(x):
        with np.errstate(under="ignore"):
            return np.maximum(_bump(np.exp(x.astype(np.float64)).astype(f32), bump), f32(0))

    def lg(x):
        return _bump(np.log(x.astype(np.float64)).astype(f32), bump)
    a, b = (q, p) if fault == "operands_unrounded" else (rb(q), rb(p))
    D = dot_rows(a, b, order, CH, fault)
    if fault == "score_unrounded":
        s_in = (D * inv_tau).astype(f32)
    elif fault == "round_after_scale":
        s_in = rb((D * inv_tau).astype(f32))
    else:
        s_in = (rb(D) * inv_tau).astype(f32)
    own = p[0:B] if fault == "qp_ignores_off" else p[off:off + B]
    Pd = fsum((q * own).astype(f32), order, CH)
    H = fsum((q[np.arange(B * k) // k] * n).astype(f32), order, CH).reshape(B, k)
    s_h = (H * inv_tau).astype(f32)
    row = np.concatenate([s_in, s_h], 1)

    def lse_of(r):
        mx = r.max(1)
        return (mx + lg(fsum(ex((r - mx[:, None]).astype(f32)), order if order != "kernel" else "seq"))).astype(f32)
    lse = lse_of(row)
    lab = np.arange(B) + (0 if fault == "label_ignores_off" else off)
    ce = (lse - s_in[np.arange(B), lab]).astype(f32)
    infonce = f32(fsum(ce, order) / f32(B))
    gs = f32(inv_tau / f32(B))
    oh = np.zeros((B, Bp), f32)
    oh[np.arange(B), lab] = 1
    G = ((ex((s_in - lse[:, None]).astype(f32)) - oh).astype(f32) * gs).astype(f32)
    if fault != "G_unrounded":
        G = rb(G)
    Gh = (ex((s_h - lse[:, None]).astype(f32)) * gs).astype(f32)
    mmse, dpos = f32(0), np.zeros(B, f32)
    if use_mm:
        df = ((Pd[:, None] - H).astype(f32) - (c.tpos[:, None] - c.tneg.reshape(B, k)).astype(f32)).astype(f32)
        mmse = f32(fsum((df * df).astype(f32).reshape(-1), order) / f32(B * k))
        dsm = ((f32(lam_mm * f32(2)) * df).astype(f32) / f32(B * k)).astype(f32)
        dpos = fsum(dsm, order)
        Gh = (Gh + dsm).astype(f32) if fault == "mm_sign" else (Gh - dsm).astype(f32)
    kdl, Gkd = f32(0), None
    if use_kd:
        o2 = 0 if fault == "kd_ignores_off" else off
        sv = (rb(D[:, o2:o2 + B]) * inv_tkd).astype(f32)
        tv = (c.tsc * inv_tkd).astype(f32)
        ls, lt = (sv - lse_of(sv)[:, None]).astype(f32), (tv - lse_of(tv)[:, None]).astype(f32)
        pt = ex(lt)
        with np.errstate(all="ignore"):
            if fault == "no_xlogy":
                term = (pt * (np.log(pt.astype(np.float64)).astype(f32) - ls).astype(f32)).astype(f32)
            else:
                term = np.where(pt > 0, (pt * (lt - ls).astype(f32)).astype(f32), f32(0))
        kdl = f32(fsum(term.reshape(-1), order) / f32(B))
        gk = f32(f32(lam_kd * inv_tkd) / f32(B))
        Gkd = ((ex(ls) - pt).astype(f32) * gk).astype(f32)
        if fault != "Gkd_unrounded":
            Gkd = rb(Gkd)
    mq = (fsum(q.T.copy(), order) / f32(B)).astype(f32)
    mp = (fsum(p[off:off + B].T.copy(), order) / f32(B)).astype(f32)
    mn = (fsum(n.T.copy(), order) / f32(B if fault == "neg_mean_over_B" else B * k)).astype(f32)
    fl = [fsum((m * m).astype(f32), order, CH) for m in (mq, mp, mn)]
    cnt = (lambda x: (x >= 0).sum()) if fault == "count_ge" else (lambda x: (x > 0).sum())
    nzq, nzd = f32(f32(cnt(q)) / f32(B)), f32(f32(cnt(p[off:off + B])) / f32(B))
    loss = f32(f32(f32(infonce + f32(lam_q * fl[0])) + f32(lam_d * fl[1])) + f32(lam_neg * fl[2]))
    if use_kd and fault != "loss_without_kd":
        loss = f32(loss + f32(lam_kd * kdl))
    if use_mm:
        loss = f32(loss + f32(lam_mm * mmse))
    out9 = np.array([[loss, infonce, fl[0], fl[1], fl[2], mmse, nzq, nzd, kdl]], f32)
    # ---- backward
    go = one if fault == "gout_ignored" else f32(c.gout)
    fq, fd = f32(f32(2 * lam_q) / f32(B)), f32(f32(2 * lam_d) / f32(B))
    fn = f32(f32(2 * lam_neg) / f32(B if fault == "fn_over_B" else B * k))
    bb, aa = rb(p), rb(q)

    def mm_(Gm, X):                                             # sum_j Gm_ij X_jc over the middle index
        return np.stack([fsum((Gm[i][:, None] * X).astype(f32).T.copy(), order) for i in range(Gm.shape[0])])
    R = mm_(G, bb)
    if use_kd:
        K = mm_(Gkd, bb[off:off + B])
        r = rb((R + K).astype(f32)) if fault == "kd_product_joint" else (rb(R) + rb(K)).astype(f32)
    else:
        r = rb(R)
    n3 = n.reshape(B, k, V)
    for kk in range(k):
        r = (r + (Gh[:, kk:kk + 1] * n3[:, kk]).astype(f32)).astype(f32)
    tail = (fq * mq[None, :]).astype(f32) if fault == "dq_without_dpos" else ((dpos[:, None] * p[off:off + B]).astype(f32) + (fq * mq[None, :]).astype(f32)).astype(f32)
    dq = (go * (r + tail).astype(f32)).astype(f32)
    rp = rb(mm_(G.T.copy(), aa))
    loc = rp[off:off + B]
    if use_kd:
        loc = (loc + rb(mm_(Gkd.T.copy(), aa))).astype(f32)
    ptail = (fd * mp[None, :]).astype(f32) if fault == "dp_without_dpos" else ((dpos[:, None] * q).astype(f32) + (fd * mp[None, :]).astype(f32)).astype(f32)
    if fault == "remote_flops":
        rp = (rp + (fd * mp[None, :]).astype(f32)).astype(f32)
        rp[off:off + B] = (loc + (dpos[:, None] * q).astype(f32)).astype(f32) + (fd * mp[None, :]).astype(f32)
    else:
        rp[off:off + B] = (loc + ptail).astype(f32)
    dp = (go * rp).astype(f32)
    dn = (go * ((Gh.reshape(-1, 1) * q[np.arange(B * k) // k]).astype(f32) + (fn * mn[None, :]).astype(f32)).astype(f32)).astype(f32)
    return {"out9": out9, "dq": dq, "dp": dp, "dn": dn, "G": G}


def outside(got, exp):
    bad = {}
    for key in ("out9", "dq", "dp", "dn"):
        lo, hi = exp[key]
        with np.errstate(invalid="ignore"):
            bad[key] = int((~((got[key] >= lo) & (got[key] <= hi))).sum())
    return bad


@pytest.fixture(scope="module")
def expected():
    memo = {}

    def get(name, family, mode):
        if (name, family, mode) not in memo:
            if len(memo) > 12:
                memo.clear()
            memo[name, family, mode] = L.expected(L.build_case(name, family), mode)
        return memo[name, family, mode]
    return get


# ----------------------------------------------------------------------------- a. conformance
@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("name", list(L.ALL_CASES))
def test_emulations_are_admitted(expected, name, family):
    c = L.build_case(name, family)
    big = c.V * c.Bp * c.B > 4_000_000
    for mode in MODES:
        exp = expected(name, family, mode)
        for order, bump in (("kernel", 0), ("seq", L.ULP_EXPF), ("pair", -L.ULP_EXPF)) if big else [(o, b) for o in ORDERS for b in (-L.ULP_EXPF, 0, L.ULP_EXPF)]:
            bad = outside(emulate(c, mode, order, bump), exp)
            assert not any(bad.values()), f"{name} {family} bf16_mm {mode} order {order} expf/logf {bump:+d} ulp: outside {bad}"


# ----------------------------------------------------------------------------- b. planted faults
T20, MMKD = "b13_6_chunks", "b13_5_chunks"
FAULTS = {
    "label_ignores_off": [(MMKD, "exact_a", 1), (MMKD, "random", 0), ("ch64", "exact_b", 1)],
    "qp_ignores_off": [(MMKD, "exact_a", 1), (MMKD, "random", 0)],
    "kd_ignores_off": [(MMKD, "exact_b", 1), ("ch64", "random", 0), ("ch64", "exact_a", 1)],
    "round_after_scale": [(T20, "exact_a", 1), (T20, "exact_b", 1), ("b17_7_chunks", "random", 1)],
    "score_unrounded": [(MMKD, "exact_a", 1), (MMKD, "exact_b", 1), (MMKD, "random", 1)],
    "operands_unrounded": [(MMKD, "exact_b", 1), (MMKD, "random", 1)],
    "G_unrounded": [(MMKD, "exact_b", 1), (MMKD, "random", 1), (MMKD, "exact_a", 1)],
    "Gkd_unrounded": [(MMKD, "exact_b", 1), (MMKD, "random", 1)],
    "kd_product_joint": [(MMKD, "exact_b", 1), (MMKD, "random", 1)],
    "neg_mean_over_B": [(MMKD, "exact_a", 0), ("b17_7_chunks", "random", 1)],
    "ragged_dropped": [(MMKD, "exact_a", 1), (MMKD, "random", 0), ("ch64", "exact_b", 1)],
    "chunk_twice": [(MMKD, "exact_a", 1), (MMKD, "random", 0), ("b1", "exact_b", 1)],
    "dp_without_dpos": [(MMKD, "exact_a", 1), (MMKD, "random", 0)],
    "dq_without_dpos": [(MMKD, "exact_a", 1), (MMKD, "random", 0)],
    "remote_flops": [(MMKD, "exact_a", 1), (MMKD, "random", 0), ("ch64", "exact_b", 1)],
    "fn_over_B": [(MMKD, "exact_a", 0), ("b17_7_chunks", "random", 1)],
    "gout_ignored": [(MMKD, "exact_a", 1), ("b3_one_chunk", "random", 0)],
    "mm_sign": [(MMKD, "exact_a", 1), ("b3_one_chunk", "random", 0)],
    "count_ge": [(MMKD, "exact_a", 1), ("b1", "random", 0)],
    "loss_without_kd": [(MMKD, "exact_b", 1), ("ch64", "random", 0)],
    "no_xlogy": [(MMKD, "exact_b", 1), ("ch64", "random", 0)],
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_rejected(expected, fault):
    for name, family, mode in FAULTS[fault]:
        c = L.build_case(name, family)
        bad = outside(emulate(c, mode, "kernel", 0, fault), expected(name, family, mode))
        assert any(bad.values()), f"{fault} at {name} {family} bf16_mm {mode}: inside every acceptance set"


# ----------------------------------------------------------------------------- c. planted structure
@pytest.mark.parametrize("name", [n for n, d in L.CASES.items() if d["B"] > 2 and d["tau"] == 1.0])
def test_exact_a_holds_a_tie_and_a_label_below_the_maximum(expected, name):
    c = L.build_case(name, "exact_a")
    e0, e1 = expected(name, "exact_a", 0)["mid"], expected(name, "exact_a", 1)["mid"]
    assert bool(np.all(e0.D.lo == e0.D.hi)), "a score of the exact family is not one value"
    assert 5e3 <= float(e0.D.lo[np.arange(c.B), c.off + np.arange(c.B)].max()) <= 2.1e4
    j1, j2 = c.tie
    d1, d2 = float(e0.D.lo[0, j1]), float(e0.D.lo[0, j2])
    assert d1 != d2 and float(bf16_round(np.float64(d1))) == float(bf16_round(np.float64(d2)))
    assert abs(d1 - d2) < 32
    g1 = e1.G.lo[0, j2], e1.G.hi[0, j2]
    lab = e1.G.lo[0, j1] + float(f32(1.0) / f32(c.B)), e1.G.hi[0, j1] + float(f32(1.0) / f32(c.B))
    assert g1[0] > 0.2 / c.B, "the tie does not carry probability"
    assert max(g1[0], lab[0]) <= min(g1[1], lab[1]) + 2.0 ** -8 * g1[1], "bf16 mode: the tied probabilities differ"
    assert e0.s_in.lo[0, j1] != e0.s_in.lo[0, j2], "fp32 mode sees the same score twice"
    last = c.B - 1
    assert int(np.argmax(e0.D.lo[last])) != c.off + last, "the last anchor's label is the arg-max"


def test_random_family_keeps_probabilities_informative(expected):
    worst = 0.0
    for name in ("b13_5_chunks", "b17_7_chunks", "ch64"):
        m = expected(name, "random", 1)["mid"]
        d = (m.s_in.hi - m.s_in.lo) / 2 + (m.lse.hi - m.lse.lo)[:, None] / 2
        worst = max(worst, float(np.expm1(d.max())))
    print(f"random family, bf16 mode: worst relative half-width of a probability {worst:.3%}")
    assert worst <= np.expm1(2 * 2.0 ** -6 + 2.0 ** -6), "scores above 4 or a lost delta"


def test_teacher_row_underflows():
    c = L.build_case("b13_5_chunks", "exact_b")
    tv = c.tsc.astype(np.float64) / 2.0
    pt = np.exp(tv[0] - tv[0].max()).astype(f32)
    assert pt[0] == 1 and bool(np.all(pt[1:] == 0))
    assert bool((c.tpos > 0).any() and (c.tpos < 0).any() and (c.tneg > 0).any() and (c.tneg < 0).any())


# ----------------------------------------------------------------------------- d. the reference's temperature division
def _autocast_scores(q, p, tau):
    """what the reference's loss does under autocast, in this repository's words: a bf16 matrix product (fp32
    accumulation, one rounding of the result), then a division of the bf16 tensor by the Python float tau, which rounds to
    bf16 a second time"""
    s = (torch.from_numpy(q).to(BF16).float() @ torch.from_numpy(p).to(BF16).float().t()).to(BF16)
    return (s / tau).float().numpy()


@pytest.mark.parametrize("tau", [1.0, 0.5, 4.0, 20.0, 500.0])
def test_temperature_division_of_the_reference(tau):
    worst_s = worst_loss = worst_G = 0.0
    for name in ("b13_5_chunks", "b17_7_chunks", "b64_8_chunks"):
        for family in ("exact_a", "exact_b"):
            c = L.build_case(name, family)
            ref = _autocast_scores(c.q, c.p, tau)
            D = _bf(dot_rows(_bf(c.q), _bf(c.p), "seq", None))
            ours = (D * f32(f32(1) / f32(tau))).astype(f32)
            if tau in (1.0, 0.5, 4.0):
                assert np.array_equal(ref, ours), f"{name} {family} tau {tau}: the contract differs from the reference's arithmetic"
                continue
            lab = c.off + np.arange(c.B)

            def soft(s):
                s = s.astype(np.float64)
                lse = np.log(np.exp(s - s.max(1, keepdims=True)).sum(1)) + s.max(1)
                return float((lse - s[np.arange(c.B), lab]).mean()), np.exp(s - lse[:, None])
            (l0, g0), (l1, g1) = soft(ref), soft(ours)
            worst_s = max(worst_s, float(np.abs(ref - ours).max() / max(np.abs(ours).max(), 1e-30)))
            worst_loss, worst_G = max(worst_loss, abs(l0 - l1)), max(worst_G, float(np.abs(g0 - g1).max()))
    if tau in (20.0, 500.0):
        print(f"tau {tau}: second bf16 rounding of the reference: scores rel {worst_s:.3e}, in-batch loss {worst_loss:.3e}, "
              f"probabilities {worst_G:.3e}")
        assert worst_s <= 2.0 ** -8, "more than one bf16 rounding apart"


# ----------------------------------------------------------------------------- e. the table reaches every class
def test_case_table_reaches_every_class():
    reached = set()
    for d in L.ALL_CASES.values():
        assert L.dims_ok(d["B"], d["Bp"], d["k"], d["V"], d["off"])
        reached |= L.case_classes(d)
    assert reached >= L.REQUIRED_CLASSES, L.REQUIRED_CLASSES - reached
    t = L.ALL_CASES.values()
    assert {d["B"] for d in t} >= {1, 3, 4, 13, 17, 64} and {d["k"] for d in t} >= {1, 3, 16}
    assert {d["tau"] for d in t} == {1.0, 20.0} and {d["gout"] for d in t} >= {1.0, 0.25, 0.3}
    assert {(d["mm"], d["kd"]) for d in t} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(d["kd"] and d["Bp"] > d["B"] and d["off"] > 0 for d in t)
    assert {d["Bp"] - d["B"] for d in t} >= {0, 1} and any(d["Bp"] == 4 * d["B"] for d in t)
    assert any(d["off"] == 0 and d["Bp"] > d["B"] for d in t) and any(0 < d["off"] < d["Bp"] - d["B"] for d in t)
    assert any(d["off"] == d["Bp"] - d["B"] > 0 for d in t)
    for bad in L.REFUSED:
        assert not L.dims_ok(*bad), bad
    assert L.lds_bytes(64, 512, 1) == (76032, 131840) and L.lds_bytes(64, 64, 1)[0] == 66048

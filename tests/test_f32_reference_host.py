"""CPU proofs about tests/f32_reference.py (no GPU): the chain emulation equals exact rational arithmetic rounded once,
planted halfway cases included; fp32 emulations of every kernel family in several summation / arrival orders lie inside
the acceptance sets (the worst err / bound is printed); and every planted fault is rejected by at least one case of the
case tables tests/test_gpu_f32_per_element.py runs, which proves that the tables reach the class."""
from fractions import Fraction

import numpy as np
import pytest

from tests import f32_reference as F

f32 = np.float32


def fl32_fraction(x):
    """a rational rounded ONCE to fp32 (round to nearest even, normal range), by integer arithmetic"""
    if x == 0:
        return 0.0
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e < 127
    scaled = a / Fraction(2) ** (e - 23)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return (-1.0 if x < 0 else 1.0) * float(n) * 2.0 ** (e - 23)


def _fr(v):
    return Fraction(float(v))


def rejected(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------- the chain
def _halfway_triples():
    """(a, b, c) with a b + c exactly half way between two fp32 neighbours (residual 0), or 2^-70 above / below it: the
    float64 sum then IS the halfway point and only the TwoSum residual says which way to go"""
    x = f32(2.0 ** -12) * (f32(1) + f32(2.0 ** -23))
    y = f32(2.0 ** -12) * (f32(1) - f32(2.0 ** -23))            # x y = 2^-24 - 2^-70
    h = f32(2.0 ** -12)                                          # h h = 2^-24
    odd, even = f32(1) + f32(2.0 ** -23), f32(1)
    out = []
    for s in (1.0, -1.0):
        for scale in (1.0, 8.0, 2.0 ** -5):
            sc = f32(scale)
            for c0 in (even, odd):
                out.append((h * sc, f32(s) * h, f32(s) * c0 * sc))            # residual 0: ties to even
                out.append((x * sc, f32(s) * y, f32(s) * c0 * sc))            # |a b| = 2^-24 - 2^-70: towards c
                out.append((x * sc, f32(-s) * y, f32(s) * (c0 + f32(2.0 ** -23)) * sc))   # c - (2^-24 - 2^-70): away from the lower
    return out


def test_chain_emulation_equals_rational_arithmetic_rounded_once():
    rng = np.random.default_rng(0)
    n = 4000
    a, b, c = F.operand_values(rng, n), F.operand_values(rng, n), F.operand_values(rng, n)
    c[::3] = (-(a[::3].astype(np.float64) * b[::3].astype(np.float64))).astype(f32)       # cancellation
    c[1::7] *= f32(2.0 ** -12)
    trip = list(zip(a, b, c)) + _halfway_triples()
    A, B, Cc = (np.array([t[i] for t in trip], dtype=f32) for i in range(3))
    got = F.fma32(A, B, Cc)
    ties = 0
    for i, (x, y, z) in enumerate(trip):
        exact = _fr(x) * _fr(y) + _fr(z)
        want = fl32_fraction(exact)
        assert float(got[i]) == want, (i, x, y, z, float(got[i]), want)
        s = float(np.float64(x) * np.float64(y) + np.float64(z))
        ties += int(Fraction(s) != exact and (np.float64(s).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000))
    assert ties >= 12, ties                                      # the planted cases did reach the residual branch
    # a whole chain against the rational recurrence
    A, B = F.operand_values(rng, (50, 37)), F.operand_values(rng, (50, 37))
    got = F.chain(A, B)
    for i in range(50):
        acc = Fraction(0)
        for k in range(37):
            acc = Fraction(fl32_fraction(acc + _fr(A[i, k]) * _fr(B[i, k])))
        assert float(got[i]) == float(acc)


def test_numpy_float32_products_and_sums_are_single_roundings():
    """what rope_expected relies on"""
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal(500).astype(f32), rng.standard_normal(500).astype(f32)
    p, s = (x * y).astype(f32), (x + y).astype(f32)
    for i in range(500):
        assert float(p[i]) == fl32_fraction(_fr(x[i]) * _fr(y[i])) and float(s[i]) == fl32_fraction(_fr(x[i]) + _fr(y[i]))


# ----------------------------------------------------------------------------- GEMM
def test_gemm_table_reaches_every_form_and_vec_class():
    forms, vecs = set(), set()
    for name, M, N, K, form, _ in F.GEMM_CASES:
        for lay in F.LAYOUTS:
            c = F.gemm_case(name, lay)
            forms.add(c.form)
            vecs.add((c.a_vec, c.b_vec))
    assert forms == {"64", "deepk", "128"} and vecs == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert {(M, N, K) for _, M, N, K, _, _ in F.GEMM_CASES} >= {(1, 1, 1), (65, 63, 15), (130, 70, 50), (33, 100, 130), (64, 64, 128),
                                                              (100, 300, 200), (2049, 2050, 33), (4100, 1030, 70)}
    for name in ("big33", "big70"):
        c = F.gemm_case(name, "nt")
        r, q = F.gemm_subset(c)
        assert len(r) >= 200_000 and c.M * c.N >= 4_194_304
        sel = np.zeros((c.M, c.N), dtype=bool)
        sel[r, q] = True
        assert sel[(c.M - 1) // 128 * 128:].all() and sel[:, (c.N - 1) // 128 * 128:].all()


@pytest.mark.parametrize("fault", F.GEMM_FAULTS)
def test_gemm_fault_is_rejected(fault):
    for name, M, N, K, form, _ in F.GEMM_CASES:
        if form == "128":
            continue
        for lay in F.LAYOUTS:
            c = F.gemm_case(name, lay)
            r, q = F.gemm_subset(c)
            if rejected(F.check_bits, "gemm", F.gemm_expected(c, r, q, fault), F.gemm_expected(c, r, q)):
                print(fault, "rejected by", name, lay)
                return
    raise AssertionError(f"no case of the table rejects {fault}")


# ----------------------------------------------------------------------------- tail
def test_tail_admission_and_every_fault_rejected():
    tally = F.Tally()
    left = set(F.TAIL_FAULTS)
    for name, lens, V, H, form in F.TAIL_CASES:
        if form == "128":
            continue
        for fam in F.TAIL_FAMILIES:
            for mk in F.TAIL_MASKS:
                c = F.tail_case(name, fam, mk)
                x = F.tail_logits(c)
                keys, tw = F.tail_fwd_emul(c, x)
                F.tail_fwd_check(c, keys, tw, F.split_keys(keys)[0], F.split_keys(tw)[0], tally=tally, x_cols=x, x_rows=x)
                for f in sorted(left):
                    k2, t2 = F.tail_fwd_emul(c, x, f)
                    if rejected(F.tail_fwd_check, c, k2, t2, F.split_keys(k2)[0], F.split_keys(t2)[0], x_cols=x, x_rows=x):
                        left.discard(f)
    assert not left, f"no case of the table rejects {sorted(left)}"
    print(tally)


def test_tail_exact_family_is_exact_and_its_log1p_sets_are_disjoint():
    for name, lens, V, H, form in F.TAIL_CASES:
        c = F.tail_case(name, "exact", "ones")
        if form == "128":
            x = F.tail_logits(c, np.arange(0, c.T, 50), None)
        else:
            x = F.tail_logits(c)
            assert np.array_equal(x, (F.chain(c.Hd[:, None, :], c.E[None, :, :]) + c.bias[None, :]).astype(f32))    # whatever the form
        v = np.unique(np.maximum(x, 0))
        lo, hi = F.log1p_set(v, F.ULP_LOG1PF)
        assert np.all(hi[:-1] < lo[1:]), "two exact logits whose log1pf sets overlap"


@pytest.mark.parametrize("with_tw", [True, False])
def test_tail_backward_admission(with_tw):
    tally = F.Tally()
    for name in ("v65", "v200"):
        for fam in F.TAIL_FAMILIES:
            c = F.tail_case(name, fam, "holes")
            keys, tw = F.tail_ref_keys(c)
            g, g_tw, gE0, gb0 = F.tail_grads(c)
            g_tw = g_tw if with_tw else None
            exp = F.tail_bwd_expected(c, keys, tw, g, g_tw, gE0, gb0, F.ulps())
            for order in ("asc", "perm", "rev"):
                F.check_sets(f"{name} {fam} {order}", F.tail_bwd_emul(c, keys, tw, g, g_tw, gE0, gb0, order), exp, tally, None, "tail bwd ")
            for fault in ("no_exp", "no_skip"):                  # c = g without exp(-y); a contribution where y <= 0
                assert rejected(F.check_sets, "x", F.tail_bwd_emul(c, keys, tw, g, g_tw, gE0, gb0, "asc", fault), exp), fault
    print(tally)


# ----------------------------------------------------------------------------- rows
@pytest.mark.parametrize("H", F.LN_H)
def test_layernorm_admission(H):
    tally = F.Tally()
    for T in (5, 67):
        for eps in F.LN_EPS:
            c = F.ln_case(T, H, eps)
            for order in ("asc", "pair", "perm"):
                for src in F.LN_FWD_MODES:
                    F.check_interval(f"fwd {src} {order} T {T}", F.ln_emul(c, src, order=order), *F.ln_fwd_expected(c, src, F.ulps()),
                                     tally, f"ln fwd src {src}")
                for mode, src in (("acc", 0), ("ow", 0), ("embed", 1), ("gelu", 2)):
                    F.check_sets(f"bwd {mode} {order} T {T}", F.ln_emul(c, src, mode, order), F.ln_bwd_expected(c, mode, F.ulps()), tally,
                                 None, f"ln bwd {mode} ")
    print(f"H {H}: {tally}")


LN_FAULT_AT = {"no_mean": (0, None), "eps_outside": (0, None), "last_stride": (0, None), "dw_with_w": (0, "ow"), "pad_row": (1, "embed"),
               "acc_overwrites": (0, "acc"), "gelu_of_xhat": (2, "gelu")}


@pytest.mark.parametrize("fault", F.LN_FAULTS)
def test_layernorm_fault_is_rejected(fault):
    src, mode = LN_FAULT_AT[fault]
    for H in F.LN_H:
        for T in reversed(F.LN_T):
            for eps in F.LN_EPS:
                c = F.ln_case(T, H, eps)
                bad = F.ln_emul(c, src, mode, fault=fault)
                if mode is None:
                    hit = rejected(F.check_interval, "ln", bad, *F.ln_fwd_expected(c, src, F.ulps()))
                else:
                    hit = rejected(F.check_sets, "ln", bad, F.ln_bwd_expected(c, mode, F.ulps()))
                if hit:
                    print(fault, "rejected at H", H, "T", T, "eps", eps)
                    return
    raise AssertionError(f"no case of the table rejects {fault}")


def test_rope_faults_are_rejected():
    left = set(F.ROPE_FAULTS)
    for hd in F.ROPE_HD:
        for heads in F.ROPE_HEADS:
            for T in F.ROPE_T:
                c = F.rope_case(T, heads, hd)
                for inverse in (0, 1):
                    want = F.rope_expected(c, inverse)
                    assert np.array_equal(want[:, 2], c.qkv[:, 2])
                    for f in sorted(left):
                        if rejected(F.check_bits, "rope", F.rope_expected(c, inverse, f), want):
                            left.discard(f)
    assert not left, sorted(left)
    c = F.rope_case(67, 4, 16)                                   # the inverse undoes the forward up to rounding
    fwd = F.rope_expected(c, 0)
    back = F.rope_expected(F.SimpleNamespace(**{**vars(c), "qkv": fwd}), 1)
    assert float(np.abs(back - c.qkv).max()) < 1e-5


def test_geglu_admission_and_faults():
    tally = F.Tally()
    left = set(F.GEGLU_FAULTS)
    for I in F.GEGLU_I:
        for T in F.GEGLU_T:
            c = F.geglu_case(T, I)
            exp = F.geglu_expected(c, F.ulps())
            F.check_sets(f"geglu T {T} I {I}", F.geglu_emul(c), exp, tally, F.geglu_expected(c, F.ulps(all=0)), "geglu ")
            for f in sorted(left):
                if rejected(F.check_sets, "geglu", F.geglu_emul(c, f), exp):
                    left.discard(f)
    assert not left, sorted(left)
    c = F.geglu_case(67, 96)
    assert all(np.any(c.u[:, :c.I] == f32(s)) and np.any(c.u[:, c.I:] == f32(s)) for s in F.SPECIALS)
    print(tally)


# ----------------------------------------------------------------------------- attention
def test_attention_tables_reach_every_class():
    for hd, salt in [(h, int(h != 16)) for h in F.ATTN_HD_TILED] + [(h, int(h != 6)) for h in F.ATTN_HD_ROWS] + \
            [(h, int(h != 16)) for h in F.ATTN_HD_BWD]:
        tab = F.attn_table(hd, salt)
        assert {(li, w) for li, w, _ in tab} == {(li, w) for li in range(len(F.ATTN_LENS)) for w in F.ATTN_WINDOWS}
        if salt == 0:
            assert {(li, r) for li, _, r in tab} == {(li, r) for li in range(len(F.ATTN_LENS)) for r in F.ATTN_RECIPES}
    assert F.ATTN_LENS == ((1,), (1, 2, 65, 257), (128, 129, 64, 63), (3,) * 30 + (300,))
    T, B = sum(F.ATTN_LENS[3]), len(F.ATTN_LENS[3])
    assert max(1, min(64, F.cdiv(F.cdiv(T, B), 128))) == 1      # the grid's z follows the mean length: the long one strides
    novis = 0
    for li, w, rec in F.attn_table(16, 0):
        c = F.attn_case(li, 2, 16, w, rec)
        r = F.attn_fwd_expected(c, F.ulps())
        novis += int((np.abs(r.out_b).max(axis=(1, 2)) == 0).sum())
    assert novis > 100                                           # rows without a visible key are there, and pinned to 0


@pytest.mark.parametrize("hd", (2, 16, 64))
def test_attention_admission(hd):
    tally = F.Tally()
    for li, w, rec in F.attn_table(hd, salt=1)[::2]:
        c = F.attn_case(li, 2 if hd < 64 else 1, hd, w, rec)
        for order in ("asc", "perm", "rev"):
            out, lse, dqkv = F.attn_emul(c, order)
            F.attn_fwd_check(f"hd {hd} lens {li} window {w} {rec} {order}", c, out, lse, tally)
            F.attn_bwd_check(f"hd {hd} lens {li} window {w} {rec} {order}", c, dqkv, out, lse, tally)
    print(f"hd {hd}: {tally}")


ATTN_FAULT_AT = {       # fault -> (predicate on (lens index, window, recipe), which check sees it)
    "drop_visible": (lambda li, w, r: li == 1, "fwd"), "include_masked": (lambda li, w, r: r == "holes" and li == 1, "fwd"),
    "window_strict": (lambda li, w, r: w == 8 and li == 1, "fwd"), "scale_8th": (lambda li, w, r: li == 1, "fwd"),
    "key65": (lambda li, w, r: li == 1 and w in (-1, 1000, 64), "fwd"), "query129": (lambda li, w, r: li == 2, "fwd"),
    "skip_q0_stride": (lambda li, w, r: li == 3, "fwd"), "lse_no_max": (lambda li, w, r: li == 1, "fwd"),
    "no_delta": (lambda li, w, r: li == 1, "bwd"), "dk_no_scale": (lambda li, w, r: li == 1, "bwd"),
    "dv_from_ds": (lambda li, w, r: li == 1, "bwd"), "novis_mean_v": (lambda li, w, r: r == "novis" or w == 0, "fwd"),
}


@pytest.mark.parametrize("fault", F.ATTN_FAULTS)
def test_attention_fault_is_rejected(fault):
    pred, which = ATTN_FAULT_AT[fault]
    for li, w, rec in F.attn_table(16, 0):                       # head_dim 16: in the tiled, the forward and the backward table
        if not pred(li, w, rec):
            continue
        c = F.attn_case(li, 2, 16, w, rec)
        out, lse, dqkv = F.attn_emul(c, fault=fault)
        if which == "fwd":
            hit = rejected(F.attn_fwd_check, "attn", c, out, lse)
        else:
            hit = rejected(F.attn_bwd_check, "attn", c, dqkv, out, lse)
        if hit:
            print(fault, "rejected at lens", li, "window", w, rec)
            return
    raise AssertionError(f"no case of the table rejects {fault}")

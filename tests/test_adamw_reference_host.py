"""Host-side proof of tests/adamw_reference.py (no GPU): the reference admits what the three kernels of
csrc/optimizer.hip can produce and rejects what they cannot.

a. Conformance.  emulate() restates snx_adamw_clip_step in numpy float32: the sum of squares in three orders (the
   kernel's: float4 groups, grid-stride per thread, the 64-lane butterfly, four waves, the partials per thread of the
   final block, the tail on thread 0; left to right; a pairwise tree), the update with every product rounded and with
   the multiply-adds contracted to fmas, powf the C library's.  Every result lies inside its acceptance set at
   every case of the table.
b. Planted faults.  FAULTS names per fault the cases that must reject it; one element outside its set is a rejection.
c. Width.  Where coef is one value the sets are a few adjacent fp32 values wide: asserted against what the derivation
   predicts (one outward rounding per operation), not against a kernel; the norm's set is as wide as gamma_n.
d. The launch arithmetic: the case table reaches every tail, clamp and pass class.  (The argument checks of the entry
   point need the library: tests/test_gpu_adamw_per_element.py.)
"""
import numpy as np
import pytest

from tests import adamw_reference as A

f32 = np.float32
ORDERS = ("kernel", "seq", "pair")


def _seq(t):
    return np.cumsum(t, dtype=f32)[-1] if t.size else f32(0)


def _pair(t):
    t = t.astype(f32)
    if not t.size:
        return f32(0)
    while t.size > 1:
        if t.size % 2:
            t = np.concatenate([t[:-2], [f32(t[-2] + t[-1])]])
        t = (t[::2] + t[1::2]).astype(f32)
    return t[0]


def _butterfly(v):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., idx ^ o]).astype(f32)
    return v[..., 0]


def _block_sum(s):
    """[blocks, 256] -> [blocks]: wave_sum, then (red0 + red1) + (red2 + red3)"""
    w = _butterfly(s.reshape(-1, 4, 64))
    return ((w[:, 0] + w[:, 1]).astype(f32) + (w[:, 2] + w[:, 3]).astype(f32)).astype(f32)


def sum_squares(g, order, fault=None):
    n = g.size
    pl = A.plan(n)
    body, tail = g[:pl.n4 * 4], g[pl.n4 * 4:]
    if fault == "tail_not_in_norm":
        tail = tail[:0]
    sq = (g * g).astype(f32) if fault != "tail_not_in_norm" else (body * body).astype(f32)
    if order == "seq":
        return _seq(sq)
    if order == "pair":
        return _pair(sq)
    v = (body * body).astype(f32).reshape(-1, 4)
    q = ((v[:, 0] + v[:, 1]).astype(f32) + (v[:, 2] + v[:, 3]).astype(f32)).astype(f32)
    threads = pl.sumsq_blocks * 256
    qq = np.zeros(max(pl.sumsq_passes, 1) * threads, f32)
    qq[:q.size] = q
    per_thread = np.cumsum(qq.reshape(-1, threads), axis=0, dtype=f32)[-1]
    part = _block_sum(per_thread.reshape(pl.sumsq_blocks, 256))
    pp = np.zeros(A.cdiv(part.size, 256) * 256, f32)
    pp[:part.size] = part
    s = np.cumsum(pp.reshape(-1, 256), axis=0, dtype=f32)[-1]
    for x in tail:
        s[0] = f32(s[0] + f32(x * x))
    return _block_sum(s[None, :])[0]


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def emulate(c, order="kernel", fused=False, fault=None):
    """-> {"norm", "p", "m", "v"} as float32"""
    hp = A.hp_array(c.hp)
    lr, b1, b2, eps, wd, max_norm = hp
    one = f32(1)
    g = c.g
    with np.errstate(all="ignore"):
        norm = np.sqrt(sum_squares(g, order, fault))
        if max_norm > 0:
            den = norm if fault == "no_1e-6" else f32(norm + f32(1e-6))
            coef = f32(max_norm / den)
            if fault != "uncapped":
                coef = min(one, coef)
        else:
            coef = one
        bc1 = f32(one - f32(A.host_powf(b1, c.step)))
        bc2 = f32(one - f32(A.host_powf(b2, c.step)))
        bc2s = bc2 if fault == "bc2_no_sqrt" else np.sqrt(bc2)
        ss = f32(lr / bc1)
        idx = np.arange(c.n, dtype=np.int64)
        nd = A.nodecay_mask(c.n, c.nd)
        if fault == "decay_at_first" and c.nd[1] > c.nd[0]:
            nd[c.nd[0]] = False
        if fault == "decay_at_last" and c.nd[1] > c.nd[0]:
            nd[min(c.nd[1], c.n) - 1] = False
        w = np.where(nd, f32(0), wd).astype(f32)
        gr = (g * coef).astype(f32)
        gm = g if fault == "unclipped_moments" else gr
        omb1, omb2 = f32(one - b1), f32(one - b2)
        if fused:
            keep = _fma(-lr, w, one)
            m = _fma(b1, c.m, (omb1 * gm).astype(f32))
            v = _fma(b2, c.v, ((omb2 * gm).astype(f32) * gm).astype(f32))
        else:
            keep = (one - (lr * w).astype(f32)).astype(f32)
            m = ((b1 * c.m).astype(f32) + (omb1 * gm).astype(f32)).astype(f32)
            v = ((b2 * c.v).astype(f32) + ((omb2 * gm).astype(f32) * gm).astype(f32)).astype(f32)
        p1 = (c.p * keep).astype(f32)
        if fault == "eps_in_sqrt":
            den = (np.sqrt((v + eps).astype(f32)) / bc2s).astype(f32)
        else:
            den = ((np.sqrt(v) / bc2s).astype(f32) + eps).astype(f32)
        upd = ((ss * m).astype(f32) / den).astype(f32)
        p = (p1 - upd).astype(f32)
    skip = np.zeros(c.n, bool)
    if fault == "tail_skipped":
        skip = idx >= 4 * (c.n // 4)
    if fault == "no_second_pass":
        skip = idx >= A.plan(c.n).update_blocks * 1024
    p, m, v = (np.where(skip, a, b).astype(f32) for a, b in ((c.p, p), (c.m, m), (c.v, v)))
    return {"norm": np.array([norm], f32), "p": p, "m": m, "v": v}


def outside(got, exp):
    """{output: number of elements outside their set}"""
    bad = {}
    for k, val in got.items():
        lo, hi = exp[k]
        v = val.reshape(lo.shape)
        bad[k] = int((~((v >= lo) & (v <= hi))).sum())
    return bad


# ----------------------------------------------------------------------------- a. conformance
@pytest.mark.parametrize("name", A.SMALL)
def test_emulations_are_admitted(name):
    c = A.build_case(name)
    exp = A.expected(c)
    for order in ORDERS:
        for fused in (False, True):
            bad = outside(emulate(c, order, fused), exp)
            assert not any(bad.values()), f"{name} order {order} fused {fused}: outside {bad}"


def test_large_case_is_admitted():
    c = A.build_case("large")
    exp = A.expected(c)
    assert exp["exact_norm"], "the large case must pin its norm to one value"
    assert exp["norm"][0] == exp["norm"][1]
    for order in ORDERS:
        bad = outside(emulate(c, order, fused=(order == "pair")), exp)
        assert not any(bad.values()), f"large, order {order}: outside {bad}"
    bad = outside(emulate(c, "seq", fault="no_second_pass"), exp)
    assert bad["p"] and bad["m"], f"the skipped second grid-stride pass went unnoticed: {bad}"


# ----------------------------------------------------------------------------- b. planted faults
FAULTS = {
    "decay_at_first": ("nd_vec_offset_0", "nd_vec_offset_1", "nd_vec_offset_2", "nd_vec_offset_3", "nd_one_element",
                       "nd_begins_in_tail", "nd_whole", "n3_nd_inside", "n5_clip"),
    "decay_at_last": ("nd_vec_offset_0", "nd_vec_offset_1", "nd_vec_offset_2", "nd_vec_offset_3", "nd_one_element",
                      "nd_ends_in_tail", "nd_whole", "n3_nd_inside", "n5_clip"),
    "tail_skipped": ("n1_step1_clip", "n3_tiny", "n5_clip", "n7_small", "n1023_step1", "n16386_clip"),
    "tail_not_in_norm": ("n1_step1_clip", "n5_clip", "n3_tiny"),
    "no_1e-6": ("n3_tiny", "n1023_tiny", "n1023_exact"),
    "uncapped": ("n7_small", "n16386_small"),
    "bc2_no_sqrt": ("n1_step1_clip", "n1023_step1", "nd_vec_offset_0"),
    "eps_in_sqrt": ("n1023_step1", "n1023_zero_grad", "n1023_late"),
    "unclipped_moments": ("n5_clip", "n1023_step1", "n16386_clip"),
    "no_second_pass": ("n16386_clip", "n16386_small"),         # and the large case: test_large_case_is_admitted
}


@pytest.mark.parametrize("fault", [f for f, cases in FAULTS.items() if cases])
def test_planted_fault_is_rejected(fault):
    for name in FAULTS[fault]:
        c = A.build_case(name)
        exp = A.expected(c)
        for order in ORDERS:
            bad = outside(emulate(c, order, fault=fault), exp)
            assert any(bad.values()), f"{fault} at {name}, order {order}: inside every acceptance set"


# ----------------------------------------------------------------------------- c. width of the sets
def _ulps(lo, hi):
    a = lo.astype(f32).view(np.int32).astype(np.int64)
    b = hi.astype(f32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return b - a + 1


def test_sets_are_a_few_values_wide():
    """m' is three operations behind coef and v' four: with coef one value (no clipping, or an exact norm) the set of v', a
    sum of non-negative terms, holds at most 5 adjacent values, and the set of m' is at most 4 ulp of |beta1 m| +
    |(1 - beta1) g| wide (its two terms may cancel); fewer than 32 roundings (outward, both corners) stand between the inputs and the
    quotient, which is free of cancellation; the decayed p is two outward roundings wide and one subtraction follows: the
    width of p' stays below 6 ulp of max(|p|, |p'|) plus 32 ulp of the step taken"""
    for name in ("n4_noclip", "n7_small", "n1023_exact", "n1023_zero_grad", "n16386_small"):
        c = A.build_case(name)
        exp = A.expected(c)
        assert int(_ulps(*exp["v"]).max()) <= 5, name
        mlo, mhi = exp["m"]
        mag = (np.abs(0.9 * c.m.astype(np.float64)) + np.abs(0.1 * c.g.astype(np.float64)))[:, None]       # coef = 1 or below
        assert bool(np.all(mhi - mlo <= 4 * 2.0 ** -23 * mag)), name
        lo, hi = exp["p"]
        upd = np.abs(c.p.astype(np.float64)[:, None] - (lo + hi) / 2)
        room = 6 * 2.0 ** -23 * np.maximum(np.abs(c.p.astype(np.float64)[:, None]), np.abs(lo + hi) / 2) + 32 * 2.0 ** -23 * upd
        assert bool(np.all(hi - lo <= room)), name
    for name in A.SMALL:                                        # clipping on: the norm's gamma_n enters, nothing else
        c = A.build_case(name)
        exp = A.expected(c)
        nlo, nhi = exp["norm"][0].item(), exp["norm"][1].item()
        assert nhi - nlo <= (2 * A.gamma(c.n) + 4 * 2.0 ** -24) * nhi, name


# ----------------------------------------------------------------------------- d. the table reaches every class
def test_case_table_reaches_every_class():
    reached = set()
    for c in A.CASES.values():
        reached |= A.plan_classes(c["n"])
    assert reached >= A.REQUIRED_CLASSES, A.REQUIRED_CLASSES - reached
    assert {c["n"] for c in A.CASES.values()} >= {1, 3, 4, 5, 7, 1023, 4096 * 4 + 2, A.LARGE_N}
    assert A.LARGE_N > 8192 * 4096 and A.LARGE_N % 4
    pl = A.plan(A.LARGE_N)
    assert (pl.sumsq_blocks, pl.update_blocks, pl.update_passes) == (2048, 8192, 5)
    assert {c["step"] for c in A.CASES.values()} >= {1, 2, 100000}
    assert any(c["max_norm"] == 0 for c in A.CASES.values()) and any(c["max_norm"] < 0 for c in A.CASES.values())
    nd = [c["nd"] for c in A.CASES.values() if c["n"] == 1023]
    assert {b % 4 for b, e in nd if e > b} == {0, 1, 2, 3} and {e % 4 for b, e in nd if e > b} == {0, 1, 2, 3}
    assert (0, 0) in nd and (0, 1023) in nd and any(b == 1023 for b, _ in nd) and any(1020 < e < 1023 for _, e in nd)

"""Float64 restatement of csrc/optimizer.hip (sumsq_partial_kernel, sumsq_final_kernel, adamw_kernel behind
snx_adamw_clip_step), the case table, a restatement of the launch arithmetic, and per-element acceptance SETS that follow
from the kernels' fp32 operations.  Plain numpy on the CPU; sibling of tests/rows_reference.py, whose guarded buffers,
outward roundings and exact-sum test it reuses.

Contracts (fl32 = one fp32 operation, correctly rounded; hp = {lr, beta1, beta2, eps, wd, max_norm} as fp32):
    norm      = sqrtf(S^), S^ = the fp32 sum of the n squares fl32(g_i g_i) in ANY order: the PRE-clip global L2 norm
    coef      = max_norm > 0 ? fminf(1, fl32(max_norm / fl32(norm + 1e-6f))) : 1
    host      bc1 = fl32(1 - powf(beta1, (float)step)), bc2s = sqrtf(fl32(1 - powf(beta2, (float)step))),
              ss = fl32(lr / bc1)                                                  (ss on the device, bc1 / bc2s on the host)
    element   gr = fl32(g coef); w = 0 inside [nodecay_begin, nodecay_end), wd outside
              p1 = fl32(p fl32(1 - fl32(lr w)));  m' = fl32(fl32(beta1 m) + fl32(fl32(1 - beta1) gr))
              v' = fl32(fl32(beta2 v) + fl32(fl32(fl32(1 - beta2) gr) gr))
              p' = fl32(p1 - fl32(fl32(ss m') / fl32(fl32(sqrtf(v') / bc2s) + eps)))
    the float4 body and the scalar tail (the last n % 4 elements, all of them when n < 4) are the same expression

Acceptance set, not a tolerance.  Every quantity is carried as an interval [lo, hi] of fp32 values:
    S^        every partial sum exact in fp32 (all squares multiples of one power of two, their sum below 2^24 of it:
              rows_reference.exact_sum_rows): S^ = S, one value.  Otherwise n products and n - 1 additions in any order,
              fused or not: |S^ - S| <= gamma_n S, gamma_n = n u / (1 - n u), u = 2^-24; the float64 evaluation of S adds
              the factor 1 + 2^-20.  (n u >= 1/2 without exact sums is refused: the large case is of the exact kind.)
    sqrtf     monotone and correctly rounded: [sqrtf(up(S lo)), sqrtf(down(S hi))]
    coef      every operation is monotone in norm: the two corners are the interval
    powf      a HOST libm call: the reference calls the same powf of the C library (ctypes), as the entry point does, so
              bc1 and bc2s are one value each.  (An interval of +-1 ulp around powf would be amplified by the
              cancellation in 1 - beta2^step to 6e-5 of the update at step 2: the sets would stop deciding.)
    element   interval arithmetic, operation by operation in the kernel's order: the real result of an operation over
              the corners of its operand intervals, rounded OUTWARD to fp32.  fl32 is monotone, so fl32 of any real
              result inside [lo, hi] lies inside [down(lo), up(hi)]; a contracted fma (one rounding fewer, the exact
              product instead of the rounded one) lies inside the same interval, whichever product the compiler fuses.
    No libm function runs on the device (sqrtf and the division are correctly rounded: snx/build.py sets no fast-math
    flag), so nothing is assumed, and no constant was fitted to a kernel's output.

Inputs (build_case): p = 0.1 randn, m = 0.01 randn, v = 1e-4 rand with every seventh element exactly 0 (the update is
m' / eps there when the gradient is 0 as well); gradients by `kind`:
    big    10 x the parameters' scale: clipping on          small  1e-3 x: clipping off (coef = 1 decides nothing)
    mixed  the two interleaved in runs of five              zero   all zero: norm = 0, coef = 1
    tiny   1e-4 randn against max_norm = 1e-4: the 1e-6 of the denominator is 1 % of it
    exact  sparse multiples of 2^-6: every partial sum of squares is exact, the norm is ONE value
The large case draws its elements from a palette of 4,093 tuples (prime: the pattern shifts by three from one 4,096-element
block to the next), element i holding tuple i % 4,093: its float64 reference is the palette's, gathered in one pass.

Launch arithmetic restated: plan(n) -> float4 count, tail, blocks and passes of the sum of squares (clamp 2,048) and of
the update (clamp 8,192).  CASES names per case the seam it is there for; tests/test_adamw_reference_host.py asserts that
the table reaches every class.

Measured on an MI355X with the kernels of commit 9db777b (the change that adds this file touches no kernel), over all
cases of tests/test_gpu_adamw_per_element.py: 25 tests, 6 to 8 s for the file, the slowest test the large case
(n = 33,558,531: 3.6 to 6.2 s over four runs, most of it the comparison on the CPU); every other test below 0.3 s.  Nothing
fell outside its acceptance set, no guard was touched, a second run gave the same bits, and where the norm's set is one
value (n1_step1_clip, the zero gradient, the two exact cases) the kernel met it bit for bit.  Nothing is assumed in this
module, so no assumption could decide an element.  No output is rounded to bf16; the number of fp32 values per set:
    coef one value (no clipping, zero or exact gradient, the large case): p median 3-4, m 2-3, v 2-4; the most in any set
        97 for p (an update 1e5 times the parameter, m / eps) and 13 for m (its two terms cancel)
    clipping on at n = 1,023: norm 690-850 values (gamma_n, any order), p median 4-5, m 6-12, v 5-7; n = 16,386: norm
        11,600 values, p median 4, m 16, v 6; where the terms of m' or the update cancel a set reaches 1e5-2e6 values
tests/test_adamw_reference_host.py: 36 tests, 16 s on the CPU (14 s of it the large case in three orders).
"""
import ctypes as C
import ctypes.util
import functools
from types import SimpleNamespace

import numpy as np

from tests.gemm_reference import U32, f32_down, f32_up
from tests.rows_reference import F64, exact_sum_rows, gamma

f32 = np.float32
TINY = 2.0 ** -126
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
SCRATCH_FLOATS = 2048
SUMSQ_CLAMP, UPDATE_CLAMP = 2048, 8192
PALETTE = 4093
LARGE_N = UPDATE_CLAMP * 4096 + 4096 + 3        # both clamps; a fifth grid-stride pass of five blocks, a tail of three


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- launch arithmetic, restated
def plan(n):
    n4 = n // 4
    sb = min(max(cdiv(n4, 256 * 8), 1), SUMSQ_CLAMP)
    ub = min(cdiv(n, 256 * 4 * 4), UPDATE_CLAMP)
    return SimpleNamespace(n4=n4, tail=n - 4 * n4, sumsq_blocks=sb, sumsq_passes=cdiv(n4, sb * 256) if n4 else 0,
                           update_blocks=ub, update_passes=cdiv(cdiv(n, 4), ub * 256))


def plan_classes(n):
    pl = plan(n)
    cl = {f"tail {pl.tail}", "n < 4" if n < 4 else "n >= 4"}
    cl.add("sumsq clamped" if cdiv(pl.n4, 256 * 8) > SUMSQ_CLAMP else "sumsq unclamped")
    cl.add("update clamped" if cdiv(n, 4096) > UPDATE_CLAMP else "update unclamped")
    if pl.update_passes > 1:
        cl.add("update second pass")
    if pl.sumsq_passes > 1:
        cl.add("sumsq grid-stride")
    if pl.update_blocks > 1:
        cl.add("more than one block")
    return cl


# ----------------------------------------------------------------------------- intervals of fp32 values
class Iv:
    """[lo, hi], float64 arrays holding fp32 values; every operation rounds its real result outward to fp32"""

    def __init__(self, lo, hi=None):
        self.lo = np.asarray(lo, dtype=np.float64)
        self.hi = self.lo if hi is None else np.asarray(hi, dtype=np.float64)

    @staticmethod
    def _out(lo, hi):
        """outward to fp32; a result below the smallest normal number may also arrive as zero (flushed)"""
        lo, hi = f32_down(np.asarray(lo, dtype=np.float64)), f32_up(np.asarray(hi, dtype=np.float64))
        return Iv(np.where((lo > 0) & (lo < TINY), 0.0, lo), np.where((hi < 0) & (hi > -TINY), 0.0, hi))

    def _corners(self, o, f):
        with np.errstate(all="ignore"):
            c = [f(a, b) for a in (self.lo, self.hi) for b in (o.lo, o.hi)]
        return Iv._out(np.minimum.reduce(c), np.maximum.reduce(c))

    def __add__(self, o):
        return Iv._out(self.lo + o.lo, self.hi + o.hi)

    def __sub__(self, o):
        return Iv._out(self.lo - o.hi, self.hi - o.lo)

    def __mul__(self, o):
        return self._corners(o, np.multiply)

    def __truediv__(self, o):
        assert bool(np.all(o.lo > 0))
        return self._corners(o, np.divide)

    def sqrt(self):
        return Iv._out(np.sqrt(self.lo), np.sqrt(self.hi))

    def gather(self, idx):
        """as float32 arrays (the corners are fp32 values): the large case keeps its memory small"""
        return SimpleNamespace(lo=self.lo.astype(f32)[idx], hi=self.hi.astype(f32)[idx])


def _c(x):
    return Iv(np.float64(f32(x)))


def norm_interval(g):
    """g float64 holding fp32 values -> (lo, hi, exact) of sqrtf(S^)"""
    sq = g * g
    S = float(sq.sum())
    n = sq.size
    if bool(exact_sum_rows(sq[None, :])[0]) and bool(np.all(sq.astype(f32).astype(np.float64) == sq)):
        lo = hi = np.float64(S)
        exact = True
    else:
        assert n * U32 < 0.5, "gamma_n is no bound at this n: use gradients whose sums are exact"
        e = F64 * gamma(n) * S
        lo, hi, exact = f32_up(np.float64(S - e)), f32_down(np.float64(S + e)), False
        lo = np.maximum(lo, 0.0)
    return (np.float64(np.sqrt(f32(lo))), np.float64(np.sqrt(f32(hi))), exact)


def coef_interval(norm_lo, norm_hi, max_norm):
    if not f32(max_norm) > 0:
        return _c(1.0)

    def one(nm):
        d = f32(f32(nm) + f32(1e-6))
        return np.float64(min(f32(1.0), f32(f32(max_norm) / d)))
    return Iv(one(norm_hi), one(norm_lo))


@functools.lru_cache(maxsize=None)
def _libm_powf():
    fn = C.CDLL(ctypes.util.find_library("m") or "libm.so.6").powf
    fn.restype, fn.argtypes = C.c_float, (C.c_float, C.c_float)
    return fn


def host_powf(beta, step):
    """powf(beta, (float)step) of the C library the entry point itself calls: one value"""
    return np.float64(_libm_powf()(float(f32(beta)), float(f32(step))))


def pow_interval(beta, step):
    return Iv(host_powf(beta, step))


def bias_corrections(hp, step):
    one = _c(1.0)
    bc1 = one - pow_interval(hp["beta1"], step)
    bc2s = (one - pow_interval(hp["beta2"], step)).sqrt()
    return bc1, bc2s


def update_interval(p, g, m, v, nodecay, coef, hp, step):
    """p, g, m, v: float64 arrays of fp32 values; nodecay: bool per element -> Iv of p', m', v'"""
    one = _c(1.0)
    lr, b1, b2, eps, wd = (_c(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    bc1, bc2s = bias_corrections(hp, step)
    ss = lr / bc1
    gr = Iv(g) * coef
    keep = one - lr * wd                                        # fl32(1 - fl32(lr wd)), or the fma: both inside
    p1 = Iv(p) * keep
    p1 = Iv(np.where(nodecay, p, p1.lo), np.where(nodecay, p, p1.hi))      # w = 0: fl32(p fl32(1 - 0)) = p
    m1 = b1 * Iv(m) + (one - b1) * gr
    v1 = b2 * Iv(v) + ((one - b2) * gr) * gr
    v1 = Iv(np.maximum(v1.lo, 0.0), v1.hi)                     # a sum of non-negative fp32 values
    den = v1.sqrt() / bc2s + eps
    p2 = p1 - (ss * m1) / den
    return p2, m1, v1


# ----------------------------------------------------------------------------- cases
def _gradient(kind, n, rng):
    if kind == "zero":
        return np.zeros(n, f32)
    if kind == "exact":
        g = np.zeros(n, f32)
        hit = rng.random(n) < max(8.0 / n, 1.0 / 512)
        hit[0] = True
        g[hit] = (rng.integers(1, 9, int(hit.sum())) * rng.choice([-1.0, 1.0], int(hit.sum())) / 64.0).astype(f32)
        return g
    big, small = (1.0 * rng.standard_normal(n)).astype(f32), (1e-4 * rng.standard_normal(n)).astype(f32)
    if kind == "big":
        return big
    if kind in ("small", "tiny"):
        return small
    assert kind == "mixed"
    return np.where((np.arange(n) // 5) % 2 == 0, big, small).astype(f32)


def _state(n, rng):
    p = (0.1 * rng.standard_normal(n)).astype(f32)
    m = (0.01 * rng.standard_normal(n)).astype(f32)
    v = (1e-4 * rng.random(n)).astype(f32)
    v[::7] = 0.0
    return p, m, v


@functools.lru_cache(maxsize=None)
def build_case(name):
    c = CASES[name]
    n, kind = c["n"], c["kind"]
    rng = np.random.default_rng(7919 * n + 31 * c["step"] + 1009 * len(kind) + sum(c["nd"]))
    if n > 10 ** 6:
        P = PALETTE
        pp, pm, pv = _state(P, rng)
        pg = _gradient(kind, P, rng)
        idx = (np.arange(n, dtype=np.int64) % P).astype(np.int32)
        p, g, m, v = pp[idx], pg[idx], pm[idx], pv[idx]
        pal = SimpleNamespace(p=pp, g=pg, m=pm, v=pv, idx=idx)
    else:
        p, m, v = _state(n, rng)
        g = _gradient(kind, n, rng)
        if kind == "zero" and n > 7:
            m[7] = f32(0.003)                                   # v = 0, g = 0: the update of this element is m' / eps
        pal = None
    hp = dict(HP, max_norm=c["max_norm"])
    return SimpleNamespace(name=name, n=n, step=c["step"], hp=hp, nd=c["nd"], kind=kind, p=p, g=g, m=m, v=v, pal=pal)


def hp_array(hp):
    return np.array([hp[k] for k in ("lr", "beta1", "beta2", "eps", "wd", "max_norm")], dtype=f32)


def nodecay_mask(n, nd, idx=None):
    i = np.arange(n, dtype=np.int64) if idx is None else idx
    return (i >= nd[0]) & (i < nd[1])


def expected(c):
    """-> {"norm": (lo, hi), "p" / "m" / "v": (lo, hi)} and the flags the records want"""
    g64 = c.g.astype(np.float64)
    nlo, nhi, exact = norm_interval(g64)
    coef = coef_interval(nlo, nhi, c.hp["max_norm"])
    if c.pal is None:
        nd = nodecay_mask(c.n, c.nd)
        out = update_interval(*(a.astype(np.float64) for a in (c.p, c.g, c.m, c.v)), nd, coef, c.hp, c.step)
    else:                                                       # the palette twice: with and without decay
        P = PALETTE
        two = [np.concatenate([a, a]).astype(np.float64) for a in (c.pal.p, c.pal.g, c.pal.m, c.pal.v)]
        pal = update_interval(*two, np.arange(2 * P) >= P, coef, c.hp, c.step)
        sel = c.pal.idx.astype(np.int64) + P * nodecay_mask(c.n, c.nd)
        out = tuple(iv.gather(sel) for iv in pal)
    e = {"norm": (np.array([[nlo]]), np.array([[nhi]]))}
    for k, iv in zip("pmv", out):
        e[k] = (iv.lo[:, None], iv.hi[:, None])
    e["exact_norm"], e["coef"] = exact, coef
    return e


def _nd_cases():
    """no-decay ranges at n = 1,023 (255 float4s and a tail of three): every offset inside a vector of four at both ends"""
    out = {}
    for o in range(4):
        out[f"nd_vec_offset_{o}"] = dict(n=1023, step=2, max_norm=1.0, nd=(8 + o, 20 + o), kind="mixed")
    out["nd_one_element"] = dict(n=1023, step=2, max_norm=1.0, nd=(513, 514), kind="mixed")        # first == last element
    out["nd_ends_in_tail"] = dict(n=1023, step=2, max_norm=1.0, nd=(1000, 1022), kind="mixed")     # tail = 1020..1022
    out["nd_begins_in_tail"] = dict(n=1023, step=2, max_norm=1.0, nd=(1021, 1023), kind="mixed")
    out["nd_begins_at_n"] = dict(n=1023, step=2, max_norm=1.0, nd=(1023, 1030), kind="mixed")
    out["nd_whole"] = dict(n=1023, step=2, max_norm=1.0, nd=(0, 1023), kind="mixed")
    return out


CASES = {
    # n < 4: no float4 at all, one block whose partial sum is 0, everything in the tail
    "n1_step1_clip": dict(n=1, step=1, max_norm=1.0, nd=(0, 0), kind="big"),
    "n3_tiny": dict(n=3, step=1, max_norm=1e-4, nd=(0, 0), kind="tiny"),              # the 1e-6 of the denominator decides
    "n3_nd_inside": dict(n=3, step=2, max_norm=1.0, nd=(1, 2), kind="big"),
    # one float4 exactly, then tails of one and three behind it
    "n4_noclip": dict(n=4, step=1, max_norm=0.0, nd=(0, 0), kind="big"),              # max_norm = 0: no clipping
    "n5_clip": dict(n=5, step=1, max_norm=1.0, nd=(4, 5), kind="big"),                # the tail's square counts in the norm
    "n7_small": dict(n=7, step=2, max_norm=1.0, nd=(0, 0), kind="small"),             # coef is capped at 1
    "n7_negative_max_norm": dict(n=7, step=100000, max_norm=-1.0, nd=(2, 6), kind="mixed"),
    # one block, tail of three
    "n1023_zero_grad": dict(n=1023, step=1, max_norm=1.0, nd=(0, 0), kind="zero"),   # norm = 0; v = 0 and g = 0: m' / eps
    "n1023_step1": dict(n=1023, step=1, max_norm=1.0, nd=(0, 0), kind="mixed"),
    "n1023_late": dict(n=1023, step=100000, max_norm=1.0, nd=(100, 900), kind="mixed"),   # both bias corrections are 1
    "n1023_exact": dict(n=1023, step=2, max_norm=0.015625, nd=(0, 0), kind="exact"),      # the norm is one value
    "n1023_tiny": dict(n=1023, step=2, max_norm=1e-4, nd=(0, 0), kind="tiny"),
    # 4,096 * 4 + 2: five update blocks, two sum-of-squares blocks, a tail of two
    "n16386_clip": dict(n=4096 * 4 + 2, step=2, max_norm=1.0, nd=(4096, 16385), kind="mixed"),
    "n16386_small": dict(n=4096 * 4 + 2, step=100000, max_norm=1.0, nd=(0, 0), kind="small"),
    # just above 8,192 * 4,096, not a multiple of 4: both grid clamps, the grid-stride second pass, exact sums
    "large": dict(n=LARGE_N, step=2, max_norm=1.0, nd=(UPDATE_CLAMP * 4096 - 5, UPDATE_CLAMP * 4096 + 6), kind="exact"),
}
CASES.update(_nd_cases())
SMALL = tuple(k for k in CASES if k != "large")
REQUIRED_CLASSES = {"tail 0", "tail 1", "tail 2", "tail 3", "n < 4", "n >= 4", "sumsq clamped", "sumsq unclamped",
                    "update clamped", "update unclamped", "update second pass", "sumsq grid-stride", "more than one block"}

"""snx_adamw_clip_step (csrc/optimizer.hip: sumsq_partial_kernel, sumsq_final_kernel, adamw_kernel) against the float64
reference of tests/adamw_reference.py, per element.  The C entry point is called through the binding snx/optim.py uses,
but into guarded buffers: 128 guard elements of a NaN sentinel before and after p, m, v and norm_out (norm_out pre-filled
with the sentinel; p, m, v hold the inputs, which the kernel updates in place), the gradient in a guarded buffer as well
(it must come back unchanged), and a scratch of EXACTLY snx_adamw_scratch_bytes, filled with the sentinel, with guards
behind it: a partial sum read from a slot no block wrote would turn the norm, and with it every element, into a NaN.

Per run: guards untouched, every element finite and inside its acceptance set, the gradient unchanged.  A second run
from the same inputs gives the same bits (no atomics).  Where the norm's set is one value (the exact gradients, the zero
gradient) it is met bit for bit.  The argument checks: misaligned pointers, n <= 0, step <= 0, null pointers.

tests/test_adamw_reference_host.py proves on the CPU that the reference admits the kernel's operations in three summation
orders, fused or not, and rejects the planted faults, and that adamw_reference.CASES reaches every tail, clamp and pass
class; which case is there for which seam: the comments of that table.

Measured on an MI355X when this file was added (kernels of commit 9db777b): 25 tests, every element of norm, p, m, v
inside its acceptance set at every case, every bit equality above met; no kernel needed a change.  The widths of the sets
stand in the docstring of tests/adamw_reference.py.  The whole file takes 6 to 8 s, the large case 3.6 to 6.2 s of it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import adamw_reference as A
from tests import rows_reference as R

pytestmark = pytest.mark.gpu
OUTS = ("p", "m", "v")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _column(a, dev):
    """a guarded [n, 1] fp32 buffer holding the fp32 array a"""
    buf, mid = R.guarded(a.size, 1, torch.float32, dev)
    mid.copy_(torch.from_numpy(a).view(-1, 1))
    return buf, mid


def _launch(c, dev):
    from snx._lib import call, fn
    from snx.ops import _p, _stream
    bufs = {k: _column(getattr(c, k), dev) for k in OUTS + ("g",)}
    bufs["norm"] = R.guarded(1, 1, torch.float32, dev)
    nb = int(fn("snx_adamw_scratch_bytes")())
    assert nb == A.SCRATCH_FLOATS * 4
    bufs["scratch"] = R.guarded(nb // 4, 1, torch.float32, dev)
    hp = (C.c_float * 6)(*[float(x) for x in A.hp_array(c.hp)])
    call("snx_adamw_clip_step", _p(bufs["p"][1]), _p(bufs["g"][1]), _p(bufs["m"][1]), _p(bufs["v"][1]), c.n, hp, c.step,
         c.nd[0], c.nd[1], _p(bufs["norm"][1]), _p(bufs["scratch"][1]), _stream())
    return {k: v[0] for k, v in bufs.items()}


def _widths(iv):
    """median and largest number of fp32 values in a set"""
    def o(x):
        b = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(b < 0, -(b & 0x7FFFFFFF), b)
    w = o(iv[1]) - o(iv[0]) + 1
    return f"values per set: median {int(np.median(w))}, most {int(w.max())}"


def _check(c, dev, again=True):
    outs = _launch(c, dev)
    twice = _launch(c, dev) if again else None
    torch.cuda.synchronize()
    exp = A.expected(c)
    R.check_guards(outs["scratch"].cpu(), A.SCRATCH_FLOATS, f"{c.name} scratch")
    g = outs["g"].cpu()
    R.check_guards(g, c.n, f"{c.name} g")
    assert torch.equal(R._raw(g[R.GUARD_ROWS:R.GUARD_ROWS + c.n, 0]), R._raw(torch.from_numpy(c.g))), f"{c.name}: the gradient changed"
    for k in ("norm",) + OUTS:
        st = R.check_guarded(outs[k].cpu(), exp[k], f"{c.name} {k}")
        if k == "norm" and exp["exact_norm"]:
            assert st.single == 1.0                             # one admissible value: this was a bit-for-bit check
        if again:
            assert torch.equal(R._raw(outs[k]), R._raw(twice[k])), f"{c.name} {k}: a second run gave other bits"
    print(f"{c.name}: " + ", ".join(f"{k} {_widths(exp[k])}" for k in ("norm",) + OUTS))


@pytest.mark.parametrize("name", A.SMALL)
def test_adamw_per_element(dev, name):
    _check(A.build_case(name), dev)


def test_adamw_large_crosses_both_clamps(dev):
    """n just above 8,192 * 4,096, n % 4 = 3: 2,048 sum-of-squares blocks of 17 passes, 8,192 update blocks of five"""
    c = A.build_case("large")
    pl = A.plan(c.n)
    assert {"sumsq clamped", "update clamped", "update second pass", "tail 3"} <= A.plan_classes(c.n)
    assert (pl.sumsq_blocks, pl.update_blocks, pl.update_passes) == (2048, 8192, 5)
    _check(c, dev, again=False)


def test_adamw_argument_checks(dev):
    from snx._lib import CONSTANTS, fn
    from snx.ops import _p, _stream
    f = fn("snx_adamw_clip_step")
    t = {k: torch.zeros(16, device=dev) for k in ("p", "g", "m", "v", "norm")}
    scratch = torch.zeros(A.SCRATCH_FLOATS, device=dev)
    hp = (C.c_float * 6)(*[float(x) for x in A.hp_array(dict(A.HP, max_norm=1.0))])

    def run(n=8, step=1, **over):
        a = {k: _p(over.get(k, v)) for k, v in t.items()}
        return f(a["p"], a["g"], a["m"], a["v"], n, hp, step, 0, 0, a["norm"], _p(over.get("scratch", scratch)), _stream())

    E_ARG, E_SHAPE = CONSTANTS["SNX_E_ARG"], CONSTANTS["SNX_E_SHAPE"]
    assert run() == 0
    assert run(n=0) == E_SHAPE and run(n=-4) == E_SHAPE and run(step=0) == E_SHAPE and run(step=-1) == E_SHAPE
    for k in ("p", "g", "m", "v"):
        assert run(**{k: t[k][1:]}) == E_ARG, f"{k} misaligned by 4 bytes"
        assert run(**{k: None}) == E_ARG, f"{k} null"
    assert run(norm=None) == E_ARG and run(scratch=None) == E_ARG
    torch.cuda.synchronize()
    for k in ("p", "m", "v"):
        assert bool((t[k] == 0).all()), f"{k} was written by a refused or zero-gradient call"

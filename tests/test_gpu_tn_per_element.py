"""The weight-gradient ("TN") GEMM family against the reference of tests/tn_reference.py, per element: snx_gemm_tn_accum,
snx_gemm_tn_accum_interleaved and snx_gemm_tn_accum_group in both kernel forms -- the 256x256 persistent kernel with its
ordered reduce, forced onto small token ranges ("tn256" 1, "tn256_min_m" 1) and once at the default switches, and the
128x128 token-split kernel ("tn256" 0) -- in both input families and both flush modes ("det_reduce" 1 and 0).  The C entry
points are called as snx.ops calls them, but into guarded buffers: dW inside 128 rows of a NaN sentinel, its body holding
dW0; dY and X between 128 rows of bf16 NaN; the workspace exactly snx_gemm_tn_workspace_bytes() bytes of the fp32 NaN
sentinel with a guard behind.  Every switch is restored on the way out of the block that set it (Switches).

Per run: all guards untouched (dW, workspace), every element finite and inside its set.  Exact family: every element equal
to THE value bit for bit -- no assumption about the MFMA, the tree or the arrival order of atomics; "det_reduce" 0 gives the
bits of 1; two launches into the same dW give dW0 + 2 sum, as bits.  With "det_reduce" 1 a second run gives the same bits,
"stream_nt" 0 gives the bits of 1, the grouped launch and the single-problem entry give the same bits on one-problem rows,
and the interleaved entry on dY[:, perm] gives the bits the plain entry gives on the natural-order dY.
tests/test_tn_reference_host.py proves on the CPU that the plans restated in tn_reference are the library's and agree with
themselves, that the tables reach every class, and that the reference rejects the planted faults.

The rows (128, 128) with M = 1 and 63 under "tn256_min_m" 1 are the tests of the dispatch fix in launch_tn_group: before
it those calls returned SNX_E_ARG (the 256 form was offered zero K-steps and demanded P x ntiles slabs of a workspace
advertised as 0 bytes).

Measured on an MI355X when this file was added (kernels of commit e0eeae8 plus that dispatch fix; no kernel arithmetic
changed): 34 tests, 207 launches, nothing outside its set and no guard touched.  Elements copied back and checked on the
CPU (the first run, the two-launch run and the atomic run of each test; every other run is compared with the first as
bits on the device):
    form      family   tests   launches   elements     pinned to one value
    256x256   exact    16      111        87,588,864   100 %   (each met it: bit for bit, "det_reduce" 1 and 0)
              random    7       29         1,245,184   0 %     (sets of M + c + 8 roundings: wider than two values everywhere)
    128x128   exact     7       49         3,588,096   100 %
              random    4       18           638,976   0 %
93,061,120 elements in all, 97.98 % of them pinned to one value.  The whole file takes 5.0 s, the slowest test 0.47 s
(the 149 M layer group at 1,408 rows).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import tn_reference as T

pytestmark = pytest.mark.gpu
SWITCHES = ("tn256", "tn256_min_m", "det_reduce", "stream_nt")
GR = T.GUARD_ROWS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Switches:
    """the family's process switches (and a CU reservation) for the duration of a block; everything back in place afterwards"""

    def __init__(self, reserved=0, **kw):
        assert set(kw) <= set(SWITCHES)
        self.kw, self.reserved = kw, reserved

    def __enter__(self):
        import snx
        from snx._lib import fn
        self.saved = {k: snx.config(k) for k in SWITCHES}
        self.saved_reserved = fn("snx_get_reserved_cus")()
        try:
            snx.configure(**self.kw)
            assert fn("snx_set_reserved_cus")(self.reserved) == 0
            assert fn("snx_get_reserved_cus")() == T.cdiv(self.reserved, 8) * 8
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        import snx
        from snx._lib import fn
        fn("snx_set_reserved_cus")(self.saved_reserved)
        snx.configure(**self.saved)
        return False


class Tally:
    def __init__(self):
        self.n = self.one = self.two = self.wide = self.runs = 0

    def add(self, st):
        self.n += st.n
        self.one += st.single * st.n
        self.two += st.two * st.n
        self.wide += st.wide * st.n

    def __str__(self):
        return (f"{self.runs} launches, {self.n} elements checked on the CPU, one {self.one / max(self.n, 1):.3%}, two "
                f"{self.two / max(self.n, 1):.3%}, wider {self.wide / max(self.n, 1):.3%} | {self.n} {self.one:.0f} {self.two:.0f}")


@functools.lru_cache(maxsize=2)
def _device_case(family, group, M):
    c = T.build_case(family, T.norm_group(group), M)
    d = dict(dY=[t.cuda() for t in c.dY], X=[t.cuda() for t in c.X], dW0=[t.cuda() for t in c.dW0],
             want=[t.cuda() for t in c.want])
    return c, d


def _natural_dy(c, d, p):
    """guarded device copy of problem p's dY with its columns in the natural row order"""
    N = c.group[p][0]
    buf, mid = T.guarded(c.M, N, T.BF16, d["dY"][p].device)
    mid.copy_(d["dY"][p][GR:GR + c.M][:, torch.from_numpy(np.argsort(T.src_rows(N))).to(buf.device)])
    return buf


def _run(c, d, tally, entry="group", launches=1, natural=False):
    """launch into fresh guarded gradients and a fresh exact-size workspace; guards checked; -> the dW bodies (device)"""
    from snx._lib import call, fn
    from snx.ops import TnProblem, _p, _stream
    dev, n, M = d["X"][0].device, len(c.group), c.M
    sizes = (TnProblem * n)(*[TnProblem(0, 0, 0, N, K, inter, 0) for N, K, inter in c.group])
    nbytes = int(fn("snx_gemm_tn_workspace_bytes")(sizes, n, M))
    assert nbytes == T.workspace_bytes(c.group, M)
    ws = T.workspace(nbytes, dev)
    wsp = _p(ws) if nbytes else C.c_void_p(0)
    bufs = [T.guarded_dw(dw0, dev) for dw0 in d["dW0"]]
    dys = [_natural_dy(c, d, p) if natural else d["dY"][p] for p in range(n)]
    mids = lambda t: t[GR:GR + M]                                              # noqa: E731
    for _ in range(launches):
        if entry == "group":
            assert not natural
            arr = (TnProblem * n)(*[TnProblem(mids(dys[p]).data_ptr(), mids(d["X"][p]).data_ptr(), bufs[p][1].data_ptr(), N, K, inter, 0)
                                    for p, (N, K, inter) in enumerate(c.group)])
            call("snx_gemm_tn_accum_group", arr, n, M, wsp, nbytes, _stream())
        else:
            assert n == 1
            N, K, inter = c.group[0]
            name = "snx_gemm_tn_accum_interleaved" if inter and not natural else "snx_gemm_tn_accum"
            call(name, _p(mids(dys[0])), _p(mids(d["X"][0])), _p(bufs[0][1]), M, N, K, wsp, nbytes, _stream())
    torch.cuda.synchronize()
    tally.runs += launches
    what = f"{c.family} {c.group} M={M} {entry}"
    T.check_workspace(ws, nbytes, what)
    for p, (buf, _) in enumerate(bufs):
        T.check_guards(buf, c.group[p][0], f"{what} dW[{p}]")
    return bufs


def _same(a, b, what):
    for p, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(T._raw(x[1]), T._raw(y[1])), f"{what}: other bits in problem {p}"


def _check(c, plan, bufs, tally, what, launches=1):
    for p, ((buf, mid), iv) in enumerate(zip(bufs, T.expected(c, plan, launches))):
        st = T.check_guarded(buf.cpu(), iv, f"{what} dW[{p}]")
        tally.add(st)
        if c.family == "exact":
            assert st.single == 1.0                                              # one admissible value: a bit-for-bit check


def _all_checks(c, d, plan, sw, reserved, atomics, what):
    tally = Tally()
    one = len(c.group) == 1
    with Switches(reserved, det_reduce=1, stream_nt=1, **sw):
        first = _run(c, d, tally)
        _check(c, plan, first, tally, what)
        if c.family == "exact":
            for (_, mid), want in zip(first, d["want"]):
                assert torch.equal(T._raw(mid), T._raw(want))
        _same(first, _run(c, d, tally), f"{what}: a second run")
        if one:
            _same(first, _run(c, d, tally, entry="single"), f"{what}: the single-problem entry point")
            if c.group[0][2]:
                _same(first, _run(c, d, tally, entry="single", natural=True), f"{what}: the plain entry on natural-order dY")
        if c.family == "exact":
            twice = _run(c, d, tally, launches=2)
            _check(c, plan, twice, tally, f"{what} two launches", launches=2)
    with Switches(reserved, det_reduce=1, stream_nt=0, **sw):
        _same(first, _run(c, d, tally), f"{what}: stream_nt 0")
    if atomics:
        with Switches(reserved, det_reduce=0, stream_nt=1, **sw):
            at = _run(c, d, tally)
            _check(c, plan, at, tally, f"{what} atomics")
            if c.family == "exact":
                _same(first, at, f"{what}: det_reduce 0")
                if one:
                    _same(first, _run(c, d, tally, entry="single"), f"{what}: det_reduce 0, single-problem entry")
    print(f"{what}: {tally}")


def _params(table, marks_at):
    out = []
    for row in table:
        marks = row[marks_at]
        name = "+".join(f"{N}x{K}{'i' if inter else ''}" for N, K, inter in T.norm_group(row[0])) + f"-M{row[1]}"
        out.append(pytest.param(*row[:marks_at - 1], "exact", T.ATOM in marks, id=f"{name}-exact"))
        if T.RND in marks:
            out.append(pytest.param(*row[:marks_at - 1], "random", T.RND_ATOM in marks, id=f"{name}-random"))
    return out


@pytest.mark.parametrize("group,M,reserved,family,atomics", _params(T.CASES_256, 4))
def test_256_form_per_element(dev, group, M, reserved, family, atomics):
    plan = T.dispatch(group, M, 1, 1, reserved)
    c, d = _device_case(family, group, M)
    _all_checks(c, d, plan, dict(tn256=1, tn256_min_m=1), reserved, atomics, f"256 form {family} {group} M={M} reserved {reserved}")


def test_256_form_at_the_default_switches(dev):
    import snx
    group, M, reserved, _ = T.CASE_DEFAULT
    assert (snx.config("tn256"), snx.config("tn256_min_m")) == (1, 8192)
    plan = T.dispatch(group, M, 1, 8192, reserved)
    c, d = _device_case("exact", group, M)
    _all_checks(c, d, plan, {}, reserved, True, f"256 form at the defaults, exact {group} M={M}")


@pytest.mark.parametrize("group,M,family,atomics", _params(T.CASES_128, 3))
def test_128_form_per_element(dev, group, M, family, atomics):
    plan = T.tn128_plan(group, M)
    c, d = _device_case(family, group, M)
    _all_checks(c, d, plan, dict(tn256=0), 0, atomics, f"128 form {family} {group} M={M}")

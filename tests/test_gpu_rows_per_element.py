"""The LayerNorm kernel family against the float64 reference of tests/rows_reference.py, per element: the four forward
entry points (snx_ln_fwd, snx_ln_fwd_add, snx_embed_ln_fwd, snx_gelu_ln_fwd), snx_ln_bwd in accumulate and overwrite mode
with and without dh_bf16, snx_gelu_ln_bwd and snx_embed_ln_bwd, at all four widths (NV = 1..4), with the ordered reduce
("det_reduce" 1) and the float atomics (0), with and without the non-temporal streams ("stream_nt").  The C entry points
are called as snx.ops calls them, but into guarded buffers: 128 guard rows of a NaN sentinel before and after every
output, the output itself pre-filled with it (or with the non-zero value it is accumulated into), and a workspace of
EXACTLY the advertised size -- snx_ln_bwd_workspace_bytes / snx_embed_ln_bwd_workspace_bytes, 256-byte rows -- with guards
behind it.  Every switch is restored on the way out of the block that set it (Switches).

Per run: guards untouched, every element written and finite and inside its acceptance set.  Bit equalities: h_out of the
add mode is fl32(h + float(y)); x0 == bf16(h_out); dh_bf16 == bf16(dh as stored); overwrite mode ignores the sentinel dh
held; the pad row and the rows of ids that do not occur keep gradE's initial bits; a second run gives the same bits
("det_reduce" 1); "stream_nt" 0 gives the bits of 1; the same launch with its rows reversed gives the reversed bits of x,
h_out, dh and dd (dw is exempt: its order changes).  tests/test_rows_reference_host.py proves on the CPU that the
reference admits the kernels' cast points in any summation order and rejects the planted faults, and that the case
tables reach every class (through ln_bwd_plan / reduce_split, asserted again here for the large cases).

Which case is there for which seam: rows_reference.FWD_T / BWD_T / BWD_LARGE / EMBED_BWD and their comments.

Measured on an MI355X when this file was added (kernels of commit 0431e50): 74 tests, every element of every output
inside its acceptance set at every width, mode and launch form, every bit equality above met; no kernel needed a
change.  The shares per entry point stand in the docstring of tests/rows_reference.py.  The whole file takes 9 s, the
slowest test 1.7 s.
"""
import functools

import pytest
import torch

from tests import rows_reference as R

pytestmark = pytest.mark.gpu
SWITCHES = ("stream_nt", "det_reduce")
INPUTS = ("h", "y", "d", "E", "ids", "w", "dy", "dyf", "dh0", "dw0", "gE0")
LN_BWD = R.BWD_ENTRIES[:4]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _device_inputs(c):
    return {k: getattr(c, k).cuda() for k in INPUTS}


@functools.lru_cache(maxsize=3)
def _case(T, H, eps=1e-5, kind="fwd"):
    c = R.build_case(T, H, eps, kind)
    return c, _device_inputs(c)


class Switches:
    """snx_configure switches for the duration of a block; everything back in place afterwards"""

    def __init__(self, **kw):
        assert set(kw) <= set(SWITCHES)
        self.kw = kw

    def __enter__(self):
        import snx
        self.saved = {k: snx.config(k) for k in SWITCHES}
        try:
            snx.configure(**self.kw)
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        import snx
        snx.configure(**self.saved)
        return False


def _workspace(nbytes, dev):
    assert nbytes > 0 and nbytes % 256 == 0
    return R.guarded(nbytes // 256, 64, torch.float32, dev), nbytes


def _launch(c, d, entry):
    """one entry point into fresh guarded buffers, as snx.ops calls it -> ({output name: guarded buffer}, workspace or None)"""
    from snx._lib import call, fn
    from snx.ops import _p, _stream
    T, H, dev = c.T, c.H, d["w"].device
    bufs, ws, nb = {}, None, 0

    def out(name, rows, dtype, init=None):
        bufs[name] = R.guarded(rows, H, dtype, dev)
        if init is not None:
            bufs[name][1].copy_(init)
        return _p(bufs[name][1])

    if entry == "ln_fwd":
        call("snx_ln_fwd", _p(d["h"]), _p(d["w"]), out("x", T, R.BF16), T, H, c.eps, _stream())
    elif entry == "ln_fwd_add":
        call("snx_ln_fwd_add", _p(d["h"]), _p(d["y"]), _p(d["w"]), out("h_out", T, torch.float32), out("x", T, R.BF16), T, H,
             c.eps, _stream())
    elif entry == "embed_ln_fwd":
        call("snx_embed_ln_fwd", _p(d["ids"]), _p(d["E"]), _p(d["w"]), out("h_out", T, torch.float32), out("x0", T, R.BF16),
             T, H, c.eps, _stream())
    elif entry == "gelu_ln_fwd":
        call("snx_gelu_ln_fwd", _p(d["d"]), _p(d["w"]), out("x", T, R.BF16), T, H, c.eps, _stream())
    elif entry in LN_BWD:
        acc = entry.startswith("ln_bwd_acc")
        (ws, _), nb = _workspace(int(fn("snx_ln_bwd_workspace_bytes")(T, H)), dev)
        dh = out("dh", T, torch.float32, d["dh0"] if acc else None)                # overwrite: the sentinel stays in place
        dhb = out("dh_bf16", T, R.BF16) if entry.endswith("_bf16") else _p(None)
        call("snx_ln_bwd", _p(d["dy"]), _p(d["h"]), _p(d["w"]), dh, dhb, out("dw", 1, torch.float32, d["dw0"]), T, H, c.eps,
             int(not acc), _p(ws[R.GUARD_ROWS:]), nb, _stream())
    elif entry == "gelu_ln_bwd":
        (ws, _), nb = _workspace(int(fn("snx_ln_bwd_workspace_bytes")(T, H)), dev)
        call("snx_gelu_ln_bwd", _p(d["dy"]), _p(d["d"]), _p(d["w"]), out("dd", T, R.BF16), out("dw", 1, torch.float32, d["dw0"]),
             T, H, c.eps, _p(ws[R.GUARD_ROWS:]), nb, _stream())
    else:
        assert entry == "embed_ln_bwd"
        (ws, _), nb = _workspace(int(fn("snx_embed_ln_bwd_workspace_bytes")(T, H, c.V)), dev)
        call("snx_embed_ln_bwd", _p(d["dyf"]), _p(d["ids"]), _p(d["E"]), _p(d["w"]), out("gradE", c.V, torch.float32, d["gE0"]),
             out("dw", 1, torch.float32, d["dw0"]), T, H, c.V, c.eps, c.pad, _p(ws[R.GUARD_ROWS:]), nb, _stream())
    return {k: v[0] for k, v in bufs.items()}, (ws, nb)


class Tally:
    """bf16 outputs: shares of elements with one, two, more admissible values; fp32 outputs: the worst |got - v| / B"""

    def __init__(self):
        self.n = self.one = self.two = self.wide = self.n32 = 0
        self.worst = 0.0

    def add(self, st, buf, iv, ratio=True):
        if buf.dtype == R.BF16:
            self.n += st.n
            self.one += st.single * st.n
            self.two += st.two * st.n
            self.wide += st.wide * st.n
        elif ratio:                                              # not fl32(dh0 + dx): its corners are rounded values
            lo, hi = iv[0], iv[1]
            half = (hi - lo) / 2
            err = abs(R.to_np(_mid(buf)) - (lo + hi) / 2)
            self.n32 += st.n
            self.worst = max(self.worst, float((err[half > 0] / half[half > 0]).max(initial=0.0)))

    def __str__(self):
        n = max(self.n, 1)
        return (f"bf16 {self.n} elements, one {self.one / n:.3%}, two {self.two / n:.3%}, wider {self.wide / n:.3%}; "
                f"fp32 {self.n32} elements, worst |got - v| / B {self.worst:.3f}")


def _mid(buf):
    return buf[R.GUARD_ROWS:buf.shape[0] - R.GUARD_ROWS]


def _run_and_check(c, d, entry, what, tally=None, again=True, inputs_untouched=True):
    """run, check every output against the reference and the exact relations; a second run for the same bits"""
    outs, (ws, nb) = _launch(c, d, entry)
    twice = _launch(c, d, entry)[0] if again else None
    torch.cuda.synchronize()
    exp = (R.expected_fwd if entry in R.FWD_ENTRIES else R.expected_bwd)(c, entry)
    assert set(exp) == set(outs)
    if ws is not None:
        R.check_guards(ws.cpu(), nb // 256, f"{what} {entry} workspace")
    for k, buf in outs.items():
        host = buf.cpu()
        st = R.check_guarded(host, exp[k], f"{what} {entry} {k}")
        if tally is not None:
            tally.add(st, host, exp[k], ratio=not (entry.startswith("ln_bwd_acc") and k == "dh"))
        if entry == "ln_fwd_add" and k == "h_out":
            assert st.single == 1.0                              # fl32(h + float(y)): this was a bit-for-bit check
        if again:
            assert torch.equal(R._raw(buf), R._raw(twice[k])), f"{what} {entry} {k}: a second run gave other bits"
    if entry == "embed_ln_fwd":
        assert torch.equal(R._raw(_mid(outs["x0"])), R._raw(_mid(outs["h_out"]).to(R.BF16))), f"{what}: x0 != bf16(h_out)"
    if "dh_bf16" in outs:
        assert torch.equal(R._raw(_mid(outs["dh_bf16"])), R._raw(_mid(outs["dh"]).to(R.BF16))), f"{what} {entry}: dh_bf16 != bf16(dh)"
    if entry == "embed_ln_bwd":
        idle = torch.ones(c.V, dtype=torch.bool)
        idle[c.ids[c.ids != c.pad]] = False                      # the pad row and every id that does not occur
        assert idle[c.pad] and torch.equal(R._raw(_mid(outs["gradE"]).cpu()[idle]), R._raw(c.gE0[idle])), f"{what}: an idle gradE row changed"
    for k in INPUTS if inputs_untouched else ():
        assert torch.equal(d[k].cpu(), getattr(c, k)), f"{what} {entry}: input {k} changed"
    return outs


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("H", R.WIDTHS)
@pytest.mark.parametrize("entry", R.FWD_ENTRIES)
def test_forward_per_element(dev, entry, H):
    tally = Tally()
    for T in R.FWD_T:
        for eps in R.EPS:
            c, d = _case(T, H, eps)
            _run_and_check(c, d, entry, f"T {T} H {H} eps {eps}", tally)
    print(f"{entry} H {H}: {tally}")


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize("H", R.WIDTHS)
@pytest.mark.parametrize("entry", R.BWD_ENTRIES[:5])
def test_backward_per_element(dev, entry, H):
    tally = Tally()
    with Switches(det_reduce=1):
        for T in R.BWD_T:
            for eps in R.EPS:
                c, d = _case(T, H, eps)
                _run_and_check(c, d, entry, f"T {T} H {H} eps {eps}", tally)
    print(f"{entry} H {H}: {tally}")


@pytest.mark.parametrize("entries", [LN_BWD, ("gelu_ln_bwd",)], ids=["ln_bwd", "gelu_ln_bwd"])
@pytest.mark.parametrize("T,H,classes,plan", R.BWD_LARGE)
def test_backward_large(dev, T, H, classes, plan, entries):
    """the launch arithmetic: the workspace ceiling, a last block with a partial second trip, three trips per wave"""
    from snx import fn
    assert set(classes) <= R.plan_classes(T) and R.ln_bwd_plan(T)[:3] == plan
    assert fn("snx_ln_bwd_workspace_bytes")(T, H) == R.ln_bwd_plan(T)[3] * H * 4
    c, d = _case(T, H)
    with Switches(det_reduce=1):
        for entry in entries:
            tally = Tally()
            _run_and_check(c, d, entry, f"T {T} H {H}", tally, inputs_untouched=False)
            print(f"{entry} T {T} H {H}: {tally}")


@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("T,H,kind", R.EMBED_BWD)
def test_embed_backward_per_element(dev, T, H, kind, det):
    tally = Tally()
    with Switches(det_reduce=det):
        for eps in R.EPS if T <= 131 else R.EPS[:1]:
            c, d = _case(T, H, eps, kind)
            _run_and_check(c, d, "embed_ln_bwd", f"T {T} H {H} eps {eps} det_reduce {det}", tally, again=bool(det))
    print(f"embed_ln_bwd T {T} H {H} det_reduce {det}: {tally}")


# ----------------------------------------------------------------------------- launch forms
@pytest.mark.parametrize("T,H", [(67, H) for H in R.WIDTHS] + [(4101, 256)])
def test_float_atomics_stay_inside_the_same_sets(dev, T, H):
    """ "det_reduce" 0: dw by one float atomic per column and block, arrival order -- the same sets, no bit-reproducibility"""
    c, d = _case(T, H)
    with Switches(det_reduce=0):
        for entry in ("ln_bwd_acc_bf16", "ln_bwd_ow", "gelu_ln_bwd"):
            _run_and_check(c, d, entry, f"T {T} H {H} det_reduce 0", again=False, inputs_untouched=T < 1000)


@pytest.mark.parametrize("T,H", [(67, H) for H in R.WIDTHS] + [(4101, 256)])
def test_stream_nt_off_gives_the_bits_of_on(dev, T, H):
    c, d = _case(T, H)
    runs = []
    for nt in (1, 0):
        with Switches(stream_nt=nt, det_reduce=1):
            runs.append({e: _run_and_check(c, d, e, f"T {T} H {H} stream_nt {nt}", again=False, inputs_untouched=T < 1000)
                         for e in ("ln_fwd_add", "ln_bwd_acc_bf16", "ln_bwd_ow_bf16")})
    for e, outs in runs[0].items():
        for k, buf in outs.items():
            assert torch.equal(R._raw(buf), R._raw(runs[1][e][k])), f"{e} {k}: stream_nt 0 gave other bits"


@pytest.mark.parametrize("H", R.WIDTHS)
def test_rows_are_independent(dev, H):
    """the same launch with its rows reversed returns the reversed bits (dw, gradE: exempt, their order changes)"""
    c, d = _case(67, H)
    cr = R.reversed_case(c)
    dr = _device_inputs(cr)
    with Switches(det_reduce=1):
        for entry in R.FWD_ENTRIES + R.BWD_ENTRIES[:5]:
            a, b = _launch(c, d, entry)[0], _launch(cr, dr, entry)[0]
            torch.cuda.synchronize()
            for k in set(a) - {"dw"}:
                assert torch.equal(R._raw(_mid(a[k])), torch.flip(R._raw(_mid(b[k])), dims=(0,))), f"{entry} {k}: rows depend on their place"

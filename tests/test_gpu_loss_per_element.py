"""snx_loss_fwd / snx_loss_bwd (csrc/loss.hip: three forward launches, one backward launch) against the float64 reference
of tests/loss_reference.py, per element, in both `bf16_mm` modes and all three input families.  The C entry points are
called through the binding snx/loss.py uses, but into guarded buffers: 128 guard rows of a NaN sentinel before and after
dq, dp, dn and out9, the outputs pre-filled with it, and a workspace of EXACTLY snx_loss_workspace_bytes, filled with the
sentinel before the forward, with guards behind it: a read of a slot nobody wrote surfaces as a NaN.

Per run: guards untouched; every element of dq, dp, dn and the nine scalars written, finite and inside its acceptance
set; the gradient coefficients G the forward left in the workspace inside theirs (a bf16-rounded quantity in bf16 mode:
its shares of one / two / more admissible values are printed); the inputs unchanged.  Bit equalities: a second run gives
the same bits (no atomics); remote dp rows with at most one coefficient, and dn with lam_neg = 0, are the bits of their
single fp32 expression; out[6] and out[7] are one value; with every lambda 0 and no teachers out[0] == out[1]; in the
exact_a family the planted tie shows in G -- the two probabilities of anchor 0 are equal in bf16 mode and differ in fp32
mode --; through snx.loss.splade_loss the three gradients are adjacent row ranges of one storage.  The shapes whose
dynamic LDS exceeds 64 KiB are launched in a test function of their own, collected last.

tests/test_loss_reference_host.py proves on the CPU that the reference admits the kernel's cast points in three summation
orders with expf / logf moved by the assumed ulps, rejects the 21 planted faults, and that the case table reaches every
pick_ch, nchunk, ragged, clamp and LDS class; which case is there for which seam: the comments of loss_reference.CASES.

Measured on an MI355X when this file was added (kernels of commit 9db777b): 38 tests, every element of every output and
of G inside its acceptance set in both modes, every bit equality above met, the launches of 83,200 / 131,840 / 135,296 B
of dynamic LDS accepted by the runtime; no kernel needed a change.  The shares stand in the docstring of
tests/loss_reference.py.  The whole file takes 5.7 s, the slowest test 0.5 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_reference as L
from tests import rows_reference as R
from tests.gemm_reference import bf16_ord

pytestmark = pytest.mark.gpu
TALLY = {"n": 0, "zero": 0, "one": 0, "two": 0, "wide": 0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _launch(c, d, mode):
    """forward and backward into fresh guarded buffers -> {name: guarded buffer}, workspace floats"""
    from snx._lib import call, fn
    from snx.ops import _p, _stream
    dev = d["q"].device
    nb = int(fn("snx_loss_workspace_bytes")(c.B, c.Bp, c.k, c.V))
    assert nb == L.workspace_bytes(c.B, c.Bp, c.k, c.V) and nb % 4 == 0
    bufs = {"ws": R.guarded(nb // 4, 1, torch.float32, dev), "out9": R.guarded(1, 9, torch.float32, dev),
            "dq": R.guarded(c.B, c.V, torch.float32, dev), "dp": R.guarded(c.Bp, c.V, torch.float32, dev),
            "dn": R.guarded(c.B * c.k, c.V, torch.float32, dev)}
    dims = (C.c_int32 * 6)(c.B, c.Bp, c.k, c.V, c.off, int(mode))
    hp = (C.c_float * 7)(*[float(x) for x in c.hp])
    call("snx_loss_fwd", _p(d["q"]), _p(d["p"]), _p(d["n"]), _p(d["tpos"]), _p(d["tneg"]), _p(d["tsc"]), hp, dims,
         _p(bufs["ws"][1]), _p(bufs["out9"][1]), _stream())
    call("snx_loss_bwd", _p(d["q"]), _p(d["p"]), _p(d["n"]), _p(d["gout"]), hp, dims, _p(bufs["ws"][1]),
         int(d["tsc"] is not None and c.hp[5] > 0), _p(bufs["dq"][1]), _p(bufs["dp"][1]), _p(bufs["dn"][1]), _stream())
    return {k: v[0] for k, v in bufs.items()}, nb // 4


def _G_of(ws, c):
    """the coefficients G [B, Bp] in the workspace (the layout of `carve`, restated)"""
    nchunk = L.cdiv(c.V, c.CH)
    o = nchunk * (c.B * c.Bp + c.B * c.k + c.B + 8) + 3 * c.V
    return ws[R.GUARD_ROWS + o:R.GUARD_ROWS + o + c.B * c.Bp, 0].reshape(c.B, c.Bp)


def _bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(R.BF16).float().numpy()


def _single_expression_rows(c, mode, ws, g, outs, what):
    """rows whose contract is ONE fp32 expression with no sum in it are met bit for bit: a remote dp row whose column of G
    holds at most one non-zero coefficient is go fl32-times [bf16](G_ij [bf16](q_ic)) (or zero); with lam_neg = 0 a dn row is
    go fl32-times fl32(Gh_r q_ic) (a product fused with a zero addend is the same value)"""
    f32 = np.float32
    rb = _bf if mode else (lambda x: x)
    go = f32(c.gout)
    mid = lambda k: outs[k].cpu()[R.GUARD_ROWS:-R.GUARD_ROWS].numpy()
    remote = [j for j in range(c.Bp) if not c.off <= j < c.off + c.B and np.count_nonzero(g[:, j]) <= 1
              and not np.any((g[:, j] != 0) & (np.abs(g[:, j]) < 2.0 ** -100))]      # keep clear of subnormal products
    if remote:
        dp = mid("dp")
        for j in remote:
            i = int(np.argmax(g[:, j] != 0))
            want = (go * rb((f32(g[i, j]) * rb(c.q[i])).astype(f32))).astype(f32)
            assert want.tobytes() == dp[j].tobytes() or np.array_equal(want, dp[j]), f"{what}: remote dp row {j} is not its single expression"
    if c.hp[3] == 0:
        o = L.cdiv(c.V, c.CH) * (c.B * c.Bp + c.B * c.k + c.B + 8) + 3 * c.V + c.B * c.Bp
        gh = ws[R.GUARD_ROWS + o:R.GUARD_ROWS + o + c.B * c.k, 0].numpy()
        want = (go * (gh[:, None] * c.q[np.arange(c.B * c.k) // c.k]).astype(f32)).astype(f32)
        assert np.array_equal(want, mid("dn")), f"{what}: dn is not go fl32(Gh q) with lam_neg = 0"
    return len(remote)


def _run_and_check(name, family, dev, again=True):
    c = L.build_case(name, family)
    d = {k: _t(getattr(c, k), dev) for k in ("q", "p", "n", "tpos", "tneg", "tsc")}
    d["gout"] = torch.tensor([c.gout], dtype=torch.float32, device=dev)
    G = {}
    for mode in (0, 1):
        what = f"{name} {family} bf16_mm {mode}"
        outs, nws = _launch(c, d, mode)
        twice = _launch(c, d, mode)[0] if again else None
        torch.cuda.synchronize()
        exp = L.expected(c, mode)
        ws = outs["ws"].cpu()
        R.check_guards(ws, nws, f"{what} workspace")
        for k in ("out9", "dq", "dp", "dn"):
            R.check_guarded(outs[k].cpu(), exp[k], f"{what} {k}")
            if again:
                assert torch.equal(R._raw(outs[k]), R._raw(twice[k])), f"{what} {k}: a second run gave other bits"
        o9 = outs["out9"].cpu()[R.GUARD_ROWS].numpy()
        lo, hi = exp["out9"]
        assert lo[0, 6] == hi[0, 6] == o9[6] and lo[0, 7] == hi[0, 7] == o9[7], f"{what}: the non-zero counts are not exact"
        if not np.any(c.hp[1:6]):
            assert o9[0].tobytes() == o9[1].tobytes(), f"{what}: loss != infonce with every lambda 0"
        g = R.to_np(_G_of(ws, c))
        m = exp["mid"]
        bad = np.argwhere(~((g >= m.G.lo) & (g <= m.G.hi)))
        assert len(bad) == 0, f"{what}: {len(bad)} coefficients G outside their set, first {tuple(bad[0])}: {g[tuple(bad[0])]!r}"
        if mode:
            w = bf16_ord(m.G.hi) - bf16_ord(m.G.lo) + 1
            zero = (np.abs(m.G.lo) <= L.BF16_TINY) & (np.abs(m.G.hi) <= L.BF16_TINY)      # zero, or a value below 2^-120
            w = np.where(zero, 0, w)
            TALLY["n"] += w.size
            TALLY["zero"] += int(zero.sum())
            TALLY["one"] += int((w == 1).sum())
            TALLY["two"] += int((w == 2).sum())
            TALLY["wide"] += int((w > 2).sum())
        G[mode] = g
        _single_expression_rows(c, mode, ws, g, outs, what)
        for k in ("q", "p", "n"):
            assert torch.equal(d[k].cpu(), torch.from_numpy(getattr(c, k))), f"{what}: input {k} changed"
    if family == "exact_a" and c.tie is not None and c.hp[0] == 1.0:
        j1, j2 = c.tie
        gs = float(np.float32(1.0) / np.float32(c.B))
        assert G[1][0, j2] > 0.2 * gs, f"{name}: the tie carries no probability in bf16 mode"
        # equal scores, equal expf: bf16((e - 1) gs) + gs against bf16(e gs), two bf16 roundings of at most 2^-9 gs each
        assert abs((G[1][0, j1] + gs) - G[1][0, j2]) <= 2.0 ** -8 * gs, f"{name}: bf16 mode does not see the planted tie"
        assert G[0][0, j1] + gs != G[0][0, j2], f"{name}: fp32 mode sees a tie that is not there"
    n = max(TALLY["n"], 1)
    print(f"{name} {family}: G in bf16 mode so far: {TALLY['n']} elements, zero or below 2^-120 {TALLY['zero'] / n:.3%}, "
          f"one value {TALLY['one'] / n:.3%}, two "
          f"{TALLY['two'] / n:.3%}, more {TALLY['wide'] / n:.3%}")


@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("name", list(L.CASES))
def test_loss_per_element(dev, name, family):
    _run_and_check(name, family, dev)


def test_loss_argument_checks(dev):
    from snx._lib import CONSTANTS, fn
    from snx.ops import _p, _stream
    wsb = fn("snx_loss_workspace_bytes")
    for B, Bp, k, V in ((0, 4, 1, 8), (5, 4, 1, 8), (4, 4, 0, 8), (4, 4, 1, 0), (-1, 4, 1, 8)):
        assert wsb(B, Bp, k, V) == 0 == L.workspace_bytes(B, Bp, k, V)
    t = torch.zeros(1 << 16, device=dev)
    hp = (C.c_float * 7)(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    for bad in L.REFUSED:
        dims = (C.c_int32 * 6)(*bad, 0)
        rc = fn("snx_loss_fwd")(_p(t), _p(t), _p(t), _p(None), _p(None), _p(None), hp, dims, _p(t), _p(t), _stream())
        assert rc == CONSTANTS["SNX_E_SHAPE"], f"snx_loss_fwd accepted {bad}"
        rc = fn("snx_loss_bwd")(_p(t), _p(t), _p(t), _p(t), hp, dims, _p(t), 0, _p(t), _p(t), _p(t), _stream())
        assert rc == CONSTANTS["SNX_E_SHAPE"], f"snx_loss_bwd accepted {bad}"
    dims = (C.c_int32 * 6)(4, 4, 1, 8, 0, 0)
    assert fn("snx_loss_fwd")(_p(None), _p(t), _p(t), _p(None), _p(None), _p(None), hp, dims, _p(t), _p(t), _stream()) == CONSTANTS["SNX_E_ARG"]
    torch.cuda.synchronize()
    assert bool((t == 0).all()), "a refused call wrote"


def test_splade_loss_gradients_share_one_storage(dev):
    from snx.loss import splade_loss
    c = L.build_case("b13_5_chunks", "random")
    q, p, n = (_t(x, dev).requires_grad_() for x in (c.q, c.p, c.n))
    loss, _ = splade_loss(q, p, n, [float(x) for x in c.hp], c.k, _t(c.tpos, dev), _t(c.tneg, dev), c.off, True, _t(c.tsc, dev))
    dq, dp, dn = torch.autograd.grad(loss, (q, p, n))
    base = dq.untyped_storage().data_ptr()
    assert dp.untyped_storage().data_ptr() == base == dn.untyped_storage().data_ptr()
    assert dq.data_ptr() == base and dp.data_ptr() == base + c.B * c.V * 4 and dn.data_ptr() == base + (c.B + c.Bp) * c.V * 4
    assert bool(torch.isfinite(dq).all() and torch.isfinite(dp).all() and torch.isfinite(dn).all())


@pytest.mark.parametrize("name", list(L.LDS_CASES))
def test_loss_dynamic_lds_above_64k(dev, name):
    """collected last: shapes whose loss_partial / loss_bwd or loss_reduce launch asks for more than 64 KiB of dynamic LDS"""
    d = L.LDS_CASES[name]
    assert max(L.lds_bytes(d["B"], d["Bp"], d["k"])) > 64 * 1024
    _run_and_check(name, "random", dev, again=False)
    _run_and_check(name, "exact_b", dev, again=False)

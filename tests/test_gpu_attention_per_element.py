"""The attention entry points behind snx.ops.attn_fwd / attn_bwd (called as those wrappers call them, but into NaN-filled
buffers) against the float64 reference of tests/attention_reference.py, PER ELEMENT (bounds and their derivation: that
module's docstring), in every launch form: forward resident and streaming; backward one-pass,
resident two-pass and streaming two-pass.  The backward takes `out` and `lse` as inputs, so its tests hand it the
REFERENCE's (rounded to bf16 / fp32) and judge it independently of the forward; a chain test runs kernel after kernel as
training does.  All shapes are small (T <= 1,601 tokens, no sequence above 513); tests/test_attention_reference_host.py
checks, without a GPU, that the bounds hold for correct rounding, that the cases contain what their comments say and
which planted faults each detects.  Needs a real MI355X:  pytest -m gpu."""
import functools

import pytest
import torch

from tests import attention_reference as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# Sequence families.  max_seqlen is DECLARED above the longest sequence where the family allows it.
FAMILIES = {
    # every length around the 16-row group and the 64-key tile; 33 units: neither 4 nor 8 divides them
    "seams64": dict(lens=[1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65], heads=3, max_seqlen=256),
    # both sides of the 128 / 192 / 256 seams: resident units of 2, 3 and 4 tiles
    "tiles": dict(lens=[127, 128, 129, 191, 192, 193, 255, 256], heads=2, max_seqlen=256),
    # streaming only: 5 to 9 tiles, one token past 256 and past 512
    "stream": dict(lens=[257, 320, 511, 513], heads=2, max_seqlen=1024),
}
# the window decides the mask recipe, so that every recipe meets a resident and a streaming family, with and without a band
# (window 0 with holes: the masked tokens are rows without a visible key).  `alternate` meets a band inside `mix` only: alone
# it hides either window + 1 or window - 1 (a key at an odd distance from a valid query is always masked).
WINDOW_RECIPE = {-1: "mix", 0: "holes", 1: "holes", 8: "mix", 63: "left", 64: "right", 65: "ones", 128: "mix"}
# seams64 has one pair of tokens 64 apart and three pairs 63 apart: they must stay valid for the seam windows to decide anything
SEAMS64_RECIPE = {63: "holes", 64: "ones"}

CASES = {}
for _fam, _kw in FAMILIES.items():
    # windows 0 and 1, and the three that meet the 64-key tile seam exactly; 128 = two tiles, on the long sequences
    for _w in (-1, 0, 1, 8, 63, 64, 65) + ((128,) if _fam == "stream" else ()):
        _r = SEAMS64_RECIPE.get(_w, WINDOW_RECIPE[_w]) if _fam == "seams64" else WINDOW_RECIPE[_w]
        CASES[f"{_fam}_w{_w}"] = dict(_kw, window=_w, recipe=_r, seed=100 + _w)
for _fam in ("tiles", "stream"):
    # global attention under each recipe: `left` masks the whole first key tile (the running maximum starts at NEG_BIG and
    # the first tile's weights are wiped by the first real one), `right` leaves one valid token / wholly masked trailing tiles
    for _i, _r in enumerate(("right", "left", "holes", "alternate")):
        CASES[f"{_fam}_{_r}"] = dict(FAMILIES[_fam], window=-1, recipe=_r, seed=200 + _i)
# sharp softmax rows whose maximum rises up to the last key tile (every tile rescales the accumulator), and the mirror image
CASES["peaked_up"] = dict(lens=[65, 130, 256], heads=2, max_seqlen=256, window=-1, recipe="ones", seed=301, peaked="up")
CASES["peaked_down"] = dict(CASES["peaked_up"], peaked="down")
# sequence groups: units of 1 and 2 tiles (30 units in workgroups of 4, 3 units in workgroups of 2: dead slots in both) ...
CASES["seams64_groups"] = dict(FAMILIES["seams64"], window=8, recipe="mix", seed=401, groups=[(0, 10, 64), (10, 1, 65)])
# ... units of 2, 3 and 4 tiles (a 3-tile unit leaves two waves of its workgroup without a unit) ...
CASES["tiles_groups"] = dict(FAMILIES["tiles"], window=64, recipe="holes", seed=402,
                             groups=[(0, 2, 128), (2, 3, 192), (5, 3, 256)])
# ... the packed resident units (1 to 4 tiles, dead slots) under the other windows, left padding and peaked rows ...
CASES["seams64_groups_w0"] = dict(CASES["seams64_groups"], window=0, recipe="holes", seed=405)
CASES["seams64_groups_w63"] = dict(CASES["seams64_groups"], window=63, recipe="holes", seed=406)
CASES["tiles_groups_left"] = dict(CASES["tiles_groups"], window=-1, recipe="left", seed=407)
CASES["tiles_groups_w65"] = dict(CASES["tiles_groups"], window=65, recipe="ones", seed=408)
CASES["peaked_groups"] = dict(CASES["peaked_up"], seed=409, groups=[(0, 1, 65), (1, 1, 130), (2, 1, 256)])
# ... and one table that mixes a <= 64, a <= 256 and a > 256 group (resident and streaming kernels in one call)
_MIXED = dict(lens=[1, 33, 64, 65, 200, 256, 257, 300], heads=3, max_seqlen=320, groups=[(0, 3, 64), (3, 3, 256), (6, 2, 320)])
CASES["mixed_groups_w64"] = dict(_MIXED, window=64, recipe="mix", seed=403)
CASES["mixed_groups_global"] = dict(_MIXED, window=-1, recipe="left", seed=404)

GROUPED = [n for n, kw in CASES.items() if "groups" in kw]
RESIDENT = [n for n, kw in CASES.items() if "groups" not in kw and max(kw["lens"]) <= 256]
STREAM_MAX_SEQLEN = 320                       # declared group max_len that routes <= 256-token sequences to the streaming kernels


def fwd_forms(name):
    return ["groups"] if name in GROUPED else (["resident"] if name in RESIDENT else []) + ["streaming"]


def bwd_forms(name):
    return ["onepass", "twopass"] if name in GROUPED else (["onepass", "resident2p"] if name in RESIDENT else []) + ["streaming"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, forward reference, out_in bf16, lse_in fp32, backward reference at those) -- computed once, never modified"""
    kw = dict(CASES[name])
    ms, groups = kw.pop("max_seqlen"), kw.pop("groups", None)
    case = R.make_case(**kw)
    case.max_seqlen, case.groups = ms, groups
    assert ms >= case.max_len
    fref = R.forward_reference(case)
    out_in, lse_in = R.backward_inputs(fref)
    return case, fref, out_in, lse_in, R.backward_reference(case, out_in, lse_in)


def _launch(case, form):
    """(max_seqlen, groups, onepass) of a launch form"""
    B = case.B
    if form in ("groups", "onepass", "twopass") and case.groups:
        return case.max_seqlen, case.groups, int(form != "twopass")
    if form == "streaming":
        ms = max(case.max_seqlen, STREAM_MAX_SEQLEN)
        return ms, [(0, B, ms)], 1
    assert case.max_seqlen <= 256
    return case.max_seqlen, [(0, B, case.max_seqlen)], int(form != "resident2p")


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _fwd(dev, case, form):
    """snx_attn_fwd_ex the way ops.attn_fwd calls it (same validation, same arguments), but into buffers pre-filled with
    NaN: ops.attn_fwd allocates with torch.empty, and the caching allocator would hand the next launch form the previous
    form's (correct) result -- a row that a kernel leaves unwritten must not pass on it."""
    from snx import ops
    from snx._lib import check, fn
    ms, groups, _ = _launch(case, form)
    qkv, cu, mask = case.qkv.to(dev), case.cu.to(dev), case.mask.to(dev)
    ops._check_seqs(cu, case.T, ms, groups)
    out = _nan((case.T, case.heads * 64), BF16, dev)
    lse = _nan((case.heads, case.T), torch.float32, dev)
    check(fn("snx_attn_fwd_ex")(ops._p(qkv), ops._p(cu), ops._p(mask), ops._p(out), ops._p(lse), ops._groups(groups), case.T,
                                case.B, ms, case.heads, 64, case.window, ops._stream()), "snx_attn_fwd_ex")
    torch.cuda.synchronize()
    return out, lse


def _bwd(dev, case, out_in, lse_in, form, rope_table=None, pos=None):
    """snx_attn_bwd_ex the way ops.attn_bwd calls it, dqkv (and the delta scratch) pre-filled with NaN"""
    import snx
    from snx import ops
    from snx._lib import check, fn
    ms, groups, onepass = _launch(case, form)
    qkv, cu, mask = case.qkv.to(dev), case.cu.to(dev), case.mask.to(dev)
    out_in, lse_in, dout = out_in.to(dev).contiguous(), lse_in.to(dev).contiguous(), case.dout.to(dev)
    tab = None if rope_table is None else rope_table.to(dev)
    pos = None if pos is None else pos.to(dev)
    ops._check_seqs(cu, case.T, ms, groups)
    dqkv = _nan(tuple(qkv.shape), BF16, dev)
    delta = _nan((case.heads, case.T), torch.float32, dev)
    before = snx.config("attn_bwd_onepass")
    try:
        snx.configure(attn_bwd_onepass=onepass)
        check(fn("snx_attn_bwd_ex")(ops._p(qkv), ops._p(out_in), ops._p(dout), ops._p(lse_in), ops._p(cu), ops._p(mask),
                                    ops._p(delta), ops._p(dqkv), ops._p(tab), ops._p(pos), ops._groups(groups), case.T,
                                    case.B, ms, case.heads, 64, case.window, ops._stream()), "snx_attn_bwd_ex")
        torch.cuda.synchronize()
    finally:
        snx.configure(attn_bwd_onepass=before)
    assert snx.config("attn_bwd_onepass") == before
    return dqkv


FWD_PARAMS = [(n, f) for n in CASES for f in fwd_forms(n)]
BWD_PARAMS = [(n, f) for n in CASES for f in bwd_forms(n)]


@pytest.mark.parametrize("name,form", FWD_PARAMS)
def test_forward_per_element(dev, name, form):
    case, fref, *_ = _case(name)
    out, lse = _fwd(dev, case, form)
    R.check_forward(out, lse, fref, what=f"{name}, forward {form}")


@pytest.mark.parametrize("name,form", BWD_PARAMS)
def test_backward_per_element(dev, name, form):
    """out_in and lse_in are the reference's: a forward error cannot hide a backward one, or be mistaken for one"""
    case, _, out_in, lse_in, bref = _case(name)
    R.check_backward(_bwd(dev, case, out_in, lse_in, form), bref, what=f"{name}, backward {form}")


@pytest.mark.parametrize("name", ["seams64_w8", "tiles_w64", "tiles_left", "stream_w65", "stream_left", "peaked_up",
                                  "mixed_groups_w64"])
def test_chain_as_training_runs_it(dev, name):
    """kernel forward, then kernel backward on the kernel's own out and lse (default forms), against the reference
    evaluated at those very inputs"""
    case, fref, *_ = _case(name)
    form = "groups" if name in GROUPED else fwd_forms(name)[0]
    out, lse = _fwd(dev, case, form)
    R.check_forward(out, lse, fref, what=f"{name}, chain forward")
    bref = R.backward_reference(case, out.cpu(), lse.cpu())
    R.check_backward(_bwd(dev, case, out, lse, "onepass" if name in GROUPED else bwd_forms(name)[0]), bref,
                     what=f"{name}, chain backward")


@pytest.mark.parametrize("name", ["seams64_w-1", "seams64_w63", "seams64_w0", "tiles_w64", "tiles_w65", "tiles_w1",
                                  "tiles_left", "tiles_alternate", "peaked_up"])
def test_launch_forms_on_the_same_data(dev, name):
    """What test_attention_resident_and_streaming_kernels_agree_bitwise states stays true on these cases: the resident
    and the streaming forward, and the resident and the streaming two-pass backward, give identical bits.  The one-pass
    backward sums in another order: it is held to the reference (test_backward_per_element), not to another kernel."""
    case, fref, out_in, lse_in, bref = _case(name)
    o1, l1 = _fwd(dev, case, "resident")
    o2, l2 = _fwd(dev, case, "streaming")
    ratios = R.check_forward(o1, l1, fref, what=f"{name}, resident forward")
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32)), \
        f"{name}: resident and streaming forward differ (resident against the reference: {ratios})"
    d1 = _bwd(dev, case, out_in, lse_in, "resident2p")
    d2 = _bwd(dev, case, out_in, lse_in, "streaming")
    ratios = R.check_backward(d1, bref, what=f"{name}, resident two-pass backward")
    assert torch.equal(d1.view(torch.int16), d2.view(torch.int16)), \
        f"{name}: resident and streaming two-pass backward differ in {int((d1 != d2).sum())} elements ({ratios})"


@pytest.mark.parametrize("form", ["onepass", "resident2p", "streaming"])
def test_fused_inverse_rope(dev, form):
    """the epilogue's transposed rotation on a multi-length case with a band and right padding, positions restarting
    in every sequence, against the rotated reference (dV is not rotated)"""
    from snx import ops
    case, _, out_in, lse_in, _ = _case("tiles_w64")
    tab = ops.rope_table(256, 64, 160000.0, "cpu")
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in case.lens])
    bref = R.backward_reference(case, out_in, lse_in, rope_table=tab, pos=pos)
    R.check_backward(_bwd(dev, case, out_in, lse_in, form, rope_table=tab, pos=pos), bref, what=f"fused inverse rope, {form}")

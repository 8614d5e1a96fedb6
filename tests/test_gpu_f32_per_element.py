"""Every kernel of the fp32 path (csrc/f32_path.hip) against tests/f32_reference.py, per element, through the C entry
points the two model functions are made of (snx_gemm_f32, snx_f32_ln_fwd / _ln_bwd, snx_f32_rope, snx_f32_geglu_fwd /
_bwd, snx_f32_attn_fwd / _bwd, snx_f32_tail_fwd / _bwd, snx_f32_seq_ids).  Every output sits inside a flat buffer of a
NaN sentinel: guards before and behind, the gap columns of a strided output (ldc - N) included, all checked untouched
afterwards; every fp32 operand sits between NaN guards, so an out-of-range read that is multiplied by zero still poisons
a result; accumulated outputs (dW, dw, gradE, gradb, dh) start from non-zero contents; the switches "f32_gemm64" and
"f32_attn_rows" are restored on the way out of the block that set them; every integer operand (mask, cu_seqlens, pos,
ids, seqid, the keys handed to the tail backward) sits between poison elements that make an out-of-range read visible.

GEMM: ONE value per element (the k-ascending fma chain), bit for bit, in all three kernel forms and operand layouts;
the decoder tail: its routed maxima against logits that are one value each (the EPI-2 path stores no logit); RoPE: the bits of numpy float32; everything else: the acceptance sets of the reference.  Which case is
there for which class: the tables of tests/f32_reference.py; tests/test_f32_reference_host.py proves on the CPU that the
sets admit fp32 arithmetic in several summation orders and that every planted fault is rejected by a case of these
tables.

Measured on an MI355X when this file was added (kernels of commit 86d3b44): 167 tests, 9.6 s, the slowest 0.8 s; every
GEMM and RoPE element bit for bit, every routed maximum of the tail the first of its maximum, nothing outside its set, no guard touched, no element decided by a libm
assumption; no kernel needed a change.  The figures per output stand in the docstring of tests/f32_reference.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import f32_reference as F

pytestmark = pytest.mark.gpu
PAD = 1024                       # guard elements before and behind every buffer
SWITCHES = ("f32_gemm64", "f32_attn_rows")
TALLY = F.Tally()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


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


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ip(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class In:
    """an fp32 operand between NaN guards: logical [rows, cols] at `offset` floats with strides (s_row, s_col); the gaps
    a stride leaves hold NaN too"""

    def __init__(self, dev, a, strides=None, offset=0):
        a = np.asarray(a, dtype=np.float32)
        a2 = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(1, -1)
        strides = strides or (a2.shape[1], 1)
        n = offset + (a2.shape[0] - 1) * strides[0] + (a2.shape[1] - 1) * strides[1] + 1
        self.buf = torch.full((PAD + n + PAD,), float("nan"), dtype=torch.float32, device=dev)
        self.buf.as_strided(a2.shape, strides, PAD + offset).copy_(torch.from_numpy(a2))
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * (PAD + offset))


class Out:
    """an fp32 output [rows, cols] with leading dimension ld inside a sentinel-filled buffer; init: the contents it is
    accumulated into (else every element must have been written)"""

    def __init__(self, dev, rows, cols, ld=None, init=None):
        self.rows, self.cols, self.ld, self.init = rows, cols, ld or cols, init is not None
        n = (rows - 1) * self.ld + cols
        self.buf = torch.full((PAD + n + PAD,), F.SENT_F32, dtype=torch.int32, device=dev).view(torch.float32)
        self.view = self.buf.as_strided((rows, cols), (self.ld, 1), PAD)
        if init is not None:
            self.view.copy_(torch.from_numpy(np.asarray(init, dtype=np.float32).reshape(rows, cols)))
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * PAD)

    def get(self, what):
        raw = self.buf.view(torch.int32).cpu().numpy()
        inside = np.zeros(raw.shape, dtype=bool)
        idx = (PAD + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]).reshape(-1)
        inside[idx] = True
        touched = np.argwhere(~inside & (raw != F.SENT_F32))
        assert len(touched) == 0, f"{what}: {len(touched)} guard or gap elements written, first at flat offset {int(touched[0][0]) - PAD}"
        got = raw[idx].reshape(self.rows, self.cols)
        if not self.init:
            never = np.argwhere(got == F.SENT_F32)
            assert len(never) == 0, f"{what}: {len(never)} elements never written, first {never[0].tolist()}"
        return got.view(np.float32)


IPAD = 64                        # poison elements before and behind every integer operand
ONE_KEY = 0x3F800000FFFFFFFF     # a key of value 1.0 at position / column 0: an out-of-range read of it adds a contribution
POISON = {"mask": 1, "cu": -1, "pos": -1, "ids": -1, "seqid": -1, "keys": ONE_KEY}


def _i(dev, a, dtype, kind):
    """an integer operand between poison elements that an out-of-range read turns into a visible error: a mask that
    counts as valid, a negative position / id / offset (it leads into the NaN guard of the fp32 operand it indexes), a
    routed key that contributes"""
    a = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    buf = torch.full((IPAD + a.numel() + IPAD,), POISON[kind], dtype=dtype)
    buf[IPAD:IPAD + a.numel()] = a.reshape(-1)
    return buf.to(dev)[IPAD:IPAD + a.numel()]


def _call(name, *args):
    from snx._lib import call
    call(name, *args, _st())


# ----------------------------------------------------------------------------- GEMM
def _run_gemm(c, dev):
    A, B = In(dev, c.A, c.a_st, c.a_off), In(dev, c.B, c.b_st, c.b_off)
    Cb = Out(dev, c.M, c.N, c.ldc, init=c.R0 if c.epi else None)
    Rb = In(dev, c.R0, (c.ldr, 1)) if c.has_r else None
    _call("snx_gemm_f32", A.ptr, c.a_st[0], c.a_st[1], B.ptr, c.b_st[0], c.b_st[1], Cb.ptr, c.ldc, Rb.ptr if Rb else None,
          c.ldr if Rb else 0, c.M, c.N, c.K, c.epi)
    torch.cuda.synchronize()
    return Cb.get(f"gemm {c.name} {c.layout}")


@pytest.mark.parametrize("layout", F.LAYOUTS)
@pytest.mark.parametrize("name", [c[0] for c in F.GEMM_CASES])
def test_gemm_is_the_k_ascending_fma_chain(dev, name, layout):
    c = F.gemm_case(name, layout)
    if name == "novec":
        assert (c.a_vec, c.b_vec) == (0, 0) and c.a_off % 4 and c.a_st[0] % 4
    if name == "mixedvec":
        assert (c.a_vec, c.b_vec) == (1, 0)
    got = _run_gemm(c, dev)
    rows, cols = F.gemm_subset(c)
    F.check_bits(f"gemm {name} {layout} ({c.form})", got[rows, cols], F.gemm_expected(c, rows, cols), TALLY, f"gemm {c.form}")
    if c.form != "64":
        with Switches(f32_gemm64=1):
            got64 = _run_gemm(c, dev)
        F.check_bits(f"gemm {name} {layout}: {c.form} form against the 64-tile form", got, got64, TALLY, f"gemm {c.form} = 64-tile")
        if c.form == "128":                                       # the 64-tile form itself, on the same subset
            F.check_bits(f"gemm {name} {layout} (64-tile)", got64[rows, cols], F.gemm_expected(c, rows, cols))
    print(TALLY)


# ----------------------------------------------------------------------------- decoder tail
def _keys(out, n):
    return np.ascontiguousarray(out).view(np.uint64).reshape(-1, n)


def _run_tail_fwd(c, dev):
    Hd, E, bias = In(dev, c.Hd), In(dev, c.E), In(dev, c.bias)
    mask, cu, pos = _i(dev, c.mask, torch.int64, "mask"), _i(dev, c.cu, torch.int32, "cu"), _i(dev, c.pos, torch.int32, "pos")
    seqid = torch.full((c.T + 2,), -7, dtype=torch.int32, device=dev)
    _call("snx_f32_seq_ids", _ip(cu), _ip(seqid[1:]), c.T, c.B)
    keys, tw = Out(dev, c.B, 2 * c.V), Out(dev, 1, 2 * c.T)
    sparse, tws = Out(dev, c.B, c.V), Out(dev, 1, c.T)
    _call("snx_f32_tail_fwd", Hd.ptr, E.ptr, bias.ptr, _ip(mask), _ip(seqid[1:]), _ip(pos), keys.ptr, tw.ptr, sparse.ptr,
          tws.ptr, c.T, c.B, c.V, c.H)
    torch.cuda.synchronize()
    sq = seqid.cpu().numpy()
    assert sq[0] == -7 and sq[-1] == -7 and np.array_equal(sq[1:-1], c.seqid), "snx_f32_seq_ids"
    what = f"tail {c.name} {c.family} {c.maskkind}"
    return (_keys(keys.get(what + " keys"), c.V), _keys(tw.get(what + " twkeys"), c.T)[0], sparse.get(what + " sparse"),
            tws.get(what + " token_weights")[0])


@pytest.mark.parametrize("maskkind", F.TAIL_MASKS)
@pytest.mark.parametrize("family", F.TAIL_FAMILIES)
@pytest.mark.parametrize("name", [c[0] for c in F.TAIL_CASES])
def test_tail_forward_routes_and_values(dev, name, family, maskkind):
    c = F.tail_case(name, family, maskkind)
    keys, tw, sparse, tws = _run_tail_fwd(c, dev)
    if c.form == "128" and family == "random":
        # the chain on the CPU for the edge tiles and a stride sample; everything else as bits against the 64-tile form
        cols = np.unique(np.concatenate([np.arange(0, c.V, 13), np.arange((c.V - 1) // 128 * 128, c.V)]))
        rows = np.unique(np.concatenate([np.arange(0, c.T, 41), np.arange((c.T - 1) // 128 * 128, c.T)]))
        assert c.T * len(cols) + len(rows) * c.V >= 200_000
        F.tail_fwd_check(c, keys, tw, sparse, tws, cols=cols, rows=rows, tally=TALLY)
    else:
        F.tail_fwd_check(c, keys, tw, sparse, tws, tally=TALLY)
    if c.form != "64":
        with Switches(f32_gemm64=1):
            k64, t64, s64, w64 = _run_tail_fwd(c, dev)
        assert np.array_equal(keys, k64) and np.array_equal(tw, t64), f"tail {name}: the {c.form} form and the 64-tile form differ"
    live = c.mask != 0
    assert np.all(tws[~live].view(np.uint32) == 0)
    if c.V >= 2:                                                  # a column whose logits are all <= 0
        assert np.all(sparse[:, c.V - 1].view(np.uint32) == 0)
    print(TALLY)


@pytest.mark.parametrize("with_tw", [True, False])
@pytest.mark.parametrize("keys_from", ["device", "reference"])
@pytest.mark.parametrize("family", F.TAIL_FAMILIES)
@pytest.mark.parametrize("name", ["v65", "v200", "deepk"])
def test_tail_backward_per_element(dev, name, family, keys_from, with_tw):
    for maskkind in F.TAIL_MASKS:
        c = F.tail_case(name, family, maskkind)
        if keys_from == "device":
            keys, tw, _, _ = _run_tail_fwd(c, dev)
        else:
            keys, tw = F.tail_ref_keys(c)
        g, g_tw, gE0, gb0 = F.tail_grads(c)
        if not with_tw:
            g_tw = None
        kd = _i(dev, keys.view(np.int64), torch.int64, "keys")
        td = _i(dev, tw.view(np.int64), torch.int64, "keys")
        Hd, E, gs = In(dev, c.Hd), In(dev, c.E), In(dev, g)
        gt = In(dev, g_tw) if with_tw else None
        cu = _i(dev, c.cu, torch.int32, "cu")
        dHd, gE, gb = Out(dev, c.T, c.H), Out(dev, c.V, c.H, init=gE0), Out(dev, 1, c.V, init=gb0)
        _call("snx_f32_tail_bwd", gs.ptr, gt.ptr if gt else None, _ip(kd), _ip(td), Hd.ptr, E.ptr, _ip(cu), dHd.ptr, gE.ptr,
              gb.ptr, c.T, c.B, c.V, c.H)
        torch.cuda.synchronize()
        what = f"tail bwd {name} {family} {maskkind} keys of the {keys_from} tw {with_tw}"
        got = {"dHd": dHd.get(what), "gE": gE.get(what), "gb": gb.get(what)[0]}
        F.check_sets(what, got, F.tail_bwd_expected(c, keys, tw, g, g_tw, gE0, gb0, F.ulps()), TALLY,
                     F.tail_bwd_expected(c, keys, tw, g, g_tw, gE0, gb0, F.ulps(all=0)), "tail bwd ")
    print(TALLY)


# ----------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("H", F.LN_H)
@pytest.mark.parametrize("src", F.LN_FWD_MODES)
def test_layernorm_forward_per_element(dev, src, H):
    for T in F.LN_T:
        for eps in F.LN_EPS:
            c = F.ln_case(T, H, eps)
            x = In(dev, c.E if src == 1 else c.a if src == 2 else c.x)
            ids = _i(dev, c.ids, torch.int64, "ids")
            w, out = In(dev, c.w), Out(dev, T, H)
            _call("snx_f32_ln_fwd", x.ptr, _ip(ids) if src == 1 else None, w.ptr, out.ptr, T, H, C.c_float(eps), src)
            torch.cuda.synchronize()
            what = f"ln fwd src {src} T {T} H {H} eps {eps}"
            lo0, hi0 = F.ln_fwd_expected(c, src, F.ulps(all=0))
            F.check_interval(what, out.get(what), *F.ln_fwd_expected(c, src, F.ulps()), TALLY, f"ln fwd src {src}", lo0, hi0)
    print(TALLY)


@pytest.mark.parametrize("H", F.LN_H)
@pytest.mark.parametrize("mode", F.LN_BWD_MODES)
def test_layernorm_backward_per_element(dev, mode, H):
    src = {"acc": 0, "ow": 0, "embed": 1, "gelu": 2}[mode]
    for T in F.LN_T:
        for eps in F.LN_EPS:
            c = F.ln_case(T, H, eps)
            x = In(dev, c.E if src == 1 else c.a if src == 2 else c.x)
            ids = _i(dev, c.ids, torch.int64, "ids")
            dy, w = In(dev, c.dy), In(dev, c.w)
            dst = Out(dev, c.V, H, init=c.gE0) if mode == "embed" else Out(dev, T, H, init=c.dh0 if mode == "acc" else None)
            dw = Out(dev, 1, H, init=c.dw0)
            _call("snx_f32_ln_bwd", dy.ptr, x.ptr, _ip(ids) if src == 1 else None, w.ptr, dst.ptr, dw.ptr, T, H, C.c_float(eps),
                  src, int(mode == "acc"), c.pad if mode == "embed" else -1)
            torch.cuda.synchronize()
            what = f"ln bwd {mode} T {T} H {H} eps {eps}"
            got = {"dst": dst.get(what), "dw": dw.get(what)}
            F.check_sets(what, got, F.ln_bwd_expected(c, mode, F.ulps()), TALLY, F.ln_bwd_expected(c, mode, F.ulps(all=0)), f"ln bwd {mode} ")
            if mode == "embed":
                idle = np.ones(c.V, dtype=bool)
                idle[c.ids[c.ids != c.pad]] = False
                assert idle[c.pad]
                F.check_bits(what + ": the pad row and the rows of ids that do not occur", got["dst"][idle], c.gE0[idle])
    print(TALLY)


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("hd", F.ROPE_HD)
def test_rope_bit_for_bit(dev, hd, inverse):
    for heads in F.ROPE_HEADS:
        for T in F.ROPE_T:
            c = F.rope_case(T, heads, hd)
            qkv = Out(dev, T, 3 * heads * hd, init=c.qkv)
            tab, pos = In(dev, c.tab.reshape(1, -1)), _i(dev, c.pos, torch.int32, "pos")
            _call("snx_f32_rope", qkv.ptr, tab.ptr, _ip(pos), T, heads, hd, inverse)
            torch.cuda.synchronize()
            what = f"rope hd {hd} heads {heads} T {T} inverse {inverse}"
            got = qkv.get(what).reshape(T, 3, heads, hd)
            F.check_bits(what, got, F.rope_expected(c, inverse), TALLY, "rope")
            F.check_bits(what + ": the v third", got[:, 2], c.qkv[:, 2])
    print(TALLY)


@pytest.mark.parametrize("I", F.GEGLU_I)
def test_geglu_forward_and_backward_per_element(dev, I):
    for T in F.GEGLU_T:
        c = F.geglu_case(T, I)
        u, dy = In(dev, c.u), In(dev, c.dy)
        y, du = Out(dev, T, I), Out(dev, T, 2 * I)
        _call("snx_f32_geglu_fwd", u.ptr, y.ptr, T, I)
        _call("snx_f32_geglu_bwd", u.ptr, dy.ptr, du.ptr, T, I)
        torch.cuda.synchronize()
        what = f"geglu T {T} I {I}"
        F.check_sets(what, {"y": y.get(what), "du": du.get(what)}, F.geglu_expected(c, F.ulps()), TALLY,
                     F.geglu_expected(c, F.ulps(all=0)), "geglu ")
    print(TALLY)


# ----------------------------------------------------------------------------- attention
def _attn_inputs(c, dev):
    return (In(dev, c.qkv.reshape(c.T, -1)), _i(dev, c.cu, torch.int32, "cu"), _i(dev, c.seqid, torch.int32, "seqid"), _i(dev, c.mask, torch.int64, "mask"))


def _run_attn_fwd(c, dev, with_mask=True, with_lse=True):
    qkv, cu, seqid, mask = _attn_inputs(c, dev)
    out = Out(dev, c.T, c.heads * c.hd)
    lse = Out(dev, c.heads, c.T) if with_lse else None
    _call("snx_f32_attn_fwd", qkv.ptr, _ip(cu), _ip(seqid), _ip(mask) if with_mask else None, out.ptr, lse.ptr if lse else None,
          c.T, c.B, c.heads, c.hd, c.window)
    torch.cuda.synchronize()
    what = f"attn fwd hd {c.hd} lens {c.lens[:4]} window {c.window} {c.recipe}"
    return out.get(what).reshape(c.T, c.heads, c.hd), lse.get(what) if lse else None


def _run_attn_bwd(c, dev, out_in, lse_in):
    qkv, cu, seqid, mask = _attn_inputs(c, dev)
    o, do, ls = In(dev, np.asarray(out_in).reshape(c.T, -1)), In(dev, c.dout.reshape(c.T, -1)), In(dev, lse_in)
    dqkv = Out(dev, c.T, 3 * c.heads * c.hd)
    _call("snx_f32_attn_bwd", qkv.ptr, o.ptr, do.ptr, ls.ptr, _ip(cu), _ip(seqid), _ip(mask), dqkv.ptr, c.T, c.B, c.heads, c.hd,
          c.window)
    torch.cuda.synchronize()
    return dqkv.get(f"attn bwd hd {c.hd} lens {c.lens[:4]} window {c.window} {c.recipe}")


@pytest.mark.parametrize("form,hd", [("tiled", h) for h in F.ATTN_HD_TILED] + [("rows", h) for h in F.ATTN_HD_ROWS])
def test_attention_forward_per_element(dev, form, hd):
    full = hd == (16 if form == "tiled" else 6)
    with Switches(f32_attn_rows=int(form == "rows")):
        for li, window, recipe in F.attn_table(hd, salt=0 if full else 1):
            c = F.attn_case(li, 2 if hd < 64 else 1, hd, window, recipe)
            out, lse = _run_attn_fwd(c, dev)
            what = f"attn fwd {form} hd {hd} lens {li} window {window} {recipe}"
            F.attn_fwd_check(what, c, out, lse, TALLY, f"attn fwd {form} ")
            novis = ~np.concatenate([F.AR.visibility(n, torch.from_numpy(c.mask[c.cu[b]:c.cu[b + 1]]), c.window).any(dim=1).numpy()
                                     for b, n in enumerate(c.lens)])
            assert np.all(out[novis] == 0) and np.all(lse[:, novis] == 0), what + ": a row without a visible key is not 0"
            if form == "tiled" and recipe == "ones":             # mask == NULL: every key valid; lse == NULL: not stored
                out2, none = _run_attn_fwd(c, dev, with_mask=False, with_lse=False)
                assert none is None
                F.check_bits(what + " without mask and lse", out2, out)
            elif form == "tiled" and li == 1:
                out2, _ = _run_attn_fwd(c, dev, with_lse=False)
                F.check_bits(what + " without lse", out2, out)
    print(TALLY)


@pytest.mark.parametrize("source", ["reference", "chain"])
@pytest.mark.parametrize("hd", F.ATTN_HD_BWD)
def test_attention_backward_per_element(dev, hd, source):
    for li, window, recipe in F.attn_table(hd, salt=0 if hd == 16 else 1):
        c = F.attn_case(li, 2 if hd < 64 else 1, hd, window, recipe)
        if source == "chain":
            out_in, lse_in = _run_attn_fwd(c, dev)
        else:
            r = F.attn_fwd_expected(c, F.ulps())
            out_in, lse_in = r.out.astype(np.float32), r.lse.astype(np.float32)
        dqkv = _run_attn_bwd(c, dev, out_in, lse_in)
        F.attn_bwd_check(f"attn bwd ({source}) hd {hd} lens {li} window {window} {recipe}", c, dqkv, out_in, lse_in, TALLY)
    print(TALLY)


# ----------------------------------------------------------------------------- model plumbing
def test_model_workspaces_are_exactly_what_is_advertised(dev):
    """a two-layer model through snx_model_forward_f32 / snx_model_backward_f32_tw into workspaces of exactly the
    advertised sizes with guards behind them; the rotating-buffer forward gives the bits of the saving forward"""
    from oracle import splade_oracle as O
    from snx._lib import call, fn
    from tests.test_gpu_model import _build_model
    cfg = O.EncoderConfig(vocab_size=300, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4,
                          local_attention=16, pad_token_id=299)
    params = O.perturb_params(O.init_params(cfg, seed=5), seed=6, scale=2.0, bias_mean=-0.1)
    rt = _build_model(cfg, params, dev).runtime
    lens = (5, 17, 1, 30)
    T, B, V = sum(lens), len(lens), cfg.vocab_size
    g = torch.Generator().manual_seed(2)
    ids = _i(dev, torch.randint(0, V - 1, (T,), generator=g).numpy(), torch.int64, "ids")
    mask = torch.ones(T, dtype=torch.int64)
    mask[7] = 0
    mask = _i(dev, mask.numpy(), torch.int64, "mask")
    cu = _i(dev, np.concatenate([[0], np.cumsum(lens)]), torch.int32, "cu")
    pos = _i(dev, np.concatenate([np.arange(n) for n in lens]), torch.int32, "pos")
    rg, rl = rt._rope_tables(64, dev, cfg.hidden_size // cfg.num_attention_heads)
    runs = {}
    for save in (1, 0):
        nbytes = int(fn("snx_model_workspace_bytes_f32")(C.byref(rt._desc), T, B, save))
        assert nbytes > 0 and nbytes % 4 == 0
        ws, sparse, tw = Out(dev, 1, nbytes // 4), Out(dev, B, V), Out(dev, 1, T)
        call("snx_model_forward_f32", C.byref(rt._desc), rt._param_ptrs(), _ip(ids), _ip(mask), _ip(cu), _ip(pos), _ip(rg), _ip(rl),
             ws.ptr, sparse.ptr, tw.ptr, T, B, save, _st())
        torch.cuda.synchronize()
        ws.init = True                                           # a scratch arena: held to its guards alone
        ws.get(f"forward workspace save {save}")
        runs[save] = (sparse.get("sparse"), tw.get("token_weights"), ws)
    F.check_bits("sparse: rotating buffers against saved activations", runs[0][0], runs[1][0])
    F.check_bits("token_weights: rotating buffers against saved activations", runs[0][1], runs[1][1])
    nb = int(fn("snx_model_bwd_workspace_bytes_f32")(C.byref(rt._desc), T))
    scratch = Out(dev, 1, nb // 4)
    scratch.init = True
    grads = [torch.zeros_like(p) for p in rt.params]
    gs = torch.randn(B, V, generator=g).to(dev)
    gt = torch.randn(T, generator=g).to(dev)
    call("snx_model_backward_f32_tw", C.byref(rt._desc), rt._param_ptrs(), rt._grad_ptrs(grads), _ip(ids), _ip(mask), _ip(cu),
         _ip(pos), _ip(rg), _ip(rl), runs[1][2].ptr, _ip(gs), _ip(gt), scratch.ptr, T, B, _st())
    torch.cuda.synchronize()
    scratch.get("backward scratch")
    runs[1][2].get("forward workspace after the backward")
    assert all(bool(torch.isfinite(x).all()) for x in grads) and any(float(x.abs().max()) > 0 for x in grads)

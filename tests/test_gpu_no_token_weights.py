"""SNX_FWD_NO_TOKEN_WEIGHTS / need_token_weights=False: a forward whose caller drops token_weights runs the fused decoder
without the row half of its epilogue and without the token_weights pass.  Nothing else may move: sparse, the saved keys,
every gradient and every trained parameter keep their BITS, and what the flag says is not written is not written.

Shapes are the smallest that reach every path: the 256x192 persistent form at the threshold snx_dec256_takes (one call,
mixed 64- and 256-token sequences), the 128x128 form below it (one call per sequence group, both tile heights, the
finalize = 0 then 1 sequence), V = 1010 (the last 192-column tile has one 96-column half partly and one wholly outside the
matrix; the last 128-column tile is partial), one sequence with masked tail tokens."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SNX_FWD_NO_TOKEN_WEIGHTS = 2
TW_SENTINEL = -12345.5                                       # token_weights are >= 0
KEY_SENTINEL = 0x5A5A5A5A
GUARD = 4096                                                 # bytes behind the scratch buffer that nobody may write


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------- kernel level
def _head_case(dev, n64, n256, H=768, V=1010, seed=5):
    """n64 sequences of 64 tokens then n256 of 256 (two sequence groups); the second 256-token sequence loses its last 37
    tokens to the mask, the first 64-token one its last 5."""
    g = torch.Generator().manual_seed(seed)
    lens = [64] * n64 + [256] * n256
    T = sum(lens)
    hd = (torch.randn(T, H, generator=g) * 0.5).to(BF16).to(dev)
    w = (torch.randn(V, H, generator=g) * 0.05).to(BF16).to(dev)
    bias = (torch.randn(V, generator=g) * 0.1 - 0.1).to(dev)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    mask = torch.ones(T, dtype=torch.int64)
    mask[int(cu[1]) - 5:int(cu[1])] = 0
    k = n64 + 1
    mask[int(cu[k + 1]) - 37:int(cu[k + 1])] = 0
    groups = [(0, n64, 64), (n64, n256, 256)]
    return dict(hd=hd, w=w, bias=bias, cu=cu.to(dev), mask=mask.to(dev), T=T, V=V, H=H, nseq=len(lens), groups=groups)


def _run_head(c, flags, calls, record=True):
    """calls: [(first sequence, sequences, longest)], the last one finalises.  Every output starts as a sentinel."""
    from snx._lib import check, fn
    from snx.ops import _p, _stream
    dev = c["hd"].device
    T, V, H = c["T"], c["V"], c["H"]
    sparse = torch.full((c["nseq"], V), float("nan"), dtype=torch.float32, device=dev)
    keys = torch.full((c["nseq"], V), KEY_SENTINEL, dtype=torch.int32, device=dev)
    tw = torch.full((T,), TW_SENTINEL, dtype=torch.float32, device=dev)
    tkeys = torch.full((T,), KEY_SENTINEL, dtype=torch.int32, device=dev) if record else None
    need = fn("snx_splade_head_scratch_bytes_notw")(T) if flags & SNX_FWD_NO_TOKEN_WEIGHTS else \
        fn("snx_splade_head_scratch_bytes")(T, V)
    scratch = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    for i, (sb, ns, ml) in enumerate(calls):
        check(fn("snx_decoder_splade_fwd_flags")(
            _p(c["hd"]), _p(c["w"]), _p(c["bias"]), C.c_void_p(c["cu"].data_ptr() + 4 * sb), _p(c["mask"]),
            C.c_void_p(sparse.data_ptr() + 4 * sb * V), C.c_void_p(keys.data_ptr() + 4 * sb * V), _p(tw), _p(tkeys),
            _p(scratch), T, ns, ml, V, H, int(i + 1 == len(calls)), flags, _stream()), "snx_decoder_splade_fwd_flags")
    torch.cuda.synchronize()
    assert bool((scratch[need:] == 0xA5).all()), "wrote behind the scratch buffer"
    return sparse, keys, tw, tkeys


def _check_head(c, calls):
    s0, k0, tw0, tk0 = _run_head(c, 0, calls)
    s1, k1, tw1, tk1 = _run_head(c, SNX_FWD_NO_TOKEN_WEIGHTS, calls)
    # flag off is today's training forward: everything written
    assert not bool(torch.isnan(s0).any()) and bool((tw0 >= 0).all()) and not bool((tk0 == KEY_SENTINEL).any())
    assert bool((s0 > 0).any()) and bool((tw0 > 0).any())
    assert torch.equal(_bits(s1), _bits(s0))
    assert torch.equal(k1, k0)
    assert bool((tw1 == TW_SENTINEL).all()), "token_weights written under SNX_FWD_NO_TOKEN_WEIGHTS"
    assert bool((tk1 == KEY_SENTINEL).all()), "token keys written under SNX_FWD_NO_TOKEN_WEIGHTS"
    # ... and with NULL in their place (what the model forward hands over)
    from snx._lib import check, fn
    from snx.ops import _p, _stream
    dev = c["hd"].device
    s2 = torch.empty_like(s0)
    k2 = torch.empty_like(k0)
    scratch = torch.empty((fn("snx_splade_head_scratch_bytes_notw")(c["T"]),), dtype=torch.uint8, device=dev)
    for sb, ns, ml in calls:
        check(fn("snx_decoder_splade_fwd_flags")(
            _p(c["hd"]), _p(c["w"]), _p(c["bias"]), C.c_void_p(c["cu"].data_ptr() + 4 * sb), _p(c["mask"]),
            C.c_void_p(s2.data_ptr() + 4 * sb * c["V"]), C.c_void_p(k2.data_ptr() + 4 * sb * c["V"]), None, None,
            _p(scratch), c["T"], ns, ml, c["V"], c["H"], 0, SNX_FWD_NO_TOKEN_WEIGHTS, _stream()),
            "snx_decoder_splade_fwd_flags")
    assert torch.equal(_bits(s2), _bits(s0)) and torch.equal(k2, k0)


def test_head_256x192_form_keeps_sparse_and_keys(dev):
    """The smallest T the persistent form takes: 16 x 64 + (T - 1024) / 256 x 256 tokens in ONE call."""
    import snx
    min_t = snx.config("dec256_min_t")
    assert snx.config("dec256") == 1 and min_t % 256 == 0 and min_t >= 1536
    c = _head_case(dev, 16, (min_t - 1024) // 256)
    assert c["T"] == min_t
    _check_head(c, [(0, c["nseq"], 256)])


def test_head_128x128_form_keeps_sparse_and_keys(dev):
    """Below the threshold: one call per sequence group (64-row tiles, then 128-row tiles), finalize = 0 then 1."""
    import snx
    c = _head_case(dev, 4, 2)
    assert c["T"] < snx.config("dec256_min_t")
    _check_head(c, c["groups"])


def test_head_flags_zero_is_the_recording_entry_point(dev):
    """flags = 0 with and without token keys is snx_decoder_splade_fwd_rec / _ex: the same bits as snx.ops hands out."""
    from snx import ops
    c = _head_case(dev, 4, 2)
    s, k, tw, tk = _run_head(c, 0, [(0, c["nseq"], 256)])
    rs, rk, rtw, rtk = ops.decoder_splade_fwd_tw(c["hd"], c["w"], c["bias"], c["cu"], c["mask"], 256)
    assert torch.equal(_bits(s), _bits(rs)) and torch.equal(k, rk) and torch.equal(_bits(tw), _bits(rtw)) and torch.equal(tk, rtk)
    s, k, tw, _ = _run_head(c, 0, [(0, c["nseq"], 256)], record=False)
    rs, rk, rtw = ops.decoder_splade_fwd(c["hd"], c["w"], c["bias"], c["cu"], c["mask"], 256)
    assert torch.equal(_bits(s), _bits(rs)) and torch.equal(k, rk) and torch.equal(_bits(tw), _bits(rtw))


# ------------------------------------------------------------------------------------------------------ model level
def _tiny_cfg():
    from oracle import splade_oracle as O
    # two layers: layer 0 global, layer 1 local (window +-8)
    return O.EncoderConfig(vocab_size=3000, hidden_size=256, intermediate_size=384, num_hidden_layers=2,
                           num_attention_heads=4, local_attention=16, pad_token_id=2999)


@pytest.fixture(scope="module")
def tiny():
    from oracle import splade_oracle as O
    cfg = _tiny_cfg()
    return cfg, O.perturb_params(O.init_params(cfg, seed=3), seed=4, scale=2.0, bias_mean=-0.1)


def _pairs(cfg, shapes, seed, dev):
    from oracle import splade_oracle as O
    gen = torch.Generator().manual_seed(seed)
    out = []
    for B, S in shapes:
        ids, mask = O.synth_ids(B, S, cfg, gen, ragged=True)
        out.append((ids.to(dev), mask.to(dev)))
    return out


# three sequence groups: below the persistent decoder's threshold (128x128 kernels, one call per group) and at it
@pytest.mark.parametrize("shapes", [[(4, 16), (3, 48), (2, 96)], [(8, 64), (4, 128), (4, 256)]], ids=["dec128", "dec256"])
def test_forward_many_without_token_weights_same_bits(dev, tiny, shapes):
    from tests.test_gpu_model import _build_model
    import snx
    cfg, params = tiny
    assert (sum(b * s for b, s in shapes) >= snx.config("dec256_min_t")) == (shapes[0][1] == 64)
    model = _build_model(cfg, params, dev)
    pairs = _pairs(cfg, shapes, 31, dev)
    gen = torch.Generator().manual_seed(32)
    gs = [torch.randn(b, cfg.vocab_size, generator=gen).to(dev) for b, _ in shapes]
    plist = list(model.parameters())

    def run(**kw):
        with torch.autocast(device_type="cuda", dtype=BF16):
            outs = model.forward_many(pairs, **kw)
        loss = sum((sp * g).sum() for (sp, _), g in zip(outs, gs))
        return outs, torch.autograd.grad(loss, plist)

    outs0, grads0 = run()
    outs1, grads1 = run(need_token_weights=False)
    for (sp0, tw0), (sp1, tw1) in zip(outs0, outs1):
        assert tw0 is not None and tw1 is None
        assert torch.equal(_bits(sp1.detach()), _bits(sp0.detach()))
    bad = [n for (n, _), a, b in zip(model.named_parameters(), grads0, grads1) if not torch.equal(_bits(a), _bits(b))]
    assert not bad, bad
    assert any(bool((g != 0).any()) for g in grads1)
    # inference (no autograd): the same
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=BF16):
        inf = model.forward_many(pairs, need_token_weights=False)
    for (sp0, _), (sp2, tw2) in zip(outs0, inf):
        assert tw2 is None and torch.equal(_bits(sp2), _bits(sp0.detach()))


def test_flagged_forward_writes_neither_token_weights_nor_token_keys(dev, tiny):
    """snx_model_forward with the flag into an arena and a token_weights buffer that the test filled with a sentinel: the
    buffer and the arena's token keys come back untouched, the arena is the smaller one, sparse has the bits of the
    unflagged forward, and a backward handed a token_weights gradient for that arena is refused (the Python wrapper raises;
    nothing is launched)."""
    from snx._lib import SnxError, check, fn
    from snx.encoder import _p, _stream
    from tests.test_gpu_model import _build_model
    cfg, params = tiny
    model = _build_model(cfg, params, dev)
    rt = model.runtime
    shapes = [(4, 16), (3, 48), (2, 96)]
    pairs = _pairs(cfg, shapes, 41, dev)
    T, B, V = sum(b * s for b, s in shapes), sum(b for b, _ in shapes), cfg.vocab_size
    flags = 1 | SNX_FWD_NO_TOKEN_WEIGHTS
    small = fn("snx_model_workspace_bytes_fwd")(C.byref(rt._desc), T, B, flags)
    assert small < fn("snx_model_workspace_bytes_fwd")(C.byref(rt._desc), T, B, 1) == \
        fn("snx_model_workspace_bytes")(C.byref(rt._desc), T, B, 1)
    off = fn("snx_model_token_keys_offset")(C.byref(rt._desc), T, B)
    assert off + 4 * T <= small
    with torch.autocast(device_type="cuda", dtype=BF16):
        ref_sparse, ref_tw, _, aux = rt.forward_many_impl(pairs, save=True)
    ids, mask, cu, pos, rg, rl, _, _, smax, groups = aux[:10]
    saved = torch.full((small + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    tw = torch.full((T,), TW_SENTINEL, dtype=torch.float32, device=dev)
    sparse = torch.empty((B, V), dtype=torch.float32, device=dev)
    check(fn("snx_model_forward")(C.byref(rt._desc), rt._param_ptrs(), _p(rt._weights()), _p(ids), _p(mask), _p(cu), _p(pos),
                                  _p(rg), _p(rl), _p(saved), _p(sparse), _p(tw), groups, T, B, smax, flags, _stream()),
          "snx_model_forward")
    torch.cuda.synchronize()
    assert torch.equal(_bits(sparse), _bits(ref_sparse))
    assert bool((tw == TW_SENTINEL).all()), "token_weights written under SNX_FWD_NO_TOKEN_WEIGHTS"
    assert bool((saved[off:off + 4 * T] == 0x5A).all()), "token keys written under SNX_FWD_NO_TOKEN_WEIGHTS"
    assert bool((saved[small:] == 0x5A).all()), "wrote behind the arena"
    g = torch.ones_like(sparse)
    g_tw = torch.ones((T,), dtype=torch.float32, device=dev)
    with pytest.raises(SnxError, match="SNX_E_ARG"):
        rt.backward_impl(saved, aux, g, g_tw=g_tw)
    grads = rt.backward_impl(saved, aux, g)                   # without one it is the ordinary backward
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in grads)
    # an unflagged forward (into the flagged one's arena when the allocator hands its block out again): its token keys
    # exist and the gradient is taken
    del saved
    full = torch.empty((fn("snx_model_workspace_bytes")(C.byref(rt._desc), T, B, 1),), dtype=torch.uint8, device=dev)
    check(fn("snx_model_forward")(C.byref(rt._desc), rt._param_ptrs(), _p(rt._weights()), _p(ids), _p(mask), _p(cu), _p(pos),
                                  _p(rg), _p(rl), _p(full), _p(sparse), _p(tw), groups, T, B, smax, 1, _stream()),
          "snx_model_forward")
    assert torch.equal(_bits(tw), _bits(ref_tw))
    rt.backward_impl(full, aux, g, g_tw=g_tw)
    torch.cuda.synchronize()


def test_autograd_through_dropped_token_weights_is_impossible(dev, tiny):
    """Python level: with the keyword there is no token_weights output to differentiate; the default still has one."""
    from tests.test_gpu_model import _build_model
    cfg, params = tiny
    model = _build_model(cfg, params, dev)
    (ids, mask), = _pairs(cfg, [(3, 32)], 51, dev)
    with torch.autocast(device_type="cuda", dtype=BF16):
        sp, tw = model(ids, mask)
        sp1, tw1 = model(ids, mask, need_token_weights=False)
        enc = model.encode(ids, mask)
    assert tw is not None and tw.requires_grad and tw1 is None and sp1.requires_grad
    assert torch.equal(_bits(sp.detach()), _bits(sp1.detach()))
    assert torch.equal(_bits(enc.detach()), _bits(sp.detach()))


# ---------------------------------------------------------------------------------------------------- trainer level
@pytest.mark.parametrize("fused", [True, False], ids=["forward_many", "three_calls"])
def test_trainer_parameters_same_bits(dev, tiny, monkeypatch, fused):
    """Two accumulation windows of micro_step + optimizer_step on the tiny model: through the trainer as it is (it passes
    need_token_weights=False) and with every runtime call forced back to the keyword's default.  `fused`: the one-pass
    micro-step (unpadded: the batches are ragged) / the reference's three model(...) calls (the micro-step arena)."""
    from oracle import splade_oracle as O
    from snx.encoder import EncoderRuntime
    from src.model.losses import SPLADELossV33
    from src.train.config.v33 import V33Config
    from src.train.core import ddp_trainer as T
    from tests.test_gpu_model import _build_model
    cfg, params = tiny
    gen = torch.Generator().manual_seed(61)
    batches = [O.synth_batch(4, 24, 70, cfg, gen, k=1, ragged=True) for _ in range(4)]
    conf = V33Config()
    conf.training.gradient_accumulation_steps = 2
    conf.training.learning_rate = 1e-3
    monkeypatch.setenv("SNX_FUSED_PASSES", "1" if fused else "0")
    real = EncoderRuntime.forward_many

    def run(force_default):
        seen = []

        def spy(self, pairs, lengths=None, need_token_weights=True):
            seen.append(need_token_weights)
            out = real(self, pairs, lengths, need_token_weights=True if force_default else need_token_weights)
            assert all((tw is None) == (not (force_default or need_token_weights)) for _, tw in out)
            return out

        monkeypatch.setattr(EncoderRuntime, "forward_many", spy)
        model = T.NativeDataParallel(_build_model(cfg, params, dev), n_buckets=3)
        loss_fn = SPLADELossV33(temperature=20.0, flops_warmup_steps=4).to(dev)
        opt = T.build_optimizer(model, conf)
        sch = T.build_scheduler(opt, 0, 4)
        losses, step = [], 0
        for i, b in enumerate(batches):
            last = (i + 1) % 2 == 0
            loss, _ = T.micro_step(model, loss_fn, b, step, dev, 2, last_of_window=last)
            losses.append(loss.clone())
            if last:
                T.optimizer_step(model, opt, sch, conf)
                step += 1
        torch.cuda.synchronize()
        assert seen and not any(seen), "the trainer asks for token_weights"
        assert len(seen) == (4 if fused else 12)
        return {n: p.detach().clone() for n, p in model.module.named_parameters()}, torch.stack(losses)

    p_old, l_old = run(True)
    p_new, l_new = run(False)
    assert torch.equal(_bits(l_new), _bits(l_old))
    bad = [n for n in p_old if not torch.equal(_bits(p_new[n]), _bits(p_old[n]))]
    assert not bad, bad
    moved = [n for n, p in p_new.items() if not torch.equal(p.cpu(), params[n])]
    assert len(moved) >= len(p_new) - 1                      # the optimizer steps really happened

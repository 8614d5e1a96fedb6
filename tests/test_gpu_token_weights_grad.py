"""token_weights is differentiable through the native SPLADE head (ref:src/model/splade_modern.py:86:
token_weights = sparse_scores.max(dim=-1).values, autograd-connected like sparse_repr).

For token row t with x = relu(logit[t, v*]), v* the FIRST column of the token's maximum:
    d logit[t, v*] += g_tw[t] * mask[t] / (1 + x)         (x > 0)
added to the max-pool gradient of the same logit before its one bf16 rounding (the oracle's bf16 cast point)."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_ulp_statement, sparse_ulp_stats

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _grad_stats(got, ref):
    g, r = got.double().flatten().cpu(), ref.double().flatten().cpu()
    return float((g @ r) / (g.norm() * r.norm() + 1e-30)), float((g - r).norm() / (r.norm() + 1e-30))


def _small():
    from oracle import splade_oracle as O
    from tests.test_gpu_model import _build_model, _small_cfg
    cfg = _small_cfg()
    params = O.perturb_params(O.init_params(cfg, seed=3), seed=4, scale=2.0, bias_mean=-0.1)
    return O, cfg, params, _build_model


def _batch(O, cfg, B, S, seed, one_token_rows=()):
    gen = torch.Generator().manual_seed(seed)
    ids, mask = O.synth_ids(B, S, cfg, gen, ragged=True)
    ids, mask = ids.clone(), mask.clone()
    for r in one_token_rows:                                  # a one-token sequence: its token owns every max-pool entry
        mask[r, 1:] = 0
        ids[r, 1:] = cfg.pad_token_id
    return ids, mask


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


# --------------------------------------------------------------------------------------------------------------- 1
def test_token_weights_are_connected(dev):
    O, cfg, params, build = _small()
    model = build(cfg, params, dev)
    ids, mask = _batch(O, cfg, 4, 32, 1)
    with torch.autocast(device_type="cuda", dtype=BF16):
        sparse, tw = model(ids.to(dev), mask.to(dev))
    assert tw.requires_grad
    w = torch.rand(tw.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    gs = torch.autograd.grad((tw * w).sum(), list(model.parameters()), allow_unused=True)
    names = [n for n, _ in model.named_parameters()]
    nz = {n: bool(g is not None and (g != 0).any()) for n, g in zip(names, gs)}
    assert nz["model.decoder.bias"] and nz["model.model.embeddings.tok_embeddings.weight"], nz
    assert sum(nz.values()) >= len(nz) - 1, nz                 # every tensor the token maximum depends on


# --------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("sparse_too", [True, False])
def test_fp32_gradients_match_the_oracle(dev, sparse_too):
    """fp32 path (no autocast), tiny config: loss = <g_s, sparse> + <g_tw, tw> (and token-only, g_s = 0) against the
    oracle's fp32 autograd on every parameter; padded rows and one-token rows included."""
    from oracle import splade_oracle as O
    from tests.test_gpu_model import _build_model
    cfg = O.EncoderConfig.tiny()
    params = O.perturb_params(O.init_params(cfg, seed=11), seed=12, scale=2.0, bias_mean=-0.1)
    model = _build_model(cfg, params, dev)
    ids, mask = _batch(O, cfg, 5, 24, 13, one_token_rows=(1, 3))
    gen = torch.Generator().manual_seed(14)
    g_s = torch.randn(5, cfg.vocab_size, generator=gen) * (1.0 if sparse_too else 0.0)
    g_tw = torch.randn(5, 24, generator=gen)
    sp, tw = model(ids.to(dev), mask.to(dev))
    ((sp * g_s.to(dev)).sum() + (tw * g_tw.to(dev)).sum()).backward()
    leaves = {n: p.clone().requires_grad_(True) for n, p in params.items()}
    osp, otw = O.splade_forward(leaves, cfg, ids, mask, "fp32")
    ((osp * g_s).sum() + (otw * g_tw).sum()).backward()
    assert float((tw.detach().cpu() - otw.detach()).abs().max()) <= 1e-5
    bad = {}
    for n, p in model.named_parameters():
        cos, rel = _grad_stats(p.grad, leaves[n].grad)
        if not (cos >= 0.99999 and rel <= 2e-4):
            bad[n] = (cos, rel)
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------- 3
def _pinned_oracle(O, cfg, params, batches, rows, vstar, gss, gtws):
    """bf16 oracle with both routings pinned to the native ones: max-pool via route_rows, token maximum via a gather of
    log1p(relu(logits).float()) * mask at the native v*."""
    leaves = {n: p.clone().requires_grad_(True) for n, p in params.items()}
    loss = 0.0
    for (ids, mask), r, v, g_s, g_tw in zip(batches, rows, vstar, gss, gtws):
        logits = O.encoder_logits(leaves, cfg, ids, mask, "bf16")
        s = torch.log1p(torch.relu(logits).float()) * mask.unsqueeze(-1).float()
        sparse = torch.gather(s, 1, r.clamp(0, s.shape[1] - 1).unsqueeze(1)).squeeze(1)
        tw = torch.gather(s, 2, v.view(s.shape[0], s.shape[1], 1)).squeeze(-1)
        loss = loss + (sparse * g_s).sum() + (tw * g_tw).sum()
    loss.backward()
    return {n: l.grad for n, l in leaves.items()}


def test_bf16_routing_and_gradients_match_the_pinned_oracle(dev):
    """Under autocast, a ragged micro-step of two sequence groups (one call, one-token rows included): the native
    token arg-max equals the oracle's wherever the top-2 gap is clear of the bf16 noise, and with both routings pinned
    every parameter gradient meets the bounds of test_gpu_parity_full.py."""
    O, cfg, params, build = _small()
    model = build(cfg, params, dev)
    rt = model.runtime
    rt.keep_last_ctx = True
    batches = [_batch(O, cfg, 4, 24, 21, one_token_rows=(2,)), _batch(O, cfg, 3, 96, 22)]
    gen = torch.Generator().manual_seed(23)
    gss = [torch.randn(ids.shape[0], cfg.vocab_size, generator=gen) for ids, _ in batches]
    gtws = [torch.randn(ids.shape, generator=gen) * 4.0 for ids, _ in batches]
    with torch.autocast(device_type="cuda", dtype=BF16):
        outs = rt.forward_many([(i.to(dev), m.to(dev)) for i, m in batches])
    saved, aux = rt.last_ctx
    rows_all = rt.routing_rows(saved, aux).cpu()
    v_all = rt.token_routing(saved, aux).cpu()
    sum((sp * g.to(dev)).sum() + (tw * t.to(dev)).sum() for (sp, tw), g, t in zip(outs, gss, gtws)).backward()
    rows, vstar, r0, t0 = [], [], 0, 0
    for ids, mask in batches:
        B, S = ids.shape
        rows.append(rows_all[r0:r0 + B])
        vstar.append(v_all[t0:t0 + B * S].view(B, S))
        r0 += B
        t0 += B * S
    checked = 0
    for (ids, mask), v, (sp, tw) in zip(batches, vstar, outs):
        with torch.no_grad():
            ref_sp, ref_tw = O.splade_forward(params, cfg, ids, mask, "bf16")
            x = torch.relu(O.encoder_logits(params, cfg, ids, mask, "bf16")).float()
        assert_ulp_statement(sparse_ulp_stats(tw.detach().reshape(-1), ref_tw.reshape(-1)), "token_weights")
        top2 = torch.topk(x, 2, dim=-1)
        bits = top2.values.to(BF16).view(torch.int16).to(torch.int32)
        clear = (mask != 0) & (top2.values[..., 0] > 0) & ((bits[..., 0] - bits[..., 1]) > 2)
        assert torch.equal(v[clear], top2.indices[..., 0][clear])
        assert (v[mask == 0] == 0).all()
        checked += int(clear.sum())
    assert checked >= 0.3 * sum(int(m.sum()) for _, m in batches), checked
    og = _pinned_oracle(O, cfg, params, batches, rows, vstar, gss, gtws)
    bad = {}
    for n, p in model.named_parameters():
        cos, rel = _grad_stats(p.grad, og[n])
        lim = 5e-2 if n == "model.decoder.bias" else 2e-2      # the relu-gate floor of test_gpu_parity_full.py (unmasked)
        if cos < 0.999 or rel > lim:
            bad[n] = (cos, rel)
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------- 4
def test_coincident_entries_add_before_the_bf16_rounding(dev):
    """Head-level: one-token sequences (every max-pool entry and the token maximum share the logit) plus longer ones; the
    routed gradients equal the dense reference built from the native routing, where the two upstream gradients of one
    logit are added in fp32 and rounded to bf16 ONCE."""
    from snx import ops
    torch.manual_seed(31)
    H, V = 256, 1000
    lens = [1, 1, 7, 1, 33, 64]
    T = sum(lens)
    cu = torch.tensor(np.cumsum([0] + lens), dtype=torch.int32, device=dev)
    hd = (torch.randn(T, H) * 0.5).to(BF16).to(dev)
    W = (torch.randn(V, H) * 0.1).to(BF16).to(dev)
    bias = (torch.randn(V) * 0.5 - 0.2).to(dev)
    mask = torch.ones(T, dtype=torch.int64, device=dev)
    mask[T - 5:] = 0                                          # a padded tail in the last sequence
    sparse, keys, tw, tkeys = ops.decoder_splade_fwd_tw(hd, W, bias, cu, mask, max(lens))
    nseq = len(lens)
    g = torch.randn(nseq, V, device=dev)
    g_tw = torch.randn(T, device=dev) * 3.0
    dhd, gE, gb = ops.splade_bwd_tw(g, keys, g_tw, tkeys, hd, W, cu, max(lens))
    # dense reference on the native routing
    k = keys.cpu().to(torch.int64) & 0xFFFFFFFF
    tk = tkeys.cpu().to(torch.int64) & 0xFFFFFFFF
    rbf = lambda t: t.to(BF16).float()                         # noqa: E731
    x_of = lambda key: (key >> 16).to(torch.int32).to(torch.int16).view(BF16).float()   # noqa: E731
    up = torch.zeros(T, V, dtype=torch.float64)
    X = torch.zeros(T, V)
    cu_h = cu.cpu().tolist()
    for b in range(nseq):
        rows = cu_h[b] + (0xFFFF - (k[b] & 0xFFFF))
        xv = x_of(k[b])
        live = xv > 0
        vv = torch.arange(V)[live]
        up[rows[live], vv] += g.cpu()[b, live].double()
        X[rows[live], vv] = xv[live]
    vstar = 0xFFFF - (tk & 0xFFFF)
    xt = x_of(tk)
    live = xt > 0
    tt = torch.arange(T)[live]
    up[tt, vstar[live]] += g_tw.cpu()[live].double()
    X[tt, vstar[live]] = xt[live]
    coef = torch.where(X > 0, rbf(up.float() / (1.0 + X)), torch.zeros(()))
    one_tok = [cu_h[b] for b in range(nseq) if lens[b] == 1]
    assert all(bool(live[t]) for t in one_tok)                # the coincident case is exercised
    ref_gb = coef.double().sum(0)
    assert torch.allclose(gb.cpu().double(), ref_gb, rtol=1e-5, atol=1e-6)
    ref_gE = coef.double().t() @ hd.cpu().double()
    assert torch.allclose(gE.cpu().double(), ref_gE, rtol=1e-4, atol=1e-5)
    ref_dhd = (coef.double() @ W.cpu().double()).float()
    d = (dhd.cpu().float() - ref_dhd).abs()
    assert float((d > ref_dhd.abs() * 2 ** -7 + 1e-5).float().mean()) == 0.0
    # what the rounding-once rule rules out: per-direction rounding moves db on the coincident columns
    two = torch.zeros(T, V)
    for t in one_tok:
        v = int(vstar[t])
        b = cu_h.index(t)
        two[t, v] = float(rbf(torch.tensor(float(g[b, v]) / (1.0 + float(X[t, v])))) +
                          rbf(torch.tensor(float(g_tw[t]) / (1.0 + float(X[t, v])))))
    moved = [t for t in one_tok if float(two[t, int(vstar[t])]) != float(coef[t, int(vstar[t])])]
    for t in moved:
        v = int(vstar[t])
        assert abs(float(gb[v]) - float(ref_gb[v])) < abs(float(two[t, v]) - float(coef[t, v])) / 4
    # the value half of tkeys is the value behind tw; masked tokens read 0
    assert torch.equal(tw.cpu()[mask.cpu() == 0], torch.zeros(5))
    assert (tk[mask.cpu() == 0] == 0xFFFF).all()
    xb = torch.expm1(tw.cpu().double()).float().to(BF16).view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(xb, tk >> 16)
    # deterministic
    dhd2, gE2, gb2 = ops.splade_bwd_tw(g, keys, g_tw, tkeys, hd, W, cu, max(lens))
    assert torch.equal(dhd, dhd2) and torch.equal(gE, gE2) and torch.equal(gb, gb2)
    # no token gradient: exactly the sparse-only backward
    a = ops.splade_bwd_tw(g, keys, None, tkeys, hd, W, cu, max(lens))
    z = ops.splade_bwd_tw(g, keys, torch.zeros_like(g_tw), tkeys, hd, W, cu, max(lens))
    assert all(torch.equal(p, q) for p, q in zip(a, z))


# --------------------------------------------------------------------------------------------------------------- 5
def _step(model, pairs, gss, gtws, tw_mode="used"):
    model.zero_grad(set_to_none=True)
    with torch.autocast(device_type="cuda", dtype=BF16):
        outs = [model(i, m) for i, m in pairs]
    loss = sum((sp * g).sum() for (sp, _), g in zip(outs, gss))
    if tw_mode == "used":
        loss = loss + sum((tw * t).sum() for (_, tw), t in zip(outs, gtws))
    elif tw_mode == "zero":
        loss = loss + sum((tw * 0.0).sum() for _, tw in outs)
    loss.backward()
    return outs, _grads(model)


def test_bit_identities(dev):
    import snx
    O, cfg, params, build = _small()
    gen = torch.Generator().manual_seed(41)
    pairs = [tuple(t.to(dev) for t in _batch(O, cfg, 4, S, 41 + j, one_token_rows=(1,))) for j, S in enumerate((24, 80, 80))]
    gss = [torch.randn(4, cfg.vocab_size, generator=gen).to(dev) for _ in pairs]
    gtws = [torch.randn(p[0].shape, generator=gen).to(dev) for p in pairs]
    m = build(cfg, params, dev)
    m.runtime.step_arena_on = False
    # tw unused / multiplied by zero: the same bits
    _, g_unused = _step(m, pairs, gss, gtws, "unused")
    _, g_zero = _step(m, pairs, gss, gtws, "zero")
    for n in g_unused:
        assert torch.equal(g_unused[n], g_zero[n]), n
    # two identical backwards
    _, g1 = _step(m, pairs, gss, gtws)
    _, g2 = _step(m, pairs, gss, gtws)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    assert not torch.equal(g1["model.decoder.bias"], g_unused["model.decoder.bias"])
    # forward_many (one call, three sequence groups) == three calls, bit for bit
    m.zero_grad(set_to_none=True)
    with torch.autocast(device_type="cuda", dtype=BF16):
        many = m.runtime.forward_many(pairs)
    sum((sp * g).sum() + (tw * t).sum() for (sp, tw), g, t in zip(many, gss, gtws)).backward()
    g_many = _grads(m)
    # the three-call loop through the micro-step arena == the fused pass
    ma = build(cfg, params, dev)
    assert ma.runtime.step_arena_on
    for _ in range(2):                                          # the first micro-step teaches the capacity
        _, g_arena = _step(ma, pairs, gss, gtws)
    assert ma.runtime.arena_stats["placed"] == 3
    for n in g_many:
        assert torch.equal(g_arena[n], g_many[n]), n
    # padded vs unpadded (lengths): the summation tree of other row blocks only
    m.zero_grad(set_to_none=True)
    lengths = [p[1].sum(1).cpu() for p in pairs]
    with torch.autocast(device_type="cuda", dtype=BF16):
        pk = m.runtime.forward_many(pairs, lengths)
    for (s1, t1), (s2, t2) in zip(many, pk):
        assert torch.equal(s1, s2) and torch.equal(t1, t2)
    sum((sp * g).sum() + (tw * t).sum() for (sp, tw), g, t in zip(pk, gss, gtws)).backward()
    g_pk = _grads(m)
    for n in g_many:
        cos, rel = _grad_stats(g_pk[n], g_many[n])
        assert cos > 0.99999 and rel < 2e-3, (n, cos, rel)
    # the 256x192 decoder vs the 128x128 kernel: the same token keys wherever the two GEMMs (other MFMA shapes, other
    # fp32 summation orders) give the same token maximum; gradients bit-identical when the forwards are
    res = {}
    before = {k: snx.config(k) for k in ("dec256", "dec256_min_t")}
    for d256 in (0, 1):
        snx.configure(dec256=d256, dec256_min_t=1)
        try:
            mm = build(cfg, params, dev)
            mm.runtime.step_arena_on = False
            mm.runtime.keep_last_ctx = True
            mm.zero_grad(set_to_none=True)
            with torch.autocast(device_type="cuda", dtype=BF16):
                o = mm.runtime.forward_many(pairs)
            tk = mm.runtime.token_routing(*mm.runtime.last_ctx).clone()
            sum((sp * g).sum() + (tw * t).sum() for (sp, tw), g, t in zip(o, gss, gtws)).backward()
            res[d256] = (tk, torch.cat([tw.reshape(-1) for _, tw in o]).detach(), [sp.detach() for sp, _ in o], _grads(mm))
            mm.runtime.last_ctx = None
        finally:
            snx.configure(**before)
    (tk0, tw0, sp0, g0), (tk1, tw1, sp1, g1_) = res[0], res[1]
    same = tw0 == tw1
    assert float(same.float().mean()) >= 0.97
    assert float((tk0 == tk1)[same].float().mean()) >= 0.999
    if bool(same.all()) and all(torch.equal(a, b) for a, b in zip(sp0, sp1)):
        assert torch.equal(tk0, tk1)
        for n in g0:
            assert torch.equal(g0[n], g1_[n]), n
    else:
        for n in g0:
            cos, rel = _grad_stats(g1_[n], g0[n])
            assert cos > 0.999 and rel < 3e-2, (n, cos, rel)

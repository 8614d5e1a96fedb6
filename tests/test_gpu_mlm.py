"""MLM pre-training on the GPU (csrc/mlm.hip, snx/mlm.py, the hidden-state entry points of csrc/model.hip,
src/model/mlm_modern.py, src/train/cli/pretrain_mlm.py) against the host references of tests/mlm_reference.py.
Needs a real MI355X: pytest -m gpu.

Tolerances:
  * masking: exact (integer arithmetic and float64 comparisons on both sides);
  * forward: lse and the row loss inside the acceptance interval (which bf16 logits an fp32 accumulation may produce)
    plus 2e-6 relative to |lse| for the device's fp32 exp / log;
  * backward: each of dh, dE, dbias within 4x its floor (two fp32 evaluations of the contract with permuted contraction
    orders, tests/mlm_reference.gradient_floors) of the float64 contract, normalised by the tensor's largest magnitude;
  * the fork of the model runtime: bit for bit."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import mlm_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- (a) masking ------------------------------------------------------------------------------------------------------
def test_mask_tokens_equals_the_reference(dev):
    from snx import mlm
    rng = np.random.default_rng(11)
    B, S, V = 5, 37, 1000
    ids = rng.integers(5, V, size=(B, S), dtype=np.int64)
    lens = np.array([37, 1, 20, 36, 9])
    att = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    ids[:, 0] = 0
    ids[att == 0] = 2
    ids[2, 5] = 3
    sample = np.array([0, 1, 2 ** 20 + 3, 77, 2 ** 33 + 5], dtype=np.int64)    # (t beyond 32 and 48 bits)
    kw = dict(special_ids=(0, 1, 2, 3, 4), mask_id=4, vocab_size=V, seed=0xFEDCBA9876543210, epoch=3, p=0.4)
    want_ids, want_labels, sel = R.mask_tokens_ref(ids, att, sample, **kw)
    assert 10 < sel.sum() < sel.size
    D = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    got_ids, got_labels = mlm.mask_tokens(D(ids), D(att), D(sample), **kw)
    assert got_ids.dtype == torch.int64 and got_labels.dtype == torch.int64
    assert np.array_equal(got_ids.cpu().numpy(), want_ids) and np.array_equal(got_labels.cpu().numpy(), want_labels)
    # the same rows in two other calls (another batch composition, another launch shape): the same tokens
    for part in ([3, 0], [1, 2, 4]):
        o, l = mlm.mask_tokens(D(ids[part]), D(att[part]), D(sample[part]), **kw)
        assert np.array_equal(o.cpu().numpy(), want_ids[part]) and np.array_equal(l.cpu().numpy(), want_labels[part])
    with pytest.raises(ValueError):
        mlm.mask_tokens(torch.zeros((1, 65536), dtype=torch.int64, device=dev),
                        torch.ones((1, 65536), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), **kw)


# ---- (b), (c) the cross-entropy ------------------------------------------------------------------------------------------
def _to_dev(case, dev):
    return (torch.from_numpy(case["h"]).to(dev).to(torch.bfloat16), torch.from_numpy(case["E"]).to(dev).to(torch.bfloat16),
            torch.from_numpy(case["bias"]).to(dev), torch.from_numpy(case["labels"]).to(dev))


FWD_CASES = [(M, V, H, v) for (M, V, H) in R.SHAPES[:4] for v in ("rand", "m30")] + [R.SHAPES[4] + ("m30",)]


@pytest.mark.parametrize("M,V,H,variant", FWD_CASES)
def test_cross_entropy_forward_inside_the_acceptance_interval(dev, M, V, H, variant):
    from snx import mlm
    case = R.ce_case(M, V, H, variant)
    labels = case["labels"]
    ref = R.ce_forward64(case["h"], case["E"], case["bias"], labels)
    acc = R.acceptance(ref, labels)
    h, E, bias, lab = _to_dev(case, dev)
    fwd = mlm.ce_forward(h, lab, E, bias)
    lse, row_loss, loss = fwd.lse.cpu().numpy(), fwd.row_loss.cpu().numpy(), float(fwd.loss)
    rows = np.arange(M)
    scale = np.maximum(np.abs(ref["lse"]), np.abs(ref["z"][rows, labels]))
    print(f"\n[{M}x{V}x{H} {variant}] loss {loss:.6f} ref {ref['loss']:.6f}; max |lse - ref| "
          f"{np.abs(lse - ref['lse']).max():.3e}, widest lse interval {(acc['lse_hi'] - acc['lse_lo']).max():.3e}; "
          f"max |row loss - ref| {np.abs(row_loss - ref['row_loss']).max():.3e}, widest loss interval "
          f"{(acc['loss_hi'] - acc['loss_lo']).max():.3e}")
    assert np.isfinite(lse).all() and np.isfinite(row_loss).all()
    bad = ~R.inside(lse, acc["lse_lo"], acc["lse_hi"], scale)
    assert not bad.any(), (np.nonzero(bad)[0][:8], lse[bad][:8], acc["lse_lo"][bad][:8], acc["lse_hi"][bad][:8])
    bad = ~R.inside(row_loss, acc["loss_lo"], acc["loss_hi"], scale)
    assert not bad.any(), (np.nonzero(bad)[0][:8], row_loss[bad][:8], acc["loss_lo"][bad][:8], acc["loss_hi"][bad][:8])
    # the stored logits are reachable values, the pad columns zero
    z = fwd.z.float().cpu().numpy()
    assert ((z[:, :V] >= acc["z_lo"]) & (z[:, :V] <= acc["z_hi"])).all() and (z[:, V:] == 0).all()
    # the mean: a sum of M fp32 terms and one division
    lo, hi = acc["loss_lo"].mean(), acc["loss_hi"].mean()
    tol = (R.EXP_LOG_REL + (M + 1) * 2.0 ** -24) * scale.max()
    assert lo - tol <= loss <= hi + tol, (loss, lo, hi)
    if variant == "m30" and M > 5:
        assert abs(row_loss[4] - math.log(V)) <= R.EXP_LOG_REL * (30 + math.log(V))        # zero row, constant bias
        assert np.abs(ref["z"][5]).max() > 150                                                # the row scaled to |z| ~ 200


@functools.lru_cache(maxsize=None)
def _floors():
    return R.gradient_floors()


@pytest.mark.parametrize("M,V,H", R.SHAPES)
def test_cross_entropy_backward_within_four_floors_of_float64(dev, M, V, H):
    from snx import mlm
    case = R.ce_case(M, V, H, "rand")
    labels = case["labels"]
    up = 0.75
    ref = R.ce_forward64(case["h"], case["E"], case["bias"], labels)
    want = R.ce_backward64(case["h"], case["E"], ref["z"], ref["lse"], labels, up)
    h, E, bias, lab = _to_dev(case, dev)
    ET = mlm.transpose_embeddings(E)
    assert torch.equal(ET[:, :V], E.t()) and (ET[:, V:] == 0).all()
    dE = torch.zeros((V, H), dtype=torch.float32, device=dev)
    dbias = torch.zeros((V,), dtype=torch.float32, device=dev)
    fwd = mlm.ce_forward(h, lab, E, bias)
    dh = mlm.ce_backward(fwd, h, lab, ET, torch.tensor(up, device=dev), dE, dbias)
    fl = _floors()
    got = {"dh": dh.float().cpu().numpy(), "dE": dE.cpu().numpy(), "dbias": dbias.cpu().numpy()}
    diffs = {k: R.normalised_diff(got[k], want[k]) for k in got}
    print(f"\n[{M}x{V}x{H}] normalised max differences {diffs}; floors {fl}")
    for k in got:
        assert np.isfinite(got[k]).all()
        assert diffs[k] <= 4 * fl[k], (k, diffs[k], fl[k])
    # the gradients ACCUMULATE into dE and dbias: a second backward on top doubles them (x + x is exact)
    fwd = mlm.ce_forward(h, lab, E, bias)
    mlm.ce_backward(fwd, h, lab, ET, torch.tensor(up, device=dev), dE, dbias)
    assert np.array_equal(dE.cpu().numpy(), 2 * got["dE"]) and np.array_equal(dbias.cpu().numpy(), 2 * got["dbias"])


# ---- (d) reproducibility, the empty batch, autograd ----------------------------------------------------------------------
def test_cross_entropy_bit_reproducible_and_empty_batch(dev):
    from snx import mlm
    M, V, H = 300, 3000, 768
    case = R.ce_case(M, V, H, "rand")
    h, E, bias, lab = _to_dev(case, dev)
    ET = mlm.transpose_embeddings(E)
    runs = []
    for _ in range(2):
        w = E.float().clone().requires_grad_(True)
        hh, bb = h.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        loss = mlm.cross_entropy_rows(hh, lab, E, bb, weight=w, ET=ET)
        (loss * 3.0).backward()
        runs.append((loss.detach().clone(), hh.grad.clone(), w.grad.clone(), bb.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert all(torch.isfinite(t).all() for t in runs[0]) and float(runs[0][2].abs().max()) > 0
    # M == 0: loss 0, zero gradients, nothing launched
    w = E.float().clone().requires_grad_(True)
    hh, bb = h[:0].clone().requires_grad_(True), bias.clone().requires_grad_(True)
    loss = mlm.cross_entropy_rows(hh, lab[:0], E, bb, weight=w, ET=ET)
    assert float(loss.detach()) == 0.0
    loss.backward()
    torch.cuda.synchronize()
    assert hh.grad.shape == (0, H) and float(w.grad.abs().max()) == 0.0 and float(bb.grad.abs().max()) == 0.0


# ---- (e) the fork of the model runtime ------------------------------------------------------------------------------------
def _tiny_cfg(layers=2):
    from oracle import splade_oracle as O
    return O.EncoderConfig(vocab_size=3000, hidden_size=256, intermediate_size=384, num_hidden_layers=layers,
                           num_attention_heads=4, local_attention=16, pad_token_id=2999)


def _build_model(cfg, params, dev):
    from src.model.splade_modern import SPLADEModernBERT
    geom = {k: getattr(cfg, k) for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
                                          "num_attention_heads", "global_attn_every_n_layers", "local_attention",
                                          "global_rope_theta", "local_rope_theta", "norm_eps", "pad_token_id")}
    m = SPLADEModernBERT(config=geom)
    sd = {k: v.clone() for k, v in params.items()}
    sd["model.decoder.weight"] = sd["model.model.embeddings.tok_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def test_hidden_entry_points_change_nothing(dev):
    """hd of snx_model_forward_hidden is the hd an ordinary forward leaves in its arena; the _hd backward, started from
    what the SPLADE backward hands to the head, reproduces every parameter gradient of the ordinary backward."""
    from oracle import splade_oracle as O
    from snx import ops
    from snx._lib import fn
    cfg = _tiny_cfg()
    params = O.perturb_params(O.init_params(cfg, seed=3), seed=4, scale=2.0, bias_mean=-0.1)
    model = _build_model(cfg, params, dev)
    rt = model.runtime
    ids, mask = O.synth_ids(4, 48, cfg, torch.Generator().manual_seed(8), ragged=True)
    ids, mask = ids.to(dev), mask.to(dev)
    V, H = cfg.vocab_size, cfg.hidden_size
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        sparse, tw, saved, aux = rt.forward_many_impl([(ids, mask)], save=True)
        T, B, S = aux[6], aux[7], aux[8]
        off = fn("snx_model_hd_offset")(C.byref(rt._desc), T, B)
        hd_ref = saved[off:off + T * H * 2].view(torch.bfloat16).view(T, H).clone()
        hd, saved_h, aux_h = rt.forward_hidden_impl(ids, mask, save=True)
        assert torch.equal(hd, hd_ref) and float(hd.float().abs().max()) > 0
        # the ordinary backward, both output gradients
        gen = torch.Generator().manual_seed(9)
        g_sparse = (torch.randn((B, V), generator=gen) * (torch.rand((B, V), generator=gen) < 0.2)).to(dev)
        g_tw = torch.randn((T,), generator=gen).to(dev)
        want = rt.backward_impl(saved, aux, g_sparse, g_tw=g_tw)
        # its first stage on its own, then the _hd backward seeded with that stage's embedding and bias gradients
        koff = fn("snx_model_keys_offset")(C.byref(rt._desc), T, B)
        toff = fn("snx_model_token_keys_offset")(C.byref(rt._desc), T, B)
        keys = saved[koff:koff + B * V * 4].view(torch.int32).view(B, V)
        tkeys = saved[toff:toff + T * 4].view(torch.int32)
        E, _ = rt.mlm_embeddings()
        A, dE, dbias = ops.splade_bwd_tw(g_sparse, keys, g_tw, tkeys, hd_ref, E, aux[2], S)
        grads = rt.grad_buffers()
        grads[0].copy_(dE)
        grads[-1].copy_(dbias)
        got = rt.backward_hidden_impl(saved_h, aux_h, A, grads)
    torch.cuda.synchronize()
    names = [n for n, _ in model.named_parameters()]
    assert len(want) == len(got) == len(names)
    for n, a, b in zip(names, want, got):
        assert float(a.abs().max()) > 0, n
        assert torch.equal(a, b), (n, float((a - b).abs().max()))
    with pytest.raises(NotImplementedError):                      # the fp32 parity runtime has no MLM path
        rt.forward_hidden_impl(ids, mask, save=True)


# ---- (f) the model ---------------------------------------------------------------------------------------------------------
def _ulp_bf16(x):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -120))) - 7)


def _masked_batch(cfg, seed=8, p=0.3):
    from oracle import splade_oracle as O
    ids, mask = O.synth_ids(4, 48, cfg, torch.Generator().manual_seed(seed), ragged=True)
    masked, labels, sel = R.mask_tokens_ref(ids.numpy(), mask.numpy(), np.arange(4), special_ids=(cfg.pad_token_id,),
                                            mask_id=cfg.vocab_size - 2, vocab_size=cfg.vocab_size, seed=5, p=p)
    assert sel.sum() >= 20
    return torch.from_numpy(masked), mask, torch.from_numpy(labels), sel


def test_mlm_model_loss_and_gradients_vs_oracle(dev):
    """Loss: the oracle's bf16-mode logits of the masked rows with an fp32 cross-entropy; the GPU's hidden states differ
    from the oracle's by the ULP statement of tests/helpers.py (a logit is the oracle's bf16 value or a close neighbour:
    within two of its ulps, or within logit_abs_tol = 1.2e-2), so every logit may move by w = max(1.2e-2, 2 ulp) and the
    row-loss interval of the forward test is taken over [z - w, z + w].  Gradients: the statement of the pinned-routing
    parity test of this geometry class (cosine >= 0.999, relative L2 <= 2e-2 per tensor); MLM has no routing to pin."""
    import torch.nn.functional as F
    from oracle import splade_oracle as O
    from src.model.mlm_modern import MLMModernBERT
    cfg = _tiny_cfg()
    params = O.perturb_params(O.init_params(cfg, seed=3), seed=4, scale=2.0, bias_mean=-0.1)
    masked, mask, labels, sel = _masked_batch(cfg)
    selt = torch.from_numpy(sel)
    leaves = {n: p.clone().requires_grad_(True) for n, p in params.items()}
    logits = O.encoder_logits(leaves, cfg, masked, mask, "bf16")
    zo = logits[selt].float()
    oloss = F.cross_entropy(zo, labels[selt])
    oloss.backward()
    model = MLMModernBERT(_build_model(cfg, params, dev))
    assert [n for n, _ in model.named_parameters()] == O.param_names(cfg)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        loss = model(masked.to(dev), mask.to(dev), labels.to(dev))
    assert loss.dim() == 0 and loss.requires_grad and model.last_masked_count == int(sel.sum())
    loss.backward()
    z = zo.detach().double().numpy()
    y = labels[selt].numpy()
    w = np.maximum(1.2e-2, 2 * _ulp_bf16(z))
    rows = np.arange(len(y))
    a = z - w; a[rows, y] = (z + w)[rows, y]
    b = z + w; b[rows, y] = (z - w)[rows, y]
    lo = (R.logsumexp64(a) - (z + w)[rows, y]).mean()
    hi = (R.logsumexp64(b) - (z - w)[rows, y]).mean()
    print(f"\nMLM model loss {float(loss.detach()):.6f}, oracle {float(oloss.detach()):.6f}, interval [{lo:.6f}, {hi:.6f}]")
    assert lo <= float(loss.detach()) <= hi
    stats = {}
    for name, prm in model.named_parameters():
        g, r = prm.grad.double().cpu().flatten(), leaves[name].grad.double().flatten()
        stats[name] = (float((g @ r) / (g.norm() * r.norm() + 1e-30)), float((g - r).norm() / (r.norm() + 1e-30)))
    worst = min(stats.items(), key=lambda kv: kv[1][0])
    print(f"worst gradient cosine {worst}; largest relative L2 {max(v[1] for v in stats.values()):.3e}")
    bad = {n: v for n, v in stats.items() if v[0] < 0.999 or v[1] > 2e-2}
    assert not bad, bad
    # outside autocast the fp32 parity runtime would run: it has no MLM head
    with pytest.raises(NotImplementedError):
        model(masked.to(dev), mask.to(dev), labels.to(dev))
    # no masked token: loss 0, zero gradients
    model.zero_grad(set_to_none=True)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        loss0 = model(masked.to(dev), mask.to(dev), torch.full_like(labels, -100).to(dev))
    loss0.backward()
    assert float(loss0.detach()) == 0.0 and all(float(p.grad.abs().max()) == 0.0 for p in model.parameters())


# ---- (g) training smoke -----------------------------------------------------------------------------------------------------
def test_thirty_steps_on_one_batch_halve_the_loss(dev):
    from oracle import splade_oracle as O
    from src.model.mlm_modern import MLMModernBERT
    cfg = _tiny_cfg()
    model = MLMModernBERT(_build_model(cfg, O.init_params(cfg, seed=3), dev))
    masked, mask, labels, _ = _masked_batch(cfg, seed=21)
    masked, mask, labels = masked.to(dev), mask.to(dev), labels.to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.0)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            loss = model(masked, mask, labels)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        final = float(model(masked, mask, labels))
    first = float(losses[0])
    print(f"\nloss {first:.4f} -> {final:.4f} after 30 steps")
    assert math.isfinite(final) and final <= 0.5 * first, (first, final)


# ---- (h) the CLI -------------------------------------------------------------------------------------------------------------
def test_pretrain_cli_writes_a_checkpoint_the_splade_trainer_reads(dev, tmp_path):
    import json
    import logging
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.cli import pretrain_mlm
    from src.train.core import ddp_trainer as T
    geom = dict(vocab_size=3000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
                local_attention=16, pad_token_id=2999)
    (tmp_path / "geom.json").write_text(json.dumps(geom))
    data = tmp_path / "data"
    data.mkdir()
    rng = np.random.default_rng(4)
    words = [f"w{i}" for i in range(200)]
    line = lambda: " ".join(rng.choice(words, size=int(rng.integers(5, 40))))   # noqa: E731
    (data / "train.txt").write_text("\n".join(line() for _ in range(40)) + "\n")
    (data / "val.txt").write_text("\n".join(line() for _ in range(8)) + "\n")
    out = tmp_path / "out"
    (tmp_path / "cfg.yaml").write_text(
        f"model_name: {tmp_path / 'geom.json'}\ndata_dir: {data}\nmax_length: 32\noutput_dir: {out}\nepochs: 1\n"
        "batch_size: 8\ngrad_accum: 1\nlr: 1.0e-3\nweight_decay: 0.01\nwarmup_ratio: 0.2\nmlm_probability: 0.15\n"
        "save_steps: 3\neval_steps: 2\nlogging_steps: 1\ndataloader_workers: 0\nseed: 42\n")
    assert pretrain_mlm.main(["--config", str(tmp_path / "cfg.yaml"), "--tokenizer", "hash:3000"]) == 0
    ckpt = T.find_latest_checkpoint(str(out))
    assert ckpt is not None and ckpt.endswith("_step5")
    logging.getLogger("src.model.splade_modern").setLevel(logging.ERROR)
    fresh = SPLADEModernBERT(config=geom)
    before = fresh.model.head.dense.weight.detach().clone()
    ts = T.load_checkpoint(fresh, None, None, ckpt)
    assert ts["global_step"] == 5 and not torch.equal(before, fresh.model.head.dense.weight.detach())
    only = SPLADEModernBERT(config=geom)
    assert T.load_checkpoint(only, None, None, str(out / "final_model")) == {"epoch": -1, "global_step": 0}
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), only.state_dict().values()))
    assert SPLADEModernBERT(model_name=str(out / "final_model")).vocab_size == 3000
    # a world size above 1 is refused with a message
    os.environ["WORLD_SIZE"] = "2"
    try:
        with pytest.raises(SystemExit, match="one process"):
            pretrain_mlm.main(["--config", str(tmp_path / "cfg.yaml"), "--tokenizer", "hash:3000"])
    finally:
        del os.environ["WORLD_SIZE"]

"""Host checks of the MLM pre-training references (tests/mlm_reference.py); no GPU.

  1. the masking reference: Philox known answer, the selected share and the 80 / 10 / 10 split, specials and padding
     never selected, a split batch gives the same tokens;
  2. the float64 cross-entropy reference on the oracle's fp32 logits equals transformers' ModernBertForMaskedLM loss;
  3. acceptance intervals of lse and the row loss, and four planted faults that fall outside them;
  4. the floor of the gradient comparison (two fp32 evaluations of the contract, contraction orders permuted)."""
import math

import numpy as np
import pytest
import torch

from oracle import splade_oracle as O
from tests import mlm_reference as R


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32-10."""
    z = np.zeros(1, np.uint64)
    assert [int(x[0]) for x in R.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = np.full(1, 0xFFFFFFFF, np.uint64)
    assert [int(x[0]) for x in R.philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6,
                                                                                        0x6d5451fd]
    c = [np.full(1, v, np.uint64) for v in (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)]
    assert [int(x[0]) for x in R.philox4x32_10(*c, 0xa4093822, 0x299f31d0)] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def _mask_batch(B=440, S=512, V=50000, seed=3):
    rng = np.random.default_rng(seed)
    ids = rng.integers(5, V, size=(B, S), dtype=np.int64)
    lens = rng.integers(S - 40, S + 1, size=B)
    att = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    ids[:, 0] = 0                                                   # [CLS]
    ids[np.arange(B), lens - 1] = 1                                 # [SEP]
    ids[att == 0] = 2                                               # [PAD]
    ids[rng.random((B, S)) < 0.01] = 3                              # a special in the running text
    return ids, att, np.arange(B, dtype=np.int64) + 7


KW = dict(special_ids=(0, 1, 2, 3, 4), mask_id=4, vocab_size=50000, seed=0x1234567887654321, epoch=2)


def test_masking_reference_distribution_and_invariances():
    ids, att, sample = _mask_batch()
    out, labels, sel = R.mask_tokens_ref(ids, att, sample, **KW)
    maskable = (att != 0) & ~np.isin(ids, KW["special_ids"])
    n = int(maskable.sum())
    assert n >= 200_000
    assert not sel[~maskable].any()                                 # specials and padding are never selected
    share = sel.sum() / n
    assert abs(share - 0.15) <= 0.005, share                        # 6 sigma = 6 sqrt(.15 .85 / 2e5) = 0.0048
    k = int(sel.sum())
    masked = (out == KW["mask_id"]) & sel
    kept = (out == ids) & sel
    rand = sel & ~masked & ~kept
    for got, want in ((masked.sum() / k, 0.8), (rand.sum() / k, 0.1), (kept.sum() / k, 0.1)):
        assert abs(got - want) <= 0.01, (got, want)                 # 6 sigma at k = 30,000: 0.014 / 0.010
    assert (labels[sel] == ids[sel]).all() and (labels[~sel] == -100).all() and (out[~sel] == ids[~sel]).all()
    # a split batch, rows in another order: every token keeps its fate
    perm = np.random.default_rng(0).permutation(len(ids))
    for part in (perm[:100], perm[100:]):
        o2, l2, _ = R.mask_tokens_ref(ids[part], att[part], sample[part], **KW)
        assert (o2 == out[part]).all() and (l2 == labels[part]).all()
    o3, _, _ = R.mask_tokens_ref(ids, att, sample, **{**KW, "epoch": 3})
    assert (o3 != out).any()                                        # another epoch draws again


def test_reference_loss_equals_transformers():
    transformers = pytest.importorskip("transformers")
    try:
        from transformers import ModernBertForMaskedLM
    except Exception:                                               # pragma: no cover
        pytest.skip("transformers without ModernBERT")
    geom = dict(vocab_size=300, hidden_size=256, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                local_attention=8, pad_token_id=299)
    cfg = O.EncoderConfig(**geom)
    params = O.perturb_params(O.init_params(cfg, seed=3), seed=4, scale=2.0, bias_mean=-0.1)
    from src.model.splade_modern import ModernBertMaskedLMWeights, _geometry_from_config
    cfgd = {k: v for k, v in ModernBertMaskedLMWeights(_geometry_from_config(geom)).hf_config_dict().items()
            if k not in ("architectures", "model_type", "dtype")}
    hf = ModernBertForMaskedLM(transformers.ModernBertConfig(**cfgd))
    sd = {k[len("model."):]: v.clone() for k, v in params.items()}
    sd["decoder.weight"] = sd["model.embeddings.tok_embeddings.weight"]
    hf.load_state_dict(sd, strict=True)
    hf.eval()
    ids, mask = O.synth_ids(3, 24, cfg, torch.Generator().manual_seed(2), ragged=True)
    masked, labels, sel = R.mask_tokens_ref(ids.numpy(), mask.numpy(), np.arange(3), special_ids=(299,), mask_id=298,
                                            vocab_size=300, seed=5, p=0.3)
    assert sel.sum() >= 8
    masked_t, labels_t = torch.from_numpy(masked), torch.from_numpy(labels)
    with torch.no_grad():
        want = float(hf(input_ids=masked_t, attention_mask=mask, labels=labels_t).loss)
        logits = O.encoder_logits(params, cfg, masked_t, mask, "fp32")
    got = R.ce_from_logits64(logits[torch.from_numpy(sel)].numpy(), labels[sel])
    assert abs(got - want) <= 1e-5, (got, want)


@pytest.mark.parametrize("M,V,H", [(37, 1000, 256), (20, 3000, 256)])
def test_acceptance_intervals_and_planted_faults(M, V, H):
    for variant in ("rand", "m30"):
        case = R.ce_case(M, V, H, variant)
        labels = case["labels"]
        f = R.ce_forward64(case["h"], case["E"], case["bias"], labels)
        acc = R.acceptance(f, labels)
        scale = np.maximum(np.abs(f["lse"]), np.abs(f["z"][np.arange(M), labels]))
        # the reference and a plain fp32 evaluation lie inside
        assert R.inside(f["lse"], acc["lse_lo"], acc["lse_hi"], scale).all()
        assert R.inside(f["row_loss"], acc["loss_lo"], acc["loss_hi"], scale).all()
        c = R.contract_fp32(case, 99)
        assert R.inside(c["lse"], acc["lse_lo"], acc["lse_hi"], scale).all()
        if variant == "m30":
            assert abs(f["row_loss"][4] - math.log(V)) < 1e-9       # zero row, constant bias
            assert np.abs(f["z"][5]).max() > 150 and np.isfinite(f["row_loss"]).all()
        z = f["z"]
        rows = np.arange(M)
        Vp = (V + 127) // 128 * 128

        def outside(lse, loss):
            bad_lse = ~R.inside(lse, acc["lse_lo"], acc["lse_hi"], scale)
            bad_loss = ~R.inside(loss, acc["loss_lo"], acc["loss_hi"], scale)
            return bad_lse, bad_loss
        # (1) pad columns counted: z = 0 there (zero operands, no bias)
        zp = np.concatenate([z, np.zeros((M, Vp - V))], axis=1)
        lse = R.logsumexp64(zp)
        bad_lse, bad_loss = outside(lse, lse - z[rows, labels])
        assert bad_lse.any() and bad_loss.any(), variant
        if variant == "m30":
            live = np.abs(z).max(axis=1) < 10                       # (not the row scaled to |z| ~ 200)
            assert ((lse - f["lse"])[live] > 20).all() and bad_lse[live].all()
        # (2) a 128-column tile dropped
        zd = np.delete(z, np.s_[128:256], axis=1)
        lse = R.logsumexp64(zd)
        bad_lse, _ = outside(lse, lse - z[rows, labels])
        assert bad_lse.mean() > 0.9, variant
        # (3) the target taken from column y + 1
        y1 = np.minimum(labels + 1, V - 1)
        _, bad_loss = outside(f["lse"], f["lse"] - z[rows, y1])
        if variant == "rand":
            assert bad_loss.mean() > 0.8
        # (4) bias not added (a constant bias shifts every logit alike: lse moves, the loss does not)
        zb = R.bf16_round(f["s"] - R.bf16_round(case["bias"].astype(np.float64))[None, :])
        lse = R.logsumexp64(zb)
        bad_lse, bad_loss = outside(lse, lse - zb[rows, labels])
        assert bad_lse.mean() > 0.9, variant
        if variant == "rand":
            assert bad_loss.mean() > 0.8


def test_gradient_floors():
    fl = R.gradient_floors()
    # a bf16 output carries at most half an ulp, 2^-9 relative, per evaluation: two of them differ by at most 2^-8 of the
    # element, plus what flipped logits and flipped g move; fp32 accumulations (dE, dbias) see only the latter
    assert 0 < fl["dh"] < 2.0 ** -6 and 0 < fl["dE"] < 2.0 ** -6 and 0 < fl["dbias"] < 2.0 ** -6, fl
    # and the float64 reference lies within the same floor of an fp32 evaluation
    M, V, H = R.SHAPES[2]
    case = R.ce_case(M, V, H, "rand")
    f = R.ce_forward64(case["h"], case["E"], case["bias"], case["labels"])
    want = R.ce_backward64(case["h"], case["E"], f["z"], f["lse"], case["labels"])
    got = R.contract_fp32(case, 7)
    for k in ("dh", "dE", "dbias"):
        assert R.normalised_diff(got[k], want[k]) <= 4 * fl[k], (k, R.normalised_diff(got[k], want[k]), fl[k])


def test_mlm_state_dict_is_the_wrapped_models():
    from src.model.mlm_modern import MLMModernBERT
    from src.model.splade_modern import SPLADEModernBERT
    import logging
    logging.getLogger("src.model.splade_modern").setLevel(logging.ERROR)
    s = SPLADEModernBERT()
    m = MLMModernBERT(s)
    assert list(m.state_dict().keys()) == list(s.state_dict().keys()) and len(m.state_dict()) == 138
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in s.named_parameters()]
    assert all(a is b for a, b in zip(m.parameters(), s.parameters()))

"""Masked-language-model pre-training head over a ``SPLADEModernBERT`` -- MI355X-native.

The reference names this stage (``configs/pretrain_mlm.yaml`` -> ``src.train.cli.pretrain_mlm``) without supplying it;
what it would run is ``transformers.ModernBertForMaskedLM(labels=...)`` under bf16 autocast.  Here the encoder up to the
head's LayerNorm is the native forward of the SPLADE model stopped before its decoder
(``snx_model_forward_hidden``), and the loss is the cross-entropy of the MASKED rows only against the tied decoder
(``snx.mlm``, ModernBERT's ``sparse_prediction``): no [T, V] tensor exists.

``MLMModernBERT`` owns no parameter of its own: it holds the wrapped model's ``model`` module under the same name, so
its ``state_dict()`` has the wrapped model's keys and a checkpoint it writes loads into ``SPLADEModernBERT`` unchanged.

Deviations from HF: a batch without a masked token gives loss 0 and zero gradients (HF: NaN); the number of
masked rows is read back to the host once per call (one synchronisation: the gathered buffers are sized by it)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from snx import mlm
from src.model.splade_modern import SPLADEModernBERT


class _MlmLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rt, input_ids, attention_mask, rows, targets, *params):
        hd, saved, aux = rt.forward_hidden_impl(input_ids, attention_mask, save=True)
        E, ET = rt.mlm_embeddings()
        h = hd.index_select(0, rows)                       # the masked rows, ascending native row order
        fwd = mlm.ce_forward(h, targets, E, params[-1])    # (decoder.bias closes the canonical order)
        ctx.rt, ctx.saved, ctx.aux, ctx.fwd, ctx.ET = rt, saved, aux, fwd, ET
        ctx.h, ctx.rows, ctx.targets = h, rows, targets
        return fwd.loss

    @staticmethod
    def backward(ctx, g):
        rt = ctx.rt
        head = (None,) * 5
        fwd, ctx.fwd = ctx.fwd, None
        if fwd is None:
            raise RuntimeError("MLMModernBERT: backward twice (the saved logits are consumed by the first)")
        grads = rt.grad_buffers()
        if ctx.rows.numel() > 0:
            T, H = ctx.aux[6], ctx.h.shape[1]
            # the head's gradients of the tied embedding matrix and of decoder.bias go straight into their buffers; the
            # encoder's backward then adds the embedding lookup's share to the same matrix
            dh = mlm.ce_backward(fwd, ctx.h, ctx.targets, ctx.ET, g, grads[0], grads[-1])
            g_hd = torch.zeros((T, H), dtype=torch.bfloat16, device=dh.device)
            g_hd.index_copy_(0, ctx.rows, dh)
            rt.backward_hidden_impl(ctx.saved, ctx.aux, g_hd, grads)
        ctx.saved = ctx.h = None
        if rt.direct_grads:
            return head + tuple(None for _ in rt.params)
        return head + tuple(grads)


class MLMModernBERT(nn.Module):
    """``forward(input_ids, attention_mask, labels) -> loss``: the mean cross-entropy over the positions whose label is
    not -100 (a 0-d fp32 tensor, autograd-connected to the wrapped model's parameters).  ``last_masked_count`` holds the
    number of those positions of the latest call.  bf16 path only: call it inside
    ``torch.autocast("cuda", torch.bfloat16)``; outside it raises NotImplementedError."""

    def __init__(self, splade: SPLADEModernBERT):
        super().__init__()
        self.model = splade.model                          # the parameters, under the wrapped model's names
        object.__setattr__(self, "_splade", splade)        # (not a submodule: its parameters are registered once)
        self.last_masked_count = 0

    @property
    def splade(self) -> SPLADEModernBERT:
        return self._splade

    @property
    def runtime(self):
        return self._splade.runtime

    @property
    def vocab_size(self) -> int:
        return self._splade.vocab_size

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        rt = self.runtime
        if labels.shape != input_ids.shape:
            raise ValueError("labels must have the shape of input_ids")
        lab = labels.to(torch.int64).reshape(-1)
        rows = torch.nonzero(lab >= 0).view(-1)             # one host synchronisation: M sizes the gathered buffers
        targets = lab.index_select(0, rows)
        self.last_masked_count = int(rows.numel())
        if torch.is_grad_enabled() and any(p.requires_grad for p in rt.params):
            return _MlmLossFn.apply(rt, input_ids, attention_mask, rows, targets, *rt.params)
        hd, _, _ = rt.forward_hidden_impl(input_ids, attention_mask, save=False)
        E, _ = rt.mlm_embeddings()
        return mlm.ce_forward(hd.index_select(0, rows), targets, E, rt.params[-1]).loss

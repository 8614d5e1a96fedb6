"""Masked-language-model pre-training ops (csrc/mlm.hip): token masking on the device and the cross-entropy of the
masked rows against the tied decoder, with its autograd Function.

Two deviations from HuggingFace, both documented in DESIGN.md:
  * the masking draws are not ``torch.bernoulli``'s stream but a pure function of (seed, epoch, sample index, position)
    -- the same distribution, other draws --, so a token's fate does not depend on what else is in the batch;
  * an empty batch (no masked token) gives loss 0 and zero gradients where HF gives NaN."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import call, fn
from .ops import BF16, _chk, _p, _stream

TILE = 128
MAX_SPECIAL = 16


def vocab_padded(V: int) -> int:
    return (int(V) + TILE - 1) // TILE * TILE


def mask_tokens(input_ids: torch.Tensor, attention_mask: torch.Tensor, sample_index: torch.Tensor, *,
                special_ids: Sequence[int], mask_id: int, vocab_size: int, seed: int, epoch: int = 0, p: float = 0.15,
                p_mask: float = 0.8, p_random: float = 0.1) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (masked_ids [B, S] int64, labels [B, S] int64, -100 where no loss is taken): the contract of
    ``DataCollatorForLanguageModeling.torch_mask_tokens``.  Draws: Philox4x32-10, key = seed, counter =
    (lo32(t), hi32(t), epoch, 0), t = sample_index * 65536 + position (include/snx.h)."""
    if input_ids.dim() != 2 or attention_mask.shape != input_ids.shape:
        raise ValueError("input_ids and attention_mask must both be [batch, seq_len]")
    B, S = int(input_ids.shape[0]), int(input_ids.shape[1])
    if S > 65535:
        raise ValueError("mask_tokens: seq_len > 65535 (the position takes the low 16 bits of the counter)")
    if S < 1:
        raise ValueError("mask_tokens: empty sequences")
    special = [int(s) for s in special_ids]
    if len(special) > MAX_SPECIAL:
        raise ValueError(f"mask_tokens: at most {MAX_SPECIAL} special ids")
    if not 0 <= int(mask_id) < int(vocab_size):
        raise ValueError("mask_tokens: mask_id outside the vocabulary")
    if not (0.0 <= p <= 1.0 and 0.0 <= p_mask and 0.0 <= p_random and p_mask + p_random <= 1.0):
        raise ValueError("mask_tokens: probabilities out of range")
    if epoch < 0 or epoch >= 2 ** 31:
        raise ValueError("mask_tokens: epoch out of range")
    ids = _chk(input_ids.to(torch.int64).contiguous(), torch.int64, "input_ids")
    mask = _chk(attention_mask.to(torch.int64).contiguous(), torch.int64, "attention_mask", (B, S))
    sample = _chk(sample_index.to(torch.int64).contiguous(), torch.int64, "sample_index", (B,))
    if ids.device != mask.device or ids.device != sample.device:
        raise ValueError("mask_tokens: inputs on different devices")
    out, labels = torch.empty_like(ids), torch.empty_like(ids)
    if B == 0:
        return out, labels
    sp = (C.c_int64 * max(len(special), 1))(*special)
    seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF
    with torch.cuda.device(ids.device):
        call("snx_mlm_mask_tokens", _p(ids), _p(mask), _p(sample), _p(out), _p(labels), B, S, sp, len(special), int(mask_id),
             int(vocab_size), seed64 - (1 << 64) if seed64 >= (1 << 63) else seed64, int(epoch), float(p), float(p_mask),
             float(p_random), _stream())
    return out, labels


def transpose_embeddings(E: torch.Tensor) -> torch.Tensor:
    """E [V, H] bf16 -> E^T [H, Vp] bf16 with zero pad columns (the operand of dh = g E)."""
    _chk(E, BF16, "E")
    V, H = E.shape
    if H % 64:
        raise ValueError("transpose_embeddings: hidden % 64 != 0")
    ET = torch.empty((H, vocab_padded(V)), dtype=BF16, device=E.device)
    with torch.cuda.device(E.device):
        call("snx_mlm_transpose_embeddings", _p(E), _p(ET), V, H, _stream())
    return ET


class CeForward(NamedTuple):
    loss: torch.Tensor        # [] fp32: mean of row_loss
    row_loss: torch.Tensor    # [M] fp32
    lse: torch.Tensor         # [M] fp32
    z: Optional[torch.Tensor]  # [M, Vp] bf16 logits (pad columns zero); ce_backward turns it into g in place


def _check_ce(h, labels, E, bias):
    _chk(h, BF16, "h"); _chk(E, BF16, "E"); _chk(bias, torch.float32, "bias"); _chk(labels, torch.int64, "labels")
    if h.dim() != 2 or E.dim() != 2 or h.shape[1] != E.shape[1]:
        raise ValueError("cross-entropy: h [M, H] and E [V, H] must share H")
    M, H = h.shape
    V = E.shape[0]
    if bias.shape != (V,) or labels.shape != (M,):
        raise ValueError("cross-entropy: bias must be [V] and labels [M]")
    if H % 128 or H > 1024:
        raise ValueError("cross-entropy: hidden must be a multiple of 128, at most 1024")
    if not (h.device == E.device == bias.device == labels.device):
        raise ValueError("cross-entropy: operands on different devices")
    return int(M), int(V), int(H)


def ce_forward(h: torch.Tensor, labels: torch.Tensor, E: torch.Tensor, bias: torch.Tensor) -> CeForward:
    """Cross-entropy of the rows h [M, H] bf16 against the tied decoder E [V, H] bf16, bias [V] fp32 (include/snx.h
    snx_mlm_ce_fwd).  labels [M] int64 must lie in [0, V); one outside makes its row and the loss NaN.
    M == 0: nothing is launched, loss 0."""
    M, V, H = _check_ce(h, labels, E, bias)
    dev = h.device
    if M == 0:
        e = torch.zeros((0,), dtype=torch.float32, device=dev)
        return CeForward(torch.zeros((), dtype=torch.float32, device=dev), e, e.clone(), None)
    Vp = vocab_padded(V)
    z = torch.empty((M, Vp), dtype=BF16, device=dev)
    part = torch.empty(((2 * (Vp // TILE) + 1) * M,), dtype=torch.float32, device=dev)
    lse = torch.empty((M,), dtype=torch.float32, device=dev)
    row_loss = torch.empty((M,), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("snx_mlm_ce_fwd", _p(h), _p(E), _p(bias), _p(labels), _p(z), _p(part), _p(lse), _p(row_loss), _p(loss), M, V, H,
             _stream())
    return CeForward(loss, row_loss, lse, z)


def ce_backward(fwd: CeForward, h: torch.Tensor, labels: torch.Tensor, ET: torch.Tensor, upstream: torch.Tensor,
                dE: torch.Tensor, dbias: torch.Tensor) -> torch.Tensor:
    """-> dh [M, H] bf16; dE [V, H] and dbias [V] (fp32) are accumulated into.  ``fwd.z`` is consumed (it becomes g).
    ``upstream``: dL/d loss, one fp32 element on the device."""
    _chk(h, BF16, "h"); _chk(ET, BF16, "ET"); _chk(labels, torch.int64, "labels")
    M, H = int(h.shape[0]), int(h.shape[1])
    V = int(dbias.shape[0])
    _chk(dE, torch.float32, "dE", (V, H)); _chk(dbias, torch.float32, "dbias", (V,))
    if tuple(ET.shape) != (H, vocab_padded(V)):
        raise ValueError("ce_backward: ET must be [H, Vp] (transpose_embeddings)")
    dh = torch.empty((M, H), dtype=BF16, device=h.device)
    if M == 0:
        return dh
    up = _chk(upstream.to(torch.float32).reshape(1).contiguous(), torch.float32, "upstream", (1,))
    _chk(fwd.z, BF16, "z", (M, vocab_padded(V))); _chk(fwd.lse, torch.float32, "lse", (M,))
    with torch.cuda.device(h.device):
        nbytes = fn("snx_mlm_ce_bwd_workspace_bytes")(M, V, H)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=h.device)
        call("snx_mlm_ce_bwd", _p(fwd.z), _p(fwd.lse), _p(labels), _p(up), _p(h), _p(ET), _p(dh), _p(dE), _p(dbias), _p(ws),
             nbytes, M, V, H, _stream())
    return dh


class _CrossEntropyRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, labels, E, ET, bias, weight):
        fwd = ce_forward(h, labels, E, bias)
        ctx.fwd, ctx.ET, ctx.has_weight = fwd, ET, weight is not None
        ctx.save_for_backward(h, labels)
        ctx.shape = (E.shape[0], E.shape[1])
        return fwd.loss.clone()

    @staticmethod
    def backward(ctx, g):
        h, labels = ctx.saved_tensors
        V, H = ctx.shape
        dE = torch.zeros((V, H), dtype=torch.float32, device=h.device)
        dbias = torch.zeros((V,), dtype=torch.float32, device=h.device)
        fwd, ctx.fwd = ctx.fwd, None
        if fwd is None:
            raise RuntimeError("cross_entropy_rows: backward twice (the logits are consumed by the first)")
        dh = ce_backward(fwd, h, labels, ctx.ET, g, dE, dbias)
        if h.shape[0] == 0:
            dh = torch.zeros_like(h)
        return dh, None, None, None, dbias, (dE if ctx.has_weight else None)


def cross_entropy_rows(h: torch.Tensor, labels: torch.Tensor, E: torch.Tensor, bias: torch.Tensor,
                       weight: Optional[torch.Tensor] = None, ET: Optional[torch.Tensor] = None) -> torch.Tensor:
    """loss [] fp32 = mean over the rows of logsumexp_v z[m, v] - z[m, labels[m]], z = bf16(h E^T + bf16(bias)): what
    ``ModernBertForMaskedLM`` computes under bf16 autocast for the rows it keeps (sparse_prediction).  Differentiable with
    respect to h (bf16), bias and -- when given -- ``weight``, the fp32 master copy [V, H] that E was cast from (the tied
    embedding matrix): its gradient is g^T h in fp32.  ``ET``: transpose_embeddings(E), built here when missing."""
    if ET is None:
        ET = transpose_embeddings(E)
    return _CrossEntropyRowsFn.apply(h, labels, E, ET, bias, weight)

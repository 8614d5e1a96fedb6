"""Host restatements of the MLM pre-training ops (csrc/mlm.hip), used by tests/test_mlm_host.py and tests/test_gpu_mlm.py.

  * Philox4x32-10 and the token masking contract, in numpy;
  * the cross-entropy of gathered rows against the tied decoder in float64, with the cast points of the contract
    (include/snx.h snx_mlm_ce_fwd / snx_mlm_ce_bwd);
  * acceptance intervals: which bf16 logits an fp32 accumulation may produce, and what lse / row loss follow;
  * the contract in torch fp32 with permuted contraction orders -- a second correct implementation, the floor of the
    gradient comparison."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Counter words (uint32 arrays of one shape), key words -> the four output words r0..r3."""
    c = [np.asarray(x, dtype=np.uint64) & U32 for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & U32]
        k0, k1 = (k0 + np.uint64(W0)) & U32, (k1 + np.uint64(W1)) & U32
    return tuple(x.astype(np.uint32) for x in c)


def mask_tokens_ref(input_ids, attention_mask, sample_index, *, special_ids, mask_id: int, vocab_size: int, seed: int,
                    epoch: int = 0, p: float = 0.15, p_mask: float = 0.8, p_random: float = 0.1):
    """-> (masked_ids, labels, selected) int64 / int64 / bool [B, S]."""
    ids = np.asarray(input_ids, dtype=np.int64)
    att = np.asarray(attention_mask) != 0
    B, S = ids.shape
    assert S <= 65535
    t = np.asarray(sample_index, dtype=np.uint64)[:, None] * np.uint64(65536) + np.arange(S, dtype=np.uint64)[None, :]
    seed &= 0xFFFFFFFFFFFFFFFF
    r0, r1, r2, _ = philox4x32_10(t & U32, t >> np.uint64(32), np.full(t.shape, epoch, np.uint64), np.zeros(t.shape, np.uint64),
                                  seed & 0xFFFFFFFF, seed >> 32)
    two32 = 1.0 / 4294967296.0
    can = att & ~np.isin(ids, np.asarray(list(special_ids), dtype=np.int64))
    sel = can & (r0.astype(np.float64) * two32 < p)
    u = r1.astype(np.float64) * two32
    rand_id = ((r2.astype(np.uint64) * np.uint64(vocab_size)) >> np.uint64(32)).astype(np.int64)
    out = ids.copy()
    to_mask = sel & (u < p_mask)
    to_rand = sel & ~to_mask & (u < p_mask + p_random)
    out[to_mask] = mask_id
    out[to_rand] = rand_id[to_rand]
    labels = np.where(sel, ids, -100)
    return out, labels, sel


# ---- bf16 in float64 ------------------------------------------------------------------------------------------------
def bf16_round(x: np.ndarray) -> np.ndarray:
    """float64 -> the nearest value with 8 significant bits (ties to even), as float64.  One rounding; the test data stays
    far from bf16's subnormals and its overflow."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def bf16_exact(x: np.ndarray) -> np.ndarray:
    """float32 data rounded to bf16 (torch), returned as float32."""
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


# ---- test data -------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1000, 256), (127, 1000, 256), (129, 3000, 256), (300, 3000, 768), (64, 50000, 768)]


def ce_case(M: int, V: int, H: int, variant: str = "rand", seed: int = 0) -> Dict[str, np.ndarray]:
    """h [M, H] and E [V, H] (bf16 values held in float32), bias [V] fp32, labels [M] int64.
    Labels: row 0 -> 0, row 1 -> V - 1, rows 2 and 3 -> one column inside the tail tile (a repeated label), the rest random
    with repeats.  variant "m30": bias -30 on every column (a counted pad column, z = 0, then moves lse by more than 20),
    row 4 of h zero (its loss is ln V), row 5 scaled so that its largest |z| is about 200."""
    rng = np.random.default_rng(1000 * seed + M + V + H)
    h = bf16_exact(rng.standard_normal((M, H)))
    E = bf16_exact(rng.standard_normal((V, H)) * 0.05)
    labels = rng.integers(0, V, size=M, dtype=np.int64)
    tail = (V - 1) // 128 * 128 + min(5, (V - 1) % 128)
    for row, lab in ((0, 0), (1, V - 1), (2, tail), (3, tail)):
        if row < M:
            labels[row] = lab
    if M == 1:
        labels[0] = tail
    if variant == "m30":
        bias = np.full((V,), -30.0, dtype=np.float32)
        if M > 4:
            h[4] = 0.0
        if M > 5:
            z = h[5].astype(np.float64) @ E.astype(np.float64).T
            h[5] = bf16_exact(h[5] * (200.0 / np.abs(z).max()))
    else:
        bias = (rng.standard_normal(V) * 0.5).astype(np.float32)
    return {"h": h, "E": E, "bias": bias, "labels": labels}


# ---- float64 reference ----------------------------------------------------------------------------------------------
def logsumexp64(z: np.ndarray) -> np.ndarray:
    m = z.max(axis=1)
    return m + np.log(np.exp(z - m[:, None]).sum(axis=1))


def ce_from_logits64(logits, labels) -> float:
    """Mean cross-entropy of float logits [M, V] at labels [M] in float64 (no rounding of its own)."""
    z = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels)
    return float((logsumexp64(z) - z[np.arange(len(labels)), labels]).mean())


def ce_forward64(h, E, bias, labels, *, cols: Optional[slice] = None):
    """The forward contract in float64: exact sums, ONE rounding of the logit to bf16.  -> z [M, V], lse, row_loss, loss,
    and (s, bound): the unrounded sums and the fp32 accumulation bound (H + 1) 2^-24 (sum |h||E| + |b|) per logit."""
    h64, E64 = np.asarray(h, np.float64), np.asarray(E, np.float64)
    b = bf16_round(np.asarray(bias, np.float64))
    s = h64 @ E64.T + b[None, :]
    bound = (h64.shape[1] + 1) * 2.0 ** -24 * (np.abs(h64) @ np.abs(E64).T + np.abs(b)[None, :])
    z = bf16_round(s)
    lse = logsumexp64(z)
    rows = np.arange(len(labels))
    row_loss = lse - z[rows, labels]
    return {"z": z, "lse": lse, "row_loss": row_loss, "loss": float(row_loss.mean()) if len(labels) else 0.0, "s": s,
            "bound": bound}


def acceptance(fwd: Dict[str, np.ndarray], labels) -> Dict[str, np.ndarray]:
    """Intervals of lse and of the row loss over every choice of z[m, v] among the bf16 values reachable from the exact sum
    within the accumulation bound.  Rounding is monotone, so the reachable values lie between bf16(s - bound) and
    bf16(s + bound); lse rises with every z; the row loss lse - z_y rises with z_v (v != y) and falls with z_y."""
    zlo, zhi = bf16_round(fwd["s"] - fwd["bound"]), bf16_round(fwd["s"] + fwd["bound"])
    rows = np.arange(len(labels))
    a = zlo.copy(); a[rows, labels] = zhi[rows, labels]      # smallest loss: others low, target high
    b = zhi.copy(); b[rows, labels] = zlo[rows, labels]      # largest loss
    return {"lse_lo": logsumexp64(zlo), "lse_hi": logsumexp64(zhi), "loss_lo": logsumexp64(a) - zhi[rows, labels],
            "loss_hi": logsumexp64(b) - zlo[rows, labels], "z_lo": zlo, "z_hi": zhi}


EXP_LOG_REL = 2e-6     # the fp32 exp / log of the device: relative to the magnitude of lse (the row loss is a difference of
                       # lse and a logit: its rounding is relative to those two, not to the possibly tiny difference)


def inside(x, lo, hi, scale) -> np.ndarray:
    x = np.asarray(x, np.float64)
    tol = EXP_LOG_REL * scale
    return (x >= lo - tol) & (x <= hi + tol)


def ce_backward64(h, E, z, lse, labels, upstream: float = 1.0):
    """The backward contract in float64 from given logits: g = bf16((exp(z - lse) - [v == y]) upstream / M),
    dh = bf16(g E), dE = g^T h, dbias = sum_m g."""
    h64, E64 = np.asarray(h, np.float64), np.asarray(E, np.float64)
    M = len(labels)
    p = np.exp(z - lse[:, None])
    p[np.arange(M), labels] -= 1.0
    g = bf16_round(p * (upstream / M))
    return {"dh": bf16_round(g @ E64), "dE": g.T @ h64, "dbias": g.sum(axis=0)}


# ---- the contract in fp32, contraction orders permuted ----------------------------------------------------------------
def contract_fp32(case: Dict[str, np.ndarray], perm_seed: Optional[int], upstream: float = 1.0) -> Dict[str, np.ndarray]:
    """Forward and backward contract in torch fp32 on the CPU (bf16 cast points as stated); with ``perm_seed`` every
    contraction (over H in the logits, over V in dh, over M in dE and dbias) runs in a permuted order -- the same products,
    another fp32 summation order (the idea of oracle.splade_oracle.CONTRACTION_PERM_SEED)."""
    h, E = torch.from_numpy(case["h"]), torch.from_numpy(case["E"])
    bias, labels = torch.from_numpy(case["bias"]), torch.from_numpy(case["labels"])
    M, H = h.shape
    V = E.shape[0]
    gen = torch.Generator().manual_seed(perm_seed if perm_seed is not None else 0)
    pk = torch.randperm(H, generator=gen) if perm_seed is not None else torch.arange(H)
    pv = torch.randperm(V, generator=gen) if perm_seed is not None else torch.arange(V)
    pm = torch.randperm(M, generator=gen) if perm_seed is not None else torch.arange(M)
    z = (h[:, pk] @ E[:, pk].t() + bias.to(torch.bfloat16).float()).to(torch.bfloat16).float()
    lse = torch.logsumexp(z[:, pv], dim=1)
    p = torch.exp(z - lse[:, None])
    p[torch.arange(M), labels] -= 1.0
    g = (p * (torch.tensor(upstream, dtype=torch.float32) / M)).to(torch.bfloat16).float()
    dh = (g[:, pv] @ E[pv]).to(torch.bfloat16).float()
    dE = g[pm].t() @ h[pm]
    dbias = g[pm].sum(dim=0)
    return {"dh": dh.numpy(), "dE": dE.numpy(), "dbias": dbias.numpy(), "lse": lse.numpy(), "z": z.numpy()}


def normalised_diff(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


FLOOR_SHAPES = SHAPES[:4]


@functools.lru_cache(maxsize=None)
def gradient_floors() -> Dict[str, float]:
    """The floor of the gradient comparison, per tensor: the largest normalised difference between two fp32 evaluations
    of the contract with different contraction orders.  What it measures is one-ulp bf16 flips (of a logit, of an element
    of g, of an element of dh) where two summation orders straddle a rounding boundary; whether a given small tensor
    contains such a flip is a coin toss (a [1, 256] dh holds 0.1 of them on average), so the floor of a tensor is taken
    over the test shapes together (all but the 50,000-column one, which costs the host too much): the largest value."""
    out = {"dh": 0.0, "dE": 0.0, "dbias": 0.0}
    for (M, V, H) in FLOOR_SHAPES:
        case = ce_case(M, V, H, "rand")
        a, b = contract_fp32(case, None), contract_fp32(case, 12345)
        for k in out:
            out[k] = max(out[k], normalised_diff(a[k], b[k]))
    return out

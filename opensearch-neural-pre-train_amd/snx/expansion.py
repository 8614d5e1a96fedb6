"""Term-expansion evaluation on the GPU (csrc/expansion.hip, include/snx.h "term-expansion evaluation"): where the judged
tokens of a source term fall in the model's own ranking of the vocabulary, and the graded metrics that follow from those
positions.  The kernels count, they do not sort; the arithmetic the reference does around them (token resolution,
denominators, IDCG, aggregation) is the host's (src/evaluation/ranking_metrics.py)."""
import ctypes as C
import math
from typing import Sequence, Tuple

import numpy as np
import torch

from ._lib import call, fn
from .ops import _p, _stream

CUTOFFS_MAX = 8
GRADE_MAX = 3

_gain_cache = {}


def gain_table(G: int) -> np.ndarray:
    """gain [3, G] float64 on the host: gain[g - 1, p - 1] = (2**g - 1) / math.log2(p + 1), the reference's DCG term of grade
    g at position p with the reference's own expression (include/snx.h: the kernel computes no logarithm)."""
    G = int(G)
    if G < 1:
        raise ValueError("gain_table: G must be >= 1")
    out = np.empty((GRADE_MAX, G), dtype=np.float64)
    for g in range(1, GRADE_MAX + 1):
        for p in range(1, G + 1):
            out[g - 1, p - 1] = (2 ** g - 1) / math.log2(p + 1)
    return out


def _gain_on(G: int, dev: torch.device) -> torch.Tensor:
    key = (G, dev.type, dev.index)
    if key not in _gain_cache:
        _gain_cache[key] = torch.from_numpy(gain_table(G)).to(dev)
    return _gain_cache[key]


def _host_ints(x, what: str) -> np.ndarray:
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"{what}: a 1-d array of ints")
    return a.astype(np.int64)


def judgment_csr(judgments, B: int):
    """Judgments -> host arrays (j_ptr int64 [B+1], j_tok int32, j_grade uint8, j_rel uint8), checked.  ``judgments``: a list
    of ``B`` rows of (token id, grade, rel) triples, or the tuple (j_ptr, j_tok, j_grade, j_rel) of int arrays / tensors.
    j_ptr starts at 0, does not decrease and ends at len(j_tok); token ids fit in int32 and are distinct within a row (ids
    outside the vocabulary are allowed: they are unranked); grades lie in 0 .. 3."""
    B = int(B)
    if isinstance(judgments, tuple) and len(judgments) == 4:
        ptr, tok, grade, rel = (_host_ints(x, f"judgments[{i}]") for i, x in enumerate(judgments))
    else:
        rows = [list(r) for r in judgments]
        if len(rows) != B:
            raise ValueError(f"judgments: {len(rows)} rows for {B} rows of rep")
        flat = [t for r in rows for t in r]
        if any(len(t) != 3 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in t[:2]) for t in flat):
            raise ValueError("judgments: rows of (token id, grade, rel) with int ids and grades")
        ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        tok = np.asarray([t[0] for t in flat], dtype=np.int64)
        grade = np.asarray([t[1] for t in flat], dtype=np.int64)
        rel = np.asarray([1 if t[2] else 0 for t in flat], dtype=np.int64)
    nj = tok.shape[0]
    if ptr.shape[0] != B + 1 or grade.shape[0] != nj or rel.shape[0] != nj:
        raise ValueError(f"judgments: j_ptr [{B + 1}] and j_tok, j_grade, j_rel of one length")
    if ptr[0] != 0 or ptr[-1] != nj or (ptr[1:] < ptr[:-1]).any():
        raise ValueError("judgments: j_ptr must start at 0, not decrease and end at len(j_tok)")
    if nj and (tok.min() < -2 ** 31 or tok.max() >= 2 ** 31):
        raise ValueError("judgments: token ids must fit in int32")
    if nj and (grade.min() < 0 or grade.max() > GRADE_MAX):
        raise ValueError(f"judgments: grades must lie in 0 .. {GRADE_MAX}")
    row = np.repeat(np.arange(B, dtype=np.int64), np.diff(ptr))
    if nj and np.unique(row * 2 ** 32 + (tok + 2 ** 31)).shape[0] != nj:
        raise ValueError("judgments: a token id is repeated within a row")
    return ptr, tok.astype(np.int32), grade.astype(np.uint8), (rel != 0).astype(np.uint8)


def _check_rows(rep, excluded, max_k, slices, what: str):
    if not isinstance(rep, torch.Tensor) or rep.dim() != 2 or rep.dtype != torch.float32 or rep.device.type != "cuda":
        raise ValueError(f"{what}: rep must be fp32 [B, V] on a GPU")
    if not rep.is_contiguous():
        raise ValueError(f"{what}: rep must be contiguous")
    B, V = rep.shape
    if V < 1:
        raise ValueError(f"{what}: V must be >= 1")
    if (not isinstance(excluded, torch.Tensor) or excluded.dtype != torch.uint8 or tuple(excluded.shape) != (V,)
            or excluded.device != rep.device or not excluded.is_contiguous()):
        raise ValueError(f"{what}: excluded must be uint8 [{V}] on rep's device")
    if isinstance(max_k, bool) or not isinstance(max_k, (int, np.integer)) or not 1 <= int(max_k) < 2 ** 31:
        raise ValueError(f"{what}: max_k must be an int >= 1")
    if isinstance(slices, bool) or not isinstance(slices, (int, np.integer)) or not 0 <= int(slices) < 2 ** 31:
        raise ValueError(f"{what}: slices must be 0 (choose) or a positive int (more than V slices run as V)")
    return int(B), int(V)


def _workspace(B: int, nj: int, dev):
    need = int(fn("snx_expansion_workspace_bytes")(B, nj))
    return torch.empty(max(need, 1), dtype=torch.uint8, device=dev), need


def judged_ranks(rep: torch.Tensor, excluded: torch.Tensor, j_ptr, j_tok, max_k: int, slices: int = 0
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Positions of judged tokens in the ranking of each row (snx_expansion_ranks).  ``rep`` fp32 [B, V] on a GPU,
    ``excluded`` uint8 [V]; an entry is ranked when rep > 0 and it is not excluded, the order is weight descending, ties
    lowest id first, cut after ``max_k``.  ``j_ptr`` [B+1], ``j_tok`` [nj]: the judged ids of every row (distinct within a
    row).  -> (rank int32 [nj]: 1-based position, 0 = not in the cut list; nranked int32 [B] = min(max_k, ranked entries)).
    ``slices``: column slices per row (0: chosen); it changes no bit."""
    B, V = _check_rows(rep, excluded, max_k, slices, "judged_ranks")
    tok = _host_ints(j_tok, "j_tok")
    ptr, tok, _, _ = judgment_csr((j_ptr, tok, np.zeros_like(tok), np.zeros_like(tok)), B)
    dev, nj = rep.device, int(tok.shape[0])
    d_ptr, d_tok = torch.from_numpy(ptr).to(dev), torch.from_numpy(tok).to(dev)
    rank = torch.empty(nj, dtype=torch.int32, device=dev)
    nranked = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return rank, nranked
    ws, need = _workspace(B, nj, dev)
    with torch.cuda.device(dev):
        call("snx_expansion_ranks", _p(rep), B, V, _p(excluded), _p(d_ptr), _p(d_tok), nj, int(max_k), int(slices),
             _p(rank), _p(nranked), _p(ws), need, _stream())
    return rank, nranked


def graded_metrics(rep: torch.Tensor, excluded: torch.Tensor, judgments, k_values: Sequence[int], max_k=None,
                   slices: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Graded ranking metrics of every row in one call (snx_expansion_metrics).  ``rep``, ``excluded``, ``slices`` as
    ``judged_ranks``; ``judgments`` as ``judgment_csr`` takes them; ``k_values``: 1 .. 8 strictly ascending cutoffs >= 1
    (one above ``max_k`` means the whole list); ``max_k``: where the ranking is cut (default: the largest cutoff).
    -> (rank int32 [nj], nranked int32 [B], first int32 [B]: smallest position among the row's ``rel`` members, 0 = none;
    hits int32 [B, ncut]: ``rel`` members at positions <= each cutoff; dcg float64 [B, ncut]: the left fold in position order
    of ``gain_table`` entries over the judged entries with grade > 0 within each cutoff)."""
    cuts = list(k_values)
    if not 1 <= len(cuts) <= CUTOFFS_MAX or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) for c in cuts):
        raise ValueError(f"graded_metrics: 1 .. {CUTOFFS_MAX} integer cutoffs")
    cuts = [int(c) for c in cuts]
    if cuts[0] < 1 or cuts[-1] >= 2 ** 31 or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError("graded_metrics: cutoffs must be >= 1 and ascend strictly")
    if max_k is None:
        max_k = cuts[-1]
    B, V = _check_rows(rep, excluded, max_k, slices, "graded_metrics")
    ptr, tok, grade, rel = judgment_csr(judgments, B)
    dev = rep.device
    d_ptr, d_tok, d_grade, d_rel = (torch.from_numpy(x).to(dev) for x in (ptr, tok, grade, rel))
    return launch_metrics(rep, excluded, d_ptr, d_tok, d_grade, d_rel, cuts, int(max_k), int(slices))


def launch_metrics(rep, excluded, d_ptr, d_tok, d_grade, d_rel, cuts, max_k: int, slices: int = 0):
    """The launch behind ``graded_metrics`` with the judgments already on the device and already checked (``judgment_csr``):
    allocates the outputs and the workspace, enqueues the call on the current stream and returns without synchronising."""
    dev, (B, V), nj, ncut = rep.device, rep.shape, int(d_tok.shape[0]), len(cuts)
    G = min(max_k, cuts[-1])
    gain = _gain_on(G, dev)
    rank = torch.empty(nj, dtype=torch.int32, device=dev)
    nranked = torch.empty(B, dtype=torch.int32, device=dev)
    first = torch.empty(B, dtype=torch.int32, device=dev)
    hits = torch.empty((B, ncut), dtype=torch.int32, device=dev)
    dcg = torch.empty((B, ncut), dtype=torch.float64, device=dev)
    if B == 0:
        return rank, nranked, first, hits, dcg
    ws, need = _workspace(B, nj, dev)
    host = (C.c_int32 * ncut)(*cuts)
    with torch.cuda.device(dev):
        call("snx_expansion_metrics", _p(rep), B, V, _p(excluded), _p(d_ptr), _p(d_tok), _p(d_grade), _p(d_rel), nj,
             max_k, C.cast(host, C.c_void_p), ncut, _p(gain), G, slices, _p(rank), _p(nranked), _p(first), _p(hits),
             _p(dcg), _p(ws), need, _stream())
    return rank, nranked, first, hits, dcg

"""Co-occurrence counts and PMI on the GPU (csrc/cooc.hip, include/snx.h "Co-occurrence and PMI"): the two loops of the
reference's src/pmi package (ref:src/pmi/cooccurrence.py:206-226, ref:src/pmi/pmi_calculator.py:142-193) as kernels.

The device sees token ids only.  The host's part is the text: splitting a document into sentence or paragraph windows,
interning tokens in first-appearance order, and the vocabulary cut (``sentence_windows``, ``paragraph_windows``,
``Interner``, ``select_vocabulary``; none of them needs a GPU).  ``cooccurrence`` turns id rows into the count matrix:
the kernels emit one record per distinct (row term, col term) of a window, in chunks of whole windows bounded by
``max_records``; a chunk is reduced by one ``torch.unique`` with exact integer sums, and the chunks are merged by the
same reduction."""
import math
import re
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._abi import CONSTANTS
from ._lib import call
from .ops import _p, _stream
from .retrieval._common import cuda_device, offsets, workspace

LDS_TOKENS = CONSTANTS["SNX_COOC_LDS_TOKENS"]     # tokens of a window that LDS holds
WAVE_TOKENS = 64                       # tokens of a window that one wave takes (CO_WAVE of csrc/cooc.hip)
DEFAULT_MAX_RECORDS = 1 << 24          # 16 Mi records of 16 (20 when normalised) bytes
WINDOW_BLOCK = 1 << 22                 # windows whose record counts one pass-1 launch takes
V_MAX = 3037000499                     # the largest V with V * V < 2^63
LOG2, LOGE, LOGB = (CONSTANTS["SNX_COOC_" + n] for n in ("LOG2", "LOGE", "LOGB"))

_SENTENCE_END = re.compile(r"[.!?\n]")


# ------------------------------------------------------------------------------------------------ host half: the text
def sentence_windows(document: str) -> List[str]:
    """The sentences of ``document``: split at any of ``.!?`` and newline, stripped, empties dropped
    (ref:cooccurrence.py:269-284)."""
    return [s for s in (p.strip() for p in _SENTENCE_END.split(document)) if s]


def paragraph_windows(document: str) -> List[str]:
    """The paragraphs of ``document``: split at an empty line, the pieces that are not blank, NOT stripped
    (ref:cooccurrence.py:300-305)."""
    return [p for p in document.split("\n\n") if p.strip()]


class Interner:
    """Strings -> ids in order of first appearance.  One interner serves the document-level stream (vocabulary and
    frequencies) and the window-level stream, so that a window token the documents never showed gets an id past the
    document terms and no vocabulary entry."""

    def __init__(self):
        self.ids: Dict[str, int] = {}
        self.terms: List[str] = []

    def __len__(self) -> int:
        return len(self.terms)

    def intern(self, tokens: Iterable[str]) -> List[int]:
        ids, terms, out = self.ids, self.terms, []
        for t in tokens:
            i = ids.get(t)
            if i is None:
                i = ids[t] = len(terms)
                terms.append(t)
            out.append(i)
        return out


def select_vocabulary(term_freq, min_term_freq: int, max_vocab_size: int) -> np.ndarray:
    """The reference's vocabulary cut (ref:cooccurrence.py:158-172) over first-appearance ids: keep ``freq >=
    min_term_freq``, order by descending frequency with ties in first-appearance order (a stable sort), keep the first
    ``max_vocab_size``.  -> int64 [len(term_freq)]: the new id of every old id, -1 for a dropped term."""
    freq = np.asarray(term_freq)
    if freq.ndim != 1 or (freq.size and not np.issubdtype(freq.dtype, np.integer)):
        raise ValueError("select_vocabulary: term_freq must be an int vector")
    if isinstance(max_vocab_size, bool) or not isinstance(max_vocab_size, (int, np.integer)) or int(max_vocab_size) < 0:
        raise ValueError("select_vocabulary: max_vocab_size must be an int >= 0")
    freq = freq.astype(np.int64)
    kept = np.flatnonzero(freq >= min_term_freq)
    order = kept[np.argsort(-freq[kept], kind="stable")][: int(max_vocab_size)]
    new = np.full(freq.size, -1, dtype=np.int64)
    new[order] = np.arange(order.size, dtype=np.int64)
    return new


def id_rows(rows: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """Lists of ids -> the CSR (ptr int64 [n+1], ids int32) that ``cooccurrence`` takes."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    if len(rows):
        np.cumsum(np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows)), out=ptr[1:])
    flat = np.fromiter((i for r in rows for i in r), dtype=np.int64, count=int(ptr[-1]))
    return ptr, flat.astype(np.int32)


def sliding_window_counts(lens: np.ndarray, window_size: int) -> np.ndarray:
    """Windows of rows of ``lens`` tokens under a sliding window (ref:cooccurrence.py:321-331): none for an empty row, one
    for a row of at most ``window_size`` tokens, else ``n - window_size + 1``."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens == 0, 0, np.where(lens <= window_size, 1, lens - window_size + 1)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ validation
def _int(v, name: str, who: str, lo: int, hi: Optional[int] = None) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{who}: {name} must be an int")
    if int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(f"{who}: {name} must be " + (f">= {lo}" if hi is None else f"in [{lo}, {hi}]"))
    return int(v)


def check_rows(ptr, ids, V, who: str = "cooccurrence") -> Tuple[np.ndarray, np.ndarray, int]:
    """Validation of the id rows (no GPU involved) -> (ptr int64, ids int32, V)."""
    V = _int(V, "V", who, 1, V_MAX)
    ptr = np.asarray(ptr.cpu() if isinstance(ptr, torch.Tensor) else ptr)
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
    if ptr.ndim != 1 or ptr.size < 1 or not np.issubdtype(ptr.dtype, np.integer):
        raise ValueError(f"{who}: ptr must be an int vector [n + 1]")
    if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
        raise ValueError(f"{who}: ids must be an int vector")
    ptr = ptr.astype(np.int64)
    if ptr[0] != 0 or ptr[-1] != ids.size or (ptr[1:] < ptr[:-1]).any():
        raise ValueError(f"{who}: ptr must start at 0, not decrease and end at len(ids)")
    if ptr.size - 1 >= 2 ** 31:
        raise ValueError(f"{who}: at most 2^31 - 1 rows")
    if ids.size and (int(ids.min()) < -1 or int(ids.max()) >= V):
        raise ValueError(f"{who}: ids must lie in [0, {V}) or be -1 (a token outside the vocabulary)")
    return ptr, ids.astype(np.int32), V


@dataclass
class CooccurrenceCSR:
    """The count matrix on the device: ``indptr`` int64 [V+1], ``indices`` int32 strictly ascending per row, ``data``
    fp32, ``counts`` int64 (None when normalised), no stored zeros."""
    indptr: torch.Tensor
    indices: torch.Tensor
    data: torch.Tensor
    counts: Optional[torch.Tensor]
    total_windows: int
    shape: Tuple[int, int]

    @property
    def nnz(self) -> int:
        return int(self.indices.numel())

    def numpy(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(data fp32, indices int32, indptr int64) on the host: the triple ``scipy.sparse.csr_matrix`` takes."""
        return self.data.cpu().numpy(), self.indices.cpu().numpy(), self.indptr.cpu().numpy()


# ------------------------------------------------------------------------------------------------ counting
def _reduce(key: torch.Tensor, m: Optional[torch.Tensor], adds: torch.Tensor, span: int):
    """Records -> one entry per distinct key (and window length), ascending, with exact integer sums."""
    u, inv = torch.unique(key, sorted=True, return_inverse=True)
    if m is None:
        return u, None, torch.zeros(u.numel(), dtype=torch.long, device=key.device).index_add_(0, inv, adds)
    u2, inv2 = torch.unique(inv * span + m.long(), sorted=True, return_inverse=True)
    total = torch.zeros(u2.numel(), dtype=torch.long, device=key.device).index_add_(0, inv2, adds)
    return u[torch.div(u2, span, rounding_mode="floor")], (u2 % span).to(torch.int32), total


def cooccurrence(ptr, ids, V: int, *, window_size: Optional[int] = None, symmetric: bool = True, normalize: bool = False,
                 max_records: int = DEFAULT_MAX_RECORDS, device="cuda") -> CooccurrenceCSR:
    """Windowed co-occurrence counts of id rows (snx_cooc_windows; include/snx.h "Co-occurrence and PMI").

    ``ptr`` int [n+1], ``ids`` int in [0, V) or -1: the rows.  ``window_size=None``: every row is one window (sentence and
    paragraph mode).  ``window_size=w``: every row is a document under a sliding window of ``w`` tokens, expanded on the
    device.  A window whose valid ids are ``idx`` (m of them, m >= 2) adds ``1`` (``1 / m`` when ``normalize``) to
    ``C[idx_i, idx_j]`` for every position pair i < j, and to ``C[idx_j, idx_i]`` when ``symmetric``.
    ``normalize=False``: exact int64 ``counts`` and ``data = fp32(counts)``.  ``normalize=True``: a cell is the sum over m
    of (additions at window length m) / m in float64, ascending m, rounded to fp32 once; ``counts`` is None.
    ``max_records`` bounds the record buffer: the windows are taken in chunks of whole windows whose records fit it (a
    window that alone exceeds it is its own chunk), and the chunk results are merged by the same sort."""
    who = "cooccurrence"
    ptr, ids, V = check_rows(ptr, ids, V, who)
    w = None if window_size is None else _int(window_size, "window_size", who, 1, 2 ** 31 - 1)
    max_records = _int(max_records, "max_records", who, 1)
    dev = cuda_device(device)
    if dev.type != "cuda":
        raise ValueError(f"{who}: runs on a GPU")
    n_rows = int(ptr.size - 1)
    lens = ptr[1:] - ptr[:-1]
    longest_row = int(lens.max()) if n_rows else 0
    if w is None:
        nwin, longest, d_win = n_rows, longest_row, None
    else:
        win = np.zeros(n_rows + 1, dtype=np.int64)
        np.cumsum(sliding_window_counts(lens, w), out=win[1:])
        nwin, longest = int(win[-1]), min(longest_row, w)
        d_win = torch.from_numpy(win).to(dev)
    if longest >= 2 ** 31:
        raise ValueError(f"{who}: a window holds at most 2^31 - 1 tokens")
    span = longest + 1                                        # window lengths m lie in [0, span)
    parts: List[tuple] = []
    merged = 0

    def merge():
        nonlocal parts, merged
        if len(parts) > 1:
            key = torch.cat([p[0] for p in parts])
            m = torch.cat([p[1] for p in parts]) if normalize else None
            parts = [_reduce(key, m, torch.cat([p[2] for p in parts]), span)]
        merged = int(parts[0][0].numel()) if parts else 0

    with torch.cuda.device(dev):
        if nwin:
            d_ptr = torch.from_numpy(ptr).to(dev)
            d_ids = torch.from_numpy(ids).to(dev) if ids.size else None
            ws, ws_bytes = workspace("snx_cooc_workspace_bytes", dev, longest)
            for b0 in range(0, nwin, WINDOW_BLOCK):
                nb = min(WINDOW_BLOCK, nwin - b0)
                cnt = torch.empty(nb, dtype=torch.long, device=dev)
                call("snx_cooc_windows", _p(d_ptr), _p(d_ids), n_rows, _p(d_win), w or 0, b0, nb, longest, V,
                     int(bool(symmetric)), None, _p(cnt), None, None, None, _p(ws), ws_bytes, _stream())
                cum = offsets(cnt)
                s = 0
                while s < nb:                                 # chunks of whole windows within max_records
                    bound = cum[s:s + 1] + max_records
                    e = min(max(int(torch.searchsorted(cum, bound, right=True)) - 1, s + 1), nb)
                    nrec = int(cum[e] - cum[s])
                    if nrec:
                        key = torch.empty(nrec, dtype=torch.long, device=dev)
                        adds = torch.empty(nrec, dtype=torch.long, device=dev)
                        m = torch.empty(nrec, dtype=torch.int32, device=dev) if normalize else None
                        rec_ptr = cum[s:e + 1].contiguous()
                        call("snx_cooc_windows", _p(d_ptr), _p(d_ids), n_rows, _p(d_win), w or 0, b0 + s, e - s, longest, V,
                             int(bool(symmetric)), _p(rec_ptr), None, _p(key), _p(adds), _p(m), _p(ws), ws_bytes,
                             _stream())
                        parts.append(_reduce(key, m, adds, span))
                        if sum(int(p[0].numel()) for p in parts) > 2 * max(merged, max_records):
                            merge()
                    s = e
        merge()
        if parts:
            key, m, adds = parts[0]
        else:
            key = adds = torch.zeros(0, dtype=torch.long, device=dev)
            m = torch.zeros(0, dtype=torch.int32, device=dev)
        if normalize:                                         # entries ascending by (key, m) -> one fp32 value per cell
            key, per_cell = torch.unique_consecutive(key, return_counts=True)
            value = torch.empty(key.numel(), dtype=torch.float32, device=dev)
            cell_ptr = offsets(per_cell)
            call("snx_cooc_normalized_cells", _p(cell_ptr), _p(m), _p(adds), int(key.numel()), _p(value), _stream())
            counts = None
        else:
            counts, value = adds, adds.to(torch.float32)
        row, col = torch.div(key, V, rounding_mode="floor"), key % V
        if symmetric and key.numel():                         # the kernels emitted row <= col only: mirror once
            off = row != col
            order = torch.argsort(torch.cat([key, col[off] * V + row[off]]))
            row, col = torch.cat([row, col[off]])[order], torch.cat([col, row[off]])[order]
            value = torch.cat([value, value[off]])[order]
            counts = None if counts is None else torch.cat([counts, counts[off]])[order]
        indptr = offsets(torch.bincount(row, minlength=V))
    return CooccurrenceCSR(indptr, col.to(torch.int32).contiguous(), value.contiguous(),
                           None if counts is None else counts.contiguous(), nwin, (V, V))


# ------------------------------------------------------------------------------------------------ PMI
def log_mode(log_base: float) -> Tuple[int, float]:
    """(base mode, ln(base)) as the reference chooses its logarithm (ref:pmi_calculator.py:182-187)."""
    if log_base == 2.0:
        return LOG2, math.log(2.0)
    if log_base == np.e:
        return LOGE, 1.0
    if not log_base > 0 or log_base == 1.0:
        raise ValueError("pmi: log_base must be > 0 and not 1")
    return LOGB, float(np.log(log_base))


def _pmi_args(csr: CooccurrenceCSR, marginals, total, config, who: str):
    if not isinstance(csr, CooccurrenceCSR) or csr.indptr.device.type != "cuda":
        raise ValueError(f"{who}: csr must be a CooccurrenceCSR on a GPU")
    dev, V = csr.indptr.device, int(csr.shape[0])
    mg = torch.as_tensor(np.ascontiguousarray(np.asarray(marginals, dtype=np.float64)))
    if mg.dim() != 1 or mg.numel() != V:
        raise ValueError(f"{who}: marginals must be float64 [{V}]")
    k = float(config.laplace_smoothing)
    if not k >= 0:
        raise ValueError(f"{who}: laplace_smoothing must be >= 0")
    mode, ln_base = log_mode(float(config.log_base))
    return dev, V, mg.to(dev), (float(total), k, float(config.min_cooccurrence), int(bool(config.use_ppmi)), mode, ln_base)


def pmi_values(csr: CooccurrenceCSR, marginals, total: float, config) -> torch.Tensor:
    """PMI of every stored cell of ``csr`` (snx_cooc_pmi_cells) -> float64 [nnz] on its device.  ``marginals`` float64
    [V] and ``total`` are the host's; ``config`` has laplace_smoothing, use_ppmi, log_base, min_cooccurrence."""
    dev, V, mg, scalars = _pmi_args(csr, marginals, total, config, "pmi_values")
    out = torch.empty(csr.nnz, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        call("snx_cooc_pmi_cells", _p(csr.indptr), _p(csr.indices), _p(csr.data), V, csr.nnz, _p(mg), *scalars, _p(out),
             _stream())
    return out


def pmi_pairs(csr: CooccurrenceCSR, rows, cols, marginals, total: float, config) -> torch.Tensor:
    """PMI of the cells (rows[i], cols[i]) (snx_cooc_pmi_pairs) -> float64 [n]; an absent cell counts 0, a negative index
    is a term outside the vocabulary: 0.0 under PPMI, -inf without."""
    dev, V, mg, scalars = _pmi_args(csr, marginals, total, config, "pmi_pairs")
    r = torch.as_tensor(np.asarray(rows)) if not isinstance(rows, torch.Tensor) else rows
    c = torch.as_tensor(np.asarray(cols)) if not isinstance(cols, torch.Tensor) else cols
    if r.dim() != 1 or c.dim() != 1 or r.numel() != c.numel() or r.is_floating_point() or c.is_floating_point():
        raise ValueError("pmi_pairs: rows and cols must be int vectors of one length")
    if r.numel() and (int(r.max()) >= V or int(c.max()) >= V):
        raise ValueError(f"pmi_pairs: indices must be < {V} (negative: outside the vocabulary)")
    r = r.clamp(min=-1).to(dev, torch.int32).contiguous()
    c = c.clamp(min=-1).to(dev, torch.int32).contiguous()
    out = torch.empty(r.numel(), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        call("snx_cooc_pmi_pairs", _p(csr.indptr), _p(csr.indices if csr.nnz else None),
             _p(csr.data if csr.nnz else None), V, _p(r), _p(c), int(r.numel()), _p(mg), *scalars, _p(out), _stream())
    return out

"""Corpus preparation on the GPU (csrc/textprep.hip, include/snx.h "Corpus preparation"): the paragraph segmentation, the
validity filter, the SHA-256 of rows and the first-occurrence dedup of the reference's MLM data script
(ref:scripts/prepare_korean_mlm_data.py:31-58, 201-217), with the reference's decisions paragraph for paragraph.

The host's part is the text: documents to a CSR of code points and paragraphs back to ``str``.  Nothing is lowered or
stripped here; the device strips."""
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np
import torch

from ._lib import call
from ._text import LoneSurrogateError, code_point_csr, csr_to_device  # noqa: F401  (the first two: this module's names too)
from .ops import _p, _stream
from .retrieval._common import offsets, workspace

TILE = 256                             # code points of one tile of the segmentation (TX_TILE of csrc/textprep.hip)
FIRST_EQUAL_MAX = 2 ** 29              # rows of one first_equal call (TX_DEDUP_MAX)
HANGUL_LO, HANGUL_HI = 0xAC00, 0xD7AF  # the reference's range, inclusive (ref:prepare_korean_mlm_data.py:20)


@dataclass
class Paragraphs:
    """The stripped, non-empty pieces of a batch of documents, in document order, as device tensors."""
    par_ptr: torch.Tensor              # int64 [np + 1]
    par_cps: torch.Tensor              # int32 [par_ptr[np]]
    par_doc: torch.Tensor              # int32 [np], the piece's document
    par_hangul: torch.Tensor           # int32 [np], code points in U+AC00 .. U+D7AF
    n_docs: int

    def __len__(self) -> int:
        return self.par_doc.numel()

    @property
    def lengths(self) -> torch.Tensor:
        return self.par_ptr[1:] - self.par_ptr[:-1]


def segment_paragraphs(docs: Sequence[str], device="cuda") -> Paragraphs:
    """Rules 1-3 of the reference's ``clean_text`` and ``split_paragraphs`` (ref:prepare_korean_mlm_data.py:31-40) on
    the GPU (snx_tx_segment_*): blank runs collapse to one U+0020, runs of two or more U+000A cut a document into pieces,
    every piece is stripped of ``str.isspace`` white space, empty pieces are dropped."""
    return segment_csr(*code_point_csr(docs, "segment_paragraphs"), device=device)


def segment_csr(ptr, code_points, device=None) -> Paragraphs:
    """``segment_paragraphs`` of documents that are already a CSR of code points (numpy arrays or tensors)."""
    d_ptr, d_cps, dev = csr_to_device(ptr, code_points, device, "segment_paragraphs")
    n = d_ptr.numel() - 1
    i32 = dict(dtype=torch.int32, device=dev)
    if n == 0:
        return Paragraphs(torch.zeros(1, dtype=torch.long, device=dev), torch.empty(0, **i32), torch.empty(0, **i32),
                          torch.empty(0, **i32), 0)
    doc_pieces = torch.empty(n, dtype=torch.long, device=dev)
    doc_cps = torch.empty(n, dtype=torch.long, device=dev)
    with torch.cuda.device(dev):
        call("snx_tx_segment_count", _p(d_ptr), _p(d_cps), n, _p(doc_pieces), _p(doc_cps), _stream())
        piece_base = offsets(doc_pieces)
        n_par, n_cps = torch.stack((piece_base[-1], doc_cps.sum())).tolist()     # the one read-back
        par_len = torch.empty(n_par, dtype=torch.long, device=dev)
        par_doc, par_hangul, par_cps = torch.empty(n_par, **i32), torch.empty(n_par, **i32), torch.empty(n_cps, **i32)
        if n_par:
            call("snx_tx_segment_meta", _p(d_ptr), _p(d_cps), n, _p(piece_base), _p(par_len), _p(par_doc),
                 _p(par_hangul), _stream())
        par_ptr = offsets(par_len)
        if n_par:
            call("snx_tx_segment_fill", _p(d_ptr), _p(d_cps), n, _p(piece_base), _p(par_ptr), _p(par_cps), _stream())
    return Paragraphs(par_ptr, par_cps, par_doc, par_hangul, n)


def valid_mask(lengths, hangul, min_length: int, min_korean_ratio: float) -> torch.Tensor:
    """The reference's ``is_valid_paragraph`` (ref:prepare_korean_mlm_data.py:43-53) on two int vectors -> bool [n].
    The ratio is Python's: ``hangul / len`` as ONE correctly rounded float64 division, then the comparison with the
    float -- not the rational comparison and not ``hangul >= ratio * len`` (at 0.1, 1 of 10 passes here and fails
    those).  An empty paragraph has ratio 0.0 (ref:prepare_korean_mlm_data.py:25-26)."""
    if isinstance(min_length, bool) or not isinstance(min_length, (int, np.integer)):
        raise ValueError("valid_mask: min_length must be an int")
    if isinstance(min_korean_ratio, bool) or not isinstance(min_korean_ratio, (int, float, np.floating, np.integer)):
        raise ValueError("valid_mask: min_korean_ratio must be a number")
    lengths, hangul = torch.as_tensor(lengths), torch.as_tensor(hangul)
    if lengths.dim() != 1 or lengths.shape != hangul.shape or lengths.is_floating_point() or hangul.is_floating_point():
        raise ValueError("valid_mask: lengths and hangul must be int vectors of one size")
    hangul = hangul.to(lengths.device)
    one = torch.ones((), dtype=torch.float64, device=lengths.device)
    ratio = torch.where(lengths > 0, hangul.to(torch.float64) / torch.where(lengths > 0, lengths.to(torch.float64), one),
                        0.0 * one)
    return ~(lengths < int(min_length)) & ~(ratio < float(min_korean_ratio))


def sha256_rows(ptr, code_points, device=None) -> torch.Tensor:
    """SHA-256 of the UTF-8 bytes of every row of a code-point CSR on the GPU (snx_tx_sha256_rows) -> uint32 [n, 8], most
    significant word first: ``"".join("%08x" % w for w in row)`` is ``hashlib.sha256(text.encode()).hexdigest()``
    (ref:prepare_korean_mlm_data.py:56-58)."""
    d_ptr, d_cps, dev = csr_to_device(ptr, code_points, device, "sha256_rows")
    if d_cps is not None and not bool(((d_cps >= 0) & (d_cps <= 0x10FFFF) & ((d_cps < 0xD800) | (d_cps > 0xDFFF))).all()):
        raise ValueError("sha256_rows: code points must be Unicode scalar values (no surrogates)")
    n = d_ptr.numel() - 1
    digest = torch.empty((n, 8), dtype=torch.int32, device=dev)
    if n:
        with torch.cuda.device(dev):
            call("snx_tx_sha256_rows", _p(d_ptr), _p(d_cps), n, _p(digest), _stream())
    return digest.view(torch.uint32)


def first_equal(digests: torch.Tensor) -> torch.Tensor:
    """``digests`` uint32 [n, 8] on a GPU -> int32 [n]: the smallest row index whose digest equals row i's in all 256
    bits (snx_tx_first_equal); row i is a first occurrence iff ``first[i] == i`` (ref:prepare_korean_mlm_data.py:210-216)."""
    if not isinstance(digests, torch.Tensor) or digests.dim() != 2 or digests.shape[1] != 8 or \
            digests.dtype not in (torch.uint32, torch.int32) or digests.device.type != "cuda":
        raise ValueError("first_equal: digests must be uint32 [n, 8] on a GPU")
    n = digests.shape[0]
    if n > FIRST_EQUAL_MAX:
        raise ValueError(f"first_equal: at most {FIRST_EQUAL_MAX} rows")
    d = digests.contiguous()
    d = d if d.dtype == torch.int32 else d.view(torch.int32)
    dev = d.device
    first = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        ws, ws_bytes = workspace("snx_tx_first_equal_workspace_bytes", dev, n)
        with torch.cuda.device(dev):
            call("snx_tx_first_equal", _p(d), n, _p(first), _p(ws), ws_bytes, _stream())
    return first


def gather_rows(ptr: torch.Tensor, values: torch.Tensor, rows) -> Tuple[torch.Tensor, torch.Tensor]:
    """The rows ``rows`` of a CSR, in that order, as a CSR of their own on the same device."""
    rows = torch.as_tensor(rows, dtype=torch.long, device=ptr.device)
    if rows.dim() != 1 or (rows.numel() and not bool(((rows >= 0) & (rows < ptr.numel() - 1)).all())):
        raise ValueError(f"gather_rows: rows must be indices in [0, {ptr.numel() - 1})")
    lens = ptr[rows + 1] - ptr[rows]
    out_ptr = offsets(lens)
    total = int(out_ptr[-1])
    src = torch.repeat_interleave(ptr[rows] - out_ptr[:-1], lens, output_size=total) + \
        torch.arange(total, dtype=torch.long, device=ptr.device)
    return out_ptr, values[src]


def csr_texts(ptr: np.ndarray, code_points: np.ndarray) -> List[str]:
    """A host CSR of code points -> its rows as ``str``."""
    whole = np.ascontiguousarray(code_points, dtype="<u4").tobytes().decode("utf-32-le", errors="surrogatepass")
    edge = ptr.tolist()
    return [whole[edge[i]:edge[i + 1]] for i in range(len(edge) - 1)]


def paragraph_texts(par_ptr: torch.Tensor, par_cps: torch.Tensor, rows=None) -> List[str]:
    """The paragraphs ``rows`` (all when None), in that order, back on the host as ``str``."""
    if rows is not None:
        par_ptr, par_cps = gather_rows(par_ptr, par_cps, rows)
    return csr_texts(par_ptr.cpu().numpy(), par_cps.cpu().numpy())

"""The host front of the text kernels (WordPiece, Unigram, MinHash, TF-IDF, corpus preparation): texts as rows of Unicode
code points in CSR form, ``ptr`` int64 [n+1] and ``code_points`` int32, and their upload.  What a section does to its
texts first (``lower``, ``strip``, a join of words, NFC) stays with the section; ``who`` is the caller's name, the prefix
of every message."""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch


class LoneSurrogateError(ValueError):
    """A text holds a lone surrogate; ``index`` is the first such text."""

    def __init__(self, message: str, index: int):
        super().__init__(message)
        self.index = index


def code_point_csr(texts: Sequence[str], who: str = "code_point_csr") -> Tuple[np.ndarray, np.ndarray]:
    """Every text as it is, as a CSR of Unicode code points: (ptr int64 [n+1], code_points int32).  A lone surrogate
    raises (it has no UTF-8 form)."""
    texts = list(texts)
    try:
        whole = "".join(texts)                                 # the join is the type check: it takes nothing but str
    except TypeError:
        raise ValueError(f"{who}: texts must be strings") from None
    ptr = np.zeros(len(texts) + 1, dtype=np.int64)
    if texts:
        np.cumsum(np.fromiter(map(len, texts), dtype=np.int64, count=len(texts)), out=ptr[1:])
    try:
        raw = whole.encode("utf-32-le")
    except UnicodeEncodeError:
        bad = next(i for i, t in enumerate(texts) if any(0xD800 <= ord(ch) <= 0xDFFF for ch in t))
        raise LoneSurrogateError(f"{who}: text {bad} holds a lone surrogate (U+D800..U+DFFF), which has no UTF-8 form",
                                 bad) from None
    return ptr, np.frombuffer(raw, dtype="<u4").astype(np.int32)


def csr_to_device(ptr, cps, device, who: str, trusted: bool = False
                  ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.device]:
    """(ptr, code_points) as numpy arrays or tensors -> int64 / int32 tensors on one GPU (no code point: None), checked to
    be a CSR.  ``trusted``: the pair is what ``code_point_csr`` returned, or rows cut out of it, and the checks of its
    contents, which read four numbers back from the device, are left out."""
    from .retrieval._common import cuda_device
    if isinstance(ptr, np.ndarray):
        ptr = torch.from_numpy(np.ascontiguousarray(ptr))
    if isinstance(cps, np.ndarray):
        cps = torch.from_numpy(np.ascontiguousarray(cps))
    if not isinstance(ptr, torch.Tensor) or not isinstance(cps, torch.Tensor) or ptr.dim() != 1 or cps.dim() != 1 or \
            ptr.dtype != torch.int64 or cps.dtype != torch.int32 or ptr.numel() < 1:
        raise ValueError(f"{who}: rows are ptr int64 [n+1] and code_points int32")
    if device is None:
        device = ptr.device if ptr.is_cuda else cps.device if cps.is_cuda else "cuda"
    dev = cuda_device(device)
    if dev.type != "cuda":
        raise ValueError(f"{who}: runs on a GPU")
    if ptr.numel() - 1 >= 2 ** 31:
        raise ValueError(f"{who}: at most 2^31 - 1 rows")
    ptr, cps = ptr.to(dev).contiguous(), cps.to(dev).contiguous()
    if not trusted:
        lens = ptr[1:] - ptr[:-1]
        if int(ptr[0]) != 0 or int(ptr[-1]) != cps.numel() or (lens.numel() and
                                                                 (int(lens.min()) < 0 or int(lens.max()) >= 2 ** 31)):
            raise ValueError(f"{who}: ptr must start at 0, not decrease, end at len(code_points), rows shorter than 2^31")
    return ptr, (cps if cps.numel() else None), dev

"""MinHash near-duplicate removal on the GPU (csrc/minhash.hip, include/snx.h "MinHash near-duplicate removal"): the two
loops of the reference's MinHashDeduplicator (ref:src/preprocessing/cleaners/deduplicator.py:10-187) as kernels, with the
reference's decisions row for row.

The host's part is the text: Python's Unicode ``lower`` and ``strip`` (ref:deduplicator.py:50), the rows as a CSR of code
points, the check that every MD5 message fits one block, and ``need``, the integer form of the reference's float
comparison ``matches / num_perm >= threshold`` (ref:deduplicator.py:96-97, 137)."""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _text
from ._abi import CONSTANTS
from ._lib import call
from .ops import _p, _stream
from .retrieval._common import workspace

MSG_MAX = CONSTANTS["SNX_MINHASH_MSG_MAX"]        # message bytes that one MD5 block holds
PERM_MAX = CONSTANTS["SNX_MINHASH_PERM_MAX"]
FIRST_MATCH_ROWS = 65535               # rows of one snx_minhash_first_match call
DEDUP_BLOCK = 512                      # rows whose order dependence one workgroup resolves (MH_B of csrc/minhash.hip)


def need_matches(num_perm: int, threshold: float) -> int:
    """The smallest integer m with ``m / num_perm >= threshold`` in Python float arithmetic, the reference's own test
    (ref:deduplicator.py:97, 137); ``num_perm + 1`` ("never") when no m in [0, num_perm] passes -- a threshold above 1,
    or a NaN."""
    num_perm = int(num_perm)
    if num_perm < 1:
        raise ValueError("need_matches: num_perm must be >= 1")
    threshold = float(threshold)
    for m in range(num_perm + 1):
        if m / num_perm >= threshold:
            return m
    return num_perm + 1


def pair_text(query: str, positive: str) -> str:
    """The text the reference signs for a (query, positive) pair (ref:deduplicator.py:130), before lower and strip."""
    return f"{query} {positive}"


def code_point_csr(texts: Sequence[str], who: str = "code_point_csr") -> Tuple[np.ndarray, np.ndarray]:
    """``text.lower().strip()`` of every text as a CSR of Unicode code points: (ptr int64 [n+1], code_points int32).
    ``lower`` is Python's and may change the length (``İ`` becomes two code points).  A lone surrogate raises, as the
    reference's ``.encode()`` does."""
    texts = list(texts)
    if any(not isinstance(t, str) for t in texts):
        raise ValueError(f"{who}: texts must be strings")
    return _text.code_point_csr([t.lower().strip() for t in texts], who)


def longest_message_bytes(ptr: np.ndarray, code_points: np.ndarray, ngram_size: int, num_perm: int) -> int:
    """The longest MD5 message of a batch: ``len(str(num_perm - 1)) + 1`` + the UTF-8 bytes of its longest n-gram."""
    n_g = int(ngram_size)
    cp = code_points.astype(np.int64)
    nbytes = 1 + (cp >= 0x80) + (cp >= 0x800) + (cp >= 0x10000)
    cum = np.concatenate([np.zeros(1, np.int64), np.cumsum(nbytes, dtype=np.int64)])
    lens = ptr[1:] - ptr[:-1]
    longest = 0
    short = lens < n_g                                       # such a row is its own single n-gram
    if short.any():
        longest = int((cum[ptr[1:][short]] - cum[ptr[:-1][short]]).max())
    if cp.size >= n_g:
        starts = np.arange(cp.size - n_g + 1, dtype=np.int64)
        row_end = np.repeat(ptr[1:], lens)[: starts.size]
        inside = starts + n_g <= row_end
        if inside.any():
            longest = max(longest, int((cum[n_g:] - cum[:-n_g])[inside].max()))
    return len(str(int(num_perm) - 1)) + 1 + longest


def _check_params(num_perm, ngram_size, who: str) -> Tuple[int, int]:
    for name, v in (("num_perm", num_perm), ("ngram_size", ngram_size)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{who}: {name} must be an int")
    if not 1 <= int(num_perm) <= PERM_MAX:
        raise ValueError(f"{who}: num_perm must be in [1, {PERM_MAX}]")
    if int(ngram_size) < 1:
        raise ValueError(f"{who}: ngram_size must be >= 1")
    return int(num_perm), int(ngram_size)


def signature_inputs(texts: Sequence[str], num_perm: int = 128, ngram_size: int = 3, who: str = "minhash_signatures"
                     ) -> Tuple[np.ndarray, np.ndarray]:
    """Validation and the host half of ``minhash_signatures``: the code-point CSR of ``texts`` after the check that every
    message fits one MD5 block (no GPU involved)."""
    num_perm, ngram_size = _check_params(num_perm, ngram_size, who)
    ptr, cps = code_point_csr(texts, who)
    if ptr.size - 1 >= 2 ** 31:
        raise ValueError(f"{who}: at most 2^31 - 1 texts")
    longest = longest_message_bytes(ptr, cps, ngram_size, num_perm)
    if longest > MSG_MAX:
        raise ValueError(f"{who}: the longest message (prefix, underscore and n-gram in UTF-8) has {longest} bytes, one "
                         f"MD5 block holds {MSG_MAX}: lower ngram_size (at {ngram_size} code points an n-gram can take "
                         f"{4 * ngram_size} bytes)")
    return ptr, cps


def minhash_signatures(texts: Sequence[str], num_perm: int = 128, ngram_size: int = 3, device="cuda") -> torch.Tensor:
    """MinHash signatures on the GPU (snx_minhash_signatures): ``texts`` are lowered and stripped here, then entry i of a
    row is the minimum over its character n-grams of ``int(md5(f"{i}_{ngram}".encode()).hexdigest(), 16)``
    (ref:deduplicator.py:59-82).  -> uint32 [n, num_perm, 4] on ``device``, most significant word first."""
    ptr, cps = signature_inputs(texts, num_perm, ngram_size)
    d_ptr, d_cps, dev = _text.csr_to_device(ptr, cps, device, "minhash_signatures", trusted=True)
    n = ptr.size - 1
    sig = torch.empty((n, int(num_perm), 4), dtype=torch.int32, device=dev)
    if n:
        with torch.cuda.device(dev):
            call("snx_minhash_signatures", _p(d_ptr), _p(d_cps), n, int(ngram_size), int(num_perm), _p(sig), _stream())
    return sig.view(torch.uint32)


def _signatures(signatures, who: str, dev=None) -> torch.Tensor:
    """``signatures`` [n, num_perm, 4], uint32 or int32 bit patterns, tensor on a GPU -> contiguous int32 view."""
    if not isinstance(signatures, torch.Tensor) or signatures.dim() != 3 or signatures.shape[2] != 4 or \
            signatures.dtype not in (torch.uint32, torch.int32) or signatures.device.type != "cuda" or \
            (dev is not None and signatures.device != dev):
        raise ValueError(f"{who}: signatures must be uint32 [n, num_perm, 4] on " + ("a GPU" if dev is None else str(dev)))
    if not 1 <= signatures.shape[1] <= PERM_MAX:
        raise ValueError(f"{who}: num_perm must be in [1, {PERM_MAX}]")
    s = signatures.contiguous()
    return s if s.dtype == torch.int32 else s.view(torch.int32)


def _need(need, who: str) -> int:
    if isinstance(need, bool) or not isinstance(need, (int, np.integer)) or not 0 <= int(need) < 2 ** 31:
        raise ValueError(f"{who}: need must be an int >= 0 (need_matches(num_perm, threshold))")
    return int(need)


def greedy_dedup(signatures: torch.Tensor, need: int, exact_group=None) -> torch.Tensor:
    """The reference's greedy rule on the GPU (snx_minhash_dedup): rows in order, row i is a duplicate iff an earlier KEPT
    row is in its ``exact_group`` or equals its signature at ``need`` positions or more.  ``exact_group``: int [n], the id
    in [0, n) of each row's exact key, or None.  -> duplicate_of int32 [n] on the signatures' device: -1 for a kept row,
    else the kept row of its group if there is one, else the smallest kept index that reaches ``need``."""
    sig = _signatures(signatures, "greedy_dedup")
    need = _need(need, "greedy_dedup")
    dev, (n, P, _) = sig.device, sig.shape
    if n >= 2 ** 31:
        raise ValueError("greedy_dedup: at most 2^31 - 1 rows")
    group = None
    if exact_group is not None:
        g = exact_group if isinstance(exact_group, torch.Tensor) else torch.as_tensor(np.asarray(exact_group))
        if g.dim() != 1 or g.numel() != n or g.is_floating_point() or g.dtype == torch.bool:
            raise ValueError(f"greedy_dedup: exact_group must be an int vector [{n}]")
        if n and not bool(((g >= 0) & (g < n)).all()):
            raise ValueError(f"greedy_dedup: exact_group ids must lie in [0, {n})")
        group = g.to(dev, torch.int32).contiguous()
    dup = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        ws, ws_bytes = workspace("snx_minhash_dedup_workspace_bytes", dev, int(n), int(P))
        with torch.cuda.device(dev):
            call("snx_minhash_dedup", _p(sig), int(n), int(P), min(need, 2 ** 31 - 1), _p(group), _p(dup), _p(ws),
                 ws_bytes, _stream())
    return dup


def first_match(signatures: torch.Tensor, kept: Optional[torch.Tensor], need: int) -> torch.Tensor:
    """``signatures`` [nq, num_perm, 4] against the kept signatures ``kept`` [nk, num_perm, 4] (snx_minhash_first_match)
    -> int32 [nq]: the smallest kept index whose signature reaches ``need``, -1 when none."""
    sig = _signatures(signatures, "first_match")
    need = _need(need, "first_match")
    dev, (nq, P, _) = sig.device, sig.shape
    k = None if kept is None or kept.shape[0] == 0 else _signatures(kept, "first_match", dev)
    if k is not None and k.shape[1] != P:
        raise ValueError("first_match: kept must have the signatures' num_perm")
    if nq > FIRST_MATCH_ROWS:
        raise ValueError(f"first_match: at most {FIRST_MATCH_ROWS} rows a call")
    out = torch.empty(nq, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("snx_minhash_first_match", _p(sig), int(nq), _p(k), 0 if k is None else int(k.shape[0]), int(P), need,
             _p(out), _stream())
    return out

"""Host plumbing the sections of snx.retrieval share, as plain functions: validators (``who`` is the caller's name, the
prefix of every message), the CSR normaliser, output and workspace allocation, the query slices and their step rules."""
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from .._lib import fn

K_MAX = 1024                           # top-k / band cap of every search


def cuda_device(device) -> torch.device:
    """torch.device(device); a "cuda" without an index becomes the current device."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def offsets(cnt: torch.Tensor) -> torch.Tensor:
    """Counts int64 [n] -> ptr int64 [n + 1] on the same device: 0, then the running sums."""
    ptr = torch.zeros(cnt.numel() + 1, dtype=torch.long, device=cnt.device)
    torch.cumsum(cnt, 0, out=ptr[1:])
    return ptr


def cat_or_empty(parts, dtype, device, *tail: int) -> torch.Tensor:
    """The batches of an index as one tensor; no batch: an empty [0, *tail]."""
    return torch.cat(parts) if parts else torch.zeros((0,) + tail, dtype=dtype, device=device)


def workspace(sizing: str, device, *args) -> Tuple[torch.Tensor, int]:
    """(uint8 workspace on ``device``, its size in bytes as the sizing call ``sizing(*args)`` states it); never empty."""
    ws_bytes = int(fn(sizing)(*args))
    return torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device), ws_bytes


def at(t: Optional[torch.Tensor], s: int) -> Optional[torch.Tensor]:
    """A per-query tensor from query ``s`` on; an absent one stays None (NULL in the C call)."""
    return None if t is None else t[s:]


def search_outputs(nq: int, k: int, device, with_target: bool):
    """(scores fp32 [nq, k], docs int32 [nq, k], rank int32 [nq] | None, tscore fp32 [nq] | None), uninitialised."""
    scores = torch.empty((nq, k), dtype=torch.float32, device=device)
    docs = torch.empty((nq, k), dtype=torch.int32, device=device)
    rank = torch.empty(nq, dtype=torch.int32, device=device) if with_target else None
    tscore = torch.empty(nq, dtype=torch.float32, device=device) if with_target else None
    return scores, docs, rank, tscore


def check_chunk_docs(chunk_docs: int, chunk_max: int, who: str) -> None:
    if not 0 <= chunk_docs <= chunk_max:
        raise ValueError(f"{who}: chunk_docs must be in [0, {chunk_max}] (0: default)")


def check_query_slice(query_slice, who: str) -> None:
    if isinstance(query_slice, bool) or int(query_slice) < 0:
        raise ValueError(f"{who}: query_slice must be >= 0 (0: default)")


def check_targets(targets, nq: int, nd: Optional[int], dev, who: str) -> Optional[torch.Tensor]:
    """``targets`` [nq] -> int32 contiguous (None stays None); ``nd=None``: ids are not range-checked."""
    if targets is None:
        return None
    if not isinstance(targets, torch.Tensor) or targets.device != dev or targets.dim() != 1 or \
            targets.numel() != nq or targets.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: targets must be an int tensor [{nq}] on {dev}")
    if nd is not None and nq and not bool(((targets >= 0) & (targets < nd)).all()):
        raise ValueError(f"{who}: targets must be doc ids in [0, {nd})")
    return targets.to(torch.int32).contiguous()


def check_ceiling(ceiling, nq: int, dev, who: str) -> Optional[torch.Tensor]:
    if ceiling is None:
        return None
    if not isinstance(ceiling, torch.Tensor) or ceiling.device != dev or ceiling.dtype != torch.float32 or \
            ceiling.dim() != 1 or ceiling.numel() != nq:
        raise ValueError(f"{who}: ceiling must be fp32 [{nq}] on {dev}")
    if nq and bool(torch.isnan(ceiling).any()):
        raise ValueError(f"{who}: ceiling must not be NaN (+inf: no ceiling)")
    return ceiling.contiguous()


def check_pairs(pairs, nq: int, nd: int, dev, who: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """``pairs`` int [n, 2] of (query row, doc id) -> the two columns, int32 contiguous."""
    if not isinstance(pairs, torch.Tensor) or pairs.device != dev or pairs.dim() != 2 or pairs.shape[1] != 2 or \
            pairs.is_floating_point():
        raise ValueError(f"{who}: pairs must be an int tensor [n, 2] on {dev}")
    pq, pd = pairs[:, 0], pairs[:, 1]
    if pq.numel() and not bool(((pq >= 0) & (pq < nq) & (pd >= 0) & (pd < nd)).all()):
        raise ValueError(f"{who}: pairs must be (query in [0, {nq}), doc in [0, {nd}))")
    return pq.to(torch.int32).contiguous(), pd.to(torch.int32).contiguous()


def csr_rows(rows, nq: int, nd: int, device, what: str, in_corpus: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The normaliser behind ``exclusion_csr`` (``in_corpus``: every id must lie in [0, nd)) and ``relevance_csr`` (any
    int32 id is kept, and list entries must be ints); ``what`` names the rows in the messages."""
    if isinstance(rows, tuple) and len(rows) == 2 and all(isinstance(x, torch.Tensor) for x in rows):
        ptr, docs = rows
        if ptr.dim() != 1 or docs.dim() != 1 or ptr.numel() != nq + 1 or ptr.is_floating_point() or docs.is_floating_point():
            raise ValueError(f"{what} rows: a CSR pair needs int tensors ptr [{nq + 1}] and docs [n]")
        ptr, docs = ptr.to(docs.device, torch.long), docs.long()        # normalised where the pair lives
        if int(ptr[0]) != 0 or int(ptr[-1]) != docs.numel() or bool((ptr[1:] < ptr[:-1]).any()):
            raise ValueError(f"{what} rows: ptr must start at 0, not decrease and end at len(docs)")
        row = torch.repeat_interleave(torch.arange(nq, dtype=torch.long, device=docs.device), ptr[1:] - ptr[:-1])
    else:
        if not in_corpus and (isinstance(rows, (str, bytes)) or not hasattr(rows, "__iter__")):
            raise ValueError(f"{what} rows: per-query doc-id lists or a CSR pair of tensors")
        rows = list(rows) if in_corpus else [list(r) for r in rows]
        if len(rows) != nq:
            raise ValueError(f"{what} rows: {len(rows)} rows for {nq} queries")
        lens = [len(r) for r in rows]
        if not in_corpus and any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) for r in rows for d in r):
            raise ValueError(f"{what} rows: doc ids must be ints")
        docs = torch.tensor([int(d) for r in rows for d in r], dtype=torch.long)
        row = torch.repeat_interleave(torch.arange(nq, dtype=torch.long), torch.tensor(lens, dtype=torch.long))
    # the sort key is row * span + (doc - lo): as narrow as the accepted id range [lo, hi) allows
    lo, hi, span = (0, nd, max(nd, 1)) if in_corpus else (-2 ** 31, 2 ** 31, 2 ** 32)
    if docs.numel() and not bool(((docs >= lo) & (docs < hi)).all()):
        raise ValueError(f"{what} rows: doc ids must " + (f"lie in [0, {nd})" if in_corpus else "fit in int32"))
    key = torch.unique(row * span + (docs - lo))             # sorted: by row, then doc; duplicates merged
    r, d = key // span, key % span + lo
    return offsets(torch.bincount(r, minlength=nq)).to(device), d.to(torch.int32).to(device)


def exclusion_csr(exclude, nq: int, nd: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exclusion rows -> (ptr int64 [nq+1], docs int32) on ``device``, every row sorted ascending and deduplicated.
    ``exclude``: a list of ``nq`` per-query doc-id lists, or a CSR pair, the tuple (ptr [nq+1], docs) of int tensors whose
    ptr starts at 0, does not decrease and ends at len(docs).  Every id must lie in [0, nd)."""
    return csr_rows(exclude, nq, nd, device, "exclusion", True)


def exclusion_or_null(exclude, nq: int, nd: int, device):
    """``exclude`` of a band search -> (ex_ptr, ex_doc) for the C call; no exclusion at all is (None, None)."""
    if exclude is None:
        return None, None
    ex_ptr, ex_doc = exclusion_csr(exclude, nq, nd, device)
    return (None, None) if ex_doc.numel() == 0 else (ex_ptr, ex_doc)


def slices(nq: int, step: int) -> Iterator[Tuple[int, int]]:
    """(start, rows) of the launches over ``nq`` queries: per-query tensors are passed sliced at ``start`` (see ``at``)."""
    for s in range(0, nq, step):
        yield s, min(step, nq - s)


def step_bytes_per_query(sizing: str, budget: int, nq: int, *args) -> int:
    """Queries per launch under a workspace budget, from the sizing call for ONE query."""
    per_q = max(1, int(fn(sizing)(1, *args)))
    return max(1, min(nq, budget // per_q))


def step_bytes_mean(sizing: str, budget: int, nq: int, *args) -> int:
    """Queries per launch under a workspace budget, from the sizing call for all ``nq`` queries, divided rounding up."""
    per_q = max(1, -(-int(fn(sizing)(max(nq, 1), *args)) // max(nq, 1)))
    return max(1, min(max(nq, 1), budget // per_q))


def step_blocks(budget: int, nd: int, chunk: int) -> int:
    """Queries per launch under a budget of (query, chunk) workgroups."""
    return max(1, budget // max(1, -(-nd // chunk)))

"""Exact MaxSim search over a ragged multi-vector store (csrc/mv_search.hip, include/snx.h "multi-vector search")."""
import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from .._lib import call
from ..ops import _p, _stream
from ._common import (K_MAX, at, cat_or_empty, check_pairs, check_query_slice, cuda_device, exclusion_or_null, search_outputs,
                      workspace)

MV_DIM_MAX = 1024
MV_CHUNK_MIN, MV_CHUNK_MAX = 64, 8192  # docs per chunk of the walk
_MV_ROWS_PER_LAUNCH = 1 << 15          # query rows of one launch: 512 query blocks


def _ptr_list(ptr, rows: int, who: str, name: str) -> List[int]:
    """``ptr`` [n + 1] -> host ints; it must ascend from 0 and end within ``rows``."""
    p = torch.as_tensor(ptr)
    if p.dim() != 1 or p.numel() < 1 or p.is_floating_point() or p.dtype == torch.bool:
        raise ValueError(f"{who}: {name} must be an int vector [n + 1]")
    p = [int(v) for v in p.tolist()]
    if p[0] != 0 or any(b < a for a, b in zip(p, p[1:])) or p[-1] > rows:
        raise ValueError(f"{who}: {name} must ascend from 0 and end within the rows")
    return p


class MultiVectorIndex:
    """Exact late-interaction (MaxSim) search over the multi-vector rows of a corpus on the GPU (csrc/mv_search.hip):
    which documents score best under ``snx.teacher.maxsim_pairs`` for each query, without listing the pairs.

        index = MultiVectorIndex(dim, device)
        index.add(mv, mv_ptr)          # encode_multivector's store; bf16 or fp32, one dtype per index; doc ids = order of addition
        index.build()
        scores, docs = index.search(qmv, q_ptr, k, chunk_docs=0, query_slice=0)
        scores, docs, found = index.search_band(qmv, q_ptr, lo, hi, exclude=None, chunk_docs=0, query_slice=0)
        s = index.pair_scores(qmv, q_ptr, pairs)

    s(q, d) is bit for bit ``maxsim_pairs``' score of the two sequences; the order is ``DenseIndex``'s (score descending,
    ties lowest doc id first, every document with rows a candidate whatever the sign of its score; unused slots 0 / -1).
    Results do not depend on ``chunk_docs``, ``query_slice`` or the order of the queries.  A sequence without rows (a
    text of one token) is legal as a document and is never returned; as a query it raises."""

    def __init__(self, dim: int, device):
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or not 1 <= int(dim) <= MV_DIM_MAX or dim % 64:
            raise ValueError(f"MultiVectorIndex: dim must be a multiple of 64, at most {MV_DIM_MAX}")
        self.dim = int(dim)
        self.device = torch.device(device) if torch.device(device).type != "cuda" else cuda_device(device)
        self.dtype: Optional[torch.dtype] = None
        self._parts: List[torch.Tensor] = []
        self._ptr: List[int] = [0]
        self.rows: Optional[torch.Tensor] = None
        self._hptr = None

    @property
    def num_docs(self) -> int:
        return len(self._ptr) - 1

    @property
    def num_rows(self) -> int:
        return self._ptr[-1]

    @property
    def built(self) -> bool:
        return self.rows is not None

    def _store(self, mv, ptr, who: str, name: str) -> Tuple[torch.Tensor, List[int]]:
        if not isinstance(mv, torch.Tensor) or mv.dim() != 2 or mv.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"MultiVectorIndex.{who}: {name} must be a [rows, {self.dim}] tensor of bf16 or fp32 rows")
        if mv.shape[1] != self.dim:
            raise ValueError(f"MultiVectorIndex.{who}: {name} has D = {mv.shape[1]}, the index {self.dim}")
        if self.dtype is not None and mv.dtype != self.dtype:
            raise ValueError(f"MultiVectorIndex.{who}: {name} is {mv.dtype}, the index holds {self.dtype}")
        if mv.device != self.device:
            raise ValueError(f"MultiVectorIndex.{who}: {name} must be on {self.device}")
        return mv.contiguous(), _ptr_list(ptr, int(mv.shape[0]), f"MultiVectorIndex.{who}", f"{name}_ptr")

    def add(self, mv: torch.Tensor, mv_ptr) -> None:
        mv, ptr = self._store(mv, mv_ptr, "add", "mv")
        if self.num_docs + len(ptr) - 1 >= 2 ** 31:
            raise ValueError("MultiVectorIndex: doc ids are int32")
        self.dtype = mv.dtype
        self._parts.append(mv[:ptr[-1]])
        self._ptr += [self._ptr[-1] + v for v in ptr[1:]]
        self.rows = None                                      # a new batch invalidates a built index

    def build(self) -> "MultiVectorIndex":
        if len(self._parts) != 1:
            self._parts = [cat_or_empty(self._parts, self.dtype or torch.bfloat16, self.device, self.dim)]
        self.rows = self._parts[0]
        self._hptr = (C.c_int64 * len(self._ptr))(*self._ptr)
        return self

    def _queries(self, who: str, qmv, q_ptr, chunk_docs, query_slice):
        if not self.built:
            raise RuntimeError(f"MultiVectorIndex.{who}: call build() first")
        chunk_docs = int(chunk_docs)
        if chunk_docs != 0 and not MV_CHUNK_MIN <= chunk_docs <= MV_CHUNK_MAX:
            raise ValueError(f"MultiVectorIndex.{who}: chunk_docs must be 0 (default) or in [{MV_CHUNK_MIN}, {MV_CHUNK_MAX}]")
        check_query_slice(query_slice, "MultiVectorIndex")
        if self.dtype is None:
            raise ValueError(f"MultiVectorIndex.{who}: the index is empty")
        qmv, ptr = self._store(qmv, q_ptr, who, "qmv")
        for i, (a, b) in enumerate(zip(ptr, ptr[1:])):
            if a == b:
                raise ValueError(f"MultiVectorIndex.{who}: query {i} has no multi-vector row (a text of one token)")
        if self.device.type != "cuda":
            raise ValueError(f"MultiVectorIndex.{who}: the search needs the index on a GPU")
        return qmv, ptr, chunk_docs

    def _slices(self, ptr: List[int], query_slice: int):
        """(first query, queries) per launch: at most ``query_slice`` queries (0: no limit) and about
        ``_MV_ROWS_PER_LAUNCH`` query rows; a query is never split."""
        s, nq = 0, len(ptr) - 1
        while s < nq:
            e = s + 1
            while e < nq and (not query_slice or e - s < int(query_slice)) and ptr[e + 1] - ptr[s] <= _MV_ROWS_PER_LAUNCH:
                e += 1
            yield s, e - s
            s = e

    def _run(self, qmv, ptr, ex_ptr, ex_doc, lo: int, hi: int, chunk_docs: int, query_slice: int, band: bool):
        nq, nd, dev = len(ptr) - 1, self.num_docs, self.device
        scores, docs, _, _ = search_outputs(nq, hi - lo, dev, False)
        found = torch.empty(nq, dtype=torch.int32, device=dev) if band else None
        f32 = int(self.dtype == torch.float32)
        with torch.cuda.device(dev):
            for s, m in self._slices(ptr, query_slice):
                rows = qmv[ptr[s]:ptr[s + m]]
                hq = (C.c_int64 * (m + 1))(*[v - ptr[s] for v in ptr[s:s + m + 1]])
                ws, ws_bytes = workspace("snx_mv_search_workspace_bytes", dev, hq, m, nd, self.num_rows, hi, chunk_docs)
                head = (_p(self.rows), _p(rows), f32, self.dim, self.num_rows, self._hptr, nd, int(rows.shape[0]), hq, m)
                tail = (_p(ws), ws_bytes, _stream())
                if band:
                    call("snx_mv_search_band", *head, _p(at(ex_ptr, s)), _p(ex_doc), lo, hi, chunk_docs, _p(docs[s:]),
                         _p(scores[s:]), _p(found[s:]), *tail)
                else:
                    call("snx_mv_search", *head, hi, chunk_docs, _p(docs[s:]), _p(scores[s:]), *tail)
        return scores, docs, found

    def search(self, qmv: torch.Tensor, q_ptr, k: int, chunk_docs: int = 0, query_slice: int = 0
               ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``qmv`` [qrows, dim] in the index's dtype with ``q_ptr`` [nq + 1] -> (scores [nq, k] fp32, docs [nq, k] int32):
        the top k of all documents with rows."""
        k = int(k)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"MultiVectorIndex.search: k must be in [1, {K_MAX}]")
        qmv, ptr, chunk_docs = self._queries("search", qmv, q_ptr, chunk_docs, query_slice)
        return self._run(qmv, ptr, None, None, 0, k, chunk_docs, query_slice, False)[:2]

    def search_band(self, qmv: torch.Tensor, q_ptr, lo: int, hi: int, exclude=None, chunk_docs: int = 0,
                    query_slice: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Ranks ``lo .. hi-1`` (0-based) of each query's ADMISSIBLE documents -- with rows, not in ``exclude[q]`` -> (scores
        [nq, hi-lo] fp32, docs [nq, hi-lo] int32, found [nq] int32); ``exclude`` as for ``DenseIndex.search_band``."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= K_MAX:
            raise ValueError(f"MultiVectorIndex.search_band: need 0 <= lo < hi <= {K_MAX}")
        qmv, ptr, chunk_docs = self._queries("search_band", qmv, q_ptr, chunk_docs, query_slice)
        ex_ptr, ex_doc = exclusion_or_null(exclude, len(ptr) - 1, self.num_docs, self.device)
        return self._run(qmv, ptr, ex_ptr, ex_doc, lo, hi, chunk_docs, query_slice, True)

    def pair_scores(self, qmv: torch.Tensor, q_ptr, pairs: torch.Tensor) -> torch.Tensor:
        """``pairs`` int [n, 2] of (query, doc id) -> s(q, d) fp32 [n], bit-equal to the scores the searches rank:
        ``snx.teacher.maxsim_pairs`` over the queries' rows and the rows of the documents named.  Every document named
        must have rows."""
        from ..teacher import maxsim_pairs
        qmv, ptr, _ = self._queries("pair_scores", qmv, q_ptr, 0, 0)
        nq, dev = len(ptr) - 1, self.device
        pq, pd = check_pairs(pairs, nq, self.num_docs, dev, "MultiVectorIndex.pair_scores")
        pq, pd = pq.tolist(), pd.tolist()
        ok = [i for i, d in enumerate(pd) if self._ptr[d + 1] > self._ptr[d]]     # a document without rows scores 0.0
        named = sorted({pd[i] for i in ok})
        local = {d: nq + i for i, d in enumerate(named)}
        take = [torch.arange(self._ptr[d], self._ptr[d + 1]) for d in named]
        sptr = list(ptr)
        for t in take:
            sptr.append(sptr[-1] + int(t.numel()))
        out = torch.zeros(len(pd), dtype=torch.float32, device=dev)
        if ok:
            store = torch.cat([qmv[:ptr[-1]], self.rows[torch.cat(take).to(dev)]])
            out[torch.tensor(ok, device=dev)] = maxsim_pairs(store, sptr, [pq[i] for i in ok], [local[pd[i]] for i in ok])
        return out

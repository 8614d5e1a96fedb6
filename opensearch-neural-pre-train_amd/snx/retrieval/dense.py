"""Exact inner-product search over dense fp32 embeddings (csrc/dense.hip, include/snx.h "exact dense retrieval")."""
from typing import List, Optional, Tuple

import numpy as np
import torch

from .._lib import call
from ..ops import _p, _stream
from ._common import (K_MAX, at, cat_or_empty, check_ceiling, check_pairs, check_query_slice, check_targets, cuda_device,
                      exclusion_or_null, search_outputs, slices, step_bytes_mean, workspace)

DENSE_DIM_MAX = 4096
DENSE_CHUNK_MIN = 128                  # docs per split of the dense search, at least (one tile); rounded up to a multiple
_DENSE_WS_BUDGET = 1 << 30             # bytes of dense search workspace per launch


class DenseIndex:
    """Exact inner-product search over dense fp32 embeddings on the GPU (csrc/dense.hip, include/snx.h "exact dense
    retrieval"): the reference's SemanticSearcher, its teacher scores and its dense hard-negative search, with no
    [nq, nd] score matrix.

        index = DenseIndex(dim, device)
        index.add(emb)                 # fp32 [n, dim] on the device; doc ids = order of addition
        index.build()
        scores, docs, rank, tscore = index.search(q, k, targets=None, chunk_docs=0)
        scores, docs, found = index.search_band(q, lo, hi, exclude=None, ceiling=None, chunk_docs=0)
        s = index.pair_scores(q, pairs)

    s(q, d) is the fp32 fmaf chain over the dimensions in ascending order from +0 (then + 0.0); the order is score
    descending, ties lowest doc id first, and EVERY doc is a candidate whatever the sign of its score.  Return types and
    conventions are ``SparseIndex``'s (unused slots 0 / -1); results are bit-reproducible and independent of
    ``chunk_docs`` and of how the queries are sliced.  Embeddings must be finite."""

    def __init__(self, dim: int, device):
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or not 1 <= int(dim) <= DENSE_DIM_MAX:
            raise ValueError(f"DenseIndex: dim must be an int in [1, {DENSE_DIM_MAX}]")
        self.dim = int(dim)
        self.device = cuda_device(device)
        self._parts: List[torch.Tensor] = []
        self.num_docs = 0
        self.emb: Optional[torch.Tensor] = None

    @property
    def built(self) -> bool:
        return self.emb is not None

    def _rows(self, x, who: str, name: str) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"DenseIndex.{who}: {name} must be an fp32 tensor [n, {self.dim}]")
        if x.device != self.device:
            raise ValueError(f"DenseIndex.{who}: {name} must be on {self.device}")
        if x.numel() and not bool(torch.isfinite(x).all()):
            raise ValueError(f"DenseIndex.{who}: {name} must be finite")
        return x.contiguous()

    def add(self, emb: torch.Tensor) -> None:
        e = self._rows(emb, "add", "emb")
        if self.num_docs + e.shape[0] >= 2 ** 31:
            raise ValueError("DenseIndex: doc ids are int32")
        self._parts.append(e)
        self.num_docs += int(e.shape[0])
        self.emb = None                                       # a new batch invalidates a built index

    def build(self) -> "DenseIndex":
        if len(self._parts) == 1:
            self.emb = self._parts[0]
        else:
            self.emb = cat_or_empty(self._parts, torch.float32, self.device, self.dim)
            self._parts = [self.emb]
        return self

    def _check(self, who: str, chunk_docs) -> int:
        if not self.built:
            raise RuntimeError(f"DenseIndex.{who}: call build() first")
        chunk_docs = int(chunk_docs)
        if chunk_docs != 0 and not DENSE_CHUNK_MIN <= chunk_docs < 2 ** 31:
            raise ValueError(f"DenseIndex.{who}: chunk_docs must be 0 (default) or at least {DENSE_CHUNK_MIN}")
        return chunk_docs

    def _step(self, nq: int, sizing: str, k: int, chunk_docs: int, query_slice: int) -> int:
        """Queries per launch: what the workspace budget allows, or ``query_slice`` where that is fewer."""
        check_query_slice(query_slice, "DenseIndex")
        step = step_bytes_mean(sizing, _DENSE_WS_BUDGET, nq, self.num_docs, k, chunk_docs)
        return min(step, int(query_slice)) if query_slice else step

    def search(self, q: torch.Tensor, k: int, targets: Optional[torch.Tensor] = None, chunk_docs: int = 0,
               query_slice: int = 0
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
        """``q`` fp32 [nq, dim] -> (scores [nq, k] fp32, docs [nq, k] int32, target_rank [nq] int32 | None,
        target_score [nq] fp32 | None): the top k of ALL docs; given ``targets`` [nq], each target's 1-based rank under the
        same order (always >= 1) and its score, bit-equal to the ranked value."""
        chunk_docs = self._check("search", chunk_docs)
        k = int(k)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"DenseIndex.search: k must be in [1, {K_MAX}]")
        q = self._rows(q, "search", "q")
        nq, nd, dev, sizing = int(q.shape[0]), self.num_docs, self.device, "snx_dense_search_workspace_bytes"
        tgt = check_targets(targets, nq, nd, dev, "DenseIndex.search")
        scores, docs, rank, tscore = search_outputs(nq, k, dev, tgt is not None)
        with torch.cuda.device(dev):
            for s, m in slices(nq, self._step(nq, sizing, k, chunk_docs, query_slice)):
                ws, ws_bytes = workspace(sizing, dev, m, nd, k, chunk_docs)
                call("snx_dense_search", _p(q[s:]), m, _p(self.emb), nd, self.dim, _p(at(tgt, s)), k, chunk_docs,
                     _p(docs[s:]), _p(scores[s:]), _p(at(rank, s)), _p(at(tscore, s)), _p(ws), ws_bytes, _stream())
        return scores, docs, rank, tscore

    def search_band(self, q: torch.Tensor, lo: int, hi: int, exclude=None, ceiling: Optional[torch.Tensor] = None,
                    chunk_docs: int = 0, query_slice: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Ranks ``lo .. hi-1`` (0-based) of each query's ADMISSIBLE docs -- not in ``exclude[q]``, score <
        ``ceiling[q]`` (fp32, strict; +inf: none) -- -> (scores [nq, hi-lo] fp32, docs [nq, hi-lo] int32, found [nq]
        int32); unused slots 0 / -1.  ``exclude`` and ``ceiling`` as for ``SparseIndex.search_band``."""
        chunk_docs = self._check("search_band", chunk_docs)
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= K_MAX:
            raise ValueError(f"DenseIndex.search_band: need 0 <= lo < hi <= {K_MAX}")
        q = self._rows(q, "search_band", "q")
        nq, nd, dev, sizing = int(q.shape[0]), self.num_docs, self.device, "snx_dense_search_band_workspace_bytes"
        ex_ptr, ex_doc = exclusion_or_null(exclude, nq, nd, dev)
        ceil = check_ceiling(ceiling, nq, dev, "DenseIndex.search_band")
        scores, docs, _, _ = search_outputs(nq, hi - lo, dev, False)
        found = torch.empty(nq, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            for s, m in slices(nq, self._step(nq, sizing, hi, chunk_docs, query_slice)):
                ws, ws_bytes = workspace(sizing, dev, m, nd, hi, chunk_docs)
                call("snx_dense_search_band", _p(q[s:]), m, _p(self.emb), nd, self.dim, _p(at(ex_ptr, s)), _p(ex_doc),
                     _p(at(ceil, s)), lo, hi, chunk_docs, _p(docs[s:]), _p(scores[s:]), _p(found[s:]), _p(ws), ws_bytes,
                     _stream())
        return scores, docs, found

    def pair_scores(self, q: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
        """``pairs`` int [n, 2] of (query row, doc id) -> s(q, d) fp32 [n], bit-equal to the scores the searches rank."""
        self._check("pair_scores", 0)
        q = self._rows(q, "pair_scores", "q")
        nq, nd, dev = int(q.shape[0]), self.num_docs, self.device
        pq, pd = check_pairs(pairs, nq, nd, dev, "DenseIndex.pair_scores")
        n = int(pq.numel())
        out = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("snx_dense_pair_scores", _p(q), nq, _p(self.emb), nd, self.dim, _p(pq), _p(pd), n, _p(out), _stream())
        return out

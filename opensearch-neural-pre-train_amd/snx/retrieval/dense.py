"""Exact inner-product search over dense fp32 embeddings (csrc/dense.hip, include/snx.h "exact dense retrieval"), and
the same result through a bf16 first pass with a certificate (csrc/dense_two_phase.hip, "two-phase dense retrieval")."""
import math
from typing import List, Optional, Tuple

import numpy as np
import torch

from .._lib import call
from ..ops import _p, _stream
from ._common import (K_MAX, at, cat_or_empty, check_ceiling, check_pairs, check_query_slice, check_targets, cuda_device,
                      exclusion_or_null, offsets, search_outputs, slices, step_bytes_mean, workspace)

DENSE_DIM_MAX = 4096
DENSE_CHUNK_MIN = 128                  # docs per split of the dense search, at least (one tile); rounded up to a multiple
_DENSE_WS_BUDGET = 1 << 30             # bytes of dense search workspace per launch


def bf16_rows(x: torch.Tensor):
    """fp32 rows [n, D] on the GPU -> (bits int16 [n, Dp], norm2, hat2, res2 float64 [n]) by snx_dense2_prepare: the bf16
    copy (round to nearest even, Dp = D rounded up to a multiple of 32, zero-filled) and the float64 left folds of x^2,
    xhat^2 and (x - xhat)^2 that the two-phase search's certificate is built from."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or not x.is_cuda or \
            not 1 <= x.shape[1] <= DENSE_DIM_MAX:
        raise ValueError(f"bf16_rows: x must be an fp32 tensor [n, D] on the GPU, 1 <= D <= {DENSE_DIM_MAX}")
    x = x.contiguous()
    n, dim, dev = int(x.shape[0]), int(x.shape[1]), x.device
    xb = torch.empty((n, (dim + 31) // 32 * 32), dtype=torch.int16, device=dev)
    sums = torch.empty((3, n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        call("snx_dense2_prepare", _p(x), n, dim, _p(xb), _p(sums[0]), _p(sums[1]), _p(sums[2]), _stream())
    return xb, sums[0], sums[1], sums[2]


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
        scores, docs, certified = index.search_two_phase(q, k, expansion=4.0, exact=False)
        scores, docs, found, certified = index.search_band_two_phase(q, lo, hi, exclude=None, ceiling=None, ...)
        approx, docs = index.candidates(q, k1)

    s(q, d) is the fp32 fmaf chain over the dimensions in ascending order from +0 (then + 0.0); the order is score
    descending, ties lowest doc id first, and EVERY doc is a candidate whatever the sign of its score.  Return types and
    conventions are ``SparseIndex``'s (unused slots 0 / -1); results are bit-reproducible and independent of
    ``chunk_docs`` and of how the queries are sliced.  Embeddings must be finite.  The two-phase searches
    (csrc/dense_two_phase.hip, include/snx.h "two-phase dense retrieval") scan bf16 copies of the operands on the bf16
    MFMA, score the candidates by the same chain and report per query whether the result is PROVEN to be the exact
    search's (``certified``); ``exact=True`` sends the other rows through the exact search."""

    def __init__(self, dim: int, device):
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or not 1 <= int(dim) <= DENSE_DIM_MAX:
            raise ValueError(f"DenseIndex: dim must be an int in [1, {DENSE_DIM_MAX}]")
        self.dim = int(dim)
        self.device = cuda_device(device)
        self._parts: List[torch.Tensor] = []
        self.num_docs = 0
        self.emb: Optional[torch.Tensor] = None
        self._bf16 = None                                     # search_two_phase's view of the docs, built on first use

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
        self._bf16 = None

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

    # ---- two-phase search (csrc/dense_two_phase.hip, include/snx.h "two-phase dense retrieval")
    def _two_phase_state(self):
        """The docs' bf16 copy and the maxima of their three norms, built on first use and dropped by ``add``."""
        if self._bf16 is None:
            xb, n2, h2, r2 = bf16_rows(self.emb)
            top = [float(torch.sqrt(v.max())) if self.num_docs else 0.0 for v in (n2, h2, r2)]
            self._bf16 = (xb, top[0], top[1], top[2])
        return self._bf16

    def _two_phase(self, q, k1: int, lo: int, hi: int, ex_ptr, ex_doc, ceil, chunk_docs: int,
                   query_slice: int):
        eb, dn, dh, dr = self._two_phase_state()
        nq, nd, dev, sizing = int(q.shape[0]), self.num_docs, self.device, "snx_dense2_workspace_bytes"
        scores, docs, _, _ = search_outputs(nq, hi - lo, dev, False)
        found = torch.empty(nq, dtype=torch.int32, device=dev)
        cert = torch.empty(nq, dtype=torch.uint8, device=dev)
        qb, qn2, qh2, qr2 = bf16_rows(q)
        with torch.cuda.device(dev):
            for s, m in slices(nq, self._step(nq, sizing, k1, chunk_docs, query_slice)):
                ws, ws_bytes = workspace(sizing, dev, m, nd, k1, chunk_docs)
                cand_doc = torch.empty((m, k1), dtype=torch.int32, device=dev)
                cand_approx = torch.empty((m, k1), dtype=torch.float32, device=dev)
                call("snx_dense2_scan", _p(qb[s:]), m, _p(eb), nd, self.dim, k1, chunk_docs, _p(cand_doc),
                     _p(cand_approx), _p(ws), ws_bytes, _stream())
                call("snx_dense2_rescore", _p(q[s:]), m, _p(self.emb), nd, self.dim, _p(cand_doc), _p(cand_approx), k1,
                     _p(qn2[s:]), _p(qh2[s:]), _p(qr2[s:]), dn, dh, dr, _p(at(ex_ptr, s)), _p(ex_doc), _p(at(ceil, s)),
                     lo, hi, _p(docs[s:]), _p(scores[s:]), _p(found[s:]), _p(cert[s:]), _stream())
        return scores, docs, found, cert.bool()

    @staticmethod
    def _expansion(who: str, expansion) -> float:
        expansion = float(expansion)
        if not 1.0 <= expansion < float("inf"):
            raise ValueError(f"DenseIndex.{who}: expansion must be a finite number >= 1")
        return expansion

    def candidates(self, q: torch.Tensor, k1: int, chunk_docs: int = 0, query_slice: int = 0
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Phase 1 alone: per query the ``k1`` best docs by the bf16 score -> (approx [nq, k1] fp32, docs [nq, k1]
        int32), approximate score descending, ties lowest doc id first; unused slots 0 / -1."""
        chunk_docs = self._check("candidates", chunk_docs)
        k1 = int(k1)
        if not 1 <= k1 <= K_MAX:
            raise ValueError(f"DenseIndex.candidates: k1 must be in [1, {K_MAX}]")
        q = self._rows(q, "candidates", "q")
        eb = self._two_phase_state()[0]
        nq, nd, dev, sizing = int(q.shape[0]), self.num_docs, self.device, "snx_dense2_workspace_bytes"
        approx, docs, _, _ = search_outputs(nq, k1, dev, False)
        qb = bf16_rows(q)[0]
        with torch.cuda.device(dev):
            for s, m in slices(nq, self._step(nq, sizing, k1, chunk_docs, query_slice)):
                ws, ws_bytes = workspace(sizing, dev, m, nd, k1, chunk_docs)
                call("snx_dense2_scan", _p(qb[s:]), m, _p(eb), nd, self.dim, k1, chunk_docs, _p(docs[s:]),
                     _p(approx[s:]), _p(ws), ws_bytes, _stream())
        return approx, docs

    def search_two_phase(self, q: torch.Tensor, k: int, expansion: float = 4.0, exact: bool = False,
                         chunk_docs: int = 0, query_slice: int = 0
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``search``'s top k through a bf16 first pass -> (scores [nq, k] fp32, docs [nq, k] int32, certified [nq] bool).
        Phase 1 keeps ``k1 = max(k, min(num_docs, 1024, ceil(k * expansion)))`` docs per query by the bf16 score, phase
        2 scores them by ``search``'s chain and ranks them.  A CERTIFIED row equals ``search``'s bit for bit: the norms
        of the operands prove that no doc outside the k1 could reach the k-th score.  ``exact=True`` sends the other
        rows through ``search``, so that the first two outputs equal ``search``'s on every row; ``certified`` still
        reports what phase 1 alone proved."""
        chunk_docs = self._check("search_two_phase", chunk_docs)
        k, expansion = int(k), self._expansion("search_two_phase", expansion)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"DenseIndex.search_two_phase: k must be in [1, {K_MAX}]")
        check_query_slice(query_slice, "DenseIndex")
        q = self._rows(q, "search_two_phase", "q")
        k1 = max(k, min(self.num_docs, K_MAX, math.ceil(k * expansion)))
        scores, docs, _, cert = self._two_phase(q, k1, 0, k, None, None, None, chunk_docs,
                                                query_slice)
        if exact and not bool(cert.all()):
            rows = torch.nonzero(~cert).flatten()
            s2, d2, _, _ = self.search(q[rows], k, chunk_docs=chunk_docs, query_slice=query_slice)
            scores[rows], docs[rows] = s2, d2
        return scores, docs, cert

    def search_band_two_phase(self, q: torch.Tensor, lo: int, hi: int, exclude=None,
                              ceiling: Optional[torch.Tensor] = None, expansion: float = 4.0, exact: bool = False,
                              chunk_docs: int = 0, query_slice: int = 0
                              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """``search_band`` through a bf16 first pass -> (scores, docs, found, certified [nq] bool).  Phase 1 keeps
        ``k1 = max(hi, min(num_docs, 1024, ceil((hi + longest exclusion row) * expansion)))`` docs per query; the
        exclusions and the ceiling act in phase 2, on exact scores.  Certified rows, and with ``exact=True`` all rows,
        equal ``search_band``'s bit for bit.  ``hi`` plus the longest exclusion row may not exceed 1024."""
        chunk_docs = self._check("search_band_two_phase", chunk_docs)
        lo, hi, expansion = int(lo), int(hi), self._expansion("search_band_two_phase", expansion)
        if not 0 <= lo < hi <= K_MAX:
            raise ValueError(f"DenseIndex.search_band_two_phase: need 0 <= lo < hi <= {K_MAX}")
        check_query_slice(query_slice, "DenseIndex")
        q = self._rows(q, "search_band_two_phase", "q")
        nq, nd, dev = int(q.shape[0]), self.num_docs, self.device
        ex_ptr, ex_doc = exclusion_or_null(exclude, nq, nd, dev)
        ceil = check_ceiling(ceiling, nq, dev, "DenseIndex.search_band_two_phase")
        longest = int((ex_ptr[1:] - ex_ptr[:-1]).max()) if ex_ptr is not None and nq else 0
        if hi + longest > K_MAX:
            raise ValueError(f"DenseIndex.search_band_two_phase: hi + the longest exclusion row = {hi + longest} exceeds "
                             f"{K_MAX} candidates; use search_band")
        k1 = max(hi, min(nd, K_MAX, math.ceil((hi + longest) * expansion)))
        scores, docs, found, cert = self._two_phase(q, k1, lo, hi, ex_ptr, ex_doc, ceil,
                                                    chunk_docs, query_slice)
        if exact and not bool(cert.all()):
            rows = torch.nonzero(~cert).flatten()
            sub = None
            if ex_ptr is not None:                               # the exclusion rows of `rows`, as a CSR pair
                a, n = ex_ptr[rows], ex_ptr[rows + 1] - ex_ptr[rows]
                ptr = offsets(n)
                take = torch.repeat_interleave(a - ptr[:-1], n) + torch.arange(int(ptr[-1]), device=dev)
                sub = (ptr, ex_doc[take])
            s2, d2, f2 = self.search_band(q[rows], lo, hi, exclude=sub, ceiling=None if ceil is None else ceil[rows],
                                          chunk_docs=chunk_docs, query_slice=query_slice)
            scores[rows], docs[rows], found[rows] = s2, d2, f2
        return scores, docs, found, cert

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

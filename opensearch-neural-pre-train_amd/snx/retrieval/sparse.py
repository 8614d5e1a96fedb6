"""Exact sparse search, band search and pair scores (csrc/retrieval.hip), pruning and two-phase search
(csrc/two_phase.hip) and ``SparseIndex.first_relevant`` (csrc/qrels.hip); the contracts are the sections of include/snx.h."""
from typing import Optional, Tuple

import numpy as np
import torch

from .._abi import CONSTANTS
from .._lib import call, check, fn   # the query-sliced launches go through this module's `fn`: the slicing test counts them
from ..ops import _chk, _p, _stream
from ._common import (K_MAX, at, cat_or_empty, check_ceiling, check_chunk_docs, check_pairs, check_query_slice,
                      check_targets, cuda_device, exclusion_or_null, offsets, search_outputs, slices, step_blocks,
                      step_bytes_per_query, workspace)
from .qrels import relevance_csr

CHUNK_MAX = 32768
WINDOW_MAX = 1024                      # rescore window cap
PRUNE_TYPES = {k: CONSTANTS["SNX_PRUNE_" + k.upper()] for k in ("max_ratio", "abs_value", "top_k", "alpha_mass")}
_SEARCH_WS_BUDGET = 256 << 20          # bytes of search workspace per launch: larger query sets go in slices
_FIRST_RELEVANT_BLOCKS = 1 << 21       # (query, chunk) workgroups per launch: larger query sets go in slices


def pack_rows(vals: torch.Tensor, ids: torch.Tensor, cnt: torch.Tensor, V: int, name: str = "rows"):
    """[B, cap] (values, ids, counts) rows, in any order within a row -> (counts int64 [B], terms int32 [nnz] ascending
    within each row, weights fp32 [nnz]) on the device.  Rows must hold distinct ids in [0, V) with weights > 0."""
    _chk(vals, torch.float32, f"{name}.vals")
    if vals.dim() != 2:
        raise ValueError(f"{name}: vals must be [B, cap]")
    B, cap = vals.shape
    _chk(ids, torch.int32, f"{name}.ids", (B, cap))
    _chk(cnt, torch.int32, f"{name}.cnt", (B,))
    if ids.device != vals.device or cnt.device != vals.device:
        raise ValueError(f"{name}: vals, ids and cnt must be on one device")
    c = cnt.long()
    live = torch.arange(cap, device=vals.device)[None, :] < c[:, None]
    key = torch.where(live, ids.long(), torch.full_like(ids, V, dtype=torch.long))
    skey, order = torch.sort(key, dim=1, stable=True)
    w = torch.gather(vals, 1, order)
    ok = (c >= 0).all() & (c <= cap).all()
    if B and cap:
        ok &= ((skey >= 0) & (skey < V) | ~live).all() & ((w > 0) & torch.isfinite(w) | ~live).all()
        ok &= ((skey[:, 1:] > skey[:, :-1]) | ~live[:, 1:]).all()
    if not bool(ok):
        raise ValueError(f"{name}: every row needs 0 <= cnt <= cap and cnt distinct ids in [0, {V}) with finite weights > 0")
    return c, skey[live].to(torch.int32), w[live].contiguous()


def _check_csr(cnt, terms, weights, who: str, n: str, one_gpu: bool = False) -> None:
    """A CSR triple as pack_rows returns it; ``one_gpu``: on one GPU, row count and counts within int32 (the prune kernel's)."""
    if not (isinstance(cnt, torch.Tensor) and isinstance(terms, torch.Tensor) and isinstance(weights, torch.Tensor)) or \
            cnt.dtype != torch.long or terms.dtype != torch.int32 or weights.dtype != torch.float32 or cnt.dim() != 1 or \
            terms.dim() != 1 or weights.shape != terms.shape:
        raise ValueError(f"{who}: counts int64 [{n}], terms int32 [nnz], weights fp32 [nnz]")
    if one_gpu and (not (cnt.device == terms.device == weights.device) or cnt.device.type != "cuda"):
        raise ValueError(f"{who}: the rows must live on one GPU")
    if (one_gpu and cnt.numel() >= 2 ** 31) or bool((cnt < 0).any()) or int(cnt.sum()) != terms.numel() or \
            (one_gpu and cnt.numel() and int(cnt.max()) >= 2 ** 31):
        raise ValueError(f"{who}: counts must be >= 0 and sum to nnz")


def _prune_code(prune_type, value) -> Tuple[int, float]:
    """(SNX_PRUNE_* code, the value as fp32) of a prune setting, validated as the C interface validates it."""
    if prune_type not in PRUNE_TYPES:
        raise ValueError(f"prune_type must be one of {list(PRUNE_TYPES)}, not {prune_type!r}")
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{prune_type}: the value must be a number")
    with np.errstate(over="ignore"):
        v = float(np.float32(value))
    ok = {"max_ratio": 0.0 <= v <= 1.0, "abs_value": v >= 0.0, "alpha_mass": 0.0 < v <= 1.0,
          "top_k": v >= 1.0 and v == float(value) and v == np.floor(v)}[prune_type]
    if not ok:                                                # NaN fails every comparison
        raise ValueError(f"{prune_type}: value {value!r} is outside its range (max_ratio [0, 1], abs_value >= 0, "
                         "top_k an integer >= 1, alpha_mass (0, 1])")
    return PRUNE_TYPES[prune_type], v


def _keep_flags(cnt: torch.Tensor, weights: torch.Tensor, code: int, value: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """snx_sparse_prune_rows over CSR rows -> (keep bool [nnz], kept counts int64 [n])."""
    dev, n, nnz = weights.device, int(cnt.numel()), int(weights.numel())
    ptr = offsets(cnt)
    keep = torch.empty(nnz, dtype=torch.uint8, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    longest = int(cnt.max()) if n else 0
    ws, ws_bytes = workspace("snx_sparse_prune_workspace_bytes", dev, code, n, longest)
    with torch.cuda.device(dev):
        call("snx_sparse_prune_rows", _p(ptr), _p(weights), n, nnz, longest, code, value, _p(keep), _p(kept), _p(ws),
             ws_bytes, _stream())
    return keep.bool(), kept.long()


def prune_rows(cnt: torch.Tensor, terms: torch.Tensor, weights: torch.Tensor, prune_type: str, value):
    """Prune CSR rows (the triple of ``pack_rows``: counts int64 [n], terms int32 ascending within a row, weights fp32
    > 0, on a GPU) by one of the rules of include/snx.h: ``max_ratio`` r in [0, 1] keeps w >= fp32(r) * w_max,
    ``abs_value`` a >= 0 keeps w >= fp32(a), ``top_k`` n >= 1 keeps the n heaviest (ties: lowest term), ``alpha_mass``
    alpha in (0, 1] keeps the shortest heaviest-first prefix holding the alpha share of the row's weight mass.
    -> (kept, rest): two CSR triples of the same layout, rows in place (a row may be empty in either)."""
    code, v = _prune_code(prune_type, value)
    _check_csr(cnt, terms, weights, "prune_rows", "n", one_gpu=True)
    cnt, terms, weights = cnt.contiguous(), terms.contiguous(), weights.contiguous()
    keep, kept = _keep_flags(cnt, weights, code, v)
    return (kept, terms[keep], weights[keep]), (cnt - kept, terms[~keep], weights[~keep])


def two_phase_window(k: int, expansion_rate: float, max_window_size: int) -> int:
    """W = min(floor(k * expansion_rate), max_window_size) in float64 (include/snx.h); k <= W <= 1024 or ValueError --
    the window is never clamped silently."""
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError(f"two-phase search: k must be in [1, {K_MAX}]")
    rate, cap = float(expansion_rate), float(max_window_size)
    if not rate > 0 or not np.isfinite(rate) or not cap >= 1:
        raise ValueError("two-phase search: expansion_rate must be finite and > 0, max_window_size >= 1")
    W = int(min(np.floor(np.float64(k) * np.float64(rate)), np.floor(cap)))
    if not k <= W <= WINDOW_MAX:
        raise ValueError(f"two-phase search: the window min(floor({k} * {rate}), {max_window_size}) = {W} must lie in "
                         f"[k, {WINDOW_MAX}]")
    return W


class SparseIndex:
    """Inverted index over sparse doc vectors, searched exactly on the GPU.

        index = SparseIndex(V, device)
        index.add(vals, ids, cnt)          # per batch: the [B, cap] output of ops.sparse_topk
        index.build()
        scores, docs, rank, tscore = index.search(q_vals, q_ids, q_cnt, k, targets=None)
        scores, docs, found = index.search_band(q_vals, q_ids, q_cnt, lo, hi, exclude=None, ceiling=None)
        s = index.pair_scores(q_vals, q_ids, q_cnt, pairs)

    Doc ids are the order of addition.  ``search`` returns top-k scores / doc ids [nq, k] (unused slots: 0 / -1) and,
    given ``targets`` [nq], the target's 1-based rank under the same tie order (0 = score 0, a miss) and its score."""

    def __init__(self, V: int, device):
        if int(V) <= 0:
            raise ValueError("SparseIndex: V must be positive")
        self.V = int(V)
        self.device = cuda_device(device)
        self._cnt, self._term, self._w = [], [], []          # per batch: counts int64, terms int32, weights fp32
        self.num_docs = 0
        self.doc_ptr = self.doc_term = self.doc_w = None
        self.term_ptr = self.post_doc = self.post_w = None

    @property
    def built(self) -> bool:
        return self.term_ptr is not None

    @property
    def nnz(self) -> int:
        return sum(int(t.numel()) for t in self._term)

    def _append(self, cnt: torch.Tensor, terms: torch.Tensor, weights: torch.Tensor) -> None:
        if self.num_docs + cnt.numel() >= 2 ** 31:
            raise ValueError("SparseIndex: doc ids are int32")
        self._cnt.append(cnt)
        self._term.append(terms)
        self._w.append(weights)
        self.num_docs += int(cnt.numel())
        self.term_ptr = None                                  # a new batch invalidates a built index

    def add(self, vals: torch.Tensor, ids: torch.Tensor, cnt: torch.Tensor) -> None:
        if vals.device != self.device:
            raise ValueError(f"SparseIndex.add: tensors must be on {self.device}")
        self._append(*pack_rows(vals, ids, cnt, self.V, "docs"))

    def add_csr(self, cnt: torch.Tensor, terms: torch.Tensor, weights: torch.Tensor) -> None:
        """Docs already packed as pack_rows returns them: counts int64 [B], terms int32 ascending within each row,
        weights fp32 > 0."""
        if not (cnt.device == terms.device == weights.device == self.device):
            raise ValueError(f"SparseIndex.add_csr: tensors must be on {self.device}")
        _check_csr(cnt, terms, weights, "SparseIndex.add_csr", "B")
        if terms.numel():
            row = torch.repeat_interleave(torch.arange(cnt.numel(), device=self.device), cnt)
            ok = ((terms >= 0) & (terms < self.V)).all() & ((weights > 0) & torch.isfinite(weights)).all()
            ok &= ((terms[1:] > terms[:-1]) | (row[1:] != row[:-1])).all()
            if not bool(ok):
                raise ValueError(f"SparseIndex.add_csr: rows need ascending distinct ids in [0, {self.V}) and "
                                 "finite weights > 0")
        self._append(cnt.contiguous(), terms.contiguous(), weights.contiguous())

    def build(self) -> "SparseIndex":
        dev, nd, V = self.device, self.num_docs, self.V
        cnt = cat_or_empty(self._cnt, torch.long, dev)
        self.doc_term = cat_or_empty(self._term, torch.int32, dev)
        self.doc_w = cat_or_empty(self._w, torch.float32, dev)
        self.doc_ptr = offsets(cnt)
        nnz = int(self.doc_term.numel())
        # the packed batches now live in the CSR: drop the per-batch copies, keep one list entry for further add()s
        self._cnt, self._term, self._w = [cnt], [self.doc_term], [self.doc_w]
        term_ptr = torch.empty(V + 1, dtype=torch.long, device=dev)
        post_doc = torch.empty(nnz, dtype=torch.int32, device=dev)
        post_w = torch.empty(nnz, dtype=torch.float32, device=dev)
        ws, ws_bytes = workspace("snx_sparse_index_workspace_bytes", dev, nd, V)
        with torch.cuda.device(dev):
            call("snx_sparse_index_build", _p(self.doc_ptr), _p(self.doc_term), _p(self.doc_w), nd, V, nnz,
                 _p(term_ptr), _p(post_doc), _p(post_w), _p(ws), ws_bytes, _stream())
        self.term_ptr, self.post_doc, self.post_w = term_ptr, post_doc, post_w
        return self

    def search(self, q_vals: torch.Tensor, q_ids: torch.Tensor, q_cnt: torch.Tensor, k: int,
               targets: Optional[torch.Tensor] = None, chunk_docs: int = 0
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
        """Queries as [nq, cap] rows (e.g. ops.sparse_topk with k=64: weight order; sorted by id here) ->
        (scores [nq, k] fp32, docs [nq, k] int32, target_rank [nq] int32 | None, target_score [nq] fp32 | None)."""
        if not self.built:
            raise RuntimeError("SparseIndex.search: call build() first")
        k, chunk_docs = int(k), int(chunk_docs)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"SparseIndex.search: k must be in [1, {K_MAX}]")
        check_chunk_docs(chunk_docs, CHUNK_MAX, "SparseIndex.search")
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "search")
        tgt = check_targets(targets, nq, self.num_docs, self.device, "SparseIndex.search")
        return self._search_csr(q_ptr, q_term, q_w, nq, k, tgt, chunk_docs)

    def _search_csr(self, q_ptr, q_term, q_w, nq: int, k: int, tgt, chunk_docs: int, query_slice: int = 0):
        """snx_sparse_search over query rows already in CSR form, in slices of the workspace budget (or of
        ``query_slice`` queries); the slicing changes no bit."""
        dev, nd, sizing = self.device, self.num_docs, "snx_sparse_search_workspace_bytes"
        scores, docs, rank, tscore = search_outputs(nq, k, dev, tgt is not None)
        step = step_bytes_per_query(sizing, _SEARCH_WS_BUDGET, nq, nd, k, chunk_docs)
        if query_slice:
            step = min(step, int(query_slice))
        with torch.cuda.device(dev):
            for s, m in slices(nq, step):
                ws, ws_bytes = workspace(sizing, dev, m, nd, k, chunk_docs)
                check(fn("snx_sparse_search")(
                    _p(q_ptr[s:]), _p(q_term), _p(q_w), m, _p(self.term_ptr), _p(self.post_doc), _p(self.post_w),
                    _p(self.doc_ptr), _p(self.doc_term), _p(self.doc_w), nd, self.V, _p(at(tgt, s)), k, chunk_docs,
                    _p(docs[s:]), _p(scores[s:]), _p(at(rank, s)), _p(at(tscore, s)), _p(ws), ws_bytes, _stream()),
                    "snx_sparse_search")
        return scores, docs, rank, tscore

    def search_csr(self, cnt: torch.Tensor, terms: torch.Tensor, weights: torch.Tensor, k: int,
                   targets: Optional[torch.Tensor] = None, chunk_docs: int = 0):
        """``search`` for queries already packed as ``add_csr`` takes docs (counts int64 [nq], terms int32 ascending
        within each row, weights fp32 > 0, on the index's device): the same four results, the same bits."""
        if not self.built:
            raise RuntimeError("SparseIndex.search_csr: call build() first")
        k, chunk_docs = int(k), int(chunk_docs)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"SparseIndex.search_csr: k must be in [1, {K_MAX}]")
        check_chunk_docs(chunk_docs, CHUNK_MAX, "SparseIndex.search_csr")
        if not (cnt.device == terms.device == weights.device == self.device):
            raise ValueError(f"SparseIndex.search_csr: tensors must be on {self.device}")
        _check_csr(cnt, terms, weights, "SparseIndex.search_csr", "nq")
        if terms.numel():
            row = torch.repeat_interleave(torch.arange(cnt.numel(), device=self.device), cnt)
            ok = ((terms >= 0) & (terms < self.V)).all() & ((weights > 0) & torch.isfinite(weights)).all()
            ok &= ((terms[1:] > terms[:-1]) | (row[1:] != row[:-1])).all()
            if not bool(ok):
                raise ValueError(f"SparseIndex.search_csr: rows need ascending distinct ids in [0, {self.V}) and "
                                 "finite weights > 0")
        nq = int(cnt.numel())
        tgt = check_targets(targets, nq, self.num_docs, self.device, "SparseIndex.search_csr")
        return self._search_csr(offsets(cnt), terms.contiguous(), weights.contiguous(), nq, k, tgt, chunk_docs)

    def _queries(self, q_vals, q_ids, q_cnt, who: str):
        if not self.built:
            raise RuntimeError(f"SparseIndex.{who}: call build() first")
        if q_vals.device != self.device:
            raise ValueError(f"SparseIndex.{who}: tensors must be on {self.device}")
        qc, q_term, q_w = pack_rows(q_vals, q_ids, q_cnt, self.V, "queries")
        return int(qc.numel()), offsets(qc), q_term, q_w

    def pair_scores(self, q_vals: torch.Tensor, q_ids: torch.Tensor, q_cnt: torch.Tensor,
                    pairs: torch.Tensor) -> torch.Tensor:
        """``pairs`` int [n, 2] of (query row, doc id) -> s(q, d) fp32 [n], bit-equal to the scores the searches rank."""
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "pair_scores")
        nd, dev = self.num_docs, self.device
        pq, pd = check_pairs(pairs, nq, nd, dev, "SparseIndex.pair_scores")
        n = int(pq.numel())
        out = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("snx_sparse_pair_scores", _p(q_ptr), _p(q_term), _p(q_w), nq, _p(self.doc_ptr), _p(self.doc_term),
                 _p(self.doc_w), nd, _p(pq), _p(pd), n, _p(out), _stream())
        return out

    def search_band(self, q_vals: torch.Tensor, q_ids: torch.Tensor, q_cnt: torch.Tensor, lo: int, hi: int,
                    exclude=None, ceiling: Optional[torch.Tensor] = None, chunk_docs: int = 0
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Ranks ``lo .. hi-1`` (0-based) of each query's ADMISSIBLE docs -- score > 0, not in ``exclude[q]``, score <
        ``ceiling[q]`` (fp32, strict; +inf: none) -- under (score desc, doc asc) -> (scores [nq, hi-lo] fp32, docs
        [nq, hi-lo] int32, found [nq] int32); unused slots 0 / -1.  ``exclude``: None, per-query doc-id lists, or a CSR
        pair (see exclusion_csr); ``ceiling``: None or fp32 [nq] on the index's device."""
        lo, hi, chunk_docs = int(lo), int(hi), int(chunk_docs)
        if not 0 <= lo < hi <= K_MAX:
            raise ValueError(f"SparseIndex.search_band: need 0 <= lo < hi <= {K_MAX}")
        check_chunk_docs(chunk_docs, CHUNK_MAX, "SparseIndex.search_band")
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "search_band")
        dev, nd, sizing = self.device, self.num_docs, "snx_sparse_search_band_workspace_bytes"
        ex_ptr, ex_doc = exclusion_or_null(exclude, nq, nd, dev)
        ceil = check_ceiling(ceiling, nq, dev, "SparseIndex.search_band")
        scores, docs, _, _ = search_outputs(nq, hi - lo, dev, False)
        found = torch.empty(nq, dtype=torch.int32, device=dev)
        step = step_bytes_per_query(sizing, _SEARCH_WS_BUDGET, nq, nd, hi, chunk_docs)
        with torch.cuda.device(dev):
            for s, m in slices(nq, step):
                ws, ws_bytes = workspace(sizing, dev, m, nd, hi, chunk_docs)
                check(fn("snx_sparse_search_band")(
                    _p(q_ptr[s:]), _p(q_term), _p(q_w), m, _p(self.term_ptr), _p(self.post_doc), _p(self.post_w), nd,
                    self.V, _p(at(ex_ptr, s)), _p(ex_doc), _p(at(ceil, s)), lo, hi, chunk_docs, _p(docs[s:]),
                    _p(scores[s:]), _p(found[s:]), _p(ws), ws_bytes, _stream()), "snx_sparse_search_band")
        return scores, docs, found

    def pruned(self, prune_type: str, value) -> "SparseIndex":
        """Ingest-time pruning: a new built index over this index's doc rows pruned by ``prune_rows``' rule, with the
        same doc ids (a doc pruned to nothing stays as an empty row).  This index is left untouched."""
        code, v = _prune_code(prune_type, value)
        if not self.built:
            raise RuntimeError("SparseIndex.pruned: call build() first")
        cnt = self.doc_ptr[1:] - self.doc_ptr[:-1]
        keep, kept = _keep_flags(cnt, self.doc_w, code, v)
        out = SparseIndex(self.V, self.device)
        out._append(kept, self.doc_term[keep], self.doc_w[keep])
        return out.build()

    def rescore(self, q_vals: torch.Tensor, q_ids: torch.Tensor, q_cnt: torch.Tensor, cand_docs: torch.Tensor, k: int,
                targets: Optional[torch.Tensor] = None, query_slice: int = 0
                ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
        """``cand_docs`` int32 [nq, W] (1 <= W <= 1024; -1: unused slot): every candidate scored with the exact s(q, d),
        the top ``k`` <= W of those with s > 0 in search order, a repeated doc counted once -> (scores [nq, k] fp32,
        docs [nq, k] int32 (unused: 0 / -1), rank [nq] int32 | None (the target's 1-based position in the output, 0 =
        absent), tscore [nq] fp32 | None).  ``query_slice``: queries per launch (0: all); it changes no bit."""
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "rescore")
        dev = self.device
        if not isinstance(cand_docs, torch.Tensor) or cand_docs.device != dev or cand_docs.dtype != torch.int32 or \
                cand_docs.dim() != 2 or cand_docs.shape[0] != nq:
            raise ValueError(f"SparseIndex.rescore: cand_docs must be int32 [{nq}, W] on {dev}")
        W, k = int(cand_docs.shape[1]), int(k)
        if not 1 <= W <= WINDOW_MAX or not 1 <= k <= W:
            raise ValueError(f"SparseIndex.rescore: need 1 <= k <= W <= {WINDOW_MAX}")
        tgt = check_targets(targets, nq, self.num_docs, dev, "SparseIndex.rescore")
        return self._rescore_csr(q_ptr, q_term, q_w, nq, cand_docs.contiguous(), k, tgt, query_slice)

    def _rescore_csr(self, q_ptr, q_term, q_w, nq: int, cand: torch.Tensor, k: int, tgt, query_slice: int = 0):
        dev, W = self.device, int(cand.shape[1])
        check_query_slice(query_slice, "SparseIndex")
        scores, docs, rank, tscore = search_outputs(nq, k, dev, tgt is not None)
        with torch.cuda.device(dev):
            for s, m in slices(nq, int(query_slice) or max(nq, 1)):
                call("snx_sparse_rescore", _p(q_ptr[s:]), _p(q_term), _p(q_w), m, _p(cand[s:]), W, _p(self.doc_ptr),
                     _p(self.doc_term), _p(self.doc_w), self.num_docs, _p(at(tgt, s)), k, _p(docs[s:]), _p(scores[s:]),
                     _p(at(rank, s)), _p(at(tscore, s)), _stream())
        return scores, docs, rank, tscore

    def search_two_phase(self, q_vals: torch.Tensor, q_ids: torch.Tensor, q_cnt: torch.Tensor, k: int,
                         prune_type: str = "max_ratio", prune_value=0.4, expansion_rate: float = 5.0,
                         max_window_size: int = 10000, targets: Optional[torch.Tensor] = None, chunk_docs: int = 0,
                         query_slice: int = 0):
        """Two-phase search (include/snx.h; OpenSearch's neural_sparse_two_phase_processor, defaults the reference's
        ref:benchmark/index_manager.py:197-238): phase 1 is ``search`` with only the query entries kept by the prune
        (Q_high) and k = W = min(floor(k * expansion_rate), max_window_size) -- ValueError unless k <= W <= 1024 --;
        phase 2 rescores that window with the full query.  Every returned score is the exact s(q, d); a doc that matches
        only dropped query terms is never found.  -> (scores [nq, k], docs [nq, k], rank | None (position in the output,
        0 = absent), tscore | None, stats {"postings_high", "postings_all", "window_filled"} -> int64 [nq]: posting-list
        lengths under the Q_high terms and under all query terms, and the docs phase 1 found).  ``chunk_docs`` and
        ``query_slice`` change no bit."""
        code, v = _prune_code(prune_type, prune_value)
        W = two_phase_window(k, expansion_rate, max_window_size)
        k, chunk_docs = int(k), int(chunk_docs)
        check_chunk_docs(chunk_docs, CHUNK_MAX, "SparseIndex.search_two_phase")
        check_query_slice(query_slice, "SparseIndex.search_two_phase")
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "search_two_phase")
        dev = self.device
        tgt = check_targets(targets, nq, self.num_docs, dev, "SparseIndex.search_two_phase")
        qc = q_ptr[1:] - q_ptr[:-1]
        keep, high_cnt = _keep_flags(qc, q_w, code, v)
        _, window, _, _ = self._search_csr(offsets(high_cnt), q_term[keep], q_w[keep], nq, W, None, chunk_docs,
                                           query_slice)
        scores, docs, rank, tscore = self._rescore_csr(q_ptr, q_term, q_w, nq, window, k, tgt, query_slice)
        lens = (self.term_ptr[1:] - self.term_ptr[:-1])[q_term.long()]
        row = torch.repeat_interleave(torch.arange(nq, device=dev), qc)
        zero = torch.zeros(nq, dtype=torch.long, device=dev)
        stats = {"postings_high": zero.index_add(0, row[keep], lens[keep]), "postings_all": zero.index_add(0, row, lens),
                 "window_filled": (window >= 0).sum(1)}
        return scores, docs, rank, tscore, stats

    def first_relevant(self, q_vals: torch.Tensor, q_ids: torch.Tensor, q_cnt: torch.Tensor, relevant, chunk_docs: int = 0
                           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The best relevant doc of every query and its rank in the WHOLE corpus (snx_sparse_first_relevant): ``relevant``
        as ``relevance_csr`` takes it.  -> (doc int32 [nq]: the row member with the highest s(q, d) > 0, ties lowest id, -1 =
        none; score fp32 [nq]: bit-equal to the ranked value; rank int32 [nq]: 1 + the docs in front of it under the
        search's order, 0 = no relevant doc scores -- the minimum over the row of ``search(targets=d)``'s rank, at the cost of
        one scoring pass; nrel int32 [nq]: row members in [0, num_docs)).  ``chunk_docs`` changes no bit."""
        chunk_docs = int(chunk_docs)
        check_chunk_docs(chunk_docs, CHUNK_MAX, "SparseIndex.first_relevant")
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "first_relevant")
        dev, nd = self.device, self.num_docs
        rel_ptr, rel_doc = relevance_csr(relevant, nq, nd, dev)
        doc, rank, nrel = (torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(3))
        score = torch.empty(nq, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            for s, m in slices(nq, step_blocks(_FIRST_RELEVANT_BLOCKS, nd, chunk_docs or 16384)):
                ws, ws_bytes = workspace("snx_sparse_first_relevant_workspace_bytes", dev, m, nd, chunk_docs)
                check(fn("snx_sparse_first_relevant")(
                    _p(q_ptr[s:]), _p(q_term), _p(q_w), m, _p(self.term_ptr), _p(self.post_doc), _p(self.post_w),
                    _p(self.doc_ptr), _p(self.doc_term), _p(self.doc_w), nd, self.V, _p(rel_ptr[s:]), _p(rel_doc),
                    chunk_docs, _p(doc[s:]), _p(score[s:]), _p(rank[s:]), _p(nrel[s:]), _p(ws), ws_bytes, _stream()),
                    "snx_sparse_first_relevant")
        return doc, score, rank, nrel

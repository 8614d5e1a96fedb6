"""Exact sparse retrieval on the GPU (csrc/retrieval.hip, include/snx.h "exact sparse retrieval").

``SparseIndex`` is the inverted index of the mid-training evaluator: the reference hands indexing and search to an
OpenSearch cluster (ref:benchmark/indexer.py, ref:benchmark/searchers.py:155-188); here the doc vectors are packed on the
device batch by batch from the ``[B, cap]`` output of ``ops.sparse_topk`` (no ``[nd, V]`` buffer ever exists), a
term-major index is built by a deterministic counting sort, and every query is scored exactly against every doc:

    s(q, d) = fmaf over the shared terms in ascending term id, fp32, starting at +0  (the plain dot product)

then ranked score descending, ties lowest doc id first.  Results are bit-reproducible and independent of
``chunk_docs``.  ``search_band`` and ``pair_scores`` serve the hard-negative miner (src.train.mining): a rank band of the
ADMISSIBLE docs (score > 0, not in the query's exclusion row, score < the query's ceiling) and s(q, d) of given pairs,
bit-equal to the ranked values.  ``SeismicIndex`` is the approximate SEISMIC search over a built ``SparseIndex``
(csrc/seismic.hip, include/snx.h "SEISMIC").  ``prune_rows``, ``SparseIndex.pruned``, ``SparseIndex.rescore`` and
``SparseIndex.search_two_phase`` are the prune rules and the two-phase search of the reference's ``rank_features``
serving path (csrc/two_phase.hip, include/snx.h "pruning and two-phase search").  ``term_counts``, ``Bm25Index`` and
``fuse_ranked`` are the lexical BM25 baseline under the model's tokenizer and the rank fusion of the reference's hybrid
searchers (csrc/hybrid.hip, include/snx.h "BM25 baseline and rank fusion").  ``relevance_csr``,
``SparseIndex.first_relevant``, ``ranked_relevance`` and ``bootstrap_means`` score any of these searches against qrels with
several relevant docs per query (csrc/qrels.hip, include/snx.h "relevance judgments").  ``DenseIndex`` is the exact
inner-product search over dense fp32 embeddings (csrc/dense.hip, include/snx.h "exact dense retrieval")."""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ._lib import check, fn
from .ops import _chk, _p, _stream

K_MAX = 1024
CHUNK_MAX = 32768
_SEARCH_WS_BUDGET = 256 << 20          # bytes of search workspace per launch: larger query sets go in slices


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


PRUNE_TYPES = {"max_ratio": 0, "abs_value": 1, "top_k": 2, "alpha_mass": 3}       # SNX_PRUNE_* of include/snx.h
WINDOW_MAX = 1024                      # rescore window cap


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
    ptr = torch.zeros(n + 1, dtype=torch.long, device=dev)
    torch.cumsum(cnt, 0, out=ptr[1:])
    keep = torch.empty(nnz, dtype=torch.uint8, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    longest = int(cnt.max()) if n else 0
    ws_bytes = int(fn("snx_sparse_prune_workspace_bytes")(code, n, longest))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(fn("snx_sparse_prune_rows")(_p(ptr), _p(weights), n, nnz, longest, code, value, _p(keep), _p(kept),
                                           _p(ws), ws_bytes, _stream()), "snx_sparse_prune_rows")
    return keep.bool(), kept.long()


def prune_rows(cnt: torch.Tensor, terms: torch.Tensor, weights: torch.Tensor, prune_type: str, value):
    """Prune CSR rows (the triple of ``pack_rows``: counts int64 [n], terms int32 ascending within a row, weights fp32
    > 0, on a GPU) by one of the rules of include/snx.h: ``max_ratio`` r in [0, 1] keeps w >= fp32(r) * w_max,
    ``abs_value`` a >= 0 keeps w >= fp32(a), ``top_k`` n >= 1 keeps the n heaviest (ties: lowest term), ``alpha_mass``
    alpha in (0, 1] keeps the shortest heaviest-first prefix holding the alpha share of the row's weight mass.
    -> (kept, rest): two CSR triples of the same layout, rows in place (a row may be empty in either)."""
    code, v = _prune_code(prune_type, value)
    if not (isinstance(cnt, torch.Tensor) and isinstance(terms, torch.Tensor) and isinstance(weights, torch.Tensor)) or \
            cnt.dtype != torch.long or terms.dtype != torch.int32 or weights.dtype != torch.float32 or cnt.dim() != 1 or \
            terms.dim() != 1 or weights.shape != terms.shape:
        raise ValueError("prune_rows: counts int64 [n], terms int32 [nnz], weights fp32 [nnz]")
    if not (cnt.device == terms.device == weights.device) or cnt.device.type != "cuda":
        raise ValueError("prune_rows: the rows must live on one GPU")
    if cnt.numel() >= 2 ** 31 or bool((cnt < 0).any()) or int(cnt.sum()) != terms.numel() or \
            (cnt.numel() and int(cnt.max()) >= 2 ** 31):
        raise ValueError("prune_rows: counts must be >= 0 and sum to nnz")
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


def exclusion_csr(exclude, nq: int, nd: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exclusion rows -> (ptr int64 [nq+1], docs int32) on ``device``, every row sorted ascending and deduplicated.
    ``exclude``: a list of ``nq`` per-query doc-id lists, or a CSR pair, the tuple (ptr [nq+1], docs) of int tensors whose
    ptr starts at 0, does not decrease and ends at len(docs).  Every id must lie in [0, nd)."""
    if isinstance(exclude, tuple) and len(exclude) == 2 and all(isinstance(x, torch.Tensor) for x in exclude):
        ptr, docs = exclude
        if ptr.dim() != 1 or docs.dim() != 1 or ptr.numel() != nq + 1 or ptr.is_floating_point() or \
                docs.is_floating_point():
            raise ValueError(f"exclusion rows: a CSR pair needs int tensors ptr [{nq + 1}] and docs [n]")
        ptr, docs = ptr.to(docs.device, torch.long), docs.long()        # normalised where the pair lives
        if int(ptr[0]) != 0 or int(ptr[-1]) != docs.numel() or bool((ptr[1:] < ptr[:-1]).any()):
            raise ValueError("exclusion rows: ptr must start at 0, not decrease and end at len(docs)")
        row = torch.repeat_interleave(torch.arange(nq, dtype=torch.long, device=docs.device), ptr[1:] - ptr[:-1])
    else:
        rows = list(exclude)
        if len(rows) != nq:
            raise ValueError(f"exclusion rows: {len(rows)} rows for {nq} queries")
        lens = [len(r) for r in rows]
        docs = torch.tensor([int(d) for r in rows for d in r], dtype=torch.long)
        row = torch.repeat_interleave(torch.arange(nq, dtype=torch.long), torch.tensor(lens, dtype=torch.long))
    if docs.numel() and not bool(((docs >= 0) & (docs < nd)).all()):
        raise ValueError(f"exclusion rows: doc ids must lie in [0, {nd})")
    key = torch.unique(row * max(nd, 1) + docs)             # sorted: by row, then doc; duplicates merged
    r, d = key // max(nd, 1), key % max(nd, 1)
    ptr = torch.zeros(nq + 1, dtype=torch.long, device=key.device)
    torch.cumsum(torch.bincount(r, minlength=nq), 0, out=ptr[1:])
    return ptr.to(device), d.to(torch.int32).to(device)


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
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._cnt: List[torch.Tensor] = []
        self._term: List[torch.Tensor] = []
        self._w: List[torch.Tensor] = []
        self.num_docs = 0
        self.doc_ptr = self.doc_term = self.doc_w = None
        self.term_ptr = self.post_doc = self.post_w = None

    @property
    def built(self) -> bool:
        return self.term_ptr is not None

    @property
    def nnz(self) -> int:
        return sum(int(t.numel()) for t in self._term)

    def add(self, vals: torch.Tensor, ids: torch.Tensor, cnt: torch.Tensor) -> None:
        if vals.device != self.device:
            raise ValueError(f"SparseIndex.add: tensors must be on {self.device}")
        c, t, w = pack_rows(vals, ids, cnt, self.V, "docs")
        if self.num_docs + c.numel() >= 2 ** 31:
            raise ValueError("SparseIndex: doc ids are int32")
        self._cnt.append(c)
        self._term.append(t)
        self._w.append(w)
        self.num_docs += int(c.numel())
        self.term_ptr = None                                  # a new batch invalidates a built index

    def add_csr(self, cnt: torch.Tensor, terms: torch.Tensor, weights: torch.Tensor) -> None:
        """Docs already packed as pack_rows returns them: counts int64 [B], terms int32 ascending within each row,
        weights fp32 > 0."""
        if not (cnt.device == terms.device == weights.device == self.device):
            raise ValueError(f"SparseIndex.add_csr: tensors must be on {self.device}")
        if cnt.dtype != torch.long or terms.dtype != torch.int32 or weights.dtype != torch.float32 or cnt.dim() != 1 or \
                terms.dim() != 1 or weights.shape != terms.shape:
            raise ValueError("SparseIndex.add_csr: counts int64 [B], terms int32 [nnz], weights fp32 [nnz]")
        if (cnt < 0).any() or int(cnt.sum()) != terms.numel():
            raise ValueError("SparseIndex.add_csr: counts must be >= 0 and sum to nnz")
        if terms.numel():
            row = torch.repeat_interleave(torch.arange(cnt.numel(), device=self.device), cnt)
            ok = ((terms >= 0) & (terms < self.V)).all() & ((weights > 0) & torch.isfinite(weights)).all()
            ok &= ((terms[1:] > terms[:-1]) | (row[1:] != row[:-1])).all()
            if not bool(ok):
                raise ValueError(f"SparseIndex.add_csr: rows need ascending distinct ids in [0, {self.V}) and "
                                 "finite weights > 0")
        if self.num_docs + cnt.numel() >= 2 ** 31:
            raise ValueError("SparseIndex: doc ids are int32")
        self._cnt.append(cnt.contiguous())
        self._term.append(terms.contiguous())
        self._w.append(weights.contiguous())
        self.num_docs += int(cnt.numel())
        self.term_ptr = None

    def build(self) -> "SparseIndex":
        dev, nd, V = self.device, self.num_docs, self.V
        cnt = torch.cat(self._cnt) if self._cnt else torch.zeros(0, dtype=torch.long, device=dev)
        self.doc_term = torch.cat(self._term) if self._term else torch.zeros(0, dtype=torch.int32, device=dev)
        self.doc_w = torch.cat(self._w) if self._w else torch.zeros(0, dtype=torch.float32, device=dev)
        self.doc_ptr = torch.zeros(nd + 1, dtype=torch.long, device=dev)
        torch.cumsum(cnt, 0, out=self.doc_ptr[1:])
        nnz = int(self.doc_term.numel())
        # the packed batches now live in the CSR: drop the per-batch copies, keep one list entry for further add()s
        self._cnt, self._term, self._w = [cnt], [self.doc_term], [self.doc_w]
        term_ptr = torch.empty(V + 1, dtype=torch.long, device=dev)
        post_doc = torch.empty(nnz, dtype=torch.int32, device=dev)
        post_w = torch.empty(nnz, dtype=torch.float32, device=dev)
        ws_bytes = int(fn("snx_sparse_index_workspace_bytes")(nd, V))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(fn("snx_sparse_index_build")(_p(self.doc_ptr), _p(self.doc_term), _p(self.doc_w), nd, V, nnz,
                                                _p(term_ptr), _p(post_doc), _p(post_w), _p(ws), ws_bytes, _stream()),
                  "snx_sparse_index_build")
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
        if not 0 <= chunk_docs <= CHUNK_MAX:
            raise ValueError(f"SparseIndex.search: chunk_docs must be in [0, {CHUNK_MAX}] (0: default)")
        if q_vals.device != self.device:
            raise ValueError(f"SparseIndex.search: tensors must be on {self.device}")
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "search")
        tgt = self._targets(targets, nq, "search")
        return self._search_csr(q_ptr, q_term, q_w, nq, k, tgt, chunk_docs)

    def _targets(self, targets, nq: int, who: str) -> Optional[torch.Tensor]:
        if targets is None:
            return None
        dev, nd = self.device, self.num_docs
        if not isinstance(targets, torch.Tensor) or targets.device != dev or targets.dim() != 1 or \
                targets.numel() != nq or targets.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"SparseIndex.{who}: targets must be an int tensor [{nq}] on {dev}")
        if nq and not bool(((targets >= 0) & (targets < nd)).all()):
            raise ValueError(f"SparseIndex.{who}: targets must be doc ids in [0, {nd})")
        return targets.to(torch.int32).contiguous()

    def _search_csr(self, q_ptr, q_term, q_w, nq: int, k: int, tgt, chunk_docs: int, query_slice: int = 0):
        """snx_sparse_search over query rows already in CSR form, in slices of the workspace budget (or of
        ``query_slice`` queries); the slicing changes no bit."""
        dev, nd = self.device, self.num_docs
        scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        docs = torch.empty((nq, k), dtype=torch.int32, device=dev)
        rank = torch.empty(nq, dtype=torch.int32, device=dev) if tgt is not None else None
        tscore = torch.empty(nq, dtype=torch.float32, device=dev) if tgt is not None else None
        per_q = max(1, int(fn("snx_sparse_search_workspace_bytes")(1, nd, k, chunk_docs)))
        step = max(1, min(nq, _SEARCH_WS_BUDGET // per_q))
        if query_slice:
            step = min(step, int(query_slice))
        with torch.cuda.device(dev):
            for s in range(0, nq, step):
                m = min(step, nq - s)
                ws_bytes = int(fn("snx_sparse_search_workspace_bytes")(m, nd, k, chunk_docs))
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
                check(fn("snx_sparse_search")(
                    _p(q_ptr[s:]), _p(q_term), _p(q_w), m, _p(self.term_ptr), _p(self.post_doc), _p(self.post_w),
                    _p(self.doc_ptr), _p(self.doc_term), _p(self.doc_w), nd, self.V,
                    _p(None if tgt is None else tgt[s:]), k, chunk_docs, _p(docs[s:]), _p(scores[s:]),
                    _p(None if rank is None else rank[s:]), _p(None if tscore is None else tscore[s:]), _p(ws), ws_bytes,
                    _stream()), "snx_sparse_search")
        return scores, docs, rank, tscore

    def _queries(self, q_vals, q_ids, q_cnt, who: str):
        if not self.built:
            raise RuntimeError(f"SparseIndex.{who}: call build() first")
        if q_vals.device != self.device:
            raise ValueError(f"SparseIndex.{who}: tensors must be on {self.device}")
        qc, q_term, q_w = pack_rows(q_vals, q_ids, q_cnt, self.V, "queries")
        q_ptr = torch.zeros(qc.numel() + 1, dtype=torch.long, device=self.device)
        torch.cumsum(qc, 0, out=q_ptr[1:])
        return int(qc.numel()), q_ptr, q_term, q_w

    def pair_scores(self, q_vals: torch.Tensor, q_ids: torch.Tensor, q_cnt: torch.Tensor,
                    pairs: torch.Tensor) -> torch.Tensor:
        """``pairs`` int [n, 2] of (query row, doc id) -> s(q, d) fp32 [n], bit-equal to the scores the searches rank."""
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "pair_scores")
        nd, dev = self.num_docs, self.device
        if not isinstance(pairs, torch.Tensor) or pairs.device != dev or pairs.dim() != 2 or pairs.shape[1] != 2 or \
                pairs.is_floating_point():
            raise ValueError(f"SparseIndex.pair_scores: pairs must be an int tensor [n, 2] on {dev}")
        n = int(pairs.shape[0])
        if n and not bool(((pairs[:, 0] >= 0) & (pairs[:, 0] < nq) & (pairs[:, 1] >= 0) & (pairs[:, 1] < nd)).all()):
            raise ValueError(f"SparseIndex.pair_scores: pairs must be (query in [0, {nq}), doc in [0, {nd}))")
        pq = pairs[:, 0].to(torch.int32).contiguous()
        pd = pairs[:, 1].to(torch.int32).contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(fn("snx_sparse_pair_scores")(_p(q_ptr), _p(q_term), _p(q_w), nq, _p(self.doc_ptr), _p(self.doc_term),
                                                _p(self.doc_w), nd, _p(pq), _p(pd), n, _p(out), _stream()),
                  "snx_sparse_pair_scores")
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
        if not 0 <= chunk_docs <= CHUNK_MAX:
            raise ValueError(f"SparseIndex.search_band: chunk_docs must be in [0, {CHUNK_MAX}] (0: default)")
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "search_band")
        dev, nd = self.device, self.num_docs
        ex_ptr = ex_doc = None
        if exclude is not None:
            ex_ptr, ex_doc = exclusion_csr(exclude, nq, nd, dev)
            if ex_doc.numel() == 0:
                ex_ptr = ex_doc = None
        ceil = None
        if ceiling is not None:
            if not isinstance(ceiling, torch.Tensor) or ceiling.device != dev or ceiling.dtype != torch.float32 or \
                    ceiling.dim() != 1 or ceiling.numel() != nq:
                raise ValueError(f"SparseIndex.search_band: ceiling must be fp32 [{nq}] on {dev}")
            if nq and bool(torch.isnan(ceiling).any()):
                raise ValueError("SparseIndex.search_band: ceiling must not be NaN (+inf: no ceiling)")
            ceil = ceiling.contiguous()
        w = hi - lo
        scores = torch.empty((nq, w), dtype=torch.float32, device=dev)
        docs = torch.empty((nq, w), dtype=torch.int32, device=dev)
        found = torch.empty(nq, dtype=torch.int32, device=dev)
        per_q = max(1, int(fn("snx_sparse_search_band_workspace_bytes")(1, nd, hi, chunk_docs)))
        step = max(1, min(nq, _SEARCH_WS_BUDGET // per_q))
        with torch.cuda.device(dev):
            for s in range(0, nq, step):
                m = min(step, nq - s)
                ws_bytes = int(fn("snx_sparse_search_band_workspace_bytes")(m, nd, hi, chunk_docs))
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
                check(fn("snx_sparse_search_band")(
                    _p(q_ptr[s:]), _p(q_term), _p(q_w), m, _p(self.term_ptr), _p(self.post_doc), _p(self.post_w), nd,
                    self.V, _p(None if ex_ptr is None else ex_ptr[s:]), _p(ex_doc), _p(None if ceil is None else ceil[s:]),
                    lo, hi, chunk_docs, _p(docs[s:]), _p(scores[s:]), _p(found[s:]), _p(ws), ws_bytes, _stream()),
                    "snx_sparse_search_band")
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
        out._cnt, out._term, out._w = [kept], [self.doc_term[keep]], [self.doc_w[keep]]
        out.num_docs = self.num_docs
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
        tgt = self._targets(targets, nq, "rescore")
        return self._rescore_csr(q_ptr, q_term, q_w, nq, cand_docs.contiguous(), k, tgt, query_slice)

    def _rescore_csr(self, q_ptr, q_term, q_w, nq: int, cand: torch.Tensor, k: int, tgt, query_slice: int = 0):
        dev, W = self.device, int(cand.shape[1])
        if isinstance(query_slice, bool) or int(query_slice) < 0:
            raise ValueError("SparseIndex: query_slice must be >= 0 (0: default)")
        scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        docs = torch.empty((nq, k), dtype=torch.int32, device=dev)
        rank = torch.empty(nq, dtype=torch.int32, device=dev) if tgt is not None else None
        tscore = torch.empty(nq, dtype=torch.float32, device=dev) if tgt is not None else None
        step = int(query_slice) or max(nq, 1)
        with torch.cuda.device(dev):
            for s in range(0, nq, step):
                m = min(step, nq - s)
                check(fn("snx_sparse_rescore")(
                    _p(q_ptr[s:]), _p(q_term), _p(q_w), m, _p(cand[s:]), W, _p(self.doc_ptr), _p(self.doc_term),
                    _p(self.doc_w), self.num_docs, _p(None if tgt is None else tgt[s:]), k, _p(docs[s:]),
                    _p(scores[s:]), _p(None if rank is None else rank[s:]),
                    _p(None if tscore is None else tscore[s:]), _stream()), "snx_sparse_rescore")
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
        if not 0 <= chunk_docs <= CHUNK_MAX:
            raise ValueError(f"SparseIndex.search_two_phase: chunk_docs must be in [0, {CHUNK_MAX}] (0: default)")
        if isinstance(query_slice, bool) or int(query_slice) < 0:
            raise ValueError("SparseIndex.search_two_phase: query_slice must be >= 0 (0: default)")
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "search_two_phase")
        tgt = self._targets(targets, nq, "search_two_phase")
        dev = self.device
        qc = q_ptr[1:] - q_ptr[:-1]
        keep, high_cnt = _keep_flags(qc, q_w, code, v)
        h_ptr = torch.zeros(nq + 1, dtype=torch.long, device=dev)
        torch.cumsum(high_cnt, 0, out=h_ptr[1:])
        _, window, _, _ = self._search_csr(h_ptr, q_term[keep], q_w[keep], nq, W, None, chunk_docs, query_slice)
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
        if not 0 <= chunk_docs <= CHUNK_MAX:
            raise ValueError(f"SparseIndex.first_relevant: chunk_docs must be in [0, {CHUNK_MAX}] (0: default)")
        nq, q_ptr, q_term, q_w = self._queries(q_vals, q_ids, q_cnt, "first_relevant")
        dev, nd = self.device, self.num_docs
        rel_ptr, rel_doc = relevance_csr(relevant, nq, nd, dev)
        doc = torch.empty(nq, dtype=torch.int32, device=dev)
        score = torch.empty(nq, dtype=torch.float32, device=dev)
        rank = torch.empty(nq, dtype=torch.int32, device=dev)
        nrel = torch.empty(nq, dtype=torch.int32, device=dev)
        chunk = chunk_docs or 16384
        step = max(1, _FIRST_RELEVANT_BLOCKS // max(1, -(-nd // chunk)))
        with torch.cuda.device(dev):
            for s in range(0, nq, step):
                m = min(step, nq - s)
                ws_bytes = int(fn("snx_sparse_first_relevant_workspace_bytes")(m, nd, chunk_docs))
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
                check(fn("snx_sparse_first_relevant")(
                    _p(q_ptr[s:]), _p(q_term), _p(q_w), m, _p(self.term_ptr), _p(self.post_doc), _p(self.post_w),
                    _p(self.doc_ptr), _p(self.doc_term), _p(self.doc_w), nd, self.V, _p(rel_ptr[s:]), _p(rel_doc),
                    chunk_docs, _p(doc[s:]), _p(score[s:]), _p(rank[s:]), _p(nrel[s:]), _p(ws), ws_bytes, _stream()),
                    "snx_sparse_first_relevant")
        return doc, score, rank, nrel


SEISMIC_Q_MAX = 1024                   # query nnz cap of the SEISMIC search (the query lives in LDS)
_SEISMIC_QUERY_SLICE = 1 << 20         # queries per search launch (one workgroup each)


def _positive_int(x, name: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < 1:
        raise ValueError(f"SeismicIndex: {name} must be an int >= 1")
    return int(x)


class SeismicIndex:
    """SEISMIC approximate search (Bruch et al., SIGIR 2024) over a built ``SparseIndex``, on the GPU.

        six = SeismicIndex(index, n_postings=300, cluster_ratio=0.1, summary_prune_ratio=0.4)
        scores, docs, rank, tscore, stats = six.search(q_vals, q_ids, q_cnt, k, top_n=10, heap_factor=1.0, targets=None)

    The definition (include/snx.h "SEISMIC") is a deterministic form of the published algorithm under OpenSearch's
    parameter names: per term the ``n_postings`` heaviest postings, ``ceil(cluster_ratio * n)`` blocks around evenly
    spaced centroids, and block summaries keeping the ``summary_prune_ratio`` share of their weight mass; a query visits
    its ``top_n`` heaviest terms and skips a block when ``heap_factor * s(q, summary)`` falls below its running k-th
    score.  Centroids are chosen deterministically, summaries stay fp32 (no quantization) and there is one index per
    corpus (no Lucene segments), so OpenSearch's own numbers are not reproduced.  Every returned score is the exact s(q, d)
    of ``SparseIndex`` bit for bit.  The index defaults are the reference's (ref:scripts/neural_sparse_search_aws.py
    :1326-1329, the model card's mapping); the query defaults ``top_n=10, heap_factor=1.0`` are OpenSearch's documented
    ones, not checked against a cluster here.  The term-major lists and doc CSR of ``index`` are used in place."""

    def __init__(self, index: "SparseIndex", n_postings: int = 300, cluster_ratio: float = 0.1,
                 summary_prune_ratio: float = 0.4):
        if not isinstance(index, SparseIndex) or not index.built:
            raise ValueError("SeismicIndex: needs a built SparseIndex")
        if index.device.type != "cuda":
            raise ValueError("SeismicIndex: the index must live on a GPU")
        self.n_postings = _positive_int(n_postings, "n_postings")
        if self.n_postings >= 2 ** 31:
            raise ValueError("SeismicIndex: n_postings must fit in int32")
        self.cluster_ratio, self.summary_prune_ratio = float(cluster_ratio), float(summary_prune_ratio)
        if not 0.0 < self.cluster_ratio <= 1.0:
            raise ValueError("SeismicIndex: cluster_ratio must lie in (0, 1]")
        if not 0.0 < self.summary_prune_ratio <= 1.0 or not np.float32(self.summary_prune_ratio) > 0:
            raise ValueError("SeismicIndex: summary_prune_ratio must lie in (0, 1]")
        self.index = index
        dev, V, nd = index.device, index.V, index.num_docs
        t0 = time.perf_counter()
        with torch.cuda.device(dev):
            lens = torch.clamp(index.term_ptr[1:] - index.term_ptr[:-1], max=self.n_postings)
            self.prune_ptr = torch.zeros(V + 1, dtype=torch.long, device=dev)
            torch.cumsum(lens, 0, out=self.prune_ptr[1:])
            p = lens.cpu().numpy().astype(np.float64)          # cluster counts in float64 on the host (the contract)
            c = np.where(p > 0, np.minimum(p, np.maximum(1.0, np.ceil(self.cluster_ratio * p))), 0.0).astype(np.int32)
            cent_cnt = torch.from_numpy(c).to(dev)
            self.cent_ptr = torch.zeros(V + 1, dtype=torch.long, device=dev)
            torch.cumsum(cent_cnt.long(), 0, out=self.cent_ptr[1:])
            P, C = int(self.prune_ptr[-1]), int(self.cent_ptr[-1])
            self.prune_doc = torch.empty(P, dtype=torch.int32, device=dev)
            self.prune_w = torch.empty(P, dtype=torch.float32, device=dev)
            self.cent_doc = torch.empty(C, dtype=torch.int32, device=dev)
            assign = torch.empty(P, dtype=torch.int32, device=dev)
            cent_size = torch.zeros(C, dtype=torch.int32, device=dev)
            check(fn("snx_seismic_build_clusters")(
                _p(index.term_ptr), _p(index.post_doc), _p(index.post_w), _p(index.doc_ptr), _p(index.doc_term),
                _p(index.doc_w), nd, V, self.n_postings, _p(self.prune_ptr), _p(cent_cnt), _p(self.cent_ptr), P, C,
                _p(self.prune_doc), _p(self.prune_w), _p(self.cent_doc), _p(assign), _p(cent_size), _stream()),
                "snx_seismic_build_clusters")
            cursor = torch.zeros(C + 1, dtype=torch.long, device=dev)   # block start of every centroid (empty: no room)
            torch.cumsum(cent_size.long(), 0, out=cursor[1:])
            self.blk_doc = torch.empty(P, dtype=torch.int32, device=dev)
            check(fn("snx_seismic_build_blocks")(_p(self.prune_ptr), _p(self.prune_doc), _p(assign), _p(self.cent_ptr),
                                                  V, P, _p(cursor), _p(self.blk_doc), _stream()),
                  "snx_seismic_build_blocks")
            live = cent_size > 0
            nb = int(live.sum())
            self.blk_ptr = torch.zeros(nb + 1, dtype=torch.long, device=dev)
            torch.cumsum(cent_size[live].long(), 0, out=self.blk_ptr[1:])
            term_of = torch.repeat_interleave(torch.arange(V, device=dev), cent_cnt.long())
            self.term_blk_ptr = torch.zeros(V + 1, dtype=torch.long, device=dev)
            torch.cumsum(torch.bincount(term_of[live], minlength=V), 0, out=self.term_blk_ptr[1:])
            self.blk_cent = (torch.arange(C, device=dev) - self.cent_ptr[term_of])[live].to(torch.int32)
            ws_bytes = int(fn("snx_seismic_build_workspace_bytes")(V, nb))
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            sum_cnt = torch.empty(nb, dtype=torch.int32, device=dev)
            summaries = fn("snx_seismic_build_summaries")
            alpha = float(np.float32(self.summary_prune_ratio))
            check(summaries(_p(index.doc_ptr), _p(index.doc_term), _p(index.doc_w), nd, V, _p(self.blk_ptr),
                            _p(self.blk_doc), nb, alpha, None, _p(sum_cnt), None, None, _p(ws), ws_bytes, _stream()),
                  "snx_seismic_build_summaries")
            self.sum_ptr = torch.zeros(nb + 1, dtype=torch.long, device=dev)
            torch.cumsum(sum_cnt.long(), 0, out=self.sum_ptr[1:])
            S = int(self.sum_ptr[-1])
            self.sum_term = torch.empty(S, dtype=torch.int32, device=dev)
            self.sum_w = torch.empty(S, dtype=torch.float32, device=dev)
            check(summaries(_p(index.doc_ptr), _p(index.doc_term), _p(index.doc_w), nd, V, _p(self.blk_ptr),
                            _p(self.blk_doc), nb, alpha, _p(self.sum_ptr), _p(sum_cnt), _p(self.sum_term),
                            _p(self.sum_w), _p(ws), ws_bytes, _stream()), "snx_seismic_build_summaries")
            torch.cuda.synchronize(dev)
        self.build_seconds = time.perf_counter() - t0

    @property
    def num_blocks(self) -> int:
        return int(self.blk_ptr.numel()) - 1

    @property
    def summary_nnz(self) -> int:
        return int(self.sum_term.numel())

    def structure(self) -> Dict[str, torch.Tensor]:
        """CPU copies of the build: ``prune_ptr`` [V+1] / ``prune_doc`` / ``prune_w`` (each term's kept postings in doc
        order), ``cent_ptr`` [V+1] / ``cent_doc`` (centroid j of term t at cent_ptr[t] + j), ``term_blk_ptr`` [V+1] /
        ``blk_cent`` (the centroid index of each block within its term), ``blk_ptr`` [nb+1] / ``blk_doc`` (each block's
        docs ascending), ``sum_ptr`` [nb+1] / ``sum_term`` / ``sum_w`` (each summary in ascending term id)."""
        keys = ("prune_ptr", "prune_doc", "prune_w", "cent_ptr", "cent_doc", "term_blk_ptr", "blk_cent", "blk_ptr",
                "blk_doc", "sum_ptr", "sum_term", "sum_w")
        return {k: getattr(self, k).cpu() for k in keys}

    def search(self, q_vals: torch.Tensor, q_ids: torch.Tensor, q_cnt: torch.Tensor, k: int, top_n: int = 10,
               heap_factor: float = 1.0, targets: Optional[torch.Tensor] = None, query_slice: int = 0
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor],
                          Dict[str, torch.Tensor]]:
        """Queries as [nq, cap] rows (as ``SparseIndex.search`` takes them; at most 1024 terms per row) ->
        (scores [nq, k] fp32, docs [nq, k] int32 (unused: 0 / -1), rank [nq] int32 | None (1-based position of the target
        in the output, 0 = absent), tscore [nq] fp32 | None (s(q, target)), stats: {"blocks_total", "blocks_scored",
        "postings_scored"} -> int64 [nq]).  ``query_slice``: queries per launch (0: default); it changes no bit."""
        idx = self.index
        k = int(k)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"SeismicIndex.search: k must be in [1, {K_MAX}]")
        top_n = _positive_int(top_n, "top_n")
        hf = float(heap_factor)
        if not hf > 0 or not np.float32(hf) > 0:
            raise ValueError("SeismicIndex.search: heap_factor must be > 0 (+inf allowed)")
        if isinstance(query_slice, bool) or int(query_slice) < 0:
            raise ValueError("SeismicIndex.search: query_slice must be >= 0 (0: default)")
        dev, V, nd = idx.device, idx.V, idx.num_docs
        if not isinstance(q_vals, torch.Tensor) or q_vals.device != dev:
            raise ValueError(f"SeismicIndex.search: tensors must be on {dev}")
        qc, q_term, q_w = pack_rows(q_vals, q_ids, q_cnt, V, "queries")
        nq = int(qc.numel())
        max_nnz = int(qc.max()) if nq else 0
        if max_nnz > SEISMIC_Q_MAX:
            raise ValueError(f"SeismicIndex.search: a query holds {max_nnz} terms; the cap is {SEISMIC_Q_MAX}")
        q_ptr = torch.zeros(nq + 1, dtype=torch.long, device=dev)
        torch.cumsum(qc, 0, out=q_ptr[1:])
        tgt = None
        if targets is not None:
            if not isinstance(targets, torch.Tensor) or targets.device != dev or targets.dim() != 1 or \
                    targets.numel() != nq or targets.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"SeismicIndex.search: targets must be an int tensor [{nq}] on {dev}")
            if nq and not bool(((targets >= 0) & (targets < nd)).all()):
                raise ValueError(f"SeismicIndex.search: targets must be doc ids in [0, {nd})")
            tgt = targets.to(torch.int32).contiguous()
        scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        docs = torch.empty((nq, k), dtype=torch.int32, device=dev)
        rank = torch.empty(nq, dtype=torch.int32, device=dev) if tgt is not None else None
        tscore = torch.empty(nq, dtype=torch.float32, device=dev) if tgt is not None else None
        stats = torch.empty((nq, 3), dtype=torch.long, device=dev)
        step = int(query_slice) or _SEISMIC_QUERY_SLICE
        with torch.cuda.device(dev):
            for s in range(0, nq, step):
                m = min(step, nq - s)
                check(fn("snx_seismic_search")(
                    _p(q_ptr[s:]), _p(q_term), _p(q_w), m, max_nnz, _p(self.term_blk_ptr), _p(self.blk_ptr),
                    _p(self.blk_doc), _p(self.sum_ptr), _p(self.sum_term), _p(self.sum_w), _p(idx.doc_ptr),
                    _p(idx.doc_term), _p(idx.doc_w), nd, V, _p(None if tgt is None else tgt[s:]), k, top_n, hf,
                    _p(docs[s:]), _p(scores[s:]), _p(None if rank is None else rank[s:]),
                    _p(None if tscore is None else tscore[s:]), _p(stats[s:]), _stream()), "snx_seismic_search")
        return scores, docs, rank, tscore, {"blocks_total": stats[:, 0], "blocks_scored": stats[:, 1],
                                            "postings_scored": stats[:, 2]}


# ------------------------------------------------------------------------------------------------ BM25 and rank fusion
FUSE_METHODS = {"rrf": 0, "weighted_rrf": 1, "linear": 2}                         # SNX_FUSE_* of include/snx.h
FUSE_L_MAX = 4
FUSE_TOP_K_MAX = 4096


def term_counts_max_len() -> int:
    """The longest row ``term_counts`` takes (the model's position limit)."""
    return int(fn("snx_term_counts_max_len")())


def term_counts(input_ids: torch.Tensor, attention_mask: torch.Tensor, allowed: torch.Tensor):
    """Lexical term counts of token rows on the GPU (snx_term_counts): ``input_ids`` / ``attention_mask`` [n, S] int as
    the tokenizer yields them, ``allowed`` [V] uint8 (benchmark.encoders.allowed_token_mask).  A position counts when its
    mask is non-zero, 0 <= id < V and allowed[id] != 0.  -> (term [n, S] int32: the distinct counted ids ascending, unused
    slots -1; tf [n, S] int32: their counts, unused 0; cnt [n] int32: distinct ids; length [n] int32: counted positions).
    (tf.float(), term, cnt) is a row triple for ``pack_rows``."""
    if not (isinstance(input_ids, torch.Tensor) and isinstance(attention_mask, torch.Tensor) and
            isinstance(allowed, torch.Tensor)) or input_ids.dim() != 2 or attention_mask.shape != input_ids.shape or \
            input_ids.is_floating_point() or attention_mask.is_floating_point():
        raise ValueError("term_counts: input_ids and attention_mask must be int tensors [n, S] of one shape")
    dev = input_ids.device
    if dev.type != "cuda" or attention_mask.device != dev or allowed.device != dev:
        raise ValueError("term_counts: input_ids, attention_mask and allowed must live on one GPU")
    _chk(allowed, torch.uint8, "allowed")
    if allowed.dim() != 1 or allowed.numel() < 1:
        raise ValueError("term_counts: allowed must be uint8 [V]")
    n, S = int(input_ids.shape[0]), int(input_ids.shape[1])
    if not 1 <= S <= term_counts_max_len():
        raise ValueError(f"term_counts: rows of {S} positions; the supported length is 1 .. {term_counts_max_len()}")
    ids = input_ids.to(torch.long).contiguous()
    mask = attention_mask.to(torch.long).contiguous()
    term = torch.empty((n, S), dtype=torch.int32, device=dev)
    tf = torch.empty((n, S), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    length = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(fn("snx_term_counts")(_p(ids), _p(mask), _p(allowed), n, S, int(allowed.numel()), _p(term), _p(tf), _p(cnt),
                                    _p(length), _stream()), "snx_term_counts")
    return term, tf, cnt, length


def bm25_idf(doc_freq, num_docs: int) -> np.ndarray:
    """idf [V] float64 on the host: numpy.log1p((N - df + 0.5) / (df + 0.5)) (include/snx.h; the `bm25` smoothing of
    ref:tools/idf-compute/src/main.rs:202, Lucene's form)."""
    df = np.asarray(doc_freq, np.float64)
    return np.log1p((np.float64(num_docs) - df + 0.5) / (df + 0.5))


class Bm25Index:
    """BM25 over token ids, on the GPU: the lexical baseline of the reference's benchmark under the model's own tokenizer.

        bm = Bm25Index(V, device, k1=1.2, b=0.75)
        bm.add_tokens(input_ids, attention_mask, allowed)      # per batch of tokenized docs
        bm.build()
        scores, docs, rank, tscore = bm.search_tokens(input_ids, attention_mask, allowed, k, targets=None)

    ``build`` turns the accumulated term counts into the weights of include/snx.h ("BM25 baseline and rank fusion":
    w = idf * tf / (tf + k1 * (1 - b + b * dl / avgdl)) in float64, rounded to fp32) and builds an ordinary
    ``SparseIndex`` over them, ``.index``: ``search_band``, ``pruned``, ``search_two_phase`` and ``SeismicIndex(bm.index)``
    work over BM25 weights as they are.  A query row weighs each term fp32(count), and the BM25 score is the exact index's
    s(q, d) -- bit-reproducible, ties lowest doc id first, ``rank`` / ``tscore`` for targets.  Not OpenSearch's BM25: no
    (k1 + 1) factor (as in Lucene >= 8), no one-byte length norms, the model's tokenizer instead of `nori`, lengths after
    the caller's truncation.  ``doc_freq`` [V] int32, ``doc_len`` [N] int32, ``idf`` [V] float64 and ``avgdl`` are exposed."""

    def __init__(self, V: int, device, k1: float = 1.2, b: float = 0.75):
        if int(V) <= 0:
            raise ValueError("Bm25Index: V must be positive")
        self.k1, self.b = float(k1), float(b)
        if not (self.k1 >= 0 and np.isfinite(self.k1)) or not 0.0 <= self.b <= 1.0:
            raise ValueError("Bm25Index: k1 must be finite and >= 0, b must lie in [0, 1]")
        self.V = int(V)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._cnt: List[torch.Tensor] = []
        self._term: List[torch.Tensor] = []
        self._tf: List[torch.Tensor] = []
        self._len: List[torch.Tensor] = []
        self.num_docs = 0
        self.doc_freq = torch.zeros(self.V, dtype=torch.int32, device=self.device)
        self.doc_len = self.idf = self.avgdl = self.index = None

    @property
    def built(self) -> bool:
        return self.index is not None

    def _allowed(self, allowed) -> torch.Tensor:
        if not isinstance(allowed, torch.Tensor) or allowed.dim() != 1 or allowed.numel() != self.V:
            raise ValueError(f"Bm25Index: allowed must be uint8 [{self.V}]")
        return allowed

    def add_tokens(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, allowed: torch.Tensor) -> None:
        if not isinstance(input_ids, torch.Tensor) or input_ids.device != self.device:
            raise ValueError(f"Bm25Index.add_tokens: tensors must be on {self.device}")
        term, tf, cnt, length = term_counts(input_ids, attention_mask, self._allowed(allowed))
        if self.num_docs + cnt.numel() >= 2 ** 31:
            raise ValueError("Bm25Index: doc ids are int32")
        live = torch.arange(term.shape[1], device=self.device)[None, :] < cnt[:, None]
        terms = term[live].contiguous()
        with torch.cuda.device(self.device):
            check(fn("snx_bm25_doc_freq")(_p(terms), int(terms.numel()), self.V, _p(self.doc_freq), _stream()),
                  "snx_bm25_doc_freq")
        self._cnt.append(cnt.long())
        self._term.append(terms)
        self._tf.append(tf[live].contiguous())
        self._len.append(length)
        self.num_docs += int(cnt.numel())
        self.index = None                                     # a new batch invalidates a built index

    def build(self) -> "Bm25Index":
        dev, N, V = self.device, self.num_docs, self.V
        cnt = torch.cat(self._cnt) if self._cnt else torch.zeros(0, dtype=torch.long, device=dev)
        terms = torch.cat(self._term) if self._term else torch.zeros(0, dtype=torch.int32, device=dev)
        tf = torch.cat(self._tf) if self._tf else torch.zeros(0, dtype=torch.int32, device=dev)
        self.doc_len = torch.cat(self._len) if self._len else torch.zeros(0, dtype=torch.int32, device=dev)
        self._cnt, self._term, self._tf, self._len = [cnt], [terms], [tf], [self.doc_len]
        idf = bm25_idf(self.doc_freq.cpu().numpy(), N)        # the log on the host: V entries, one libm
        total = int(self.doc_len.long().sum())                # exact integer sum
        self.avgdl = float(np.float64(total) / np.float64(N)) if N else 0.0
        self.idf = torch.from_numpy(idf).to(dev)
        ptr = torch.zeros(N + 1, dtype=torch.long, device=dev)
        torch.cumsum(cnt, 0, out=ptr[1:])
        w = torch.empty(terms.numel(), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(fn("snx_bm25_weights")(_p(ptr), _p(terms), _p(tf), _p(self.doc_len), _p(self.idf), N,
                                         int(terms.numel()), V, self.avgdl, self.k1, self.b, _p(w), _stream()),
                  "snx_bm25_weights")
        index = SparseIndex(V, dev)
        index.add_csr(cnt, terms, w)
        self.index = index.build()
        return self

    def search_tokens(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, allowed: torch.Tensor, k: int,
                      targets: Optional[torch.Tensor] = None):
        """Tokenized queries -> what ``SparseIndex.search`` returns: (scores [nq, k] fp32, docs [nq, k] int32, rank |
        None, tscore | None).  A repeated query term counts as often as it occurs; terms no doc holds are legal."""
        if not self.built:
            raise RuntimeError("Bm25Index.search_tokens: call build() first")
        return self.index.search(*self.query_rows(input_ids, attention_mask, allowed), k, targets=targets)

    def query_rows(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, allowed: torch.Tensor):
        """Tokenized queries -> the (vals, ids, cnt) rows every search of ``.index`` takes: weights fp32(count)."""
        if not isinstance(input_ids, torch.Tensor) or input_ids.device != self.device:
            raise ValueError(f"Bm25Index: tensors must be on {self.device}")
        term, tf, cnt, _ = term_counts(input_ids, attention_mask, self._allowed(allowed))
        return tf.float(), term, cnt


def fuse_ranked(lists, method: str, top_k: int, targets: Optional[torch.Tensor] = None, **params):
    """Fuse ``L`` <= 4 ranked lists per query on the GPU (snx_fuse_ranked; the rules of ref:benchmark/score_fusion.py and
    the triple RRF of ref:benchmark/hybrid_searcher.py:501-522, bit for bit in float64).  ``lists``: a sequence of (docs
    int32 [nq, R], scores fp32 [nq, R]) pairs as the searches return them (R <= 1024; a list ends at its first negative
    doc id; doc ids distinct within a list).  ``method`` and its ``params``: "rrf" (k=60), "weighted_rrf" (k=60,
    weights=one per list, (0.4, 0.6) for two lists), "linear" (alpha=0.4, two lists, list 0 weighted by alpha).
    -> (scores float64 [nq, top_k], docs int32 [nq, top_k] (unused: 0 / -1), rank int32 [nq] | None (the target's 1-based
    position in the whole fused order, 0 = in no list), total int32 [nq] (the size of the union)).  Order: fused score
    descending, ties lowest doc id first."""
    if method not in FUSE_METHODS:
        raise ValueError(f"Unknown fusion method: {method}. Choose from {list(FUSE_METHODS)}")
    lists = list(lists)
    L = len(lists)
    if not 1 <= L <= FUSE_L_MAX:
        raise ValueError(f"fuse_ranked: 1 .. {FUSE_L_MAX} lists, not {L}")
    known = {"rrf": ("k",), "weighted_rrf": ("k", "weights"), "linear": ("alpha",)}[method]
    bad = set(params) - set(known)
    if bad:
        raise ValueError(f"fuse_ranked: {method} takes {known}, not {sorted(bad)}")
    if method == "linear":
        if L != 2:
            raise ValueError("fuse_ranked: linear fusion takes exactly two lists")
        alpha = float(params.get("alpha", 0.4))
        if not 0 <= alpha <= 1:
            raise ValueError("alpha must be between 0 and 1")
        prm = [alpha]
    else:
        k = float(params.get("k", 60))
        if not (k >= 0 and np.isfinite(k)):
            raise ValueError("fuse_ranked: k must be finite and >= 0")
        prm = [k]
        if method == "weighted_rrf":
            weights = params.get("weights", (0.4, 0.6) if L == 2 else None)
            if weights is None or len(weights) != L or not all(np.isfinite(float(x)) for x in weights):
                raise ValueError(f"fuse_ranked: weighted_rrf needs {L} finite weights")
            prm += [float(x) for x in weights]
    top_k = int(top_k)
    if not 1 <= top_k <= FUSE_TOP_K_MAX:
        raise ValueError(f"fuse_ranked: top_k must be in [1, {FUSE_TOP_K_MAX}]")
    d0 = lists[0][0]
    if not isinstance(d0, torch.Tensor) or d0.dim() != 2 or d0.device.type != "cuda":
        raise ValueError("fuse_ranked: lists are (docs int32 [nq, R], scores fp32 [nq, R]) pairs on a GPU")
    dev, (nq, R) = d0.device, d0.shape
    if not 1 <= R <= K_MAX:
        raise ValueError(f"fuse_ranked: lists of 1 .. {K_MAX} entries")
    for d, s in lists:
        if not (isinstance(d, torch.Tensor) and isinstance(s, torch.Tensor)) or d.dtype != torch.int32 or \
                s.dtype != torch.float32 or d.shape != (nq, R) or s.shape != (nq, R) or d.device != dev or s.device != dev:
            raise ValueError(f"fuse_ranked: every list is (docs int32, scores fp32) of shape [{nq}, {R}] on {dev}")
    docs = torch.stack([d for d, _ in lists]).contiguous()
    scores = torch.stack([s for _, s in lists]).contiguous()
    tgt = None
    if targets is not None:
        if not isinstance(targets, torch.Tensor) or targets.device != dev or targets.dim() != 1 or \
                targets.numel() != nq or targets.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"fuse_ranked: targets must be an int tensor [{nq}] on {dev}")
        tgt = targets.to(torch.int32).contiguous()
    out_s = torch.empty((nq, top_k), dtype=torch.float64, device=dev)
    out_d = torch.empty((nq, top_k), dtype=torch.int32, device=dev)
    total = torch.empty(nq, dtype=torch.int32, device=dev)
    rank = torch.empty(nq, dtype=torch.int32, device=dev) if tgt is not None else None
    import ctypes as C
    host = (C.c_double * len(prm))(*prm)
    with torch.cuda.device(dev):
        check(fn("snx_fuse_ranked")(_p(docs), _p(scores), L, int(nq), int(R), FUSE_METHODS[method],
                                    C.cast(host, C.c_void_p), _p(tgt), top_k, _p(out_d), _p(out_s), _p(total), _p(rank),
                                    _stream()), "snx_fuse_ranked")
    return out_s, out_d, rank, total


# ------------------------------------------------------------------------------------------------ relevance judgments
RANKED_R_MAX = 4096
CUTOFFS_MAX = 8
BOOTSTRAP_M_MAX = 16
BOOTSTRAP_SEGMENT = 64                 # SNX_BOOTSTRAP_SEGMENT of include/snx.h: part of the summation order
_FIRST_RELEVANT_BLOCKS = 1 << 21       # (query, chunk) workgroups per launch: larger query sets go in slices


def relevance_csr(relevant, nq: int, nd: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Relevance rows (qrels) -> (ptr int64 [nq+1], docs int32) on ``device``, every row sorted ascending and
    deduplicated.  ``relevant`` takes the two forms of ``exclusion_csr``: a list of ``nq`` per-query doc-id lists, or a
    CSR pair, the tuple (ptr [nq+1], docs) of int tensors whose ptr starts at 0, does not decrease and ends at len(docs).
    Unlike an exclusion row a relevance row may name ids outside [0, nd) (a judged doc that is not in the corpus): they
    stay in the row and the kernels skip them (include/snx.h "relevance judgments").  Ids must fit in int32."""
    nq, nd = int(nq), int(nd)
    if nq < 0 or nd < 0:
        raise ValueError("relevance rows: nq and nd must be >= 0")
    if isinstance(relevant, tuple) and len(relevant) == 2 and all(isinstance(x, torch.Tensor) for x in relevant):
        ptr, docs = relevant
        if ptr.dim() != 1 or docs.dim() != 1 or ptr.numel() != nq + 1 or ptr.is_floating_point() or \
                docs.is_floating_point():
            raise ValueError(f"relevance rows: a CSR pair needs int tensors ptr [{nq + 1}] and docs [n]")
        ptr, docs = ptr.to(docs.device, torch.long), docs.long()
        if int(ptr[0]) != 0 or int(ptr[-1]) != docs.numel() or bool((ptr[1:] < ptr[:-1]).any()):
            raise ValueError("relevance rows: ptr must start at 0, not decrease and end at len(docs)")
        row = torch.repeat_interleave(torch.arange(nq, dtype=torch.long, device=docs.device), ptr[1:] - ptr[:-1])
    else:
        if isinstance(relevant, (str, bytes)) or not hasattr(relevant, "__iter__"):
            raise ValueError("relevance rows: per-query doc-id lists or a CSR pair of tensors")
        rows = [list(r) for r in relevant]
        if len(rows) != nq:
            raise ValueError(f"relevance rows: {len(rows)} rows for {nq} queries")
        flat = [d for r in rows for d in r]
        if any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) for d in flat):
            raise ValueError("relevance rows: doc ids must be ints")
        docs = torch.tensor([int(d) for d in flat], dtype=torch.long)
        row = torch.repeat_interleave(torch.arange(nq, dtype=torch.long),
                                      torch.tensor([len(r) for r in rows], dtype=torch.long))
    if docs.numel() and not bool(((docs >= -2 ** 31) & (docs < 2 ** 31)).all()):
        raise ValueError("relevance rows: doc ids must fit in int32")
    key = torch.unique(row * 2 ** 32 + (docs + 2 ** 31))      # sorted: by row, then doc; duplicates merged
    r, d = key // 2 ** 32, key % 2 ** 32 - 2 ** 31
    ptr = torch.zeros(nq + 1, dtype=torch.long, device=key.device)
    torch.cumsum(torch.bincount(r, minlength=nq), 0, out=ptr[1:])
    return ptr.to(device), d.to(torch.int32).to(device)


def discount_table(R: int) -> np.ndarray:
    """disc [R] float64 on the host: 1.0 / numpy.log2(p + 1), p = 1 .. R (include/snx.h: the kernel computes no log)."""
    return 1.0 / np.log2(np.arange(1, int(R) + 1, dtype=np.float64) + 1.0)


def ranked_relevance(docs: torch.Tensor, relevant, nd: int, cutoffs=(1, 5, 10)
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Ranked lists against relevance rows on the GPU (snx_ranked_relevance).  ``docs`` int32 [nq, R] (R <= 4096; a list
    ends at its first negative id): the doc output of ``search``, ``search_two_phase``, ``SeismicIndex.search``,
    ``Bm25Index.search_tokens`` or ``fuse_ranked``; ``relevant`` as ``relevance_csr`` takes it, ``nd`` the corpus size;
    ``cutoffs``: 1 .. 8 strictly ascending ints in [1, R].  -> (first int32 [nq]: 1-based position of the first relevant
    entry, 0 = none; hits int32 [nq, ncut]: relevant entries within each cutoff; dcg float64 [nq, ncut]: the left fold in
    position order of ``discount_table(R)[p - 1]`` over the relevant positions within each cutoff)."""
    if not isinstance(docs, torch.Tensor) or docs.dim() != 2 or docs.dtype != torch.int32 or docs.device.type != "cuda":
        raise ValueError("ranked_relevance: docs must be int32 [nq, R] on a GPU")
    dev, (nq, R) = docs.device, docs.shape
    if not 1 <= R <= RANKED_R_MAX:
        raise ValueError(f"ranked_relevance: lists of 1 .. {RANKED_R_MAX} entries")
    cuts = [c for c in cutoffs]
    if not 1 <= len(cuts) <= CUTOFFS_MAX or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) for c in cuts):
        raise ValueError(f"ranked_relevance: 1 .. {CUTOFFS_MAX} integer cutoffs")
    cuts = [int(c) for c in cuts]
    if cuts[0] < 1 or cuts[-1] > R or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"ranked_relevance: cutoffs must ascend strictly within [1, {R}]")
    rel_ptr, rel_doc = relevance_csr(relevant, int(nq), nd, dev)
    docs = docs.contiguous()
    disc = torch.from_numpy(discount_table(R)).to(dev)
    first = torch.empty(nq, dtype=torch.int32, device=dev)
    hits = torch.empty((nq, len(cuts)), dtype=torch.int32, device=dev)
    dcg = torch.empty((nq, len(cuts)), dtype=torch.float64, device=dev)
    import ctypes as C
    host = (C.c_int32 * len(cuts))(*cuts)
    with torch.cuda.device(dev):
        check(fn("snx_ranked_relevance")(_p(docs), int(nq), int(R), int(nd), _p(rel_ptr), _p(rel_doc),
                                         C.cast(host, C.c_void_p), len(cuts), _p(disc), _p(first), _p(hits), _p(dcg),
                                         _stream()), "snx_ranked_relevance")
    return first, hits, dcg


def bootstrap_indices(n: int, n_bootstrap: int = 1000, seed: int = 42) -> np.ndarray:
    """Resample indices int32 [n_bootstrap, n], drawn on the host as the reference draws them
    (ref:benchmark/metrics.py:198-204): ``numpy.random.RandomState(seed)``, then one ``randint(0, n, size=n)`` per
    resample, in order -- the stream of ``numpy.random.seed(seed)`` followed by ``numpy.random.choice(n, size=n,
    replace=True)`` per resample (tests/test_qrels_host.py holds the two equal over all draws)."""
    n, n_bootstrap = int(n), int(n_bootstrap)
    if n < 1 or n >= 2 ** 31 or n_bootstrap < 0:
        raise ValueError("bootstrap_indices: need 1 <= n < 2^31 and n_bootstrap >= 0")
    rs = np.random.RandomState(int(seed))
    out = np.empty((n_bootstrap, n), dtype=np.int32)
    for b in range(n_bootstrap):
        out[b] = rs.randint(0, n, size=n)
    return out


def bootstrap_means(values, n_bootstrap: int = 1000, seed: int = 42, device=None, indices=None) -> torch.Tensor:
    """Bootstrap means on the GPU (snx_bootstrap_means): ``values`` [n] or [n, M] (M <= 16; a tensor or an array, taken as
    float64) -> float64 [n_bootstrap, M] on the device: out[b, m] = the mean of column m over resample b, summed in the
    fixed order of include/snx.h (segments of 64 positions, left folds inside and across), bit-identical from run to
    run.  The resamples are ``bootstrap_indices(n, n_bootstrap, seed)`` unless ``indices`` int [n_bootstrap, n] is
    given; an index outside [0, n) is an argument error (checked here, where the indices are drawn: the C interface's
    precondition).  ``device``: where to run (default: the values' GPU, else the current one)."""
    if isinstance(values, torch.Tensor):
        if device is None and values.device.type == "cuda":
            device = values.device
        v = values.detach().to(torch.float64).cpu().numpy()
    else:
        v = np.asarray(values, dtype=np.float64)
    if v.ndim == 1:
        v = v[:, None]
    if v.ndim != 2 or v.shape[0] < 1 or not 1 <= v.shape[1] <= BOOTSTRAP_M_MAX:
        raise ValueError(f"bootstrap_means: values must be [n] or [n, M] with n >= 1 and M <= {BOOTSTRAP_M_MAX}")
    n, M = v.shape
    if indices is None:
        idx = bootstrap_indices(n, n_bootstrap, seed)
    else:
        idx = indices.cpu().numpy() if isinstance(indices, torch.Tensor) else np.asarray(indices)
        if idx.ndim != 2 or idx.shape[1] != n or idx.dtype.kind not in "iu":
            raise ValueError(f"bootstrap_means: indices must be an int array [n_bootstrap, {n}]")
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            from ._lib import SnxError
            raise SnxError(f"snx_bootstrap_means failed: SNX_E_ARG (a resample index lies outside [0, {n}))")
        idx = idx.astype(np.int32)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError("bootstrap_means: runs on a GPU")
    nb = int(idx.shape[0])
    vals = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    didx = torch.from_numpy(np.ascontiguousarray(idx)).to(dev)
    out = torch.empty((nb, M), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(fn("snx_bootstrap_means")(_p(vals), int(n), int(M), _p(didx), nb, _p(out), _stream()),
              "snx_bootstrap_means")
    return out


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
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
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
            self.emb = torch.cat(self._parts) if self._parts else torch.zeros((0, self.dim), dtype=torch.float32,
                                                                              device=self.device)
            self._parts = [self.emb]
        return self

    def _check(self, who: str, chunk_docs) -> int:
        if not self.built:
            raise RuntimeError(f"DenseIndex.{who}: call build() first")
        chunk_docs = int(chunk_docs)
        if chunk_docs != 0 and not DENSE_CHUNK_MIN <= chunk_docs < 2 ** 31:
            raise ValueError(f"DenseIndex.{who}: chunk_docs must be 0 (default) or at least {DENSE_CHUNK_MIN}")
        return chunk_docs

    def _slices(self, nq: int, sizing: str, k: int, chunk_docs: int, query_slice: int):
        """(start, rows, workspace bytes) of the launches: slices of the workspace budget, or of ``query_slice``."""
        if isinstance(query_slice, bool) or int(query_slice) < 0:
            raise ValueError("DenseIndex: query_slice must be >= 0 (0: default)")
        size = fn(sizing)
        per_q = max(1, -(-int(size(max(nq, 1), self.num_docs, k, chunk_docs)) // max(nq, 1)))
        step = max(1, min(max(nq, 1), _DENSE_WS_BUDGET // per_q))
        if query_slice:
            step = min(step, int(query_slice))
        for s in range(0, nq, step):
            m = min(step, nq - s)
            yield s, m, int(size(m, self.num_docs, k, chunk_docs))

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
        nq, nd, dev = int(q.shape[0]), self.num_docs, self.device
        tgt = None
        if targets is not None:
            if not isinstance(targets, torch.Tensor) or targets.device != dev or targets.dim() != 1 or \
                    targets.numel() != nq or targets.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"DenseIndex.search: targets must be an int tensor [{nq}] on {dev}")
            if nq and not bool(((targets >= 0) & (targets < nd)).all()):
                raise ValueError(f"DenseIndex.search: targets must be doc ids in [0, {nd})")
            tgt = targets.to(torch.int32).contiguous()
        scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        docs = torch.empty((nq, k), dtype=torch.int32, device=dev)
        rank = torch.empty(nq, dtype=torch.int32, device=dev) if tgt is not None else None
        tscore = torch.empty(nq, dtype=torch.float32, device=dev) if tgt is not None else None
        with torch.cuda.device(dev):
            for s, m, ws_bytes in self._slices(nq, "snx_dense_search_workspace_bytes", k, chunk_docs, query_slice):
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
                check(fn("snx_dense_search")(
                    _p(q[s:]), m, _p(self.emb), nd, self.dim, _p(None if tgt is None else tgt[s:]), k, chunk_docs,
                    _p(docs[s:]), _p(scores[s:]), _p(None if rank is None else rank[s:]),
                    _p(None if tscore is None else tscore[s:]), _p(ws), ws_bytes, _stream()), "snx_dense_search")
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
        nq, nd, dev = int(q.shape[0]), self.num_docs, self.device
        ex_ptr = ex_doc = None
        if exclude is not None:
            ex_ptr, ex_doc = exclusion_csr(exclude, nq, nd, dev)
            if ex_doc.numel() == 0:
                ex_ptr = ex_doc = None
        ceil = None
        if ceiling is not None:
            if not isinstance(ceiling, torch.Tensor) or ceiling.device != dev or ceiling.dtype != torch.float32 or \
                    ceiling.dim() != 1 or ceiling.numel() != nq:
                raise ValueError(f"DenseIndex.search_band: ceiling must be fp32 [{nq}] on {dev}")
            if nq and bool(torch.isnan(ceiling).any()):
                raise ValueError("DenseIndex.search_band: ceiling must not be NaN (+inf: no ceiling)")
            ceil = ceiling.contiguous()
        w = hi - lo
        scores = torch.empty((nq, w), dtype=torch.float32, device=dev)
        docs = torch.empty((nq, w), dtype=torch.int32, device=dev)
        found = torch.empty(nq, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            for s, m, ws_bytes in self._slices(nq, "snx_dense_search_band_workspace_bytes", hi, chunk_docs, query_slice):
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
                check(fn("snx_dense_search_band")(
                    _p(q[s:]), m, _p(self.emb), nd, self.dim, _p(None if ex_ptr is None else ex_ptr[s:]), _p(ex_doc),
                    _p(None if ceil is None else ceil[s:]), lo, hi, chunk_docs, _p(docs[s:]), _p(scores[s:]),
                    _p(found[s:]), _p(ws), ws_bytes, _stream()), "snx_dense_search_band")
        return scores, docs, found

    def pair_scores(self, q: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
        """``pairs`` int [n, 2] of (query row, doc id) -> s(q, d) fp32 [n], bit-equal to the scores the searches rank."""
        self._check("pair_scores", 0)
        q = self._rows(q, "pair_scores", "q")
        nq, nd, dev = int(q.shape[0]), self.num_docs, self.device
        if not isinstance(pairs, torch.Tensor) or pairs.device != dev or pairs.dim() != 2 or pairs.shape[1] != 2 or \
                pairs.is_floating_point():
            raise ValueError(f"DenseIndex.pair_scores: pairs must be an int tensor [n, 2] on {dev}")
        n = int(pairs.shape[0])
        if n and not bool(((pairs[:, 0] >= 0) & (pairs[:, 0] < nq) & (pairs[:, 1] >= 0) & (pairs[:, 1] < nd)).all()):
            raise ValueError(f"DenseIndex.pair_scores: pairs must be (query in [0, {nq}), doc in [0, {nd}))")
        pq = pairs[:, 0].to(torch.int32).contiguous()
        pd = pairs[:, 1].to(torch.int32).contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(fn("snx_dense_pair_scores")(_p(q), nq, _p(self.emb), nd, self.dim, _p(pq), _p(pd), n, _p(out),
                                               _stream()), "snx_dense_pair_scores")
        return out

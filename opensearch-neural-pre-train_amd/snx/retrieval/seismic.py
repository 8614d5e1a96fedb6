"""SEISMIC approximate search over a built ``SparseIndex`` (csrc/seismic.hip, include/snx.h "SEISMIC")."""
import time
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .._lib import call
from ..ops import _p, _stream
from ._common import K_MAX, at, check_query_slice, check_targets, offsets, search_outputs, slices, workspace
from .sparse import SparseIndex, pack_rows

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
            self.prune_ptr = offsets(lens)
            p = lens.cpu().numpy().astype(np.float64)          # cluster counts in float64 on the host (the contract)
            c = np.where(p > 0, np.minimum(p, np.maximum(1.0, np.ceil(self.cluster_ratio * p))), 0.0).astype(np.int32)
            cent_cnt = torch.from_numpy(c).to(dev)
            self.cent_ptr = offsets(cent_cnt.long())
            P, C = int(self.prune_ptr[-1]), int(self.cent_ptr[-1])
            self.prune_doc = torch.empty(P, dtype=torch.int32, device=dev)
            self.prune_w = torch.empty(P, dtype=torch.float32, device=dev)
            self.cent_doc = torch.empty(C, dtype=torch.int32, device=dev)
            assign = torch.empty(P, dtype=torch.int32, device=dev)
            cent_size = torch.zeros(C, dtype=torch.int32, device=dev)
            call("snx_seismic_build_clusters", _p(index.term_ptr), _p(index.post_doc), _p(index.post_w),
                 _p(index.doc_ptr), _p(index.doc_term), _p(index.doc_w), nd, V, self.n_postings, _p(self.prune_ptr),
                 _p(cent_cnt), _p(self.cent_ptr), P, C, _p(self.prune_doc), _p(self.prune_w), _p(self.cent_doc),
                 _p(assign), _p(cent_size), _stream())
            cursor = offsets(cent_size.long())                 # block start of every centroid (empty: no room)
            self.blk_doc = torch.empty(P, dtype=torch.int32, device=dev)
            call("snx_seismic_build_blocks", _p(self.prune_ptr), _p(self.prune_doc), _p(assign), _p(self.cent_ptr), V,
                 P, _p(cursor), _p(self.blk_doc), _stream())
            live = cent_size > 0
            nb = int(live.sum())
            self.blk_ptr = offsets(cent_size[live].long())
            term_of = torch.repeat_interleave(torch.arange(V, device=dev), cent_cnt.long())
            self.term_blk_ptr = offsets(torch.bincount(term_of[live], minlength=V))
            self.blk_cent = (torch.arange(C, device=dev) - self.cent_ptr[term_of])[live].to(torch.int32)
            ws, ws_bytes = workspace("snx_seismic_build_workspace_bytes", dev, V, nb)
            sum_cnt = torch.empty(nb, dtype=torch.int32, device=dev)
            alpha = float(np.float32(self.summary_prune_ratio))
            call("snx_seismic_build_summaries", _p(index.doc_ptr), _p(index.doc_term), _p(index.doc_w), nd, V,
                 _p(self.blk_ptr), _p(self.blk_doc), nb, alpha, None, _p(sum_cnt), None, None, _p(ws), ws_bytes, _stream())
            self.sum_ptr = offsets(sum_cnt.long())
            S = int(self.sum_ptr[-1])
            self.sum_term = torch.empty(S, dtype=torch.int32, device=dev)
            self.sum_w = torch.empty(S, dtype=torch.float32, device=dev)
            call("snx_seismic_build_summaries", _p(index.doc_ptr), _p(index.doc_term), _p(index.doc_w), nd, V,
                 _p(self.blk_ptr), _p(self.blk_doc), nb, alpha, _p(self.sum_ptr), _p(sum_cnt), _p(self.sum_term),
                 _p(self.sum_w), _p(ws), ws_bytes, _stream())
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
        check_query_slice(query_slice, "SeismicIndex.search")
        dev, V, nd = idx.device, idx.V, idx.num_docs
        if not isinstance(q_vals, torch.Tensor) or q_vals.device != dev:
            raise ValueError(f"SeismicIndex.search: tensors must be on {dev}")
        qc, q_term, q_w = pack_rows(q_vals, q_ids, q_cnt, V, "queries")
        nq = int(qc.numel())
        max_nnz = int(qc.max()) if nq else 0
        if max_nnz > SEISMIC_Q_MAX:
            raise ValueError(f"SeismicIndex.search: a query holds {max_nnz} terms; the cap is {SEISMIC_Q_MAX}")
        q_ptr = offsets(qc)
        tgt = check_targets(targets, nq, nd, dev, "SeismicIndex.search")
        scores, docs, rank, tscore = search_outputs(nq, k, dev, tgt is not None)
        stats = torch.empty((nq, 3), dtype=torch.long, device=dev)
        with torch.cuda.device(dev):
            for s, m in slices(nq, int(query_slice) or _SEISMIC_QUERY_SLICE):
                call("snx_seismic_search", _p(q_ptr[s:]), _p(q_term), _p(q_w), m, max_nnz, _p(self.term_blk_ptr),
                     _p(self.blk_ptr), _p(self.blk_doc), _p(self.sum_ptr), _p(self.sum_term), _p(self.sum_w),
                     _p(idx.doc_ptr), _p(idx.doc_term), _p(idx.doc_w), nd, V, _p(at(tgt, s)), k, top_n, hf,
                     _p(docs[s:]), _p(scores[s:]), _p(at(rank, s)), _p(at(tscore, s)), _p(stats[s:]), _stream())
        return scores, docs, rank, tscore, {"blocks_total": stats[:, 0], "blocks_scored": stats[:, 1],
                                            "postings_scored": stats[:, 2]}

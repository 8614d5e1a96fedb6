"""Graph approximate inner-product search over dense fp32 embeddings (csrc/graph.hip, include/snx.h "graph dense
retrieval")."""
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .._lib import call
from ..ops import _p, _stream
from ._common import (K_MAX, at, cat_or_empty, check_pairs, check_query_slice, cuda_device, exclusion_or_null,
                      search_outputs, slices, step_bytes_mean, workspace)
from .dense import DENSE_DIM_MAX

GRAPH_DEGREE_MAX = 64
GRAPH_KNN_MAX = 128
GRAPH_EF_MAX = K_MAX
GRAPH_WIDTH_MAX = 8
_GRAPH_WS_BUDGET = 1 << 30             # bytes of workspace per launch, build and search (the tests force a tiny one)


def _int_in(x, lo: int, hi: int, who: str, name: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError(f"{who}: {name} must be an int in [{lo}, {hi}]")
    return int(x)


def entry_sample(nd: int, nentry: int) -> np.ndarray:
    """entry_i = floor(i * nd / nentry), i = 0 .. nentry-1, in int64."""
    return (np.arange(nentry, dtype=np.int64) * np.int64(nd)) // np.int64(max(nentry, 1))


class GraphIndex:
    """Fixed-degree graph index over dense fp32 embeddings on the GPU, in the ROLE of the HNSW ``knn_vector`` field behind
    the reference's dense benchmark rows (ref:benchmark/index_manager.py:98-110, ref:benchmark/searchers.py:97-127), with
    the scores, order and conventions of ``DenseIndex``.

        index = GraphIndex(dim, device, degree=32, knn=64, ef=100, width=4, nentry=None)
        index.add(emb); index.build(neighbors=None)
        index.structure()                   # dict(neighbors, forward, graph, entry)
        scores, docs = index.search(q, k, ef=None, width=None, max_iter=0, query_slice=0)
        scores, docs, found = index.search_band(q, lo, hi, exclude=None, ceiling=None, ef=None, width=None, max_iter=0)
        s = index.pair_scores(q, pairs)     # DenseIndex's
        index.last_iterations               # int32 [nq] of the last search

    The defaults map the reference's settings: ``m = 16`` is 32 links on HNSW's layer 0, hence ``degree = 32``;
    ``ef_construction = 128`` is a candidate list of twice the degree, hence ``knn = 64``; ``ef = 100`` is the k-NN plugin's
    default ``ef_search`` (the reference sets none).  The graph is NOT the one FAISS would build: it is the deterministic
    graph of include/snx.h (exact kNN lists, CAGRA's detour pruning, reverse edges) searched by a best-first beam of
    ``ef`` entries that expands ``width`` of them per iteration from the best of ``nentry`` evenly spaced entry docs
    (default ``4 * ceil(sqrt(nd))``).  ``build(neighbors=)`` takes int32 [nd, knn] lists from elsewhere instead of the
    exact ones.  With ``ef >= nd`` the result is ``DenseIndex.search``'s, bit for bit.  Results are bit-reproducible and
    independent of the query slicing, the workspace budget and the batches of ``add``."""

    def __init__(self, dim: int, device, degree: int = 32, knn: int = 64, ef: int = 100, width: int = 4,
                 nentry: Optional[int] = None):
        self.dim = _int_in(dim, 1, DENSE_DIM_MAX, "GraphIndex", "dim")
        self.device = cuda_device(device)
        self._parts: List[torch.Tensor] = []
        self.num_docs = 0
        self.emb: Optional[torch.Tensor] = None               # the rows in order of addition
        self.degree = _int_in(degree, 2, GRAPH_DEGREE_MAX, "GraphIndex", "degree")
        if self.degree % 2:
            raise ValueError("GraphIndex: degree must be even")
        self.knn = _int_in(knn, self.degree, GRAPH_KNN_MAX, "GraphIndex", "knn")
        self.ef = self._ef(ef, "GraphIndex")
        self.width = self._width(width, "GraphIndex")
        self.nentry = None if nentry is None else _int_in(nentry, 1, 2 ** 31 - 1, "GraphIndex", "nentry")
        self.neighbors: Optional[torch.Tensor] = None
        self.forward: Optional[torch.Tensor] = None
        self.graph: Optional[torch.Tensor] = None
        self.last_iterations: Optional[torch.Tensor] = None
        self._entries: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}

    @property
    def built(self) -> bool:
        return self.graph is not None

    def _ef(self, ef, who: str) -> int:
        return self.ef if ef is None else _int_in(ef, 1, GRAPH_EF_MAX, who, "ef")

    def _width(self, width, who: str) -> int:
        return self.width if width is None else _int_in(width, 1, GRAPH_WIDTH_MAX, who, "width")

    def _rows(self, x, who: str, name: str) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"GraphIndex.{who}: {name} must be an fp32 tensor [n, {self.dim}]")
        if x.device != self.device:
            raise ValueError(f"GraphIndex.{who}: {name} must be on {self.device}")
        if x.numel() and not bool(torch.isfinite(x).all()):
            raise ValueError(f"GraphIndex.{who}: {name} must be finite")
        return x.contiguous()

    # -------------------------------------------------------------------------------------------- build
    def add(self, emb: torch.Tensor) -> None:
        e = self._rows(emb, "add", "emb")
        if self.num_docs + e.shape[0] >= 2 ** 31:
            raise ValueError("GraphIndex: doc ids are int32")
        self._parts.append(e)
        self.num_docs += int(e.shape[0])
        self.graph = None                                     # a new batch invalidates a built index

    def _gather(self) -> None:
        if len(self._parts) == 1:
            self.emb = self._parts[0]
        else:
            self.emb = cat_or_empty(self._parts, torch.float32, self.device, self.dim)
            self._parts = [self.emb]

    def exact_neighbors(self) -> torch.Tensor:
        """N of the header over the docs added so far, int32 [nd, knn]: snx_dense_search_band, lo = 0, hi = knn, doc u
        excluded from its own row.  ``build()`` calls it when no lists are handed in."""
        self._gather()
        nd, dev, sizing = self.num_docs, self.device, "snx_dense_search_band_workspace_bytes"
        scores, ids, _, _ = search_outputs(nd, self.knn, dev, False)
        found = torch.empty(nd, dtype=torch.int32, device=dev)
        ex_ptr = torch.arange(nd + 1, dtype=torch.long, device=dev)
        ex_doc = torch.arange(nd, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            for s, m in slices(nd, step_bytes_mean(sizing, _GRAPH_WS_BUDGET, nd, nd, self.knn, 0)):
                ws, ws_bytes = workspace(sizing, dev, m, nd, self.knn, 0)
                call("snx_dense_search_band", _p(self.emb[s:]), m, _p(self.emb), nd, self.dim, _p(ex_ptr[s:]), _p(ex_doc),
                     None, 0, self.knn, 0, _p(ids[s:]), _p(scores[s:]), _p(found[s:]), _p(ws), ws_bytes, _stream())
        return ids

    def _given_neighbors(self, neighbors) -> torch.Tensor:
        nd, knn, dev = self.num_docs, self.knn, self.device
        if not isinstance(neighbors, torch.Tensor) or neighbors.dtype != torch.int32 or \
                tuple(neighbors.shape) != (nd, knn):
            raise ValueError(f"GraphIndex.build: neighbors must be an int32 tensor [{nd}, {knn}]")
        if neighbors.device != dev:
            raise ValueError(f"GraphIndex.build: neighbors must be on {dev}")
        n = neighbors.contiguous()
        if nd:
            own = torch.arange(nd, dtype=torch.int32, device=dev).unsqueeze(1)
            valid = n >= 0
            if not bool(((n >= -1) & (n < nd) & (n != own)).all()):
                raise ValueError(f"GraphIndex.build: neighbors must be doc ids in [0, {nd}) other than the row's own, or -1")
            if bool((valid[:, 1:] & ~valid[:, :-1]).any()):
                raise ValueError("GraphIndex.build: a neighbors row must hold its ids first and -1 after them")
            ordered = torch.sort(n, dim=1).values
            if bool(((ordered[:, 1:] == ordered[:, :-1]) & (ordered[:, 1:] >= 0)).any()):
                raise ValueError("GraphIndex.build: a neighbors row must not hold a doc twice")
        return n.clone()

    def build(self, neighbors: Optional[torch.Tensor] = None) -> "GraphIndex":
        self._gather()
        nd, dev, sizing = self.num_docs, self.device, "snx_graph_optimize_workspace_bytes"
        self.neighbors = self.exact_neighbors() if neighbors is None else self._given_neighbors(neighbors)
        self.forward = torch.empty((nd, self.degree), dtype=torch.int32, device=dev)
        graph = torch.empty((nd, self.degree), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws, ws_bytes = workspace(sizing, dev, nd, self.knn, self.degree)
            call("snx_graph_optimize", _p(self.neighbors), nd, self.knn, self.degree, _p(graph), _p(self.forward), _p(ws),
                 ws_bytes, _stream())
        self.graph = graph
        self._entries = {}
        return self

    def _check_built(self, who: str) -> None:
        if not self.built:
            raise RuntimeError(f"GraphIndex.{who}: call build() first")

    def entry_count(self, ef: int) -> int:
        """Entry docs of a search with ``ef``: ``nentry`` (default 4 * ceil(sqrt(nd))) clamped to [min(ef, nd), nd]."""
        nd = self.num_docs
        want = self.nentry if self.nentry is not None else 4 * (math.isqrt(max(nd - 1, 0)) + 1)   # 4 * ceil(sqrt(nd))
        return max(min(ef, nd), min(want, nd))

    def _entry(self, ef: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(entry ids int64 [nentry], their rows) for a search with ``ef``."""
        ne = self.entry_count(ef)
        if ne not in self._entries:
            ids = torch.from_numpy(entry_sample(self.num_docs, ne)).to(self.device)
            self._entries = {ne: (ids, self.emb.index_select(0, ids))}
        return self._entries[ne]

    def structure(self) -> Dict[str, torch.Tensor]:
        self._check_built("structure")
        return {"neighbors": self.neighbors, "forward": self.forward, "graph": self.graph,
                "entry": self._entry(self.ef)[0].to(torch.int32)}

    # -------------------------------------------------------------------------------------------- search
    def _seeds(self, q: torch.Tensor, ef: int) -> torch.Tensor:
        """The best min(ef, nentry) entry docs of every query: snx_dense_search over the entry rows, ids mapped back."""
        ids, rows = self._entry(ef)
        n, ne, dev, sizing = int(q.shape[0]), int(ids.numel()), self.device, "snx_dense_search_workspace_bytes"
        k = min(ef, ne)
        scores, local, _, _ = search_outputs(n, k, dev, False)
        with torch.cuda.device(dev):
            for s, m in slices(n, step_bytes_mean(sizing, _GRAPH_WS_BUDGET, n, ne, k, 0)):
                ws, ws_bytes = workspace(sizing, dev, m, ne, k, 0)
                call("snx_dense_search", _p(q[s:]), m, _p(rows), ne, self.dim, None, k, 0, _p(local[s:]), _p(scores[s:]),
                     None, None, _p(ws), ws_bytes, _stream())
        return ids[local.long()].to(torch.int32).contiguous()

    def _ceiling(self, ceiling, nq: int, who: str) -> Optional[torch.Tensor]:
        # as check_ceiling, but a NaN is let through: the header defines it (it admits nothing)
        if ceiling is None:
            return None
        if not isinstance(ceiling, torch.Tensor) or ceiling.device != self.device or ceiling.dtype != torch.float32 or \
                ceiling.dim() != 1 or ceiling.numel() != nq:
            raise ValueError(f"{who}: ceiling must be fp32 [{nq}] on {self.device}")
        return ceiling.contiguous()

    def _walk(self, who, q, lo, hi, exclude, ceiling, ef, width, max_iter, query_slice, with_found):
        self._check_built(who)
        name = f"GraphIndex.{who}"
        ef, width = self._ef(ef, name), self._width(width, name)
        max_iter = _int_in(max_iter, 0, 2 ** 31 - 1, name, "max_iter")
        if hi > ef:
            raise ValueError(f"{name}: the ranks asked for must lie inside ef = {ef}")
        q = self._rows(q, who, "q")
        check_query_slice(query_slice, "GraphIndex")
        nq, nd, dev, sizing = int(q.shape[0]), self.num_docs, self.device, "snx_graph_search_workspace_bytes"
        ex_ptr, ex_doc = exclusion_or_null(exclude, nq, nd, dev)
        ceil = self._ceiling(ceiling, nq, name)
        scores, docs, _, _ = search_outputs(nq, hi - lo, dev, False)
        found = torch.empty(nq, dtype=torch.int32, device=dev) if with_found else None
        iters = torch.zeros(nq, dtype=torch.int32, device=dev)
        if nd and nq:
            seeds = self._seeds(q, ef)
        else:
            seeds = torch.zeros((nq, 0), dtype=torch.int32, device=dev)
        nseed = int(seeds.shape[1])
        step = step_bytes_mean(sizing, _GRAPH_WS_BUDGET, nq, ef, width, self.degree)
        if query_slice:
            step = min(step, int(query_slice))
        with torch.cuda.device(dev):
            for s, m in slices(nq, step):
                ws, ws_bytes = workspace(sizing, dev, m, ef, width, self.degree)
                call("snx_graph_search", _p(q[s:]), m, self.dim, _p(self.emb), nd, _p(self.graph), self.degree,
                     _p(seeds[s:]), nseed, ef, width, max_iter, _p(at(ex_ptr, s)), _p(ex_doc), _p(at(ceil, s)), lo, hi,
                     _p(docs[s:]), _p(scores[s:]), _p(at(found, s)), _p(iters[s:]), _p(ws), ws_bytes, _stream())
        self.last_iterations = iters
        return scores, docs, found

    def search(self, q: torch.Tensor, k: int, ef: Optional[int] = None, width: Optional[int] = None, max_iter: int = 0,
               query_slice: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """``q`` fp32 [nq, dim] -> (scores [nq, k] fp32, docs [nq, k] int32): ranks 0 .. k-1 of the walk's pool, k <= ef;
        unused slots 0 / -1."""
        k = _int_in(k, 1, K_MAX, "GraphIndex.search", "k")
        scores, docs, _ = self._walk("search", q, 0, k, None, None, ef, width, max_iter, query_slice, False)
        return scores, docs

    def search_band(self, q: torch.Tensor, lo: int, hi: int, exclude=None, ceiling: Optional[torch.Tensor] = None,
                    chunk_docs: int = 0, query_slice: int = 0, ef: Optional[int] = None, width: Optional[int] = None,
                    max_iter: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Ranks ``lo .. hi-1`` (hi <= ef) of the ADMISSIBLE entries of the walk's final pool (``DenseIndex.search_band``'s
        rules; the walk itself does not see them) -> (scores, docs, found).  ``chunk_docs`` is accepted for
        ``DenseIndex``'s signature and ignored."""
        if isinstance(lo, bool) or isinstance(hi, bool) or not isinstance(lo, (int, np.integer)) or \
                not isinstance(hi, (int, np.integer)) or not 0 <= int(lo) < int(hi) <= K_MAX:
            raise ValueError(f"GraphIndex.search_band: need 0 <= lo < hi <= {K_MAX}")
        return self._walk("search_band", q, int(lo), int(hi), exclude, ceiling, ef, width, max_iter, query_slice, True)

    def pair_scores(self, q: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
        """``pairs`` int [n, 2] of (query row, doc id) -> s(q, d) fp32 [n], bit-equal to the scores the searches rank."""
        self._check_built("pair_scores")
        q = self._rows(q, "pair_scores", "q")
        nq, nd, dev = int(q.shape[0]), self.num_docs, self.device
        pq, pd = check_pairs(pairs, nq, nd, dev, "GraphIndex.pair_scores")
        n = int(pq.numel())
        out = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("snx_dense_pair_scores", _p(q), nq, _p(self.emb), nd, self.dim, _p(pq), _p(pd), n, _p(out), _stream())
        return out

"""IVF-Flat approximate inner-product search over dense fp32 embeddings (csrc/ivf.hip, include/snx.h "IVF-Flat dense
retrieval")."""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .._lib import call
from ..ops import _p, _stream
from ._common import (K_MAX, at, cat_or_empty, check_ceiling, check_pairs, check_query_slice, cuda_device,
                      exclusion_or_null, search_outputs, slices, step_bytes_mean, workspace)
from .dense import DENSE_DIM_MAX

IVF_NLIST_MAX = 65536
IVF_SPLIT_MIN = 128                    # docs per split of a list, at least (one tile)
_IVF_WS_BUDGET = 1 << 30               # bytes of search workspace per launch (the tests force a tiny one)
_IVF_SPLIT_DOCS = 0                    # docs per split of a long list (0: the kernel's default); changes no result


class IvfFlatIndex:
    """Inverted-file index with flat (uncompressed) lists over dense fp32 embeddings on the GPU: the
    ``faiss.IndexIVFFlat`` of the reference's dense miner (ref:src/preprocessing/miners/bge_m3_miner.py:91-136) with the
    scores, order and conventions of ``DenseIndex``.

        index = IvfFlatIndex(dim, nlist, device, nprobe=1, niter=10, seed=0)
        index.train(x)                      # fp32 [n, dim] on the device, n >= nlist; or
        index.set_centroids(c)              # fp32 [nlist, dim]
        index.add(emb); index.build()       # build() trains on the added rows when neither was called
        scores, lists = index.probe(q, nprobe=None)
        scores, docs = index.search(q, k, nprobe=None, query_slice=0)
        scores, docs, found = index.search_band(q, lo, hi, exclude=None, ceiling=None, nprobe=None)
        s = index.pair_scores(q, pairs)     # bit-equal to DenseIndex.pair_scores
        index.structure()                   # dict(centroids, list_ptr, list_doc)

    A doc lives in the list of its best centroid (ties to the lowest list); a query reads the ``nprobe`` best lists and
    gets the top ``k`` of the docs in them, ties to the lowest ORIGINAL doc id.  With ``nprobe == nlist`` the result is
    ``DenseIndex.search``'s, bit for bit.  Training is the index's own deterministic spherical k-means (``niter`` steps from
    the rows ``numpy.random.RandomState(seed).permutation(n)[:nlist]``): the lists are NOT the ones FAISS would build.
    ``nlist`` is clamped to the doc count when ``build()`` trains.  Results are bit-reproducible and independent of the
    query slicing, the workspace budget, the split of long lists and the batches of ``add``."""

    def __init__(self, dim: int, nlist: int, device, nprobe: int = 1, niter: int = 10, seed: int = 0):
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or not 1 <= int(dim) <= DENSE_DIM_MAX:
            raise ValueError(f"IvfFlatIndex: dim must be an int in [1, {DENSE_DIM_MAX}]")
        if isinstance(nlist, bool) or not isinstance(nlist, (int, np.integer)) or not 1 <= int(nlist) <= IVF_NLIST_MAX:
            raise ValueError(f"IvfFlatIndex: nlist must be an int in [1, {IVF_NLIST_MAX}]")
        if isinstance(niter, bool) or not isinstance(niter, (int, np.integer)) or int(niter) < 0:
            raise ValueError("IvfFlatIndex: niter must be an int >= 0")
        self.dim, self.nlist, self.niter, self.seed = int(dim), int(nlist), int(niter), int(seed)
        self.nprobe = self._nprobe(nprobe, "IvfFlatIndex")
        self.device = cuda_device(device)
        self._parts: List[torch.Tensor] = []
        self.num_docs = 0
        self.emb: Optional[torch.Tensor] = None               # the rows in order of addition (pair_scores)
        self.centroids: Optional[torch.Tensor] = None
        self.list_ptr: Optional[torch.Tensor] = None
        self.list_doc: Optional[torch.Tensor] = None
        self.list_emb: Optional[torch.Tensor] = None           # the rows in list order (the fine scan)
        self.max_list = 0

    @property
    def built(self) -> bool:
        return self.list_ptr is not None

    def _nprobe(self, nprobe, who: str) -> int:
        if nprobe is None:
            return self.nprobe
        top = min(self.nlist, K_MAX)
        if isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or not 1 <= int(nprobe) <= top:
            raise ValueError(f"{who}: nprobe must be an int in [1, {top}]")
        return int(nprobe)

    def _rows(self, x, who: str, name: str) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"IvfFlatIndex.{who}: {name} must be an fp32 tensor [n, {self.dim}]")
        if x.device != self.device:
            raise ValueError(f"IvfFlatIndex.{who}: {name} must be on {self.device}")
        if x.numel() and not bool(torch.isfinite(x).all()):
            raise ValueError(f"IvfFlatIndex.{who}: {name} must be finite")
        return x.contiguous()

    # -------------------------------------------------------------------------------------------- quantizer
    def _best(self, x: torch.Tensor, c: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ``k`` best rows of ``c`` for every row of ``x`` under the dense order: snx_dense_search over the centroids."""
        n, nc, dev, sizing = int(x.shape[0]), int(c.shape[0]), self.device, "snx_dense_search_workspace_bytes"
        scores, ids, _, _ = search_outputs(n, k, dev, False)
        with torch.cuda.device(dev):
            for s, m in slices(n, step_bytes_mean(sizing, _IVF_WS_BUDGET, n, nc, k, 0)):
                ws, ws_bytes = workspace(sizing, dev, m, nc, k, 0)
                call("snx_dense_search", _p(x[s:]), m, _p(c), nc, self.dim, None, k, 0, _p(ids[s:]), _p(scores[s:]),
                     None, None, _p(ws), ws_bytes, _stream())
        return scores, ids

    def _sorted_by_list(self, lists: torch.Tensor, nlist: int, emb: Optional[torch.Tensor]):
        """Stable counting sort of rows by list -> (list_ptr int64 [nlist+1], list_doc int32 [n], rows in list order)."""
        n, dev = int(lists.numel()), self.device
        ptr = torch.empty(nlist + 1, dtype=torch.long, device=dev)
        doc = torch.empty(n, dtype=torch.int32, device=dev)
        out = torch.empty((n, self.dim), dtype=torch.float32, device=dev) if emb is not None else None
        with torch.cuda.device(dev):
            ws, ws_bytes = workspace("snx_ivf_build_workspace_bytes", dev, n, nlist)
            call("snx_ivf_build", _p(lists), n, nlist, _p(emb), self.dim, _p(ptr), _p(doc), _p(out), _p(ws), ws_bytes,
                 _stream())
        return ptr, doc, out

    def _update(self, x: torch.Tensor, ptr: torch.Tensor, rows: torch.Tensor, prev: torch.Tensor) -> torch.Tensor:
        out = torch.empty_like(prev)
        with torch.cuda.device(self.device):
            call("snx_ivf_kmeans_update", _p(x), int(x.shape[0]), self.dim, _p(ptr), _p(rows), int(prev.shape[0]),
                 _p(prev), _p(out), _stream())
        return out

    def _kmeans(self, x: torch.Tensor, nlist: int) -> torch.Tensor:
        n, dev = int(x.shape[0]), self.device
        first = np.random.RandomState(self.seed).permutation(n)[:nlist].astype(np.int32)
        ptr = torch.arange(nlist + 1, dtype=torch.long, device=dev)
        c = self._update(x, ptr, torch.from_numpy(first).to(dev), torch.zeros((nlist, self.dim), device=dev))
        for _ in range(self.niter):
            _, lists = self._best(x, c, 1)
            ptr, rows, _ = self._sorted_by_list(lists.reshape(-1), nlist, None)
            c = self._update(x, ptr, rows, c)
        return c

    def train(self, x: torch.Tensor) -> "IvfFlatIndex":
        """Spherical k-means over ``x`` fp32 [n, dim], n >= nlist (see the class docstring)."""
        x = self._rows(x, "train", "x")
        if x.shape[0] < self.nlist:
            raise ValueError(f"IvfFlatIndex.train: {int(x.shape[0])} rows for {self.nlist} lists")
        self.centroids = self._kmeans(x, self.nlist)
        self.list_ptr = None
        return self

    def set_centroids(self, c: torch.Tensor) -> "IvfFlatIndex":
        c = self._rows(c, "set_centroids", "c")
        if c.shape[0] != self.nlist:
            raise ValueError(f"IvfFlatIndex.set_centroids: c must hold {self.nlist} rows")
        self.centroids = c.clone()
        self.list_ptr = None
        return self

    # -------------------------------------------------------------------------------------------- docs
    def add(self, emb: torch.Tensor) -> None:
        e = self._rows(emb, "add", "emb")
        if self.num_docs + e.shape[0] >= 2 ** 31:
            raise ValueError("IvfFlatIndex: doc ids are int32")
        self._parts.append(e)
        self.num_docs += int(e.shape[0])
        self.list_ptr = None                                  # a new batch invalidates a built index

    def build(self) -> "IvfFlatIndex":
        if len(self._parts) == 1:
            self.emb = self._parts[0]
        else:
            self.emb = cat_or_empty(self._parts, torch.float32, self.device, self.dim)
            self._parts = [self.emb]
        if self.centroids is None:
            if self.num_docs == 0:
                raise RuntimeError("IvfFlatIndex.build: no centroids and no docs to train on")
            self.nlist = min(self.nlist, self.num_docs)       # as the reference clamps it (ref:bge_m3_miner.py:125)
            self.nprobe = min(self.nprobe, self.nlist)
            self.centroids = self._kmeans(self.emb, self.nlist)
        _, lists = self._best(self.emb, self.centroids, 1)
        self.list_ptr, self.list_doc, self.list_emb = self._sorted_by_list(lists.reshape(-1), self.nlist, self.emb)
        self.max_list = int((self.list_ptr[1:] - self.list_ptr[:-1]).max()) if self.num_docs else 0
        return self

    def structure(self) -> Dict[str, torch.Tensor]:
        self._check("structure")
        return {"centroids": self.centroids, "list_ptr": self.list_ptr, "list_doc": self.list_doc}

    def _check(self, who: str) -> None:
        if not self.built:
            raise RuntimeError(f"IvfFlatIndex.{who}: call build() first")

    # -------------------------------------------------------------------------------------------- search
    def probe(self, q: torch.Tensor, nprobe: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``q`` fp32 [nq, dim] -> (scores [nq, nprobe] fp32, lists [nq, nprobe] int32): the best centroids, best first."""
        if self.centroids is None:
            raise RuntimeError("IvfFlatIndex.probe: no centroids yet")
        nprobe = self._nprobe(nprobe, "IvfFlatIndex.probe")
        return self._best(self._rows(q, "probe", "q"), self.centroids, nprobe)

    def _search(self, who, q, lo, hi, exclude, ceiling, query_slice, nprobe, with_found):
        self._check(who)
        nprobe = self._nprobe(nprobe, f"IvfFlatIndex.{who}")
        q = self._rows(q, who, "q")
        check_query_slice(query_slice, "IvfFlatIndex")
        nq, nd, dev, sizing = int(q.shape[0]), self.num_docs, self.device, "snx_ivf_search_workspace_bytes"
        ex_ptr, ex_doc = exclusion_or_null(exclude, nq, nd, dev)
        ceil = check_ceiling(ceiling, nq, dev, f"IvfFlatIndex.{who}")
        scores, docs, _, _ = search_outputs(nq, hi - lo, dev, False)
        found = torch.empty(nq, dtype=torch.int32, device=dev) if with_found else None
        _, lists = self._best(q, self.centroids, nprobe)
        shape = (nd, self.nlist, nprobe, hi, self.max_list, _IVF_SPLIT_DOCS)
        step = step_bytes_mean(sizing, _IVF_WS_BUDGET, nq, *shape)
        if query_slice:
            step = min(step, int(query_slice))
        with torch.cuda.device(dev):
            for s, m in slices(nq, step):
                ws, ws_bytes = workspace(sizing, dev, m, *shape)
                call("snx_ivf_search", _p(q[s:]), m, self.dim, _p(self.list_emb), _p(self.list_ptr), _p(self.list_doc),
                     nd, self.nlist, self.max_list, _p(lists[s:]), nprobe, _p(at(ex_ptr, s)), _p(ex_doc), _p(at(ceil, s)),
                     lo, hi, _IVF_SPLIT_DOCS, _p(docs[s:]), _p(scores[s:]), _p(at(found, s)), _p(ws), ws_bytes, _stream())
        return scores, docs, found

    def search(self, q: torch.Tensor, k: int, nprobe: Optional[int] = None, query_slice: int = 0
               ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``q`` fp32 [nq, dim] -> (scores [nq, k] fp32, docs [nq, k] int32): the top k of the docs in the probed lists;
        unused slots 0 / -1."""
        k = int(k)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"IvfFlatIndex.search: k must be in [1, {K_MAX}]")
        scores, docs, _ = self._search("search", q, 0, k, None, None, query_slice, nprobe, False)
        return scores, docs

    def search_band(self, q: torch.Tensor, lo: int, hi: int, exclude=None, ceiling: Optional[torch.Tensor] = None,
                    chunk_docs: int = 0, query_slice: int = 0, nprobe: Optional[int] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Ranks ``lo .. hi-1`` of each query's ADMISSIBLE docs in its probed lists (``DenseIndex.search_band``'s rules) ->
        (scores, docs, found).  ``chunk_docs`` is accepted for ``DenseIndex``'s signature and ignored."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= K_MAX:
            raise ValueError(f"IvfFlatIndex.search_band: need 0 <= lo < hi <= {K_MAX}")
        return self._search("search_band", q, lo, hi, exclude, ceiling, query_slice, nprobe, True)

    def pair_scores(self, q: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
        """``pairs`` int [n, 2] of (query row, doc id) -> s(q, d) fp32 [n], bit-equal to the scores the searches rank."""
        self._check("pair_scores")
        q = self._rows(q, "pair_scores", "q")
        nq, nd, dev = int(q.shape[0]), self.num_docs, self.device
        pq, pd = check_pairs(pairs, nq, nd, dev, "IvfFlatIndex.pair_scores")
        n = int(pq.numel())
        out = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("snx_dense_pair_scores", _p(q), nq, _p(self.emb), nd, self.dim, _p(pq), _p(pd), n, _p(out), _stream())
        return out

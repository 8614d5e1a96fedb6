"""MaxSim search over a ragged multi-vector store: exact (csrc/mv_search.hip, include/snx.h "multi-vector search") and
through a centroid-interaction candidate pass (csrc/mv_centroid.hip, "multi-vector candidate search"), over bf16 rows or
over a residual-compressed store ("multi-vector residual store")."""
import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from .._lib import call, fn
from ..ops import _p, _stream
from .dense import DENSE_DIM_MAX, DenseIndex
from ._common import (K_MAX, at, cat_or_empty, check_pairs, check_query_slice, cuda_device, exclusion_csr, exclusion_or_null,
                      offsets, search_outputs, workspace)

MV_DIM_MAX = 1024
MV_CHUNK_MIN, MV_CHUNK_MAX = 64, 8192  # docs per chunk of the walk
MV_CENTROIDS_MAX = 4096                # a query group's centroid table has to fit LDS
_MV_ASSIGN_ROWS = 1 << 18              # store rows cast to fp32 per slice of the code assignment
_MV_ROWS_PER_LAUNCH = 1 << 15          # query rows of one launch: 512 query blocks
MV_NBITS = (1, 2, 4)                   # bits per dimension of a residual-compressed store
MV_NPROBE_MAX = 64                     # centroids a query row probes
_MV_QUANTILE_MAX = 1 << 24             # elements torch.quantile takes
MV_FDE_KSIM_MAX = 6                    # 2^k_sim buckets per repetition of a fixed-dimensional encoding
MV_FDE_REPS_MAX = 32
MV_FDE_DPROJ = (16, 32, 64)
_MV_FDE_ROWS = 1 << 18                 # store rows of one encode call
_MV_FDE_SEQS = 1 << 16                 # and its sequences


def _ptr_list(ptr, rows: int, who: str, name: str) -> List[int]:
    """``ptr`` [n + 1] -> host ints; it must ascend from 0 and end within ``rows``."""
    p = torch.as_tensor(ptr)
    if p.dim() != 1 or p.numel() < 1 or p.is_floating_point() or p.dtype == torch.bool:
        raise ValueError(f"{who}: {name} must be an int vector [n + 1]")
    p = [int(v) for v in p.tolist()]
    if p[0] != 0 or any(b < a for a, b in zip(p, p[1:])) or p[-1] > rows:
        raise ValueError(f"{who}: {name} must ascend from 0 and end within the rows")
    return p


class FdeEncoder:
    """MUVERA's fixed-dimensional encoding of ragged bf16 multi-vector rows on the GPU (csrc/mv_fde.hip, include/snx.h
    "multi-vector fixed-dimensional encodings"): one fp32 vector of ``fde_dim = reps * 2^k_sim * d_proj`` per sequence, such
    that <query FDE, document FDE> approximates the MaxSim sum.  Data-oblivious: nothing is trained.

        enc = FdeEncoder(dim, k_sim, reps, d_proj, device, seed=0, planes=None, proj=None)
        fde = enc.encode_documents(mv, mv_ptr)         # fp32 [n, fde_dim]
        qfde = enc.encode_queries(qmv, q_ptr)

    ``dim`` a multiple of 64, at most 1024; ``k_sim`` 0 .. 6; ``reps`` 1 .. 32; ``d_proj`` 16, 32 or 64; ``fde_dim`` at most
    ``DENSE_DIM_MAX``.  ``planes`` [reps, k_sim, dim] and ``proj`` [reps, d_proj, dim] are bf16 (given, or rounded to it).
    Without them, exactly

        planes = torch.randn(reps, k_sim, dim, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)
        proj = (2 * torch.randint(0, 2, (reps, d_proj, dim), generator=torch.Generator().manual_seed(seed + 1)) - 1)
               .to(torch.bfloat16)

    both drawn on the CPU.  The encoding itself is the header's: bit-reproducible, a pure function of the sequence's own
    rows.  Only bf16 rows are encoded; fp32 rows raise."""

    def __init__(self, dim: int, k_sim: int, reps: int, d_proj: int, device, seed: int = 0, planes=None, proj=None):
        for name, v in (("dim", dim), ("k_sim", k_sim), ("reps", reps), ("d_proj", d_proj), ("seed", seed)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"FdeEncoder: {name} must be an int")
        if not 1 <= dim <= MV_DIM_MAX or dim % 64:
            raise ValueError(f"FdeEncoder: dim must be a multiple of 64, at most {MV_DIM_MAX}")
        if not 0 <= k_sim <= MV_FDE_KSIM_MAX or not 1 <= reps <= MV_FDE_REPS_MAX or d_proj not in MV_FDE_DPROJ:
            raise ValueError(f"FdeEncoder: need k_sim in [0, {MV_FDE_KSIM_MAX}], reps in [1, {MV_FDE_REPS_MAX}] and d_proj "
                             f"in {MV_FDE_DPROJ}")
        self.dim, self.k_sim, self.reps, self.d_proj = int(dim), int(k_sim), int(reps), int(d_proj)
        self.fde_dim = self.reps * (1 << self.k_sim) * self.d_proj
        if self.fde_dim > DENSE_DIM_MAX:
            raise ValueError(f"FdeEncoder: fde_dim = reps * 2^k_sim * d_proj = {self.fde_dim} exceeds {DENSE_DIM_MAX}")
        self.device = torch.device(device) if torch.device(device).type != "cuda" else cuda_device(device)
        if (planes is None) != (proj is None):
            raise ValueError("FdeEncoder: give both planes and proj, or neither")
        if planes is None:
            planes = torch.randn(self.reps, self.k_sim, self.dim, generator=torch.Generator().manual_seed(int(seed)))
            proj = 2 * torch.randint(0, 2, (self.reps, self.d_proj, self.dim),
                                     generator=torch.Generator().manual_seed(int(seed) + 1)) - 1
        for name, x, mid in (("planes", planes, self.k_sim), ("proj", proj, self.d_proj)):
            if not isinstance(x, torch.Tensor) or tuple(x.shape) != (self.reps, mid, self.dim) or \
                    not bool(torch.isfinite(x.float()).all()):
                raise ValueError(f"FdeEncoder: {name} must be a finite tensor [{self.reps}, {mid}, {self.dim}]")
        self.planes = planes.to(torch.bfloat16).to(self.device).contiguous()
        self.proj = proj.to(torch.bfloat16).to(self.device).contiguous()
        self._packed: Optional[torch.Tensor] = None               # the MFMA operand, packed by the first encode

    def _geometry(self):
        return self.dim, self.k_sim, self.reps, self.d_proj

    def _encode(self, who: str, mv, ptr, is_query: int) -> torch.Tensor:
        if not isinstance(mv, torch.Tensor) or mv.dim() != 2 or mv.shape[1] != self.dim:
            raise ValueError(f"FdeEncoder.{who}: the rows must be a [rows, {self.dim}] tensor")
        if mv.dtype != torch.bfloat16:
            raise ValueError(f"FdeEncoder.{who}: only bf16 rows are encoded, got {mv.dtype}")
        if mv.device != self.device:
            raise ValueError(f"FdeEncoder.{who}: the rows must be on {self.device}")
        ptr = _ptr_list(ptr, int(mv.shape[0]), f"FdeEncoder.{who}", "ptr")
        if self.device.type != "cuda":
            raise ValueError(f"FdeEncoder.{who}: the encoder needs a GPU")
        mv, n, dev = mv.contiguous(), len(ptr) - 1, self.device
        out = torch.empty((n, self.fde_dim), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if self._packed is None:
                packed = torch.empty(int(fn("snx_mv_fde_packed_bytes")(*self._geometry())), dtype=torch.uint8, device=dev)
                call("snx_mv_fde_pack", _p(self.planes if self.k_sim else None), _p(self.proj), *self._geometry(),
                     _p(packed), _stream())
                self._packed = packed
            s = 0
            while s < n:                                          # slices of whole sequences
                e = s + 1
                while e < n and e - s < _MV_FDE_SEQS and ptr[e + 1] - ptr[s] <= _MV_FDE_ROWS:
                    e += 1
                rows = mv[ptr[s]:ptr[e]]
                hp = (C.c_int64 * (e - s + 1))(*[v - ptr[s] for v in ptr[s:e + 1]])
                ws, ws_bytes = workspace("snx_mv_fde_workspace_bytes", dev, hp, e - s)
                call("snx_mv_fde_encode", _p(rows), int(rows.shape[0]), hp, e - s, _p(self._packed), *self._geometry(),
                     is_query, _p(out[s:]), _p(ws), ws_bytes, _stream())
                s = e
        return out

    def encode_documents(self, mv: torch.Tensor, mv_ptr) -> torch.Tensor:
        """``mv`` bf16 [rows, dim] with ``mv_ptr`` [n + 1] -> the document FDEs, fp32 [n, fde_dim]: bucket means, an empty
        block filled from the nearest code.  A sequence without rows encodes to zeros."""
        return self._encode("encode_documents", mv, mv_ptr, 0)

    def encode_queries(self, qmv: torch.Tensor, q_ptr) -> torch.Tensor:
        """The query FDEs: bucket sums, an empty block 0."""
        return self._encode("encode_queries", qmv, q_ptr, 1)


class MultiVectorIndex:
    """Exact late-interaction (MaxSim) search over the multi-vector rows of a corpus on the GPU (csrc/mv_search.hip):
    which documents score best under ``snx.teacher.maxsim_pairs`` for each query, without listing the pairs.

        index = MultiVectorIndex(dim, device)
        index.add(mv, mv_ptr)          # encode_multivector's store; bf16 or fp32, one dtype per index; doc ids = order of addition
        index.build()
        scores, docs = index.search(qmv, q_ptr, k, chunk_docs=0, query_slice=0)
        scores, docs, found = index.search_band(qmv, q_ptr, lo, hi, exclude=None, chunk_docs=0, query_slice=0)
        s = index.pair_scores(qmv, q_ptr, pairs)

    and the same searches through a candidate pass over centroid codes (2 bytes per document row, not 2 D):

        index.train_centroids(ncentroids, niter=10, seed=0, sample_rows=0)      # after build(); or
        index.set_centroids(c)                                                  # fp32 [nc, dim], unit rows
        a, docs = index.candidates(qmv, q_ptr, ncand, exclude=None, chunk_docs=0, query_slice=0)
        scores, docs = index.search_two_phase(qmv, q_ptr, k, ncand, chunk_docs=0, query_slice=0)
        scores, docs, found = index.search_band_two_phase(qmv, q_ptr, lo, hi, ncand, exclude=None, ...)

    The three take ``nprobe`` (0: every document is walked; 1 .. 64: the probed pass, include/snx.h "multi-vector probed
    candidates").  A query row then looks only at the documents that own a row in one of its ``nprobe`` best centroids
    (key descending, centroid id ascending); the candidates are the best ``ncand`` of the union over the query's rows,
    under the same a(q, d).  ``index.list_ptr`` (int64 [nc + 1]) / ``index.list_docs`` (int32) are the centroids' inverted
    lists, ascending doc ids, built by the first probed call; ``nprobe`` >= nc gives the unprobed result bit for bit.

    ``index.codes`` (uint16 [num_rows]) is every row's best centroid under ``DenseIndex``'s order, ``index.centroids`` the
    centroids in the store's dtype.  a(q, d) = mean over the query's rows of the best bf16-rounded product of the row
    with a centroid of the document; the ``ncand`` best documents by (a descending, doc ascending) are scored exactly, in
    place, and ranked.  With ``ncand`` at least the number of documents with rows the result is the exact search's, bit
    for bit; below it the result is approximate, and every returned score is still s(q, d).  ``add`` invalidates both.

    Or the candidates come from fixed-dimensional encodings (``FdeEncoder``), with no centroids at all:

        index.set_fde(FdeEncoder(dim, k_sim, reps, d_proj, device))             # after build(); bf16 stores
        scores, docs = index.search_two_phase(qmv, q_ptr, k, ncand, fde=True)   # also candidates, search_band_two_phase

    ``index.fde`` (fp32 [num_docs, fde_dim]) holds the documents' FDEs; the candidates are the best ``ncand`` documents with
    rows, outside ``exclude``, by <query FDE, document FDE> under ``DenseIndex``'s chain and order, and the rescore is the
    same exact one.  ``fde=True`` with ``nprobe`` > 0 raises.  ``add`` invalidates the FDEs.

    A bf16 index can drop its rows for ColBERTv2's residual form, ``codes`` plus ``nbits`` bits per dimension:

        index.compress(nbits, cutoffs=None, weights=None, sample_rows=1 << 14, keep_rows=False)   # after the centroids
        rows = index.decompress(row_ids)       # fp32 [n, dim]: centroid[code] + weights[bucket], what the packed form holds

    ``index.residuals`` (uint8 [num_rows, dim * nbits / 8]) holds, for dimension k of a row, the bucket
    #{m : cutoffs[m] < fp32(row[k]) - fp32(centroid[k])} at bit k * nbits of the row's bytes (little-endian).  The
    two-phase searches and ``pair_scores`` then score from the packed form (include/snx.h: the query-centroid product and
    the query-weight product, each an MFMA chain, added once): s(q, d) is the MaxSim of the query with the decompressed
    rows up to fp32 rounding, no longer ``maxsim_pairs``' bits.  ``candidates`` is unchanged.  Without ``keep_rows`` the
    bf16 rows are released, and ``search``, ``search_band``, ``train_centroids`` and ``set_centroids`` raise.

    A compressed index also answers by token retrieval (include/snx.h "multi-vector token retrieval"; XTR's imputed
    similarity), with no candidate list and no second pass:

        scores, docs = index.search_tokens(qmv, q_ptr, k, nprobe, query_slice=0)
        scores, docs, found = index.search_band_tokens(qmv, q_ptr, lo, hi, nprobe, exclude=None, query_slice=0)

    A query row scores only the packed rows whose code is one of its ``nprobe`` (1 .. 64) best centroids; per query row a
    document counts with the best of those scores, or, when it shows the row none, with the row's product with its next
    centroid; the mean over the query's rows ranks the documents that were probed at all.  ``nprobe`` >= nc gives
    ``search_two_phase`` over every document, bit for bit.  ``index.row_list_ptr`` (int64 [nc + 1]) / ``index.row_list``
    (int32 [num_rows]) are the row ids grouped by code, built by the first call after ``compress``.

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
        self.centroids: Optional[torch.Tensor] = None         # [nc, dim] in the store's dtype, as the table kernel reads them
        self.codes: Optional[torch.Tensor] = None             # uint16 [num_rows]: the best centroid of every row
        self._unlist()
        self._uncompress()
        self._unfde()

    def _unfde(self) -> None:
        self.fde: Optional[torch.Tensor] = None               # fp32 [num_docs, fde_dim]: the documents' FDEs (set_fde)
        self._fde_encoder: Optional[FdeEncoder] = None
        self._fde_index: Optional[DenseIndex] = None          # the dense index over them
        self._fde_rowless: Optional[torch.Tensor] = None      # int64: the documents without rows, ascending

    def _unlist(self) -> None:
        self.list_ptr: Optional[torch.Tensor] = None          # int64 [nc + 1]: the inverted lists of the codes,
        self.list_docs: Optional[torch.Tensor] = None         # int32 [list_ptr[nc]]: ascending doc ids per centroid
        self._hlist = None

    def _uncompress(self) -> None:
        self.nbits = 0                                        # 0: not compressed
        self.residuals: Optional[torch.Tensor] = None         # uint8 [num_rows, dim * nbits / 8]
        self.cutoffs: Optional[torch.Tensor] = None           # fp32 [2^nbits - 1], strictly ascending
        self.weights: Optional[torch.Tensor] = None           # fp32 [2^nbits]: the bf16 weights, widened
        self.weights_bf16: Optional[torch.Tensor] = None
        self._unrows()

    def _unrows(self) -> None:
        self.row_list_ptr: Optional[torch.Tensor] = None      # int64 [nc + 1]: the rows grouped by code (search_tokens),
        self.row_list: Optional[torch.Tensor] = None          # int32 [num_rows]: ascending row ids per centroid
        self._row_doc: Optional[torch.Tensor] = None          # int32 [num_rows]: the document of every row
        self._hrows = None

    @property
    def num_docs(self) -> int:
        return len(self._ptr) - 1

    @property
    def num_rows(self) -> int:
        return self._ptr[-1]

    @property
    def built(self) -> bool:
        return self.rows is not None or self.residuals is not None

    def _need_rows(self, who: str) -> None:
        if self.rows is None and self.residuals is not None:
            raise RuntimeError(f"MultiVectorIndex.{who}: the bf16 rows were released by compress(); it needs "
                               "compress(..., keep_rows=True)")

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
        self._need_rows("add")                                # the earlier rows are gone: the store cannot be rebuilt
        mv, ptr = self._store(mv, mv_ptr, "add", "mv")
        if self.num_docs + len(ptr) - 1 >= 2 ** 31:
            raise ValueError("MultiVectorIndex: doc ids are int32")
        self.dtype = mv.dtype
        self._parts.append(mv[:ptr[-1]])
        self._ptr += [self._ptr[-1] + v for v in ptr[1:]]
        self.rows = None                                      # a new batch invalidates a built index
        self.centroids = self.codes = None                    # and its codes
        self._unlist()                                        # and their lists
        self._uncompress()                                    # and their residuals
        self._unfde()                                         # and the FDEs

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
        self._need_rows("search")
        qmv, ptr, chunk_docs = self._queries("search", qmv, q_ptr, chunk_docs, query_slice)
        return self._run(qmv, ptr, None, None, 0, k, chunk_docs, query_slice, False)[:2]

    def search_band(self, qmv: torch.Tensor, q_ptr, lo: int, hi: int, exclude=None, chunk_docs: int = 0,
                    query_slice: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Ranks ``lo .. hi-1`` (0-based) of each query's ADMISSIBLE documents -- with rows, not in ``exclude[q]`` -> (scores
        [nq, hi-lo] fp32, docs [nq, hi-lo] int32, found [nq] int32); ``exclude`` as for ``DenseIndex.search_band``."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= K_MAX:
            raise ValueError(f"MultiVectorIndex.search_band: need 0 <= lo < hi <= {K_MAX}")
        self._need_rows("search_band")
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
        if self.residuals is not None:
            return self._pair_scores_residual(qmv, ptr, pq, pd)
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

    # -------------------------------------------------------------------------------------------- candidate search
    def _quantizer(self, who: str, nc: int, niter: int = 0, seed: int = 0):
        """The dense helpers of ``IvfFlatIndex`` (k-means step, nearest centroid) over this index's dim and device."""
        from .ivf import IvfFlatIndex
        self._need_rows(who)
        if not self.built:
            raise RuntimeError(f"MultiVectorIndex.{who}: call build() first")
        if self.num_rows == 0:
            raise ValueError(f"MultiVectorIndex.{who}: the index has no rows")
        if self.device.type != "cuda":
            raise ValueError(f"MultiVectorIndex.{who}: the code assignment needs the index on a GPU")
        return IvfFlatIndex(self.dim, nc, self.device, niter=niter, seed=seed)

    def _assign(self, quantizer, c: torch.Tensor) -> None:
        """``centroids`` = ``c`` in the store's dtype; ``codes`` = every row's best of those (ties: the lowest)."""
        self.centroids = c.to(self.dtype).contiguous()
        seen = self.centroids.float()
        codes = torch.empty(self.num_rows, dtype=torch.int32, device=self.device)
        for s in range(0, self.num_rows, _MV_ASSIGN_ROWS):
            codes[s:s + _MV_ASSIGN_ROWS] = quantizer._best(self.rows[s:s + _MV_ASSIGN_ROWS].float(), seen, 1)[1].reshape(-1)
        self.codes = codes.to(torch.uint16)
        self._unlist()                                        # lists of other codes
        self._uncompress()                                    # residuals of other codes

    def train_centroids(self, ncentroids: int, niter: int = 10, seed: int = 0, sample_rows: int = 0) -> "MultiVectorIndex":
        """Spherical k-means over the store's rows as fp32 (``sample_rows`` > 0: over that many evenly spaced rows), by
        ``IvfFlatIndex``'s procedure and seed rule; then the codes.  ``ncentroids`` is clamped to the rows trained on."""
        if isinstance(ncentroids, bool) or not isinstance(ncentroids, (int, np.integer)) or \
                not 1 <= int(ncentroids) <= MV_CENTROIDS_MAX:
            raise ValueError(f"MultiVectorIndex.train_centroids: ncentroids must be an int in [1, {MV_CENTROIDS_MAX}]")
        if int(sample_rows) < 0:
            raise ValueError("MultiVectorIndex.train_centroids: sample_rows must be >= 0 (0: every row)")
        n = self.num_rows if self.built else 0
        m = min(int(sample_rows), n) if int(sample_rows) > 0 else n
        nc = min(int(ncentroids), max(m, 1))
        quantizer = self._quantizer("train_centroids", nc, niter, seed)
        x = self.rows if m == n else self.rows[(torch.arange(m, device=self.device) * n) // m]
        self._assign(quantizer, quantizer._kmeans(x.float(), nc))
        return self

    def set_centroids(self, c: torch.Tensor) -> "MultiVectorIndex":
        """``c`` fp32 [nc, dim] with unit rows, 1 <= nc <= 4096, on the index's device: the centroids, without training."""
        if not isinstance(c, torch.Tensor) or c.dtype != torch.float32 or c.dim() != 2 or c.shape[1] != self.dim or \
                not 1 <= c.shape[0] <= MV_CENTROIDS_MAX:
            raise ValueError(f"MultiVectorIndex.set_centroids: c must be fp32 [nc, {self.dim}], 1 <= nc <= {MV_CENTROIDS_MAX}")
        if c.device != self.device:
            raise ValueError(f"MultiVectorIndex.set_centroids: c must be on {self.device}")
        if not bool(torch.isfinite(c).all()):
            raise ValueError("MultiVectorIndex.set_centroids: c must be finite")
        self._assign(self._quantizer("set_centroids", int(c.shape[0])), c)
        return self

    def _two_phase(self, who: str, ncand, hi: int, nprobe=0, fde: bool = False) -> int:
        if fde and nprobe:
            raise ValueError(f"MultiVectorIndex.{who}: fde=True takes its candidates from the dense index over the FDEs; "
                             "nprobe must be 0")
        if isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or not 0 <= int(nprobe) <= MV_NPROBE_MAX:
            raise ValueError(f"MultiVectorIndex.{who}: nprobe must be an int in [0, {MV_NPROBE_MAX}] (0: no probing)")
        if isinstance(ncand, bool) or not isinstance(ncand, (int, np.integer)) or not 1 <= int(ncand) <= K_MAX:
            raise ValueError(f"MultiVectorIndex.{who}: ncand must be an int in [1, {K_MAX}]")
        if hi > int(ncand):
            raise ValueError(f"MultiVectorIndex.{who}: ranks up to {hi} need ncand >= {hi}")
        if fde and self._fde_index is None:
            raise RuntimeError(f"MultiVectorIndex.{who}: call set_fde() first")
        if not fde and self.built and self.codes is None:
            raise RuntimeError(f"MultiVectorIndex.{who}: call train_centroids() or set_centroids() first")
        return int(ncand)

    def _launches(self, qmv, ptr, query_slice):
        """Per launch: (first query, queries, their rows, their host pointer array)."""
        for s, m in self._slices(ptr, query_slice):
            yield s, m, qmv[ptr[s]:ptr[s + m]], (C.c_int64 * (m + 1))(*[v - ptr[s] for v in ptr[s:s + m + 1]])

    def _lists(self) -> None:
        """``list_ptr`` / ``list_docs`` from the codes (csrc's ``mvp_list_*`` kernels), once per code assignment."""
        if self.list_ptr is not None:
            return
        nd, dev, nc = self.num_docs, self.device, int(self.centroids.shape[0])
        list_ptr = torch.empty(nc + 1, dtype=torch.int64, device=dev)
        docs = torch.empty(max(self.num_rows, 1), dtype=torch.int32, device=dev)     # a row adds at most one entry
        with torch.cuda.device(dev):
            ws, ws_bytes = workspace("snx_mv_lists_workspace_bytes", dev, nd, nc)
            call("snx_mv_lists_build", _p(self.codes), self.num_rows, self._hptr, nd, nc, _p(list_ptr), _p(docs), _p(ws),
                 ws_bytes, _stream())
        host = list_ptr.tolist()
        self.list_ptr, self.list_docs = list_ptr, docs[:host[-1]].clone()
        self._hlist = (C.c_int64 * (nc + 1))(*host)

    def _candidates(self, qmv, ptr, ex_ptr, ex_doc, ncand: int, chunk_docs: int, query_slice: int, nprobe: int = 0):
        nq, nd, dev, nc = len(ptr) - 1, self.num_docs, self.device, int(self.centroids.shape[0])
        approx, docs, _, _ = search_outputs(nq, ncand, dev, False)
        if nprobe:
            self._lists()
        with torch.cuda.device(dev):
            for s, m, rows, hq in self._launches(qmv, ptr, query_slice):
                if nprobe:
                    ws, ws_bytes = workspace("snx_mv_candidates_probed_workspace_bytes", dev, hq, m, nd, nc, ncand,
                                             chunk_docs, nprobe)
                    call("snx_mv_candidates_probed", _p(self.codes), self.num_rows, self._hptr, nd, _p(self.centroids), nc,
                         _p(rows), int(self.dtype == torch.float32), self.dim, int(rows.shape[0]), hq, m, _p(at(ex_ptr, s)),
                         _p(ex_doc), ncand, chunk_docs, self._hlist, _p(self.list_docs), int(self.list_docs.numel()), nprobe,
                         _p(docs[s:]), _p(approx[s:]), _p(ws), ws_bytes, _stream())
                    continue
                ws, ws_bytes = workspace("snx_mv_candidates_workspace_bytes", dev, hq, m, nd, nc, ncand, chunk_docs)
                call("snx_mv_candidates", _p(self.codes), self.num_rows, self._hptr, nd, _p(self.centroids), nc, _p(rows),
                     int(self.dtype == torch.float32), self.dim, int(rows.shape[0]), hq, m, _p(at(ex_ptr, s)), _p(ex_doc),
                     ncand, chunk_docs, _p(docs[s:]), _p(approx[s:]), _p(ws), ws_bytes, _stream())
        return approx, docs

    def _rescore(self, qmv, ptr, cand: torch.Tensor, lo: int, hi: int, query_slice: int):
        nq, nd, dev, ncand = len(ptr) - 1, self.num_docs, self.device, int(cand.shape[1])
        scores, docs, _, _ = search_outputs(nq, hi - lo, dev, False)
        found = torch.empty(nq, dtype=torch.int32, device=dev)
        if self.residuals is not None:
            self._rescore_residual(qmv, ptr, cand, lo, hi, query_slice, docs, scores, found, None)
            return scores, docs, found
        with torch.cuda.device(dev):
            for s, m, rows, hq in self._launches(qmv, ptr, query_slice):
                ws, ws_bytes = workspace("snx_mv_rescore_workspace_bytes", dev, hq, m, nd, ncand)
                call("snx_mv_rescore", _p(self.rows), _p(rows), int(self.dtype == torch.float32), self.dim, self.num_rows,
                     self._hptr, nd, int(rows.shape[0]), hq, m, _p(cand[s:]), ncand, lo, hi, _p(docs[s:]), _p(scores[s:]),
                     _p(found[s:]), _p(ws), ws_bytes, _stream())
        return scores, docs, found

    def candidates(self, qmv: torch.Tensor, q_ptr, ncand: int, exclude=None, chunk_docs: int = 0, query_slice: int = 0,
                   nprobe: int = 0, fde: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ``ncand`` best documents of each query under the centroid score a(q, d) (the class docstring) among the
        documents with rows that are not in ``exclude[q]`` -> (a [nq, ncand] fp32, docs [nq, ncand] int32); unused slots
        0 / -1.  ``nprobe`` > 0: among the probed documents only.  ``fde=True`` (after ``set_fde``): the score is the inner
        product of the query's FDE with the document's instead, under ``DenseIndex.search_band``'s chain and order;
        ``chunk_docs`` is then unused."""
        ncand = self._two_phase("candidates", ncand, 0, nprobe, fde)
        qmv, ptr, chunk_docs = self._queries("candidates", qmv, q_ptr, chunk_docs, query_slice)
        if fde:
            return self._fde_candidates(qmv, ptr, exclude, ncand, query_slice)
        ex_ptr, ex_doc = exclusion_or_null(exclude, len(ptr) - 1, self.num_docs, self.device)
        return self._candidates(qmv, ptr, ex_ptr, ex_doc, ncand, chunk_docs, query_slice, int(nprobe))

    def search_two_phase(self, qmv: torch.Tensor, q_ptr, k: int, ncand: int, chunk_docs: int = 0, query_slice: int = 0,
                         nprobe: int = 0, fde: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """``search`` over the ``ncand`` >= ``k`` candidates of ``candidates``, scored exactly."""
        k = int(k)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"MultiVectorIndex.search_two_phase: k must be in [1, {K_MAX}]")
        ncand = self._two_phase("search_two_phase", ncand, k, nprobe, fde)
        qmv, ptr, chunk_docs = self._queries("search_two_phase", qmv, q_ptr, chunk_docs, query_slice)
        if fde:
            _, cand = self._fde_candidates(qmv, ptr, None, ncand, query_slice)
        else:
            _, cand = self._candidates(qmv, ptr, None, None, ncand, chunk_docs, query_slice, int(nprobe))
        return self._rescore(qmv, ptr, cand, 0, k, query_slice)[:2]

    def search_band_two_phase(self, qmv: torch.Tensor, q_ptr, lo: int, hi: int, ncand: int, exclude=None,
                              chunk_docs: int = 0, query_slice: int = 0, nprobe: int = 0, fde: bool = False
                              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``search_band`` over the ``ncand`` >= ``hi`` candidates of ``candidates`` (``exclude`` applies there), scored
        exactly."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= K_MAX:
            raise ValueError(f"MultiVectorIndex.search_band_two_phase: need 0 <= lo < hi <= {K_MAX}")
        ncand = self._two_phase("search_band_two_phase", ncand, hi, nprobe, fde)
        qmv, ptr, chunk_docs = self._queries("search_band_two_phase", qmv, q_ptr, chunk_docs, query_slice)
        if fde:
            _, cand = self._fde_candidates(qmv, ptr, exclude, ncand, query_slice)
            return self._rescore(qmv, ptr, cand, lo, hi, query_slice)
        ex_ptr, ex_doc = exclusion_or_null(exclude, len(ptr) - 1, self.num_docs, self.device)
        _, cand = self._candidates(qmv, ptr, ex_ptr, ex_doc, ncand, chunk_docs, query_slice, int(nprobe))
        return self._rescore(qmv, ptr, cand, lo, hi, query_slice)

    # -------------------------------------------------------------------------------------------- fixed-dimensional encodings
    def set_fde(self, encoder: FdeEncoder, slice_docs: int = 1 << 14) -> "MultiVectorIndex":
        """After ``build()``: ``index.fde`` = ``encoder.encode_documents`` of the store, ``slice_docs`` documents at a time,
        and a ``DenseIndex`` over it; ``fde=True`` then draws the candidates of the two-phase searches from that index.  No
        centroids are needed.  bf16 stores only; ``add`` invalidates it."""
        who = "MultiVectorIndex.set_fde"
        if not isinstance(encoder, FdeEncoder) or encoder.dim != self.dim or encoder.device != self.device:
            raise ValueError(f"{who}: encoder must be an FdeEncoder of dim {self.dim} on {self.device}")
        if self.dtype == torch.float32:
            raise ValueError(f"{who}: an fp32 index is kept for exactness; only a bf16 index is encoded")
        if isinstance(slice_docs, bool) or int(slice_docs) < 1:
            raise ValueError(f"{who}: slice_docs must be positive")
        self._need_rows("set_fde")
        if not self.built:
            raise RuntimeError(f"{who}: call build() first")
        nd, ptr = self.num_docs, self._ptr
        fde = torch.empty((nd, encoder.fde_dim), dtype=torch.float32, device=self.device)
        for s in range(0, nd, int(slice_docs)):
            e = min(nd, s + int(slice_docs))
            fde[s:e] = encoder.encode_documents(self.rows[ptr[s]:ptr[e]], [v - ptr[s] for v in ptr[s:e + 1]])
        lens = torch.tensor(ptr).diff()
        self.fde, self._fde_encoder = fde, encoder
        self._fde_rowless = torch.nonzero(lens == 0).flatten()
        self._fde_index = DenseIndex(encoder.fde_dim, self.device)
        self._fde_index.add(fde)
        self._fde_index.build()
        return self

    def _fde_candidates(self, qmv, ptr, exclude, ncand: int, query_slice: int):
        """The best ``ncand`` admissible documents by <query FDE, document FDE>: ``DenseIndex.search_band`` with the
        documents without rows (their FDE is zero, their score 0) added to every exclusion row."""
        nq, nd = len(ptr) - 1, self.num_docs
        if self._fde_rowless.numel():
            ex_ptr, ex_doc = exclusion_csr(exclude if exclude is not None else [[]] * nq, nq, nd, "cpu")
            row = torch.repeat_interleave(torch.arange(nq), ex_ptr.diff())
            key = torch.unique(torch.cat([row * nd + ex_doc.long(),
                                          (torch.arange(nq)[:, None] * nd + self._fde_rowless[None, :]).reshape(-1)]))
            exclude = (offsets(torch.bincount(key // nd, minlength=nq)), (key % nd).to(torch.int32))
        qfde = self._fde_encoder.encode_queries(qmv[:ptr[-1]], ptr)
        scores, docs, _ = self._fde_index.search_band(qfde, 0, ncand, exclude=exclude, query_slice=query_slice)
        return scores, docs

    # -------------------------------------------------------------------------------------------- residual store
    def compress(self, nbits: int, cutoffs=None, weights=None, sample_rows: int = 1 << 14, keep_rows: bool = False
                 ) -> "MultiVectorIndex":
        """Packs the bf16 rows into ``residuals`` (the class docstring) by csrc's ``mvr_encode_kernel``, a slice of rows at
        a time.  ``cutoffs`` [2^nbits - 1] strictly ascending and ``weights`` [2^nbits] (rounded to bf16); without them,
        ColBERTv2's quantiles of the residuals of ``sample_rows`` evenly spaced rows (at most 2^24 / dim: what
        ``torch.quantile`` takes): cutoffs at m / 2^nbits, weights at (m + 0.5) / 2^nbits.  ``keep_rows=False`` releases
        the bf16 rows."""
        who = "MultiVectorIndex.compress"
        if isinstance(nbits, bool) or not isinstance(nbits, (int, np.integer)) or int(nbits) not in MV_NBITS:
            raise ValueError(f"{who}: nbits must be 1, 2 or 4")
        nbits = int(nbits)
        if self.dtype == torch.float32:
            raise ValueError(f"{who}: an fp32 index is kept for exactness; only a bf16 index is compressed")
        self._need_rows("compress")
        if not self.built:
            raise RuntimeError(f"{who}: call build() first")
        if self.codes is None:
            raise RuntimeError(f"{who}: call train_centroids() or set_centroids() first")
        if (cutoffs is None) != (weights is None):
            raise ValueError(f"{who}: give both cutoffs and weights, or neither")
        if isinstance(sample_rows, bool) or int(sample_rows) < 1:
            raise ValueError(f"{who}: sample_rows must be positive")
        if cutoffs is not None:
            cutoffs = torch.as_tensor(cutoffs, dtype=torch.float32).reshape(-1)
            weights = torch.as_tensor(weights, dtype=torch.float32).reshape(-1)
            if cutoffs.numel() != (1 << nbits) - 1 or weights.numel() != 1 << nbits:
                raise ValueError(f"{who}: nbits = {nbits} takes {(1 << nbits) - 1} cutoffs and {1 << nbits} weights")
            if not bool(torch.isfinite(cutoffs).all()) or not bool(torch.isfinite(weights).all()) or \
                    not bool((cutoffs[1:] > cutoffs[:-1]).all()):
                raise ValueError(f"{who}: cutoffs must be finite and strictly ascending, weights finite")
        if self.device.type != "cuda":
            raise ValueError(f"{who}: the codec needs the index on a GPU")
        n, dev = self.num_rows, self.device
        if cutoffs is None:
            m = min(int(sample_rows), _MV_QUANTILE_MAX // self.dim, n)
            pick = (torch.arange(m, device=dev) * n) // m
            res = (self.rows[pick].float() - self.centroids[self._codes_of(pick)].float()).reshape(-1)
            steps = torch.arange(1 << nbits, device=dev, dtype=torch.float32) / (1 << nbits)
            cutoffs, weights = torch.quantile(res, steps[1:]), torch.quantile(res, steps + 0.5 / (1 << nbits))
            if not bool((cutoffs[1:] > cutoffs[:-1]).all()):
                raise ValueError(f"{who}: the residuals' quantiles do not ascend strictly; give cutoffs and weights")
        self.cutoffs = cutoffs.to(dev).contiguous()
        self.weights_bf16 = weights.to(dev).to(torch.bfloat16).contiguous()
        self.weights = self.weights_bf16.float()
        packed = torch.empty((n, self.dim * nbits // 8), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            for s in range(0, n, _MV_ASSIGN_ROWS):
                rows = self.rows[s:s + _MV_ASSIGN_ROWS]
                call("snx_mv_residual_encode", _p(rows), int(rows.shape[0]), _p(self.codes[s:]), _p(self.centroids),
                     int(self.centroids.shape[0]), self.dim, nbits, _p(self.cutoffs), _p(packed[s:]), _stream())
        self.residuals, self.nbits = packed, nbits
        self._unrows()                                        # the row lists are built once per compression
        if not keep_rows:
            self.rows, self._parts = None, []
        return self

    def _codes_of(self, row_ids: torch.Tensor) -> torch.Tensor:
        return self.codes.view(torch.int16)[row_ids].long() & 0xFFFF

    def decompress(self, row_ids) -> torch.Tensor:
        """fp32 [n, dim] = fp32(centroid[code]) + weights[bucket] for the rows named: what the packed form holds."""
        if self.residuals is None:
            raise RuntimeError("MultiVectorIndex.decompress: call compress() first")
        ids = torch.as_tensor(row_ids, device=self.device).long().reshape(-1)
        if ids.numel() and not bool(((ids >= 0) & (ids < self.num_rows)).all()):
            raise ValueError(f"MultiVectorIndex.decompress: row ids must lie in [0, {self.num_rows})")
        shifts = torch.arange(0, 8, self.nbits, device=self.device, dtype=torch.int32)
        buckets = (self.residuals[ids].to(torch.int32)[:, :, None] >> shifts) & ((1 << self.nbits) - 1)
        return self.centroids[self._codes_of(ids)].float() + self.weights[buckets.reshape(ids.numel(), self.dim).long()]

    def _rescore_residual(self, qmv, ptr, cand, lo, hi, query_slice, docs, scores, found, raw) -> None:
        nd, dev, ncand, nc = self.num_docs, self.device, int(cand.shape[1]), int(self.centroids.shape[0])
        with torch.cuda.device(dev):
            for s, m, rows, hq in self._launches(qmv, ptr, query_slice):
                ws, ws_bytes = workspace("snx_mv_rescore_residual_workspace_bytes", dev, hq, m, nd, nc, ncand)
                call("snx_mv_rescore_residual", _p(self.codes), _p(self.residuals), _p(self.centroids),
                     _p(self.weights_bf16), nc, self.nbits, _p(rows), 0, self.dim, self.num_rows, self._hptr, nd,
                     int(rows.shape[0]), hq, m, _p(cand[s:]), ncand, lo, hi, _p(docs[s:]), _p(scores[s:]), _p(found[s:]),
                     _p(at(raw, s)), _p(ws), ws_bytes, _stream())

    # -------------------------------------------------------------------------------------------- token retrieval
    def _row_lists(self) -> None:
        """``row_list_ptr`` / ``row_list`` (every row id grouped by its code, ascending within a centroid) and the
        row-to-document map, once per compression: a stable device sort, plumbing in front of the ``mvt_`` kernels."""
        if self.row_list_ptr is not None:
            return
        nc, dev = int(self.centroids.shape[0]), self.device
        codes = self._codes_of(torch.arange(self.num_rows, device=dev))
        ptr = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.bincount(codes, minlength=nc).cumsum(0)
        lens = torch.tensor(self._ptr, dtype=torch.int64).diff().to(dev)
        self.row_list = torch.sort(codes, stable=True).indices.to(torch.int32).contiguous()
        self._row_doc = torch.repeat_interleave(torch.arange(self.num_docs, dtype=torch.int32, device=dev), lens).contiguous()
        self._hrows = (C.c_int64 * (nc + 1))(*ptr.tolist())
        self.row_list_ptr = ptr

    def _tokens(self, who: str, qmv, q_ptr, lo: int, hi: int, nprobe, exclude, query_slice):
        if isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or not 1 <= int(nprobe) <= MV_NPROBE_MAX:
            raise ValueError(f"MultiVectorIndex.{who}: nprobe must be an int in [1, {MV_NPROBE_MAX}]")
        if self.dtype == torch.float32:
            raise ValueError(f"MultiVectorIndex.{who}: token retrieval reads the compressed store; an fp32 index has none")
        if self.built and self.residuals is None:
            raise RuntimeError(f"MultiVectorIndex.{who}: call compress() first; token retrieval scores the packed rows")
        qmv, ptr, _ = self._queries(who, qmv, q_ptr, 0, query_slice)
        nq, nd, dev, nc = len(ptr) - 1, self.num_docs, self.device, int(self.centroids.shape[0])
        ex_ptr, ex_doc = exclusion_or_null(exclude, nq, nd, dev)
        self._row_lists()
        scores, docs, _, _ = search_outputs(nq, hi - lo, dev, False)
        found = torch.empty(nq, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            for s, m, rows, hq in self._launches(qmv, ptr, query_slice):
                ws, ws_bytes = workspace("snx_mv_token_search_workspace_bytes", dev, hq, m, nd, self.num_rows, nc,
                                         int(nprobe), hi)
                call("snx_mv_token_search", _p(self.codes), _p(self.residuals), _p(self.centroids), _p(self.weights_bf16),
                     nc, self.nbits, _p(rows), 0, self.dim, self.num_rows, self._hptr, nd, self._hrows, _p(self.row_list),
                     _p(self._row_doc), int(rows.shape[0]), hq, m, _p(at(ex_ptr, s)), _p(ex_doc), int(nprobe), lo, hi,
                     _p(docs[s:]), _p(scores[s:]), _p(found[s:]), _p(ws), ws_bytes, _stream())
        return scores, docs, found

    def search_tokens(self, qmv: torch.Tensor, q_ptr, k: int, nprobe: int, query_slice: int = 0
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Token retrieval over the compressed store (include/snx.h "multi-vector token retrieval") -> (scores [nq, k]
        fp32, docs [nq, k] int32): the top k of the documents that own a row in one of the ``nprobe`` best centroids of
        some query row, by x(q, d) -- per query row the best packed-form score among those rows, or the row's next-best
        centroid product when the document shows it none.  No candidate list, no second pass."""
        k = int(k)
        if not 1 <= k <= K_MAX:
            raise ValueError(f"MultiVectorIndex.search_tokens: k must be in [1, {K_MAX}]")
        return self._tokens("search_tokens", qmv, q_ptr, 0, k, nprobe, None, query_slice)[:2]

    def search_band_tokens(self, qmv: torch.Tensor, q_ptr, lo: int, hi: int, nprobe: int, exclude=None,
                           query_slice: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Ranks ``lo .. hi-1`` of ``search_tokens``' order among the probed documents outside ``exclude[q]`` -> (scores,
        docs, found [nq] int32)."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= K_MAX:
            raise ValueError(f"MultiVectorIndex.search_band_tokens: need 0 <= lo < hi <= {K_MAX}")
        return self._tokens("search_band_tokens", qmv, q_ptr, lo, hi, nprobe, exclude, query_slice)

    def _pair_scores_residual(self, qmv, ptr, pq: List[int], pd: List[int]) -> torch.Tensor:
        """The pairs grouped per query into candidate rows of at most ``K_MAX`` slots; the scores are ``raw_score``'s, so
        they are the bits the searches rank.  A document without rows scores 0.0, as on the uncompressed index."""
        nq, dev = len(ptr) - 1, self.device
        out = torch.zeros(len(pd), dtype=torch.float32, device=dev)
        slot, todo = [0] * nq, list(range(len(pd)))
        while todo:                                           # one pass per K_MAX pairs of the busiest query
            width = min(K_MAX, max(sum(1 for i in todo if pq[i] == q) for q in {pq[i] for i in todo}))
            cand = torch.full((nq, width), -1, dtype=torch.int32)
            used, where, rest = [0] * nq, [], []
            for i in todo:
                if used[pq[i]] < width:
                    cand[pq[i], used[pq[i]]] = pd[i]
                    where.append((i, pq[i] * width + used[pq[i]]))
                    used[pq[i]] += 1
                else:
                    rest.append(i)
            cand = cand.to(dev)
            scores, docs, _, _ = search_outputs(nq, 1, dev, False)
            found = torch.empty(nq, dtype=torch.int32, device=dev)
            raw = torch.empty((nq, width), dtype=torch.float32, device=dev)
            self._rescore_residual(qmv, ptr, cand, 0, 1, 0, docs, scores, found, raw)
            out[torch.tensor([i for i, _ in where], device=dev)] = raw.reshape(-1)[torch.tensor([j for _, j in where], device=dev)]
            todo = rest
        return out

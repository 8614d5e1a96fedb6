"""Ranked lists against multi-relevant qrels and the bootstrap (csrc/qrels.hip, include/snx.h "relevance judgments")."""
import ctypes as C
from typing import Tuple

import numpy as np
import torch

from .._abi import CONSTANTS
from .._lib import SnxError, call
from ..ops import _p, _stream
from ._common import csr_rows, cuda_device

RANKED_R_MAX = 4096
CUTOFFS_MAX = 8
BOOTSTRAP_M_MAX = 16
BOOTSTRAP_SEGMENT = CONSTANTS["SNX_BOOTSTRAP_SEGMENT"]       # part of the summation order


def relevance_csr(relevant, nq: int, nd: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Relevance rows (qrels) -> (ptr int64 [nq+1], docs int32) on ``device``, every row sorted ascending and
    deduplicated.  ``relevant`` takes the two forms of ``exclusion_csr``: a list of ``nq`` per-query doc-id lists, or a
    CSR pair, the tuple (ptr [nq+1], docs) of int tensors whose ptr starts at 0, does not decrease and ends at len(docs).
    Unlike an exclusion row a relevance row may name ids outside [0, nd) (a judged doc that is not in the corpus): they
    stay in the row and the kernels skip them (include/snx.h "relevance judgments").  Ids must fit in int32."""
    nq, nd = int(nq), int(nd)
    if nq < 0 or nd < 0:
        raise ValueError("relevance rows: nq and nd must be >= 0")
    return csr_rows(relevant, nq, nd, device, "relevance", False)


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
    host = (C.c_int32 * len(cuts))(*cuts)
    with torch.cuda.device(dev):
        call("snx_ranked_relevance", _p(docs), int(nq), int(R), int(nd), _p(rel_ptr), _p(rel_doc),
             C.cast(host, C.c_void_p), len(cuts), _p(disc), _p(first), _p(hits), _p(dcg), _stream())
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
            raise SnxError(f"snx_bootstrap_means failed: SNX_E_ARG (a resample index lies outside [0, {n}))")
        idx = idx.astype(np.int32)
    dev = cuda_device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError("bootstrap_means: runs on a GPU")
    nb = int(idx.shape[0])
    vals = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    didx = torch.from_numpy(np.ascontiguousarray(idx)).to(dev)
    out = torch.empty((nb, M), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        call("snx_bootstrap_means", _p(vals), int(n), int(M), _p(didx), nb, _p(out), _stream())
    return out

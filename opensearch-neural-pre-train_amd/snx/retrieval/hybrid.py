"""The lexical BM25 baseline and the rank fusion (csrc/hybrid.hip, include/snx.h "BM25 baseline and rank fusion")."""
import ctypes as C
from typing import Optional

import numpy as np
import torch

from .._abi import CONSTANTS
from .._lib import call, fn
from ..ops import _chk, _p, _stream
from ._common import K_MAX, cat_or_empty, check_targets, cuda_device, offsets
from .sparse import SparseIndex

FUSE_METHODS = {k: CONSTANTS["SNX_FUSE_" + k.upper()] for k in ("rrf", "weighted_rrf", "linear")}
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
        call("snx_term_counts", _p(ids), _p(mask), _p(allowed), n, S, int(allowed.numel()), _p(term), _p(tf), _p(cnt),
             _p(length), _stream())
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
        self.device = cuda_device(device)
        self._cnt, self._term, self._tf, self._len = [], [], [], []     # per batch, as term_counts returns them
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
            call("snx_bm25_doc_freq", _p(terms), int(terms.numel()), self.V, _p(self.doc_freq), _stream())
        self._cnt.append(cnt.long())
        self._term.append(terms)
        self._tf.append(tf[live].contiguous())
        self._len.append(length)
        self.num_docs += int(cnt.numel())
        self.index = None                                     # a new batch invalidates a built index

    def build(self) -> "Bm25Index":
        dev, N, V = self.device, self.num_docs, self.V
        cnt = cat_or_empty(self._cnt, torch.long, dev)
        terms = cat_or_empty(self._term, torch.int32, dev)
        tf = cat_or_empty(self._tf, torch.int32, dev)
        self.doc_len = cat_or_empty(self._len, torch.int32, dev)
        self._cnt, self._term, self._tf, self._len = [cnt], [terms], [tf], [self.doc_len]
        idf = bm25_idf(self.doc_freq.cpu().numpy(), N)        # the log on the host: V entries, one libm
        total = int(self.doc_len.long().sum())                # exact integer sum
        self.avgdl = float(np.float64(total) / np.float64(N)) if N else 0.0
        self.idf = torch.from_numpy(idf).to(dev)
        ptr = offsets(cnt)
        w = torch.empty(terms.numel(), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("snx_bm25_weights", _p(ptr), _p(terms), _p(tf), _p(self.doc_len), _p(self.idf), N, int(terms.numel()),
                 V, self.avgdl, self.k1, self.b, _p(w), _stream())
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
    tgt = check_targets(targets, nq, None, dev, "fuse_ranked")     # any id: a target outside every list ranks 0
    out_s = torch.empty((nq, top_k), dtype=torch.float64, device=dev)
    out_d = torch.empty((nq, top_k), dtype=torch.int32, device=dev)
    total = torch.empty(nq, dtype=torch.int32, device=dev)
    rank = torch.empty(nq, dtype=torch.int32, device=dev) if tgt is not None else None
    host = (C.c_double * len(prm))(*prm)
    with torch.cuda.device(dev):
        call("snx_fuse_ranked", _p(docs), _p(scores), L, int(nq), int(R), FUSE_METHODS[method],
             C.cast(host, C.c_void_p), _p(tgt), top_k, _p(out_d), _p(out_s), _p(total), _p(rank), _stream())
    return out_s, out_d, rank, total

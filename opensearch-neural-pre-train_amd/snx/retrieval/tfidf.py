"""Character n-gram TF-IDF on the GPU (csrc/tfidf.hip, include/snx.h "Character n-gram TF-IDF"): the vectorizer of the
reference's lexical hard-negative mining (ref:scripts/mine_hard_negatives.py:141-146), scikit-learn's
``TfidfVectorizer(analyzer="char_wb", ngram_range=(2, 3), max_features=30000, sublinear_tf=True)`` with L2-normalised rows.

The host's part is the text (Python's ``lower`` and ``split``, the words joined by one U+0020, the rows as a CSR of code
points), the one device-wide sort of the fit (``torch.unique`` over the corpus's row keys) and the two logarithms (idf and
the sublinear tf table, numpy).  N-gram extraction, counting, vocabulary lookup, weighting and normalisation are kernels."""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .._abi import CONSTANTS
from .._lib import call
from .._text import code_point_csr, csr_to_device
from ..ops import _p, _stream
from ._common import cat_or_empty, cuda_device, offsets, search_outputs, workspace
from .sparse import SparseIndex

LDS_KEYS = CONSTANTS["SNX_TFIDF_LDS_KEYS"]        # slots of a row the LDS form sorts
NGRAM_MAX = 3


def check_ngram_range(ngram_range, who: str = "TfidfIndex") -> Tuple[int, int]:
    try:
        lo, hi = ngram_range
    except (TypeError, ValueError):
        raise ValueError(f"{who}: ngram_range must be a pair (min_n, max_n)") from None
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{who}: ngram_range must hold ints")
    if not 1 <= int(lo) <= int(hi) <= NGRAM_MAX:
        raise ValueError(f"{who}: supported ngram_range is 1 <= min_n <= max_n <= {NGRAM_MAX}, not {tuple(ngram_range)}")
    return int(lo), int(hi)


def slots_per_position(min_n: int, max_n: int) -> int:
    """NS of include/snx.h: slots a position of the padded row owns (a U+0020 between two words is two 1-grams)."""
    return max_n - min_n + 1 + (1 if min_n == 1 else 0)


def lds_row_capacity(ngram_range=(2, 3)) -> int:
    """The longest row (code points after the join) that one workgroup counts in LDS; longer rows go through workspace."""
    lo, hi = check_ngram_range(ngram_range, "lds_row_capacity")
    return LDS_KEYS // slots_per_position(lo, hi) - 2


def word_rows(texts: Sequence[str], who: str = "TfidfIndex") -> Tuple[np.ndarray, np.ndarray]:
    """``" ".join(text.lower().split())`` of every text as a CSR of code points (ptr int64 [n+1], code_points int32): what
    scikit-learn's ``char_wb`` analyzer sees after its ``lower``, with one U+0020 between the words."""
    texts = list(texts)
    if any(not isinstance(t, str) for t in texts):
        raise ValueError(f"{who}: texts must be strings")
    return code_point_csr([" ".join(t.lower().split()) for t in texts], who)


def keys_to_ngrams(keys) -> List[str]:
    """int64 n-gram keys ((c0+1) << 42 | (c1+1) << 21 | (c2+1), 0 = absent) -> the n-gram strings."""
    out = []
    for k in np.asarray(keys.cpu() if isinstance(keys, torch.Tensor) else keys, dtype=np.int64).tolist():
        cs = [(k >> s) & 0x1FFFFF for s in (42, 21, 0)]
        out.append("".join(chr(c - 1) for c in cs if c))
    return out


def tfidf_idf(doc_freq, num_docs: int) -> np.ndarray:
    """idf [F] float64 on the host: numpy.log((1 + N) / (1 + df)) + 1, scikit-learn's smooth idf."""
    df = np.asarray(doc_freq, np.float64)
    return np.log((1.0 + np.float64(num_docs)) / (1.0 + df)) + 1.0


def tf_table(tmax: int, sublinear_tf: bool) -> np.ndarray:
    """float64 [tmax + 1]: the term-frequency factor of a count c at index c (index 0 unused)."""
    c = np.arange(max(int(tmax), 1) + 1, dtype=np.float64)
    if sublinear_tf:
        c[1:] = np.log(c[1:]) + 1.0
    return c


def select_features(total: torch.Tensor, max_features: Optional[int]) -> torch.Tensor:
    """Positions (ascending) of the ``max_features`` entries of ``total`` (int64, one per distinct key, keys ascending) with
    the largest total count, ties lowest key first; None or >= len(total): all."""
    n = int(total.numel())
    if max_features is None or int(max_features) >= n:
        return torch.arange(n, device=total.device)
    order = torch.sort(total, descending=True, stable=True).indices      # stable: equal totals keep ascending key order
    return torch.sort(order[: int(max_features)]).values


def row_counts(ptr: np.ndarray, cps: np.ndarray, ngram_range, device):
    """Code-point rows -> (cnt int64 [n], keys int64 [nnz] ascending within each row, counts int32 [nnz]) on ``device``
    (snx_tfidf_row_counts, snx_tfidf_compact_counts)."""
    lo, hi = check_ngram_range(ngram_range, "row_counts")
    d_ptr, d_cps, dev = csr_to_device(ptr, cps, device, "row_counts", trusted=True)
    n = int(ptr.size - 1)
    if n == 0:
        return (torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.long, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev))
    NS = slots_per_position(lo, hi)
    longest = int((ptr[1:] - ptr[:-1]).max())
    slots = (int(ptr[-1]) + 2 * n) * NS
    s_key = torch.empty(slots, dtype=torch.long, device=dev)
    s_count = torch.empty(slots, dtype=torch.int32, device=dev)
    cnt32 = torch.empty(n, dtype=torch.int32, device=dev)
    ws, ws_bytes = workspace("snx_tfidf_counts_workspace_bytes", dev, longest, lo, hi)
    with torch.cuda.device(dev):
        call("snx_tfidf_row_counts", _p(d_ptr), _p(d_cps), n, longest, lo, hi, _p(s_key), _p(s_count), _p(cnt32),
             _p(ws), ws_bytes, _stream())
        cnt = cnt32.long()
        dst = offsets(cnt)
        src = (d_ptr[:-1] + 2 * torch.arange(n, device=dev)) * NS
        nnz = int(dst[-1])
        keys = torch.empty(nnz, dtype=torch.long, device=dev)
        counts = torch.empty(nnz, dtype=torch.int32, device=dev)
        call("snx_tfidf_compact_counts", _p(src), _p(dst), n, _p(s_key), _p(s_count), _p(keys), _p(counts), _stream())
    return cnt, keys, counts


def weight_rows(cnt: torch.Tensor, keys: torch.Tensor, counts: torch.Tensor, feature_keys: torch.Tensor, idf: torch.Tensor,
                sublinear_tf: bool = True):
    """Rows of (key, count) as ``row_counts`` returns them -> the L2-normalised tf-idf rows as ``SparseIndex.add_csr``
    takes them: (cnt int64 [n], feature ids int32 ascending, weights fp32 > 0) (snx_tfidf_weights, snx_tfidf_compact_rows).
    ``feature_keys`` int64 [F] strictly ascending, ``idf`` float64 [F], on the rows' device."""
    dev, n, nnz, F = keys.device, int(cnt.numel()), int(keys.numel()), int(feature_keys.numel())
    if n == 0:
        return (torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.float32, device=dev))
    if feature_keys.dtype != torch.long or idf.dtype != torch.float64 or idf.numel() != F or feature_keys.device != dev or \
            idf.device != dev:
        raise ValueError("weight_rows: feature_keys int64 [F] and idf float64 [F] on the rows' device")
    tmax = int(counts.max()) if nnz else 1
    table = torch.from_numpy(tf_table(tmax, sublinear_tf)).to(dev)
    src = offsets(cnt)
    p_fid = torch.empty(nnz, dtype=torch.int32, device=dev)
    p_w = torch.empty(nnz, dtype=torch.float32, device=dev)
    known32 = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("snx_tfidf_weights", _p(src), _p(keys), _p(counts), n, _p(feature_keys), _p(idf), F, _p(table),
             max(tmax, 1), _p(p_fid), _p(p_w), _p(known32), _stream())
        known = known32.long()
        dst = offsets(known)
        m = int(dst[-1])
        fid = torch.empty(m, dtype=torch.int32, device=dev)
        w = torch.empty(m, dtype=torch.float32, device=dev)
        call("snx_tfidf_compact_rows", _p(src), _p(dst), n, _p(p_fid), _p(p_w), _p(fid), _p(w), _stream())
    return known, fid, w


class TfidfIndex:
    """Character n-gram TF-IDF with cosine search, on the GPU: the index of the reference's lexical hard-negative mining.

        tf = TfidfIndex(device, ngram_range=(2, 3), max_features=30000, sublinear_tf=True)
        tf.fit_add(texts)                                       # per batch of corpus documents
        tf.build()
        scores, docs, rank, tscore = tf.search_texts(queries, k, targets=None)

    ``build`` fits the vocabulary on everything added (include/snx.h "Character n-gram TF-IDF": the ``max_features``
    n-grams of largest total count, ties lowest key first -- scikit-learn leaves ties at the cut to an unstable argsort --
    numbered in ascending key order, which is scikit-learn's feature order; idf = log((1 + N) / (1 + df)) + 1), weighs the
    rows ((1 + log c) * idf in float64, L2-normalised, rounded to fp32 once) and builds an ordinary ``SparseIndex`` over
    them, ``.index``.  A search is that index's: s(q, d) the fp32 fmaf chain over the shared features ascending, score
    descending, ties lowest doc id, only scores > 0 -- a document sharing no n-gram with the query is never returned,
    where the reference's ranking of all documents hands out zero-cosine ones in arbitrary order.  ``feature_keys`` [F]
    int64, ``doc_freq`` [F] int32, ``idf`` [F] float64 (device tensors) and ``feature_ngrams()`` are exposed."""

    def __init__(self, device, ngram_range=(2, 3), max_features: Optional[int] = 30000, sublinear_tf: bool = True):
        self.ngram_range = check_ngram_range(ngram_range)
        if max_features is not None and (isinstance(max_features, bool) or not isinstance(max_features, (int, np.integer))
                                         or int(max_features) < 1):
            raise ValueError("TfidfIndex: max_features must be None or an int >= 1")
        self.max_features = None if max_features is None else int(max_features)
        self.sublinear_tf = bool(sublinear_tf)
        self.device = cuda_device(device)
        if self.device.type != "cuda":
            raise ValueError("TfidfIndex: runs on a GPU")
        self._cnt, self._key, self._count = [], [], []          # per batch, as row_counts returns them
        self.num_docs = 0
        self.feature_keys = self.doc_freq = self.idf = self.total_count = self.index = None

    @property
    def built(self) -> bool:
        return self.index is not None

    def fit_add(self, texts: Sequence[str]) -> None:
        ptr, cps = word_rows(texts, "TfidfIndex.fit_add")
        if self.num_docs + ptr.size - 1 >= 2 ** 31:
            raise ValueError("TfidfIndex: doc ids are int32")
        cnt, keys, counts = row_counts(ptr, cps, self.ngram_range, self.device)
        self._cnt.append(cnt)
        self._key.append(keys)
        self._count.append(counts)
        self.num_docs += int(cnt.numel())
        self.index = None                                     # a new batch invalidates a built index

    def build(self) -> "TfidfIndex":
        dev, N = self.device, self.num_docs
        cnt = cat_or_empty(self._cnt, torch.long, dev)
        keys = cat_or_empty(self._key, torch.long, dev)
        counts = cat_or_empty(self._count, torch.int32, dev)
        self._cnt, self._key, self._count = [cnt], [keys], [counts]
        # the fit: one device-wide sort (torch.unique), exact integer sums
        distinct, inverse = torch.unique(keys, sorted=True, return_inverse=True)
        total = torch.zeros(distinct.numel(), dtype=torch.long, device=dev).index_add_(0, inverse, counts.long())
        df = torch.bincount(inverse, minlength=distinct.numel())
        sel = select_features(total, self.max_features)
        self.feature_keys = distinct[sel].contiguous()
        self.total_count = total[sel].contiguous()
        self.doc_freq = df[sel].to(torch.int32).contiguous()
        self.idf = torch.from_numpy(tfidf_idf(self.doc_freq.cpu().numpy(), N)).to(dev)   # the log on the host: one libm
        index = SparseIndex(max(int(self.feature_keys.numel()), 1), dev)
        index.add_csr(*weight_rows(cnt, keys, counts, self.feature_keys, self.idf, self.sublinear_tf))
        self.index = index.build()
        return self

    def feature_ngrams(self) -> List[str]:
        """The vocabulary as strings, in feature order (scikit-learn's ``get_feature_names_out``)."""
        if self.feature_keys is None:
            raise RuntimeError("TfidfIndex.feature_ngrams: call build() first")
        return keys_to_ngrams(self.feature_keys)

    def doc_rows(self):
        """The indexed rows as the CSR triple (cnt int64 [N], feature ids int32, weights fp32)."""
        if not self.built:
            raise RuntimeError("TfidfIndex.doc_rows: call build() first")
        ix = self.index
        return ix.doc_ptr[1:] - ix.doc_ptr[:-1], ix.doc_term, ix.doc_w

    def query_rows(self, texts: Sequence[str]):
        """Texts -> the CSR triple (cnt int64 [nq], feature ids int32 ascending, weights fp32) that
        ``.index.search_csr`` and ``SparseIndex.add_csr`` take; a text with no known n-gram is an empty row.  Row-local
        kernels only: no device-wide sort."""
        if not self.built:
            raise RuntimeError("TfidfIndex.query_rows: call build() first")
        ptr, cps = word_rows(texts, "TfidfIndex.query_rows")
        cnt, keys, counts = row_counts(ptr, cps, self.ngram_range, self.device)
        return weight_rows(cnt, keys, counts, self.feature_keys, self.idf, self.sublinear_tf)

    def search_texts(self, texts: Sequence[str], k: int, targets: Optional[torch.Tensor] = None):
        """Texts -> what ``SparseIndex.search`` returns: (scores [nq, k] fp32, docs [nq, k] int32 (unused: 0 / -1), rank |
        None, tscore | None)."""
        cnt, fid, w = self.query_rows(texts)
        if cnt.numel() == 0:
            return search_outputs(0, int(k), self.device, targets is not None)
        return self.index.search_csr(cnt, fid, w, k, targets=targets)

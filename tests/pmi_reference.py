"""Plain-Python restatement of the co-occurrence and PMI contract (include/snx.h "Co-occurrence and PMI"), for the tests.

The counting is the reference's loop over position pairs of every window, over id rows, into a dict of cells.
``count_window`` is that double loop as written; ``count_window_fast`` gives the same cells with the inner loop handed to
numpy (the tests of long windows use it; the host tests hold the two equal).  The PMI formula is numpy float64, operation
for operation.  tests/golden/g18_pmi (written by tools/make_golden_pmi.py from the reference's own run) pins all of it."""
import json
import os
from collections import defaultdict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

Cells = Dict[Tuple[int, int], Dict[int, int]]                 # (row, col) -> {window length m: additions made at m}


def windows_of(rows: Sequence[Sequence[int]], window_size: Optional[int]) -> List[List[int]]:
    """Rows are windows (``window_size=None``), or every row slides a window over its tokens."""
    if window_size is None:
        return [list(r) for r in rows]
    out = []
    for r in rows:
        r = list(r)
        if len(r) <= window_size:
            if r:
                out.append(r)
        else:
            out.extend(r[i:i + window_size] for i in range(len(r) - window_size + 1))
    return out


def count_window(cells: Cells, window: Sequence[int], symmetric: bool) -> None:
    idx = [t for t in window if t >= 0]
    m = len(idx)
    if m < 2:
        return
    for i in range(m):
        for j in range(i + 1, m):
            cells[(idx[i], idx[j])][m] += 1
            if symmetric:
                cells[(idx[j], idx[i])][m] += 1


def count_window_fast(cells: Cells, window: Sequence[int], symmetric: bool) -> None:
    idx = np.asarray([t for t in window if t >= 0], dtype=np.int64)
    m = int(idx.size)
    if m < 2:
        return
    for i in range(m - 1):
        later, times = np.unique(idx[i + 1:], return_counts=True)
        a = int(idx[i])
        for b, c in zip(later.tolist(), times.tolist()):
            cells[(a, b)][m] += c
            if symmetric:
                cells[(b, a)][m] += c


def count_cells(rows, window_size: Optional[int] = None, symmetric: bool = True, fast: bool = False) -> Tuple[Cells, int]:
    """-> (cells, total_windows)."""
    cells: Cells = defaultdict(lambda: defaultdict(int))
    wins = windows_of(rows, window_size)
    for win in wins:
        (count_window_fast if fast else count_window)(cells, win, symmetric)
    return cells, len(wins)


def to_csr(cells: Cells, V: int, normalize: bool = False):
    """-> (indptr int64 [V+1], indices int32, data fp32, counts int64 | None).  Not normalised: the additions.  Normalised:
    sum over m ascending of additions / m in float64 from +0, rounded to fp32 once."""
    keys = sorted(cells)
    indptr = np.zeros(V + 1, dtype=np.int64)
    for r, _ in keys:
        indptr[r + 1] += 1
    np.cumsum(indptr, out=indptr)
    indices = np.array([c for _, c in keys], dtype=np.int32)
    counts = np.array([sum(cells[k].values()) for k in keys], dtype=np.int64)
    if not normalize:
        return indptr, indices, counts.astype(np.float32), counts
    data = np.zeros(len(keys), dtype=np.float64)
    for i, k in enumerate(keys):
        s = 0.0
        for m in sorted(cells[k]):
            s += cells[k][m] / m
        data[i] = s
    return indptr, indices, data.astype(np.float32), None


def cooccurrence(rows, V: int, window_size: Optional[int] = None, symmetric: bool = True, normalize: bool = False,
                 fast: bool = False):
    cells, total = count_cells(rows, window_size, symmetric, fast)
    return to_csr(cells, V, normalize) + (total,)


# ------------------------------------------------------------------------------------------------ the text half
def tokenize(text: str) -> List[str]:
    return text.split()


def sentence_pieces(document: str) -> List[str]:
    out, cur = [], []
    for ch in document:
        if ch in ".!?\n":
            if cur:
                out.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    if cur:
        out.append("".join(cur).strip())
    return [s for s in out if s]


def paragraph_pieces(document: str) -> List[str]:
    return [p for p in document.split("\n\n") if p.strip()]


def build(documents: Sequence[str], window_type: str, window_size: int, min_term_freq: int, max_vocab_size: int):
    """The text half: -> (vocab list in id order, term_freq dict, doc_freq dict, id rows, window_size or None)."""
    tf: Dict[str, int] = {}
    df: Dict[str, int] = {}
    for doc in documents:
        toks = tokenize(doc)
        for t in toks:
            tf[t] = tf.get(t, 0) + 1
        for t in set(toks):
            df[t] = df.get(t, 0) + 1
    terms = [t for t, f in tf.items() if f >= min_term_freq]
    terms.sort(key=lambda t: -tf[t])
    terms = terms[:max_vocab_size]
    vocab = {t: i for i, t in enumerate(terms)}
    if window_type == "sliding":
        pieces, w = [tokenize(d) for d in documents], window_size
    else:
        split = sentence_pieces if window_type == "sentence" else paragraph_pieces
        pieces, w = [tokenize(p) for d in documents for p in split(d)], None
    rows = [[vocab.get(t, -1) for t in p] for p in pieces]
    return terms, {t: tf[t] for t in terms}, {t: df[t] for t in terms}, rows, w


# ------------------------------------------------------------------------------------------------ PMI
def marginals_total(vocab: Sequence[str], term_freq: Dict[str, int], data: np.ndarray, alpha: float):
    V = len(vocab)
    freqs = np.zeros(V, dtype=np.float64)
    if alpha != 1.0:
        for i, t in enumerate(vocab):
            freqs[i] = term_freq.get(t, 0)
        sm = np.power(freqs + 1e-10, alpha)
        marg = sm / sm.sum()
    else:
        total_freq = sum(term_freq.values())
        for i, t in enumerate(vocab):
            freqs[i] = term_freq.get(t, 0) / total_freq
        marg = freqs
    total = float(np.asarray(data, dtype=np.float64).sum())    # integer cells below 2^24 in all: exact in any order
    return marg, total if total != 0 else 1.0


def pmi_cell(c: float, p1: float, p2: float, total: float, V: int, k: float, use_ppmi: bool, log_base: float,
             min_cooccurrence: float) -> float:
    none = 0.0 if use_ppmi else float("-inf")
    c = float(c)
    if c < min_cooccurrence:
        if k > 0:
            c = k
        else:
            return none
    p_joint = (c + k) / (total + k * V * V)
    if p1 == 0 or p2 == 0:
        return none
    x = p_joint / (p1 * p2)
    if log_base == 2.0:
        pmi = np.log2(x)
    elif log_base == np.e:
        pmi = np.log(x)
    else:
        pmi = np.log(x) / np.log(log_base)
    if use_ppmi:
        pmi = max(0.0, pmi)
    return float(pmi)


def dense_of(indptr, indices, data, V: int) -> np.ndarray:
    """A small matrix as a dense array (tests only)."""
    out = np.zeros((V, V), dtype=np.asarray(data).dtype)
    for r in range(V):
        out[r, indices[indptr[r]:indptr[r + 1]]] = data[indptr[r]:indptr[r + 1]]
    return out


def pmi_all_pairs(indptr, indices, data, vocab, term_freq, cfg: dict) -> np.ndarray:
    """PMI of every (i, j) of the vocabulary -> float64 [V, V]."""
    V = len(vocab)
    marg, total = marginals_total(vocab, term_freq, data, cfg["context_smoothing_alpha"])
    dense = dense_of(indptr, indices, np.asarray(data, dtype=np.float32), V)
    out = np.zeros((V, V), dtype=np.float64)
    for i in range(V):
        for j in range(V):
            out[i, j] = pmi_cell(dense[i, j], marg[i], marg[j], total, V, cfg["laplace_smoothing"], cfg["use_ppmi"],
                                 cfg["log_base"], cfg["min_cooccurrence"])
    return out


def ulps64(a, b) -> np.ndarray:
    """Distance in float64 ulps of finite values of one sign (or zero)."""
    a = np.asarray(a, dtype=np.float64).view(np.int64)
    b = np.asarray(b, dtype=np.float64).view(np.int64)
    return np.abs(a - b)


# ------------------------------------------------------------------------------------------------ g18
def setting_name(s: dict) -> str:
    return "{window_type}_w{window_size}_{sym}_f{min_term_freq}_v{max_vocab_size}_{norm}".format(
        sym="sym" if s["symmetric"] else "asym", norm="norm" if s["normalize"] else "count", **s)


def load_g18(path: str) -> dict:
    with open(os.path.join(path, "g18.json"), "r", encoding="utf-8") as f:
        g = json.load(f)
    with np.load(os.path.join(path, "arrays.npz")) as z:
        g["arrays"] = {k: z[k] for k in z.files}
    for v in g["validations"]:                                # JSON has no -inf: the tool wrote repr strings
        for p in v["pairs"]:
            p["pmi_score"] = float(p["pmi_score"])
    return g


def check_validation(g18, v, validated, result, thresholds) -> None:
    """What ``SynonymValidator.validate`` returned against validation ``v`` of g18: flags, statuses, counts; the
    thresholds to 1e-9."""
    assert len(validated) == len(v["pairs"]) == len(g18["pairs"])
    for got, want in zip(validated, v["pairs"]):
        assert (got.source, got.target, got.category) == (want["source"], want["target"], want["category"])
        assert got.oov_status == want["oov_status"] and got.is_valid == want["is_valid"], want
    want = v["result"]
    assert (result.total_pairs, result.valid_pairs, result.removed_pairs, result.oov_pairs) == \
        (want["total_pairs"], want["valid_pairs"], want["removed_pairs"], want["oov_pairs"])
    assert result.pmi_threshold == want["pmi_threshold"]
    assert thresholds.keys() == v["thresholds"].keys()
    for k in thresholds:
        assert abs(thresholds[k] - v["thresholds"][k]) <= 1e-9

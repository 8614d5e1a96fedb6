"""Restatement of the reference's IDF line in Python ints and float64, for the tests of snx.idf (tests/test_idf_host.py,
tests/test_gpu_idf.py, tests/test_gpu_idf_training.py).  Nothing here imports the product code.

  document frequencies ... ref:tools/idf-compute/src/main.rs:160-176 (a `seen` set per document, ids >= vocab ignored)
  IDF formulas ........... ref:tools/idf-compute/src/main.rs:199-205 (bm25, standard),
                           ref:tests/test_korean_neural_sparse.py:110 (smooth)
  penalty weights ........ ref:scripts/test_idf_math.py:61-126, ref:docs/concepts/04-loss-functions.md §5 "V26"
  penalty and gradient ... ref:scripts/test_idf_math.py:176-246 (sum_j w_j * mean_j) with the quadratic FLOPS term of
                           ref:src/model/losses.py:136-152 weighted alike
  query rows ............. ref:tests/test_korean_neural_sparse.py:417-427 (idf[token] once per distinct token)
"""
import math

import numpy as np


# ------------------------------------------------------------------------------------------------ document frequencies
def doc_freq(ids, mask, V):
    """df [V] Python ints -> int64, num_docs = rows.  A row counts once per distinct id in [0, V) at a masked-in position."""
    ids, mask = np.asarray(ids), np.asarray(mask)
    df = [0] * V
    for r in range(ids.shape[0]):
        seen = set()
        for t, m in zip(ids[r].tolist(), mask[r].tolist()):
            if m != 0 and 0 <= t < V:
                seen.add(t)
        for t in seen:
            df[t] += 1
    return np.asarray(df, dtype=np.int64), int(ids.shape[0])


# ------------------------------------------------------------------------------------------------ IDF
def idf_value(n, df, smoothing):
    n, df = float(n), float(df)
    if smoothing == "bm25":
        return math.log(1.0 + (n - df + 0.5) / (df + 0.5))              # main.rs:202
    if smoothing == "standard":
        return math.log(n / (df + 1.0))                                 # main.rs:203
    if smoothing == "smooth":
        return math.log((n + 1.0) / (df + 1.0)) + 1.0                   # test_korean_neural_sparse.py:110
    raise ValueError(smoothing)


def idf(df, n, smoothing):
    return np.asarray([idf_value(n, d, smoothing) for d in np.asarray(df).tolist()], dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------ penalty weights
def penalty_weights(idf_v, alpha=4.0, special_ids=(), special_penalty=100.0, stopword_ids=(), stopword_penalty=15.0):
    """float64 list arithmetic, one rounding to fp32 at the end."""
    v = [float(x) for x in np.asarray(idf_v, dtype=np.float64).tolist()]
    special, stop = set(special_ids), set(stopword_ids)
    real = [x for i, x in enumerate(v) if i not in special]
    lo, hi = min(real), max(real)
    out = []
    for i, x in enumerate(v):
        w = math.exp(-alpha * ((x - lo) / (hi - lo + 1e-8)))
        if i in stop:
            w *= stopword_penalty
        if i in special:
            w = special_penalty
        out.append(w)
    return np.asarray(out, dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------ penalty
def column_means_fp32(x):
    """fp32 sum over ascending rows, divided by fp32(R): the order the device defines."""
    x = np.asarray(x, dtype=np.float32)
    s = np.zeros(x.shape[1], dtype=np.float32)
    for r in range(x.shape[0]):
        s = (s + x[r]).astype(np.float32)
    return (s / np.float32(x.shape[0])).astype(np.float32)


def penalty_terms_fp32(a, w):
    """t1 = w |a|, t2 = w (a a), every product rounded to fp32."""
    a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
    t1 = (w * np.abs(a)).astype(np.float32)
    t2 = (w * (a * a).astype(np.float32)).astype(np.float32)
    return t1, t2


def penalty(a, w, beta):
    """-> (S1, S2, P, A1, A2): exact sums (math.fsum) of the fp32 terms, P = S1 + fp32(beta) * S2 in float64, and the sums of
    the terms' magnitudes for the error bound."""
    t1, t2 = penalty_terms_fp32(a, w)
    s1, s2 = math.fsum(t1.tolist()), math.fsum(t2.tolist())
    a1, a2 = math.fsum(np.abs(t1).tolist()), math.fsum(np.abs(t2).tolist())
    b = float(np.float32(beta))
    return s1, s2, s1 + b * s2, a1, a2


def penalty_bound(V, sum_abs, value):
    """|got - fsum| <= V * 2^-52 * sum|t| (float64 accumulation of V addends) + 2^-24 * |value| (the fp32 rounding)."""
    return V * 2.0 ** -52 * sum_abs + 2.0 ** -24 * abs(value)


def penalty_grad_coef(a, w, beta, lam, g, R):
    """d(g * lam * P)/dx[r, j] = g lam w_j (sign(a_j) + 2 beta a_j) / R in float64 from the fp32 inputs; sign(0) = 0."""
    a64, w64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    b, l, g = float(np.float32(beta)), float(np.float32(lam)), float(np.float32(g))
    return g * l * w64 * (np.sign(a64) + 2.0 * b * a64) / float(R)


# ------------------------------------------------------------------------------------------------ queries
def query_rows(ids, mask, allowed, idf_v, positive_only=True):
    """Per row: the distinct counted ids ascending and idf[id] once each.  ``positive_only``: a sparse query row holds
    weights > 0 (a term of weight 0 adds nothing to a dot product; OpenSearch's sparse fields take positive weights), so
    ids with idf <= 0 leave the row; the dense matrix keeps them."""
    ids, mask, allowed = np.asarray(ids), np.asarray(mask), np.asarray(allowed)
    V = allowed.shape[0]
    rows = []
    for r in range(ids.shape[0]):
        seen = sorted({t for t, m in zip(ids[r].tolist(), mask[r].tolist()) if m != 0 and 0 <= t < V and allowed[t] != 0
                       and (not positive_only or idf_v[t] > 0)})
        rows.append((seen, [np.float32(idf_v[t]) for t in seen]))
    return rows


def query_dense(ids, mask, allowed, idf_v):
    rows = query_rows(ids, mask, allowed, idf_v, positive_only=False)
    q = np.zeros((len(rows), np.asarray(allowed).shape[0]), dtype=np.float32)
    for r, (terms, vals) in enumerate(rows):
        for t, v in zip(terms, vals):
            q[r, t] = v
    return q


def scores(q_rows, doc_dense):
    """float64 dot products of query rows against dense fp32 documents [N, V]: -> [nq, N]."""
    d = np.asarray(doc_dense, dtype=np.float64)
    out = np.zeros((len(q_rows), d.shape[0]), dtype=np.float64)
    for r, (terms, vals) in enumerate(q_rows):
        for t, v in zip(terms, vals):
            out[r] += float(v) * d[:, t]
    return out

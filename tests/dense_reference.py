"""Plain numpy restatement of the "exact dense retrieval" section of include/snx.h: the tests' reference for csrc/dense.hip.

Score: per step acc = float32(float64(acc) + float64(a) * float64(b)), j ascending from +0, then + 0.0.  A float64 holds
the product of two fp32 values exactly, so this IS the ABI's fmaf chain bit for bit whenever the float64 sum is exact too
-- which holds for the dyadic test values (integers in [-8, 8] divided by 8: every partial sum is a multiple of 1/64 far
below 2^24) -- and differs from it by double rounding only in rare cases otherwise.
Order: score descending as real numbers, ties lowest doc id first; every doc is a candidate."""
import numpy as np

K_MAX = 1024


def chain_scores(Q: np.ndarray, E: np.ndarray) -> np.ndarray:
    """[nq, D] x [nd, D] fp32 -> s [nq, nd] fp32 by the chain above."""
    Q = np.asarray(Q, np.float32)
    E = np.asarray(E, np.float32)
    acc = np.zeros((Q.shape[0], E.shape[0]), np.float32)
    Q64, E64 = Q.astype(np.float64), E.astype(np.float64)
    with np.errstate(under="ignore"):
        for j in range(Q.shape[1]):
            acc = (acc.astype(np.float64) + Q64[:, j, None] * E64[None, :, j]).astype(np.float32)
    return acc + np.float32(0.0)


def exact_scores(Q: np.ndarray, E: np.ndarray) -> np.ndarray:
    """chain_scores for DYADIC operands (multiples of 1/8 in [-1, 1], D <= 4096), as one float64 matmul: every product is a
    multiple of 1/64 and every partial sum stays below 2^12, so no step of the chain rounds and the chain equals the exact
    sum (tests/test_dense_host.py holds the two functions together at D = 1024)."""
    Q = np.asarray(Q, np.float32)
    E = np.asarray(E, np.float32)
    for x in (Q, E):
        assert x.shape[1] <= 4096 and np.array_equal(np.round(x * 8), x * 8) and (np.abs(x) <= 1).all()
    return (Q.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32) + np.float32(0.0)


def ranked(scores_row: np.ndarray, admissible=None) -> np.ndarray:
    """Doc ids of one query in search order (score desc, doc asc); ``admissible``: bool mask or None."""
    ids = np.arange(scores_row.shape[0])
    if admissible is not None:
        ids = ids[admissible]
    return ids[np.lexsort((ids, -scores_row[ids].astype(np.float64)))]


def search(S: np.ndarray, k: int, targets=None):
    """-> (scores [nq, k] fp32, docs [nq, k] int32, rank [nq] int32 | None, tscore [nq] fp32 | None)."""
    nq, nd = S.shape
    scores = np.zeros((nq, k), np.float32)
    docs = np.full((nq, k), -1, np.int32)
    for q in range(nq):
        order = ranked(S[q])[:k]
        docs[q, :len(order)] = order
        scores[q, :len(order)] = S[q, order]
    if targets is None:
        return scores, docs, None, None
    t = np.asarray(targets, np.int64)
    ts = S[np.arange(nq), t]
    d = np.arange(nd)[None, :]
    rank = 1 + (S > ts[:, None]).sum(1) + ((S == ts[:, None]) & (d < t[:, None])).sum(1)
    return scores, docs, rank.astype(np.int32), ts.astype(np.float32)


def search_band(S: np.ndarray, lo: int, hi: int, exclude=None, ceiling=None):
    """-> (scores [nq, hi-lo] fp32, docs [nq, hi-lo] int32, found [nq] int32).  ``exclude``: per-query doc-id lists or
    None; ``ceiling``: fp32 [nq] or None (s < ceiling, strict; NaN admits nothing)."""
    nq, nd = S.shape
    w = hi - lo
    scores = np.zeros((nq, w), np.float32)
    docs = np.full((nq, w), -1, np.int32)
    found = np.zeros(nq, np.int32)
    for q in range(nq):
        ok = np.ones(nd, bool)
        if exclude is not None and len(exclude[q]):
            ok[np.asarray(list(exclude[q]), np.int64)] = False
        if ceiling is not None:
            with np.errstate(invalid="ignore"):
                ok &= S[q] < np.float32(ceiling[q])
        order = ranked(S[q], ok)[lo:hi]
        found[q] = len(order)
        docs[q, :len(order)] = order
        scores[q, :len(order)] = S[q, order]
    return scores, docs, found


class NumpyDenseIndex:
    """CPU stand-in for snx.retrieval.DenseIndex with numpy arrays in and out (the chain above), for the host tests of the
    teacher pipeline (src.train.mining.dense takes the index as a parameter)."""

    def __init__(self, dim: int, device=None):
        self.dim = int(dim)
        self._parts = []
        self.emb = None
        self.num_docs = 0

    def add(self, emb):
        e = np.asarray(emb, np.float32).reshape(-1, self.dim)
        self._parts.append(e)
        self.num_docs += e.shape[0]

    def build(self):
        self.emb = np.concatenate(self._parts) if self._parts else np.zeros((0, self.dim), np.float32)
        return self

    def search(self, q, k, targets=None, chunk_docs=0):
        return search(chain_scores(np.asarray(q, np.float32).reshape(-1, self.dim), self.emb), k, targets)

    def search_band(self, q, lo, hi, exclude=None, ceiling=None, chunk_docs=0):
        return search_band(chain_scores(np.asarray(q, np.float32).reshape(-1, self.dim), self.emb), lo, hi, exclude,
                           ceiling)

    def pair_scores(self, q, pairs):
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        out = np.zeros(len(pairs), np.float32)
        for i, (a, b) in enumerate(pairs):
            out[i] = chain_scores(q[a:a + 1], self.emb[b:b + 1])[0, 0]
        return out

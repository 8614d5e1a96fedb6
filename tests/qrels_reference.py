"""Plain numpy restatement of the "relevance judgments" section of include/snx.h: the tests' reference for
csrc/qrels.hip.

Rows are (terms ascending, weights) pairs; weights are taken as fp32.  ``scores`` is the brute-force s(q, d): per query
term in ascending id, acc = fp32(float64(acc) + float64(q_w) * float64(d_w)) -- the product of two fp32 values is exact
in float64, so for the small-integer weights of the tests (every partial sum exact) this is the ABI's fmaf chain bit for
bit.  The folds of ``ranked_relevance`` and ``bootstrap_means`` are written out add by add."""
import numpy as np

SEGMENT = 64                                       # SNX_BOOTSTRAP_SEGMENT


def rows32(rows):
    return [(np.asarray(t, np.int64), np.asarray(w, np.float32)) for t, w in rows]


def scores(queries, docs, V):
    """s(q, d) [nq, nd] fp32 by the ascending-term fma chain."""
    docs = rows32(docs)
    D = np.zeros((len(docs), V), np.float64)
    for i, (t, w) in enumerate(docs):
        D[i, t] = w
    S = np.zeros((len(queries), len(docs)), np.float32)
    for q, (t, w) in enumerate(rows32(queries)):
        acc = np.zeros(len(docs), np.float32)
        for term, qw in zip(t, w):
            col = D[:, term]
            acc = np.where(col != 0, (acc.astype(np.float64) + np.float64(qw) * col).astype(np.float32), acc)
        S[q] = acc
    return S


def rank_of(S_row, d):
    """The single-target rank of snx_sparse_search: 1 + #{s > s_d} + #{d' < d: s == s_d}, 0 when s_d == 0 or d is out of
    range."""
    if not 0 <= d < len(S_row) or not S_row[d] > 0:
        return 0
    s = S_row[d]
    return 1 + int((S_row > s).sum()) + int((S_row[:d] == s).sum())


def first_relevant(S, relevant):
    """-> (doc int32 [nq], score fp32 [nq], rank int32 [nq], nrel int32 [nq]) by the definition."""
    nq, nd = S.shape
    doc, score = np.full(nq, -1, np.int32), np.zeros(nq, np.float32)
    rank, nrel = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
    for q in range(nq):
        row = sorted({int(d) for d in relevant[q] if 0 <= int(d) < nd})
        nrel[q] = len(row)
        best = None
        for d in row:                              # ascending: a later doc wins only with a strictly higher score
            if S[q, d] > 0 and (best is None or S[q, d] > S[q, best]):
                best = d
        if best is not None:
            doc[q], score[q], rank[q] = best, S[q, best], rank_of(S[q], best)
    return doc, score, rank, nrel


def discount_table(R):
    return 1.0 / np.log2(np.arange(1, R + 1, dtype=np.float64) + 1.0)


def ranked_relevance(docs, relevant, nd, cutoffs, disc=None):
    """docs [nq, R] -> (first int32 [nq], hits int32 [nq, ncut], dcg float64 [nq, ncut]); dcg is a left fold from +0.0,
    one float64 add per relevant position."""
    docs = np.asarray(docs)
    nq, R = docs.shape
    disc = discount_table(R) if disc is None else disc
    first = np.zeros(nq, np.int32)
    hits = np.zeros((nq, len(cutoffs)), np.int32)
    dcg = np.zeros((nq, len(cutoffs)), np.float64)
    for q in range(nq):
        row = {int(d) for d in relevant[q] if 0 <= int(d) < nd}
        acc = [np.float64(0.0) for _ in cutoffs]       # one fold per cutoff, each from +0.0
        for p in range(1, R + 1):
            d = int(docs[q, p - 1])
            if d < 0:
                break
            if d in row:
                if first[q] == 0:
                    first[q] = p
                for j, c in enumerate(cutoffs):
                    if p <= c:
                        hits[q, j] += 1
                        acc[j] = np.float64(acc[j] + disc[p - 1])
        dcg[q] = acc
    return first, hits, dcg


def bootstrap_means(values, idx):
    """values [n, M] float64, idx [nboot, n] -> [nboot, M] in the ABI's order: left folds from +0.0 inside segments of
    SEGMENT positions, a left fold from +0.0 over the segment sums, one division by float64(n)."""
    values = np.asarray(values, np.float64)
    if values.ndim == 1:
        values = values[:, None]
    n, M = values.shape
    g = values[np.asarray(idx)]                     # [nboot, n, M] in resample order
    total = np.zeros((g.shape[0], M), np.float64)
    for s0 in range(0, n, SEGMENT):
        seg = np.zeros((g.shape[0], M), np.float64)
        for i in range(s0, min(n, s0 + SEGMENT)):
            seg = seg + g[:, i]
        total = total + seg
    return total / np.float64(n)

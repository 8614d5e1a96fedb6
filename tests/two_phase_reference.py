"""Plain numpy pruning, rescoring and two-phase search: the tests' reference for csrc/two_phase.hip (the definition:
include/snx.h "pruning and two-phase search").

Rows are (terms ascending, weights) pairs; weights are taken as fp32.  The tests use dyadic weights (multiples of 1/64
below 2), for which every product and every partial sum of a score is exact in fp32: the float64 dot product of the dense
rows, rounded to fp32, then IS the ABI's ascending-term fmaf chain bit for bit.  The prune thresholds fp32(r) * w_max and
fp32(alpha) * total and the alpha-mass folds are computed in np.float32, i.e. as the kernel computes them."""
import numpy as np

PRUNE_TYPES = ("max_ratio", "abs_value", "top_k", "alpha_mass")


def rows32(rows):
    return [(np.asarray(t, np.int64), np.asarray(w, np.float32)) for t, w in rows]


def keep_mask(w, prune_type, value):
    """fp32 weights of one row (term order) -> bool keep mask."""
    w = np.asarray(w, np.float32)
    n = len(w)
    keep = np.zeros(n, bool)
    if n == 0:
        return keep
    if prune_type == "max_ratio":
        return w >= np.float32(np.float32(value) * w.max())
    if prune_type == "abs_value":
        return w >= np.float32(value)
    order = np.lexsort((np.arange(n), -w.astype(np.float64)))          # weight desc, term asc
    if prune_type == "top_k":
        keep[order[:int(value)]] = True
        return keep
    assert prune_type == "alpha_mass"
    total = np.float32(0)
    for i in order:
        total = np.float32(total + w[i])
    goal = np.float32(np.float32(value) * total)
    acc = np.float32(0)
    for i in order:
        acc = np.float32(acc + w[i])
        keep[i] = True
        if acc >= goal:
            break
    return keep


def prune(rows, prune_type, value):
    """-> (kept rows, rest rows), rows in place."""
    kept, rest = [], []
    for t, w in rows32(rows):
        m = keep_mask(w, prune_type, value)
        kept.append((t[m], w[m]))
        rest.append((t[~m], w[~m]))
    return kept, rest


def dense(rows, V):
    D = np.zeros((len(rows), V), np.float64)
    for i, (t, w) in enumerate(rows32(rows)):
        D[i, t] = w
    return D


def scores(queries, docs, V):
    """s(q, d) [nq, nd] fp32 -- exact for dyadic weights (see the module docstring)."""
    return (dense(queries, V) @ dense(docs, V).T).astype(np.float32)


def top(S_row, ids, k):
    """The ids (distinct) with score > 0 in search order (score desc, lowest id first), at most k."""
    ids = np.asarray(sorted(set(int(d) for d in ids)), np.int64)
    ids = ids[S_row[ids] > 0] if len(ids) else ids
    return ids[np.lexsort((ids, -S_row[ids].astype(np.float64)))][:k]


def search(S, k):
    """Exact search over the score matrix -> (scores [nq, k] fp32, docs [nq, k] int32)."""
    nq, nd = S.shape
    out_s, out_d = np.zeros((nq, k), np.float32), np.full((nq, k), -1, np.int32)
    for q in range(nq):
        o = top(S[q], range(nd), k)
        out_d[q, :len(o)], out_s[q, :len(o)] = o, S[q, o]
    return out_s, out_d


def rescore(S, cand, k, targets=None):
    """cand [nq, W] (ids outside [0, nd): unused) -> (scores, docs, rank | None, tscore | None)."""
    nq, nd = S.shape
    out_s, out_d = np.zeros((nq, k), np.float32), np.full((nq, k), -1, np.int32)
    rank = np.zeros(nq, np.int32) if targets is not None else None
    tscore = np.zeros(nq, np.float32) if targets is not None else None
    for q in range(nq):
        o = top(S[q], [d for d in cand[q] if 0 <= d < nd], k)
        out_d[q, :len(o)], out_s[q, :len(o)] = o, S[q, o]
        if targets is not None:
            tg = int(targets[q])
            rank[q] = next((r + 1 for r, d in enumerate(o) if d == tg), 0)
            tscore[q] = S[q, tg] if 0 <= tg < nd else 0
    return out_s, out_d, rank, tscore


def window(k, expansion_rate, max_window_size):
    return int(min(np.floor(np.float64(k) * np.float64(expansion_rate)), max_window_size))


def two_phase(docs, queries, V, k, prune_type="max_ratio", value=0.4, expansion_rate=5.0, max_window_size=10000,
              targets=None):
    """-> (scores, docs, rank, tscore, stats [nq, 3] int64: postings_high, postings_all, window_filled)."""
    W = window(k, expansion_rate, max_window_size)
    assert k <= W <= 1024
    high, _ = prune(queries, prune_type, value)
    _, C = search(scores(high, docs, V), W)
    out = rescore(scores(queries, docs, V), C, k, targets)
    lens = (dense(docs, V) > 0).sum(0)
    stats = np.array([[lens[h[0]].sum(), lens[np.asarray(q[0], np.int64)].sum(), (c >= 0).sum()]
                      for h, q, c in zip(high, queries, C)], np.int64).reshape(len(queries), 3)
    return out + (stats,)

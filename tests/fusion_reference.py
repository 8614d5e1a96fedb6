"""Plain numpy rank fusion: the tests' reference for snx_fuse_ranked (csrc/hybrid.hip; the definition: include/snx.h "BM25
baseline and rank fusion").

One query at a time: ``lists`` is a sequence of (docs, scores) rows; a list is the leading entries up to the first negative
doc id, the rank of an entry its position + 1, a doc absent from a list ranks max(len_0 + 1, ..., 100).  Everything is
np.float64 array arithmetic, one rounded operation per numpy call and in the operand order of ref:benchmark/score_fusion.py
(numpy never contracts a product and a sum), so the fused scores are the reference's bit for bit (tests/golden/
g13_fusion.json holds the reference's own).  Order: fused score descending, ties lowest doc id first."""
import numpy as np

METHODS = ("rrf", "weighted_rrf", "linear")


def list_len(docs):
    neg = np.nonzero(np.asarray(docs) < 0)[0]
    return int(neg[0]) if len(neg) else len(docs)


def fuse(lists, method, **params):
    """-> (docs int64 [U], scores float64 [U]) in fused order; U = the size of the union."""
    L = len(lists)
    lens = [list_len(d) for d, _ in lists]
    docs = [np.asarray(d, np.int64)[:n] for (d, _), n in zip(lists, lens)]
    max_rank = max([n + 1 for n in lens] + [100])
    union = np.unique(np.concatenate(docs + [np.zeros(0, np.int64)]))
    where = [np.searchsorted(union, d) for d in docs]
    if method == "linear":
        assert L == 2
        alpha = np.float64(params.get("alpha", 0.4))
        assert 0 <= alpha <= 1
        norm = []
        for (_, s), n, w in zip(lists, lens, where):
            s = np.asarray(s, np.float32)[:n].astype(np.float64)
            v = np.zeros(len(union), np.float64)                      # an absent doc
            if n:
                lo, hi = s.min(), s.max()
                v[w] = 1.0 if hi == lo else (s - lo) / (hi - lo)
            norm.append(v)
        fused = alpha * norm[0] + (np.float64(1.0) - alpha) * norm[1]
    else:
        assert method in ("rrf", "weighted_rrf")
        k = np.float64(params.get("k", 60))
        weights = params.get("weights", (0.4, 0.6) if L == 2 else None) if method == "weighted_rrf" else [1.0] * L
        assert len(weights) == L
        fused = None
        for n, w, wt in zip(lens, where, weights):
            rank = np.full(len(union), max_rank, np.float64)
            rank[w] = np.arange(1, n + 1, dtype=np.float64)
            term = np.float64(wt) / (k + rank)
            fused = term if fused is None else fused + term           # the left fold, in list order
    order = np.lexsort((union, -fused))
    return union[order], fused[order]


def fuse_batch(docs, scores, method, top_k, targets=None, **params):
    """docs [L, nq, R] int, scores [L, nq, R] fp32 -> (scores float64 [nq, top_k], docs int32 [nq, top_k] (unused: 0 /
    -1), rank int32 [nq] | None (1-based position in the whole fused order, 0 = in no list), total int32 [nq])."""
    docs, scores = np.asarray(docs), np.asarray(scores, np.float32)
    L, nq, _ = docs.shape
    out_s, out_d = np.zeros((nq, top_k), np.float64), np.full((nq, top_k), -1, np.int32)
    total = np.zeros(nq, np.int32)
    rank = np.zeros(nq, np.int32) if targets is not None else None
    for q in range(nq):
        d, s = fuse([(docs[l, q], scores[l, q]) for l in range(L)], method, **params)
        m = min(len(d), top_k)
        out_d[q, :m], out_s[q, :m], total[q] = d[:m], s[:m], len(d)
        if targets is not None:
            hit = np.nonzero(d == int(targets[q]))[0]
            rank[q] = hit[0] + 1 if len(hit) else 0
    return out_s, out_d, rank, total

"""Plain Python and numpy restatement of the "graph dense retrieval" section of include/snx.h: the tests' reference for
csrc/graph.hip and the CPU stand-in for snx.retrieval.GraphIndex.

Structure (neighbour lists, detours, F, R, G, entry sample) is integer work on a score matrix.  ``scores64`` is the float64
dot product rounded to fp32: on the dyadic data of the tests every product and partial sum is exact, so that IS the ABI's
fp32 chain bit for bit.  On other data the walk takes a ``score(q_row, doc_ids)`` callable, so that it can run on the bits
of the GPU's ``pair_scores``.  The walk keeps the EXACT set of scored docs."""
import math

import numpy as np


def scores64(Q, E) -> np.ndarray:
    S = np.asarray(Q, np.float32).astype(np.float64) @ np.asarray(E, np.float32).astype(np.float64).T
    return S.astype(np.float32) + np.float32(0.0)


def neighbor_lists(S: np.ndarray, knn: int) -> np.ndarray:
    """[nd, nd] scores -> N [nd, knn]: per row the best min(knn, nd-1) other docs, ties to the lowest id, then -1."""
    nd = S.shape[0]
    N = np.full((nd, knn), -1, np.int32)
    ids = np.arange(nd)
    for u in range(nd):
        order = ids[np.lexsort((ids, -S[u].astype(np.float64)))]
        order = order[order != u][:knn]
        N[u, :len(order)] = order
    return N


def valid_prefix(row) -> list:
    out = []
    for x in row:
        if x < 0:
            break
        out.append(int(x))
    return out


def rank_tables(N: np.ndarray) -> list:
    """rank[w][x] = the column of x in N[w]."""
    return [{x: c for c, x in enumerate(valid_prefix(row))} for row in N]


def detours(N: np.ndarray, u: int, rank=None) -> list:
    """detour(u, j) = #{ i < j : rank_{v_i}(v_j) < j } for every valid column j of N[u]."""
    v = valid_prefix(N[u])
    rank = rank_tables(N) if rank is None else rank
    return [sum(1 for i in range(j) if rank[v[i]].get(v[j], math.inf) < j) for j in range(len(v))]


def forward_lists(N: np.ndarray, degree: int) -> np.ndarray:
    nd = N.shape[0]
    F = np.full((nd, degree), -1, np.int32)
    rank = rank_tables(N)
    for u in range(nd):
        v, det = valid_prefix(N[u]), detours(N, u, rank)
        cols = sorted(range(len(v)), key=lambda j: (det[j], j))[:degree]
        F[u, :len(cols)] = [v[j] for j in cols]
    return F


def reverse_lists(F: np.ndarray) -> list:
    """R[v]: the u of the pairs (p, u) with F[u][p] == v, ordered by (p, u), the first `degree` kept."""
    nd, degree = F.shape
    R = [[] for _ in range(nd)]
    for p in range(degree):
        for u in range(nd):
            v = int(F[u, p])
            if v >= 0 and len(R[v]) < degree:
                R[v].append(u)
    return R


def interleave(f: list, r: list, degree: int) -> list:
    """The first `degree` distinct ids of f[0], r[0], f[1], r[1], ...; a list that ran out is passed over."""
    out = []
    for t in range(max(len(f), len(r))):
        for lst in (f, r):
            if t < len(lst) and lst[t] not in out and len(out) < degree:
                out.append(lst[t])
    return out


def optimize(N: np.ndarray, degree: int):
    """N -> (F, G)."""
    F = forward_lists(N, degree)
    R = reverse_lists(F)
    G = np.full(F.shape, -1, np.int32)
    for v in range(F.shape[0]):
        row = interleave(valid_prefix(F[v]), R[v], degree)
        G[v, :len(row)] = row
    return F, G


def default_nentry(nd: int) -> int:
    return 4 * (math.isqrt(max(nd - 1, 0)) + 1)              # 4 * ceil(sqrt(nd))


def clamp_nentry(nentry, ef: int, nd: int) -> int:
    want = default_nentry(nd) if nentry is None else int(nentry)
    return max(min(ef, nd), min(want, nd))


def entry_sample(nd: int, nentry: int) -> np.ndarray:
    return np.array([(i * nd) // nentry for i in range(nentry)], np.int64)


def ordered(scores, docs) -> list:
    """(score, doc) pairs in the ABI's order: score descending, doc ascending."""
    return sorted(zip((float(s) for s in scores), (int(d) for d in docs)), key=lambda e: (-e[0], e[1]))


def walk(score, q_row, G: np.ndarray, entry: np.ndarray, ef: int, width: int, max_iter: int = 0):
    """The walk of the header for one query -> (pool [(score, doc)] in order, iterations).  ``score(q_row, ids)`` returns
    the fp32 scores of the docs ``ids``."""
    nseed = min(ef, len(entry))
    entry = [int(e) for e in entry]
    seeds = ordered(score(q_row, entry), entry)[:nseed] if entry else []
    scored = {d for _, d in seeds}
    pool = [[s, d, False] for s, d in seeds]                 # in order: seeds are sorted
    iters = 0
    while max_iter == 0 or iters < max_iter:
        parents = [e for e in pool if not e[2]][:width]
        if not parents:
            break
        iters += 1
        batch = []
        for e in parents:
            e[2] = True
            for x in G[e[1]]:
                x = int(x)
                if x >= 0 and x not in scored:
                    scored.add(x)                            # a second occurrence in the batch finds it here
                    batch.append(x)
        if batch:
            pool += [[float(s), d, False] for s, d in zip(score(q_row, batch), batch)]
            pool.sort(key=lambda e: (-e[0], e[1]))
            del pool[ef:]
    return [(s, d) for s, d, _ in pool], iters


def band(pool, lo: int, hi: int, exclude=(), ceiling=None):
    """Ranks lo .. hi-1 of the admissible entries of a final pool -> (scores [hi-lo], docs [hi-lo], found)."""
    ex = set(int(d) for d in exclude)
    keep = [(s, d) for s, d in pool if d not in ex and (ceiling is None or np.float32(s) < np.float32(ceiling))]
    cut = keep[lo:hi]
    scores, docs = np.zeros(hi - lo, np.float32), np.full(hi - lo, -1, np.int32)
    for j, (s, d) in enumerate(cut):
        scores[j], docs[j] = np.float32(s), d
    return scores, docs, len(cut)


class NumpyGraphIndex:
    """The stand-in: numpy arrays in and out, the methods of snx.retrieval.GraphIndex.  ``score``: see ``walk``; the
    default scores through ``scores64``."""

    def __init__(self, dim, device=None, degree=32, knn=64, ef=100, width=4, nentry=None, score=None):
        self.dim, self.degree, self.knn, self.ef, self.width, self.nentry = dim, degree, knn, ef, width, nentry
        self._parts, self.num_docs, self.last_iterations = [], 0, None
        self.score = score or (lambda q_row, ids: scores64(q_row[None, :], self.emb[np.asarray(ids, np.int64)])[0])

    def add(self, emb):
        e = np.asarray(emb, np.float32).reshape(-1, self.dim)
        self._parts.append(e)
        self.num_docs += e.shape[0]

    def build(self, neighbors=None):
        self.emb = np.concatenate(self._parts) if self._parts else np.zeros((0, self.dim), np.float32)
        self.neighbors = neighbor_lists(scores64(self.emb, self.emb), self.knn) if neighbors is None else \
            np.asarray(neighbors, np.int32)
        self.forward, self.graph = optimize(self.neighbors, self.degree)
        return self

    def entry(self, ef=None):
        ef = self.ef if ef is None else ef
        return entry_sample(self.num_docs, clamp_nentry(self.nentry, ef, self.num_docs))

    def structure(self):
        return {"neighbors": self.neighbors, "forward": self.forward, "graph": self.graph,
                "entry": self.entry().astype(np.int32)}

    def pools(self, q, ef=None, width=None, max_iter=0):
        ef, width = self.ef if ef is None else ef, self.width if width is None else width
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        out = [walk(self.score, row, self.graph, self.entry(ef), ef, width, max_iter) for row in q]
        self.last_iterations = np.array([it for _, it in out], np.int32)
        return [p for p, _ in out]

    def search_band(self, q, lo, hi, exclude=None, ceiling=None, ef=None, width=None, max_iter=0):
        pools = self.pools(q, ef, width, max_iter)
        rows = [band(p, lo, hi, exclude[i] if exclude is not None else (), None if ceiling is None else ceiling[i])
                for i, p in enumerate(pools)]
        w = hi - lo
        return (np.stack([r[0] for r in rows]).reshape(len(rows), w), np.stack([r[1] for r in rows]).reshape(len(rows), w),
                np.array([r[2] for r in rows], np.int32))

    def search(self, q, k, ef=None, width=None, max_iter=0, query_slice=0):
        return self.search_band(q, 0, k, ef=ef, width=width, max_iter=max_iter)[:2]

"""Plain numpy restatement of the "IVF-Flat dense retrieval" section of include/snx.h: the tests' reference for
csrc/ivf.hip and the CPU stand-in for snx.retrieval.IvfFlatIndex (numpy arrays in and out, the same methods).

Scores are float64 dot products rounded to fp32.  On the dyadic and small-integer data of the tests every product and
every partial sum is exact, so that IS the ABI's fp32 chain bit for bit, in any order of summation.
The search walks the probed lists in probe order and keeps a running top k, the way the kernel does; what decides whether
a doc enters is the FULL order (score descending, then original doc id ascending).  ``fault`` plants one-line mistakes
that the host tests must catch:
  "tie_high"         a doc (and a query) tied between centroids goes to the HIGHEST one
  "carry_threshold"  a doc that only ties the running k-th score loses, across lists (right inside one list, where ids
                     ascend; wrong across lists)
  "fill_slots"       an unused slot names doc nd - 1 (what indexing a pool with -1 hands out) instead of -1"""
import bisect

import numpy as np

K_MAX = 1024
KM_SEG = 1024                          # members per segment of the centroid sum (include/snx.h)


def scores64(Q, E) -> np.ndarray:
    return np.asarray(Q, np.float32).astype(np.float64) @ np.asarray(E, np.float32).astype(np.float64).T


def best_lists(S: np.ndarray, k: int, fault=None) -> np.ndarray:
    """[n, nlist] scores -> the k best lists per row, score descending, ties to the lowest list."""
    ids = np.arange(S.shape[1])
    tie = -ids if fault == "tie_high" else ids
    return np.stack([ids[np.lexsort((tie, -row))][:k] for row in S]).astype(np.int32).reshape(S.shape[0], k)


def kmeans_update(X: np.ndarray, lists: np.ndarray, prev: np.ndarray) -> np.ndarray:
    """One spherical k-means step in the header's fixed float64 order."""
    X64 = np.asarray(X, np.float32).astype(np.float64)
    out = np.array(prev, np.float32, copy=True)
    for c in range(prev.shape[0]):
        members = np.flatnonzero(lists == c)                 # ascending
        if not len(members):
            continue                                         # an empty cluster keeps its centroid
        total = np.zeros(X64.shape[1])
        for s in range(0, len(members), KM_SEG):
            part = np.zeros(X64.shape[1])
            for r in members[s:s + KM_SEG]:
                part = part + X64[r]
            total = total + part
        mean = total / np.float64(len(members))
        ss = np.float64(0.0)
        for m in mean:
            ss = ss + m * m
        norm = np.sqrt(ss)
        out[c] = (mean / norm).astype(np.float32) if norm > 0 else 0.0
    return out


def kmeans(X: np.ndarray, nlist: int, niter: int, seed: int) -> np.ndarray:
    X = np.asarray(X, np.float32)
    first = np.random.RandomState(seed).permutation(X.shape[0])[:nlist]
    lists = np.full(X.shape[0], -1, np.int64)
    lists[first] = np.arange(nlist)
    c = kmeans_update(X, lists, np.zeros((nlist, X.shape[1]), np.float32))
    for _ in range(niter):
        c = kmeans_update(X, best_lists(scores64(X, c), 1)[:, 0], c)
    return c


class NumpyIvfFlatIndex:
    def __init__(self, dim, nlist, device=None, nprobe=1, niter=10, seed=0, fault=None):
        self.dim, self.nlist, self.nprobe, self.niter, self.seed, self.fault = int(dim), int(nlist), int(nprobe), int(niter), int(seed), fault
        self._parts = []
        self.num_docs = 0
        self.emb = self.centroids = self.list_ptr = self.list_doc = self.doc_list = None

    def train(self, x):
        x = np.asarray(x, np.float32).reshape(-1, self.dim)
        assert x.shape[0] >= self.nlist
        self.centroids = kmeans(x, self.nlist, self.niter, self.seed)
        return self

    def set_centroids(self, c):
        self.centroids = np.array(c, np.float32).reshape(self.nlist, self.dim)
        return self

    def add(self, emb):
        e = np.asarray(emb, np.float32).reshape(-1, self.dim)
        self._parts.append(e)
        self.num_docs += e.shape[0]

    def build(self):
        self.emb = np.concatenate(self._parts) if self._parts else np.zeros((0, self.dim), np.float32)
        if self.centroids is None:
            self.nlist = min(self.nlist, self.num_docs)
            self.nprobe = min(self.nprobe, self.nlist)
            self.centroids = kmeans(self.emb, self.nlist, self.niter, self.seed)
        self.doc_list = best_lists(scores64(self.emb, self.centroids), 1, self.fault)[:, 0] if self.num_docs else \
            np.zeros(0, np.int32)
        order = np.argsort(self.doc_list, kind="stable")
        self.list_doc = order.astype(np.int32)
        self.list_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.doc_list, minlength=self.nlist))]).astype(np.int64)
        return self

    def structure(self):
        return {"centroids": self.centroids, "list_ptr": self.list_ptr, "list_doc": self.list_doc}

    def probe(self, q, nprobe=None):
        S = scores64(np.asarray(q, np.float32).reshape(-1, self.dim), self.centroids)
        lists = best_lists(S, self.nprobe if nprobe is None else int(nprobe), self.fault)
        return np.take_along_axis(S, lists.astype(np.int64), 1).astype(np.float32) + np.float32(0.0), lists

    def _walk(self, srow, lists, hi, ok):
        """The best ``hi`` admissible docs of the probed lists, as (score, doc) in search order."""
        kept = []                                            # (-score, doc) ascending: the search order
        for c in lists:
            for d in self.list_doc[self.list_ptr[c]:self.list_ptr[c + 1]].tolist():
                if not ok[d]:
                    continue
                key = (-float(srow[d]), d)
                if len(kept) == hi:
                    beats = key < kept[-1]
                    if self.fault == "carry_threshold":
                        beats = key[0] < kept[-1][0]
                    if not beats:
                        continue
                    kept.pop()
                bisect.insort(kept, key)
        return [(-a, d) for a, d in kept]

    def search_band(self, q, lo, hi, exclude=None, ceiling=None, chunk_docs=0, query_slice=0, nprobe=None):
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        S = scores64(q, self.emb)
        _, lists = self.probe(q, nprobe)
        nq, w = q.shape[0], hi - lo
        scores, docs, found = np.zeros((nq, w), np.float32), np.full((nq, w), -1, np.int32), np.zeros(nq, np.int32)
        if self.fault == "fill_slots":
            docs[:] = self.num_docs - 1
        for i in range(nq):
            ok = np.ones(self.num_docs, bool)
            if exclude is not None and len(exclude[i]):
                ok[np.asarray(list(exclude[i]), np.int64)] = False
            if ceiling is not None:
                with np.errstate(invalid="ignore"):
                    ok &= S[i].astype(np.float32) < np.float32(ceiling[i])
            band = self._walk(S[i], lists[i], hi, ok)[lo:]
            found[i] = len(band)
            for j, (s, d) in enumerate(band):
                scores[i, j], docs[i, j] = np.float32(s) + np.float32(0.0), d
        return scores, docs, found

    def search(self, q, k, nprobe=None, query_slice=0):
        return self.search_band(q, 0, k, nprobe=nprobe)[:2]

    def pair_scores(self, q, pairs):
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        S = scores64(q, self.emb)
        return (S[pairs[:, 0], pairs[:, 1]].astype(np.float32) + np.float32(0.0)) if len(pairs) else np.zeros(0, np.float32)

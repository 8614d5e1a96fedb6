"""Plain numpy SEISMIC, the tests' reference for csrc/seismic.hip (the definition: include/snx.h "SEISMIC").

Rows are (terms ascending, weights) pairs; weights are taken as fp32.  ``build`` and ``search`` take a score primitive
``pair_scores(A, B, pairs) -> fp32 [n]`` = s(A[i], B[j]) for every (i, j) of ``pairs``:
  * ``dyadic_pairs`` (the default): fp32 multiply then fp32 add over the shared terms in ascending term id.  For dyadic
    weights every product and partial sum is exact, so this is the ABI's fmaf chain bit for bit;
  * ``gpu_pairs(device)``: the ABI itself, ``SparseIndex.pair_scores`` over a throwaway index of the B rows with the A
    rows passed as queries (bit-equal to the ABI by contract): summaries are indexed as docs, docs are passed as queries.
The alpha folds are np.float32 adds, i.e. fp32 adds."""
import math

import numpy as np


def rows32(rows):
    return [(np.asarray(t, np.int64), np.asarray(w, np.float32)) for t, w in rows]


def dyadic_pairs(A, B, pairs):
    out = np.zeros(len(pairs), np.float32)
    for n, (i, j) in enumerate(pairs):
        (ta, wa), (tb, wb) = A[i], B[j]
        _, ia, ib = np.intersect1d(ta, tb, assume_unique=True, return_indices=True)
        acc = np.float32(0)
        for x, y in zip(ia, ib):
            acc = np.float32(acc + np.float32(wa[x] * wb[y]))
        out[n] = acc
    return out


def to_device(rows, dev):
    import torch
    cap = max([1] + [len(t) for t, _ in rows])
    vals = np.zeros((len(rows), cap), np.float32)
    ids = np.zeros((len(rows), cap), np.int32)
    cnt = np.zeros(len(rows), np.int32)
    for i, (t, w) in enumerate(rows):
        vals[i, :len(t)] = w
        ids[i, :len(t)] = t
        cnt[i] = len(t)
    return torch.from_numpy(vals).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(cnt).to(dev)


def gpu_pairs(dev):
    import torch
    from snx.retrieval import SparseIndex

    def f(A, B, pairs):
        if len(pairs) == 0:
            return np.zeros(0, np.float32)
        V = 1 + max([0] + [int(t.max()) for t, _ in list(A) + list(B) if len(t)])
        idx = SparseIndex(V, dev)
        idx.add(*to_device(B, dev))
        idx.build()
        p = torch.tensor(np.asarray(pairs, np.int64).reshape(-1, 2), device=dev)
        return idx.pair_scores(*to_device(A, dev), p).cpu().numpy()
    return f


def build(docs, V, n_postings, cluster_ratio, alpha, pair_scores=dyadic_pairs):
    """-> dict of numpy arrays with the keys and layout of SeismicIndex.structure()."""
    docs = rows32(docs)
    lists = [[] for _ in range(V)]
    for d, (t, w) in enumerate(docs):
        for u, x in zip(t, w):
            lists[int(u)].append((d, np.float32(x)))
    ordered, prune_ptr, prune_doc, prune_w, cent_ptr, cent_doc = [], [0], [], [], [0], []
    for t in range(V):
        P = sorted(lists[t], key=lambda e: (-float(e[1]), e[0]))[:n_postings]
        ordered.append(P)
        kept = sorted(P)
        prune_doc += [d for d, _ in kept]
        prune_w += [w for _, w in kept]
        prune_ptr.append(len(prune_doc))
        p = len(P)
        c = 0 if p == 0 else int(min(p, max(1, math.ceil(cluster_ratio * p))))
        cent_doc += [P[(i * p) // c][0] for i in range(c)]
        cent_ptr.append(len(cent_doc))
    pairs = [(d, cent_doc[cent_ptr[t] + j]) for t in range(V) for d, _ in sorted(ordered[t])
             for j in range(cent_ptr[t + 1] - cent_ptr[t])]
    S = pair_scores(docs, docs, pairs)
    pos, blocks, term_blk_ptr = 0, [], [0]
    for t in range(V):
        c = cent_ptr[t + 1] - cent_ptr[t]
        groups = [[] for _ in range(c)]
        for d, _ in sorted(ordered[t]):
            groups[int(np.argmax(S[pos:pos + c]))].append(d)      # first maximum: ties to the lowest j
            pos += c
        blocks += [(j, g) for j, g in enumerate(groups) if g]
        term_blk_ptr.append(len(blocks))
    a32 = np.float32(alpha)
    sum_ptr, sum_term, sum_w = [0], [], []
    for _, g in blocks:
        m = {}
        for d in g:
            for u, x in zip(*docs[d]):
                m[int(u)] = max(m.get(int(u), np.float32(0)), x)
        ent = sorted(m.items(), key=lambda e: (-float(e[1]), e[0]))
        total = np.float32(0)
        for _, x in ent:
            total = np.float32(total + x)
        goal = np.float32(a32 * total)
        acc, keep = np.float32(0), 0
        for _, x in ent:
            acc = np.float32(acc + x)
            keep += 1
            if acc >= goal:
                break
        kept = sorted(ent[:keep])
        sum_term += [u for u, _ in kept]
        sum_w += [x for _, x in kept]
        sum_ptr.append(len(sum_term))
    i64, i32, f32 = np.int64, np.int32, np.float32
    return {"prune_ptr": np.array(prune_ptr, i64), "prune_doc": np.array(prune_doc, i32),
            "prune_w": np.array(prune_w, f32), "cent_ptr": np.array(cent_ptr, i64), "cent_doc": np.array(cent_doc, i32),
            "term_blk_ptr": np.array(term_blk_ptr, i64), "blk_cent": np.array([j for j, _ in blocks], i32),
            "blk_ptr": np.cumsum([0] + [len(g) for _, g in blocks]).astype(i64),
            "blk_doc": np.array([d for _, g in blocks for d in g], i32), "sum_ptr": np.array(sum_ptr, i64),
            "sum_term": np.array(sum_term, i32), "sum_w": np.array(sum_w, f32)}


def query_scores(struct, docs, queries, pair_scores=dyadic_pairs):
    """(s(q, summary) [nq, nblocks], s(q, d) [nq, nd]) fp32."""
    docs, queries = rows32(docs), rows32(queries)
    sp = struct["sum_ptr"]
    summ = [(struct["sum_term"][a:b].astype(np.int64), struct["sum_w"][a:b]) for a, b in zip(sp[:-1], sp[1:])]
    nq, nb, nd = len(queries), len(summ), len(docs)
    R = pair_scores(queries, summ, [(q, b) for q in range(nq) for b in range(nb)]).reshape(nq, nb)
    D = pair_scores(queries, docs, [(q, d) for q in range(nq) for d in range(nd)]).reshape(nq, nd)
    return R, D


def search(struct, docs, queries, k, top_n, heap_factor, targets=None, pair_scores=dyadic_pairs, scores=None):
    """-> (scores [nq, k] fp32, docs [nq, k] int32, rank [nq] | None, tscore [nq] | None, stats [nq, 3] int64)."""
    queries = rows32(queries)
    R, D = scores if scores is not None else query_scores(struct, docs, queries, pair_scores)
    tbp, bp, bd = struct["term_blk_ptr"], struct["blk_ptr"], struct["blk_doc"]
    hf = np.float32(heap_factor)
    nq = len(queries)
    out_s = np.zeros((nq, k), np.float32)
    out_d = np.full((nq, k), -1, np.int32)
    stats = np.zeros((nq, 3), np.int64)
    rank = np.zeros(nq, np.int32) if targets is not None else None
    tscore = np.zeros(nq, np.float32) if targets is not None else None
    for q, (qt, qw) in enumerate(queries):
        cut = sorted(range(len(qt)), key=lambda i: (-float(qw[i]), qt[i]))[:top_n]
        H = []
        for i in cut:
            t = int(qt[i])
            for b in range(tbp[t], tbp[t + 1]):
                stats[q, 0] += 1
                if len(H) == k:
                    with np.errstate(invalid="ignore", over="ignore"):
                        prod = np.float32(hf * R[q, b])
                    if prod < H[-1][0]:
                        continue
                stats[q, 1] += 1
                stats[q, 2] += bp[b + 1] - bp[b]
                have = {d for _, d in H}
                H += [(D[q, d], int(d)) for d in bd[bp[b]:bp[b + 1]] if D[q, d] > 0 and int(d) not in have]
                H = sorted(H, key=lambda e: (-float(e[0]), e[1]))[:k]
        for r, (s, d) in enumerate(H):
            out_s[q, r], out_d[q, r] = s, d
        if targets is not None:
            tg = int(targets[q])
            rank[q] = next((r + 1 for r, (_, d) in enumerate(H) if d == tg), 0)
            tscore[q] = D[q, tg]
    return out_s, out_d, rank, tscore, stats

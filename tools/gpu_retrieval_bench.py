#!/usr/bin/env python3
"""Index build time and search throughput of the native sparse retrieval (snx.retrieval.SparseIndex,
csrc/retrieval.hip) on synthetic Zipf-skewed data.

    python tools/gpu_retrieval_bench.py [--sizes 1000x200,100000x10000,1000000x10000] [--out result.json]
    python tools/gpu_retrieval_bench.py --band [--sizes 1000000x10000] [--miner-records 4000]
    python tools/gpu_retrieval_bench.py --seismic [--sizes 1000000x10000]
    python tools/gpu_retrieval_bench.py --two-phase [--sizes 100000x10000,1000000x10000]
    python tools/gpu_retrieval_bench.py --hybrid [--sizes 100000x10000,1000000x10000]
    python tools/gpu_retrieval_bench.py --qrels [--sizes 100000x2000,1000000x2000]
    python tools/gpu_retrieval_bench.py --dense [--dense-docs N] [--dense-reps 5]

Docs draw 128 terms (with replacement, duplicates dropped: ~99 distinct) from a Zipf(1.0) law over V = 50000 with
weights uniform in [0.1, 3); queries draw 64 the same way (~53 distinct).  Retrieval size 10 with a target per query
(the evaluator's call).  Comparison row: torch.sparse CSR (docs) @ dense query block + torch.topk over query chunks,
where the torch build supports it.

--band: the miner's search (SparseIndex.search_band, ranks [10, 50)) against plain search at k = 50 on the same data,
with 1% of the docs excluded per query, without and with a ceiling (half the query's 100th score); the exclusion rows'
normalisation (exclusion_csr, on the device) is timed on its own.  Then one timed end-to-end miner run
(src.train.mining.mine_negatives) on synthetic triplet shards with a random-init model, in docs/s and queries/s.

--seismic: SeismicIndex (csrc/seismic.hip) at the reference's index defaults (n_postings 300, cluster_ratio 0.1,
summary_prune_ratio 0.4) on the same data: build seconds, then per heap_factor in {0.5, 1, 2} at top_n 10 and k = 10
the queries/s against exact search, the mean overlap@10 with the exact top 10 and the fraction of the Q_cut terms'
postings that were scored.

--two-phase: SparseIndex.search_two_phase (csrc/two_phase.hip) at the reference's setting (max_ratio 0.4, expansion_rate
5, max_window_size 10000; k = 10, so a window of 50) against plain search on the same data, alternating, median of 5 after
a warm-up: queries/s, the mean overlap@10 with the exact top 10 and the share of the query terms' postings under the kept
terms; then the prune kernel alone over the whole doc CSR per prune type, and the build time of pruned("max_ratio", 0.1).

--hybrid: the BM25 baseline and rank fusion (csrc/hybrid.hip).  Token rows of 128 (docs) and 16 (queries) positions are
drawn with replacement from the same Zipf law, every id allowed: Bm25Index.add_tokens + build in docs/s (term counts, df,
weights, the SparseIndex build), BM25 search_tokens at k = 100 in queries/s, then fuse_ranked (RRF, top 10 with targets)
over L = 2 and 3 random lists of R = 100 and 1000 doc ids in queries/s, medians of 5 after a warm-up; as a comparison
row the same rule as plain Python dicts on the host over the first 200 queries.

--qrels: scoring against qrels (csrc/qrels.hip) on the Zipf data of the first mode, every query with 1 .. 8 random
relevant docs (mean 4.5), medians of 5 after a warm-up.  SparseIndex.first_relevant against the emulation it replaces: one
search(k = 1, targets=...) per row position and the minimum of the ranks on the host.  ranked_relevance over the search's
top 100 against the reference's Python set loop over the same lists on the host (transfer included, first 2000 queries).
bootstrap_means (1000 resamples, 3 columns; the host-side index draws timed apart) against the reference-style numpy loop,
one fancy-indexed mean per resample and column.

--dense: the exact dense search (snx.retrieval.DenseIndex, csrc/dense.hip) at the reference miner's shape, nq = 4096,
D = 1024, k = 100, over a synthetic L2-normalised Gaussian corpus, against the reference's own form on the same GPU:
torch.mm(q_batch[4096, D], docs.T) + torch.topk(100) in 4096-query batches (ref:scripts/mine_multi_negatives.py:208-210).
The corpus is as large as that form's [4096, nd] fp32 score matrix allows (--dense-docs 0: a quarter of the free device
memory for the matrix, at most 2^22 docs; a multiple of 128).  After a warm-up of both, the two alternate --dense-reps
times; the row holds every time, the medians, the spread (max - min over the median) and ratio = torch median / ours.
It also checks that the two top lists agree (same doc at every rank where the neighbouring scores differ by more than the
fp32 rounding of the sums)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opensearch-neural-pre-train_amd"))

import torch  # noqa: E402

V = 50000


def zipf_rows(n, m, gen, dev, probs):
    """[n, m] (vals, ids, cnt) rows of distinct Zipf-drawn ids, sentinel-padded after the live entries."""
    ids = torch.multinomial(probs, n * m, replacement=True, generator=gen).view(n, m).to(dev)
    ids, _ = torch.sort(ids, dim=1)
    dup = torch.zeros_like(ids, dtype=torch.bool)
    dup[:, 1:] = ids[:, 1:] == ids[:, :-1]
    ids = torch.where(dup, torch.full_like(ids, V), ids)
    ids, _ = torch.sort(ids, dim=1)
    cnt = (ids < V).sum(1).to(torch.int32)
    ids = torch.where(ids < V, ids, torch.zeros_like(ids)).to(torch.int32)
    vals = (torch.rand(n, m, generator=gen) * 2.9 + 0.1).to(dev)
    return vals.contiguous(), ids.contiguous(), cnt


def sync_time(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def run_case(nd, nq, dev, torch_cmp=True):
    from snx.retrieval import SparseIndex
    gen = torch.Generator().manual_seed(nd + nq)
    probs = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
    probs /= probs.sum()
    batches = [zipf_rows(min(100_000, nd - s), 128, gen, dev, probs) for s in range(0, nd, 100_000)]
    q = zipf_rows(nq, 64, gen, dev, probs)
    targets = torch.randint(0, nd, (nq,), generator=gen).to(dev)

    def build():
        idx = SparseIndex(V, dev)
        for b in batches:
            idx.add(*b)
        return idx.build()

    build()                                                    # warm-up (library load, allocator)
    t_build, idx = sync_time(build)
    t_core, _ = sync_time(idx.build)                           # the native build alone (CSR already packed)
    idx.search(q[0][:64], q[1][:64], q[2][:64], 10, targets=targets[:64])
    times = []
    for _ in range(3):
        t, res = sync_time(lambda: idx.search(*q, 10, targets=targets))
        times.append(t)
    t_search = min(times)
    row = {"docs": nd, "queries": nq, "nnz_docs": idx.nnz, "avg_nnz_doc": idx.nnz / nd,
           "avg_nnz_query": float(q[2].float().mean()), "build_s_incl_packing": t_build, "build_s_native": t_core,
           "search_s": t_search, "queries_per_s": nq / t_search}
    if torch_cmp:
        row["torch_sparse"] = torch_sparse_row(idx, q, nd, nq, dev)
    return row


def torch_sparse_row(idx, q, nd, nq, dev, budget_s=20.0):
    """CSR docs [nd, V] @ dense query block [V, c] -> [nd, c] scores -> torch.topk(10) per query."""
    try:
        D = torch.sparse_csr_tensor(idx.doc_ptr, idx.doc_term.long(), idx.doc_w, size=(nd, V))
        c = max(1, min(nq, (512 << 20) // (4 * nd)))         # the [nd, c] fp32 block <= 512 MiB
        from snx.retrieval import pack_rows
        qc, qt, qw = pack_rows(*q, V)
        qptr = torch.zeros(nq + 1, dtype=torch.long, device=dev)
        torch.cumsum(qc, 0, out=qptr[1:])
        Q = torch.sparse_csr_tensor(qptr, qt.long(), qw, size=(nq, V)).to_dense()
        done, t0 = 0, None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while done < nq:
            blk = Q[done:done + c].t().contiguous()
            s = D @ blk
            torch.topk(s.t(), 10, dim=1)
            done += blk.shape[1]
            torch.cuda.synchronize()
            if time.perf_counter() - t0 > budget_s:
                break
        t = time.perf_counter() - t0
        return {"ok": True, "queries_timed": done, "search_s": t, "queries_per_s": done / t, "query_block": c}
    except Exception as e:                                       # noqa: BLE001 -- reported, not hidden
        return {"ok": False, "error": f"{type(e).__name__}: {e}"[:300]}


def band_case(nd, nq, dev, lo=10, hi=50):
    from snx.retrieval import SparseIndex, exclusion_csr
    gen = torch.Generator().manual_seed(nd + nq)
    probs = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
    probs /= probs.sum()
    idx = SparseIndex(V, dev)
    for s in range(0, nd, 100_000):
        idx.add(*zipf_rows(min(100_000, nd - s), 128, gen, dev, probs))
    idx.build()
    q = zipf_rows(nq, 64, gen, dev, probs)
    m = max(1, nd // 100)
    ex_docs = torch.randint(0, nd, (nq * m,), generator=gen).to(dev)
    ex_ptr = torch.arange(0, nq * m + 1, m, dtype=torch.long, device=dev)
    t_norm, ex = sync_time(lambda: exclusion_csr((ex_ptr, ex_docs), nq, nd, dev))
    top, _, _, _ = idx.search(*q, 100)
    ceiling = (top[:, -1] * 0.5 + top[:, 0] * 0.5).contiguous()
    idx.search(q[0][:64], q[1][:64], q[2][:64], hi)

    def best(f):
        return min(sync_time(f)[0] for _ in range(3))

    t_search = best(lambda: idx.search(*q, hi))
    t_band = best(lambda: idx.search_band(*q, lo, hi, exclude=ex))
    t_band_ceil = best(lambda: idx.search_band(*q, lo, hi, exclude=ex, ceiling=ceiling))
    t_band_none = best(lambda: idx.search_band(*q, lo, hi))
    return {"docs": nd, "queries": nq, "band": [lo, hi], "excluded_per_query": m, "search_k_s": t_search,
            "band_s": t_band, "band_ceiling_s": t_band_ceil, "band_no_exclusion_s": t_band_none,
            "exclusion_normalise_s": t_norm, "band_over_search": t_band / t_search,
            "band_ceiling_over_search": t_band_ceil / t_search}


def seismic_case(nd, nq, dev, k=10, top_n=10):
    from snx.retrieval import SeismicIndex, SparseIndex
    from src.train.eval import cut_postings, overlap_at
    gen = torch.Generator().manual_seed(nd + nq)
    probs = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
    probs /= probs.sum()
    idx = SparseIndex(V, dev)
    for s in range(0, nd, 100_000):
        idx.add(*zipf_rows(min(100_000, nd - s), 128, gen, dev, probs))
    idx.build()
    q = zipf_rows(nq, 64, gen, dev, probs)
    idx.search(q[0][:64], q[1][:64], q[2][:64], k)

    def best(f):
        return min(sync_time(f)[0] for _ in range(3))

    t_exact = best(lambda: idx.search(*q, k))
    _, exact_docs, _, _ = idx.search(*q, k)
    SeismicIndex(idx, 300, 0.1, 0.4)                           # warm-up (code objects, allocator)
    t_build, six = sync_time(lambda: SeismicIndex(idx, 300, 0.1, 0.4))
    cut = int(cut_postings(idx, q, top_n).sum())
    row = {"docs": nd, "queries": nq, "k": k, "top_n": top_n, "build_s": t_build, "num_blocks": six.num_blocks,
           "summary_nnz": six.summary_nnz, "exact_search_s": t_exact, "exact_queries_per_s": nq / t_exact, "legs": []}
    for hf in (0.5, 1.0, 2.0):
        t = best(lambda: six.search(*q, k, top_n=top_n, heap_factor=hf))
        _, docs, _, _, stats = six.search(*q, k, top_n=top_n, heap_factor=hf)
        row["legs"].append({"heap_factor": hf, "search_s": t, "queries_per_s": nq / t, "over_exact": t / t_exact,
                            "overlap@10": overlap_at(docs.cpu().numpy(), exact_docs.cpu().numpy(), k),
                            "postings_frac": float(stats["postings_scored"].sum()) / cut if cut else 0.0})
    return row


def two_phase_case(nd, nq, dev, k=10, reps=5):
    from statistics import median
    from snx.retrieval import PRUNE_TYPES, SparseIndex
    from snx.retrieval.sparse import _keep_flags
    from src.train.eval import overlap_at
    gen = torch.Generator().manual_seed(nd + nq)
    probs = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
    probs /= probs.sum()
    idx = SparseIndex(V, dev)
    for s in range(0, nd, 100_000):
        idx.add(*zipf_rows(min(100_000, nd - s), 128, gen, dev, probs))
    idx.build()
    q = zipf_rows(nq, 64, gen, dev, probs)
    idx.search(*q, k)                                          # warm-up of both paths at the timed shapes
    idx.search_two_phase(*q, k)
    t_exact, t_two = [], []
    for _ in range(reps):                                      # alternating: both see the same machine state
        t_exact.append(sync_time(lambda: idx.search(*q, k))[0])
        t_two.append(sync_time(lambda: idx.search_two_phase(*q, k))[0])
    _, exact_docs, _, _ = idx.search(*q, k)
    _, docs, _, _, stats = idx.search_two_phase(*q, k)
    te, tt = median(t_exact), median(t_two)
    row = {"docs": nd, "queries": nq, "k": k, "prune": ["max_ratio", 0.4], "expansion_rate": 5.0, "window": 50,
           "exact_search_s": te, "exact_search_s_all": t_exact, "two_phase_s": tt, "two_phase_s_all": t_two,
           "exact_queries_per_s": nq / te, "two_phase_queries_per_s": nq / tt, "two_phase_over_exact": tt / te,
           "overlap@10": overlap_at(docs.cpu().numpy(), exact_docs.cpu().numpy(), k),
           "postings_frac": float(stats["postings_high"].sum()) / max(1, int(stats["postings_all"].sum())),
           "window_filled_mean": float(stats["window_filled"].double().mean()), "prune_kernel": {}}
    cnt = idx.doc_ptr[1:] - idx.doc_ptr[:-1]
    for name, value in (("max_ratio", 0.1), ("abs_value", 0.5), ("top_k", 64.0), ("alpha_mass", 0.9)):
        _keep_flags(cnt, idx.doc_w, PRUNE_TYPES[name], value)
        ts = [sync_time(lambda: _keep_flags(cnt, idx.doc_w, PRUNE_TYPES[name], value))[0] for _ in range(reps)]
        _, kept = _keep_flags(cnt, idx.doc_w, PRUNE_TYPES[name], value)
        row["prune_kernel"][name] = {"value": value, "seconds": median(ts), "entries_per_s": idx.nnz / median(ts),
                                     "kept_frac": int(kept.sum()) / idx.nnz}
    idx.pruned("max_ratio", 0.1)
    ts = [sync_time(lambda: idx.pruned("max_ratio", 0.1))[0] for _ in range(3)]
    row["pruned_build_s"] = median(ts)
    return row


def dict_rrf(docs, k=60.0, top_k=10):
    """ref:benchmark/score_fusion.py's rule over one query's lists of doc ids, as Python dicts (ties: lowest id first)."""
    ranks = [{d: i + 1 for i, d in enumerate(lst)} for lst in docs]
    max_rank = max([len(lst) + 1 for lst in docs] + [100])
    fused = {}
    for d in set().union(*ranks):
        acc = None
        for r in ranks:
            term = 1.0 / (k + r.get(d, max_rank))
            acc = term if acc is None else acc + term
        fused[d] = acc
    return sorted(fused.items(), key=lambda x: (-x[1], x[0]))[:top_k]


def hybrid_case(nd, nq, dev, reps=5, host_queries=200):
    from statistics import median
    from snx.retrieval import Bm25Index, fuse_ranked
    gen = torch.Generator().manual_seed(nd + nq)
    probs = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
    probs /= probs.sum()
    allowed = torch.ones(V, dtype=torch.uint8, device=dev)

    def tokens(n, m):
        ids = torch.multinomial(probs, n * m, replacement=True, generator=gen).view(n, m).to(dev)
        return ids, torch.ones_like(ids)
    batches = [tokens(min(100_000, nd - s), 128) for s in range(0, nd, 100_000)]
    qi, qm = tokens(nq, 16)

    def build():
        bm = Bm25Index(V, dev)
        for ids, mask in batches:
            bm.add_tokens(ids, mask, allowed)
        return bm.build()
    build()                                                    # warm-up
    ts = [sync_time(build)[0] for _ in range(3)]
    bm = build()
    bm.search_tokens(qi, qm, allowed, 100)
    tq = [sync_time(lambda: bm.search_tokens(qi, qm, allowed, 100))[0] for _ in range(reps)]
    row = {"docs": nd, "queries": nq, "doc_tokens": 128, "query_tokens": 16, "bm25_build_s": median(ts),
           "bm25_build_docs_per_s": nd / median(ts), "bm25_nnz": bm.index.nnz, "avgdl": bm.avgdl,
           "bm25_search_s": median(tq), "bm25_search_queries_per_s": nq / median(tq), "fuse": []}
    targets = torch.randint(0, nd, (nq,), generator=gen).to(torch.int32).to(dev)
    for R in (100, 1000):
        pool = min(nd, 4 * R)                                  # lists drawn from a pool of 4 R docs: heavy overlap
        lists = []
        for _ in range(3):
            d = torch.argsort(torch.rand(nq, pool, generator=gen), 1)[:, :R].to(torch.int32).to(dev)
            sc = torch.sort(torch.rand(nq, R, generator=gen), 1, descending=True)[0].to(dev)
            lists.append((d, sc))
        for L in (2, 3):
            fuse_ranked(lists[:L], "rrf", 10, targets=targets)
            tf = [sync_time(lambda: fuse_ranked(lists[:L], "rrf", 10, targets=targets))[0] for _ in range(reps)]
            _, gd, _, _ = fuse_ranked(lists[:L], "rrf", 10, targets=targets)
            m = min(nq, host_queries)
            host = [lst[0][:m].cpu().tolist() for lst in lists[:L]]
            t0 = time.perf_counter()
            hd = [[d for d, _ in dict_rrf([h[q] for h in host])] for q in range(m)]
            th = time.perf_counter() - t0
            row["fuse"].append({"R": R, "L": L, "seconds": median(tf), "queries_per_s": nq / median(tf),
                                "python_dict_queries": m, "python_dict_queries_per_s": m / th,
                                "same_docs_as_python": gd[:m].cpu().tolist() == hd})
    return row


def qrels_case(nd, nq, dev, reps=5, host_queries=2000):
    from statistics import median
    import numpy as np
    from snx.retrieval import SparseIndex, bootstrap_indices, bootstrap_means, ranked_relevance, relevance_csr
    gen = torch.Generator().manual_seed(nd + nq)
    probs = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
    probs /= probs.sum()
    idx = SparseIndex(V, dev)
    for s in range(0, nd, 100_000):
        idx.add(*zipf_rows(min(100_000, nd - s), 128, gen, dev, probs))
    idx.build()
    q = zipf_rows(nq, 64, gen, dev, probs)
    rng = np.random.default_rng(nd + nq)
    rows = [sorted(set(rng.integers(0, nd, int(rng.integers(1, 9))).tolist())) for _ in range(nq)]
    rel = relevance_csr(rows, nq, nd, dev)
    width = max(len(r) for r in rows)

    def emulated():
        best = torch.zeros(nq, dtype=torch.int32)
        for j in range(width):
            tgt = torch.tensor([r[j] if j < len(r) else 0 for r in rows], dtype=torch.int32, device=dev)
            live = torch.tensor([j < len(r) for r in rows])
            rk = idx.search(*q, 1, targets=tgt)[2].cpu()
            use = live & (rk > 0) & ((best == 0) | (rk < best))
            best = torch.where(use, rk, best)
        return best
    idx.first_relevant(*q, rel)
    t_new = median(sync_time(lambda: idx.first_relevant(*q, rel))[0] for _ in range(reps))
    t_old, best = sync_time(emulated)
    rank = idx.first_relevant(*q, rel)[2]
    row = {"docs": nd, "queries": nq, "mean_row": sum(len(r) for r in rows) / nq, "max_row": width,
           "first_relevant_s": t_new, "per_doc_search_min_s": t_old, "speedup": t_old / t_new,
           "same_ranks": bool(torch.equal(best, rank.cpu()))}
    docs = idx.search(*q, 100)[1]
    ranked_relevance(docs, rel, nd)
    t_rr = median(sync_time(lambda: ranked_relevance(docs, rel, nd))[0] for _ in range(reps))
    m = min(nq, host_queries)

    def set_loop():                                            # ref:benchmark/hf_runner.py:198-203 per query
        lists = docs[:m].cpu().tolist()
        out = []
        for qi in range(m):
            relevant, hit = set(rows[qi]), 0
            for r, d in enumerate(lists[qi], 1):
                if d < 0:
                    break
                if d in relevant:
                    hit = r
                    break
            out.append(hit)
        return out
    t_loop, first_host = sync_time(set_loop)
    first = ranked_relevance(docs, rel, nd)[0]
    row.update(ranked_relevance_s=t_rr, ranked_relevance_queries_per_s=nq / t_rr, python_set_loop_queries=m,
               python_set_loop_queries_per_s=m / t_loop, same_first_as_python=first[:m].cpu().tolist() == first_host)
    vals = np.stack([(rng.random(nq) < 0.4).astype(np.float64), rng.random(nq), rng.random(nq)], 1)
    t0 = time.perf_counter()
    bidx = bootstrap_indices(nq, 1000, 42)
    t_draw = time.perf_counter() - t0
    bootstrap_means(vals, indices=bidx, device=dev)
    t_bm = median(sync_time(lambda: bootstrap_means(vals, indices=bidx, device=dev))[0] for _ in range(reps))

    def numpy_loop():                                          # ref:benchmark/metrics.py:198-206 with array metrics
        np.random.seed(42)
        out = np.empty((1000, 3))
        for b in range(1000):
            ind = np.random.choice(nq, size=nq, replace=True)
            for c in range(3):
                out[b, c] = np.mean(vals[ind, c])
        return out
    t_np, host = sync_time(numpy_loop)
    got = bootstrap_means(vals, indices=bidx, device=dev).cpu().numpy()
    row.update(bootstrap_means_s=t_bm, bootstrap_index_draw_s=t_draw, numpy_loop_s=t_np,
               bootstrap_max_abs_diff=float(np.abs(got - host).max()))
    return row


def miner_case(n_records, dev):
    import tempfile
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.data import SyntheticTripletDataset
    from src.train.data.collator import create_tokenizer
    from src.train.mining import mine_negatives
    ds = SyntheticTripletDataset(n_records, num_negatives=3, seed=1)
    with tempfile.TemporaryDirectory() as d:
        for sh in range(2):
            with open(os.path.join(d, f"train_{sh:02d}.jsonl"), "w") as f:
                for i in range(sh, n_records, 2):
                    f.write(json.dumps(ds[i]) + "\n")
        torch.manual_seed(0)
        model = SPLADEModernBERT(model_name="skt/A.X-Encoder-base").to(dev)
        tok = create_tokenizer("hash:50000")
        files = sorted(os.path.join(d, f) for f in os.listdir(d))
        t, summ = sync_time(lambda: mine_negatives(model, tok, files, os.path.join(d, "out"), device=dev))
    return {"records": summ["records"], "docs": summ["docs"], "queries": summ["queries"], "seconds": t,
            "docs_per_s": summ["docs"] / t, "queries_per_s": summ["queries"] / t, "band_fill": summ["band_fill"]}


def dense_case(nd, dev, nq=4096, D=1024, k=100, reps=5):
    import statistics
    from snx.retrieval import DenseIndex
    gen = torch.Generator(device=dev).manual_seed(7)
    if nd <= 0:
        free, _ = torch.cuda.mem_get_info(dev)
        nd = min(1 << 22, int(free // 4 // (4 * nq)))
    nd = max(128, nd // 128 * 128)
    docs = torch.nn.functional.normalize(torch.randn(nd, D, generator=gen, device=dev), dim=1)
    q = torch.nn.functional.normalize(torch.randn(nq, D, generator=gen, device=dev), dim=1)
    t_build, idx = sync_time(lambda: (lambda i: (i.add(docs), i.build())[1])(DenseIndex(D, dev)))

    def ours():
        return idx.search(q, k)

    def ref():
        out = []
        for s in range(0, nq, 4096):
            out.append(torch.topk(torch.mm(q[s:s + 4096], docs.T), k, dim=1))
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

    sync_time(ours)
    sync_time(ref)
    t_ours, t_ref = [], []
    for _ in range(reps):
        t, (sc, dc, _, _) = sync_time(ours)
        t_ours.append(t)
        t, (rs, rd) = sync_time(ref)
        t_ref.append(t)
    # same lists: torch's sums round in another order, so only ranks whose neighbours are further apart than that count
    gap = torch.minimum((rs[:, :-1] - rs[:, 1:]).abs()[:, :-1], (rs[:, 1:] - rs[:, 2:]).abs())
    clear = gap > 1e-5
    agree = float((dc[:, 1:-1].long() == rd[:, 1:-1])[clear].float().mean()) if bool(clear.any()) else 1.0
    mo, mr = statistics.median(t_ours), statistics.median(t_ref)
    flop = 2.0 * nq * nd * D
    return {"dense": {"nd": nd, "nq": nq, "D": D, "k": k, "build_s": t_build, "search_s": t_ours, "torch_mm_topk_s": t_ref,
                      "search_median_s": mo, "torch_median_s": mr, "search_spread": (max(t_ours) - min(t_ours)) / mo,
                      "torch_spread": (max(t_ref) - min(t_ref)) / mr, "ratio_torch_over_ours": mr / mo,
                      "search_tflops": flop / mo / 1e12, "torch_tflops": flop / mr / 1e12,
                      "score_matrix_bytes_avoided": 4 * min(nq, 4096) * nd, "max_abs_score_diff": float((sc - rs).abs().max()),
                      "rank_agreement_where_clear": agree}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000x200,100000x10000,1000000x10000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--band", action="store_true", help="search_band vs search, then an end-to-end miner run")
    ap.add_argument("--miner-records", type=int, default=4000)
    ap.add_argument("--seismic", action="store_true", help="SeismicIndex build and search against exact search")
    ap.add_argument("--two-phase", action="store_true", help="search_two_phase, the prune kernel and pruned() vs search")
    ap.add_argument("--hybrid", action="store_true", help="Bm25Index build and search, fuse_ranked vs Python dicts")
    ap.add_argument("--qrels", action="store_true", help="first_relevant, ranked_relevance, bootstrap_means vs host loops")
    ap.add_argument("--dense", action="store_true", help="DenseIndex.search vs torch.mm + topk at nq 4096, D 1024, k 100")
    ap.add_argument("--dense-docs", type=int, default=0, help="corpus size (0: what the torch form's score matrix allows)")
    ap.add_argument("--dense-reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    if args.dense:
        rows.append(dense_case(args.dense_docs, dev, reps=args.dense_reps))
        print(json.dumps(rows[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        return
    if args.qrels:
        sizes = args.sizes if args.sizes != ap.get_default("sizes") else "100000x2000,1000000x2000"
        for s in sizes.split(","):
            nd, nq = (int(x) for x in s.split("x"))
            rows.append(qrels_case(nd, nq, dev))
            print(json.dumps(rows[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        return
    if args.hybrid:
        sizes = args.sizes if args.sizes != ap.get_default("sizes") else "100000x10000,1000000x10000"
        for s in sizes.split(","):
            nd, nq = (int(x) for x in s.split("x"))
            rows.append(hybrid_case(nd, nq, dev))
            print(json.dumps(rows[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        return
    if args.two_phase:
        sizes = args.sizes if args.sizes != ap.get_default("sizes") else "100000x10000,1000000x10000"
        for s in sizes.split(","):
            nd, nq = (int(x) for x in s.split("x"))
            rows.append(two_phase_case(nd, nq, dev))
            print(json.dumps(rows[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        return
    if args.seismic:
        sizes = args.sizes if args.sizes != ap.get_default("sizes") else "1000000x10000"
        for s in sizes.split(","):
            nd, nq = (int(x) for x in s.split("x"))
            rows.append(seismic_case(nd, nq, dev))
            print(json.dumps(rows[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        return
    if args.band:
        sizes = args.sizes if args.sizes != ap.get_default("sizes") else "1000000x10000"
        for s in sizes.split(","):
            nd, nq = (int(x) for x in s.split("x"))
            rows.append(band_case(nd, nq, dev))
            print(json.dumps(rows[-1]), flush=True)
        if args.miner_records > 0:
            rows.append({"miner": miner_case(args.miner_records, dev)})
            print(json.dumps(rows[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        return
    for s in args.sizes.split(","):
        nd, nq = (int(x) for x in s.split("x"))
        row = run_case(nd, nq, dev, torch_cmp=not args.no_torch)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

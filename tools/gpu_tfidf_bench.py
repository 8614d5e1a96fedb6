#!/usr/bin/env python3
"""Character n-gram TF-IDF hard-negative mining: the GPU path at 50,000 and 1,000,000 documents, and scikit-learn plus a
chunked scipy product on the CPU at 50,000 where scikit-learn is installed.

    python tools/gpu_tfidf_bench.py [--docs 50000,1000000] [--queries 2000] [--cpu-docs 50000] [--repeats 3]

Synthetic documents of 12 .. 18 pseudo-words (Hangul syllables and Latin letters, about 80 code points), queries of 3 .. 6
words of which half come from one document.  The GPU side is snx.retrieval.TfidfIndex with the reference's settings
(ngram_range (2, 3), max_features 30000, sublinear tf), timed in three parts that each end in a device synchronise:
``fit`` (fit_add: Python's lower / split / join, the code-point CSR, the row kernel), ``build`` (the device-wide unique,
the vocabulary, the weights, the SparseIndex) and ``mine`` (search_texts of all queries in batches of 1000, top 10, hits
copied to the host).  The median, minimum and maximum of ``--repeats`` runs after one warm-up run go into one JSON line per
size.  The CPU side is TfidfVectorizer(analyzer="char_wb", ngram_range=(2, 3), max_features=30000, sublinear_tf=True)
.fit_transform, normalize, and queries @ corpus.T in corpus chunks of 10,000 with argpartition -- the same three parts, the
same repeats; at equal sizes the line also says for how many queries both sides chose the same best document.  Nothing is
asserted about speed."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SETTINGS = dict(ngram_range=(2, 3), max_features=30000, sublinear_tf=True)
TOP_K, BATCH, CPU_CHUNK = 10, 1000, 10000


def synth(n_docs: int, n_queries: int, query_docs: int, seed: int = 0):
    r = random.Random(seed)
    syll = [chr(c) for c in range(0xAC00, 0xAC00 + 28 * 40, 28)]         # 40 open Hangul syllables
    vocab = ["".join(r.choice(syll) for _ in range(r.randint(1, 4))) for _ in range(15000)] + \
            ["".join(r.choice("abcdefghijklmnoprstuvwyz") for _ in range(r.randint(2, 8))) for _ in range(15000)]
    docs = [" ".join(r.choice(vocab) for _ in range(r.randint(12, 18))) for _ in range(n_docs)]
    queries = []
    for _ in range(n_queries):
        words = docs[r.randrange(query_docs)].split(" ")           # a document every timed size holds
        k = r.randint(3, 6)
        queries.append(" ".join(r.sample(words, k // 2) + [r.choice(vocab) for _ in range(k - k // 2)]))
    return docs, queries


def summary(runs):
    return {"median_s": round(statistics.median(runs), 4), "min_s": round(min(runs), 4), "max_s": round(max(runs), 4)}


def gpu_run(docs, queries, repeats, device, fit_batch=100000):
    import torch
    from snx.retrieval import TfidfIndex
    parts = {"fit": [], "build": [], "mine": []}
    best = None
    for it in range(repeats + 1):
        tf = TfidfIndex(device, **SETTINGS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(0, len(docs), fit_batch):
            tf.fit_add(docs[b:b + fit_batch])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tf.build()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        hits = [tf.search_texts(queries[b:b + BATCH], TOP_K)[1].cpu().numpy() for b in range(0, len(queries), BATCH)]
        t3 = time.perf_counter()                                 # the copy to the host synchronises
        if it:                                                   # the first pass warms up
            parts["fit"].append(t1 - t0)
            parts["build"].append(t2 - t1)
            parts["mine"].append(t3 - t2)
        best = np.concatenate(hits)[:, 0]
        features, nnz = int(tf.feature_keys.numel()), int(tf.index.doc_term.numel())
        del tf
        torch.cuda.empty_cache()
    return parts, best, features, nnz


def cpu_run(docs, queries, repeats):
    from sklearn.feature_extraction.text import TfidfVectorizer
    from sklearn.preprocessing import normalize
    parts = {"fit": [], "build": [], "mine": []}
    best = None
    for it in range(repeats + 1):
        t0 = time.perf_counter()
        vec = TfidfVectorizer(analyzer="char_wb", **SETTINGS)
        corpus = normalize(vec.fit_transform(docs), norm="l2", axis=1, copy=False)     # fit and build are one call here
        t1 = time.perf_counter()
        out = []
        for b in range(0, len(queries), BATCH):
            q = normalize(vec.transform(queries[b:b + BATCH]), norm="l2", axis=1, copy=False)
            top_s = np.full((q.shape[0], 0), 0.0)
            top_d = np.zeros((q.shape[0], 0), dtype=np.int64)
            for c in range(0, corpus.shape[0], CPU_CHUNK):
                s = (q @ corpus[c:c + CPU_CHUNK].T).toarray()
                s = np.concatenate([top_s, s], axis=1)
                d = np.concatenate([top_d, np.broadcast_to(np.arange(c, c + s.shape[1] - top_d.shape[1]),
                                                           (q.shape[0], s.shape[1] - top_d.shape[1]))], axis=1)
                keep = np.argpartition(-s, min(TOP_K, s.shape[1] - 1), axis=1)[:, :TOP_K]
                top_s, top_d = np.take_along_axis(s, keep, 1), np.take_along_axis(d, keep, 1)
            out.append(top_d[np.arange(q.shape[0]), np.argmax(top_s, axis=1)])
        t2 = time.perf_counter()
        if it:
            parts["fit"].append(t1 - t0)
            parts["build"].append(0.0)
            parts["mine"].append(t2 - t1)
        best = np.concatenate(out)
    return parts, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=str, default="50000,1000000")
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--cpu-docs", type=int, default=50000, help="0: no CPU side")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_tfidf_bench: needs a GPU; a CPU timing says nothing about it")
    sizes = [int(x) for x in args.docs.split(",") if x]
    docs, queries = synth(max(sizes + [args.cpu_docs]), args.queries, min(sizes + ([args.cpu_docs] if args.cpu_docs else [])))
    gpu_best = {}
    for n in sizes:
        q = queries
        parts, best, features, nnz = gpu_run(docs[:n], q, args.repeats, args.device)
        gpu_best[n] = best
        line = {"bench": "tfidf_gpu", "docs": n, "queries": len(q), "runs": args.repeats, "features": features,
                "index_nnz": nnz}
        for k, v in parts.items():
            line[k] = summary(v)
        line["total_median_s"] = round(sum(statistics.median(v) for v in parts.values()), 4)
        print(json.dumps(line), flush=True)
    if args.cpu_docs:
        try:
            import sklearn  # noqa: F401
        except ImportError:
            print(json.dumps({"bench": "tfidf_cpu", "skipped": "scikit-learn is not installed"}), flush=True)
            return
        n = args.cpu_docs
        parts, best = cpu_run(docs[:n], queries, args.repeats)
        line = {"bench": "tfidf_cpu", "docs": n, "queries": len(queries), "runs": args.repeats,
                "what": "TfidfVectorizer + normalize + chunked scipy product"}
        for k in ("fit", "mine"):
            line[k] = summary(parts[k])
        line["total_median_s"] = round(sum(statistics.median(parts[k]) for k in ("fit", "mine")), 4)
        if n in gpu_best:
            line["same_best_document"] = int((gpu_best[n] == best).sum())
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

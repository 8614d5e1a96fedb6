"""A checkpoint against a benchmark directory with qrels, scored the way the reference's benchmark runner scores
(ref:benchmark/hf_runner.py:191-237 over ref:benchmark/hf_data_loader.py:401-459 data), offline on one GPU.

    python -m src.train.cli.eval_benchmark --checkpoint outputs/train_v33/final_model --benchmark-dir data/bench \\
        [--methods sparse,bm25,bm25_sparse_rrf,two_phase,seismic] [--top-k 10] [--bootstrap 1000] [--max-queries N] \\
        [--report OUT.json] [--methods sparse,doc_only --idf outputs/idf_weights/idf]

The directory holds ``corpus.jsonl``, ``queries.jsonl`` and ``qrels.jsonl`` (src.train.eval.load_benchmark_dir).  Every
method returns its top ``--top-k`` docs per query; a hit is the first returned doc that is in the query's relevant set.
One JSON line per method: recall@1/5/10, mrr, ndcg@10 under that rule, recall_frac@c and ndcg_multi@c over all relevant
docs, ``ci`` (bootstrap intervals of recall@1, mrr and ndcg@10: the reference's resamples, the means formed on the GPU),
``wall_s`` (the method's batch search time over all queries -- NOT the per-request latency percentiles of the
reference's table, which time an OpenSearch round trip and are not claimed here) and, for ``sparse``,
``first_relevant``: the rank of each query's best relevant doc in the WHOLE corpus, not only the top k.  Then one line per
method pair with the paired t-test over reciprocal first-relevant ranks (hf_runner.run_statistical_tests).  ``--report``
writes {method: metrics} with the reference's key names.  One process (not torchrun).
``doc_only`` (not in the default list; needs ``--idf``, an IDF table of src.train.cli.compute_idf): ``sparse`` over the same
document index, but the queries are never encoded -- their rows are idf[token] once per distinct kept token
(snx.idf.idf_query_rows), OpenSearch's inference-free query mode.  It joins the pairwise t-tests like any other method."""
from __future__ import annotations

import argparse
import json
import time
from typing import List, Optional

METHODS = ("sparse", "bm25", "bm25_sparse_rrf", "two_phase", "seismic")   # the default list
OPTIONAL_METHODS = ("doc_only",)                                            # run when named; doc_only needs --idf
RRF_K = 60                   # ref:benchmark/hybrid_searcher.py:621-631
RETRIEVAL_K = 100            # depth of the two lists a fused row is formed from
CI_KEYS = ("recall@1", "mrr", "ndcg@10")


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="retrieval methods against a benchmark directory with qrels (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--checkpoint", type=str, default=None,
                    help="checkpoint directory holding model.pt, or a model.pt file (default: random init)")
    ap.add_argument("--model-name", type=str, default="skt/A.X-Encoder-base")
    ap.add_argument("--tokenizer", type=str, default=None, help="tokenizer dir or hash:<vocab> (default: --model-name)")
    ap.add_argument("--benchmark-dir", type=str, required=True)
    ap.add_argument("--methods", type=str, default=",".join(METHODS))
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--bootstrap", type=int, default=1000, help="resamples of the confidence intervals (0: none)")
    ap.add_argument("--max-queries", type=int, default=None)
    ap.add_argument("--report", type=str, default=None, help="write {method: metrics} with the reference's key names")
    ap.add_argument("--query-max-length", type=int, default=64)
    ap.add_argument("--doc-max-length", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--idf", type=str, default=None,
                    help="IDF table for the doc_only method (path without extension: .bin + .json; or a .pt tensor)")
    args = ap.parse_args(argv)
    args.methods = [m for m in args.methods.split(",") if m]
    bad = [m for m in args.methods if m not in METHODS + OPTIONAL_METHODS]
    if bad or not args.methods or len(set(args.methods)) != len(args.methods):
        ap.error(f"--methods: distinct names out of {','.join(METHODS + OPTIONAL_METHODS)}")
    if "doc_only" in args.methods and not args.idf:
        ap.error("--methods doc_only needs --idf PATH")
    if not 10 <= args.top_k <= RETRIEVAL_K:
        ap.error(f"--top-k must lie in [10, {RETRIEVAL_K}] (the metrics read cutoffs 1, 5 and 10)")
    if args.bootstrap < 0:
        ap.error("--bootstrap must be >= 0")
    return args


def main(argv: Optional[List[str]] = None) -> List[dict]:
    args = parse_args(argv)
    import numpy as np
    import torch
    from snx.retrieval import SeismicIndex, fuse_ranked, ranked_relevance
    from src.train.cli.mine_negatives import load_model
    from src.train.data.collator import create_tokenizer
    from src.train.eval import (QRELS_CUTOFFS, REPORT_KEYS, BenchmarkEvaluator, bm25_index, bootstrap_confidence_interval,
                                cat_query_rows, first_relevant_values, hybrid_params, load_benchmark_dir, paired_t_test,
                                qrels_metrics)
    device = torch.device("cuda:0")
    data = load_benchmark_dir(args.benchmark_dir, args.max_queries)
    if not data.queries or not data.docs:
        raise ValueError(f"{args.benchmark_dir}: no queries or no docs to evaluate")
    tokenizer = create_tokenizer(args.tokenizer or args.model_name)
    model = load_model(args, device)
    ev = BenchmarkEvaluator(tokenizer, data, device=str(device), query_max_length=args.query_max_length,
                            doc_max_length=args.doc_max_length, batch_size=args.batch_size)
    index, queries = ev.encode(model)
    nq, nd, k = len(data.queries), len(data.docs), args.top_k
    bm = bm_queries = None
    if any(m.startswith("bm25") for m in args.methods):
        bm, bm_queries = bm25_index(ev, index.V, hybrid_params({}))
    _, _, fr_rank, nrel = index.first_relevant(*queries, ev.relevant)
    idf_queries = None
    if "doc_only" in args.methods:
        from snx.idf import load_idf
        table = load_idf(args.idf)[0]
        if table.shape[0] < index.V:                            # an id the IDF corpus never showed: as rare as the rarest
            table = np.concatenate([table, np.full(index.V - table.shape[0], table.max(), dtype=np.float32)])
        ev.query_idf = torch.from_numpy(np.ascontiguousarray(table[:index.V]))
        idf_queries = cat_query_rows(list(ev._idf_queries(index.V)))

    def run(method: str) -> torch.Tensor:
        if method == "sparse":
            return index.search(*queries, k)[1]
        if method == "doc_only":
            return index.search(*idf_queries, k)[1]
        if method == "bm25":
            return bm.index.search(*bm_queries, k)[1]
        if method == "bm25_sparse_rrf":                         # list 0 = BM25, as in the reference's hybrid searcher
            b_s, b_d, _, _ = bm.index.search(*bm_queries, RETRIEVAL_K)
            s_s, s_d, _, _ = index.search(*queries, RETRIEVAL_K)
            return fuse_ranked([(b_d, b_s), (s_d, s_s)], "rrf", k, k=RRF_K)[1]
        if method == "two_phase":
            return index.search_two_phase(*queries, k)[1]
        return SeismicIndex(index).search(*queries, k)[1]

    lines, ranks = [], {}
    for method in args.methods:
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        docs = run(method)
        torch.cuda.synchronize(device)
        wall = time.perf_counter() - t0
        first, hits, dcg = ranked_relevance(docs, ev.relevant, nd, QRELS_CUTOFFS)
        ranks[method] = first.cpu().tolist()
        line = dict(method=method, num_docs=nd, top_k=k, **qrels_metrics(first, hits, dcg, nrel, QRELS_CUTOFFS, k=k))
        if args.bootstrap:
            cols = [list(REPORT_KEYS).index(key) for key in CI_KEYS]
            vals = first_relevant_values(first, k)[:, cols]
            ci = bootstrap_confidence_interval(vals, n_bootstrap=args.bootstrap, seed=42, device=device)
            line["ci"] = dict(zip(CI_KEYS, ci))
        if method == "sparse":
            r = fr_rank.cpu().numpy().astype(np.int64)
            found = r[r > 0]
            line["first_relevant"] = dict(
                found=int(found.size), mean_rank=float(found.mean()) if found.size else 0.0,
                median_rank=float(np.median(found)) if found.size else 0.0, max_rank=int(found.max()) if found.size else 0,
                mrr_full=float(np.mean(np.where(r > 0, 1.0 / np.maximum(r, 1), 0.0))))
        line["wall_s"] = wall
        lines.append(line)
        print(json.dumps(line), flush=True)
    for i, a in enumerate(args.methods):                        # ref:benchmark/hf_runner.py:217-237
        for b in args.methods[i + 1:]:
            t = paired_t_test(ranks[a], ranks[b], k=k)
            # json has no nan: a t-test without variation is written as null
            line = dict(test=f"{a}_vs_{b}", statistic=None if t["statistic"] != t["statistic"] else t["statistic"],
                        p_value=None if t["p_value"] != t["p_value"] else t["p_value"], significant=t["significant"])
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.report:
        report = {x["method"]: {**{REPORT_KEYS[key]: x[key] for key in REPORT_KEYS}, "num_queries": x["num_queries"]}
                  for x in lines if "method" in x}
        with open(args.report, "w") as f:
            json.dump({"metrics": report}, f, indent=1)
    return lines


if __name__ == "__main__":
    main()

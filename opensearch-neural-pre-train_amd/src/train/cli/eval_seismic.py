"""SEISMIC parameter sweeps of a checkpoint against exact retrieval, offline (snx.retrieval.SeismicIndex).

    python -m src.train.cli.eval_seismic --checkpoint outputs/train_v33/final_model --val-file data/val.jsonl \\
        --reference-sweep

The reference measures what SEISMIC costs on a live OpenSearch cluster, against a generous SEISMIC index as its
baseline (ref:scripts/neural_sparse_search_aws.py:929-958, 1314-1510).  Here the evaluator's corpus is encoded once, the
exact index is built once and is the baseline, and one SeismicIndex is built per index setting; every query setting
runs on it.  ``--reference-sweep`` runs the reference's two one-dimensional sweeps as it ran them (14 index settings at
the default query, then 7 query settings on the default index; duplicates of the default kept).  One JSON line per
(index, query) setting: the parameters, the exact metrics, the seismic_* metrics, overlap@5, the counters' means,
build_s and search_s.  One process (not torchrun)."""
from __future__ import annotations

import argparse
import itertools
import json
from typing import List, Optional, Tuple

DEFAULT_INDEX = (300, 0.1, 0.4)        # n_postings, cluster_ratio, summary_prune_ratio: ref :1326-1329
DEFAULT_QUERY = (10, 1.0)              # top_n, heap_factor


def reference_sweep() -> List[Tuple[tuple, List[tuple]]]:
    """ref:scripts/neural_sparse_search_aws.py:1314-1430 (index) and :1443-1510 (query), in its order."""
    n, r, a = DEFAULT_INDEX
    index = [(x, r, a) for x in (10, 50, 100, 300, 500, 1000)] + [(n, x, a) for x in (0.01, 0.05, 0.2, 0.5)] + \
            [(n, r, x) for x in (0.1, 0.2, 0.6, 0.8)]
    groups = [(i, [DEFAULT_QUERY]) for i in index]
    queries = [DEFAULT_QUERY] + [(DEFAULT_QUERY[0], h) for h in (0.5, 1.0, 2.0)] + \
              [(t, DEFAULT_QUERY[1]) for t in (5, 10, 20)]
    groups.append((DEFAULT_INDEX, queries))
    return groups


def _list(kind):
    def parse(s: str):
        try:
            vals = [kind(x) for x in s.split(",") if x.strip()]
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e))
        if not vals:
            raise argparse.ArgumentTypeError("empty list")
        return vals
    return parse


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="SEISMIC sweeps against exact sparse retrieval (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--checkpoint", type=str, default=None,
                    help="checkpoint directory holding model.pt, or a model.pt file (default: random init)")
    ap.add_argument("--model-name", type=str, default="skt/A.X-Encoder-base")
    ap.add_argument("--tokenizer", type=str, default=None, help="tokenizer dir or hash:<vocab> (default: --model-name)")
    ap.add_argument("--val-file", type=str, default="data/v29.0_kd/val.jsonl")
    ap.add_argument("--max-queries", type=int, default=2000)
    ap.add_argument("--max-docs", type=int, default=50000)
    ap.add_argument("--query-max-length", type=int, default=64)
    ap.add_argument("--doc-max-length", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--n-postings", type=_list(int), default=[DEFAULT_INDEX[0]])
    ap.add_argument("--cluster-ratio", type=_list(float), default=[DEFAULT_INDEX[1]])
    ap.add_argument("--summary-prune-ratio", type=_list(float), default=[DEFAULT_INDEX[2]])
    ap.add_argument("--top-n", type=_list(int), default=[DEFAULT_QUERY[0]])
    ap.add_argument("--heap-factor", type=_list(float), default=[DEFAULT_QUERY[1]])
    ap.add_argument("--reference-sweep", action="store_true",
                    help="the reference's 14 index + 7 query settings instead of the lists")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON lines to this file")
    args = ap.parse_args(argv)
    if any(x < 1 for x in args.n_postings + args.top_n):
        ap.error("--n-postings and --top-n must be >= 1")
    if any(not 0 < x <= 1 for x in args.cluster_ratio + args.summary_prune_ratio):
        ap.error("--cluster-ratio and --summary-prune-ratio must lie in (0, 1]")
    if any(not x > 0 for x in args.heap_factor):
        ap.error("--heap-factor must be > 0")
    return args


def settings(args: argparse.Namespace) -> List[Tuple[tuple, List[tuple]]]:
    """[(index setting, [query settings])] in run order."""
    if args.reference_sweep:
        return reference_sweep()
    queries = list(itertools.product(args.top_n, args.heap_factor))
    return [(i, queries) for i in itertools.product(args.n_postings, args.cluster_ratio, args.summary_prune_ratio)]


def main(argv: Optional[List[str]] = None) -> List[dict]:
    args = parse_args(argv)
    import torch
    from snx.retrieval import SeismicIndex
    from src.train.cli.mine_negatives import load_model
    from src.train.data.collator import create_tokenizer
    from src.train.eval import RETRIEVAL_SIZE, MidTrainingEvaluator, metrics_from_ranks, seismic_eval
    device = torch.device("cuda:0")
    tokenizer = create_tokenizer(args.tokenizer or args.model_name)
    model = load_model(args, device)
    ev = MidTrainingEvaluator(tokenizer, args.val_file, max_queries=args.max_queries, max_docs=args.max_docs,
                              device=str(device), query_max_length=args.query_max_length,
                              doc_max_length=args.doc_max_length, batch_size=args.batch_size)
    index, queries = ev.encode(model)
    if queries is None:
        raise ValueError(f"{args.val_file}: no queries or no docs to evaluate")
    targets = torch.tensor(ev.corpus.targets, dtype=torch.int32, device=device)
    _, exact_docs, rank, _ = index.search(*queries, RETRIEVAL_SIZE, targets=targets)
    exact = metrics_from_ranks(rank.cpu().tolist())
    lines = []
    out = open(args.out, "w") if args.out else None
    try:
        for (n, r, a), qsets in settings(args):
            six = SeismicIndex(index, n, r, a)
            for top_n, hf in qsets:
                params = {"n_postings": n, "cluster_ratio": r, "summary_prune_ratio": a, "top_n": top_n,
                          "heap_factor": hf}
                m, info = seismic_eval(index, queries, targets, exact_docs, params, six=six)
                line = dict(params, num_queries=len(ev.corpus.queries), num_docs=len(ev.corpus.docs), **exact, **m)
                line["overlap@5"] = m["seismic_overlap@5"]
                line.update({k: info[k] for k in ("blocks_total", "blocks_scored", "postings_scored")})
                line.update(num_blocks=six.num_blocks, summary_nnz=six.summary_nnz, build_s=info["build_s"],
                            search_s=info["search_s"])
                lines.append(line)
                text = json.dumps(line)
                print(text, flush=True)
                if out:
                    out.write(text + "\n")
    finally:
        if out:
            out.close()
    return lines


if __name__ == "__main__":
    main()

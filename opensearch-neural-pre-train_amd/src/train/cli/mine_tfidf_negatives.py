"""Lexical hard negatives for raw triplet shards by character n-gram TF-IDF on one GPU (src.train.mining.tfidf,
snx.retrieval.TfidfIndex): the reference's ``scripts/mine_hard_negatives.py`` with its flags and defaults.

    python -m src.train.cli.mine_tfidf_negatives --data-dir data/v29.0 --output-dir data/v29.0_neg --max-corpus 1000000

Every record of ``train_shard_*.jsonl`` without a ``negative`` receives the best tf-idf cosine hit among the unique
positives that is not its own positive, and ``difficulty = "hard"``; without ``--output-dir`` the shards are rewritten in
place.  ``--max-corpus`` keeps the reference's default of 50,000, the most its scikit-learn form affords; the GPU index
has no such limit.  ``--corpus-chunk-size`` is accepted for compatibility and ignored: no score matrix exists here.  One
JSON line of stats goes to stdout: total, already_had_negative, added, failed, corpus, features, seconds.  Runs as a single
process."""
from __future__ import annotations

import argparse
import json
import logging
import time
from pathlib import Path
from typing import List, Optional


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="TF-IDF hard negative mining of triplet shards (GPU)",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--data-dir", type=Path, default=Path("data/v29.0"),
                        help="directory holding train_shard_*.jsonl files")
    parser.add_argument("--output-dir", type=Path, default=None, help="where the updated shards go (default: in place)")
    parser.add_argument("--max-corpus", type=int, default=50_000, help="unique positives to index at most")
    parser.add_argument("--max-features", type=int, default=30_000, help="size of the n-gram vocabulary at most")
    parser.add_argument("--top-k", type=int, default=10, help="hits considered per query")
    parser.add_argument("--shard-range", type=str, default="all", help='"all", "0-10" or "5"')
    parser.add_argument("--batch-size", type=int, default=1000, help="queries per search call")
    parser.add_argument("--corpus-chunk-size", type=int, default=10_000, help="accepted and ignored")
    parser.add_argument("--dry-run", action="store_true", help="stats only, nothing is written")
    parser.add_argument("--device", type=str, default="cuda:0")
    return parser.parse_args(argv)


def main(argv: Optional[List[str]] = None) -> dict:
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s")
    if not args.data_dir.exists():
        raise FileNotFoundError(f"Data directory not found: {args.data_dir}")
    from snx.retrieval import TfidfIndex
    from src.train.mining.tfidf import collect_shard_files, mine_tfidf_negatives
    t0 = time.time()
    files = collect_shard_files(str(args.data_dir), args.shard_range)
    index = TfidfIndex(args.device, ngram_range=(2, 3), max_features=args.max_features, sublinear_tf=True)
    out = mine_tfidf_negatives(files, index, output_dir=None if args.output_dir is None else str(args.output_dir),
                               max_corpus=args.max_corpus, top_k=args.top_k, batch_size=args.batch_size,
                               dry_run=args.dry_run)
    summary = {k: out[k] for k in ("total", "already_had_negative", "added", "failed", "corpus")}
    summary["features"] = 0 if index.feature_keys is None else int(index.feature_keys.numel())
    summary["seconds"] = round(time.time() - t0, 3)
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()

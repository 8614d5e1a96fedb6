"""Teacher scores and dense hard negatives from cached teacher embeddings (src.train.mining.dense), on one GPU.

    python -m src.train.cli.teacher_scores score --embeddings cache/embeddings.npy --text-index cache/text_index.json \\
        --input-pattern "data/v29.0/train_*.jsonl" --output-dir data/v29.0_kd
    python -m src.train.cli.teacher_scores mine --embeddings cache/embeddings.npy --text-index cache/text_index.json \\
        --input-pattern "data/v29.0_kd/train_*.jsonl" --output-dir data/v30.0_multi_neg --k 7 --rank-start 10 --rank-end 50

``score`` is ref:scripts/precompute_teacher_scores.py without the encoder (the cache is its ``embeddings.npy`` /
``text_index.json``); ``mine`` is ref:scripts/mine_multi_negatives.py.  Flags shared with those scripts keep their names
and defaults.  Both run as a single process."""
from __future__ import annotations

import argparse
import logging
from typing import List, Optional

logger = logging.getLogger(__name__)


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Teacher scores / dense hard negatives from cached embeddings (GPU)")
    sub = ap.add_subparsers(dest="command", required=True)
    for name in ("score", "mine"):
        sp = sub.add_parser(name, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
        sp.add_argument("--embeddings", type=str, required=True, help="cached embeddings, .npy [n, D]")
        sp.add_argument("--text-index", type=str, required=True, help="JSON map md5(text)[:16] -> row")
        sp.add_argument("--input-pattern", type=str,
                        default="data/v29.0/train_*.jsonl" if name == "score" else "data/v29.0_kd/train_*.jsonl")
        sp.add_argument("--val-pattern", type=str, default="data/v29.0/val.jsonl" if name == "score" else
                        "data/v29.0_kd/val.jsonl")
        sp.add_argument("--output-dir", type=str, default="data/v29.0_kd" if name == "score" else "data/v30.0_multi_neg")
        sp.add_argument("--device", type=str, default="cuda:0")
        if name == "mine":
            sp.add_argument("--k", type=int, default=7, help="hard negatives per record")
            sp.add_argument("--rank-start", type=int, default=10)
            sp.add_argument("--rank-end", type=int, default=50)
            sp.add_argument("--sample", choices=("first", "random"), default="first")
            sp.add_argument("--seed", type=int, default=42)
            sp.add_argument("--chunk-docs", type=int, default=0)
    args = ap.parse_args(argv)
    if args.command == "mine" and (args.k < 1 or not 0 <= args.rank_start < args.rank_end <= 1024):
        ap.error("need --k >= 1 and 0 <= --rank-start < --rank-end <= 1024")
    return args


def main(argv: Optional[List[str]] = None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s")
    import torch
    from snx.retrieval import DenseIndex
    from src.train.mining import copy_val_files, expand_files
    from src.train.mining.dense import load_teacher_cache, mine_dense_negatives, write_teacher_scores
    files = expand_files([args.input_pattern])
    if not files:
        raise FileNotFoundError(f"no input files match {args.input_pattern!r}")
    embeddings, text_to_idx = load_teacher_cache(args.embeddings, args.text_index)
    index = DenseIndex(int(embeddings.shape[1]), torch.device(args.device))
    if args.command == "score":
        out = write_teacher_scores(files, args.output_dir, embeddings, text_to_idx, index)
        logger.info(f"scored {out} record(s) of {len(files)} file(s) into {args.output_dir}")
    else:
        out = mine_dense_negatives(files, args.output_dir, embeddings, text_to_idx, index, k=args.k,
                                   rank_start=args.rank_start, rank_end=args.rank_end, sample=args.sample,
                                   seed=args.seed, chunk_docs=args.chunk_docs)
    copy_val_files([args.val_pattern], args.output_dir)
    return out


if __name__ == "__main__":
    main()

"""Self-mining of hard negatives with a trained checkpoint (src.train.mining).

    torchrun --nproc_per_node=8 -m src.train.cli.mine_negatives --checkpoint outputs/train_v33/final_model \\
        --input-pattern "data/v29.0_kd/train_*.jsonl" --output-dir data/v33_self_neg --k 7

Flags shared with ref:scripts/mine_multi_negatives.py keep its names and defaults (--input-pattern, --val-pattern,
--output-dir, --k, --rank-start, --rank-end).  The output feeds ``data.train_files`` with ``data.num_hard_negatives = k``.
Without torchrun it runs as one rank."""
from __future__ import annotations

import argparse
import logging
import os
from typing import List, Optional

import torch

logger = logging.getLogger(__name__)


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Mine hard negatives with the model's own sparse index (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--input-pattern", type=str, default="data/v29.0_kd/train_*.jsonl")
    ap.add_argument("--val-pattern", type=str, default="data/v29.0_kd/val.jsonl")
    ap.add_argument("--output-dir", type=str, default="data/v33_self_neg")
    ap.add_argument("--k", type=int, default=7, help="hard negatives per record")
    ap.add_argument("--rank-start", type=int, default=10)
    ap.add_argument("--rank-end", type=int, default=50)
    ap.add_argument("--checkpoint", type=str, default=None,
                    help="checkpoint directory holding model.pt, or a model.pt file (default: random init)")
    ap.add_argument("--model-name", type=str, default="skt/A.X-Encoder-base")
    ap.add_argument("--tokenizer", type=str, default=None, help="tokenizer dir or hash:<vocab> (default: --model-name)")
    ap.add_argument("--query-max-length", type=int, default=64)
    ap.add_argument("--doc-max-length", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--query-top-k", type=int, default=64)
    ap.add_argument("--max-score-ratio", type=float, default=None,
                    help="admit only docs scoring below ratio * the query's lowest positive score")
    ap.add_argument("--sample", choices=("first", "random"), default="first")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--teacher-scores", choices=("none", "self"), default="none")
    ap.add_argument("--chunk-docs", type=int, default=0)
    args = ap.parse_args(argv)
    if args.k < 1 or not 0 <= args.rank_start < args.rank_end <= 1024:
        ap.error("need --k >= 1 and 0 <= --rank-start < --rank-end <= 1024")
    if args.max_score_ratio is not None and not args.max_score_ratio > 0:
        ap.error("--max-score-ratio must be > 0")
    return args


def load_model(args: argparse.Namespace, device: torch.device):
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.core import ddp_trainer as T
    torch.manual_seed(args.seed)                             # a random init is the same on every rank
    model = SPLADEModernBERT(model_name=args.model_name)
    if args.checkpoint:
        if os.path.isdir(args.checkpoint):
            T.load_checkpoint(model, None, None, args.checkpoint)
        else:
            model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    return model.to(device).eval()


def main(argv: Optional[List[str]] = None) -> dict:
    args = parse_args(argv)
    for key, val in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"),
                     ("MASTER_PORT", "29571")):
        os.environ.setdefault(key, val)                      # plain `python -m`: one rank
    from src.train.core import ddp_trainer as T
    from src.train.data.collator import create_tokenizer
    from src.train.mining import expand_files, mine_negatives
    local_rank = T.setup_distributed()
    logging.basicConfig(level=logging.INFO if T.is_main_process() else logging.WARNING,
                        format="%(asctime)s [%(levelname)s] %(message)s")
    try:
        device = torch.device(f"cuda:{local_rank}")
        files = expand_files([args.input_pattern])
        if not files:
            raise FileNotFoundError(f"no input files match {args.input_pattern!r}")
        tokenizer = create_tokenizer(args.tokenizer or args.model_name)
        model = load_model(args, device)
        summary = mine_negatives(model, tokenizer, files, args.output_dir, k=args.k, rank_start=args.rank_start,
                                 rank_end=args.rank_end, query_max_length=args.query_max_length,
                                 doc_max_length=args.doc_max_length, batch_size=args.batch_size,
                                 query_top_k=args.query_top_k, max_score_ratio=args.max_score_ratio,
                                 sample=args.sample, seed=args.seed, teacher_scores=args.teacher_scores,
                                 chunk_docs=args.chunk_docs, val_patterns=[args.val_pattern], device=device)
        if T.is_main_process():
            logger.info(f"wrote {len(files)} file(s) to {args.output_dir}")
        return summary
    finally:
        T.cleanup_distributed()


if __name__ == "__main__":
    main()

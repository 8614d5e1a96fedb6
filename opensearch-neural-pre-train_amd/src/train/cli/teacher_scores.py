"""Teacher embeddings, teacher scores and dense hard negatives (snx.teacher, src.train.mining.dense), on one GPU.

    python -m src.train.cli.teacher_scores encode --model-dir /models/bge-m3 --input-pattern "data/v29.0/train_*.jsonl" \\
        --output-dir cache [--max-length 256] [--batch-tokens 16384] [--precision bf16|fp32] [--num-shards n --shard-index i] \\
        [--tokenizer gpu:TOKENIZER_DIR|unigram:TOKENIZER_DIR]
    python -m src.train.cli.teacher_scores encode --merge --output-dir cache        # after a sharded run
    python -m src.train.cli.teacher_scores score --embeddings cache/embeddings.npy --text-index cache/text_index.json \\
        --input-pattern "data/v29.0/train_*.jsonl" --output-dir data/v29.0_kd
    python -m src.train.cli.teacher_scores mine --embeddings cache/embeddings.npy --text-index cache/text_index.json \\
        --input-pattern "data/v29.0_kd/train_*.jsonl" --output-dir data/v30.0_multi_neg --k 7 --rank-start 10 --rank-end 50 \\
        [--index flat|flat2|ivf|graph --expansion 4 --no-exact --nlist 100 --nprobe 1 --degree 32 --ef 0]

``encode`` is the encoder of ref:scripts/precompute_teacher_scores.py:49-159 (unique texts in first-occurrence order, BGE-M3
dense embeddings, L2-normalised) on the native XLM-RoBERTa forward; it writes ``embeddings.npy`` / ``text_index.json``.  A
sharded run (one process per GPU, ``--num-shards n --shard-index i``) writes ``embeddings.part{i}.npy`` and ``--merge`` joins
them.  ``score`` is the rest of that script (it reads the cache); ``mine`` is ref:scripts/mine_multi_negatives.py.  Flags
shared with those scripts keep their names and defaults.  ``mine --index ivf`` searches an ``snx.retrieval.IvfFlatIndex``
(``--nlist`` lists trained on the corpus rows, ``--nprobe`` of them read per query) instead of every doc; ``--nprobe`` equal
to the list count writes the files of ``--index flat``.  ``mine --index graph`` searches an ``snx.retrieval.GraphIndex``
(``--degree`` links per doc, a beam of ``--ef`` entries, 0: max(100, --rank-end)); an ``--ef`` of at least the doc count
writes the files of ``--index flat``.  ``mine --index flat2`` is the exact search through a bf16 first pass
(``DenseIndex.search_band_two_phase``: ``--expansion`` times the band's depth in candidates per query, an exact rescore, and
the exact search for every query the first pass could not certify): it writes the files of ``--index flat`` byte for byte
and adds ``certified_fraction`` to the stats; ``--no-exact`` keeps the uncertified rows as the first pass left them.  Every
subcommand runs as a single process."""
from __future__ import annotations

import argparse
import json
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
            sp.add_argument("--index", choices=("flat", "flat2", "ivf", "graph"), default="flat",
                            help="exact search, the same through a bf16 first pass, IVF-Flat, or the graph index")
            sp.add_argument("--expansion", type=float, default=4.0, help="flat2: candidates per wanted rank")
            sp.add_argument("--no-exact", action="store_true",
                            help="flat2: keep the rows the first pass could not certify instead of searching them exactly")
            sp.add_argument("--nlist", type=int, default=100, help="IVF lists (clamped to the doc count)")
            sp.add_argument("--nprobe", type=int, default=1, help="IVF lists read per query")
            sp.add_argument("--degree", type=int, default=32, help="graph: links per doc (even)")
            sp.add_argument("--ef", type=int, default=0, help="graph: beam entries (0: max(100, --rank-end))")
    sp = sub.add_parser("encode", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sp.add_argument("--model-dir", type=str, default=None, help="local HF directory of the teacher (never a model name)")
    sp.add_argument("--input-pattern", type=str, default="data/v29.0/train_*.jsonl")
    sp.add_argument("--output-dir", type=str, required=True, help="cache directory")
    sp.add_argument("--max-length", type=int, default=256)
    sp.add_argument("--batch-tokens", type=int, default=16384, help="token rows per forward")
    sp.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    sp.add_argument("--num-shards", type=int, default=1)
    sp.add_argument("--shard-index", type=int, default=0)
    sp.add_argument("--merge", action="store_true", help="join the parts of a sharded run into embeddings.npy")
    sp.add_argument("--tokenizer", type=str, default=None,
                    help="gpu:DIR: the native Unigram tokenizer of DIR/tokenizer.json on the GPU, its token ids go to the "
                         "forward without leaving the device; unigram:DIR: the same ids from plain Python; default: the "
                         "Hugging Face tokenizer stored in --model-dir")
    sp.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args(argv)
    if args.command == "encode":
        if not args.merge and not args.model_dir:
            ap.error("encode needs --model-dir (or --merge)")
        if args.num_shards < 1 or not 0 <= args.shard_index < args.num_shards or args.max_length < 1 or args.batch_tokens < 1:
            ap.error("need --num-shards >= 1, 0 <= --shard-index < --num-shards, --max-length >= 1, --batch-tokens >= 1")
        if args.tokenizer is not None and not args.tokenizer.startswith(("gpu:", "unigram:")):
            ap.error("--tokenizer must be gpu:DIR or unigram:DIR")
    if args.command == "mine" and (args.k < 1 or not 0 <= args.rank_start < args.rank_end <= 1024):
        ap.error("need --k >= 1 and 0 <= --rank-start < --rank-end <= 1024")
    if args.command == "mine" and not 1.0 <= args.expansion < float("inf"):
        ap.error("need a finite --expansion >= 1")
    if args.command == "mine" and not 1 <= args.nprobe <= args.nlist:
        ap.error("need 1 <= --nprobe <= --nlist")
    if args.command == "mine" and (not (args.ef == 0 or args.rank_end <= args.ef <= 1024) or not 2 <= args.degree <= 64
                                   or args.degree % 2):
        ap.error("need --ef 0 or --rank-end <= --ef <= 1024, and an even --degree in [2, 64]")
    return args


def encode_main(args: argparse.Namespace, tokenizer=None):
    """``encode``: (unique texts, rows written), or the merged rows for ``--merge``.  ``tokenizer``: an HF tokenizer to use
    instead of the one stored in ``--model-dir`` (it goes before ``--tokenizer``)."""
    from src.train.mining import expand_files
    from src.train.mining.dense import merge_teacher_cache, write_teacher_cache
    if args.merge:
        n = merge_teacher_cache(args.output_dir)
        logger.info(f"merged {n} row(s) into {args.output_dir}/embeddings.npy")
        return n
    files = expand_files([args.input_pattern])
    if not files:
        raise FileNotFoundError(f"no input files match {args.input_pattern!r}")
    from src.model.teachers import BGEM3Teacher
    if tokenizer is None and args.tokenizer:
        tokenizer = args.tokenizer                               # gpu:DIR | unigram:DIR, resolved on the teacher's device
    teacher = BGEM3Teacher(args.model_dir, device=args.device, max_length=args.max_length, normalize_embeddings=True,
                           tokenizer=tokenizer, precision=args.precision, batch_tokens=args.batch_tokens)
    out = write_teacher_cache(files, args.output_dir, teacher.encode, teacher.model.config.hidden_size,
                              num_shards=args.num_shards, shard_index=args.shard_index)
    logger.info(f"encoded {out[1]} of {out[0]} unique text(s) of {len(files)} file(s) into {args.output_dir}")
    return out


def main(argv: Optional[List[str]] = None, tokenizer=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s")
    if args.command == "encode":
        return encode_main(args, tokenizer)
    import torch
    from snx.retrieval import DenseIndex, GraphIndex, IvfFlatIndex
    from src.train.mining import copy_val_files, expand_files
    from src.train.mining.dense import load_teacher_cache, mine_dense_negatives, write_teacher_scores
    files = expand_files([args.input_pattern])
    if not files:
        raise FileNotFoundError(f"no input files match {args.input_pattern!r}")
    embeddings, text_to_idx = load_teacher_cache(args.embeddings, args.text_index)
    if args.command == "mine" and args.index == "ivf":
        index = IvfFlatIndex(int(embeddings.shape[1]), args.nlist, torch.device(args.device), nprobe=args.nprobe)
    elif args.command == "mine" and args.index == "graph":
        index = GraphIndex(int(embeddings.shape[1]), torch.device(args.device), degree=args.degree, knn=2 * args.degree,
                           ef=args.ef or max(100, args.rank_end))
    else:
        index = DenseIndex(int(embeddings.shape[1]), torch.device(args.device))
    if args.command == "score":
        out = write_teacher_scores(files, args.output_dir, embeddings, text_to_idx, index)
        logger.info(f"scored {out} record(s) of {len(files)} file(s) into {args.output_dir}")
    else:
        out = mine_dense_negatives(files, args.output_dir, embeddings, text_to_idx, index, k=args.k,
                                   rank_start=args.rank_start, rank_end=args.rank_end, sample=args.sample,
                                   seed=args.seed, chunk_docs=args.chunk_docs,
                                   **({"two_phase": (args.expansion, not args.no_exact)} if args.index == "flat2" else {}))
        if args.index == "flat2":
            logger.info("mine stats: " + json.dumps(out))
    copy_val_files([args.val_pattern], args.output_dir)
    return out


if __name__ == "__main__":
    main()

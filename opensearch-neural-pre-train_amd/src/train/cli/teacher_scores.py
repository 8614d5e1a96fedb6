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
    python -m src.train.cli.teacher_scores score-mv --model-dir /models/bge-m3 --input-pattern "data/v29.0/train_*.jsonl" \\
        --output-dir data/v29.0_kd_mv [--mode colbert|dense+colbert|sparse|dense+sparse|sparse+colbert|dense+sparse+colbert] \\
        [--dense-weight 1 --sparse-weight 1 --colbert-weight 1] [--max-length 256] \\
        [--batch-tokens 16384] [--chunk-records 256] [--precision bf16|fp32] [--tokenizer gpu:DIR|unigram:DIR]
    python -m src.train.cli.teacher_scores mine-mv --model-dir /models/bge-m3 --input-pattern "data/v29.0_kd/train_*.jsonl" \\
        --output-dir data/v30.0_mv_neg [--k 7 --rank-start 10 --rank-end 50 --max-length 256 --precision bf16] \\
        [--index exact|centroid|fde --ncentroids 1024 --ncand 0 --nbits 0 --nprobe 0 --k-sim 4 --reps 16 --d-proj 16]

``mine-mv`` mines hard negatives under the multi-vector teacher (src.train.mining.multivector.mine_multivector_negatives): the
unique positives of the shards are encoded into an ``snx.retrieval.MultiVectorIndex`` (csrc/mv_search.hip), every query is
searched exactly under MaxSim, and ranks [--rank-start, --rank-end) of its non-positives become the record's negatives.  It
prints one JSON line of counts, the store's rows and bytes among them.
``score-mv`` writes ``score``'s fields from BGE-M3's multi-vector (MaxSim) scores, computed straight behind the forward
chunk by chunk (src.train.mining.multivector, csrc/maxsim.hip); it needs ``colbert_linear.pt`` in ``--model-dir`` and keeps
no cache.  A ``--mode`` with ``sparse`` adds BGE-M3's lexical matching score of the same forward (csrc/teacher_lex.hip) and
needs ``sparse_linear.pt``; ``sparse`` and ``dense+sparse`` need no ``colbert_linear.pt``.  ``encode`` is the encoder of ref:scripts/precompute_teacher_scores.py:49-159 (unique texts in first-occurrence order, BGE-M3
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
    sp = sub.add_parser("score-mv", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sp.add_argument("--model-dir", type=str, required=True,
                    help="local HF directory of the teacher, with colbert_linear.pt (never a model name)")
    sp.add_argument("--input-pattern", type=str, default="data/v29.0/train_*.jsonl")
    sp.add_argument("--val-pattern", type=str, default="data/v29.0/val.jsonl")
    sp.add_argument("--output-dir", type=str, default="data/v29.0_kd_mv")
    sp.add_argument("--max-length", type=int, default=256)
    sp.add_argument("--batch-tokens", type=int, default=16384, help="token rows per forward")
    sp.add_argument("--chunk-records", type=int, default=256, help="records per forward-and-score round")
    sp.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    sp.add_argument("--tokenizer", type=str, default=None, help="gpu:DIR or unigram:DIR, as for encode")
    sp.add_argument("--mode", choices=("colbert", "dense+colbert", "sparse", "dense+sparse", "sparse+colbert",
                                       "dense+sparse+colbert"), default="colbert")
    sp.add_argument("--dense-weight", type=float, default=1.0)
    sp.add_argument("--sparse-weight", type=float, default=1.0)
    sp.add_argument("--colbert-weight", type=float, default=1.0)
    sp.add_argument("--device", type=str, default="cuda:0")
    sp = sub.add_parser("mine-mv", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sp.add_argument("--model-dir", type=str, required=True,
                    help="local HF directory of the teacher, with colbert_linear.pt (never a model name)")
    sp.add_argument("--input-pattern", type=str, default="data/v29.0_kd/train_*.jsonl")
    sp.add_argument("--val-pattern", type=str, default="data/v29.0_kd/val.jsonl")
    sp.add_argument("--output-dir", type=str, default="data/v30.0_mv_neg")
    sp.add_argument("--k", type=int, default=7, help="hard negatives per record")
    sp.add_argument("--rank-start", type=int, default=10)
    sp.add_argument("--rank-end", type=int, default=50)
    sp.add_argument("--max-length", type=int, default=256)
    sp.add_argument("--batch-tokens", type=int, default=16384, help="token rows per forward")
    sp.add_argument("--chunk-texts", type=int, default=256, help="texts per encoder call")
    sp.add_argument("--chunk-docs", type=int, default=0)
    sp.add_argument("--index", choices=("exact", "centroid", "fde", "token"), default="exact",
                    help="centroid: candidates from the centroid-interaction pass (csrc/mv_centroid.hip), scored exactly; "
                         "fde: from a dense search over fixed-dimensional encodings (csrc/mv_fde.hip), no centroids; "
                         "token: token retrieval over the compressed store (needs --nbits and --nprobe, takes no --ncand)")
    sp.add_argument("--k-sim", type=int, default=4, help="--index fde: sign bits per repetition, 0 .. 6")
    sp.add_argument("--reps", type=int, default=16, help="--index fde: repetitions, 1 .. 32")
    sp.add_argument("--d-proj", type=int, choices=(16, 32, 64), default=16, help="--index fde: projected width")
    sp.add_argument("--ncentroids", type=int, default=1024, help="--index centroid: centroids trained over the store's rows")
    sp.add_argument("--ncand", type=int, default=0,
                    help="--index centroid: candidates per query (0: max(4 * rank_end, 128), capped at 1024)")
    sp.add_argument("--nbits", type=int, choices=(0, 1, 2, 4), default=0,
                    help="--index centroid, bf16: residual-compress the store to this many bits per dimension and score "
                         "from the packed form (0: keep the bf16 rows)")
    sp.add_argument("--nprobe", type=int, default=0,
                    help="--index centroid: centroid lists a query row probes for candidates, 1 .. 64 (0: every document "
                         "is walked)")
    sp.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    sp.add_argument("--tokenizer", type=str, default=None, help="gpu:DIR or unigram:DIR, as for encode")
    sp.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args(argv)
    if args.command == "mine-mv":
        if args.nbits and (args.index not in ("centroid", "token") or args.precision != "bf16"):
            ap.error("--nbits needs --index centroid or token and --precision bf16")
        if not 0 <= args.nprobe <= 64 or (args.nprobe and args.index not in ("centroid", "token")):
            ap.error("need --nprobe 0, or 1 .. 64 with --index centroid or token")
        if args.index == "token" and (not args.nbits or not args.nprobe or args.ncand):
            ap.error("--index token needs --nbits 1, 2 or 4 and --nprobe 1 .. 64, and takes no --ncand")
        if args.index == "fde" and (not 0 <= args.k_sim <= 6 or not 1 <= args.reps <= 32 or
                                    args.reps * (1 << args.k_sim) * args.d_proj > 4096 or args.precision != "bf16"):
            ap.error("--index fde needs --precision bf16, 0 <= --k-sim <= 6, 1 <= --reps <= 32 and "
                     "reps * 2^k_sim * d_proj <= 4096")
        if args.k < 1 or not 0 <= args.rank_start < args.rank_end <= 1024:
            ap.error("need --k >= 1 and 0 <= --rank-start < --rank-end <= 1024")
        if not 1 <= args.ncentroids <= 4096 or not (args.ncand == 0 or args.rank_end <= args.ncand <= 1024):
            ap.error("need 1 <= --ncentroids <= 4096 and --ncand 0 or --rank-end <= --ncand <= 1024")
        if args.max_length < 2 or args.batch_tokens < 1 or args.chunk_texts < 1:
            ap.error("need --max-length >= 2, --batch-tokens >= 1, --chunk-texts >= 1")
        if args.tokenizer is not None and not args.tokenizer.startswith(("gpu:", "unigram:")):
            ap.error("--tokenizer must be gpu:DIR or unigram:DIR")
    if args.command == "score-mv":
        if args.max_length < 2 or args.batch_tokens < 1 or args.chunk_records < 1:
            ap.error("need --max-length >= 2, --batch-tokens >= 1, --chunk-records >= 1")
        if args.dense_weight < 0 or args.colbert_weight < 0 or args.dense_weight + args.colbert_weight <= 0:
            ap.error("need non-negative --dense-weight and --colbert-weight, not both zero")
        used = [getattr(args, f"{m}_weight") for m in args.mode.split("+")]
        if args.sparse_weight < 0 or sum(used) <= 0:
            ap.error("need a non-negative --sparse-weight, and a positive weight among the modes of --mode")
        if args.tokenizer is not None and not args.tokenizer.startswith(("gpu:", "unigram:")):
            ap.error("--tokenizer must be gpu:DIR or unigram:DIR")
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


def score_mv_main(args: argparse.Namespace, tokenizer=None) -> int:
    """``score-mv``: MaxSim and lexical teacher scores straight from the encoder (src.train.mining.multivector); the
    records scored."""
    from src.model.teachers.bge_m3 import lexical_scores, maxsim_scores
    from src.model.teachers import BGEM3Teacher
    from src.train.mining import copy_val_files, expand_files
    from src.train.mining.multivector import write_multivector_scores
    files = expand_files([args.input_pattern])
    if not files:
        raise FileNotFoundError(f"no input files match {args.input_pattern!r}")
    teacher = BGEM3Teacher(args.model_dir, device=args.device, max_length=args.max_length, normalize_embeddings=True,
                           tokenizer=tokenizer if tokenizer is not None else args.tokenizer, precision=args.precision,
                           batch_tokens=args.batch_tokens)
    sparse = "sparse" in args.mode
    if "colbert" in args.mode and not teacher.model.has_multivector:
        raise FileNotFoundError(f"{args.model_dir} has no colbert_linear.pt: score-mv needs the multi-vector head")
    if sparse and not teacher.model.has_sparse:
        raise FileNotFoundError(f"{args.model_dir} has no sparse_linear.pt: score-mv --mode {args.mode} needs the sparse head")
    out = write_multivector_scores(files, args.output_dir, teacher.encode_m3 if sparse else teacher.encode_multivector,
                                   maxsim_scores, mode=args.mode,
                                   weights=(args.dense_weight, args.sparse_weight, args.colbert_weight),
                                   chunk_records=args.chunk_records, lex_scorer=lexical_scores)
    logger.info(f"scored {out} record(s) of {len(files)} file(s) into {args.output_dir} ({args.mode})")
    copy_val_files([args.val_pattern], args.output_dir)
    return out


def mine_mv_main(args: argparse.Namespace, tokenizer=None) -> dict:
    """``mine-mv``: hard negatives from the exact MaxSim search (src.train.mining.multivector); the counts, also printed
    as one JSON line."""
    from snx.retrieval import MultiVectorIndex
    from src.model.teachers import BGEM3Teacher
    from src.train.mining import copy_val_files, expand_files
    from src.train.mining.multivector import mine_multivector_negatives
    files = expand_files([args.input_pattern])
    if not files:
        raise FileNotFoundError(f"no input files match {args.input_pattern!r}")
    teacher = BGEM3Teacher(args.model_dir, device=args.device, max_length=args.max_length, normalize_embeddings=True,
                           tokenizer=tokenizer if tokenizer is not None else args.tokenizer, precision=args.precision,
                           batch_tokens=args.batch_tokens)
    if not teacher.model.has_multivector:
        raise FileNotFoundError(f"{args.model_dir} has no colbert_linear.pt: mine-mv needs the multi-vector head")
    index = MultiVectorIndex(teacher.model.config.hidden_size, args.device)
    out = mine_multivector_negatives(files, args.output_dir, teacher.encode_multivector, index, k=args.k,
                                     rank_start=args.rank_start, rank_end=args.rank_end, chunk_texts=args.chunk_texts,
                                     chunk_docs=args.chunk_docs, index_type=args.index, ncentroids=args.ncentroids,
                                     ncand=args.ncand, nbits=args.nbits, nprobe=args.nprobe,
                                     k_sim=args.k_sim, reps=args.reps, d_proj=args.d_proj)
    print(json.dumps(out))
    copy_val_files([args.val_pattern], args.output_dir)
    return out


def main(argv: Optional[List[str]] = None, tokenizer=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s")
    if args.command == "encode":
        return encode_main(args, tokenizer)
    if args.command == "score-mv":
        return score_mv_main(args, tokenizer)
    if args.command == "mine-mv":
        return mine_mv_main(args, tokenizer)
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

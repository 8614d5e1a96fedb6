"""MLM corpus preparation on one GPU (src.preprocessing.mlm_data; ref:scripts/prepare_korean_mlm_data.py).

    python -m src.train.cli.prepare_mlm_data --input "raw/wiki_*.jsonl" --max-docs 0 --input raw/mc4.jsonl \\
        --max-docs 500000 --output-dir data/mlm_korean --report data/mlm_korean/report.jsonl

From raw documents to the ``train.txt`` and ``val.txt`` that ``src.train.cli.pretrain_mlm`` reads.  Every ``--input`` is
one source, in the order given; a pattern's files are sorted.  A ``.jsonl`` file holds one JSON object per line with the
text in ``--text-field`` (a missing or non-string field is the empty document, as the reference's ``article.get("text",
"")``); any other file is one document as a whole.  ``--max-docs`` gives, in the order of the ``--input`` options, the
number of leading documents each source contributes (0 = all; the reference's ``--max-wiki`` and ``--max-mc4``); fewer
values than inputs leave the rest at 0.  The sources are files only: no dataset name is resolved and nothing is fetched.

One JSON line goes to stdout: documents, pieces, valid, unique, train, val, mean_length, mean_korean_ratio, seconds.
``--report`` writes one JSON line per input document: source, document, pieces, valid, kept.  Exit status 1 with a
message when no valid paragraph remains (ref:prepare_korean_mlm_data.py:344-346).  Runs as a single process."""
from __future__ import annotations

import argparse
import glob
import json
import sys
import time
from typing import Iterator, List, Optional


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Prepare line-delimited text for MLM pre-training (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--input", action="append", required=True, metavar="PATTERN",
                    help="a source: a file or a glob of .jsonl / .txt files; repeatable, order significant")
    ap.add_argument("--max-docs", action="append", type=int, default=None, metavar="N",
                    help="leading documents of the matching --input to use, 0 = all; repeatable")
    ap.add_argument("--text-field", type=str, default="text")
    ap.add_argument("--output-dir", type=str, default="data/mlm_korean")
    ap.add_argument("--min-length", type=int, default=50)
    ap.add_argument("--korean-ratio", type=float, default=0.3)
    ap.add_argument("--val-ratio", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batch-code-points", type=int, default=1 << 24)
    ap.add_argument("--report", type=str, default=None, help="write the per-document counts to this JSONL file")
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args(argv)
    args.max_docs = list(args.max_docs or [])
    if len(args.max_docs) > len(args.input):
        ap.error("more --max-docs than --input")
    if any(m < 0 for m in args.max_docs):
        ap.error("--max-docs must be >= 0")
    args.max_docs += [0] * (len(args.input) - len(args.max_docs))
    return args


def read_documents(pattern: str, text_field: str = "text", max_docs: int = 0) -> Iterator[str]:
    """The documents of one source: the files of ``pattern`` sorted, the first ``max_docs`` documents (0 = all)."""
    files = sorted(glob.glob(pattern))
    if not files:
        raise FileNotFoundError(f"no input files match {pattern!r}")
    n = 0
    for path in files:
        if path.endswith(".jsonl"):
            with open(path, encoding="utf-8") as f:
                for line in f:
                    if not line.strip():
                        continue
                    if max_docs and n >= max_docs:
                        return
                    rec = json.loads(line)
                    text = rec.get(text_field, "") if isinstance(rec, dict) else ""
                    yield text if isinstance(text, str) else ""
                    n += 1
        else:
            if max_docs and n >= max_docs:
                return
            with open(path, encoding="utf-8", newline="") as f:
                yield f.read()
            n += 1


def main(argv: Optional[List[str]] = None) -> dict:
    args = parse_args(argv)
    from src.preprocessing import mlm_data
    t0 = time.time()
    sources = [read_documents(p, args.text_field, m) for p, m in zip(args.input, args.max_docs)]
    corpus = mlm_data.prepare_mlm_corpus(sources, min_length=args.min_length, min_korean_ratio=args.korean_ratio,
                                         val_ratio=args.val_ratio, seed=args.seed,
                                         batch_code_points=args.batch_code_points, device=args.device,
                                         source_names=[f"--input {p}" for p in args.input])
    if args.report:
        with open(args.report, "w", encoding="utf-8") as f:
            for r in corpus.report:
                f.write(json.dumps(r) + "\n")
    if not corpus.unique:
        print("ERROR: No valid paragraphs collected. Exiting.", file=sys.stderr)
        sys.exit(1)
    mlm_data.write_corpus(corpus, args.output_dir)
    summary = {"documents": corpus.documents, "pieces": corpus.pieces, "valid": corpus.valid, "unique": corpus.unique,
               "train": len(corpus.train), "val": len(corpus.val), "mean_length": corpus.stats["mean_length"],
               "mean_korean_ratio": corpus.stats["mean_korean_ratio"], "seconds": round(time.time() - t0, 3)}
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()

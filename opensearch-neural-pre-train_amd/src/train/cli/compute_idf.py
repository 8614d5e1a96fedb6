"""Document frequencies and IDF weights of a JSONL corpus (the counterpart of ref:tools/idf-compute, its arguments and
its output format), counted on one GPU.

    python -m src.train.cli.compute_idf --input "data/v29.0/train_shard_*.jsonl" --output outputs/idf_weights/idf \\
        --tokenizer <dir | hash:VOCAB> [--smoothing bm25|standard|smooth] [--batch-docs 4096] [--idf-json idf.json]

Every non-empty ``query`` / ``positive`` / ``negative`` / ``text`` / ``document`` field of every record is one document
(ref:tools/idf-compute/src/main.rs:147-176); it is tokenised WITHOUT special tokens and without truncation.  Writes
``<output>.bin`` (little-endian f32 x vocab_size) and ``<output>.json`` (vocab_size, num_docs, smoothing, tokenizer_name,
dtype, byte_order) -- readable by ref:tools/idf-compute/load_idf.py -- and prints one JSON line: num_docs, vocab_size,
nonzero, min, max.  Tokenisation runs on the host and dominates the wall time; the GPU only counts
(snx.idf.doc_freq), so the Rust tool's speed-up over a Python loop is not claimed here."""
from __future__ import annotations

import argparse
import glob
import json
from typing import Iterator, List, Optional

FIELDS = ("query", "positive", "negative", "text", "document")      # main.rs:148-154, in that order
SMOOTHINGS = ("bm25", "standard", "smooth")


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="document frequencies and IDF weights of a JSONL corpus (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--input", "-i", type=str, default="data/v29.0/train_shard_*.jsonl", help="glob of JSONL files")
    ap.add_argument("--output", "-o", type=str, default="outputs/idf_weights/idf", help="output path without extension")
    ap.add_argument("--tokenizer", "-t", type=str, required=True, help="tokenizer directory or hash:<vocab>")
    ap.add_argument("--smoothing", "-s", type=str, default="bm25")
    ap.add_argument("--batch-docs", type=int, default=4096, help="documents per GPU batch")
    ap.add_argument("--idf-json", type=str, default=None, help="also write token -> weight (the idf.json a model ships)")
    ap.add_argument("--pt", action="store_true", help="also write <output>.pt")
    args = ap.parse_args(argv)
    if args.smoothing not in SMOOTHINGS:
        ap.error(f"--smoothing: one of {', '.join(SMOOTHINGS)}")
    if args.batch_docs < 1:
        ap.error("--batch-docs must be >= 1")
    args.files = sorted(glob.glob(args.input))
    if not args.files:
        ap.error(f"no files found matching: {args.input}")
    return args


def documents(files: List[str]) -> Iterator[str]:
    """Every non-empty text field of every record; unreadable lines are skipped, as the reference skips them."""
    for path in files:
        with open(path, encoding="utf-8", errors="replace") as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                try:
                    rec = json.loads(line)
                except ValueError:
                    continue
                if not isinstance(rec, dict):
                    continue
                for key in FIELDS:
                    text = rec.get(key)
                    if isinstance(text, str) and text:
                        yield text


def tokenizer_vocab_size(tokenizer) -> int:
    """With added tokens, as ``get_vocab_size(true)`` (main.rs:94)."""
    try:
        return int(len(tokenizer))
    except TypeError:
        return int(tokenizer.vocab_size)


def main(argv: Optional[List[str]] = None) -> dict:
    args = parse_args(argv)
    import numpy as np
    import torch
    from snx.idf import IdfTable
    from src.train.data.collator import create_tokenizer
    tokenizer = create_tokenizer(args.tokenizer)
    V = tokenizer_vocab_size(tokenizer)
    table = IdfTable(V, torch.device("cuda:0"), tokenizer_name=args.tokenizer)

    def flush(rows: List[List[int]]) -> None:
        S = max(1, max(len(r) for r in rows))
        ids = np.zeros((len(rows), S), dtype=np.int64)
        mask = np.zeros((len(rows), S), dtype=np.int64)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = r
            mask[i, :len(r)] = 1
        table.fit_tokens(torch.from_numpy(ids), torch.from_numpy(mask))

    rows: List[List[int]] = []
    for text in documents(args.files):
        rows.append(list(tokenizer.encode(text, add_special_tokens=False)))
        if len(rows) == args.batch_docs:
            flush(rows)
            rows = []
    if rows:
        flush(rows)
    w = table.idf(args.smoothing)
    table.save(args.output, args.smoothing)
    if args.pt:
        table.to_pt(args.output, args.smoothing)
    if args.idf_json:
        table.save_idf_json(args.idf_json, tokenizer, args.smoothing)
    line = dict(num_docs=int(table.num_docs), vocab_size=V, nonzero=int((w > 0).sum()), min=float(w.min()),
                max=float(w.max()))
    print(json.dumps(line), flush=True)
    return line


if __name__ == "__main__":
    main()

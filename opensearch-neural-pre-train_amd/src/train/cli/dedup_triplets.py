"""Near-duplicate removal of triplet shards by MinHash on one GPU (src.preprocessing.cleaners.MinHashDeduplicator).

    python -m src.train.cli.dedup_triplets --input-pattern "data/v30.0_multi_neg/train_*.jsonl" \\
        --output-dir data/v30.0_dedup --num-perm 128 --threshold 0.8 --ngram-size 3 --report data/v30.0_dedup/report.jsonl

The step between mining and training: the shards are read as the miners read them (``expand_files``, then the dataset of
``load_training_data``: sorted paths, blank lines skipped), all records form ONE sequence in that order, and the kept
records are written unchanged -- the line as it was read -- to a file of the same name in ``--output-dir``.  The rule is
the reference's MinHashDeduplicator (ref:src/preprocessing/cleaners/deduplicator.py:146-181) on the records' (query,
positive) pairs.  One JSON line goes to stdout: rows_in, rows_kept, exact_duplicates (dropped for the exact key of a kept
row), minhash_duplicates (dropped by signature alone), seconds.  ``--report`` writes one JSON line per input row: its
file, its line among the file's records, and ``duplicate_of`` as (file, line) of the kept row it repeats, null if kept.
Runs as a single process."""
from __future__ import annotations

import argparse
import glob
import json
import logging
import os
import time
from typing import List, Optional

logger = logging.getLogger(__name__)


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="MinHash near-duplicate removal of triplet shards (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--input-pattern", type=str, required=True)
    ap.add_argument("--output-dir", type=str, required=True)
    ap.add_argument("--num-perm", type=int, default=128)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--ngram-size", type=int, default=3)
    ap.add_argument("--report", type=str, default=None, help="write duplicate_of per input row to this JSONL file")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap.parse_args(argv)


def main(argv: Optional[List[str]] = None) -> dict:
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s")
    from src.preprocessing.cleaners.deduplicator import MinHashDeduplicator, exact_groups
    from src.train.data import load_training_data
    from src.train.mining import expand_files
    files = expand_files([args.input_pattern])
    if not files:
        raise FileNotFoundError(f"no input files match {args.input_pattern!r}")
    out_dir = os.path.abspath(args.output_dir)
    if any(os.path.dirname(os.path.abspath(f)) == out_dir for f in files):
        raise ValueError("--output-dir must not be the directory of the input shards")
    t0 = time.time()
    ds = load_training_data([glob.escape(f) for f in files])
    n = len(ds)
    pairs, raw = [], []
    handles = [open(f, "rb") for f in files]
    try:
        for i in range(n):
            rec = ds[i]
            pairs.append((rec["query"], rec["positive"]))
            fi, off = ds.index[i]
            handles[fi].seek(off)
            raw.append(handles[fi].readline())
    finally:
        for h in handles:
            h.close()
    dedup = MinHashDeduplicator(num_perm=args.num_perm, threshold=args.threshold, ngram_size=args.ngram_size)
    dedup.device = args.device
    dup = dedup.deduplicate_pairs(pairs)
    group = exact_groups(pairs)
    exact = sum(1 for i in range(n) if dup[i] >= 0 and group[dup[i]] == group[i])
    os.makedirs(out_dir, exist_ok=True)
    line_of = []                                             # per row: its line among its file's records
    seen = [0] * len(files)
    outs = [open(os.path.join(out_dir, os.path.basename(f)), "wb") for f in files]
    try:
        for i in range(n):
            fi = ds.index[i][0]
            line_of.append(seen[fi])
            seen[fi] += 1
            if dup[i] < 0:
                outs[fi].write(raw[i] if raw[i].endswith(b"\n") else raw[i] + b"\n")
    finally:
        for h in outs:
            h.close()
    if args.report:
        with open(args.report, "w", encoding="utf-8") as f:
            for i in range(n):
                d = int(dup[i])
                f.write(json.dumps({"row": i, "file": os.path.basename(files[ds.index[i][0]]), "line": line_of[i],
                                    "duplicate_of": None if d < 0 else
                                    {"row": d, "file": os.path.basename(files[ds.index[d][0]]), "line": line_of[d]}})
                        + "\n")
    kept = int((dup < 0).sum())
    summary = {"rows_in": n, "rows_kept": kept, "exact_duplicates": int(exact), "minhash_duplicates": n - kept - int(exact),
               "seconds": round(time.time() - t0, 3)}
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()

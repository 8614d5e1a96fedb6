"""Validate synonym / expansion pairs against a corpus by PMI on one GPU (src.pmi, snx.cooc).

    python -m src.train.cli.validate_synonyms --corpus corpus.txt --pairs pairs.json --output-dir out/pmi

``--corpus``: one document a line (a literal ``\\n\\n`` inside a line is not a paragraph break; paragraph mode is for
callers of src.pmi).  ``--pairs``: a JSON list of {"source", "target", "similarity", "category"}.  The co-occurrence
files, validated_pairs.jsonl, invalid_pairs.jsonl and validation_report.json go to ``--output-dir``.  One JSON line of
counts goes to stdout: documents, vocab_size, total_windows, nnz, total_pairs, valid_pairs, removed_pairs, oov_pairs,
thresholds, seconds."""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path
from typing import List, Optional


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="PMI validation of synonym pairs (GPU)",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--corpus", type=Path, required=True, help="text file, one document a line")
    parser.add_argument("--pairs", type=Path, required=True, help="JSON list of pairs")
    parser.add_argument("--output-dir", type=Path, required=True)
    parser.add_argument("--window-type", choices=("sentence", "paragraph", "sliding"), default="sentence")
    parser.add_argument("--window-size", type=int, default=10)
    parser.add_argument("--min-term-freq", type=int, default=5)
    parser.add_argument("--max-vocab-size", type=int, default=120000)
    parser.add_argument("--no-symmetric", action="store_true")
    parser.add_argument("--normalize", action="store_true")
    parser.add_argument("--laplace-smoothing", type=float, default=1.0)
    parser.add_argument("--context-smoothing-alpha", type=float, default=0.75)
    parser.add_argument("--no-ppmi", action="store_true")
    parser.add_argument("--log-base", type=float, default=2.0)
    parser.add_argument("--min-cooccurrence", type=int, default=1)
    parser.add_argument("--pmi-percentile-threshold", type=float, default=10.0)
    parser.add_argument("--pmi-absolute-threshold", type=float, default=None)
    parser.add_argument("--min-embedding-similarity", type=float, default=0.5)
    parser.add_argument("--oov-strategy", choices=("remove", "keep", "smooth"), default="keep")
    parser.add_argument("--no-separate-bpe", action="store_true")
    parser.add_argument("--device", type=str, default="cuda:0")
    return parser.parse_args(argv)


def configs_of(args: argparse.Namespace):
    """(CooccurrenceConfig, PMIConfig, ValidationConfig) of the command line."""
    from src.pmi import CooccurrenceConfig, OOVStrategy, PMIConfig, ValidationConfig, WindowType
    return (CooccurrenceConfig(window_type=WindowType(args.window_type), window_size=args.window_size,
                               min_term_freq=args.min_term_freq, max_vocab_size=args.max_vocab_size,
                               symmetric=not args.no_symmetric, normalize=args.normalize),
            PMIConfig(laplace_smoothing=args.laplace_smoothing, context_smoothing_alpha=args.context_smoothing_alpha,
                      use_ppmi=not args.no_ppmi, log_base=args.log_base, min_cooccurrence=args.min_cooccurrence),
            ValidationConfig(pmi_percentile_threshold=args.pmi_percentile_threshold,
                             pmi_absolute_threshold=args.pmi_absolute_threshold,
                             min_embedding_similarity=args.min_embedding_similarity,
                             oov_strategy=OOVStrategy(args.oov_strategy),
                             separate_bpe_validation=not args.no_separate_bpe))


def main(argv: Optional[List[str]] = None) -> dict:
    args = parse_args(argv)
    from src.pmi import SynonymValidator, create_pmi_pipeline
    cooc_config, pmi_config, validation_config = configs_of(args)
    t0 = time.time()
    with open(args.corpus, "r", encoding="utf-8") as f:
        documents = [line.rstrip("\n") for line in f]
    with open(args.pairs, "r", encoding="utf-8") as f:
        pairs = json.load(f)
    builder, calc = create_pmi_pipeline(documents, cooc_config=cooc_config, pmi_config=pmi_config,
                                        save_path=args.output_dir, show_progress=False, device=args.device)
    validator = SynonymValidator(calc, validation_config)
    validated, result = validator.validate(pairs, show_progress=False)
    validator.save_validation_report(validated, result, args.output_dir)
    stats = builder.get_stats()
    summary = {"documents": stats.total_documents, "vocab_size": stats.vocab_size, "total_windows": stats.total_windows,
               "nnz": stats.total_cooccurrences, "total_pairs": result.total_pairs, "valid_pairs": result.valid_pairs,
               "removed_pairs": result.removed_pairs, "oov_pairs": result.oov_pairs, "thresholds": validator.thresholds,
               "seconds": round(time.time() - t0, 3)}
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()

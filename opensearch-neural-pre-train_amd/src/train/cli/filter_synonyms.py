"""Filter synonym / expansion pairs by information gain in embedding space on one GPU (src.information_gain, snx.infogain).

    python -m src.train.cli.filter_synonyms --pairs pairs.json --embeddings E.npy --terms terms.json --output-dir out/ig

``--pairs``: the JSON list ``validate_synonyms`` takes, {"source", "target"[, "similarity", ...]}.  ``--embeddings``: an
fp32 array [n, D], one row per term of ``--terms`` (a JSON list of n strings); the encoder that made them stays outside.
The corpus of the entropy estimates is the whole array.  A pair with a term that ``--terms`` does not hold is reported as
skipped and is not scored.  ``ig_report.json`` goes to ``--output-dir``: the configuration, the threshold, one record per
scored pair with the fields of InformationGainResult, the skipped pairs, and analyze_ig_distribution.  One JSON line of
counts goes to stdout: terms, dim, total_pairs, scored_pairs, skipped_pairs, filtered_pairs, kept_pairs, method, threshold,
seconds."""
from __future__ import annotations

import argparse
import dataclasses
import json
import time
from pathlib import Path
from typing import List, Optional


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="Information-gain filtering of synonym pairs (GPU)",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--pairs", type=Path, required=True, help="JSON list of pairs")
    parser.add_argument("--embeddings", type=Path, required=True, help=".npy, fp32 [n, D]")
    parser.add_argument("--terms", type=Path, required=True, help="JSON list of the n terms, in row order")
    parser.add_argument("--output-dir", type=Path, required=True)
    parser.add_argument("--k-entropy", type=int, default=10)
    parser.add_argument("--k-neighborhood", type=int, default=50)
    parser.add_argument("--percentile-threshold", type=float, default=10.0)
    parser.add_argument("--min-ig-absolute", type=float, default=0.0)
    parser.add_argument("--method", choices=("percentile", "otsu", "mad"), default="percentile")
    parser.add_argument("--no-normalize", action="store_true")
    parser.add_argument("--batch-size", type=int, default=1000)
    return parser.parse_args(argv)


def main(argv: Optional[List[str]] = None) -> dict:
    args = parse_args(argv)
    import numpy as np
    from src.information_gain import (InformationGainConfig, analyze_ig_distribution, compute_adaptive_threshold,
                                      filter_synonym_pairs)
    t0 = time.time()
    emb = np.load(args.embeddings)
    with open(args.terms, "r", encoding="utf-8") as f:
        terms = json.load(f)
    with open(args.pairs, "r", encoding="utf-8") as f:
        pairs = json.load(f)
    if emb.ndim != 2 or len(terms) != emb.shape[0]:
        raise SystemExit(f"--embeddings {emb.shape} does not hold one row per term of --terms ({len(terms)})")
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    row = {t: i for i, t in enumerate(terms)}
    scored, skipped = [], []
    for p in pairs:
        missing = [p[side] for side in ("source", "target") if p[side] not in row]
        if missing:
            skipped.append({"source": p["source"], "target": p["target"], "missing": missing})
        else:
            scored.append((p["source"], p["target"], float(p.get("similarity", 0.0))))
    config = InformationGainConfig(k_entropy=args.k_entropy, k_neighborhood=args.k_neighborhood,
                                   percentile_threshold=args.percentile_threshold, min_ig_absolute=args.min_ig_absolute,
                                   batch_size=args.batch_size, normalize_embeddings=not args.no_normalize)
    results, threshold, distribution = [], None, {}
    if scored:
        src = emb[[row[s] for s, _, _ in scored]]
        tgt = emb[[row[t] for _, t, _ in scored]]
        results = filter_synonym_pairs(scored, src, tgt, emb, config, method=args.method)
        ig = np.array([r.information_gain for r in results], dtype=np.float32)
        threshold = compute_adaptive_threshold(ig, method=args.method, percentile=args.percentile_threshold)
        distribution = analyze_ig_distribution(results)
    args.output_dir.mkdir(parents=True, exist_ok=True)
    with open(args.output_dir / "ig_report.json", "w", encoding="utf-8") as f:
        json.dump({"config": dataclasses.asdict(config), "method": args.method, "threshold": threshold,
                   "results": [dataclasses.asdict(r) for r in results], "skipped": skipped,
                   "distribution": distribution}, f, ensure_ascii=False, indent=1)
        f.write("\n")
    summary = {"terms": len(terms), "dim": int(emb.shape[1]), "total_pairs": len(pairs), "scored_pairs": len(results),
               "skipped_pairs": len(skipped), "filtered_pairs": sum(r.is_filtered for r in results),
               "kept_pairs": sum(not r.is_filtered for r in results), "method": args.method, "threshold": threshold,
               "seconds": round(time.time() - t0, 3)}
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()

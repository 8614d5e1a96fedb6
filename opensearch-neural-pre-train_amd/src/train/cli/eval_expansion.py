"""Graded term-expansion evaluation of a checkpoint on one GPU (src.evaluation, snx.expansion): Recall@K, MRR and nDCG@K
of each source term's judged synonyms in the model's own ranking of the vocabulary.

    python -m src.train.cli.eval_expansion --checkpoint CKPT_DIR (--eval-set FILE.json | --synonym-pairs FILE.json | --sample)
        [--k-values 5,10,20,50,100] [--batch-size 32] [--domain D] [--compare CKPT_B] [--report OUT.json]

``--eval-set``: a file written by ``EvaluationDataset.save``.  ``--synonym-pairs``: the JSON list
``EvaluationDataset.from_synonym_pairs`` takes, {"source", "synonyms": {"exact", "partial", "related"}, "domain"?}.
``--sample``: the sample dataset of the Korean legal, medical and general domains.  ``--domain`` keeps the queries of one
domain.  One JSON line per checkpoint goes to stdout: ``EvaluationResult.to_dict()`` without the per-query list, plus
``checkpoint``; with ``--compare`` one more line holds ``ModelComparison.metrics_compared`` of the two.  ``--report``
receives everything, per-query lists included."""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import List, Optional

K_VALUES = "5,10,20,50,100"


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="graded term-expansion evaluation of a checkpoint (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--checkpoint", type=str, default=None,
                    help="checkpoint directory holding model.pt, or a model.pt file (default: random init)")
    ap.add_argument("--model-name", type=str, default="skt/A.X-Encoder-base")
    ap.add_argument("--tokenizer", type=str, default=None, help="tokenizer dir or hash:<vocab> (default: --model-name)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--eval-set", type=Path, default=None, help="EvaluationDataset.save output")
    src.add_argument("--synonym-pairs", type=Path, default=None, help="JSON list for from_synonym_pairs")
    src.add_argument("--sample", action="store_true", help="the sample legal / medical / general dataset")
    ap.add_argument("--k-values", type=str, default=K_VALUES)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--domain", type=str, default=None)
    ap.add_argument("--compare", type=str, default=None, help="a second checkpoint, compared on the same queries")
    ap.add_argument("--report", type=Path, default=None)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args(argv)
    try:
        args.k_values = [int(k) for k in args.k_values.split(",") if k]
    except ValueError:
        ap.error("--k-values: comma-separated integers")
    if not args.k_values or min(args.k_values) < 1:
        ap.error("--k-values: at least one cutoff, each >= 1")
    if args.batch_size < 1:
        ap.error("--batch-size must be >= 1")
    return args


def _plain(x):
    """numpy scalars and the integer keys of the result dicts -> what json.dumps takes; inf stays a float."""
    import numpy as np
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


def load_dataset(args: argparse.Namespace):
    from src.evaluation import EvaluationDataset, create_korean_legal_medical_eval_dataset
    if args.sample:
        data = create_korean_legal_medical_eval_dataset()
    elif args.eval_set is not None:
        data = EvaluationDataset.load(args.eval_set)
    else:
        with open(args.synonym_pairs, "r", encoding="utf-8") as f:
            data = EvaluationDataset.from_synonym_pairs(json.load(f), name=args.synonym_pairs.stem)
    return data.filter_by_domain(args.domain) if args.domain else data


def main(argv: Optional[List[str]] = None) -> List[dict]:
    args = parse_args(argv)
    import torch
    from src.evaluation import ModelComparison, RankingMetrics
    from src.train.cli.mine_negatives import load_model
    from src.train.data.collator import create_tokenizer
    device = torch.device("cuda:0")
    data = load_dataset(args)
    if len(data) == 0:
        raise ValueError("no queries to evaluate")
    tokenizer = create_tokenizer(args.tokenizer or args.model_name)
    metrics = RankingMetrics(tokenizer, k_values=args.k_values)
    lines, results = [], []
    for ckpt in [args.checkpoint] + ([args.compare] if args.compare else []):
        one = argparse.Namespace(**{**vars(args), "checkpoint": ckpt})
        res = metrics.evaluate(load_model(one, device), data, batch_size=args.batch_size, device=device)
        results.append(res)
        d = _plain(res.to_dict())
        d.pop("per_query_metrics")
        lines.append({"checkpoint": ckpt, "dataset": data.name, **d})
    if args.compare:
        cmp_ = ModelComparison.compare_models(results[0], results[1], str(args.checkpoint), str(args.compare))
        lines.append({"comparison": [str(args.checkpoint), str(args.compare)],
                      "metrics_compared": _plain(cmp_.metrics_compared)})
    for line in lines:
        print(json.dumps(line, ensure_ascii=False), flush=True)
    if args.report is not None:
        with open(args.report, "w", encoding="utf-8") as f:
            json.dump({"dataset": data.name, "k_values": args.k_values, "lines": lines,
                       "per_query_metrics": [_plain(r.per_query_metrics) for r in results]}, f, ensure_ascii=False, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()

"""Pruning and two-phase search of a checkpoint against exact retrieval, offline (snx.retrieval.SparseIndex.pruned /
search_two_phase).

    python -m src.train.cli.eval_pruning --checkpoint outputs/train_v33/final_model --val-file data/val.jsonl [--sweep]

The reference serves its ``rank_features`` index through OpenSearch's neural_sparse_two_phase_processor with one
setting (ref:benchmark/index_manager.py:197-238: prune_ratio 0.4, expansion_rate 5, max_window_size 10000) and
publishes no sweep for it; without ``--sweep`` that one setting runs.  The grid of ``--sweep`` is this project's own:
prune_ratio in {0.1, 0.2, 0.4, 0.6, 0.8} at expansion_rate 5, expansion_rate in {1, 2, 5, 10, 20} at ratio 0.4, then
ingest-time pruning of the doc vectors -- max_ratio {0.05, 0.1, 0.2}, top_k {32, 64, 128}, alpha_mass {0.8, 0.9, 0.95}
-- under exact search (a query prune that keeps everything).  The evaluator's corpus is encoded once and the exact index
is the baseline.  One JSON line per setting: the parameters, the exact metrics, the two_phase_* metrics, overlap@5, the
counters' means and search_s (ingest settings add doc_postings_frac).  One process (not torchrun)."""
from __future__ import annotations

import argparse
import json
from typing import List, Optional, Tuple

DEFAULT = ("max_ratio", 0.4, 5.0)      # query prune type, value, expansion_rate: ref:benchmark/index_manager.py:197-238
MAX_WINDOW = 10000
EXACT = ("max_ratio", 0.0, 1.0)        # keeps every query entry: the two-phase result is the exact search's


def sweep() -> List[Tuple[tuple, Optional[tuple]]]:
    """[((query prune type, value, expansion_rate), doc prune (type, value) | None)] in run order."""
    t, r, e = DEFAULT
    grid = [((t, x, e), None) for x in (0.1, 0.2, 0.4, 0.6, 0.8)] + [((t, r, x), None) for x in (1.0, 2.0, 5.0, 10.0, 20.0)]
    for dt, values in (("max_ratio", (0.05, 0.1, 0.2)), ("top_k", (32, 64, 128)), ("alpha_mass", (0.8, 0.9, 0.95))):
        grid += [(EXACT, (dt, v)) for v in values]
    return grid


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="pruning and two-phase search against exact sparse retrieval (GPU)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--checkpoint", type=str, default=None,
                    help="checkpoint directory holding model.pt, or a model.pt file (default: random init)")
    ap.add_argument("--model-name", type=str, default="skt/A.X-Encoder-base")
    ap.add_argument("--tokenizer", type=str, default=None, help="tokenizer dir or hash:<vocab> (default: --model-name)")
    ap.add_argument("--val-file", type=str, default="data/v29.0_kd/val.jsonl")
    ap.add_argument("--max-queries", type=int, default=2000)
    ap.add_argument("--max-docs", type=int, default=50000)
    ap.add_argument("--query-max-length", type=int, default=64)
    ap.add_argument("--doc-max-length", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--prune-ratio", type=float, default=DEFAULT[1], help="max_ratio of the query prune")
    ap.add_argument("--expansion-rate", type=float, default=DEFAULT[2])
    ap.add_argument("--max-window-size", type=int, default=MAX_WINDOW)
    ap.add_argument("--sweep", action="store_true", help="this project's 19-setting grid instead of the one setting")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON lines to this file")
    args = ap.parse_args(argv)
    if not 0 <= args.prune_ratio <= 1:
        ap.error("--prune-ratio must lie in [0, 1]")
    if not args.expansion_rate > 0 or args.max_window_size < 1:
        ap.error("--expansion-rate must be > 0 and --max-window-size >= 1")
    return args


def settings(args: argparse.Namespace) -> List[Tuple[tuple, Optional[tuple]]]:
    if args.sweep:
        return sweep()
    return [((DEFAULT[0], args.prune_ratio, args.expansion_rate), None)]


def main(argv: Optional[List[str]] = None) -> List[dict]:
    args = parse_args(argv)
    import torch
    from src.train.cli.mine_negatives import load_model
    from src.train.data.collator import create_tokenizer
    from src.train.eval import RETRIEVAL_SIZE, MidTrainingEvaluator, metrics_from_ranks, two_phase_eval
    device = torch.device("cuda:0")
    tokenizer = create_tokenizer(args.tokenizer or args.model_name)
    model = load_model(args, device)
    ev = MidTrainingEvaluator(tokenizer, args.val_file, max_queries=args.max_queries, max_docs=args.max_docs,
                              device=str(device), query_max_length=args.query_max_length,
                              doc_max_length=args.doc_max_length, batch_size=args.batch_size)
    index, queries = ev.encode(model)
    if queries is None:
        raise ValueError(f"{args.val_file}: no queries or no docs to evaluate")
    targets = torch.tensor(ev.corpus.targets, dtype=torch.int32, device=device)
    _, exact_docs, rank, _ = index.search(*queries, RETRIEVAL_SIZE, targets=targets)
    exact = metrics_from_ranks(rank.cpu().tolist())
    lines = []
    out = open(args.out, "w") if args.out else None
    try:
        for (ptype, pvalue, rate), doc_prune in settings(args):
            params = {"prune_type": ptype, "prune_value": pvalue, "expansion_rate": rate,
                      "max_window_size": args.max_window_size}
            m, info = two_phase_eval(index, queries, targets, exact_docs, params, doc_prune=doc_prune)
            line = dict(params, doc_prune_type=doc_prune[0] if doc_prune else None,
                        doc_prune_value=doc_prune[1] if doc_prune else None, num_queries=len(ev.corpus.queries),
                        num_docs=len(ev.corpus.docs), **exact, **m)
            line["overlap@5"] = m["two_phase_overlap@5"]
            line.update({k: info[k] for k in ("postings_high", "postings_all", "window_filled", "search_s")})
            lines.append(line)
            text = json.dumps(line)
            print(text, flush=True)
            if out:
                out.write(text + "\n")
    finally:
        if out:
            out.close()
    return lines


if __name__ == "__main__":
    main()

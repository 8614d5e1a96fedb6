#!/usr/bin/env python3
"""MinHash near-duplicate removal: the Python loops of the reference's class on the CPU against the GPU path.

    python tools/gpu_minhash_bench.py [--cpu-rows 2000] [--gpu-rows 2000,100000,1000000] [--reference DIR] [--dup 0.2]

Synthetic (query, positive) rows of about 110 characters; a fraction ``--dup`` of them repeat an earlier row, half of
those with one word changed, a quarter with case and blanks changed only (the exact key catches them).  The CPU side is
the reference's MinHashDeduplicator when ``--reference`` names a checkout (loaded by file path), otherwise this
repository's restatement of it (tests/minhash_reference.py: the same two loops over hashlib), at ``--cpu-rows`` rows, one
run: it takes minutes.  The GPU side is MinHashDeduplicator.deduplicate_pairs at each of ``--gpu-rows``: host text work
(lower, strip, code points, keys), signatures (host half included), greedy rule -- timed as a whole and in parts, the median of
``--repeats`` runs after one warm-up.  One JSON line per measurement; at the CPU's row count also the ratio of the two
and the check that both kept the same rows.  Nothing is asserted about speed."""
import argparse
import importlib.util
import json
import os
import random
import statistics
import sys
import time
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

Triplet = namedtuple("Triplet", "query positive idx")


def synth_rows(n: int, dup: float, seed: int = 0):
    r = random.Random(seed)
    vocab = [f"w{r.randrange(30000)}" for _ in range(5000)]
    rows = []
    for i in range(n):
        if i and r.random() < dup:
            q, p = rows[r.randrange(i)]
            kind = r.random()
            if kind < 0.5:
                words = p.split(" ")
                words[r.randrange(len(words))] = r.choice(vocab)
                p = " ".join(words)
            elif kind < 0.75:
                q, p = f" {q.upper()}", f"{p} "
            rows.append((q, p))
        else:
            rows.append((" ".join(r.choice(vocab) for _ in range(r.randint(3, 6))),
                         " ".join(r.choice(vocab) for _ in range(r.randint(12, 18)))))
    return rows


def cpu_run(rows, reference):
    if reference:
        spec = importlib.util.spec_from_file_location(
            "ref_deduplicator", os.path.join(reference, "src", "preprocessing", "cleaners", "deduplicator.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        d = mod.MinHashDeduplicator()
        t0 = time.perf_counter()
        kept = [t.idx for t in d.deduplicate([Triplet(q, p, i) for i, (q, p) in enumerate(rows)])]
        return time.perf_counter() - t0, kept, "reference class"
    from tests import minhash_reference as R
    t0 = time.perf_counter()
    dup, _ = R.deduplicate(rows)
    return time.perf_counter() - t0, [i for i, d in enumerate(dup) if d < 0], "restatement (hashlib loops, numpy compare)"


def gpu_run(rows, repeats, device):
    import torch
    from snx import minhash as M
    from src.preprocessing.cleaners.deduplicator import MinHashDeduplicator, exact_groups
    d = MinHashDeduplicator()
    d.device = device
    need = M.need_matches(d.num_perm, d.threshold)
    whole, parts = [], {"host_s": [], "signatures_s": [], "greedy_s": []}
    for it in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dup = d.deduplicate_pairs(rows)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        texts = [M.pair_text(q, p) for q, p in rows]
        group = exact_groups(rows)
        M.signature_inputs(texts, d.num_perm, d.ngram_size)
        t2 = time.perf_counter()
        sig = M.minhash_signatures(texts, d.num_perm, d.ngram_size, device=device)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        M.greedy_dedup(sig, need, group)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if it:                                               # the first pass warms up
            whole.append(t1 - t0)
            parts["host_s"].append(t2 - t1)
            parts["signatures_s"].append(t3 - t2)             # with its own host half (lower, strip, code points) again
            parts["greedy_s"].append(t4 - t3)
    med = {k: statistics.median(v) for k, v in parts.items()}
    return statistics.median(whole), (min(whole), max(whole)), med, [i for i, x in enumerate(dup) if x < 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-rows", type=int, default=2000)
    ap.add_argument("--gpu-rows", type=str, default="2000,100000,1000000")
    ap.add_argument("--reference", type=str, default=None)
    ap.add_argument("--dup", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    sizes = [int(x) for x in args.gpu_rows.split(",") if x]
    rows = synth_rows(max(sizes + [args.cpu_rows]), args.dup)
    cpu_s, cpu_kept, what = (None, None, None)
    if args.cpu_rows:
        cpu_s, cpu_kept, what = cpu_run(rows[:args.cpu_rows], args.reference)
        print(json.dumps({"bench": "minhash_cpu", "rows": args.cpu_rows, "what": what, "seconds": round(cpu_s, 3),
                          "kept": len(cpu_kept), "runs": 1}), flush=True)
    for n in sizes:
        s, (lo, hi), parts, kept = gpu_run(rows[:n], args.repeats, args.device)
        line = {"bench": "minhash_gpu", "rows": n, "seconds": round(s, 4), "min_s": round(lo, 4), "max_s": round(hi, 4),
                "runs": args.repeats, "kept": len(kept), **{k: round(v, 4) for k, v in parts.items()}}
        if cpu_s is not None and n == args.cpu_rows:
            line["cpu_over_gpu"] = round(cpu_s / s, 1)
            line["same_rows_kept"] = kept == cpu_kept
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Graded term-expansion metrics on the GPU (snx.expansion.graded_metrics) at B x V = 4096 x 50368 and 32 x 50368 (the form
that splits rows over workgroups), 10 judgments per row, max_k = 100, cutoffs 5, 10, 20, 50, 100 -- and, on the same GPU and
the same rows, the per-query procedure the reference uses, restated: clone the row, write -inf at each special id one
element at a time, torch.topk, pull the (id, value) pairs to the host with .item(), then walk the list once per metric and
cutoff in Python.

    python tools/gpu_expansion_bench.py [--sizes 4096x50368,32x50368] [--repeats 20] [--loop-queries 64]

Synthetic rows: relu(normal - 2.5), about 0.6 % positive as a SPLADE row is; the first 7 ids are special.  Six of a row's
judged ids are drawn from its positive entries, four from anywhere.  Per size, after two untimed calls: ``call`` is a host
clock around graded_metrics (judgment check and upload, workspace clear, both kernels) ending in a synchronise; ``device``
is a pair of stream events around 10 back-to-back launches with the judgments already on the device (workspace clear and
both kernels, output allocation included), divided by 10.  Median, minimum and maximum of ``--repeats`` runs.
``row_bytes_per_s`` is B * V * 4 over the median device time -- the bytes the algorithm must read, not a counter -- next to
6.3e12, about what a plain float4 copy reaches from the MI355X's HBM (8e12 peak).  The 32-row block (6.4 MB) sits in the
last-level cache after the first call; only the 4096-row block (825 MB) is an HBM measurement.  The loop is timed over
``--loop-queries`` rows, per query.  One JSON line per measurement; nothing is asserted about speed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CUTOFFS = [5, 10, 20, 50, 100]
MAX_K = 100
SPECIAL = list(range(7))
HBM_ACHIEVABLE = 6.3e12
INNER = 10                                  # launches between the two events of a device timing


def spread(times):
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs": len(times)}


def synth(B, V, device, seed=0):
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    rep = torch.relu(torch.randn((B, V), generator=g, device=device) - 2.5).contiguous()
    ex = torch.zeros(V, dtype=torch.uint8, device=device)
    ex[SPECIAL] = 1
    rng = np.random.default_rng(seed)
    pos = (rep[:, :4096] > 0).cpu().numpy()                   # judged positives from the first 4096 ids: cheap to find
    tok = np.empty((B, 10), np.int64)
    for b in range(B):
        on = np.nonzero(pos[b])[0]
        tok[b, :6] = rng.choice(on, 6, replace=False) if len(on) >= 6 else np.arange(7, 13)
        rest = np.setdiff1d(rng.choice(V, 16, replace=False), tok[b, :6])[:4]
        tok[b, 6:] = rest
    grade = rng.integers(0, 4, size=B * 10)
    rel = (grade > 0).astype(np.int64)
    ptr = np.arange(B + 1, dtype=np.int64) * 10
    return rep, ex, (ptr, tok.reshape(-1), grade, rel)


def gpu_run(B, V, repeats, device, slices):
    import torch
    from snx.expansion import graded_metrics, judgment_csr, launch_metrics
    rep, ex, judgments = synth(B, V, device)
    on_dev = [torch.from_numpy(x).to(device) for x in judgment_csr(judgments, B)]
    call, dev_t = [], []
    for r in range(repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = graded_metrics(rep, ex, judgments, CUTOFFS, max_k=MAX_K, slices=slices)
        torch.cuda.synchronize()
        if r >= 2:
            call.append(time.perf_counter() - t0)
    for r in range(repeats + 2):                              # the launch alone: judgments already on the device
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(INNER):
            launch_metrics(rep, ex, *on_dev, CUTOFFS, MAX_K, slices)
        b.record()
        torch.cuda.synchronize()
        if r >= 2:
            dev_t.append(a.elapsed_time(b) / 1e3 / INNER)
    d = spread(dev_t)
    return {"call": spread(call), "device": d, "row_bytes": B * V * 4,
            "row_bytes_per_s": B * V * 4 / d["median_s"], "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
            "judged_in_list": int((out[0] > 0).sum()), "mean_first": float(out[2].float().mean())}, (rep, ex, judgments, out)


def loop_run(rep, judgments, nq, repeats):
    """The reference's per-query procedure, restated, over the first ``nq`` rows."""
    import math
    import torch
    ptr, tok, grade, rel = judgments
    times = []
    firsts = []
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        firsts = []
        for q in range(nq):
            masked = rep[q].clone()
            for s in SPECIAL:
                masked[s] = -float("inf")
            values, indices = torch.topk(masked, k=min(MAX_K, masked.shape[0]))
            ranking = [(i.item(), v.item()) for i, v in zip(indices, values) if v.item() > 0]
            ids = tok[ptr[q]:ptr[q + 1]].tolist()
            g_of = dict(zip(ids, grade[ptr[q]:ptr[q + 1]].tolist()))
            wanted = {t for t in ids if g_of[t] >= 1}
            first = 0
            for p, (t, _) in enumerate(ranking, start=1):
                if t in wanted:
                    first = p
                    break
            for k in CUTOFFS:
                len(wanted & {t for t, _ in ranking[:k]})
                acc = 0.0
                for p, (t, _) in enumerate(ranking[:k], start=1):
                    if g_of.get(t, 0) > 0:
                        acc += (2 ** g_of[t] - 1) / math.log2(p + 1)
            firsts.append(first)
        torch.cuda.synchronize()
        if r:
            times.append((time.perf_counter() - t0) / nq)
    return {"per_query": spread(times), "queries": nq}, firsts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096x50368,32x50368")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--loop-queries", type=int, default=64, help="0: no loop side")
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--slices", type=int, default=0)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_expansion_bench: needs a GPU")
    kept = None
    for size in [s for s in args.sizes.split(",") if s]:
        B, V = (int(x) for x in size.split("x"))
        res, state = gpu_run(B, V, args.repeats, args.device, args.slices)
        kept = kept or state
        print(json.dumps({"bench": "expansion_gpu", "B": B, "V": V, "judgments_per_row": 10, "max_k": MAX_K,
                          "slices": args.slices, **res}), flush=True)
    if args.loop_queries and kept is not None:
        rep, _, judgments, out = kept
        nq = min(args.loop_queries, rep.shape[0])
        res, firsts = loop_run(rep, judgments, nq, args.loop_repeats)
        same = firsts == out[2][:nq].cpu().tolist()
        print(json.dumps({"bench": "expansion_reference_loop", "B": nq, "V": rep.shape[1], **res,
                          "first_relevant_equal_to_gpu": same}), flush=True)


if __name__ == "__main__":
    main()

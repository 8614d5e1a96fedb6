#!/usr/bin/env python3
"""Timings of the IDF line on one GPU.  Nothing is asserted about speed; no test and no bench.py leg reads this.

    python tools/gpu_idf_bench.py [--legs step,kernels,docfreq] [--rounds 15] [--rows 1000000]

step     one micro-step (ddp_trainer.micro_step, fused passes, bf16, no optimizer step) of the 149M model at BASELINE config
         2's shapes (bs 64, q64 / d256, one negative) with SPLADELossV33, with SPLADELossIDF in encoder mode and with
         SPLADELossIDF in doc-only mode, INTERLEAVED round by round in one process: every round times the three once, each
         between two synchronisations.  The comparison row is always the SPLADELossV33 step of the same run.
kernels  snx_idf_flops_fwd and snx_idf_flops_bwd_accum alone at R in {64, 448}, V = 50368: stream events around 20
         back-to-back launches.  bytes = what the algorithm must move (forward: R V 4 read; backward: R V 4 read and R V 4
         written), next to 6.3e12 B/s, about what a plain copy reaches from HBM.  The 64-row block (13 MB) stays in the
         last-level cache between launches; only the 448-row block (90 MB) approaches an HBM measurement.
docfreq  snx.idf.doc_freq over --rows rows of 256 tokens drawn log-uniformly over the vocabulary (Zipf with s = 1), in
         chunks of 2^17 rows; the hottest id's share of all tokens is reported with the time.
Medians with minimum and maximum over --rounds runs after two untimed ones.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_ACHIEVABLE = 6.3e12
INNER = 20
V_FULL = 50368


def spread(times):
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs": len(times)}


def leg_step(dev, rounds):
    import logging
    import numpy as np
    import torch
    from bench import make_batches
    from snx.idf import penalty_weights
    from src.model.losses import SPLADELossIDF, SPLADELossV33
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.core import ddp_trainer as T
    logging.getLogger("src.model.splade_modern").setLevel(logging.ERROR)
    torch.manual_seed(42)
    model = SPLADEModernBERT().to(dev)
    wrapped = T.NativeDataParallel(model)
    V = model.vocab_size
    rng = np.random.default_rng(0)
    idf = torch.from_numpy((rng.random(V) * 8 + 0.2).astype(np.float32))
    w = penalty_weights(idf, special_ids=[0, 1, model.config.pad_token_id])
    kw = dict(lambda_q=1e-2, lambda_d=3e-3, temperature=1.0, flops_warmup_steps=20000)
    losses = {"v33": SPLADELossV33(**kw).to(dev),
              "idf_encoder": SPLADELossIDF(penalty_weights=w, **kw).to(dev),
              "idf_doc_only": SPLADELossIDF(penalty_weights=w, query_idf=idf, **kw).to(dev)}
    batches = make_batches(4, 64, 64, 256, 1, V, model.config.pad_token_id, 42, dev)
    times = {k: [] for k in losses}
    for r in range(rounds + 2):
        for name, fn in losses.items():
            wrapped.zero_grad()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T.micro_step(wrapped, fn, batches[r % 4], 100, dev, 1)
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append(time.perf_counter() - t0)
    base = statistics.median(times["v33"])
    for name, t in times.items():
        print(json.dumps({"bench": "idf_micro_step", "loss": name, "batch": 64, "q_len": 64, "d_len": 256, **spread(t),
                          "median_over_v33": statistics.median(t) / base}), flush=True)
    print(json.dumps({"bench": "idf_micro_step_token_rows", "three_pass": 64 * (64 + 2 * 256), "two_pass": 64 * 2 * 256,
                      "query_share": 64 / (64 + 2 * 256)}), flush=True)


def leg_kernels(dev, rounds):
    import torch
    from snx.idf import flops_workspace, idf_flops_bwd_accum, idf_flops_fwd
    for R in (64, 448):
        g = torch.Generator(device=dev).manual_seed(R)
        x = torch.relu(torch.randn((R, V_FULL), generator=g, device=dev) - 1.0).contiguous()
        w = torch.rand(V_FULL, generator=g, device=dev)
        dx = torch.randn((R, V_FULL), generator=g, device=dev)
        gout = torch.ones(1, device=dev)
        ws = flops_workspace(V_FULL, dev)
        for name, call, nbytes in (("snx_idf_flops_fwd", lambda: idf_flops_fwd(x, w, 0.3, 0.01, ws=ws), R * V_FULL * 4),
                                   ("snx_idf_flops_bwd_accum", lambda: idf_flops_bwd_accum(dx, ws, w, 0.3, 1e-6, gout),
                                    2 * R * V_FULL * 4)):
            t = []
            for r in range(rounds + 2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(INNER):
                    call()
                b.record()
                torch.cuda.synchronize()
                if r >= 2:
                    t.append(a.elapsed_time(b) / 1e3 / INNER)
            s = spread(t)
            print(json.dumps({"bench": "idf_kernel", "kernel": name, "R": R, "V": V_FULL, **s, "bytes": nbytes,
                              "bytes_per_s": nbytes / s["median_s"], "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}),
                  flush=True)


def leg_docfreq(dev, rounds, rows):
    import math
    import torch
    from snx.idf import doc_freq
    V, S, chunk = 250002, 256, 1 << 17
    g = torch.Generator(device=dev).manual_seed(1)
    parts = []
    for s in range(0, rows, chunk):
        u = torch.rand((min(chunk, rows - s), S), generator=g, device=dev)
        parts.append((torch.exp(u * math.log(V)).long() - 1).clamp_(0, V - 1))      # log-uniform: P(id) ~ 1 / (id + 1)
    mask = torch.ones((chunk, S), dtype=torch.long, device=dev)
    hot = sum(int((p == 0).sum()) for p in parts) / float(rows * S)
    t = []
    for r in range(min(rounds, 5) + 2):
        df = torch.zeros(V, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in parts:
            doc_freq(p, mask[:p.shape[0]], V, out=df)
        torch.cuda.synchronize()
        if r >= 2:
            t.append(time.perf_counter() - t0)
    s = spread(t)
    print(json.dumps({"bench": "idf_doc_freq", "rows": rows, "S": S, "V": V, **s, "rows_per_s": rows / s["median_s"],
                      "token_bytes_per_s": rows * S * 16 / s["median_s"], "hottest_id_token_share": hot,
                      "hottest_id_doc_freq": int(df[0]), "distinct_ids_seen": int((df > 0).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=str, default="step,kernels,docfreq")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_idf_bench: needs a GPU")
    dev = torch.device(args.device)
    legs = [x for x in args.legs.split(",") if x]
    if "kernels" in legs:
        leg_kernels(dev, args.rounds)
    if "docfreq" in legs:
        leg_docfreq(dev, args.rounds, args.rows)
    if "step" in legs:
        leg_step(dev, args.rounds)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timings of MLM pre-training on one GPU.  Nothing is asserted about speed; no test and no bench.py leg reads this.

    python tools/gpu_mlm_bench.py [--rounds 15] [--batch 32] [--seq 512] [--p 0.15]

The 149M geometry, bf16, one [B, S] batch of random ids masked with probability p (M of its B S rows carry a label).
Four variants, INTERLEAVED round by round in one process, each between two synchronisations:

step       one micro-step of MLMModernBERT: hidden-state forward, masked-row cross-entropy, its backward and the encoder's
           backward, accumulated into the flat gradient (no optimizer step)
ce_native  the cross-entropy kernels alone on the step's gathered rows: snx.mlm.ce_forward + ce_backward (tile kernel,
           merge, z -> g, the two GEMMs of the backward, the bias sum)
ce_torch   the same loss and gradients from torch.nn.functional.linear + cross_entropy under bf16 autocast on the same
           rows, the same bf16 embedding matrix's fp32 master copy and the same GPU (forward + backward)
encoder    the micro-step without the head: hidden-state forward and the backward from a given g_hd

Medians with minimum and maximum over --rounds runs after two untimed ones.  One JSON line per measurement."""
import argparse
import json
import logging
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def spread(times):
    return {"median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times),
            "runs": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--p", type=float, default=0.15)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from snx import mlm
    from src.model.mlm_modern import MLMModernBERT
    from src.model.splade_modern import SPLADEModernBERT
    logging.getLogger("src.model.splade_modern").setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    splade = SPLADEModernBERT().to(dev)
    model = MLMModernBERT(splade)
    rt = model.runtime
    rt.enable_direct_grads(True)
    V, H = splade.vocab_size, splade.hidden_size
    B, S = args.batch, args.seq
    gen = torch.Generator().manual_seed(1)
    ids = torch.randint(6, V - 1, (B, S), generator=gen).to(dev)
    att = torch.ones((B, S), dtype=torch.int64, device=dev)
    masked, labels = mlm.mask_tokens(ids, att, torch.arange(B, device=dev), special_ids=(0, 1, V - 1), mask_id=4,
                                     vocab_size=V, seed=42, p=args.p)
    rows = torch.nonzero(labels.view(-1) >= 0).view(-1)
    y = labels.view(-1)[rows]
    M = int(rows.numel())
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        hd, saved, aux = rt.forward_hidden_impl(masked, att, save=True)
        E, ET = rt.mlm_embeddings()
    h = hd.index_select(0, rows).clone()
    g_hd = torch.zeros_like(hd)
    bias = rt.params[-1]
    dE = torch.zeros((V, H), dtype=torch.float32, device=dev)
    dbias = torch.zeros((V,), dtype=torch.float32, device=dev)
    one = torch.ones((), device=dev)
    w32 = rt.params[0].detach().clone().requires_grad_(True)
    b32 = bias.detach().clone().requires_grad_(True)

    def step():
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            loss = model(masked, att, labels)
        loss.backward()

    def ce_native():
        fwd = mlm.ce_forward(h, y, E, bias)
        mlm.ce_backward(fwd, h, y, ET, one, dE, dbias)

    def ce_torch():
        hh = h.detach().clone().requires_grad_(True)
        w32.grad = b32.grad = None
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            loss = F.cross_entropy(F.linear(hh, w32, b32), y)
        loss.backward()

    def encoder():
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            _, sv, ax = rt.forward_hidden_impl(masked, att, save=True)
            rt.backward_hidden_impl(sv, ax, g_hd)

    variants = {"step": step, "ce_native": ce_native, "ce_torch": ce_torch, "encoder": encoder}
    times = {k: [] for k in variants}
    for r in range(args.rounds + 2):
        for name, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append(time.perf_counter() - t0)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        ours = float(mlm.ce_forward(h, y, E, bias).loss)
        theirs = float(F.cross_entropy(F.linear(h, w32.detach(), b32.detach()), y))
    for name in variants:
        print(json.dumps({"measurement": name, "B": B, "S": S, "M": M, "V": V, "H": H, **spread(times[name])}))
    print(json.dumps({"measurement": "loss", "native": ours, "torch_autocast": theirs,
                      "peak_memory_GB": torch.cuda.max_memory_allocated() / 1e9}))


if __name__ == "__main__":
    main()

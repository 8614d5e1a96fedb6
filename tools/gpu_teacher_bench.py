#!/usr/bin/env python3
"""Throughput of the dense teacher encoder (snx.teacher, csrc/teacher.hip) at BGE-M3's geometry, random weights.

    python tools/gpu_teacher_bench.py [--layers 24] [--rows 16384] [--reps 5] [--warmup 2] [--no-hf] [--out FILE.json]

Workloads: full batches of length 64 / 256 / 512 (``--rows`` token rows each) and a ragged batch of lengths U[8, 256];
both precisions; per workload the median, minimum and maximum wall time of ``encode_tokens`` (token ids on the device,
synchronised), texts/s and token rows/s.  Where transformers imports, its XLMRobertaModel -- what sentence-transformers
runs underneath -- is timed on the same GPU, padded, in fp32 and bf16, as the comparison row.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opensearch-neural-pre-train_amd"))


def random_weights(cfg, device, seed=0):
    """N(0, 0.02) matrices, zero biases, unit LayerNorm weights, made on the device (the recipe of the tests draws 568 M
    numbers on the host)."""
    from snx.teacher import param_keys, param_shapes
    gen = torch.Generator(device=device).manual_seed(seed)
    shapes = param_shapes(cfg)
    out = {}
    for k in param_keys(cfg):
        if k.endswith(".bias"):
            out[k] = torch.zeros(shapes[k], device=device)
        elif "LayerNorm" in k:
            out[k] = torch.ones(shapes[k], device=device)
        else:
            out[k] = 0.02 * torch.randn(shapes[k], device=device, generator=gen)
    return out


def workloads(rows, vocab, seed=0):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for length in (64, 256, 512):
        n = max(1, rows // length)
        out.append((f"len{length}", [length] * n))
    lens, total = [], 0
    while total < rows:
        lens.append(int(torch.randint(8, 257, (1,), generator=gen)))
        total += lens[-1]
    out.append(("ragged_u8_256", lens))
    batches = []
    for name, lens in out:
        S = max(lens)
        ids = torch.full((len(lens), S), 1, dtype=torch.long)
        mask = torch.zeros((len(lens), S), dtype=torch.long)
        for i, n in enumerate(lens):
            ids[i, :n] = torch.randint(3, vocab, (n,), generator=gen)
            ids[i, 0], ids[i, n - 1] = 0, 2
            mask[i, :n] = 1
        batches.append((name, ids, mask, sum(lens)))
    return batches


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def row(name, which, n, rows, t):
    med, lo, hi = t
    return {"workload": name, "engine": which, "texts": n, "token_rows": rows, "median_ms": round(med * 1e3, 3),
            "min_ms": round(lo * 1e3, 3), "max_ms": round(hi * 1e3, 3), "texts_per_s": round(n / med, 1),
            "token_rows_per_s": round(rows / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from snx.teacher import TeacherConfig, TeacherEncoder
    dev = torch.device("cuda:0")
    cfg = TeacherConfig(num_hidden_layers=args.layers)
    sd = random_weights(cfg, dev)
    batches = [(name, ids.to(dev), mask.to(dev), rows) for name, ids, mask, rows in workloads(args.rows, cfg.vocab_size)]
    results = []
    for precision in ("bf16", "fp32"):
        enc = TeacherEncoder(cfg, sd, dev, precision)
        for name, ids, mask, rows in batches:
            t = timed(lambda: enc.encode_tokens(ids, mask), args.reps, args.warmup)
            results.append(row(name, f"snx {precision}", int(ids.shape[0]), rows, t))
            print(json.dumps(results[-1]), flush=True)
        del enc
    hf = "not measured (--no-hf)"
    if not args.no_hf:
        try:
            from transformers import XLMRobertaConfig, XLMRobertaModel
            hf_cfg = XLMRobertaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
                                      intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
                                      num_attention_heads=cfg.num_attention_heads,
                                      max_position_embeddings=cfg.max_position_embeddings, type_vocab_size=1, pad_token_id=1,
                                      layer_norm_eps=cfg.layer_norm_eps, hidden_act="gelu")
            model = XLMRobertaModel(hf_cfg, add_pooling_layer=False)
            model.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=False)
            del sd
            for dtype, label in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                model = model.to(dev, dtype).eval()
                for name, ids, mask, rows in batches:
                    def run():
                        with torch.no_grad():
                            h = model(input_ids=ids, attention_mask=mask).last_hidden_state[:, 0]
                            return torch.nn.functional.normalize(h.float(), dim=-1)
                    results.append(row(name, f"transformers {label} (padded)", int(ids.shape[0]), rows,
                                       timed(run, args.reps, args.warmup)))
                    print(json.dumps(results[-1]), flush=True)
            hf = "measured"
        except ImportError as e:
            hf = f"not measured ({e})"
    doc = {"geometry": {k: getattr(cfg, k) for k in cfg.__dataclass_fields__}, "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup, "transformers": hf, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

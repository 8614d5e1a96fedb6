#!/usr/bin/env python3
"""Benchmark of the SPLADE-ModernBERT data-parallel training step on MI355X.

    python bench.py --gpus 1 --steps 16 --warmup 4
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one micro-step of BASELINE.json config 2 per GPU: 64 synthetic triplets (query 64
tokens, positive and negative document 256 tokens each, full length), i.e. three encoder
forward passes + SPLADELossV33 + backward, and on every `--accum`-th step the gradient
all-reduce (N>1), clip, AdamW and LR-schedule update -- the work of
ref:src/train/cli/train_v33_ddp.py:316-374.  Inputs are resident in HBM before the timed region.
Prints ONE JSON line (rank 0): metric triplets/s (whole job) and ms_per_step.  A plain run sets up, warms up, times
`--steps` micro-steps, writes the outputs of the last one (`--dump-outputs DIR`) and prints that line; `--full` adds
the per-kernel-class roofline, the reference's literal loop, the trained-sparsity regime, BASELINE configs 4 / 5, the
communicator record (N > 1) and the CPU baseline.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "opensearch-neural-pre-train_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def flops_per_triplet(Sq: int, Sd: int, k: int, window: int = 64):
    """Algorithmic FLOPs: forward per token 22*(Wqkv+Wo+Wi+Wo_mlp) + head + decoder,
    attention 4*768*(#unmasked pairs); step = 3 x forward (backward = 2 x forward convention)."""
    per_tok = 22 * (2 * 768 * 2304 + 2 * 768 * 768 + 2 * 768 * 2304 + 2 * 1152 * 768) + 2 * 768 * 768 + 2 * 768 * 50000

    def attn(S):
        band = sum(min(S - 1, i + window) - max(0, i - window) + 1 for i in range(S))
        return 4 * 768 * (8 * S * S + 14 * band)
    tokens = Sq + (1 + k) * Sd
    fwd = per_tok * tokens + attn(Sq) + (1 + k) * attn(Sd)
    dec_bwd_dense = 2 * (2 * 768 * 50000) * tokens          # dense dX + dW of the decoder
    dec_bwd_sparse = 2 * 2 * 768 * 50000 * (2 + k)          # routed: one row per (sequence, vocab) entry
    return {"fwd": fwd, "step": 3 * fwd, "step_executed": 3 * fwd - dec_bwd_dense + dec_bwd_sparse}


def synth_ids(B, S, vocab, pad, gen, dev):
    ids = torch.randint(6, pad, (B, S), generator=gen)
    ids[:, 0] = 0
    ids[:, -1] = 1
    return ids.to(dev), torch.ones(B, S, dtype=torch.int64, device=dev)


def make_batches(n, B, Sq, Sd, k, vocab, pad, seed, dev, teacher=False):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        q, qm = synth_ids(B, Sq, vocab, pad, gen, dev)
        p, pm = synth_ids(B, Sd, vocab, pad, gen, dev)
        n_, nm = synth_ids(B * k, Sd, vocab, pad, gen, dev)
        b = {"query_input_ids": q, "query_attention_mask": qm, "positive_input_ids": p,
             "positive_attention_mask": pm, "negative_input_ids": n_, "negative_attention_mask": nm,
             "num_negatives": k}
        if teacher:                                  # pos ~ U(0.5, 1), neg ~ U(0, 0.6)
            b["teacher_pos_scores"] = (0.5 + 0.5 * torch.rand(B, generator=gen)).to(dev)
            tn = 0.6 * torch.rand(B, k, generator=gen)
            b["teacher_neg_scores"] = (tn if k > 1 else tn[:, 0]).to(dev)
        out.append(b)
    return out


def cpu_baseline(seconds_budget: float = 30.0, cores: int | None = None):
    """The oracle (CPU restatement of the reference step, fp32, torch CPU threads = host cores given
    to this process) on a bounded sample: B=4 triplets per micro-step, q64/d256 full length."""
    from oracle import splade_oracle as O
    # The GPU box gives one GPU's job a 16-core share of the host: the default sample runs on 16 threads.  `cores`
    # (--cpu-baseline-only --cpu-cores N | all) times the same sample on any thread count; the all-physical-cores run of
    # SURVEY 8(d) is kept under profiles/ (r04_cpu_baseline_cores.json) beside the 16-thread one.
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cores = max(1, min(16, avail)) if cores is None else max(1, cores)
    torch.set_num_threads(cores)
    try:
        import psutil
        host = {"logical": psutil.cpu_count(logical=True), "physical": psutil.cpu_count(logical=False), "affinity": avail}
    except Exception:
        host = {"logical": os.cpu_count(), "physical": None, "affinity": avail}
    cfg = O.EncoderConfig()
    params = O.init_params(cfg, seed=42)
    st = O.TrainState(params)
    lc = O.LossConfig()
    gen = torch.Generator().manual_seed(42)
    times = []
    t_start = time.time()
    n = 0
    while True:
        b = O.synth_batch(4, 64, 256, cfg, gen, k=1, ragged=False)
        t0 = time.time()
        O.train_micro_steps(cfg, lc, st, [b], grad_accum=1, base_lr=5e-5, wd=0.01, clip=1.0, warmup=10,
                            total_steps=1000, global_step=n)
        times.append(time.time() - t0)
        n += 1
        if n >= 3 and (time.time() - t_start > seconds_budget or n >= 6):
            break
    timed = times[1:] if len(times) > 1 else times
    return {"value": 4.0 * len(timed) / sum(timed), "unit": "triplets/s", "cores": cores, "host_cores": host, "kind": "port",
            "sample": f"{len(timed)} timed micro-steps (after 1 warm-up) of 4 triplets q64/d256, oracle fp32 incl. "
                      "clip+AdamW every step",
            "cores_note": "16 threads = the host share of one GPU's job on the box; SURVEY 8(d) asks for all physical cores: "
                          "the same sample on 64 / 128 threads of the shared host measured SLOWER (0.57 / 0.24 triplets/s, "
                          "profiles/r04_cpu_baseline_cores.json; `bench.py --cpu-baseline-only --cpu-cores all` repeats it)"}


# kernel names (as tools/pmc_traffic.py keys them) behind each profiler class, for the PMC traffic lookup
PMC_KERNELS = {
    "gemm_nt_bf16": ["gemm_nt_kernel<128, 128, 2, 2, 0", "gemm_nt_kernel<128, 128, 2, 2, 2",
                     "gemm_nt_kernel<128, 128, 2, 2, 3", "gemm_nt_kernel<128, 128, 2, 2, 4",
                     "gemm_nt256_kernel<0", "gemm_nt256_kernel<2", "gemm_nt256_kernel<3", "gemm_nt256_kernel<4",
                     "gemm_nt_geglu_bwd_pipe_kernel"],
    "gemm_nt_resid": ["gemm_nt_kernel<128, 128, 2, 2, 1", "gemm_nt256_kernel<1"],
    "gemm_tn_accum": ["gemm_tn256_kernel", "gemm_tn_kernel"],
    "decoder_splade_fwd": ["decoder256_kernel", "decoder_splade_kernel"],
    "attn_fwd": ["attn_fwd_unit_kernel", "attn_fwd_kernel"],
    "attn_bwd": ["attn_bwd_1p_kernel", "attn_bwd_dq_unit_kernel", "attn_bwd_dkv_unit_kernel", "attn_bwd_dq_kernel",
                 "attn_bwd_dk"],
}


def kernel_source_hash() -> str:
    """sha256 over the kernel sources (csrc/*.hip, *.h): the PMC file records the hash it was measured on."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "opensearch-neural-pre-train_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


PMC_FILE = os.path.join("profiles", "r06_pmc_traffic.json")


def pmc_traffic(cls: str):
    """(average fabric bytes per launch of the class's kernels, provenance) from the committed counter passes
    (tools/pmc_traffic.py).  The counters cannot be collected inside a timed run, so the figure is only
    reported when the file was measured on EXACTLY the kernel sources being benchmarked (source hash
    recorded in the file); otherwise traffic is null."""
    path = os.path.join(ROOT, PMC_FILE)
    try:
        with open(path) as fh:
            doc = json.load(fh)
        kernels = doc["kernels"]
    except (OSError, KeyError, ValueError):
        return None, {"file": PMC_FILE, "status": "absent"}
    prov = {"file": PMC_FILE, "kernel_source_sha256": doc.get("kernel_source_sha256"),
            "workload": doc.get("workload")}
    if doc.get("kernel_source_sha256") != kernel_source_hash():
        prov["status"] = "stale: kernel sources changed since the counter passes; traffic withheld"
        return None, prov
    tot = n = 0.0
    for name, rec in kernels.items():
        if any(name.startswith(k) for k in PMC_KERNELS.get(cls, [])):
            tot += rec["fabric_bytes_per_launch"] * rec["launches"]
            n += rec["launches"]
    prov["status"] = "current"
    return (tot / n if n else None), prov


def dump_outputs(out_dir: str, loss, loss_dict: dict, model, per_param: int = 8192) -> None:
    """What the timed path computed in its last micro-step, as float32 .npy files: the loss and every entry of its loss
    dict (what ddp_trainer.micro_step returns), and a fixed, seeded sample of every parameter after that step (the
    optimizer's output: up to `per_param` entries per tensor, in named_parameters order; ~4.5 MB for the 149 M model)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), np.asarray(float(loss), dtype=np.float32))
    for key, v in loss_dict.items():
        np.save(os.path.join(out_dir, f"loss_dict_{key}.npy"), np.asarray(float(v), dtype=np.float32))
    gen = torch.Generator().manual_seed(1234)
    parts = []
    with torch.no_grad():
        for _, p in model.named_parameters():
            flat = p.detach().reshape(-1)
            if flat.numel() > per_param:
                idx = torch.randint(flat.numel(), (per_param,), generator=gen).to(flat.device)
                flat = flat[idx]
            parts.append(flat.float().cpu())
    np.save(os.path.join(out_dir, "params_sample.npy"), torch.cat(parts).numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--q-len", type=int, default=64)
    ap.add_argument("--d-len", type=int, default=256)
    ap.add_argument("--negatives", type=int, default=1)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--margin-mse", type=float, default=0.0, help="lambda_margin_mse (v34 configs: 0.5)")
    ap.add_argument("--cross-gpu-negatives", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-item-sync-leg", action="store_true",
                    help="skip the extra leg that times the reference's literal loop (three forwards + loss.item())")
    ap.add_argument("--no-sparse-regime-leg", action="store_true",
                    help="skip the extra leg that times the step with a trained model's output sparsity")
    ap.add_argument("--no-config-legs", action="store_true",
                    help="skip the extra legs that time BASELINE configs 5 (d512, 4 negatives, MarginMSE) and, at N > 1, "
                         "4 (cross-GPU in-batch negatives) beside the headline configuration")
    ap.add_argument("--cpu-baseline-only", action="store_true", help="time the CPU oracle sample and exit (no GPU)")
    ap.add_argument("--cpu-cores", default=None, help="threads of the CPU sample: a number, or 'all' (physical cores)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: per-kernel-class roofline, the extra "
                         "legs (--no-* above switch them off one by one), the communicator record at N > 1, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed micro-step to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    # A plain run does only what its headline figure needs; every other measurement or check is behind --full.
    if not args.full:
        args.no_cpu_baseline = args.no_profile = args.no_item_sync_leg = True
        args.no_sparse_regime_leg = args.no_config_legs = True

    if args.cpu_baseline_only:
        n = None
        if args.cpu_cores == "all":
            try:
                import psutil
                n = psutil.cpu_count(logical=False)
            except Exception:
                n = os.cpu_count()
        elif args.cpu_cores:
            n = int(args.cpu_cores)
        t0 = time.time()
        rec = cpu_baseline(cores=n)
        rec["wall_s_of_the_sample"] = time.time() - t0
        print(json.dumps(rec))
        return

    # N > 1 without a launcher: this process becomes the launcher.  It starts N fresh workers through
    # torch.distributed.run BEFORE making any GPU call of its own (counting devices is not one) and exits with their
    # code; a line that says n_gpus 1 can therefore never come out of a --gpus N invocation.
    if args.gpus > 1 and "RANK" not in os.environ:
        import socket
        import subprocess
        ndev = torch.cuda.device_count()
        if os.environ.get("SNX_BENCH_BACKEND", "nccl") == "nccl" and ndev < args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but {ndev} GPU(s) visible; one process per GPU over RCCL")
        with socket.socket() as sk:
            sk.bind(("", 0))        # wildcard, as the rendezvous store listens on all addresses
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        print(f"[bench] --gpus {args.gpus} without RANK: launching {' '.join(cmd)}", file=sys.stderr, flush=True)
        raise SystemExit(subprocess.run(cmd).returncode)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch N ranks for --gpus N "
                         "(python -m torch.distributed.run --nproc-per-node N bench.py --gpus N), or plain "
                         "`python bench.py --gpus N`, which starts them itself")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    # SNX_BENCH_BACKEND=gloo: REHEARSAL of the N > 1 launch line on fewer GPUs than ranks (ranks share devices, the
    # gradient buckets move through host copies: snx.dist.rccl()) -- exercises this file's multi-rank control flow, its
    # numbers mean nothing.  The measured configuration is one rank per GPU over RCCL.
    backend = os.environ.get("SNX_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and local_rank >= ndev:
        raise SystemExit(f"bench.py: rank {rank} has no GPU of its own ({ndev} visible); one process per GPU")
    local_dev = local_rank % max(ndev, 1)
    torch.cuda.set_device(local_dev)
    dev = torch.device(f"cuda:{local_dev}")
    # one process per GPU over RCCL; a 1-rank launch under torchrun with SNX_DIST_FORCE=1 also builds the group, so
    # that the collectives of the data-parallel path can be rehearsed on a single GPU
    use_pg = world > 1 or ("RANK" in os.environ and os.environ.get("SNX_DIST_FORCE", "0") == "1")
    if use_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    from snx._lib import fn
    from src.model.losses import SPLADELossV33
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.config.v33 import V33Config
    from src.train.core import ddp_trainer as T

    torch.manual_seed(42)                       # same init on every rank (DDP would broadcast rank 0)
    import logging
    logging.getLogger("src.model.splade_modern").setLevel(logging.ERROR)
    model = SPLADEModernBERT().to(dev)
    config = V33Config()
    config.training.gradient_accumulation_steps = args.accum
    wrapped = T.NativeDataParallel(model)
    loss_fn = SPLADELossV33(lambda_q=config.loss.lambda_q, lambda_d=config.loss.lambda_d,
                            temperature=config.loss.temperature, flops_warmup_steps=config.loss.flops_warmup_steps,
                            lambda_initial_ratio=config.loss.lambda_initial_ratio,
                            lambda_margin_mse=args.margin_mse).to(dev)
    optimizer = T.build_optimizer(wrapped, config)
    scheduler = T.build_scheduler(optimizer, 100, 10000)
    B, Sq, Sd, k = args.batch, args.q_len, args.d_len, args.negatives
    n_batches = min(args.steps + args.warmup, 32)   # pre-staged device batches; a timed micro-step never waits for the host
    batches = make_batches(n_batches, B, Sq, Sd, k, model.vocab_size, model.config.pad_token_id, 42 + rank, dev,
                           teacher=args.margin_mse > 0)
    xneg = args.cross_gpu_negatives
    state = {"i": 0, "gs": 0, "sync": False, "last": 0.0, "loss_dict": None}

    def one_step():
        b = batches[state["i"] % n_batches]
        if state["sync"]:
            os.environ["SNX_FUSED_PASSES"] = "0"
        loss, state["loss_dict"] = T.micro_step(wrapped, loss_fn, b, state["gs"], dev, args.accum, xneg,
                                                last_of_window=(state["i"] + 1) % args.accum == 0)
        state["i"] += 1
        if state["sync"]:
            state["last"] = loss.item()                    # ref:train_v33_ddp.py:444, one host sync per micro-step
        if state["i"] % args.accum == 0:
            T.optimizer_step(wrapped, optimizer, scheduler, config)
            state["gs"] += 1
        return loss

    def barrier():
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()

    wrapped.zero_grad()
    for _ in range(args.warmup):
        one_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = one_step()
    barrier()
    dt = time.perf_counter() - t0
    if use_pg:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    final_loss = float(loss)
    if args.dump_outputs and rank == 0:                 # before any --full leg moves the parameters on
        dump_outputs(args.dump_outputs, loss, state["loss_dict"], model)

    fl = flops_per_triplet(Sq, Sd, k)
    triplets_per_s = args.steps * B * world / dt
    result = {
        "metric": f"triplets/sec (q{Sq}/d{Sd}, bs={B}/GPU)", "value": triplets_per_s, "unit": "triplets/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000.0 * dt / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"SPLADEModernBERT 149M (A.X-Encoder-base geometry, random init) DDP step: "
                               f"bs={B}/GPU, q{Sq}/d{Sd}, {k} neg, InfoNCE+FLOPS, grad-accum {args.accum}, "
                               f"AdamW+clip every {args.accum} micro-steps"
                               + (", MarginMSE 0.5 with synthetic teacher scores" if args.margin_mse > 0 else "")
                               + (", cross-GPU in-batch negatives" if xneg else "")
                               + f"; {n_batches} pre-staged device batches cycled through ddp_trainer.micro_step / "
                                 "optimizer_step (the body of train_epoch); no per-micro-step loss.item() "
                                 "(ref:train_v33_ddp.py:444 has one): the loss stays on the device",
                   "global_batch": B * world, "parallelism": f"dp{world}", "final_loss": final_loss},
        "mfma_roofline_frac_step": triplets_per_s * fl["step"] / (world * PEAK_BF16_TFLOPS * 1e12),
        "mfma_roofline_frac_executed": triplets_per_s * fl["step_executed"] / (world * PEAK_BF16_TFLOPS * 1e12),
        "gflop_per_triplet": {"algorithmic_3x_fwd": fl["step"] / 1e9, "executed_sparse_decoder_bwd": fl["step_executed"] / 1e9},
    }

    # ---- what the communicator itself saw (N > 1): a SCALE record must not rest on this file's own `world` variable ----
    if use_pg and args.full:
        ck = torch.tensor([float(rank), 1.0], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(ck, op=dist.ReduceOp.SUM)                  # through the same group the gradients use
        names = [None] * dist.get_world_size()
        dist.all_gather_object(names, f"{torch.cuda.get_device_name(dev)}#{local_dev}")
        try:
            rccl_version = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception as e:                                      # noqa: BLE001
            rccl_version = f"unavailable: {e}"
        gs = wrapped.module.runtime.grad_sync
        result["comm"] = {"world_size": dist.get_world_size(), "backend": str(dist.get_backend()),
                          "rccl_version": rccl_version, "rank_checksum": float(ck[0]),
                          "rank_checksum_expected": world * (world - 1) / 2.0, "ranks_counted": float(ck[1]),
                          "devices": names, "grad_exchange": getattr(gs, "mode", None),
                          "grad_buckets": getattr(gs, "n_buckets", None),
                          "reserved_cus": getattr(gs, "reserved_cus", None),
                          "note": "all-reduced over the default process group after the timed region: sum of ranks and "
                                  "count of ranks as the collective library delivered them"}
        if int(ck[1]) != world or float(ck[0]) != world * (world - 1) / 2.0:
            raise SystemExit(f"bench.py: the process group reduced over {int(ck[1])} ranks (checksum {float(ck[0])}), "
                             f"expected {world}")

    # ---- per-kernel-class attribution (HIP events on the launch stream, a few extra steps) ----
    if rank == 0 and not args.no_profile:
        ncls = fn("snx_prof_num_classes")()
        names = [fn("snx_prof_class_name")(i).decode() for i in range(ncls)]
        fn("snx_prof_enable")(1)
        psteps = args.accum
        for _ in range(psteps):
            one_step()
        torch.cuda.synchronize()
        ms = (C.c_double * ncls)(); cnt = (C.c_int64 * ncls)(); work = (C.c_double * ncls)()
        fn("snx_prof_read")(ms, cnt, work)
        fn("snx_prof_enable")(0)
        classes = {}
        for i, nme in enumerate(names):
            if cnt[i]:
                classes[nme] = {"ms_per_step": ms[i] / psteps, "launches_per_step": cnt[i] / psteps,
                                "avg_us": 1000.0 * ms[i] / cnt[i], "work_per_s": work[i] / (ms[i] * 1e-3)}
        mfma = {"gemm_nt_bf16", "gemm_nt_resid", "gemm_tn_accum", "decoder_splade_fwd", "attn_fwd", "attn_bwd"}
        dom = max((c for c in classes if c in mfma), key=lambda c: classes[c]["ms_per_step"])
        ach = classes[dom]["work_per_s"] / 1e12
        traffic, prov = pmc_traffic(dom)
        result["roofline"] = {"bound": "mfma", "kernel": dom, "achieved": ach, "peak": PEAK_BF16_TFLOPS,
                              "unit": "TFLOP/s", "frac": ach / PEAK_BF16_TFLOPS, "traffic": traffic,
                              "traffic_provenance": prov,
                              "avg_launch_us": classes[dom]["avg_us"],
                              "note": "algorithmic FLOPs of every launch of this kernel class in a step / summed "
                                      "HIP-event durations of those launches (rank 0; accum extra steps right after "
                                      "the timed region, with the backward's side stream folded into the launch "
                                      "stream so that kernels are timed one at a time); traffic = fabric bytes per "
                                      "launch from the committed PMC passes (2 x FETCH_SIZE + WRITE_SIZE, averaged "
                                      "over this class's kernels), null unless measured on these kernel sources"}
        result["kernel_classes"] = classes
    elif world > 1 and not args.no_profile:
        for _ in range(args.accum):     # keep collectives matched with rank 0's profiled steps
            one_step()
        torch.cuda.synchronize()

    # ---- the reference's literal loop: model(q); model(p); model(n) and one loss.item() per micro-step ----
    if not args.no_item_sync_leg:
        fused_before = os.environ.get("SNX_FUSED_PASSES")
        state["sync"] = True
        while state["i"] % args.accum:                 # start on a window boundary
            one_step()
        for _ in range(args.accum):
            one_step()
        barrier()
        ksync = max(args.accum, min(args.steps, 4 * args.accum))
        t0 = time.perf_counter()
        for _ in range(ksync):
            one_step()
        barrier()
        dts = time.perf_counter() - t0
        state["sync"] = False
        if fused_before is None:
            os.environ.pop("SNX_FUSED_PASSES", None)
        else:
            os.environ["SNX_FUSED_PASSES"] = fused_before
        if use_pg:
            tmax = torch.tensor([dts], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dts = float(tmax.item())
        result["extra"] = {"value_with_item_sync": ksync * B * world / dts, "ms_per_step": 1000.0 * dts / ksync,
                           "steps": ksync,
                           "note": "the reference's call pattern unchanged (ref:train_v33_ddp.py:339-343,444): three "
                                   "separate forwards per micro-step (SNX_FUSED_PASSES=0) and loss.item() after "
                                   "every backward -- the three calls fill one micro-step arena and share one deferred "
                                   "backward (snx.encoder.StepArena; SNX_STEP_ARENA=0: three independent passes, "
                                   "1,145 triplets/s in round 5); `value` above runs the three batches as one native "
                                   "pass and keeps the loss on the device"}

    # ---- the step where training actually lives: a trained model's output sparsity ----
    # At random init every (sequence, vocabulary) entry of the pooled output is active, the worst case of the arg-max-routed
    # decoder backward (and the only case `value` sees).  The reference's trained model has ~54 active dimensions per
    # document and ~33 per query (ref:huggingface/v33/README.md:240-245; the FLOPS regulariser ref:src/model/losses.py:57-73
    # drives it there).  This leg shifts the decoder bias by one scalar so that the positives of batch 0 keep 54 active
    # dimensions on average, times the same micro-step, and restores the bias.  Reported under `extra`; headline untouched.
    if not args.no_sparse_regime_leg:
        from torch.amp import autocast
        bias = model.model.decoder.bias
        saved_bias = bias.detach().clone()
        b0 = batches[0]
        with torch.no_grad(), autocast(device_type="cuda", dtype=torch.bfloat16):
            (_, _), (p_rep, _) = model.forward_many([(b0["query_input_ids"], b0["query_attention_mask"]),
                                                     (b0["positive_input_ids"], b0["positive_attention_mask"])])
        kth = torch.topk(torch.expm1(p_rep.float()), 55, dim=-1).values[:, -1].mean().reshape(1)   # pooled logit of rank 55
        if use_pg:
            src_dev = kth if backend == "nccl" else kth.cpu()
            dist.broadcast(src_dev, src=0)                          # one shift for every rank: replicas stay identical
            kth = src_dev.to(dev)
        with torch.no_grad():
            bias.sub_(kth)
        wrapped.zero_grad()
        while state["i"] % args.accum:
            one_step()
        for _ in range(args.accum):
            one_step()
        barrier()
        ks = max(args.accum, min(args.steps, 4 * args.accum))
        t0 = time.perf_counter()
        for _ in range(ks):
            one_step()
        barrier()
        dtsp = time.perf_counter() - t0
        if use_pg:
            tmax = torch.tensor([dtsp], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dtsp = float(tmax.item())
        leg = {"ms_per_step": 1000.0 * dtsp / ks, "value": ks * B * world / dtsp, "steps": ks,
               "bias_shift": -float(kth.item())}
        b_last = batches[state["i"] % n_batches]
        _, ld = T.micro_step(wrapped, loss_fn, b_last, state["gs"], dev, args.accum, xneg,
                             last_of_window=(state["i"] + 1) % args.accum == 0)
        state["i"] += 1
        if state["i"] % args.accum == 0:
            T.optimizer_step(wrapped, optimizer, scheduler, config)
            state["gs"] += 1
        leg["active_dims_query"], leg["active_dims_doc"] = float(ld["nonzero_q"]), float(ld["nonzero_d"])
        if rank == 0 and not args.no_profile:
            ncls = fn("snx_prof_num_classes")()
            names = [fn("snx_prof_class_name")(i).decode() for i in range(ncls)]
            fn("snx_prof_enable")(1)
            for _ in range(args.accum):
                one_step()
            torch.cuda.synchronize()
            ms = (C.c_double * ncls)(); cnt = (C.c_int64 * ncls)(); work = (C.c_double * ncls)()
            fn("snx_prof_read")(ms, cnt, work)
            fn("snx_prof_enable")(0)
            leg["kernel_class_ms_per_step"] = {nme: ms[i] / args.accum for i, nme in enumerate(names) if cnt[i]
                                               and nme in ("splade_bwd", "decoder_splade_fwd", "embed_ln", "gemm_tn_accum")}
        elif world > 1 and not args.no_profile:
            for _ in range(args.accum):
                one_step()
            torch.cuda.synchronize()
        with torch.no_grad():
            bias.copy_(saved_bias)
        leg["note"] = ("same micro-step with the decoder bias shifted by one scalar so that ~54 vocabulary dimensions per "
                       "document stay active (the trained model's regime, ref:huggingface/v33/README.md:240-245) instead of "
                       "all 50,000 (random init, the headline's worst case for the arg-max-routed decoder backward)")
        result.setdefault("extra", {})["sparse_regime"] = leg

    # ---- BASELINE configs 4 and 5 beside the headline (config 2 / 3), so that the driver's record carries them ----
    # Only when the headline IS config 2 / 3 (the defaults): a run that was asked for another shape reports that shape alone.
    default_shape = (B, Sq, Sd, k) == (64, 64, 256, 1) and args.margin_mse == 0.0 and not xneg
    if default_shape and not args.no_config_legs:
        def timed_leg(leg_batches, leg_loss, leg_xneg, nsteps):
            st = {"i": 0}

            def step():
                bb = leg_batches[st["i"] % len(leg_batches)]
                T.micro_step(wrapped, leg_loss, bb, state["gs"], dev, args.accum, leg_xneg,
                             last_of_window=(st["i"] + 1) % args.accum == 0)
                st["i"] += 1
                if st["i"] % args.accum == 0:
                    T.optimizer_step(wrapped, optimizer, scheduler, config)
                    state["gs"] += 1
            wrapped.zero_grad()
            for _ in range(args.accum):
                step()
            barrier()
            t0 = time.perf_counter()
            for _ in range(nsteps):
                step()
            barrier()
            d = time.perf_counter() - t0
            if use_pg:
                tm = torch.tensor([d], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
                dist.all_reduce(tm, op=dist.ReduceOp.MAX)
                d = float(tm.item())
            return d
        legs = result.setdefault("extra", {})
        # Every rank takes the same branches below (the conditions are rank-independent), so the collectives inside the
        # legs stay matched; an exception inside a leg is recorded instead of costing the run its headline line.
        if backend == "nccl":                                # (two rehearsal ranks on ONE device would not fit two config-5 arenas)
            # config 5: q64 / d512, 4 negatives per query, MarginMSE 0.5 with synthetic teacher scores (2,624 tokens per triplet)
            try:
                k5, sd5 = 4, 512
                b5 = make_batches(4, B, Sq, sd5, k5, model.vocab_size, model.config.pad_token_id, 4242 + rank, dev, teacher=True)
                loss5 = SPLADELossV33(lambda_q=config.loss.lambda_q, lambda_d=config.loss.lambda_d,
                                      temperature=config.loss.temperature, flops_warmup_steps=config.loss.flops_warmup_steps,
                                      lambda_initial_ratio=config.loss.lambda_initial_ratio, lambda_margin_mse=0.5).to(dev)
                n5 = 2 * args.accum
                d5 = timed_leg(b5, loss5, False, n5)
                fl5 = flops_per_triplet(Sq, sd5, k5)
                v5 = n5 * B * world / d5
                legs["config5"] = {"workload": f"bs={B}/GPU, q{Sq}/d{sd5}, {k5} neg, InfoNCE+FLOPS+MarginMSE 0.5, "
                                               f"grad-accum {args.accum}",
                                   "value": v5, "unit": "triplets/s", "ms_per_step": 1000.0 * d5 / n5, "steps": n5,
                                   "mfma_roofline_frac_step": v5 * fl5["step"] / (world * PEAK_BF16_TFLOPS * 1e12),
                                   "mfma_roofline_frac_executed": v5 * fl5["step_executed"] / (world * PEAK_BF16_TFLOPS * 1e12)}
                del b5
            except Exception as e:                                  # noqa: BLE001
                legs["config5"] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.empty_cache()
        if world > 1:
            # config 4: config 3 + the all-gather of the positive vectors (exchange stream) / reduce-scatter backward
            try:
                n4 = 2 * args.accum
                d4 = timed_leg(batches, loss_fn, True, n4)
                legs["config4"] = {"workload": f"bs={B}/GPU, q{Sq}/d{Sd}, {k} neg, cross-GPU in-batch negatives "
                                               f"({world * B} positives per anchor row)",
                                   "value": n4 * B * world / d4, "unit": "triplets/s", "ms_per_step": 1000.0 * d4 / n4,
                                   "steps": n4}
            except Exception as e:                                  # noqa: BLE001
                legs["config4"] = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline()
    if rank == 0:
        print(json.dumps(result))
    if use_pg:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

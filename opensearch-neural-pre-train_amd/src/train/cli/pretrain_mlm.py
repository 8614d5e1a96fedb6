"""Masked-language-model pre-training of the encoder (the stage in front of SPLADE training).

The reference ships the configuration of this stage (ref:configs/pretrain_mlm.yaml) and the script that prepares its
data (ref:scripts/prepare_korean_mlm_data.py: ``train.txt`` / ``val.txt``, one paragraph per line); the CLI the yaml
points at is absent from the reference tree.  This module supplies it for the MI355X-native model:

    python -m src.train.cli.pretrain_mlm --config configs/pretrain_mlm.yaml --tokenizer DIR|hash:<vocab>

Keys read from the yaml (the reference's): model_name, data_dir, max_length, output_dir, epochs, batch_size,
grad_accum, lr, weight_decay, warmup_ratio, mlm_probability, save_steps, eval_steps, logging_steps, dataloader_workers,
seed.  ``model_name`` is a local directory (config.json [+ weights]) or a JSON file holding the geometry; it is never
resolved as a hub name.  Masking happens on the GPU (snx.mlm.mask_tokens: a token's draw depends on the seed, the epoch,
its line and its position only), the loss is the native masked-row cross-entropy (src.model.mlm_modern).  Optimizer,
schedule and checkpoint layout are the SPLADE trainer's (src.train.core.ddp_trainer), so a checkpoint directory written
here is what ``train_v33_ddp --checkpoint`` reads; ``output_dir/final_model`` holds the weights alone (model.pt +
config.json: a model-only directory, which starts a fine-tune).  Gradients are clipped at norm 1.0, the default of the
HF Trainer such a script would have used.

One process, one GPU: a world size above 1 is refused (the multi-GPU form has not run anywhere)."""
from __future__ import annotations

import argparse
import json
import logging
import math
import os
from types import SimpleNamespace
from typing import List, Optional

import torch
from torch.utils.data import DataLoader, Dataset

from snx import mlm
from src.model.mlm_modern import MLMModernBERT
from src.model.splade_modern import SPLADEModernBERT
from src.train.core import ddp_trainer as T
from src.train.data.collator import create_tokenizer

logger = logging.getLogger(__name__)

DEFAULTS = dict(model_name=None, data_dir=None, max_length=512, output_dir="outputs/pretrain_mlm", epochs=3, batch_size=32,
                grad_accum=4, lr=5.0e-5, weight_decay=0.01, warmup_ratio=0.05, mlm_probability=0.15, save_steps=2000,
                eval_steps=1000, logging_steps=100, dataloader_workers=4, seed=42)
EVAL_EPOCH = 0x7FFFFFFF            # the "epoch" word of the evaluation masks: the same masks at every evaluation
MAX_GRAD_NORM = 1.0


def load_config(path: str) -> SimpleNamespace:
    import yaml
    with open(path, encoding="utf-8") as f:
        raw = yaml.safe_load(f) or {}
    unknown = sorted(set(raw) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"{path}: unknown keys {unknown} (known: {sorted(DEFAULTS)})")
    cfg = {**DEFAULTS, **raw}
    for k in ("model_name", "data_dir"):
        if not cfg[k]:
            raise ValueError(f"{path}: {k} is required")
    for k in ("max_length", "epochs", "batch_size", "grad_accum", "save_steps", "eval_steps", "logging_steps",
              "dataloader_workers", "seed"):
        cfg[k] = int(cfg[k])
    for k in ("lr", "weight_decay", "warmup_ratio", "mlm_probability"):
        cfg[k] = float(cfg[k])
    return SimpleNamespace(**cfg)


def build_model(model_name: str) -> SPLADEModernBERT:
    """A local directory or a geometry JSON file; never a hub name."""
    if os.path.isdir(model_name):
        return SPLADEModernBERT(model_name=model_name)
    if os.path.isfile(model_name):
        with open(model_name, encoding="utf-8") as f:
            return SPLADEModernBERT(config=json.load(f))
    raise FileNotFoundError(f"model_name {model_name!r} is neither a directory with config.json nor a geometry JSON file "
                            "(names are not resolved: there is no hub here)")


def read_lines(path: str) -> List[str]:
    with open(path, encoding="utf-8") as f:
        return [ln.strip() for ln in f if ln.strip()]


class _Lines(Dataset):
    def __init__(self, lines: List[str]):
        self.lines = lines

    def __len__(self):
        return len(self.lines)

    def __getitem__(self, i):
        return i, self.lines[i]


def _collate(tokenizer, max_length: int):
    def fn(items):
        idx = torch.tensor([i for i, _ in items], dtype=torch.int64)
        enc = tokenizer([t for _, t in items], padding=True, truncation=True, max_length=max_length, return_tensors="pt")
        return idx, enc["input_ids"], enc["attention_mask"]
    return fn


def special_ids_of(tokenizer, mask_id: int) -> List[int]:
    ids = {mask_id}
    for name in ("pad_token_id", "bos_token_id", "eos_token_id", "cls_token_id", "sep_token_id", "unk_token_id"):
        v = getattr(tokenizer, name, None)
        if v is not None:
            ids.add(int(v))
    return sorted(ids)


def mask_id_of(tokenizer, override: Optional[int]) -> int:
    if override is not None:
        return int(override)
    v = getattr(tokenizer, "mask_token_id", None)
    if v is not None:
        return int(v)
    if type(tokenizer).__name__ == "HashTokenizer":
        return 4                                           # one of its unused ids below 6
    raise ValueError("the tokenizer has no mask token; pass --mask-token-id")


@torch.no_grad()
def evaluate(model: MLMModernBERT, loader, mask_kw: dict, device) -> dict:
    """Token-level mean loss and perplexity over the loader (the same masks at every call)."""
    tot = torch.zeros((), dtype=torch.float64, device=device)
    n = 0
    for idx, ids, att in loader:
        ids, att = ids.to(device), att.to(device)
        masked, labels = mlm.mask_tokens(ids, att, idx.to(device), epoch=EVAL_EPOCH, **mask_kw)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            loss = model(masked, att, labels)
        tot += loss.double() * model.last_masked_count
        n += model.last_masked_count
    loss = float(tot) / max(n, 1)
    return {"loss": loss, "perplexity": math.exp(min(loss, 80.0)), "masked_tokens": n}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--tokenizer", type=str, default=None, help="tokenizer dir or hash:<vocab> (default: model_name)")
    ap.add_argument("--mask-token-id", type=int, default=None, help="for tokenizers without a mask token")
    ap.add_argument("--max-steps", type=int, default=0, help="stop after this many optimizer steps (0: run the epochs)")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("pretrain_mlm runs in one process on one GPU; a world size above 1 is not supported (start it "
                         "without torchrun, or with --nproc_per_node=1)")
    if not torch.cuda.is_available():
        raise SystemExit("pretrain_mlm needs an AMD GPU: there is no CPU path")
    cfg = load_config(args.config)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    torch.manual_seed(cfg.seed)

    tokenizer = create_tokenizer(args.tokenizer or cfg.model_name)
    splade = build_model(cfg.model_name)
    model = MLMModernBERT(splade).to(device)
    mask_id = mask_id_of(tokenizer, args.mask_token_id)
    mask_kw = dict(special_ids=special_ids_of(tokenizer, mask_id), mask_id=mask_id, vocab_size=model.vocab_size,
                   seed=cfg.seed, p=cfg.mlm_probability)

    train_lines = read_lines(os.path.join(cfg.data_dir, "train.txt"))
    val_path = os.path.join(cfg.data_dir, "val.txt")
    val_lines = read_lines(val_path) if os.path.exists(val_path) else []
    # (a tokenizer that lives on the GPU cannot be used from worker processes)
    workers = 0 if getattr(tokenizer, "device", None) not in (None, "cpu") else cfg.dataloader_workers
    collate = _collate(tokenizer, cfg.max_length)
    gen = torch.Generator().manual_seed(cfg.seed)
    train_dl = DataLoader(_Lines(train_lines), batch_size=cfg.batch_size, shuffle=True, generator=gen, num_workers=workers,
                          collate_fn=collate, drop_last=False)
    val_dl = DataLoader(_Lines(val_lines), batch_size=cfg.batch_size, shuffle=False, num_workers=0, collate_fn=collate)

    steps_per_epoch = max(1, math.ceil(len(train_dl) / cfg.grad_accum))
    total_steps = steps_per_epoch * cfg.epochs
    if args.max_steps:
        total_steps = min(total_steps, args.max_steps)
    tcfg = SimpleNamespace(model=SimpleNamespace(name=cfg.model_name), loss=SimpleNamespace(kind="mlm", mlm_probability=cfg.mlm_probability),
                           data=SimpleNamespace(data_dir=cfg.data_dir, max_length=cfg.max_length, batch_size=cfg.batch_size),
                           training=SimpleNamespace(learning_rate=cfg.lr, weight_decay=cfg.weight_decay, warmup_ratio=cfg.warmup_ratio,
                                                    gradient_accumulation_steps=cfg.grad_accum, num_epochs=cfg.epochs, seed=cfg.seed))
    optimizer = T.build_optimizer(model, tcfg)
    scheduler = T.build_scheduler(optimizer, int(cfg.warmup_ratio * total_steps), total_steps)
    os.makedirs(cfg.output_dir, exist_ok=True)
    logger.info("MLM pre-training: %d train lines, %d val lines, %d optimizer steps, vocab %d, mask id %d", len(train_lines),
                len(val_lines), total_steps, model.vocab_size, mask_id)

    global_step, micro, last_ckpt = 0, 0, ""
    run_loss = torch.zeros((), dtype=torch.float32, device=device)
    run_n = 0
    optimizer.zero_grad(set_to_none=True)
    done = False
    for epoch in range(cfg.epochs):
        for idx, ids, att in train_dl:
            ids, att = ids.to(device, non_blocking=True), att.to(device, non_blocking=True)
            masked, labels = mlm.mask_tokens(ids, att, idx.to(device), epoch=epoch, **mask_kw)
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                loss = model(masked, att, labels)
            (loss / cfg.grad_accum).backward()
            run_loss += loss.detach()
            run_n += 1
            micro += 1
            if micro % cfg.grad_accum:
                continue
            torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_GRAD_NORM)
            optimizer.step()
            scheduler.step()
            optimizer.zero_grad(set_to_none=True)
            global_step += 1
            if global_step % cfg.logging_steps == 0:
                mean = float(run_loss) / max(run_n, 1)
                logger.info("step %d epoch %d loss %.4f ppl %.2f lr %.3e", global_step, epoch, mean, math.exp(min(mean, 80.0)),
                            scheduler.get_last_lr()[0])
                run_loss.zero_()
                run_n = 0
            if val_lines and global_step % cfg.eval_steps == 0:
                ev = evaluate(model, val_dl, mask_kw, device)
                logger.info("step %d val loss %.4f val ppl %.2f (%d masked tokens)", global_step, ev["loss"], ev["perplexity"],
                            ev["masked_tokens"])
            if global_step % cfg.save_steps == 0:
                last_ckpt = T.save_checkpoint(model, optimizer, scheduler, epoch, global_step, cfg.output_dir, tcfg)
            if global_step >= total_steps:
                done = True
                break
        if done:
            break
    if val_lines:
        ev = evaluate(model, val_dl, mask_kw, device)
        logger.info("final val loss %.4f val ppl %.2f (%d masked tokens)", ev["loss"], ev["perplexity"], ev["masked_tokens"])
    last_ckpt = T.save_checkpoint(model, optimizer, scheduler, epoch, global_step, cfg.output_dir, tcfg)
    final = os.path.join(cfg.output_dir, "final_model")
    os.makedirs(final, exist_ok=True)
    torch.save(model.state_dict(), os.path.join(final, "model.pt"))
    with open(os.path.join(final, "config.json"), "w") as f:
        json.dump(splade.model.hf_config_dict(), f, indent=2)
    tokenizer.save_pretrained(final)
    logger.info("done: %d optimizer steps; checkpoint %s; model-only directory %s", global_step, last_ckpt, final)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Shared pieces of the dense-teacher tests: the g21 golden (tools/make_golden_teacher.py), padded batches, a toy tokenizer
and one-layer configurations.  Everything is computed once per process and must not be modified by a test."""
import functools
import hashlib
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g21_teacher", "teacher.json")


def pad_batch(seqs, pad_id=1):
    S = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), S), pad_id, dtype=torch.long)
    mask = torch.zeros((len(seqs), S), dtype=torch.long)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = torch.tensor(s, dtype=torch.long)
        mask[i, :len(s)] = 1
    return ids, mask


@functools.lru_cache(maxsize=None)
def golden():
    """(json, TeacherConfig, normalised fp32 state dict from the recipe)."""
    from snx.teacher import TeacherConfig, normalize_state_dict, random_state_dict
    with open(GOLDEN) as f:
        g = json.load(f)
    cfg = TeacherConfig(**g["config"])
    return g, cfg, normalize_state_dict(cfg, random_state_dict(cfg, g["seed"]))


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def golden_reference(call: str):
    """Per golden call: (ids, mask, golden cls, golden emb, forward_torch fp32 emb, forward_torch emulated-bf16 emb,
    e_ref = max |emulated - fp32|): the comparator's own numbers, computed on the CPU."""
    from snx.teacher import forward_torch
    g, cfg, sd = golden()
    c = g["calls"][call]
    ids, mask = pad_batch(c["sequences"], cfg.pad_token_id)
    _, e32 = forward_torch(cfg, sd, ids, mask)
    _, e16 = forward_torch(cfg, sd, ids, mask, emulate_bf16=True)
    return (ids, mask, torch.tensor(c["cls"], dtype=torch.float64).float(), torch.tensor(c["emb"], dtype=torch.float64).float(),
            e32, e16, float((e16 - e32).abs().max()))


def one_layer_config(hidden: int):
    """One-layer models of the two wide geometries: 768 / 12 heads / 3072 (NV = 3) and 1024 / 16 heads / 4096 (NV = 4)."""
    from snx.teacher import TeacherConfig
    return TeacherConfig(vocab_size=300, hidden_size=hidden, intermediate_size=4 * hidden, num_hidden_layers=1,
                         num_attention_heads=hidden // 64, max_position_embeddings=300, type_vocab_size=1, pad_token_id=1,
                         layer_norm_eps=1e-5)


def ragged_sequences(lengths, vocab=300, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return [[0] + torch.randint(3, vocab, (n - 2,), generator=gen).tolist() + [2] for n in lengths]


class ToyTokenizer:
    """Whitespace words -> ids in [3, vocab) by a fixed hash, <s> = 0 first and </s> = 2 last; the call signature of an HF
    tokenizer as far as the encoder uses it."""

    def __init__(self, vocab=300):
        self.vocab = vocab

    def __call__(self, texts, truncation=True, max_length=512, padding=False, **kw):
        if isinstance(texts, str):
            texts = [texts]
        out = []
        for t in texts:
            body = [3 + int(hashlib.md5(w.encode("utf-8")).hexdigest(), 16) % (self.vocab - 3) for w in t.split()]
            out.append([0] + body[:max(0, max_length - 2)] + [2])
        return {"input_ids": out}


TEXTS = ["what is a cat", "a cat is a small animal that purrs", "dogs bark", "서울의 수도", "서울은 대한민국의 수도이다",
         "부산은 항구 도시이다", "how tall is everest", "everest is 8849 m tall", "k2 is the second highest mountain on earth",
         "rain in spain", "the rain in spain stays mainly in the plain " * 12, "x"]

#!/usr/bin/env python3
"""Write tests/golden/g21_teacher/teacher.json by RUNNING transformers' XLMRobertaModel.

    python tools/make_golden_teacher.py

A tiny XLMRobertaModel(add_pooling_layer=False) -- hidden 256, 4 heads, intermediate 512, 2 layers, vocab 300, 300
positions, one token type, pad id 1, eps 1e-5 -- in fp32 eval mode, on the CPU.  Its weights are not committed: they come
from ``snx.teacher.random_state_dict(config, SEED)`` (N(0, 0.1) matrices: see its docstring for why not 0.02), and the JSON
records the SHA-256 of every tensor so that a test notices a recipe that drifted.  Two calls: a right-padded batch of
lengths 2, 3, 17, 64, 65, 130, 257 (<s> = 0 first, </s> = 2 last, pads = 1 with mask 0) and a single sequence.  The JSON
holds the seed, the config, the hashes, the token ids, and per call the CLS rows of last_hidden_state and their
L2-normalised form.  The generator refuses to write a golden whose embeddings all point the same way (largest
off-diagonal cosine >= 0.99)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opensearch-neural-pre-train_amd"))
OUT = os.path.join(ROOT, "tests", "golden", "g21_teacher", "teacher.json")
SEED = 2101
INPUT_SEED = 2102
LENGTHS = [2, 3, 17, 64, 65, 130, 257]
SINGLE = 33
CONFIG = dict(vocab_size=300, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
              max_position_embeddings=300, type_vocab_size=1, pad_token_id=1, layer_norm_eps=1e-5)


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def sequences(lengths, rs):
    out = []
    for n in lengths:
        body = rs.randint(3, CONFIG["vocab_size"], size=n - 2).tolist()
        out.append([0] + body + [2])
    return out


def pad(seqs, pad_id):
    S = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), S), pad_id, dtype=torch.long)
    mask = torch.zeros((len(seqs), S), dtype=torch.long)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = torch.tensor(s)
        mask[i, :len(s)] = 1
    return ids, mask


def main():
    from transformers import XLMRobertaConfig, XLMRobertaModel

    from snx.teacher import TeacherConfig, hf_parameter_order, random_state_dict
    cfg = TeacherConfig(**CONFIG)
    sd = random_state_dict(cfg, SEED)
    model = XLMRobertaModel(XLMRobertaConfig(hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                             bos_token_id=0, eos_token_id=2, **CONFIG), add_pooling_layer=False)
    names = [n for n, _ in model.named_parameters()]
    assert names == hf_parameter_order(cfg), "named_parameters order differs from snx.teacher.hf_parameter_order"
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(not k.endswith((".weight", ".bias")) for k in missing), (missing, unexpected)
    model = model.float().eval()
    rs = np.random.RandomState(INPUT_SEED)
    calls = {}
    for name, lengths in (("batch", LENGTHS), ("single", [SINGLE])):
        seqs = sequences(lengths, rs)
        ids, mask = pad(seqs, cfg.pad_token_id)
        with torch.no_grad():
            cls = model(input_ids=ids, attention_mask=mask).last_hidden_state[:, 0].contiguous()
        emb = torch.nn.functional.normalize(cls, p=2, dim=-1)
        calls[name] = {"sequences": seqs, "cls": cls.double().tolist(), "emb": emb.double().tolist()}
        if len(seqs) > 1:
            cos = emb.double() @ emb.double().t()
            off = cos - 2.0 * torch.eye(len(seqs), dtype=torch.float64)
            calls[name]["max_offdiag_cosine"] = float(off.max())
            assert float(off.max()) < 0.99, f"embeddings too alike: {float(off.max())}"
    out = {"about": "tools/make_golden_teacher.py: transformers XLMRobertaModel(add_pooling_layer=False), fp32, eval, CPU",
           "seed": SEED, "input_seed": INPUT_SEED, "config": CONFIG,
           "sha256": {k: sha(sd[k]) for k in hf_parameter_order(cfg)}, "calls": calls}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); max off-diagonal cosine {calls['batch']['max_offdiag_cosine']:.4f}")


if __name__ == "__main__":
    main()

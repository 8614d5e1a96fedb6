#!/usr/bin/env python3
"""Write tests/golden/g15_teacher_scores.json by RUNNING the reference's teacher-score writer.

    python tools/make_golden_dense.py --reference <checkout of the reference project>

Loads ref:scripts/precompute_teacher_scores.py by file path (it needs numpy, torch and tqdm; sentence_transformers is
imported only inside its encoder, which is not called) and runs its own ``compute_and_save_scores`` over two tiny JSONL
shards and a tiny embedding cache.  The cache holds DYADIC embeddings (integers in [-8, 8] divided by 8, D = 16), so every
dot product is exact in fp32 whatever the order of summation, and numpy's dot and this project's fmaf chain must agree
to the last digit.  The shards cover: a plain triplet, a record without a negative, an empty negative, a negative, a
query and a positive that are missing from the cache, existing teacher keys that get overwritten, meta keys, non-ASCII
text, a line that is not JSON, and a record without a positive while the empty string IS in the cache.

The JSON records the texts in cache order, their embeddings (multiplied by 8: small integers), the shards' raw lines and
the files the reference wrote, line by line.  Tests read only the JSON."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g15_teacher_scores.json")
DIM = 16

TEXTS = ["what is a cat", "a cat is a small animal", "dogs bark", "서울의 수도", "서울은 대한민국의 수도이다", "부산은 항구 도시이다",
         "how tall is everest", "everest is 8849 m tall", "k2 is the second highest", "", "rain in spain",
         "the rain stays mainly in the plain"]
SHARDS = {
    "train_000.jsonl": [
        {"query": TEXTS[0], "positive": TEXTS[1], "negative": TEXTS[2]},
        {"query": TEXTS[3], "positive": TEXTS[4], "negative": TEXTS[5], "pair_type": "qa", "source": "kowiki"},
        {"query": TEXTS[6], "positive": TEXTS[7]},
        {"query": TEXTS[6], "positive": TEXTS[7], "negative": ""},
        "this line is not json",
        {"query": TEXTS[6], "positive": TEXTS[8], "negative": "not in the cache"},
        {"query": "a query that is not in the cache", "positive": TEXTS[1], "negative": TEXTS[2]},
    ],
    "train_001.jsonl": [
        {"query": TEXTS[10], "positive": "a positive that is not in the cache", "negative": TEXTS[2]},
        {"query": TEXTS[10], "positive": TEXTS[11], "negative": TEXTS[8], "teacher_pos_score": 9.5,
         "teacher_neg_score": -9.5, "difficulty": "hard"},
        {"query": TEXTS[0], "negative": TEXTS[2]},
        {"query": TEXTS[3], "positive": TEXTS[5], "negative": TEXTS[4]},
    ],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        "ref_precompute_teacher_scores", os.path.join(args.reference, "scripts", "precompute_teacher_scores.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(15)
    ints = rng.integers(-8, 9, size=(len(TEXTS), DIM))
    emb = (ints / 8.0).astype(np.float32)
    text_to_idx = {mod.text_hash(t): i for i, t in enumerate(TEXTS)}
    assert len(text_to_idx) == len(TEXTS)
    raw = {name: [x if isinstance(x, str) else json.dumps(x, ensure_ascii=False) for x in items]
           for name, items in SHARDS.items()}
    with tempfile.TemporaryDirectory() as td:
        src, dst = Path(td) / "in", Path(td) / "out"
        src.mkdir()
        for name, lines in raw.items():
            (src / name).write_text("".join(x + "\n" for x in lines), encoding="utf-8")
        total = mod.compute_and_save_scores([str(src / "train_*.jsonl")], dst, emb, text_to_idx)
        written = {name: (dst / name).read_text(encoding="utf-8").splitlines() for name in raw}
    out = {"source": "ref:scripts/precompute_teacher_scores.py compute_and_save_scores", "dim": DIM, "texts": TEXTS,
           "embeddings_times_8": ints.tolist(), "shards": raw, "expected": written, "total": int(total)}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {total} records scored")


if __name__ == "__main__":
    main()

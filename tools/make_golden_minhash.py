#!/usr/bin/env python3
"""Write tests/golden/g16/ by RUNNING the reference's MinHashDeduplicator.

    python tools/make_golden_minhash.py --reference <checkout of the reference project>

Loads ref:src/preprocessing/cleaners/deduplicator.py by file path (it needs only hashlib) and runs its own
``deduplicate`` over the rows below at four settings of (num_perm, threshold, ngram_size).  Data only:

  rows.json         the (query, positive) rows and, per setting, the indices the reference kept
  signatures.npz    per (num_perm, ngram_size) the reference's signatures of ALL rows (``_compute_minhash`` of
                    ``_get_ngrams`` of the row text), uint32 [n, num_perm, 4], most significant word first

The rows cover: the empty pair text's neighbours (one side empty), texts of 1 .. 4 code points, 1-, 2-, 3- and 4-byte
UTF-8, upper case with a length-changing ``lower`` (U+0130), blanks at both ends, one repeated character, exact-key
duplicates whose text differs, near duplicates above and below the thresholds, and a chain A~B~C with A and C apart."""
import argparse
import importlib.util
import json
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g16")
SETTINGS = [(128, 0.8, 3), (128, 0.5, 3), (100, 0.8, 2), (16, 1.0, 5)]

BASE = "the quick brown fox jumps over the lazy dog near the river bank"
ROWS = [
    ("", ""),
    ("a", ""),
    ("", "b"),
    ("a", "b"),
    ("ab", "c"),
    ("  What is a cat  ", "  A cat is a small animal  "),
    ("what is a cat", "a cat is a small animal"),
    ("What is a CAT", "a cat is a small animal"),
    ("what is a cat ", " a cat is a small animal"),
    ("what is a cat?", "a cat is a small animal."),
    ("what is a dog", "a dog is a loyal animal"),
    ("서울의 수도", "서울은 대한민국의 수도이다"),
    ("서울의 수도는", "서울은 대한민국의 수도이다"),
    ("부산은 어디", "부산은 항구 도시이다"),
    ("İstanbul NEREDE", "İSTANBUL Türkiye'de"),
    ("i̇stanbul nerede", "i̇stanbul türkiye'de"),
    ("москва столица", "Москва - столица России"),
    ("emoji \U0001F600 test", "smile \U0001F600\U0001F601 é ñ 한"),
    ("aaaaaaaaaaaaaaaa", "aaaaaaaaaaaaaaaaaaaaaaaa"),
    ("aaaaaaaa", "aaaa"),
    (BASE, "foxes are quick and dogs are lazy"),
    (BASE + "s", "foxes are quick and dogs are lazy"),
    (BASE, "foxes are quick and dogs are lazy!"),
    (BASE.replace("river", "rover"), "foxes are quick and dogs are lazy"),
    (BASE.replace("quick brown", "slow black"), "foxes are quick but dogs are lazy today"),
    (BASE.replace("quick brown fox", "slow black cat"), "cats are slow but dogs are lazy today ok"),
    ("how tall is everest", "everest is 8849 m tall"),
    ("how tall is everest", "everest is 8848 m tall"),
    ("how tall is k2", "k2 is 8611 m tall"),
    ("rain in spain", "the rain stays mainly in the plain"),
    ("rain in spain", "the rain stays mainly on the plain"),
    ("Rain In Spain", "The Rain Stays Mainly In The Plain"),
    ("x", "y"),
    ("xy", ""),
    ("x y", ""),
    ("abcdefghij", "klmnopqrst"),
    ("abcdefghij", "klmnopqrsu"),
    ("abcdefghix", "klmnopqrst"),
    ("abcdefghxx", "klmnopqrst"),
    ("abcdexghxx", "klmnopqrst"),
    ("1234567890", "0987654321"),
    ("1234567890", "0987654321 "),
    ("\t tabs and newlines \n", "\n kept inside\tthe text \n"),
    ("tabs and newlines", "kept inside the text"),
    ("한", "글"),
    ("\U0001F600", "\U0001F600"),
    ("\U0001F600\U0001F600", "\U0001F600\U0001F600"),
    ("éé", "é"),
]

Triplet = namedtuple("Triplet", "query positive idx")


def words(sig) -> np.ndarray:
    out = np.zeros((len(sig), 4), dtype=np.uint32)
    for i, v in enumerate(sig):
        for w in range(4):
            out[i, w] = (v >> (32 * (3 - w))) & 0xFFFFFFFF
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        "ref_deduplicator", os.path.join(args.reference, "src", "preprocessing", "cleaners", "deduplicator.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    triplets = [Triplet(q, p, i) for i, (q, p) in enumerate(ROWS)]
    kept, sigs = {}, {}
    for num_perm, threshold, ngram in SETTINGS:
        d = mod.MinHashDeduplicator(num_perm=num_perm, threshold=threshold, ngram_size=ngram)
        kept[f"{num_perm},{threshold},{ngram}"] = [t.idx for t in d.deduplicate(triplets)]
        name = f"p{num_perm}_n{ngram}"
        if name not in sigs:
            sigs[name] = np.stack([words(d._compute_minhash(d._get_ngrams(f"{q} {p}"))) for q, p in ROWS])
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "rows.json"), "w", encoding="utf-8") as f:
        json.dump({"source": "ref:src/preprocessing/cleaners/deduplicator.py MinHashDeduplicator",
                   "settings": [list(s) for s in SETTINGS], "rows": [list(r) for r in ROWS], "kept": kept}, f,
                  ensure_ascii=False, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(OUT, "signatures.npz"), **sigs)
    print(f"wrote {OUT}: {len(ROWS)} rows, kept " + ", ".join(f"{k}: {len(v)}" for k, v in kept.items()))


if __name__ == "__main__":
    main()

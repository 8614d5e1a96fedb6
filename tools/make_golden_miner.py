#!/usr/bin/env python3
"""Write tests/golden/g22_miner/miner.json by RUNNING the reference's dense hard-negative miner on its flat index.

    python tools/make_golden_miner.py --reference <checkout of the reference project>

Loads ref:src/preprocessing/miners/bge_m3_miner.py by file path.  The three things it imports that are not on this machine
are replaced by this repository's own tiny stand-ins, registered in ``sys.modules`` before the miner runs:
  faiss                              a numpy flat inner-product index (hits ordered score descending, ties lowest id first)
                                     and ``normalize_L2``
  the BGE-M3 model                   a fixed embedding table: ``encode(texts)`` returns ``{"dense_vecs": rows}``
  src.preprocessing.converters.base  a ``Triplet`` dataclass with the reference's field names
Only the flat index is recorded: the IVF lists of this project are its own, not FAISS's.

The table holds sign vectors divided by 4 at D = 16: every row has norm exactly 1 and every dot product is 1 - h / 8 for
a Hamming distance h, exact in fp32 in any order of summation, so the recorded scores are exact and the flat index of
this project must reproduce them to the last bit.  The cases cover every skip rule of ref:bge_m3_miner.py:216-226 (the
record's positive, a doc whose text is the query, a positive of another record, a score below and above the band), a
search cut at k = 10 * num_negatives, a band that leaves fewer than num_negatives, and mine_for_triplets with and without
skip_complete (a triplet that stays without a negative included)."""
import argparse
import dataclasses
import importlib.util
import json
import os
import sys
import types
from typing import Any, Dict, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g22_miner", "miner.json")
DIM = 16

Q1 = list(range(8, 16))
# text -> the positions whose sign is flipped against the all-plus vector
TABLE = {
    "what do cats eat": [],
    "which planet is the largest": Q1,
    "how are pearls made": [0, 2, 4, 6, 8, 10, 12, 14],
    "cats eat meat and fish": [0],                           # positive of query 0 (0.875)
    "jupiter is the largest planet": [1, 2],                 # positive of query 1, and 0.75 from query 0
    "cats are obligate carnivores": [3],                     # 0.875 from query 0: above the band
    "a cat's diet is mostly protein": [4, 5],                # 0.75
    "kittens drink milk": [6, 7, 8],                         # 0.625
    "dogs eat almost anything": [0, 1, 2, 3, 4, 5],          # 0.25: below the band
    "many pets eat dry food": [9, 10, 11, 12],               # 0.5
    "saturn is the second largest planet": Q1 + [0],         # 0.875 from query 1
    "jupiter has a great red spot": Q1 + [0, 1],             # 0.75 from query 1
    "planets orbit the sun": Q1 + [0, 1, 2, 3],              # 0.5 from query 1
    "fish swim in the sea": [5, 6, 7, 9, 11],                # 0.375
}
QUERIES = list(TABLE)[:3]
DOCUMENTS = [QUERIES[0]] + list(TABLE)[3:]                   # the pool holds a doc whose text is query 0
CASES = [
    {"num_negatives": 2, "min_score": 0.3, "max_score": 0.85},
    {"num_negatives": 5, "min_score": 0.3, "max_score": 0.85},
    {"num_negatives": 1, "min_score": 0.55, "max_score": 0.7},
    {"num_negatives": 1, "min_score": -1.0, "max_score": 2.0},
]


@dataclasses.dataclass
class Triplet:
    query: str
    positive: str
    negative: Optional[str] = None
    pair_type: str = "unknown"
    difficulty: str = "medium"
    source: str = ""
    metadata: Dict[str, Any] = dataclasses.field(default_factory=dict)


def embeddings(texts):
    out = np.full((len(texts), DIM), 0.25, np.float32)
    for i, t in enumerate(texts):
        out[i, TABLE[t]] = -0.25
    return out


class _FlatIP:
    def __init__(self, dim):
        self.dim, self.rows, self.ntotal = dim, np.zeros((0, dim), np.float32), 0

    def add(self, x):
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])
        self.ntotal = self.rows.shape[0]

    def search(self, q, k):
        s = np.asarray(q, np.float32) @ self.rows.T
        order = np.argsort(-s, axis=1, kind="stable")[:, :k]
        return np.take_along_axis(s, order, 1), order


def _normalize_l2(x):
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))


class _Model:
    def encode(self, batch, batch_size=None, max_length=None):
        return {"dense_vecs": embeddings(batch)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    faiss = types.ModuleType("faiss")
    faiss.IndexFlatIP, faiss.normalize_L2 = _FlatIP, _normalize_l2
    base = types.ModuleType("src.preprocessing.converters.base")
    base.Triplet = Triplet
    saved = {n: sys.modules.get(n) for n in ("faiss", "src", "src.preprocessing", "src.preprocessing.converters",
                                             "src.preprocessing.converters.base")}
    sys.modules["faiss"] = faiss
    for name in ("src", "src.preprocessing", "src.preprocessing.converters"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    sys.modules["src.preprocessing.converters.base"] = base
    spec = importlib.util.spec_from_file_location(
        "ref_bge_m3_miner", os.path.join(args.reference, "src", "preprocessing", "miners", "bge_m3_miner.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    miner = mod.BGEM3HardNegativeMiner(device="cpu")
    miner._model = _Model()
    miner.build_index(list(DOCUMENTS), index_type="flat")
    positives = [list(TABLE)[3], list(TABLE)[4], list(TABLE)[9]]
    cases = []
    for kw in CASES:
        res = miner.mine_negatives(list(QUERIES), list(positives), **kw)
        cases.append({"kind": "mine_negatives", "queries": QUERIES, "positives": positives, "kwargs": kw,
                      "results": [dataclasses.asdict(r) for r in res]})
    triplets = [Triplet(QUERIES[0], positives[0], None, "qa", "easy", "pets", {"id": 7}),
                Triplet(QUERIES[1], positives[1], "planets orbit the sun", "qa", "medium", "space", {}),
                Triplet(QUERIES[2], positives[2], None, "qa", "medium", "sea", {"id": 9})]
    for skip in (True, False):
        kw = {"num_negatives": 1, "min_score": 0.3, "max_score": 0.85, "skip_complete": skip}
        res = miner.mine_for_triplets([dataclasses.replace(t) for t in triplets], **kw)
        cases.append({"kind": "mine_for_triplets", "triplets": [dataclasses.asdict(t) for t in triplets], "kwargs": kw,
                      "results": [dataclasses.asdict(t) for t in res]})
    for n, m in saved.items():
        if m is None:
            sys.modules.pop(n, None)
        else:
            sys.modules[n] = m
    texts = list(TABLE)
    out = {"source": "ref:src/preprocessing/miners/bge_m3_miner.py BGEM3HardNegativeMiner, index_type='flat'", "dim": DIM,
           "texts": texts, "embeddings_times_4": (embeddings(texts) * 4).astype(int).tolist(), "documents": DOCUMENTS,
           "cases": cases}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(cases)} cases")


if __name__ == "__main__":
    main()

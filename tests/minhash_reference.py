"""Host restatement of MinHash near-duplicate removal (include/snx.h "MinHash near-duplicate removal") with hashlib and
plain Python integers: what csrc/minhash.hip is held to, and what tests/golden/g16 (written by RUNNING the reference's
MinHashDeduplicator, tools/make_golden_minhash.py) holds this file to."""
import hashlib

import numpy as np


def row_text(query: str, positive: str) -> str:
    return f"{query} {positive}".lower().strip()


def ngrams(text: str, n: int) -> set:
    """``text`` is lowered and stripped already."""
    if len(text) < n:
        return {text}
    return {text[i:i + n] for i in range(len(text) - n + 1)}


def signature(text: str, num_perm: int, n: int) -> list:
    """num_perm Python ints (128 bits each) of a lowered, stripped text."""
    grams = ngrams(text, n)
    return [min(int(hashlib.md5(f"{i}_{g}".encode()).hexdigest(), 16) for g in grams) for i in range(num_perm)]


def words(sigs) -> np.ndarray:
    """Signatures (lists of ints) -> uint32 [n, num_perm, 4], most significant word first."""
    out = np.zeros((len(sigs), len(sigs[0]) if sigs else 0, 4), dtype=np.uint32)
    for r, s in enumerate(sigs):
        for i, v in enumerate(s):
            for w in range(4):
                out[r, i, w] = (v >> (32 * (3 - w))) & 0xFFFFFFFF
    return out


def signatures(texts, num_perm: int = 128, n: int = 3) -> np.ndarray:
    """Raw texts (lowered and stripped here) -> uint32 [n, num_perm, 4]."""
    return words([signature(t.lower().strip(), num_perm, n) for t in texts])


def pair_key(query: str, positive: str) -> str:
    return hashlib.md5(f"{query.strip().lower()}|||{positive.strip().lower()}".encode()).hexdigest()


def need_matches(num_perm: int, threshold: float) -> int:
    for m in range(num_perm + 1):
        if m / num_perm >= threshold:
            return m
    return num_perm + 1


def greedy(sig: np.ndarray, need: int, group=None) -> np.ndarray:
    """The greedy rule on uint32 [n, P, 4] signatures -> duplicate_of int32 [n]."""
    n = sig.shape[0]
    dup = np.full(n, -1, dtype=np.int32)
    kept = []
    keeper = {}
    for i in range(n):
        d = -1
        if group is not None and int(group[i]) in keeper:
            d = keeper[int(group[i])]
        elif kept:
            counts = (sig[kept] == sig[i]).all(axis=2).sum(axis=1)       # positions equal on all 128 bits, per kept row
            hit = np.flatnonzero(counts >= need)
            if hit.size:
                d = kept[int(hit[0])]
        dup[i] = d
        if d < 0:
            kept.append(i)
            if group is not None:
                keeper[int(group[i])] = i
    return dup


def deduplicate(pairs, num_perm: int = 128, threshold: float = 0.8, n: int = 3):
    """(query, positive) tuples -> (duplicate_of int32 [n], signatures uint32 [n, num_perm, 4])."""
    sig = signatures([f"{q} {p}" for q, p in pairs], num_perm, n)
    first = {}
    group = np.array([first.setdefault(pair_key(q, p), i) for i, (q, p) in enumerate(pairs)], dtype=np.int32)
    return greedy(sig, need_matches(num_perm, threshold), group), sig

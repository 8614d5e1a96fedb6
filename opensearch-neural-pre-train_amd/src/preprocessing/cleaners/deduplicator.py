"""Deduplication of triplets by their (query, positive) pair (ref:src/preprocessing/cleaners/deduplicator.py).

``MinHashDeduplicator`` has the reference's constructor, ``deduplicate``, ``is_duplicate`` and ``clear`` and makes the
reference's decisions row for row; its two hot loops run on the GPU (``snx.minhash``, csrc/minhash.hip):

  deduplicate    one batch: every row's signature in one launch, then the greedy rule block by block.  Afterwards
                 ``duplicate_of`` (numpy int32 [n]: -1 for a kept row, else the kept row it repeats) and ``signatures``
                 (uint32 [n, num_perm, 4] on the device) can be read from the object.
  is_duplicate   one row against the kept signatures, which stay on the device; fed the rows of a batch one at a time it
                 answers as ``deduplicate`` does, and after a ``deduplicate`` it continues from that batch's kept rows,
                 as the reference's does.

The exact key of a pair is the reference's string ``f"{query.strip().lower()}|||{positive.strip().lower()}"``
(ref:deduplicator.py:109); the reference stores its MD5, equal exactly when the strings are.  ``ExactDeduplicator`` is the
host-only class the reference's pipeline uses instead (ref:src/preprocessing/pipeline.py:112): its key neither lowers
nor is shared with the one above."""
from __future__ import annotations

import logging
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

logger = logging.getLogger(__name__)


def pair_key(query: str, positive: str) -> str:
    """The exact key of a pair (ref:deduplicator.py:109)."""
    return f"{query.strip().lower()}|||{positive.strip().lower()}"


def exact_groups(pairs: Sequence[Tuple[str, str]]) -> np.ndarray:
    """int32 [n]: per row the index of the first row with the same exact key."""
    first: Dict[str, int] = {}
    return np.fromiter((first.setdefault(pair_key(q, p), i) for i, (q, p) in enumerate(pairs)), dtype=np.int32,
                       count=len(pairs))


class MinHashDeduplicator:
    """Remove near-duplicate triplets by MinHash signatures of their (query, positive) text."""

    device = "cuda"                                          # where the signatures live; set before the first call

    def __init__(self, num_perm: int = 128, threshold: float = 0.8, ngram_size: int = 3):
        self.num_perm = num_perm
        self.threshold = threshold
        self.ngram_size = ngram_size
        self.duplicate_of: Optional[np.ndarray] = None
        self.signatures = None
        self._seen: Set[str] = set()
        self._kept = None                                    # int32 [capacity, num_perm, 4] on the device
        self._nk = 0

    def _need(self) -> int:
        from snx import minhash as M
        return M.need_matches(self.num_perm, self.threshold)

    def deduplicate_pairs(self, pairs: Sequence[Tuple[str, str]]) -> np.ndarray:
        """``deduplicate`` on (query, positive) tuples -> duplicate_of, numpy int32 [n]."""
        import torch
        from snx import minhash as M
        pairs = list(pairs)
        self.clear()
        texts = [M.pair_text(q, p) for q, p in pairs]
        sig = M.minhash_signatures(texts, self.num_perm, self.ngram_size, device=self.device)
        dup = M.greedy_dedup(sig, self._need(), exact_groups(pairs))
        self.signatures = sig
        self.duplicate_of = dup.cpu().numpy()
        kept = np.flatnonzero(self.duplicate_of < 0)
        self._seen = {pair_key(*pairs[i]) for i in kept}
        self._kept = sig.view(torch.int32)[torch.from_numpy(kept).to(sig.device)]
        self._nk = int(kept.size)
        return self.duplicate_of

    def deduplicate(self, triplets: List["Triplet"]) -> List["Triplet"]:
        """The triplets that are no duplicate of an earlier kept one, in order (ref:deduplicator.py:146-181)."""
        logger.info(f"Deduplicating {len(triplets)} triplets")
        dup = self.deduplicate_pairs([(t.query, t.positive) for t in triplets])
        unique = [t for t, d in zip(triplets, dup) if d < 0]
        logger.info(f"Deduplication complete: {len(triplets)} -> {len(unique)} "
                    f"(removed {len(triplets) - len(unique)} duplicates)")
        return unique

    def is_duplicate(self, query: str, positive: str) -> bool:
        """True if the pair repeats one seen before; a new pair is remembered (ref:deduplicator.py:112-144)."""
        import torch
        from snx import minhash as M
        key = pair_key(query, positive)
        if key in self._seen:
            return True
        sig = M.minhash_signatures([M.pair_text(query, positive)], self.num_perm, self.ngram_size,
                                   device=self.device).view(torch.int32)
        if self._nk and int(M.first_match(sig, self._kept[:self._nk], self._need())[0]) >= 0:
            return True
        if self._kept is None or self._nk == self._kept.shape[0]:
            grown = torch.empty((max(256, 2 * self._nk), sig.shape[1], 4), dtype=torch.int32, device=sig.device)
            if self._nk:
                grown[:self._nk] = self._kept[:self._nk]
            self._kept = grown
        self._kept[self._nk] = sig[0]
        self._nk += 1
        self._seen.add(key)
        return False

    def clear(self) -> None:
        """Forget every pair seen."""
        self._seen = set()
        self._kept = None
        self._nk = 0
        self.duplicate_of = None
        self.signatures = None
        logger.info("Deduplicator state cleared")


class ExactDeduplicator:
    """Exact-match deduplication on the host (ref:deduplicator.py:190-231): the key is the stripped pair, case kept."""

    def __init__(self):
        self._seen: Set[str] = set()

    def _get_key(self, query: str, positive: str) -> str:
        return f"{query.strip()}|||{positive.strip()}"

    def is_duplicate(self, query: str, positive: str) -> bool:
        key = self._get_key(query, positive)
        if key in self._seen:
            return True
        self._seen.add(key)
        return False

    def deduplicate(self, triplets: List["Triplet"]) -> List["Triplet"]:
        self._seen.clear()
        unique = [t for t in triplets if not self.is_duplicate(t.query, t.positive)]
        logger.info(f"Exact deduplication: {len(triplets)} -> {len(unique)} "
                    f"(removed {len(triplets) - len(unique)} duplicates)")
        return unique

    def clear(self) -> None:
        self._seen.clear()

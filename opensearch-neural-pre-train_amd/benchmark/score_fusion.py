"""The fusion classes of ref:benchmark/score_fusion.py over the GPU rule ``snx.retrieval.fuse_ranked``.

``RankedResult``, ``RRFFusion(k=60)``, ``LinearFusion(alpha=0.4)``, ``WeightedRRFFusion(k=60, sparse_weight=0.4,
dense_weight=0.6)`` and ``create_fusion_method(method, **kwargs)`` keep the reference's constructor arguments, defaults
and return types: ``fuse(sparse_results, dense_results)`` takes and returns lists of ``RankedResult`` whose ``doc_id`` is
any hashable.  Underneath, the two lists become int32 / fp32 rows and one ``snx_fuse_ranked`` launch fuses them; fused
scores are the reference's float64 values bit for bit.  Where the reference leaves the order of equal fused scores to
Python's set iteration, here the doc that appears first (sparse list, then dense list) comes first.  Scores are taken
as fp32, the type every search of this project returns.  A list may hold up to 1024 results with distinct doc ids."""
from __future__ import annotations

from abc import ABC, abstractmethod
from dataclasses import dataclass
from typing import Hashable, List


@dataclass
class RankedResult:
    """A search result with rank information."""

    doc_id: Hashable
    score: float
    rank: int


class ScoreFusion(ABC):
    """Base class of the fusion methods."""

    method = ""

    @abstractmethod
    def _params(self) -> dict:
        ...

    def fuse(self, sparse_results: List[RankedResult], dense_results: List[RankedResult]) -> List[RankedResult]:
        """Fused and re-ranked results of the two lists (rank = position in each list, as the reference's searchers
        number them)."""
        import torch
        from snx.retrieval import fuse_ranked
        lists = [sorted(rs, key=lambda r: r.rank) for rs in (sparse_results, dense_results)]
        if any([r.rank for r in rs] != list(range(1, len(rs) + 1)) for rs in lists):
            raise ValueError("fuse: ranks must be 1 .. len(results) within each list")
        number: dict = {}
        for rs in lists:
            for r in rs:
                number.setdefault(r.doc_id, len(number))
        names = list(number)
        R = max(1, max(len(rs) for rs in lists))
        dev = torch.device("cuda", torch.cuda.current_device())
        pairs = []
        for rs in lists:
            docs = torch.full((1, R), -1, dtype=torch.int32)
            scores = torch.zeros((1, R), dtype=torch.float32)
            docs[0, :len(rs)] = torch.tensor([number[r.doc_id] for r in rs], dtype=torch.int32)
            scores[0, :len(rs)] = torch.tensor([float(r.score) for r in rs], dtype=torch.float32)
            pairs.append((docs.to(dev), scores.to(dev)))
        scores, docs, _, total = fuse_ranked(pairs, self.method, max(1, len(names)), **self._params())
        n = int(total[0])
        return [RankedResult(doc_id=names[d], score=s, rank=i + 1)
                for i, (d, s) in enumerate(zip(docs[0, :n].tolist(), scores[0, :n].tolist()))]


class RRFFusion(ScoreFusion):
    """Reciprocal Rank Fusion: score = sum over the systems of 1 / (k + rank); a doc absent from a list takes the rank
    max(len(sparse) + 1, len(dense) + 1, 100)."""

    method = "rrf"

    def __init__(self, k: int = 60):
        self.k = k

    def _params(self) -> dict:
        return {"k": self.k}


class LinearFusion(ScoreFusion):
    """score = alpha * norm(sparse_score) + (1 - alpha) * norm(dense_score), min-max normalised per list."""

    method = "linear"

    def __init__(self, alpha: float = 0.4):
        if not 0 <= alpha <= 1:
            raise ValueError("alpha must be between 0 and 1")
        self.alpha = alpha

    def _params(self) -> dict:
        return {"alpha": self.alpha}


class WeightedRRFFusion(ScoreFusion):
    """score = sparse_weight / (k + rank_sparse) + dense_weight / (k + rank_dense)."""

    method = "weighted_rrf"

    def __init__(self, k: int = 60, sparse_weight: float = 0.4, dense_weight: float = 0.6):
        self.k = k
        self.sparse_weight = sparse_weight
        self.dense_weight = dense_weight

    def _params(self) -> dict:
        return {"k": self.k, "weights": (self.sparse_weight, self.dense_weight)}


def create_fusion_method(method: str, **kwargs) -> ScoreFusion:
    """One of "rrf", "linear", "weighted_rrf" with its constructor arguments."""
    methods = {"rrf": RRFFusion, "linear": LinearFusion, "weighted_rrf": WeightedRRFFusion}
    if method not in methods:
        raise ValueError(f"Unknown fusion method: {method}. Choose from {list(methods.keys())}")
    return methods[method](**kwargs)

"""Dense hard-negative mining over teacher embeddings on the GPU: the reference's ``BGEM3HardNegativeMiner``
(ref:src/preprocessing/miners/bge_m3_miner.py), with its FAISS indexes replaced by ``snx.retrieval.DenseIndex``
(``index_type="flat"``) and ``snx.retrieval.IvfFlatIndex`` (``"ivf"``), and FlagEmbedding by the native teacher encoder.

Parity with the reference is claimed for the flat index and for the selection rules.  The IVF lists are the index's own
deterministic spherical k-means (include/snx.h "IVF-Flat dense retrieval"), NOT the lists FAISS would train: FAISS's
sampling and random generator are not reproduced, so an ``"ivf"`` run finds the reference's negatives only as far as
both clusterings put them into the probed list.

One deliberate deviation: when a search returns fewer than ``k`` hits (an IVF probe whose lists hold fewer docs) the
unfilled slots are doc ``-1``; they are skipped here.  The reference would index its document pool with ``-1`` and hand
out the LAST document of the pool."""
from __future__ import annotations

import dataclasses
import logging
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import numpy as np

logger = logging.getLogger(__name__)


@dataclass
class MiningResult:
    """Result of hard negative mining."""

    query: str
    positive: str
    negatives: List[str]
    negative_scores: List[float]


def _normalized(x: np.ndarray) -> np.ndarray:
    """Rows divided by their L2 norm in fp32, as ``faiss.normalize_L2`` does; a zero row stays zero."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    norm = np.sqrt((x * x).sum(axis=1, dtype=np.float32, keepdims=True), dtype=np.float32)
    return np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)


class BGEM3HardNegativeMiner:
    """Finds semantically similar but non-relevant documents as hard negatives (ref:bge_m3_miner.py:22-329).

    ``model_name`` is a LOCAL directory of the teacher (``src.model.teachers.BGEM3Teacher``); a hub name is never
    resolved.  ``encode``: a callable ``texts -> array-like [len(texts), dim]`` used instead of a model (cached embeddings,
    tests).  ``index_classes``: ``{"flat": cls, "ivf": cls}`` with the interfaces of ``DenseIndex`` / ``IvfFlatIndex``
    (default: those two); a class whose instances have no ``device`` attribute is fed numpy arrays."""

    def __init__(self, model_name: str = "BAAI/bge-m3", batch_size: int = 32, max_length: int = 192,
                 device: Optional[str] = None, use_fp16: bool = True, *, encode: Optional[Callable] = None,
                 index_classes: Optional[Dict[str, type]] = None):
        self.model_name = model_name
        self.batch_size = batch_size
        self.max_length = max_length
        self.use_fp16 = use_fp16
        self._encode = encode
        self._index_classes = index_classes
        self._model = None
        self._index = None
        self._document_pool: List[str] = []
        self._document_embeddings: Optional[np.ndarray] = None
        if device is None:
            import torch
            self.device = "cuda" if torch.cuda.is_available() else "cpu"
        else:
            self.device = device
        logger.info(f"BGE-M3 miner initialized (device={self.device})")

    @property
    def model(self):
        """The teacher, loaded on first use from the local directory ``model_name``."""
        if self._model is None:
            if not os.path.isdir(self.model_name):
                raise FileNotFoundError(f"BGEM3HardNegativeMiner: {self.model_name!r} is not a local model directory "
                                        "(model names are not resolved; pass a directory or encode=...)")
            from src.model.teachers import BGEM3Teacher
            self._model = BGEM3Teacher(self.model_name, device=self.device, max_length=self.max_length,
                                       normalize_embeddings=True, precision="bf16" if self.use_fp16 else "fp32")
        return self._model

    def _encode_batch(self, texts: List[str]) -> np.ndarray:
        """Texts -> fp32 embeddings [len(texts), dim] on the host."""
        out = self._encode(list(texts)) if self._encode is not None else self.model.encode(list(texts))
        if isinstance(out, dict):
            out = out["dense_vecs"]
        if not isinstance(out, np.ndarray):
            out = out.detach().float().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
        return np.ascontiguousarray(out, dtype=np.float32).reshape(len(texts), -1)

    def _classes(self) -> Dict[str, type]:
        if self._index_classes is not None:
            return self._index_classes
        from snx.retrieval import DenseIndex, IvfFlatIndex
        return {"flat": DenseIndex, "ivf": IvfFlatIndex}

    def _to_index(self, a: np.ndarray):
        dev = getattr(self._index, "device", None)
        if dev is None:
            return a
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def build_index(self, documents: List[str], index_type: str = "flat", nlist: int = 100,
                    nprobe: int = 1) -> None:
        """Index ``documents`` (ref:bge_m3_miner.py:91-136).  ``"ivf"``: ``min(nlist, len(documents))`` lists, searched
        with ``nprobe`` of them (FAISS's default 1, which the reference never changes).  As in the reference, the IVF
        quantizer is trained on the rows BEFORE they are L2-normalised; BGE-M3's rows arrive normalised, so that only
        matters for other encoders."""
        if index_type not in ("flat", "ivf"):
            raise ValueError(f"Unknown index type: {index_type}")
        logger.info(f"Building {index_type} index for {len(documents)} documents")
        self._document_pool = documents
        emb = self._encode_batch(documents)
        dim = int(emb.shape[1])
        if index_type == "flat":
            self._index = self._classes()["flat"](dim, self.device)
        else:
            nlist = min(int(nlist), len(documents))
            self._index = self._classes()["ivf"](dim, nlist, self.device, nprobe=min(int(nprobe), nlist))
            self._index.train(self._to_index(emb))
        self._document_embeddings = _normalized(emb)
        self._index.add(self._to_index(self._document_embeddings))
        self._index.build()
        logger.info(f"Index built: {self._index.num_docs} vectors")

    def mine_negatives(self, queries: List[str], positives: List[str], num_negatives: int = 5, min_score: float = 0.3,
                       max_score: float = 0.85) -> List[MiningResult]:
        """Hard negatives for query-positive pairs (ref:bge_m3_miner.py:166-249): the top ``10 * num_negatives`` hits in
        rank order, skipping -- in this order -- the record's positive, the query, any positive of the set, a score
        below ``min_score`` and a score above ``max_score``, until ``num_negatives`` are kept."""
        if self._index is None:
            raise RuntimeError("Index not built. Call build_index() first.")
        logger.info(f"Mining negatives for {len(queries)} queries")
        positive_set = set(positives)
        ntotal = int(self._index.num_docs)
        k = min(num_negatives * 10, ntotal)
        results: List[MiningResult] = []
        scores = indices = None
        if k >= 1 and len(queries):
            q = self._to_index(_normalized(self._encode_batch(queries)))
            out = self._index.search(q, k)
            scores, indices = (x if isinstance(x, np.ndarray) else x.cpu().numpy() for x in out[:2])
        for i, (query, positive) in enumerate(zip(queries, positives)):
            negatives: List[str] = []
            negative_scores: List[float] = []
            for j in range(k if scores is not None else 0):
                if len(negatives) >= num_negatives:
                    break
                idx, score = int(indices[i, j]), scores[i, j]
                if idx < 0:                                  # an unfilled slot (the deviation of the module docstring)
                    continue
                candidate = self._document_pool[idx]
                if candidate == positive:
                    continue
                if candidate == query:
                    continue
                if candidate in positive_set:
                    continue
                if score < min_score:
                    continue
                if score > max_score:
                    continue
                negatives.append(candidate)
                negative_scores.append(float(score))
            results.append(MiningResult(query=query, positive=positive, negatives=negatives,
                                        negative_scores=negative_scores))
        found = sum(1 for r in results if r.negatives)
        avg = sum(len(r.negatives) for r in results) / len(results) if results else 0
        logger.info(f"Mining complete: {found}/{len(queries)} queries found negatives (avg {avg:.1f} per query)")
        return results

    def mine_for_triplets(self, triplets: List, num_negatives: int = 1, min_score: float = 0.3, max_score: float = 0.85,
                          skip_complete: bool = True) -> List:
        """Fill the missing ``negative`` of triplets (ref:bge_m3_miner.py:251-322).  ``triplets``: dataclass instances
        with the reference's field names (query, positive, negative, difficulty, metadata, ...); an updated triplet is
        ``dataclasses.replace`` of the original.  Returns ``complete + updated``, as the reference does."""
        if skip_complete:
            needs_mining = [t for t in triplets if t.negative is None]
            complete = [t for t in triplets if t.negative is not None]
        else:
            needs_mining = triplets
            complete = []
        if not needs_mining:
            logger.info("No triplets need mining")
            return triplets
        if self._index is None:
            self.build_index(list(set(t.positive for t in triplets)))
        results = self.mine_negatives([t.query for t in needs_mining], [t.positive for t in needs_mining],
                                      num_negatives, min_score, max_score)
        updated = []
        for triplet, result in zip(needs_mining, results):
            if result.negatives:
                updated.append(dataclasses.replace(
                    triplet, negative=result.negatives[0], difficulty="hard",
                    metadata={**triplet.metadata, "negative_score": result.negative_scores[0]}))
            else:
                updated.append(triplet)
        return complete + updated

    def clear_index(self) -> None:
        """Drop the index and the document pool."""
        self._index = None
        self._document_pool = []
        self._document_embeddings = None
        logger.info("Index cleared")

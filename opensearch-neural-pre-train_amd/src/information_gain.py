"""Information-gain filtering of synonym / expansion pairs in embedding space, on one GPU.

The reference's module of the same name (ref:src/information_gain.py) scores a pair source -> target as

    IG = H(target) - H(target | source)

with both entropies Kozachenko-Leonenko k-nearest-neighbour estimates: H(target) against the whole corpus of term
embeddings, H(target | source) against the ``k_neighborhood`` corpus rows nearest to the source.  A low IG marks a trivial
expansion (a truncation, a case change).  Public names and defaults are the reference's; the distance work -- a float64
cdist against the corpus and one argsort per pair there -- runs in snx.infogain (csrc/infogain.hip), the formulas over one
value per pair in float64 numpy.  No scipy: psi at an integer is -gamma + sum_{i<k} 1/i, and ln Gamma is snx.infogain.log_gamma, which has gammaln's bits.

Where results can differ from the reference's: a distance is the float64 fma chain of include/snx.h "exact L2 nearest
neighbours", so a value can sit on the other side of an fp32 rounding boundary (one fp32 ulp of an entropy); and when two
corpus rows are equally far from a source at the neighbourhood boundary the reference keeps whichever numpy's unstable
argsort puts first, while here the lowest corpus id wins.  ``use_faiss`` is accepted and changes nothing: the GPU index
answers ``get_knn_faiss`` in IndexFlatL2's convention."""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Dict, List, Literal, Optional, Sequence, Tuple, Union

import numpy as np

logger = logging.getLogger(__name__)

_NORM_EPS = 1e-10


@dataclass
class InformationGainResult:
    """The score of one pair and the filter's decision."""
    source: str
    target: str
    information_gain: float
    target_entropy: float
    conditional_entropy: float
    similarity: float
    is_filtered: bool
    filter_reason: Optional[str] = None


@dataclass
class InformationGainConfig:
    k_entropy: int = 10                # k of the entropy estimate
    k_neighborhood: int = 50           # corpus rows that make a source's neighbourhood
    percentile_threshold: float = 10.0  # the bottom percentile is filtered
    min_ig_absolute: float = 0.0       # hard floor on IG
    batch_size: int = 1000             # pairs per device batch
    use_faiss: bool = True             # accepted; the GPU index serves either way
    normalize_embeddings: bool = True  # L2-normalise on the host first
    verbose: bool = False


def _normalize_rows(x: np.ndarray) -> np.ndarray:
    """x / (norm(x, axis=1, keepdims=True) + 1e-10) in fp32 numpy, exactly as the reference writes it: numpy's pairwise
    fp32 sum defines the operand the device sees."""
    return x / (np.linalg.norm(x, axis=1, keepdims=True) + _NORM_EPS)


def _normalize_vector(x: np.ndarray) -> np.ndarray:
    return x / (np.linalg.norm(x) + _NORM_EPS)


def _f32(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x), dtype=np.float32)


def _log_volume_unit_ball(d: int) -> float:
    """ln V_d, the log volume of the unit ball in d dimensions (the reference's private name)."""
    from snx.infogain import log_volume_unit_ball
    return log_volume_unit_ball(d)


# ------------------------------------------------------------------------------------------------ entropies
def knn_entropy_kl(query_embedding, reference_embeddings, k: int = 10, eps: float = 1e-10, *, index=None) -> float:
    """KL entropy (nats) of one point against a reference set: k = min(k, n - 1), 0.0 when k < 1; rho is the k-th nearest
    distance, skipping the nearest when it is below ``eps`` (the query is in the set).  ``index``: an ``L2Index`` of
    ``reference_embeddings`` built earlier."""
    from snx.infogain import K_MAX, L2Index, kl_entropy
    ref = _f32(reference_embeddings)
    n_ref, d = ref.shape
    k = min(int(k), n_ref - 1)
    if k < 1:
        return 0.0
    if k + 1 > K_MAX:
        raise ValueError(f"knn_entropy_kl: k must be below {K_MAX}")
    index = index or L2Index(ref)
    d2, _ = index.knn(_f32(np.atleast_2d(query_embedding)), k + 1)
    dist = np.sqrt(d2[0].cpu().numpy())
    rho = dist[k] if dist[0] < eps else dist[k - 1]
    return float(kl_entropy(max(float(rho), eps), d, n_ref, k))


def knn_entropy_batch(query_embeddings, reference_embeddings, k: int = 10, eps: float = 1e-10, *, index=None) -> np.ndarray:
    """KL entropy of every query against the reference set -> fp32 [m]; rho is the distance at 0-based position
    min(k, n - 1) of the ascending distances (no self-exclusion, as the reference's batch form)."""
    from snx.infogain import K_MAX, L2Index, kl_entropy
    q, ref = _f32(query_embeddings), _f32(reference_embeddings)
    n_ref, d = ref.shape
    k = min(int(k), n_ref - 1)
    if k < 1:
        return np.zeros(q.shape[0], dtype=np.float32)
    if k + 1 > K_MAX:
        raise ValueError(f"knn_entropy_batch: k must be below {K_MAX}")
    index = index or L2Index(ref)
    d2, _ = index.knn(q, k + 1)
    rho = np.maximum(np.sqrt(d2[:, k].cpu().numpy()), eps)
    return kl_entropy(rho, d, n_ref, k).astype(np.float32)


def get_knn_indices(query_embedding, reference_embeddings, k: int, *, index=None) -> np.ndarray:
    """Corpus ids of the min(k, n) nearest rows, nearest first, int64."""
    from snx.infogain import L2Index
    ref = _f32(reference_embeddings)
    k = min(int(k), ref.shape[0])
    if k < 1:
        return np.zeros(0, dtype=np.int64)
    index = index or L2Index(ref)
    _, ids = index.knn(_f32(np.atleast_2d(query_embedding)), k)
    return ids[0].cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------------ information gain
def compute_information_gain(source_embedding, target_embedding, corpus_embeddings,
                             config: Optional[InformationGainConfig] = None) -> Tuple[float, float, float]:
    """(IG, H(target), H(target | source)) of one pair as Python floats.  Both entropies follow ``knn_entropy_kl``'s
    self-exclusion rule, the marginal one too, as the reference's single-pair path does."""
    from snx.infogain import L2Index
    config = config or InformationGainConfig()
    src, tgt, corpus = _f32(source_embedding).reshape(-1), _f32(target_embedding).reshape(-1), _f32(corpus_embeddings)
    if config.normalize_embeddings:
        src, tgt, corpus = _normalize_vector(src), _normalize_vector(tgt), _normalize_rows(corpus)
    index = L2Index(corpus)
    target_entropy = knn_entropy_kl(tgt, corpus, k=config.k_entropy, index=index)
    neighbours = get_knn_indices(src, corpus, config.k_neighborhood, index=index)
    conditional_entropy = knn_entropy_kl(tgt, corpus[neighbours], k=min(config.k_entropy, config.k_neighborhood - 1))
    return target_entropy - conditional_entropy, target_entropy, conditional_entropy


def compute_information_gain_batch(source_embeddings, target_embeddings, corpus_embeddings=None,
                                   config: Optional[InformationGainConfig] = None, *, index=None
                                   ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(information_gains, target_entropies, conditional_entropies), fp32 [m].  ``index``: an ``L2Index`` of the corpus as
    the scores should see it (already normalised when the configuration says so); ``corpus_embeddings`` is then unused."""
    from snx.infogain import L2Index, information_gain
    config = config or InformationGainConfig()
    src, tgt = _f32(source_embeddings), _f32(target_embeddings)
    if config.normalize_embeddings:
        src, tgt = _normalize_rows(src), _normalize_rows(tgt)
    if index is None:
        corpus = _f32(corpus_embeddings)
        index = L2Index(_normalize_rows(corpus) if config.normalize_embeddings else corpus)
    logger.info("Computing distances for %d pairs against %d corpus embeddings", src.shape[0], index.n)
    return information_gain(index, src, tgt, config.k_entropy, config.k_neighborhood,
                            max(1, min(int(config.batch_size), max(1, src.shape[0]))))


# ------------------------------------------------------------------------------------------------ thresholds
def compute_percentile_threshold(scores, percentile: float = 10.0) -> float:
    return float(np.percentile(scores, percentile))


def _otsu_threshold(scores, n_bins: int = 256) -> float:
    """Otsu over a histogram of ``n_bins``: the bin centre that maximises the between-class variance w0 w1 (mu0 - mu1)^2
    over the cuts 1 .. n_bins - 2, the first maximum winning; the first centre when no cut separates anything."""
    hist, edges = np.histogram(scores, bins=n_bins)
    centers = (edges[:-1] + edges[1:]) / 2
    total = hist.sum()
    if total == 0:
        return float(np.median(scores))
    below = np.cumsum(hist)
    weighted = np.cumsum(hist * centers)
    best, threshold = 0.0, centers[0]
    for i in range(1, n_bins - 1):
        w0 = below[i] / total
        w1 = 1 - w0
        if w0 <= 0 or w1 <= 0:
            continue
        mu0 = weighted[i] / below[i]
        mu1 = (weighted[-1] - weighted[i]) / (total - below[i])
        between = w0 * w1 * (mu0 - mu1) ** 2
        if between > best:
            best, threshold = between, centers[i]
    return float(threshold)


def compute_adaptive_threshold(scores, method: Literal["percentile", "otsu", "mad"] = "percentile",
                               percentile: float = 10.0, mad_multiplier: float = 2.0) -> float:
    """The filter threshold from the scores themselves: a percentile, Otsu's cut, or median - multiplier * MAD."""
    if method == "percentile":
        return compute_percentile_threshold(scores, percentile)
    if method == "otsu":
        return _otsu_threshold(scores)
    if method == "mad":
        median = np.median(scores)
        return float(median - mad_multiplier * np.median(np.abs(scores - median)))
    raise ValueError(f"Unknown thresholding method: {method}")


# ------------------------------------------------------------------------------------------------ the filter
Pair = Union[Tuple[str, str, float], Sequence]


def decide_pairs(pairs: Sequence[Pair], ig, h_t, h_c, threshold: float, config: InformationGainConfig,
            method: str) -> List[InformationGainResult]:
    results = []
    for i, (source, target, similarity) in enumerate(pairs):
        below_floor = bool(ig[i] < config.min_ig_absolute)
        filtered = bool(ig[i] < threshold) or below_floor
        reason = None
        if below_floor:
            reason = f"Below absolute threshold ({config.min_ig_absolute})"
        elif filtered and method == "percentile":
            reason = f"Below percentile threshold (p{config.percentile_threshold}={threshold:.4f})"
        elif filtered:
            reason = f"Below {method} threshold ({threshold:.4f})"
        results.append(InformationGainResult(source=source, target=target, information_gain=float(ig[i]),
                                             target_entropy=float(h_t[i]), conditional_entropy=float(h_c[i]),
                                             similarity=similarity, is_filtered=filtered, filter_reason=reason))
    return results


def filter_synonym_pairs(pairs: Sequence[Pair], source_embeddings, target_embeddings, corpus_embeddings=None,
                         config: Optional[InformationGainConfig] = None, *, index=None,
                         method: str = "percentile") -> List[InformationGainResult]:
    """Score ``pairs`` (source, target, similarity) and mark those with ``ig < threshold or ig < min_ig_absolute``; the
    threshold is the ``percentile_threshold`` percentile of the scores (``method``: ``otsu`` or ``mad`` instead)."""
    config = config or InformationGainConfig()
    ig, h_t, h_c = compute_information_gain_batch(source_embeddings, target_embeddings, corpus_embeddings, config,
                                                  index=index)
    if len(pairs) != ig.shape[0]:
        raise ValueError("filter_synonym_pairs: one embedding row per pair")
    if not len(pairs):
        return []
    threshold = compute_adaptive_threshold(ig, method=method, percentile=config.percentile_threshold)
    logger.info("IG statistics: min=%.4f, max=%.4f, mean=%.4f, std=%.4f; threshold %.4f", ig.min(), ig.max(), ig.mean(),
                ig.std(), threshold)
    results = decide_pairs(pairs, ig, h_t, h_c, threshold, config, method)
    logger.info("Filtered %d/%d pairs", sum(r.is_filtered for r in results), len(results))
    return results


class InformationGainFilter:
    """The filter with the corpus held on the GPU:

        f = InformationGainFilter(config).fit(corpus_embeddings, term_to_idx)
        results = f.filter_pairs(pairs, source_embeddings, target_embeddings)

    ``fit`` normalises (when configured) and uploads once.  As in the reference, ``corpus_embeddings`` keeps the rows
    normalised once while the scoring path normalises what ``fit`` kept a second time (ref:information_gain.py:594-597,
    648-654, 325-326): the index holds those rows, so ``filter_pairs`` sees the reference's bits."""

    def __init__(self, config: Optional[InformationGainConfig] = None):
        self.config = config or InformationGainConfig()
        self.corpus_embeddings: Optional[np.ndarray] = None
        self.term_to_idx: Optional[Dict[str, int]] = None
        self.is_fitted = False
        self._index = None             # the rows the scores see
        self._searched = None          # the rows get_knn_faiss searches, uploaded at the first call

    def fit(self, corpus_embeddings, term_to_idx: Optional[Dict[str, int]] = None) -> "InformationGainFilter":
        from snx.infogain import L2Index
        self.corpus_embeddings = _f32(corpus_embeddings)
        self.term_to_idx = term_to_idx
        scored = self.corpus_embeddings
        if self.config.normalize_embeddings:
            self.corpus_embeddings = _normalize_rows(self.corpus_embeddings)
            scored = _normalize_rows(self.corpus_embeddings)
        self._index = L2Index(scored)
        self._searched = None if self.config.normalize_embeddings else self._index
        self.is_fitted = True
        return self

    def _need_fit(self) -> None:
        if not self.is_fitted:
            raise RuntimeError("Filter not fitted. Call fit() first.")

    def get_knn_faiss(self, query, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """(squared distances fp32 [k], corpus ids int64 [k]) of one query against the rows ``fit`` kept, nearest first:
        IndexFlatL2's convention (-1 and +inf past the corpus)."""
        self._need_fit()
        from snx.infogain import L2Index
        if self._searched is None:                           # corpus_embeddings: normalised once, as FAISS held them
            self._searched = L2Index(self.corpus_embeddings)
        d2, ids = self._searched.knn(_f32(np.atleast_2d(query)), int(k))
        return d2[0].cpu().numpy().astype(np.float32), ids[0].cpu().numpy().astype(np.int64)

    def filter_pairs(self, pairs: Sequence[Pair], source_embeddings, target_embeddings,
                     method: str = "percentile") -> List[InformationGainResult]:
        self._need_fit()
        return filter_synonym_pairs(pairs, source_embeddings, target_embeddings, None, self.config, index=self._index,
                                    method=method)

    def compute_threshold(self, ig_scores, method: Literal["percentile", "otsu", "mad"] = "percentile") -> float:
        return compute_adaptive_threshold(ig_scores, method=method, percentile=self.config.percentile_threshold)


def analyze_ig_distribution(results: Sequence[InformationGainResult]) -> Dict[str, Union[float, int]]:
    """Counts and float64 statistics of the scores, with the filtered and the kept ones apart when there are any."""
    ig = np.array([r.information_gain for r in results])
    flags = np.array([r.is_filtered for r in results], dtype=bool)
    stats: Dict[str, Union[float, int]] = {"total_pairs": len(results), "filtered_pairs": int(flags.sum()),
                                           "kept_pairs": int((~flags).sum())}
    stats.update(ig_mean=float(ig.mean()), ig_std=float(ig.std()), ig_min=float(ig.min()), ig_max=float(ig.max()),
                 ig_median=float(np.median(ig)))
    for p in (10, 25, 75, 90):
        stats[f"ig_p{p}"] = float(np.percentile(ig, p))
    if flags.any():
        stats["filtered_ig_mean"] = float(ig[flags].mean())
        stats["filtered_ig_max"] = float(ig[flags].max())
    if (~flags).any():
        stats["kept_ig_mean"] = float(ig[~flags].mean())
        stats["kept_ig_min"] = float(ig[~flags].min())
    return stats

"""PMI with Laplace and context-distribution smoothing (ref:src/pmi/pmi_calculator.py) with the per-cell and per-pair
arithmetic on the GPU (snx.cooc.pmi_values / pmi_pairs, float64).  The V marginals and the total are numpy's, as in the
reference, so they agree with it to the bit; one pair (``compute_pmi``) is a host lookup and needs no kernel."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import numpy as np


@dataclass
class PMIConfig:
    laplace_smoothing: float = 1.0
    context_smoothing_alpha: float = 0.75
    use_ppmi: bool = True
    log_base: float = 2.0
    min_cooccurrence: int = 1


def _triple(matrix) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A scipy matrix, a snx.cooc.CooccurrenceCSR or a (data, indices, indptr) triple -> canonical host triple."""
    if hasattr(matrix, "numpy") and hasattr(matrix, "total_windows"):
        data, indices, indptr = matrix.numpy()
    elif isinstance(matrix, tuple):
        data, indices, indptr = matrix
    else:
        m = matrix.tocsr()
        if not m.has_sorted_indices:
            m = m.sorted_indices()
        data, indices, indptr = m.data, m.indices, m.indptr
    return np.asarray(data, dtype=np.float32), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int64)


def matrix_sum(data: np.ndarray, indptr: np.ndarray) -> float:
    """``float(matrix.sum())`` as scipy evaluates it for a fp32 csr matrix: every row summed front to back in fp32, the
    row sums added by numpy in fp32.  Integer cells below 2^24 in all need no order: their sum is exact."""
    if not data.size:
        return 0.0
    exact = data.astype(np.float64)
    if exact.sum() < 2 ** 24 and not (exact != np.floor(exact)).any():
        return float(exact.sum())
    rows = np.zeros(indptr.size - 1, dtype=np.float32)
    for r in np.flatnonzero(indptr[1:] > indptr[:-1]):
        rows[r] = np.cumsum(data[indptr[r]:indptr[r + 1]], dtype=np.float32)[-1]
    return float(rows.sum(dtype=np.float32))


class PMICalculator:
    """PMI of term pairs from co-occurrence statistics; the reference's class.  ``cooccurrence_matrix``: a scipy sparse
    matrix, a snx.cooc.CooccurrenceCSR, or the numpy triple of ``CooccurrenceMatrixBuilder.cooccurrence_csr()``."""

    def __init__(self, cooccurrence_matrix, term_frequencies: Dict[str, int], vocabulary: Dict[str, int],
                 total_windows: int, config: Optional[PMIConfig] = None, device="cuda"):
        self.cooc_matrix = cooccurrence_matrix
        self.term_freq = term_frequencies
        self.vocab = vocabulary
        self.reverse_vocab = {idx: term for term, idx in vocabulary.items()}
        self.total_windows = total_windows
        self.config = config or PMIConfig()
        self.device = device
        self._host = _triple(cooccurrence_matrix)
        on_device = hasattr(cooccurrence_matrix, "numpy") and hasattr(cooccurrence_matrix, "total_windows")
        self._device_csr = cooccurrence_matrix if on_device else None
        self._compute_marginals()

    def _compute_marginals(self) -> None:
        V = len(self.vocab)
        alpha = self.config.context_smoothing_alpha
        freqs = np.zeros(V, dtype=np.float64)
        if alpha != 1.0:
            for term, idx in self.vocab.items():
                freqs[idx] = self.term_freq.get(term, 0)
            smoothed = np.power(freqs + 1e-10, alpha)
            self._marginal_probs = smoothed / smoothed.sum()
        else:
            total_freq = sum(self.term_freq.values())
            for term, idx in self.vocab.items():
                freqs[idx] = self.term_freq.get(term, 0) / total_freq
            self._marginal_probs = freqs
        self._total_cooc = matrix_sum(self._host[0], self._host[2])
        if self._total_cooc == 0:
            self._total_cooc = 1.0

    def _none(self) -> float:
        return 0.0 if self.config.use_ppmi else float("-inf")

    def _csr_on_device(self):
        if self._device_csr is None:
            import torch
            from snx import cooc
            from snx.retrieval._common import cuda_device
            dev = cuda_device(self.device)
            data, indices, indptr = self._host
            V = len(self.vocab)
            self._device_csr = cooc.CooccurrenceCSR(torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev),
                                                    torch.from_numpy(data).to(dev), None, int(self.total_windows), (V, V))
        return self._device_csr

    def compute_pmi(self, term1: str, term2: str) -> float:
        i, j = self.vocab.get(term1), self.vocab.get(term2)
        if i is None or j is None:
            return self._none()
        return self._compute_pmi_by_index(i, j)

    def _compute_pmi_by_index(self, idx1: int, idx2: int) -> float:
        from src.pmi.cooccurrence import csr_cell
        cfg = self.config
        count = float(csr_cell(self._host, idx1, idx2))
        if count < cfg.min_cooccurrence:
            if cfg.laplace_smoothing > 0:
                count = cfg.laplace_smoothing
            else:
                return self._none()
        k, V = cfg.laplace_smoothing, len(self.vocab)
        p_joint = (count + k) / (self._total_cooc + k * V * V)
        p1, p2 = self._marginal_probs[idx1], self._marginal_probs[idx2]
        if p1 == 0 or p2 == 0:
            return self._none()
        ratio = p_joint / (p1 * p2)
        if cfg.log_base == 2.0:
            pmi = np.log2(ratio)
        elif cfg.log_base == np.e:
            pmi = np.log(ratio)
        else:
            pmi = np.log(ratio) / np.log(cfg.log_base)
        if cfg.use_ppmi:
            pmi = max(0.0, pmi)
        return float(pmi)

    def compute_pmi_batch(self, term_pairs: List[Tuple[str, str]], show_progress: bool = True) -> List[float]:
        from snx import cooc
        if not len(term_pairs):
            return []
        get = self.vocab.get
        rows = np.fromiter((get(a, -1) for a, _ in term_pairs), dtype=np.int64, count=len(term_pairs))
        cols = np.fromiter((get(b, -1) for _, b in term_pairs), dtype=np.int64, count=len(term_pairs))
        if len(self.vocab) == 0:
            return [self._none()] * len(term_pairs)
        out = cooc.pmi_pairs(self._csr_on_device(), rows, cols, self._marginal_probs, self._total_cooc, self.config)
        return out.cpu().tolist()

    def compute_pmi_matrix(self):
        """The PMI of every stored cell as a fp32 matrix with the count matrix's structure (-inf stored as 0.0): a scipy
        csr_matrix, or the numpy triple when scipy does not import."""
        from snx import cooc
        _, indices, indptr = self._host
        V = len(self.vocab)
        if indices.size:
            values = cooc.pmi_values(self._csr_on_device(), self._marginal_probs, self._total_cooc, self.config)
            values = values.cpu().numpy()
            values[np.isinf(values)] = 0.0
        else:
            values = np.zeros(0, dtype=np.float64)
        data = values.astype(np.float32)
        try:
            from scipy import sparse
        except ImportError:
            return data, indices, indptr
        return sparse.csr_matrix((data, indices, indptr), shape=(V, V))

    def get_pmi_percentile(self, term_pairs: List[Tuple[str, str]], percentile: float) -> float:
        scores = [s for s in self.compute_pmi_batch(term_pairs, show_progress=False) if not np.isinf(s)]
        return float(np.percentile(scores, percentile)) if scores else 0.0

    def filter_by_pmi_threshold(self, term_pairs: List[Tuple[str, str]], threshold: Optional[float] = None,
                                percentile: Optional[float] = None, show_progress: bool = True
                                ) -> Tuple[List[Tuple[str, str]], List[float]]:
        if threshold is None and percentile is None:
            raise ValueError("Either threshold or percentile must be provided")
        scores = self.compute_pmi_batch(term_pairs, show_progress)
        if threshold is None:
            finite = [s for s in scores if not np.isinf(s)]
            threshold = np.percentile(finite, percentile) if finite else 0.0
        kept = [(p, s) for p, s in zip(term_pairs, scores) if s >= threshold]
        return [p for p, _ in kept], [s for _, s in kept]

    def get_stats(self) -> Dict[str, Union[int, float]]:
        return {"vocab_size": len(self.vocab), "total_windows": self.total_windows,
                "total_cooccurrences": self._total_cooc, "laplace_smoothing": self.config.laplace_smoothing,
                "context_smoothing_alpha": self.config.context_smoothing_alpha, "use_ppmi": self.config.use_ppmi}


class PPMICalculator(PMICalculator):
    """Positive PMI in bits: PMICalculator with ``use_ppmi=True, log_base=2``."""

    def __init__(self, cooccurrence_matrix, term_frequencies: Dict[str, int], vocabulary: Dict[str, int],
                 total_windows: int, laplace_smoothing: float = 1.0, context_smoothing_alpha: float = 0.75, device="cuda"):
        super().__init__(cooccurrence_matrix, term_frequencies, vocabulary, total_windows,
                         PMIConfig(laplace_smoothing=laplace_smoothing, context_smoothing_alpha=context_smoothing_alpha,
                                   use_ppmi=True, log_base=2.0), device)


def compute_npmi(pmi_score: float, p_joint: float, log_base: float = 2.0) -> float:
    """Normalised PMI: ``pmi / -log(p_joint)``, 0.0 where that is undefined."""
    if p_joint <= 0:
        return 0.0
    h_joint = -np.log2(p_joint) if log_base == 2.0 else -np.log(p_joint) / np.log(log_base)
    return 0.0 if h_joint == 0 else pmi_score / h_joint

"""Co-occurrence matrix construction (ref:src/pmi/cooccurrence.py) with the counting on the GPU.

The text work stays on the host: tokenising, interning, the vocabulary cut, splitting documents into windows
(snx.cooc).  The windows then go to the device as rows of vocabulary ids (-1 for a token outside the vocabulary) and
``snx.cooc.cooccurrence`` counts them.  The vocabulary and the frequencies come from the tokens of the WHOLE document, the
windows from the tokens of EACH sentence or paragraph, as in the reference: a term such as ``a.b`` (whitespace tokens) is
in the vocabulary, yet sentence mode never sees it."""
import json
from dataclasses import dataclass
from enum import Enum
from pathlib import Path
from typing import Callable, Dict, List, Optional, Tuple, Union

import numpy as np

from snx import cooc

FILES = ("cooccurrence_matrix.npz", "vocabulary.json", "term_frequencies.json", "config.json", "stats.json")


class WindowType(Enum):
    SENTENCE = "sentence"
    PARAGRAPH = "paragraph"
    SLIDING = "sliding"


@dataclass
class CooccurrenceConfig:
    window_type: WindowType = WindowType.SENTENCE
    window_size: int = 10
    min_term_freq: int = 5
    max_vocab_size: int = 120000
    symmetric: bool = True
    normalize: bool = False


@dataclass
class CooccurrenceStats:
    vocab_size: int = 0
    total_documents: int = 0
    total_windows: int = 0
    total_cooccurrences: int = 0
    sparsity: float = 0.0


def _scipy_sparse():
    try:
        from scipy import sparse
    except ImportError:
        return None
    return sparse


class CooccurrenceMatrixBuilder:
    """Builds the sparse co-occurrence matrix of a corpus; the reference's class, counted by the kernels.

        builder = CooccurrenceMatrixBuilder(config).fit(texts)
        matrix = builder.get_cooccurrence_matrix()        # scipy csr_matrix (fp32)
        data, indices, indptr = builder.cooccurrence_csr()   # the same without scipy
    """

    def __init__(self, config: Optional[CooccurrenceConfig] = None, device="cuda",
                 max_records: int = cooc.DEFAULT_MAX_RECORDS):
        self.config = config or CooccurrenceConfig()
        self.device = device
        self.max_records = max_records
        self._vocab: Dict[str, int] = {}
        self._reverse_vocab: Dict[int, str] = {}
        self._term_freq: Dict[str, int] = {}
        self._doc_freq: Dict[str, int] = {}
        self._csr: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]] = None      # (data, indices, indptr)
        self._counts: Optional[np.ndarray] = None
        self._device_csr = None
        self._stats = CooccurrenceStats()

    # ---------------------------------------------------------------------------------------------- host half
    def _tokenize(self, text: str, tokenizer: Optional[Callable]) -> List[str]:
        return tokenizer(text) if tokenizer is not None else text.split()

    def prepare(self, documents: List[str], tokenizer: Optional[Callable] = None):
        """The host half of ``fit`` (no GPU): vocabulary and frequencies, then the windows as id rows.
        -> (ptr int64, ids int32 vocabulary ids or -1, window_size or None); sets the vocabulary and frequency tables."""
        cfg = self.config
        interner = cooc.Interner()
        doc_ids = [interner.intern(self._tokenize(doc, tokenizer)) for doc in documents]
        n_terms = len(interner)
        flat = np.fromiter((i for d in doc_ids for i in d), dtype=np.int64)
        tf = np.bincount(flat, minlength=n_terms) if n_terms else np.zeros(0, np.int64)
        seen = np.fromiter((i for d in doc_ids for i in set(d)), dtype=np.int64)
        df = np.bincount(seen, minlength=n_terms) if n_terms else np.zeros(0, np.int64)
        new_id = cooc.select_vocabulary(tf, cfg.min_term_freq, cfg.max_vocab_size)
        terms = interner.terms[:n_terms]
        kept = np.flatnonzero(new_id >= 0)
        kept = kept[np.argsort(new_id[kept])]
        self._vocab = {terms[o]: i for i, o in enumerate(kept)}
        self._reverse_vocab = {i: t for t, i in self._vocab.items()}
        self._term_freq = {terms[i]: int(tf[i]) for i in range(n_terms)}
        self._doc_freq = {terms[i]: int(df[i]) for i in range(n_terms)}
        self._stats = CooccurrenceStats(vocab_size=len(self._vocab), total_documents=len(documents))
        if cfg.window_type == WindowType.SLIDING:
            rows, w = doc_ids, int(cfg.window_size)
        else:
            split = cooc.sentence_windows if cfg.window_type == WindowType.SENTENCE else cooc.paragraph_windows
            rows = [interner.intern(self._tokenize(piece, tokenizer)) for doc in documents for piece in split(doc)]
            w = None
        ptr, old = cooc.id_rows(rows)
        table = np.full(len(interner), -1, dtype=np.int64)    # window-only tokens lie past n_terms: outside the vocabulary
        table[:n_terms] = new_id
        ids = table[old].astype(np.int32) if old.size else old
        return ptr, ids, w

    def fit(self, documents: List[str], tokenizer: Optional[Callable] = None, show_progress: bool = True
            ) -> "CooccurrenceMatrixBuilder":
        ptr, ids, w = self.prepare(documents, tokenizer)
        self._csr = self._counts = self._device_csr = None
        V = len(self._vocab)
        if V == 0:                                            # as the reference: no matrix, no window counted
            return self
        csr = cooc.cooccurrence(ptr, ids, V, window_size=w, symmetric=self.config.symmetric,
                                normalize=self.config.normalize, max_records=self.max_records, device=self.device)
        self._device_csr = csr
        self._csr = csr.numpy()
        self._counts = None if csr.counts is None else csr.counts.cpu().numpy()
        self._stats.total_windows = csr.total_windows
        self._stats.total_cooccurrences = csr.nnz
        self._stats.sparsity = 1.0 - csr.nnz / (V * V)
        return self

    # ---------------------------------------------------------------------------------------------- results
    def cooccurrence_csr(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(data fp32, indices int32, indptr int64) of the matrix; works without scipy."""
        if self._csr is None:
            raise ValueError("Matrix not built. Call fit() first.")
        return self._csr

    def cooccurrence_counts(self) -> Optional[np.ndarray]:
        """The exact int64 counts beside ``cooccurrence_csr()``'s data; None for a normalised or loaded matrix."""
        return self._counts

    def set_cooccurrence_csr(self, data, indices, indptr, total_windows: int) -> None:
        """Adopt a matrix over the current vocabulary that was counted elsewhere (indices ascending per row)."""
        V = len(self._vocab)
        data, indices = np.asarray(data, dtype=np.float32), np.asarray(indices, dtype=np.int32)
        indptr = np.asarray(indptr, dtype=np.int64)
        if indptr.shape != (V + 1,) or data.shape != indices.shape or data.ndim != 1 or indptr[0] != 0 or \
                indptr[-1] != data.size or (indptr[1:] < indptr[:-1]).any():
            raise ValueError(f"set_cooccurrence_csr: a csr triple over {V} terms is expected")
        self._csr, self._counts, self._device_csr = (data, indices, indptr), None, None
        self._stats.total_windows = int(total_windows)
        self._stats.total_cooccurrences = int(data.size)
        self._stats.sparsity = 1.0 - data.size / (V * V) if V else 0.0

    def device_csr(self):
        """The snx.cooc.CooccurrenceCSR of the last ``fit`` (None after ``load``)."""
        return self._device_csr

    def get_cooccurrence_matrix(self):
        data, indices, indptr = self.cooccurrence_csr()
        sparse = _scipy_sparse()
        if sparse is None:
            raise ImportError("get_cooccurrence_matrix returns a scipy.sparse.csr_matrix and scipy does not import; "
                              "cooccurrence_csr() returns the same matrix as numpy arrays")
        V = len(self._vocab)
        return sparse.csr_matrix((data, indices, indptr), shape=(V, V))

    def get_term_frequencies(self) -> Dict[str, int]:
        return {term: self._term_freq.get(term, 0) for term in self._vocab}

    def get_document_frequencies(self) -> Dict[str, int]:
        return {term: self._doc_freq.get(term, 0) for term in self._vocab}

    def get_vocabulary(self) -> Dict[str, int]:
        return self._vocab.copy()

    def get_term_by_index(self, index: int) -> Optional[str]:
        return self._reverse_vocab.get(index)

    def get_index_by_term(self, term: str) -> Optional[int]:
        return self._vocab.get(term)

    def get_cooccurrence_count(self, term1: str, term2: str) -> float:
        if self._csr is None:
            return 0.0
        i, j = self._vocab.get(term1), self._vocab.get(term2)
        if i is None or j is None:
            return 0.0
        return float(csr_cell(self._csr, i, j))

    def get_stats(self) -> CooccurrenceStats:
        return self._stats

    # ---------------------------------------------------------------------------------------------- files
    def save(self, path: Union[str, Path]) -> None:
        """The reference's five files.  The matrix is written with numpy in the layout of ``scipy.sparse.save_npz``."""
        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        if self._csr is not None:
            data, indices, indptr = self._csr
            V = len(self._vocab)
            np.savez_compressed(path / FILES[0], indices=indices.astype(np.int32), indptr=indptr.astype(np.int32)
                                if indptr[-1] < 2 ** 31 else indptr, format="csr".encode("ascii"),
                                shape=np.array([V, V], dtype=np.int64), data=data)
        cfg, st = self.config, self._stats
        for name, obj, ascii_ in (
                (FILES[1], self._vocab, False),
                (FILES[2], {t: self._term_freq.get(t, 0) for t in self._vocab}, False),
                (FILES[3], {"window_type": cfg.window_type.value, "window_size": cfg.window_size,
                            "min_term_freq": cfg.min_term_freq, "max_vocab_size": cfg.max_vocab_size,
                            "symmetric": cfg.symmetric, "normalize": cfg.normalize}, True),
                (FILES[4], {"vocab_size": st.vocab_size, "total_documents": st.total_documents,
                            "total_windows": st.total_windows, "total_cooccurrences": st.total_cooccurrences,
                            "sparsity": st.sparsity}, True)):
            with open(path / name, "w", encoding="utf-8") as f:
                json.dump(obj, f, ensure_ascii=ascii_, indent=2)

    @classmethod
    def load(cls, path: Union[str, Path]) -> "CooccurrenceMatrixBuilder":
        path = Path(path)
        with open(path / FILES[3], "r", encoding="utf-8") as f:
            c = json.load(f)
        builder = cls(CooccurrenceConfig(window_type=WindowType(c["window_type"]), window_size=c["window_size"],
                                         min_term_freq=c["min_term_freq"], max_vocab_size=c["max_vocab_size"],
                                         symmetric=c["symmetric"], normalize=c["normalize"]))
        with open(path / FILES[1], "r", encoding="utf-8") as f:
            builder._vocab = json.load(f)
        builder._reverse_vocab = {i: t for t, i in builder._vocab.items()}
        with open(path / FILES[2], "r", encoding="utf-8") as f:
            builder._term_freq = json.load(f)
        with np.load(path / FILES[0]) as z:
            fmt = z["format"].item()
            if (fmt.decode() if isinstance(fmt, bytes) else fmt) != "csr":
                raise ValueError(f"{path / FILES[0]}: a csr matrix is expected")
            builder._csr = (z["data"].astype(np.float32), z["indices"].astype(np.int32), z["indptr"].astype(np.int64))
        with open(path / FILES[4], "r", encoding="utf-8") as f:
            builder._stats = CooccurrenceStats(**json.load(f))
        return builder


def csr_cell(csr: Tuple[np.ndarray, np.ndarray, np.ndarray], i: int, j: int):
    """Cell (i, j) of a (data, indices ascending per row, indptr) triple; 0 when it is not stored."""
    data, indices, indptr = csr
    r0, r1 = int(indptr[i]), int(indptr[i + 1])
    p = r0 + int(np.searchsorted(indices[r0:r1], j))
    return data[p] if p < r1 and indices[p] == j else data.dtype.type(0)

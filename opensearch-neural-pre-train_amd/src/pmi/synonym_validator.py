"""Synonym validation by PMI (ref:src/pmi/synonym_validator.py): expansion pairs proposed by embedding similarity are
kept only when the corpus supports them.  Host logic over ``compute_pmi_batch``: any object with ``.vocab`` and
``.compute_pmi_batch(term_pairs, show_progress)`` serves as the calculator."""
import json
from dataclasses import dataclass, field
from enum import Enum
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Set, Tuple, Union

import numpy as np

from src.pmi.cooccurrence import CooccurrenceConfig, CooccurrenceMatrixBuilder
from src.pmi.pmi_calculator import PMICalculator, PMIConfig


class OOVStrategy(Enum):
    REMOVE = "remove"                  # a pair with a term outside the vocabulary is invalid
    KEEP = "keep"                      # it is valid without a PMI test
    SMOOTH = "smooth"                  # it is valid with the neutral score 0


@dataclass
class SynonymPair:
    source: str
    target: str
    embedding_similarity: float = 0.0
    pmi_score: float = 0.0
    is_valid: bool = True
    category: str = ""
    oov_status: str = "both_in_vocab"  # or "source_oov", "target_oov", "both_oov"

    def to_dict(self) -> Dict[str, Any]:
        return {"source": self.source, "target": self.target, "embedding_similarity": float(self.embedding_similarity),
                "pmi_score": 0.0 if np.isinf(self.pmi_score) else float(self.pmi_score), "is_valid": bool(self.is_valid),
                "category": self.category, "oov_status": self.oov_status}


@dataclass
class ValidationConfig:
    pmi_percentile_threshold: float = 10.0
    pmi_absolute_threshold: Optional[float] = None
    min_embedding_similarity: float = 0.5
    oov_strategy: OOVStrategy = OOVStrategy.KEEP
    separate_bpe_validation: bool = True


@dataclass
class ValidationResult:
    total_pairs: int = 0
    valid_pairs: int = 0
    removed_pairs: int = 0
    oov_pairs: int = 0
    pmi_threshold: float = 0.0         # the reference never fills this in; ``SynonymValidator.thresholds`` has them
    stats: Dict[str, Any] = field(default_factory=dict)


def _ratio_table(pairs: List[SynonymPair], key: Callable[[SynonymPair], str]) -> Dict[str, Dict[str, Any]]:
    table: Dict[str, Dict[str, Any]] = {}
    for name in set(key(p) for p in pairs):
        group = [p for p in pairs if key(p) == name]
        valid = sum(1 for p in group if p.is_valid)
        table[name] = {"total": len(group), "valid": valid, "valid_ratio": valid / len(group) if group else 0}
    return table


class SynonymValidator:
    """validated_pairs, result = SynonymValidator(pmi_calculator, config).validate(pairs)

    ``thresholds`` holds the PMI threshold of every batch of the last ``validate``: "all", or "cluster" and "BPE" when
    BPE pairs are validated separately."""

    def __init__(self, pmi_calculator, config: Optional[ValidationConfig] = None):
        self.pmi_calc = pmi_calculator
        self.config = config or ValidationConfig()
        self._vocabulary = set(pmi_calculator.vocab.keys())
        self.thresholds: Dict[str, float] = {}

    def validate(self, pairs: List[Dict[str, Any]], show_progress: bool = True
                 ) -> Tuple[List[SynonymPair], ValidationResult]:
        result = ValidationResult(total_pairs=len(pairs))
        items = [self._create_synonym_pair(p) for p in pairs]
        self.thresholds = {}
        if self.config.separate_bpe_validation:
            validated = self._validate_batch([p for p in items if p.category != "BPE"], show_progress, "cluster") + \
                self._validate_batch([p for p in items if p.category == "BPE"], show_progress, "BPE")
        else:
            validated = self._validate_batch(items, show_progress, "all")
        result.valid_pairs = sum(1 for p in validated if p.is_valid)
        result.removed_pairs = result.total_pairs - result.valid_pairs
        result.oov_pairs = sum(1 for p in validated if p.oov_status != "both_in_vocab")
        result.stats = self._compute_validation_stats(validated)
        return validated, result

    def _create_synonym_pair(self, pair: Dict[str, Any]) -> SynonymPair:
        source, target = pair.get("source", ""), pair.get("target", "")
        s_in, t_in = source in self._vocabulary, target in self._vocabulary
        status = "both_in_vocab" if s_in and t_in else "both_oov" if not s_in and not t_in else \
            "source_oov" if not s_in else "target_oov"
        return SynonymPair(source=source, target=target, embedding_similarity=pair.get("similarity", 0.0), pmi_score=0.0,
                           is_valid=True, category=pair.get("category", ""), oov_status=status)

    def _validate_batch(self, pairs: List[SynonymPair], show_progress: bool, name: str = "all") -> List[SynonymPair]:
        if not pairs:
            return []
        scores = self.pmi_calc.compute_pmi_batch([(p.source, p.target) for p in pairs], show_progress)
        for pair, score in zip(pairs, scores):
            pair.pmi_score = score
        if self.config.pmi_absolute_threshold is not None:
            threshold = self.config.pmi_absolute_threshold
        else:                                                 # the percentile over in-vocabulary finite scores
            known = [p.pmi_score for p in pairs if p.oov_status == "both_in_vocab" and not np.isinf(p.pmi_score)]
            threshold = np.percentile(known, self.config.pmi_percentile_threshold) if known else 0.0
        self.thresholds[name] = float(threshold)
        for pair in pairs:
            pair.is_valid = self._is_pair_valid(pair, threshold)
        return pairs

    def _is_pair_valid(self, pair: SynonymPair, pmi_threshold: float) -> bool:
        if pair.embedding_similarity < self.config.min_embedding_similarity:
            return False
        if pair.oov_status != "both_in_vocab":
            if self.config.oov_strategy == OOVStrategy.REMOVE:
                return False
            if self.config.oov_strategy == OOVStrategy.SMOOTH:
                pair.pmi_score = 0.0
            return True
        if np.isinf(pair.pmi_score) and pair.pmi_score < 0:
            return False
        return bool(pair.pmi_score >= pmi_threshold)

    def _compute_validation_stats(self, pairs: List[SynonymPair]) -> Dict[str, Any]:
        valid = [p for p in pairs if p.is_valid]
        invalid = [p for p in pairs if not p.is_valid]
        stats: Dict[str, Any] = {"total": len(pairs), "valid": len(valid), "invalid": len(invalid),
                                 "by_category": _ratio_table(pairs, lambda p: p.category),
                                 "by_oov_status": _ratio_table(pairs, lambda p: p.oov_status), "pmi_stats": {}}
        for name, group, with_std in (("valid", valid, True), ("invalid", invalid, False)):
            scores = [p.pmi_score for p in group if not np.isinf(p.pmi_score)]
            if scores:
                entry = {"min": float(np.min(scores)), "max": float(np.max(scores)), "mean": float(np.mean(scores)),
                         "median": float(np.median(scores))}
                if with_std:
                    entry["std"] = float(np.std(scores))
                stats["pmi_stats"][name] = entry
        return stats

    def get_oov_terms(self, pairs: List[Dict[str, Any]]) -> Set[str]:
        terms = (p.get(side, "") for p in pairs for side in ("source", "target"))
        return {t for t in terms if t not in self._vocabulary}

    def save_validation_report(self, pairs: List[SynonymPair], result: ValidationResult, path: Union[str, Path]) -> None:
        """validated_pairs.jsonl, invalid_pairs.jsonl and validation_report.json under ``path``."""
        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        for name, keep in (("validated_pairs.jsonl", True), ("invalid_pairs.jsonl", False)):
            with open(path / name, "w", encoding="utf-8") as f:
                for pair in pairs:
                    if pair.is_valid == keep:
                        f.write(json.dumps(pair.to_dict(), ensure_ascii=False) + "\n")
        cfg = self.config
        report = {"total_pairs": result.total_pairs, "valid_pairs": result.valid_pairs,
                  "removed_pairs": result.removed_pairs, "oov_pairs": result.oov_pairs,
                  "pmi_threshold": result.pmi_threshold,
                  "validation_ratio": result.valid_pairs / result.total_pairs if result.total_pairs > 0 else 0,
                  "stats": result.stats,
                  "config": {"pmi_percentile_threshold": cfg.pmi_percentile_threshold,
                             "pmi_absolute_threshold": cfg.pmi_absolute_threshold,
                             "min_embedding_similarity": cfg.min_embedding_similarity,
                             "oov_strategy": cfg.oov_strategy.value,
                             "separate_bpe_validation": cfg.separate_bpe_validation}}
        with open(path / "validation_report.json", "w", encoding="utf-8") as f:
            json.dump(report, f, ensure_ascii=False, indent=2)


def create_pmi_pipeline(documents: List[str], tokenizer: Optional[Callable] = None,
                        cooc_config: Optional[CooccurrenceConfig] = None, pmi_config: Optional[PMIConfig] = None,
                        save_path: Optional[Union[str, Path]] = None, show_progress: bool = True, device="cuda"
                        ) -> Tuple[CooccurrenceMatrixBuilder, PMICalculator]:
    """Builder and calculator in one step; ``save_path`` also saves the builder's files."""
    builder = CooccurrenceMatrixBuilder(cooc_config or CooccurrenceConfig(), device=device)
    builder.fit(documents, tokenizer, show_progress)
    if save_path:
        builder.save(save_path)
    matrix = builder.device_csr()
    if matrix is None:
        raise ValueError("Matrix not built. Call fit() first.")
    calc = PMICalculator(cooccurrence_matrix=matrix, term_frequencies=builder.get_term_frequencies(),
                         vocabulary=builder.get_vocabulary(), total_windows=builder.get_stats().total_windows,
                         config=pmi_config or PMIConfig(), device=device)
    return builder, calc

"""Graded term-expansion evaluation (the reference's src/evaluation package) with the ranking positions and the gain folds
on the GPU (snx.expansion, csrc/expansion.hip): RankingMetrics, the judgment dataclasses and ModelComparison."""
from src.evaluation.ranking_metrics import (EvaluationDataset, EvaluationResult, GradedRelevance, ModelComparison,
                                            RankingMetrics, create_korean_legal_medical_eval_dataset)

__all__ = [
    "RankingMetrics", "GradedRelevance", "EvaluationDataset", "EvaluationResult", "ModelComparison",
    "create_korean_legal_medical_eval_dataset",
]

"""PMI synonym validation (the reference's src/pmi package) with the counting and the PMI arithmetic on the GPU
(snx.cooc, csrc/cooc.hip): CooccurrenceMatrixBuilder, PMICalculator / PPMICalculator, SynonymValidator."""
from src.pmi.cooccurrence import CooccurrenceConfig, CooccurrenceMatrixBuilder, CooccurrenceStats, WindowType
from src.pmi.pmi_calculator import PMICalculator, PMIConfig, PPMICalculator, compute_npmi
from src.pmi.synonym_validator import (OOVStrategy, SynonymPair, SynonymValidator, ValidationConfig, ValidationResult,
                                       create_pmi_pipeline)

__all__ = [
    "WindowType", "CooccurrenceConfig", "CooccurrenceStats", "CooccurrenceMatrixBuilder", "PMIConfig", "PMICalculator",
    "PPMICalculator", "compute_npmi", "OOVStrategy", "SynonymPair", "ValidationConfig", "ValidationResult",
    "SynonymValidator", "create_pmi_pipeline",
]

"""Deduplicators (ref:src/preprocessing/cleaners/__init__.py exports ``MinHashDeduplicator`` as the package's cleaner)."""
from src.preprocessing.cleaners.deduplicator import MinHashDeduplicator

__all__ = ["MinHashDeduplicator"]

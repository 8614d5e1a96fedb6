"""Teacher models for knowledge distillation (ref:src/model/teachers/__init__.py)."""
from .bge_m3 import BGEM3Teacher, KDLossWithBGEM3, create_bge_m3_teacher

__all__ = ["BGEM3Teacher", "KDLossWithBGEM3", "create_bge_m3_teacher"]

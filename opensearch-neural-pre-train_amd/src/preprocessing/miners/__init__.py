"""Hard-negative miners (ref:src/preprocessing/miners/__init__.py exports ``BGEM3HardNegativeMiner`` and ``MiningResult``)."""
from src.preprocessing.miners.bge_m3_miner import BGEM3HardNegativeMiner, MiningResult

__all__ = ["BGEM3HardNegativeMiner", "MiningResult"]

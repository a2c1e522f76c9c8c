from .scheduler import StreamScheduler
from .similarity import StochasticSimilarityFilter
from .engine import LORA_KEEP, StreamDiffusionEngine

__all__ = ["StreamScheduler", "StochasticSimilarityFilter", "StreamDiffusionEngine",
           "LORA_KEEP"]

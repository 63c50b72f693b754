from .generator import Generator
from .stream import StreamInfer, BatchedStreamInfer, StreamDoor

__all__ = ["Generator", "StreamInfer", "BatchedStreamInfer", "StreamDoor"]

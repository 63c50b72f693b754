from .generator import Generator
from .stream import StreamInfer, BatchedStreamInfer, StreamDoor, StreamGate, StreamDenoise

__all__ = ["Generator", "StreamInfer", "BatchedStreamInfer", "StreamDoor", "StreamGate", "StreamDenoise"]

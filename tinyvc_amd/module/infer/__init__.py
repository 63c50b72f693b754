from .generator import Generator
from .stream import StreamInfer, BatchedStreamInfer, StreamDoor, StreamGate, StreamDenoise, StreamLoudness, StreamLimiter

__all__ = ["Generator", "StreamInfer", "BatchedStreamInfer", "StreamDoor", "StreamGate", "StreamDenoise", "StreamLoudness", "StreamLimiter"]

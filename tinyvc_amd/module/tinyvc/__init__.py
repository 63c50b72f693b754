from .encoder import Encoder
from .decoder import Decoder
from .feature_retrieval import Blend, build_index, check_blend, compact_index, index_columns, match_features, match_features_blend
from .feature_retrieval import PitchRegister, pitch_register, semitones_between

# The reference also exports `Discriminator` here; it is training-only and outside this package's
# scope.
__all__ = ["Encoder", "Decoder", "match_features", "build_index", "compact_index", "index_columns", "Blend", "check_blend", "match_features_blend", "PitchRegister", "pitch_register",
           "semitones_between"]

from .encoder import Encoder
from .decoder import Decoder
from .feature_retrieval import build_index, compact_index, index_columns, match_features

# The reference also exports `Discriminator` here; it is training-only and outside this package's
# scope.
__all__ = ["Encoder", "Decoder", "match_features", "build_index", "compact_index", "index_columns"]

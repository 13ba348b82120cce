from .range_coder import (RangeEncoder, RangeDecoder, encode_with_freqs,
                          decode_with_freqs)
from .entropy import (ProbclassTesting, PredictionNetwork, encode_symbols,
                      decode_symbols, encode_symbols_batch,
                      decode_symbols_batch)
from .bitstream import (compress, decompress, compress_batch,
                        decompress_batch)

__all__ = ["RangeEncoder", "RangeDecoder", "encode_with_freqs",
           "decode_with_freqs", "ProbclassTesting", "PredictionNetwork",
           "encode_symbols", "decode_symbols", "encode_symbols_batch",
           "decode_symbols_batch", "compress", "decompress",
           "compress_batch", "decompress_batch"]

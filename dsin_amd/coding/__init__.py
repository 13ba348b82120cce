from .range_coder import (RangeEncoder, RangeDecoder, encode_with_freqs,
                          decode_with_freqs)
from .entropy import (ProbclassTesting, PredictionNetwork, encode_symbols,
                      decode_symbols, encode_symbols_batch,
                      decode_symbols_batch, encode_symbols_ragged,
                      decode_symbols_ragged)
from .bitstream import (compress, decompress, compress_batch,
                        decompress_batch, compress_many, decompress_many,
                        pack_archive, unpack_archive)

__all__ = ["RangeEncoder", "RangeDecoder", "encode_with_freqs",
           "decode_with_freqs", "ProbclassTesting", "PredictionNetwork",
           "encode_symbols", "decode_symbols", "encode_symbols_batch",
           "decode_symbols_batch", "encode_symbols_ragged",
           "decode_symbols_ragged", "compress", "decompress",
           "compress_batch", "decompress_batch", "compress_many",
           "decompress_many", "pack_archive", "unpack_archive"]

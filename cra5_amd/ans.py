"""Drop-in for the reference's pybind11 module `compressai.ans`
(cra5/models/compressai/cpp_exts/rans/rans_interface.cpp:361-381): same three classes, same
method names and argument meaning (Python lists / bytes in and out), backed by the C ABI of
libcra5_amd.so.  `import cra5_amd.ans as ans; sys.modules["compressai.ans"] = ans` is all a
reference checkout needs."""
import ctypes

import numpy as np

from . import ops
from ._lib import check, lib


_i32, _tables = ops._np_i32, ops._tables


class RansEncoder:
    def encode_with_indexes(self, symbols, indexes, cdfs, cdfs_sizes, offsets):
        return ops.rans_encode(symbols, indexes, cdfs, cdfs_sizes, offsets)


class BufferedRansEncoder:
    def __init__(self):
        self._h = ctypes.c_void_p(lib().cra5_rans_encoder_new())
        if not self._h:
            raise MemoryError("cra5_rans_encoder_new")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().cra5_rans_encoder_free(self._h)
            self._h = None

    def encode_with_indexes(self, symbols, indexes, cdfs, cdfs_sizes, offsets):
        s, i = _i32(symbols).reshape(-1), _i32(indexes).reshape(-1)
        if s.size != i.size:
            raise ValueError("`symbols` and `indexes` should have the same size.")
        c, l, o = _tables(cdfs, cdfs_sizes, offsets)
        check(lib().cra5_rans_encoder_push(self._h, s.ctypes.data, i.ctypes.data, s.size, c.ctypes.data, c.shape[0],
                                           c.shape[1], l.ctypes.data, o.ctypes.data), "cra5_rans_encoder_push")

    def flush(self):
        return ops._encoded("cra5_rans_encoder_flush", self._h)


class RansDecoder:
    def __init__(self):
        self._h = ctypes.c_void_p(lib().cra5_rans_decoder_new())
        if not self._h:
            raise MemoryError("cra5_rans_decoder_new")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().cra5_rans_decoder_free(self._h)
            self._h = None

    def decode_with_indexes(self, encoded, indexes, cdfs, cdfs_sizes, offsets):
        return ops.rans_decode(encoded, indexes, cdfs, cdfs_sizes, offsets).tolist()

    def set_stream(self, encoded):
        buf = (ctypes.c_char * len(encoded)).from_buffer_copy(encoded)
        check(lib().cra5_rans_decoder_set_stream(self._h, ctypes.addressof(buf), len(encoded)),
              "cra5_rans_decoder_set_stream")

    def decode_stream(self, indexes, cdfs, cdfs_sizes, offsets):
        i = _i32(indexes).reshape(-1)
        c, l, o = _tables(cdfs, cdfs_sizes, offsets)
        out = np.empty(i.size, dtype=np.int32)
        check(lib().cra5_rans_decoder_decode_stream(self._h, i.ctypes.data, i.size, c.ctypes.data, c.shape[0],
                                                    c.shape[1], l.ctypes.data, o.ctypes.data, out.ctypes.data),
              "cra5_rans_decoder_decode_stream")
        return out.tolist()


def pmf_to_quantized_cdf(pmf, precision):
    """`compressai._CXX.pmf_to_quantized_cdf` (ops.cpp:112-118): list in, list out."""
    return ops.pmf_to_quantized_cdf(np.asarray(pmf, dtype=np.float32), precision).tolist()

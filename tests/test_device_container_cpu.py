"""sz3hip_compress_from_device / sz3hip_decompress_to_device without a GPU: the symbols, the argument checks that need no device, and a
loud failure (never a fallback) where a device would be needed."""
import ctypes as C

import numpy as np
import pytest

import sz3_amd

L = sz3_amd.lib()
L.sz3hip_last_error_code.restype = C.c_int


def _codes():  # the error enum of include/sz3hip.h
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sz3hip.h")) as f:
        txt = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SZ3HIP_E[A-Z]+) = (-?\d+)", txt)}


CODES = _codes()


def _conf(*dims):
    c = sz3_amd.Config(*dims)
    c.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
    c.absErrorBound = 1e-3
    return c


def _compress_dev(conf, dt, ptr=0x1000, strides=None, cap=None):
    if cap is None:
        cap = int(L.sz3hip_compress_bound(C.byref(conf._c), dt))
    out = np.empty(max(cap, 1), np.uint8)
    st = (C.c_int64 * len(strides))(*strides) if strides else None
    n = L.sz3hip_compress_from_device(C.byref(conf._c), dt, ptr, st, out.ctypes.data, cap, None)
    return n, L.sz3hip_last_error_code(), L.sz3hip_last_error().decode()


def test_symbols_exported():
    assert hasattr(L, "sz3hip_compress_from_device") and hasattr(L, "sz3hip_decompress_to_device")


def test_unknown_data_type():
    n, code, msg = _compress_dev(_conf(8, 8), 10, cap=1 << 20)
    assert n == 0 and code == CODES["SZ3HIP_EUNSUPPORTED"] and "dataType" in msg


def test_rank_outside_1_to_4():
    c = _conf(8, 8)
    c._c.N = 5
    n, code, msg = _compress_dev(c, 0, cap=1 << 20)
    assert n == 0 and code == CODES["SZ3HIP_EINVAL"] and "dimension" in msg
    c._c.N = 0
    n, code, _ = _compress_dev(c, 0, cap=1 << 20)
    assert n == 0 and code == CODES["SZ3HIP_EINVAL"]


def test_num_must_match_dims():
    c = _conf(8, 8)
    c._c.num = 65
    n, code, msg = _compress_dev(c, 0, cap=1 << 20)
    assert n == 0 and code == CODES["SZ3HIP_EINVAL"] and "num" in msg


def test_capacity_too_small():
    c = _conf(16, 16)
    cap = int(L.sz3hip_compress_bound(C.byref(c._c), 0))
    n, code, msg = _compress_dev(c, 0, cap=cap - 1)
    assert n == 0 and code == CODES["SZ3HIP_ECAPACITY"] and "not large enough" in msg


def test_negative_stride_refused():
    n, code, msg = _compress_dev(_conf(8, 8), 0, strides=[8, -1])
    assert n == 0 and code == CODES["SZ3HIP_EINVAL"] and "negative" in msg


def _lossless_container(shape=(6, 10)):
    """a container this machine can write without a device: ALGO_LOSSLESS is zstd alone"""
    a = np.arange(np.prod(shape), dtype=np.float32).reshape(shape)
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = sz3_amd.ALGO_LOSSLESS
    blob, _ = sz3_amd.compress(a, c)
    return np.ascontiguousarray(blob)


@pytest.mark.parametrize("strides", [[10, 0], [1, 1], [5, 1], [1, 5]])
def test_overlapping_output_strides_refused(strides):
    blob = _lossless_container()
    c = sz3_amd.Config(1)
    st = (C.c_int64 * 2)(*strides)
    rc = L.sz3hip_decompress_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, 0x1000, st, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and "overlap" in L.sz3hip_last_error().decode()


def test_non_overlapping_strides_pass_the_check():
    """a transposed or padded view is a valid output: without a device the call stops at the pointer check, not at the strides"""
    blob = _lossless_container()
    c = sz3_amd.Config(1)
    for strides in ([1, 6], [16, 1]):
        st = (C.c_int64 * 2)(*strides)
        rc = L.sz3hip_decompress_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, 0x1000, st, None)
        assert rc != 0 and "overlap" not in L.sz3hip_last_error().decode()


def test_without_a_device_both_calls_fail():
    """a host pointer (or no device at all) is an error; nothing falls back to a host path"""
    a = np.random.default_rng(0).random((16, 16), dtype=np.float32)
    n, code, msg = _compress_dev(_conf(16, 16), 0, ptr=a.ctypes.data)
    assert n == 0 and code == CODES["SZ3HIP_EINVAL"] and "device memory" in msg
    blob = _lossless_container()
    c = sz3_amd.Config(1)
    out = np.zeros(60, np.float32)
    rc = L.sz3hip_decompress_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, out.ctypes.data, None, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and "device memory" in L.sz3hip_last_error().decode()
    assert not out.any()

"""The coarse decode without a GPU: the symbols and Python names, sz3hip_coarse_dims (a pure function), the argument checks that need no
device, and a loud failure (never a fallback) where a device would be needed."""
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


def test_symbols_and_names_exist():
    for sym in ("sz3hip_coarse_dims", "sz3hip_decompress_device_coarse", "sz3hip_decompress_coarse_to_device"):
        assert hasattr(L, sym), sym
    assert callable(sz3_amd.coarse_dims) and callable(sz3_amd.decompress_coarse)
    assert callable(sz3_amd.DeviceCompressor.decompress_coarse)


def _random_dims(rng):
    n = int(rng.integers(1, 5))
    special = [1, 2, 3]
    for e in range(2, 13):
        special += [2 ** e - 1, 2 ** e, 2 ** e + 1]
    return [int(rng.choice(special)) if rng.random() < 0.7 else int(rng.integers(1, 5000)) for _ in range(n)]


def test_coarse_dims_is_the_length_of_the_strided_range():
    rng = np.random.default_rng(20261018)
    seen_one = seen_pow = False
    for _ in range(300):
        dims = _random_dims(rng)
        c = sz3_amd._CConfig()  # (the C function keeps extents of 1: the raw struct, not Config, which drops them)
        c.N = len(dims)
        for i, d in enumerate(dims):
            c.dims[i] = d
        for k in range(13):
            out = (C.c_uint64 * 4)()
            assert L.sz3hip_coarse_dims(C.byref(c), k, out) == 0
            want = [len(range(0, d, 2 ** k)) for d in dims]
            assert [int(out[i]) for i in range(len(dims))] == want, (dims, k)
            seen_one |= 1 in want
            seen_pow |= any(d & (d - 1) == 0 and d > 2 for d in dims)
    assert seen_one and seen_pow


def test_python_coarse_dims():
    conf = sz3_amd.Config(5, 40, 70)
    assert sz3_amd.coarse_dims(conf, 0) == (5, 40, 70)
    assert sz3_amd.coarse_dims(conf, 1) == (3, 20, 35)
    assert sz3_amd.coarse_dims(conf, 3) == (1, 5, 9)
    assert sz3_amd.coarse_dims(sz3_amd.Config(4097), 12) == (2,)


@pytest.mark.parametrize("level", [-1, 31])
def test_level_out_of_range(level):
    conf = sz3_amd.Config(8, 8)
    out = (C.c_uint64 * 4)()
    assert L.sz3hip_coarse_dims(C.byref(conf._c), level, out) == CODES["SZ3HIP_EINVAL"]
    assert "level" in L.sz3hip_last_error().decode()
    with pytest.raises(sz3_amd.SZ3HipError):
        sz3_amd.coarse_dims(conf, level)
    blob = _lossless_container()
    c = sz3_amd.Config(1)
    rc = L.sz3hip_decompress_coarse_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, level, 0x1000, None, None)
    assert rc == CODES["SZ3HIP_EINVAL"]


def _lossless_container(shape=(6, 10)):
    """a container this machine can write without a device: ALGO_LOSSLESS is zstd alone"""
    a = np.arange(np.prod(shape), dtype=np.float32).reshape(shape)
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = sz3_amd.ALGO_LOSSLESS
    blob, _ = sz3_amd.compress(a, c)
    return np.ascontiguousarray(blob)


def test_integer_types_are_unsupported():
    blob = _lossless_container()
    c = sz3_amd.Config(1)
    rc = L.sz3hip_decompress_coarse_to_device(C.byref(c._c), 7, blob.ctypes.data, blob.size, 1, 0x1000, None, None)
    assert rc == CODES["SZ3HIP_EUNSUPPORTED"] and "integer" in L.sz3hip_last_error().decode()


def test_truncated_container():
    blob = _lossless_container()
    c = sz3_amd.Config(1)
    part = np.ascontiguousarray(blob[:blob.size - 5])
    rc = L.sz3hip_decompress_coarse_to_device(C.byref(c._c), 0, part.ctypes.data, part.size, 1, 0x1000, None, None)
    assert rc == CODES["SZ3HIP_EFORMAT"]


def test_overlapping_output_strides_refused():
    blob = _lossless_container()  # 6 x 10: level 1 is 3 x 5
    c = sz3_amd.Config(1)
    st = (C.c_int64 * 2)(1, 1)
    rc = L.sz3hip_decompress_coarse_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, 1, 0x1000, st, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and "overlap" in L.sz3hip_last_error().decode()
    assert tuple(c.dims) == (6, 10), "conf stays the full array's"


def test_without_a_device_the_calls_fail_loudly():
    """a host pointer (or no device at all) is an error; nothing falls back to a host path"""
    blob = _lossless_container()
    c = sz3_amd.Config(1)
    out = np.zeros(15, np.float32)
    rc = L.sz3hip_decompress_coarse_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, 1, out.ctypes.data, None, None)
    assert rc < 0 and L.sz3hip_last_error().decode()
    assert rc == CODES["SZ3HIP_EINVAL"] and "device memory" in L.sz3hip_last_error().decode()
    assert not out.any()
    with pytest.raises(ValueError):
        sz3_amd.decompress_coarse(blob, np.float32, 1)  # (neither device= nor out=)
    with pytest.raises(ValueError):
        sz3_amd.decompress_coarse(blob, np.float32, 1, out=out)  # (a host array)


def test_device_context_call_fails_loudly_without_a_context():
    """without a device no context can be made, and the call refuses a missing one: a negative code and a message"""
    from conftest import gpu_available
    if not gpu_available():
        with pytest.raises(sz3_amd.SZ3HipError):
            sz3_amd.DeviceCompressor(1000, np.float32)
    rc = L.sz3hip_decompress_device_coarse(None, 0x1000, 4096, 1, 0x2000, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and L.sz3hip_last_error().decode()

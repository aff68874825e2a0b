"""The opened stream, without a GPU: the symbols, struct sz3hip_stream_stats' layout against the header, the argument
checks that come before anything touches a device, and the Python names and signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import sz3_amd
from test_region_cpu import CODES

L = sz3_amd.lib()
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sz3hip.h")
SYMBOLS = ("sz3hip_stream_open", "sz3hip_stream_open_payload", "sz3hip_stream_config", "sz3hip_stream_tiles", "sz3hip_stream_stats", "sz3hip_stream_close",
           "sz3hip_debug_chain_points", "sz3hip_debug_get_chain_points")


def err():
    return L.sz3hip_last_error().decode()


def test_symbols_exist():
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
    with open(HEADER) as f:
        txt = f.read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, txt), "%s is not declared in include/sz3hip.h" % sym


def test_stats_layout_matches_the_header():
    with open(HEADER) as f:
        txt = f.read()
    body = re.search(r"struct sz3hip_stream_stats \{(.*?)\};", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r"(uint32_t|uint64_t)\s+(\w+)\s*;", body)]
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    assert [(n, ctype[t]) for n, t in fields] == list(sz3_amd._CStreamStats._fields_)
    for need in ("fast", "units_total", "huffman_stages", "requests", "launches_last_request", "chain_levels_last_request", "scratch_elems", "resident_bytes"):
        assert need in dict(fields), need
    assert C.sizeof(sz3_amd._CStreamStats) == 56
    off = 0  # natural alignment, no hidden padding: what a C compiler lays out
    for n, t in sz3_amd._CStreamStats._fields_:
        assert getattr(sz3_amd._CStreamStats, n).offset == off, n
        off += C.sizeof(t)


def test_open_refuses_before_any_device_work():
    blob = np.zeros(64, dtype=np.uint8)
    conf = sz3_amd.Config(1)
    h = C.c_void_p()
    assert L.sz3hip_stream_open(None, C.byref(conf._c), 0, blob.ctypes.data, blob.size, 0) == CODES["SZ3HIP_EINVAL"] and "out" in err()
    for dt in range(2, 10):  # the integer element types: the partial calls' code and wording
        assert L.sz3hip_stream_open(C.byref(h), C.byref(conf._c), dt, blob.ctypes.data, blob.size, 0) == CODES["SZ3HIP_EUNSUPPORTED"]
        assert err() == "the region decode reads float / double arrays; integer element types are not supported yet" and not h.value
        assert L.sz3hip_decompress_tiles_to_device(C.byref(conf._c), dt, blob.ctypes.data, blob.size, 0, None, 0, None, None) == CODES["SZ3HIP_EUNSUPPORTED"]
        assert err() == "the region decode reads float / double arrays; integer element types are not supported yet"
        assert L.sz3hip_stream_open_payload(C.byref(h), 0, dt, None, 0, None) == CODES["SZ3HIP_EUNSUPPORTED"] and "integer element types" in err()
    for dt in (-1, 10):
        assert L.sz3hip_stream_open(C.byref(h), C.byref(conf._c), dt, blob.ctypes.data, blob.size, 0) == CODES["SZ3HIP_EUNSUPPORTED"] and "dataType" in err()
    assert L.sz3hip_stream_open(C.byref(h), None, 0, blob.ctypes.data, blob.size, 0) == CODES["SZ3HIP_EINVAL"] and "conf" in err()
    assert L.sz3hip_stream_open(C.byref(h), C.byref(conf._c), 0, None, 0, 0) == CODES["SZ3HIP_EINVAL"] and "cmpData" in err()
    rc = L.sz3hip_stream_open(C.byref(h), C.byref(conf._c), 0, blob.ctypes.data, blob.size, 0)  # (64 zero bytes are no container)
    assert rc == L.sz3hip_peek_config(C.byref(conf._c), blob.ctypes.data, blob.size) != 0 and not h.value
    assert L.sz3hip_stream_open_payload(None, 0, 0, None, 0, None) == CODES["SZ3HIP_EINVAL"] and "out" in err()
    assert L.sz3hip_stream_open_payload(C.byref(h), 0, 0, None, 1 << 20, None) == CODES["SZ3HIP_EINVAL"] and "payload is NULL" in err()
    assert L.sz3hip_stream_open_payload(C.byref(h), 0, 0, 4096, 8, None) == CODES["SZ3HIP_EFORMAT"] and "shorter than its header" in err()
    assert not h.value


def test_calls_refuse_a_null_handle():
    boxes = (sz3_amd._CBox * 1)()
    outs = (C.c_void_p * 1)(4096)
    st = sz3_amd._CStreamStats()
    conf = sz3_amd.Config(1)
    assert L.sz3hip_stream_tiles(None, 0, boxes, 1, outs, None) == CODES["SZ3HIP_EINVAL"] and "no handle" in err()
    assert L.sz3hip_stream_stats(None, C.byref(st)) == CODES["SZ3HIP_EINVAL"] and "no handle" in err()
    assert L.sz3hip_stream_config(None, C.byref(conf._c)) == CODES["SZ3HIP_EINVAL"] and "no handle" in err()
    L.sz3hip_stream_close(None)  # (allowed, like free)


def test_chain_points_setter():
    before = L.sz3hip_debug_get_chain_points()
    try:
        for v in (0, 64, 2048, 1 << 31, 0xFFFFFFFF):
            sz3_amd.set_chain_points(v)
            assert sz3_amd.get_chain_points() == L.sz3hip_debug_get_chain_points() == v
    finally:
        L.sz3hip_debug_chain_points(before)


def test_python_names_and_signatures():
    def params(f):
        return list(inspect.signature(f).parameters)

    assert params(sz3_amd.open_stream) == ["blob", "dtype", "device"] and inspect.signature(sz3_amd.open_stream).parameters["device"].default is None
    assert params(sz3_amd.DeviceCompressor.open_stream) == ["self", "d_payload", "size", "stream"]
    assert inspect.signature(sz3_amd.DeviceCompressor.open_stream).parameters["stream"].default == 0
    S = sz3_amd.Stream
    assert params(S.tiles) == ["self", "level", "boxes", "out", "stream"]
    assert params(S.tile) == ["self", "level", "lo", "shape", "out", "stream"]
    assert params(S.region) == ["self", "lo", "shape", "out", "stream"]
    assert params(S.coarse) == ["self", "level", "out", "stream"]
    for f in (S.tiles, S.tile, S.region, S.coarse):
        p = inspect.signature(f).parameters
        assert p["out"].default is None and p["stream"].default is None
    for name in ("stats", "close", "__enter__", "__exit__"):
        assert callable(getattr(S, name)), name
    assert callable(sz3_amd.set_chain_points) and callable(sz3_amd.get_chain_points)

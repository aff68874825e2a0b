"""GPU tests (-m gpu) of the host decode chain's copy-out branches (csrc/sz3hip_host.cpp, d2h_out) and of the decode side of
SZ3HIP_STOCK_HOST_HUFFMAN (stock_huff_run). 256 x 256 x 128 f32 is exactly 32 MiB, the smallest array for which the staging ring
(d2h_staging_wanted) and the population of the output's pages (Prefault::start) act; one plane less takes the plain copy whatever the
switches say. Every way of handing the same container's array out must give the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sz3_amd  # noqa: E402
from fields import field1d, field3d  # noqa: E402

AT, BELOW = (256, 256, 128), (256, 256, 127)
EB = 1e-3
HOST_WAYS = [{}, {"SZ3HIP_D2H_STAGED": "0"}, {"SZ3HIP_D2H_STAGED": "0", "SZ3HIP_NO_PREFAULT": "1"}]


@pytest.fixture(scope="module")
def field_at():
    a = field3d(AT)
    a.setflags(write=False)
    return a


def _compress(a, algo=None, stock=False):
    conf = sz3_amd.Config(*a.shape)
    if algo is not None:
        conf.cmprAlgo = algo
    conf.absErrorBound = EB
    L = sz3_amd.lib()
    if stock:
        L.sz3hip_set_stock_format(1)
    try:
        blob, _ = sz3_amd.compress(a, conf)
    finally:
        if stock:
            L.sz3hip_set_stock_format(0)
    return blob


def _host_ways(blob, a, monkeypatch):
    """default, SZ3HIP_D2H_STAGED=0, SZ3HIP_D2H_STAGED=0 + SZ3HIP_NO_PREFAULT=1: a fresh array each time"""
    decs = []
    for env in HOST_WAYS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            dec, conf = sz3_amd.decompress(blob, a.dtype, a.shape)
        decs.append(dec)
    assert float(np.max(np.abs(decs[0].astype(np.float64) - a.astype(np.float64)))) <= EB
    for env, d in zip(HOST_WAYS[1:], decs[1:]):
        assert np.array_equal(d.view(np.uint32), decs[0].view(np.uint32)), "the decode under %s differs from the default one" % env
    return decs[0], conf


def test_copy_out_at_the_threshold_native_stream(field_at, monkeypatch):
    a = field_at
    assert a.nbytes == 32 << 20
    blob = _compress(a)
    first, conf = _host_ways(blob, a, monkeypatch)
    assert conf.cmprAlgo in (sz3_amd.ALGO_HIP_LORENZO, sz3_amd.ALGO_HIP_INTERP) and conf.openmp == 0
    kept = np.full(a.shape, np.float32(-7.0))  # (pages touched before: the caller's own array)
    got, _ = sz3_amd.decompress(blob, a.dtype, a.shape, out=kept)
    assert np.shares_memory(got, kept)
    assert np.array_equal(kept.view(np.uint32), first.view(np.uint32)), "the decode into out= differs"
    t, _ = sz3_amd.decompress(blob, a.dtype, a.shape, device="cuda")
    assert np.array_equal(t.cpu().numpy().view(np.uint32), first.view(np.uint32)), "the decode into a device tensor differs"


def test_plain_path_below_the_threshold(monkeypatch):
    a = field3d(BELOW)
    assert a.nbytes < 32 << 20
    _, conf = _host_ways(_compress(a), a, monkeypatch)
    assert conf.openmp == 0


def test_copy_out_at_the_threshold_stock_stream(field_at, monkeypatch):
    a = field_at
    blob = _compress(a, sz3_amd.ALGO_INTERP, stock=True)
    _, conf = _host_ways(blob, a, monkeypatch)
    assert conf.cmprAlgo == sz3_amd.ALGO_INTERP, "not a stock interpolation container"


def _both_huffmans(blob, a, algo, monkeypatch):
    decs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SZ3HIP_STOCK_HOST_HUFFMAN", mode)
        decs[mode], conf = sz3_amd.decompress(blob, a.dtype, a.shape)
        assert conf.cmprAlgo == algo, "not the stock container asked for"
    assert np.array_equal(decs["0"].view(np.uint32), decs["1"].view(np.uint32)), "host and device Huffman stages decode different arrays"
    return decs["0"]


@pytest.mark.parametrize("algo", [sz3_amd.ALGO_INTERP, sz3_amd.ALGO_LORENZO_REG], ids=["interp", "lorenzo-reg"])
@pytest.mark.parametrize("what", ["field-3d", "one-value-3d"])
def test_stock_readers_host_huffman_against_device_huffman(what, algo, monkeypatch):
    """one-value-3d: zeros, every point predicted exactly from the start. The Lorenzo / regression stream then holds one code, the tree of
    a single symbol (no bits at all); the interpolation stream holds two, its anchor points being stored as unpredictable values (code 0)."""
    shape = (40, 48, 56)
    a = field3d(shape) if what == "field-3d" else np.zeros(shape, np.float32)
    dec = _both_huffmans(_compress(a, algo, stock=True), a, algo, monkeypatch)
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= EB


def test_stock_1d_lorenzo_reg_host_huffman_against_device_huffman(monkeypatch):
    a = field1d(4096)
    dec = _both_huffmans(_compress(a, sz3_amd.ALGO_LORENZO_REG, stock=True), a, sz3_amd.ALGO_LORENZO_REG, monkeypatch)
    assert float(np.max(np.abs(dec.astype(np.float64) - a.astype(np.float64)))) <= EB

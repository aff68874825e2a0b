"""Coarse decode on the MI355X: decompress_coarse(blob, dtype, k) is, bit for bit, decompress(blob, dtype)[::2**k, ...] — for every
container the device call decodes, with the interpolation streams taking the fast path (the level kernels on the compact grid). The one
assertion everywhere is raw-byte identity with the full decode, subsampled; there are no tolerances.

Every (shape, bound) of a case that must be a lossy interpolation stream was compressed with the CPU oracle first (ratio well above the
dispatcher's ratio < 3 rule); such a case asserts the trailer's cmprAlgo instead of skipping."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from sz3_amd import Dbg  # noqa: E402
from partial_cases import CODES, DEV, EB, FALLBACKS, INTERP_IDS, conf_for, container, device_payload, raw, smooth, spiky  # noqa: E402,F401

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
L.sz3hip_last_error_code.restype = C.c_int


def subsampled(full, k):
    return full[(slice(None, None, 2 ** k),) * full.dim()]


def check_levels(blob, dtype, levels, algos=None, full=None):
    """the full decode once; then every level against it"""
    if full is None:
        full, conf = sz3_amd.decompress(blob, dtype, device=DEV)
    else:
        conf = sz3_amd.Config(1)
        assert L.sz3hip_peek_config(C.byref(conf._c), blob.ctypes.data, blob.size) == 0
    if algos is not None:
        assert conf.cmprAlgo in algos, "the case must be a lossy interpolation stream (cmprAlgo %d)" % conf.cmprAlgo
    for k in levels:
        got, c2 = sz3_amd.decompress_coarse(blob, dtype, k, device=DEV)
        want = subsampled(full, k)
        assert tuple(got.shape) == sz3_amd.coarse_dims(conf, k) == tuple(want.shape)
        assert c2.dims == conf.dims, "conf must stay the full array's"
        assert np.array_equal(raw(got), raw(want)), "level %d differs from the full decode, subsampled" % k
    return full, conf


# ---- geometry --------------------------------------------------------------------------------------------------------------
SHAPES = [(4097,), (5000,), (129, 200), (97, 131), (33, 20, 37), (65, 47, 130), (64, 64, 64), (9, 17, 18, 21)]


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_geometry(shape, dtype, interp):
    a = smooth(shape, dtype)
    for direction in sorted({0, math.factorial(len(shape)) - 1}):
        blob = container(a, conf_for(shape, interpAlgo=interp, interpDirection=direction))
        check_levels(blob, np.dtype(dtype), (1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("shape,k", [((2, 40, 70), 1), ((5, 40, 70), 3)], ids=["2x40x70_k1", "5x40x70_k3"])
def test_extent_not_above_the_stride(shape, k, interp):
    """an extent <= 2^k: the coarse extent is 1, and it is kept"""
    blob = container(smooth(shape), conf_for(shape, interpAlgo=interp))
    _, conf = check_levels(blob, np.float32, (k,), algos=(sz3_amd.ALGO_HIP_INTERP,))
    assert sz3_amd.coarse_dims(conf, k)[0] == 1


# ---- level shift: the per-level bound goes by the FULL array's level numbers -----------------------------------------------
@pytest.mark.parametrize("kw", [dict(interpAlpha=1.5, interpBeta=3.0), dict(interpAlpha=-1.0)], ids=["alpha1.5_beta3", "alpha-1"])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
def test_level_shift(kw, interp):
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape, interpAlgo=interp, **kw))
    check_levels(blob, np.float32, (1, 2), algos=(sz3_amd.ALGO_HIP_INTERP,))


# ---- anchors ---------------------------------------------------------------------------------------------------------------
def test_anchor_stride_4():
    """k = 1: anchor stride 2 on the coarse grid; k = 2: every coarse point is an anchor; k = 3: the coarse grid is a subset of them"""
    shape = (33, 40, 37)
    blob = container(smooth(shape), conf_for(shape, interpAnchorStride=4))
    check_levels(blob, np.float32, (1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))


def test_anchor_stride_0():
    shape = (33, 40, 37)
    blob = container(smooth(shape), conf_for(shape, interpAnchorStride=0))
    check_levels(blob, np.float32, (1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))


def test_no_extent_above_the_default_stride():
    """20^3 under the 3-D default stride of 32: the first-point path, in the full array and on the coarse grid"""
    shape = (20, 20, 20)
    blob = container(smooth(shape), conf_for(shape))
    check_levels(blob, np.float32, (1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))


# ---- unpredictable values on and off the coarse grid -----------------------------------------------------------------------
def test_spikes():
    a, pos = spiky()
    on_grid = (pos % 2 == 0).all(axis=1)
    assert on_grid.any() and (~on_grid).any(), "the seeded spikes must lie both on and off the grid of stride 2"
    blob = container(a, conf_for(a.shape, quantbinCnt=256))
    full, _ = check_levels(blob, np.float32, (1, 2), algos=(sz3_amd.ALGO_HIP_INTERP,))
    assert float(full.max()) == 1e6


# ---- the level kernels on the coarse grid ----------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
def test_level_kernels_on_the_coarse_grid(interp):
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape, interpAlgo=interp))
    full, _ = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.debug_flags(Dbg.INTERP_LEVELS_ANY_SIZE):  # (every level of every 3-D array through k_interp_level; reset on the way out)
        check_levels(blob, np.float32, (1, 2), algos=(sz3_amd.ALGO_HIP_INTERP,), full=full)


# ---- stock format ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 47, 130), (129, 200)], ids=["65x47x130", "129x200"])
def test_stock_format(shape):
    sz3_amd.set_stock_format(1)
    try:
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    check_levels(blob, np.float32, (1, 2), algos=(sz3_amd.ALGO_INTERP,))


# ---- fallback containers: the full decode, then the strided gather ---------------------------------------------------------
@pytest.mark.parametrize("name,kw", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_fallback_containers(name, kw):
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **kw))
    _, conf = check_levels(blob, np.float32, (1, 2))
    assert conf.cmprAlgo not in INTERP_IDS
    if name == "lossless":
        assert conf.cmprAlgo == sz3_amd.ALGO_LOSSLESS


def test_fallback_openmp_slabs(monkeypatch):
    """three slabs over 50 rows: slab starts (16, 33) are no multiples of the stride"""
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    shape = (50, 30, 40)
    blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, openmp=1))
    _, conf = check_levels(blob, np.float32, (1, 2))
    assert conf.openmp


# ---- views and streams -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interp_case():
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == sz3_amd.ALGO_HIP_INTERP
    return blob, full, conf


@pytest.mark.parametrize("which", ["interp", "lorenzo"])
def test_out_is_a_sub_box(interp_case, which):
    if which == "interp":
        blob, full, conf = interp_case
    else:
        shape = (40, 48, 56)
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0))
        full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    k = 1
    cd = sz3_amd.coarse_dims(conf, k)
    big = torch.full(tuple(d + 3 for d in cd), 77.0, dtype=torch.float32, device=DEV)
    inner = tuple(slice(1, 1 + d) for d in cd)
    out, _ = sz3_amd.decompress_coarse(blob, np.float32, k, out=big[inner])
    assert out.data_ptr() == big[inner].data_ptr()
    got = big.cpu().numpy()
    assert np.array_equal(got[inner].reshape(-1).view(np.uint8), raw(subsampled(full, k)))
    mask = np.ones(got.shape, bool)
    mask[inner] = False
    assert (got[mask] == 77).all(), "elements outside the view were written"


def test_waits_for_the_producer(interp_case):
    blob, full, conf = interp_case
    k = 1
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = torch.empty(sz3_amd.coarse_dims(conf, k), dtype=torch.float32, device=DEV)
        torch.cuda._sleep(20_000_000)  # (the producer is still busy when the call is made)
        out.fill_(77.0)
        sz3_amd.decompress_coarse(blob, np.float32, k, out=out, stream=side)
    torch.cuda.synchronize()
    assert np.array_equal(raw(out), raw(subsampled(full, k)))


def test_level_0_is_decompress(interp_case):
    blob, full, conf = interp_case
    got, c2 = sz3_amd.decompress_coarse(blob, np.float32, 0, device=DEV)
    assert tuple(got.shape) == conf.dims == c2.dims
    assert np.array_equal(raw(got), raw(full))


# ---- device context --------------------------------------------------------------------------------------------------------
def ctx_coarse(dc, pl, size, conf, k):
    out = torch.full(sz3_amd.coarse_dims(conf, k), 77.0, dtype=torch.float32, device=DEV)
    dc.decompress_coarse(pl.data_ptr(), size, k, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def test_device_context():
    shape = (65, 47, 130)
    a = smooth(shape)
    conf = conf_for(shape)
    dc, pl, size, full = device_payload(a, conf)
    got1 = ctx_coarse(dc, pl, size, conf, 1)
    assert np.array_equal(raw(got1), raw(subsampled(full, 1)))
    got2 = ctx_coarse(dc, pl, size, conf, 2)  # (the same context, another level)
    fresh = sz3_amd.DeviceCompressor(a.size, a.dtype)
    want2 = ctx_coarse(fresh, pl, size, conf, 2)
    assert np.array_equal(raw(got2), raw(want2)) and np.array_equal(raw(got2), raw(subsampled(full, 2)))
    got0 = ctx_coarse(dc, pl, size, conf, 0)
    assert np.array_equal(raw(got0), raw(full))
    after = torch.empty_like(full)  # (the full decode of the same context is what it was)
    dc.decompress(pl.data_ptr(), size, after.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(raw(after), raw(full))


def test_device_context_refuses_a_lorenzo_payload():
    shape = (40, 48, 56)
    a = smooth(shape)
    conf = conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0)
    dc, pl, size, _ = device_payload(a, conf)
    out = torch.full(sz3_amd.coarse_dims(conf, 1), 77.0, dtype=torch.float32, device=DEV)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        dc.decompress_coarse(pl.data_ptr(), size, 1, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"] and "sz3hip_decompress_coarse_to_device" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 77).all())


# ---- errors: out is left untouched -----------------------------------------------------------------------------------------
def test_integer_dtype_is_unsupported(interp_case):
    blob, _, conf = interp_case
    out = torch.full(sz3_amd.coarse_dims(conf, 1), 77, dtype=torch.int32, device=DEV)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.decompress_coarse(blob, np.int32, 1, out=out)
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"]
    c = sz3_amd.Config(1)
    rc = L.sz3hip_decompress_coarse_to_device(C.byref(c._c), 7, blob.ctypes.data, blob.size, 1, out.data_ptr(), None, None)
    assert rc == CODES["SZ3HIP_EUNSUPPORTED"]
    assert bool((out == 77).all())


def test_host_pointer_is_refused(interp_case):
    blob, _, conf = interp_case
    out = np.full(sz3_amd.coarse_dims(conf, 1), 77, np.float32)
    c = sz3_amd.Config(1)
    rc = L.sz3hip_decompress_coarse_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, 1, out.ctypes.data, None, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and "device memory" in L.sz3hip_last_error().decode()
    assert (out == 77).all()


def test_truncated_blob(interp_case):
    blob, _, conf = interp_case
    out = torch.full(sz3_amd.coarse_dims(conf, 1), 77.0, dtype=torch.float32, device=DEV)
    c = sz3_amd.Config(1)
    for cut in (20, blob.size // 2, blob.size - 5):
        part = np.ascontiguousarray(blob[:cut])
        rc = L.sz3hip_decompress_coarse_to_device(C.byref(c._c), 0, part.ctypes.data, part.size, 1, out.data_ptr(), None, None)
        assert rc == CODES["SZ3HIP_EFORMAT"], (cut, rc, L.sz3hip_last_error().decode())
    assert bool((out == 77).all())

"""Region decode on the MI355X: decompress_region(blob, dtype, lo, shape) is, bit for bit, the same slice of decompress(blob, dtype) — for
every container the device call decodes, with the interpolation streams taking the fast path (the passes over the box's windows, one compact
buffer per level). The one assertion everywhere is raw-byte identity with the full decode's slice; there are no tolerances.

The fields, bounds and the 1024 quantisation bins are those of partial_cases.py (conf_for says why); a case that must be a lossy interpolation
stream asserts the trailer's cmprAlgo instead of skipping."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from sz3_amd import Dbg  # noqa: E402
from partial_cases import CODES, DEV, EB, FALLBACKS, INTERP_IDS, box_slices, boxes_of, conf_for, container, device_payload, raw, smooth, spiky  # noqa: E402,F401

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
L.sz3hip_last_error_code.restype = C.c_int


def check_boxes(blob, dtype, boxes, algos=None, full=None):
    """the full decode once; then every box against its slice. A single interpolation stream must take the fast path (the library counts
    those calls), every other container the fallback."""
    if full is None:
        full, conf = sz3_amd.decompress(blob, dtype, device=DEV)
    else:
        conf = sz3_amd.Config(1)
        assert L.sz3hip_peek_config(C.byref(conf._c), blob.ctypes.data, blob.size) == 0
    if algos is not None:
        assert conf.cmprAlgo in algos, "the case must be a lossy interpolation stream (cmprAlgo %d)" % conf.cmprAlgo
    fast = conf.cmprAlgo in INTERP_IDS and not conf.openmp
    for lo, ext in boxes:
        before = L.sz3hip_debug_region_fast_calls()
        got, c2 = sz3_amd.decompress_region(blob, dtype, lo, ext, device=DEV)
        assert L.sz3hip_debug_region_fast_calls() - before == (1 if fast else 0), "cmprAlgo %d took the %s" % (conf.cmprAlgo, "fallback" if fast else "fast path")
        want = full[box_slices(lo, ext)]
        assert tuple(got.shape) == tuple(ext) == tuple(want.shape)
        assert c2.dims == conf.dims, "conf must stay the full array's"
        assert np.array_equal(raw(got), raw(want)), "the box lo %s shape %s differs from the full decode's slice" % (lo, ext)
    return full, conf


# ---- geometry --------------------------------------------------------------------------------------------------------------
SHAPES = [(300,), (129, 200), (65, 47, 130), (9, 12, 17, 20)]


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_geometry(shape, dtype, interp):
    """(300 points are too few to pay for a stream's fixed part under every dtype: that shape takes whichever container the dispatcher
    writes; the others must be interpolation streams)"""
    blob = container(smooth(shape, dtype), conf_for(shape, interpAlgo=interp))
    check_boxes(blob, np.dtype(dtype), boxes_of(shape), algos=None if shape == (300,) else (sz3_amd.ALGO_HIP_INTERP,))


def test_geometry_1d_is_an_interpolation_stream():
    """the 1-D geometry once more on an array long enough to be written as an interpolation stream, anchors (stride 4096) included"""
    shape = (5000,)
    blob = container(smooth(shape), conf_for(shape))
    check_boxes(blob, np.float32, boxes_of(shape) + [((4001,), (200,))], algos=(sz3_amd.ALGO_HIP_INTERP,))


# ---- direction: the pass windows depend on the permutation -------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("direction", [0, 3, 5])
def test_direction(direction, interp):
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape, interpAlgo=interp, interpDirection=direction))
    check_boxes(blob, np.float32, boxes_of(shape)[1:], algos=(sz3_amd.ALGO_HIP_INTERP,))


# ---- anchors and level bounds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchor", [4, 0, -1], ids=["stride4", "stride0", "default"])
def test_anchor_strides(anchor):
    shape = (33, 40, 37)
    blob = container(smooth(shape), conf_for(shape, interpAnchorStride=anchor))
    check_boxes(blob, np.float32, boxes_of(shape), algos=(sz3_amd.ALGO_HIP_INTERP,))


def test_no_extent_above_the_default_stride():
    """20^3 under the 3-D default stride of 32: the first-point path"""
    shape = (20, 20, 20)
    blob = container(smooth(shape), conf_for(shape))
    check_boxes(blob, np.float32, boxes_of(shape), algos=(sz3_amd.ALGO_HIP_INTERP,))


@pytest.mark.parametrize("kw", [dict(interpAlpha=1.5, interpBeta=3.0), dict(interpAlpha=-1.0)], ids=["alpha1.5_beta3", "alpha-1"])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
def test_level_bounds(kw, interp):
    """the levels keep their numbers in a region decode (no shift is involved): the per-level bounds are the full decode's"""
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape, interpAlgo=interp, **kw))
    check_boxes(blob, np.float32, boxes_of(shape)[1:], algos=(sz3_amd.ALGO_HIP_INTERP,))


# ---- unpredictable values inside and outside the windows -----------------------------------------------------------------------
def test_spikes():
    a, pos = spiky()
    blob = container(a, conf_for(a.shape, quantbinCnt=256))
    with_spikes = ((10, 8, 20), (30, 25, 70))
    inside = ((pos >= np.array(with_spikes[0])) & (pos < np.array(with_spikes[0]) + np.array(with_spikes[1]))).all(axis=1)
    assert inside.any() and (~inside).any()
    # a box without a spike: the seeded positions leave this one free
    free = None
    for z in range(0, 60, 3):
        for y in range(0, 40, 3):
            for x in range(0, 120, 5):
                lo = np.array((z, y, x))
                if not ((pos >= lo) & (pos < lo + 5)).all(axis=1).any():
                    free = (tuple(int(v) for v in lo), (5, 5, 5))
                    break
            if free:
                break
        if free:
            break
    assert free is not None
    full, _ = check_boxes(blob, np.float32, [with_spikes, free], algos=(sz3_amd.ALGO_HIP_INTERP,))
    assert float(full[box_slices(*with_spikes)].max()) == 1e6 and float(full[box_slices(*free)].max()) < 1e3


# ---- against the level kernels' output -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
def test_against_the_level_kernels(interp):
    """the full decode under the hook runs k_interp_level on every level; the region decode's pass kernels must give the same bits"""
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape, interpAlgo=interp))
    with sz3_amd.debug_flags(Dbg.INTERP_LEVELS_ANY_SIZE):
        full, _ = sz3_amd.decompress(blob, np.float32, device=DEV)
    plain, _ = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert np.array_equal(raw(full), raw(plain))
    check_boxes(blob, np.float32, boxes_of(shape), algos=(sz3_amd.ALGO_HIP_INTERP,), full=full)


# ---- stock format --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 47, 130), (129, 200)], ids=["65x47x130", "129x200"])
def test_stock_format(shape):
    sz3_amd.set_stock_format(1)
    try:
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    check_boxes(blob, np.float32, boxes_of(shape), algos=(sz3_amd.ALGO_INTERP,))


# ---- fallback containers: the full decode, then the strided gather of the box ---------------------------------------------------
@pytest.mark.parametrize("name,kw", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_fallback_containers(name, kw):
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **kw))
    _, conf = check_boxes(blob, np.float32, [((3, 7, 11), (20, 9, 30))])
    assert conf.cmprAlgo not in INTERP_IDS
    if name == "lossless":
        assert conf.cmprAlgo == sz3_amd.ALGO_LOSSLESS


def test_fallback_openmp_slabs(monkeypatch):
    """three slabs over 50 rows: the box spans two slab boundaries"""
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    shape = (50, 30, 40)
    blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, openmp=1))
    _, conf = check_boxes(blob, np.float32, [((11, 3, 5), (30, 20, 17))])
    assert conf.openmp


# ---- views and streams ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interp_case():
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == sz3_amd.ALGO_HIP_INTERP
    return blob, full, conf


BOX = ((7, 9, 29), (20, 11, 40))


@pytest.mark.parametrize("which", ["interp", "lorenzo"])
def test_out_is_a_sub_box(interp_case, which):
    if which == "interp":
        blob, full, conf = interp_case
        lo, ext = BOX
    else:
        shape = (40, 48, 56)
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0))
        full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
        lo, ext = (3, 7, 11), (20, 9, 30)
    big = torch.full(tuple(d + 3 for d in ext), 77.0, dtype=torch.float32, device=DEV)
    inner = tuple(slice(1, 1 + d) for d in ext)
    out, _ = sz3_amd.decompress_region(blob, np.float32, lo, ext, out=big[inner])
    assert out.data_ptr() == big[inner].data_ptr()
    got = big.cpu().numpy()
    assert np.array_equal(got[inner].reshape(-1).view(np.uint8), raw(full[box_slices(lo, ext)]))
    mask = np.ones(got.shape, bool)
    mask[inner] = False
    assert (got[mask] == 77).all(), "elements outside the view were written"


def test_waits_for_the_producer(interp_case):
    blob, full, conf = interp_case
    lo, ext = BOX
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = torch.empty(ext, dtype=torch.float32, device=DEV)
        torch.cuda._sleep(20_000_000)  # (the producer is still busy when the call is made)
        out.fill_(77.0)
        sz3_amd.decompress_region(blob, np.float32, lo, ext, out=out, stream=side)
    torch.cuda.synchronize()
    assert np.array_equal(raw(out), raw(full[box_slices(lo, ext)]))


# ---- device context ------------------------------------------------------------------------------------------------------------
def ctx_region(dc, pl, size, lo, ext):
    out = torch.full(ext, 77.0, dtype=torch.float32, device=DEV)
    dc.decompress_region(pl.data_ptr(), size, lo, ext, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def test_device_context_and_its_scratch():
    shape = (65, 47, 130)
    a = smooth(shape)
    conf = conf_for(shape)
    dc, pl, size, full = device_payload(a, conf)
    assert dc.region_scratch() == 0
    lo, ext = BOX
    plan = sz3_amd.region_plan(conf, lo, ext)
    got = ctx_region(dc, pl, size, lo, ext)
    assert np.array_equal(raw(got), raw(full[box_slices(lo, ext)]))
    cap = dc.region_scratch()
    assert cap >= plan["scratch_elems"] > 0
    # the same plan again, then a smaller one: nothing is allocated
    got = ctx_region(dc, pl, size, lo, ext)
    assert np.array_equal(raw(got), raw(full[box_slices(lo, ext)])) and dc.region_scratch() == cap
    small = ((31, 21, 63), (1, 1, 1))
    got = ctx_region(dc, pl, size, *small)
    assert np.array_equal(raw(got), raw(full[box_slices(*small)])) and dc.region_scratch() == cap
    # a larger plan grows it
    whole = ((0, 0, 0), shape)
    got = ctx_region(dc, pl, size, *whole)
    assert np.array_equal(raw(got), raw(full))
    assert dc.region_scratch() >= sz3_amd.region_plan(conf, *whole)["scratch_elems"] > cap
    after = torch.empty_like(full)  # (the full decode of the same context is what it was)
    dc.decompress(pl.data_ptr(), size, after.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(raw(after), raw(full))


def test_device_context_checks_the_box_before_any_launch():
    shape = (65, 47, 130)
    dc, pl, size, _ = device_payload(smooth(shape), conf_for(shape))
    out = torch.full((4, 4, 4), 77.0, dtype=torch.float32, device=DEV)
    for lo, ext, dim in (((0, 0, 128), (4, 4, 4), 2), ((0, 47, 0), (4, 1, 4), 1), ((1, 1, 1), (0, 4, 4), 0)):
        with pytest.raises(sz3_amd.SZ3HipError) as e:
            dc.decompress_region(pl.data_ptr(), size, lo, ext, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert e.value.code == CODES["SZ3HIP_EINVAL"] and "dimension %d" % dim in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and dc.region_scratch() == 0


def test_device_context_refuses_a_lorenzo_payload():
    shape = (40, 48, 56)
    a = smooth(shape)
    conf = conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0)
    dc, pl, size, _ = device_payload(a, conf)
    out = torch.full((4, 4, 4), 77.0, dtype=torch.float32, device=DEV)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        dc.decompress_region(pl.data_ptr(), size, (1, 1, 1), (4, 4, 4), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"] and "sz3hip_decompress_region_to_device" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 77).all())


# ---- errors: out is left untouched ---------------------------------------------------------------------------------------------
def _call(blob, dt, lo, ext, ptr):
    c = sz3_amd.Config(1)
    return L.sz3hip_decompress_region_to_device(C.byref(c._c), dt, blob.ctypes.data, blob.size, (C.c_uint64 * 4)(*lo), (C.c_uint64 * 4)(*ext), ptr, None, None)


def test_integer_dtype_is_unsupported(interp_case):
    blob, _, conf = interp_case
    lo, ext = BOX
    out = torch.full(ext, 77, dtype=torch.int32, device=DEV)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.decompress_region(blob, np.int32, lo, ext, out=out)
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"]
    assert _call(blob, 7, lo, ext, out.data_ptr()) == CODES["SZ3HIP_EUNSUPPORTED"]
    assert bool((out == 77).all())


def test_host_pointer_is_refused(interp_case):
    blob, _, conf = interp_case
    lo, ext = BOX
    out = np.full(ext, 77, np.float32)
    assert _call(blob, 0, lo, ext, out.ctypes.data) == CODES["SZ3HIP_EINVAL"] and "device memory" in L.sz3hip_last_error().decode()
    assert (out == 77).all()


def test_box_outside_the_array(interp_case):
    blob, _, conf = interp_case
    out = torch.full((4, 4, 4), 77.0, dtype=torch.float32, device=DEV)
    assert _call(blob, 0, (62, 0, 0), (4, 4, 4), out.data_ptr()) == CODES["SZ3HIP_EINVAL"] and "dimension 0" in L.sz3hip_last_error().decode()
    assert bool((out == 77).all())


def test_truncated_blob(interp_case):
    blob, _, conf = interp_case
    lo, ext = BOX
    out = torch.full(ext, 77.0, dtype=torch.float32, device=DEV)
    for cut in (20, blob.size // 2, blob.size - 5):
        part = np.ascontiguousarray(blob[:cut])
        rc = _call(part, 0, lo, ext, out.data_ptr())
        assert rc == CODES["SZ3HIP_EFORMAT"], (cut, rc, L.sz3hip_last_error().decode())
    assert bool((out == 77).all())

"""Tile decode on the MI355X: decompress_tile(blob, dtype, k, lo, shape) is, bit for bit, decompress(blob, dtype)[::2**k, ...][box] — the box
of the grid of every 2^k-th point — with the Huffman stage of this library's own interpolation streams decoding only the units the box needs.
The one assertion on values everywhere is raw-byte identity with the full decode's slice; there are no tolerances. Fields, bound and the 1024
quantisation bins are partial_cases.py's."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, boxes_of, conf_for, container, device_payload, raw, smooth, spiky  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
DEF_ANCHOR = (4096, 128, 32, 16)


def coarse_shape(shape, k):
    return tuple(((d - 1) >> k) + 1 for d in shape)


def coarse_view(full, k):
    return full[tuple(slice(None, None, 1 << k) for _ in full.shape)]


def tile_boxes(shape):
    """boxes_of(shape), clipped to the grid: a coarse grid may be shorter along x than the offsets boxes_of starts its straddling box at"""
    out = []
    for lo, ext in boxes_of(shape):
        lo = tuple(min(max(a, 0), d - 1) for a, d in zip(lo, shape))
        out.append((lo, tuple(max(1, min(e, d - a)) for e, d, a in zip(ext, shape, lo))))
    return out


def check_tiles(blob, dtype, levels, algos=None, full=None, boxes=None):
    """the full decode once; then every box of tile_boxes(coarse shape) at every level against its slice. A single interpolation stream must take
    the fast path (the library counts those calls), every other container the fallback."""
    if full is None:
        full, conf = sz3_amd.decompress(blob, dtype, device=DEV)
    else:
        conf = sz3_amd.Config(1)
        assert L.sz3hip_peek_config(C.byref(conf._c), blob.ctypes.data, blob.size) == 0
    if algos is not None:
        assert conf.cmprAlgo in algos, "the case must be a lossy interpolation stream (cmprAlgo %d)" % conf.cmprAlgo
    fast = conf.cmprAlgo in INTERP_IDS and not conf.openmp
    for k in levels:
        cv = coarse_view(full, k)
        assert tuple(cv.shape) == coarse_shape(conf.dims, k) == sz3_amd.coarse_dims(conf, k)
        for lo, ext in (tile_boxes(tuple(cv.shape)) if boxes is None else boxes(tuple(cv.shape))):
            before = L.sz3hip_debug_region_fast_calls()
            got, c2 = sz3_amd.decompress_tile(blob, dtype, k, lo, ext, device=DEV)
            assert L.sz3hip_debug_region_fast_calls() - before == (1 if fast else 0), "cmprAlgo %d took the %s" % (conf.cmprAlgo, "fallback" if fast else "fast path")
            want = cv[box_slices(lo, ext)]
            assert tuple(got.shape) == tuple(ext) == tuple(want.shape)
            assert c2.dims == conf.dims, "conf must stay the full array's"
            assert np.array_equal(raw(got), raw(want)), "level %d: the box lo %s shape %s differs from the full decode's slice" % (k, lo, ext)
    return full, conf


# ---- bit identity: shapes, levels, boxes, types, rules -------------------------------------------------------------------------
SHAPES = [(65, 47, 130), (33, 70), (1000,), (9, 12, 17, 20), (5, 9, 1100)]


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bit_identity(shape, dtype, interp):
    """k = 0 .. 3 and the k whose stride is the default anchor stride (every coarse point an anchor; 1-D: no extent above 4096, the first point).
    (1000 points are too few to pay for an interpolation stream's fixed part: that shape takes whichever container the dispatcher writes)"""
    blob = container(smooth(shape, dtype), conf_for(shape, interpAlgo=interp))
    k_anchor = int(np.log2(DEF_ANCHOR[len(shape) - 1]))
    check_tiles(blob, np.dtype(dtype), (0, 1, 2, 3, k_anchor), algos=None if shape == (1000,) else (sz3_amd.ALGO_HIP_INTERP,))


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("direction", [3, 5])
def test_direction(direction, interp):
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape, interpAlgo=interp, interpDirection=direction))
    check_tiles(blob, np.float32, (0, 1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))


@pytest.mark.parametrize("shape", [(65, 47, 130), (5, 9, 1100)], ids=["65x47x130", "5x9x1100"])
@pytest.mark.parametrize("anchor", [0, 4], ids=["stride0", "stride4"])
def test_anchor_strides(anchor, shape):
    """stride 4: k = 1 has anchors at every second coarse point, from k = 2 on every coarse point is an anchor; stride 0: the first point"""
    blob = container(smooth(shape), conf_for(shape, interpAnchorStride=anchor))
    check_tiles(blob, np.float32, (0, 1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))


def test_no_extent_above_the_default_stride():
    """20^3 under the 3-D default stride of 32: the first-point path at every level, down to the grid of one point"""
    shape = (20, 20, 20)
    blob = container(smooth(shape), conf_for(shape))
    check_tiles(blob, np.float32, (1, 2, 4, 5), algos=(sz3_amd.ALGO_HIP_INTERP,))


@pytest.mark.parametrize("shape", [(65, 47, 130), (33, 70), (5, 9, 1100)], ids=["65x47x130", "33x70", "5x9x1100"])
def test_stock_format(shape):
    sz3_amd.set_stock_format(1)
    try:
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    check_tiles(blob, np.float32, (0, 1, 2, 3, int(np.log2(DEF_ANCHOR[len(shape) - 1]))), algos=(sz3_amd.ALGO_INTERP,))


@pytest.mark.parametrize("stock", [0, 1], ids=["id17", "stock"])
def test_spikes(stock):
    """raw records inside and outside every window, on and off the coarse grid"""
    a, pos = spiky()
    sz3_amd.set_stock_format(stock)
    try:
        blob = container(a, conf_for(a.shape, algo=sz3_amd.ALGO_INTERP_LORENZO if stock else sz3_amd.ALGO_INTERP, quantbinCnt=256))
    finally:
        sz3_amd.set_stock_format(0)
    for k in (1, 2):
        on = (pos % (1 << k) == 0).all(axis=1)
        assert on.any() and (~on).any(), "spikes on and off the level-%d grid" % k
    full, _ = check_tiles(blob, np.float32, (0, 1, 2, 3), algos=(sz3_amd.ALGO_INTERP if stock else sz3_amd.ALGO_HIP_INTERP,))
    assert float(coarse_view(full, 2).max()) == 1e6


# ---- level shift: the per-level bound goes by the FULL array's level numbers -----------------------------------------------
@pytest.mark.parametrize("kw", [dict(interpAlpha=1.5, interpBeta=3.0), dict(interpAlpha=-1.0)], ids=["alpha1.5_beta3", "alpha-1"])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
def test_level_shift(kw, interp):
    """a tile's level b is the array's level b + k: with bounds that differ by level, a decoder that does not shift the numbers is off"""
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape, interpAlgo=interp, **kw))
    check_tiles(blob, np.float32, (1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))


# ---- the existing calls --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interp_case():
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == sz3_amd.ALGO_HIP_INTERP
    return blob, full, conf


def test_equals_the_region_and_the_coarse_decode(interp_case):
    blob, full, conf = interp_case
    for lo, ext in boxes_of(conf.dims):
        a, _ = sz3_amd.decompress_tile(blob, np.float32, 0, lo, ext, device=DEV)
        b, _ = sz3_amd.decompress_region(blob, np.float32, lo, ext, device=DEV)
        assert np.array_equal(raw(a), raw(b))
    for k in (1, 2, 3, 5):
        cd = sz3_amd.coarse_dims(conf, k)
        a, _ = sz3_amd.decompress_tile(blob, np.float32, k, (0,) * len(cd), cd, device=DEV)
        b, _ = sz3_amd.decompress_coarse(blob, np.float32, k, device=DEV)
        assert tuple(a.shape) == tuple(b.shape) and np.array_equal(raw(a), raw(b))


# ---- sparse decode really runs -------------------------------------------------------------------------------------------------
def small_boxes(shape):
    b = boxes_of(shape)
    return [b[1], b[2], b[3]]  # point, origin, far


@pytest.mark.parametrize("shape", [(65, 47, 130), (5, 9, 1100)], ids=["65x47x130", "5x9x1100"])
def test_sparse_decode_runs(shape):
    blob = container(smooth(shape), conf_for(shape))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == sz3_amd.ALGO_HIP_INTERP
    total = -(-int(np.prod(shape)) // 512)
    assert sz3_amd.get_sparse_decode()
    for k in (0, 1):
        cv = coarse_view(full, k)
        for lo, ext in small_boxes(tuple(cv.shape)):
            units = sz3_amd.tile_units(conf, k, lo, ext)
            plan = sz3_amd.tile_plan(conf, k, lo, ext)
            assert plan["units_total"] == total and plan["units_needed"] == units.size
            assert 2 * units.size <= total, "the case must be one the sparse stage takes (%d of %d units)" % (units.size, total)
            d0, t0 = sz3_amd.debug_tile_units()
            got, _ = sz3_amd.decompress_tile(blob, np.float32, k, lo, ext, device=DEV)
            d1, t1 = sz3_amd.debug_tile_units()
            assert (d1 - d0, t1 - t0) == (units.size, total) and d1 - d0 < t1 - t0
            want = raw(cv[box_slices(lo, ext)])
            assert np.array_equal(raw(got), want)
            sz3_amd.set_sparse_decode(0)
            try:
                dense, _ = sz3_amd.decompress_tile(blob, np.float32, k, lo, ext, device=DEV)
            finally:
                sz3_amd.set_sparse_decode(1)
            d2, t2 = sz3_amd.debug_tile_units()
            assert (d2 - d1, t2 - t1) == (total, total), "switched off: every unit"
            assert np.array_equal(raw(dense), want)
    # the whole array as box: dense
    d0, t0 = sz3_amd.debug_tile_units()
    got, _ = sz3_amd.decompress_tile(blob, np.float32, 0, (0,) * len(shape), shape, device=DEV)
    d1, t1 = sz3_amd.debug_tile_units()
    assert (d1 - d0, t1 - t0) == (total, total) and np.array_equal(raw(got), raw(full))


def test_stock_streams_decode_every_unit():
    shape = (65, 47, 130)
    sz3_amd.set_stock_format(1)
    try:
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == sz3_amd.ALGO_INTERP
    total = -(-int(np.prod(shape)) // 512)
    for lo, ext in small_boxes(shape):
        d0, t0 = sz3_amd.debug_tile_units()
        got, _ = sz3_amd.decompress_tile(blob, np.float32, 0, lo, ext, device=DEV)
        d1, t1 = sz3_amd.debug_tile_units()
        assert (d1 - d0, t1 - t0) == (total, total)
        assert np.array_equal(raw(got), raw(full[box_slices(lo, ext)]))


# ---- stale codes: the units that are not decoded keep what the code array held ---------------------------------------------------
def ctx_tile(dc, pl, size, k, lo, ext):
    out = torch.full(tuple(ext), 77.0, dtype=torch.float32, device=DEV)
    dc.decompress_tile(pl.data_ptr(), size, k, lo, ext, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def test_stale_codes():
    """one context, two containers of the same shape: a unit the list misses shows up as the other container's codes"""
    shape = (65, 47, 130)
    conf = conf_for(shape)
    a, b = smooth(shape, seed=7), (smooth(shape, seed=8)[::-1, ::-1, ::-1] * 1.7).copy()
    dc = sz3_amd.DeviceCompressor(a.size, a.dtype)
    cap = dc.payload_bound(a.size, worst_case=True)
    s = torch.cuda.current_stream().cuda_stream
    pls, sizes, fulls = [], [], []
    for x in (a, b):
        t = torch.from_numpy(x).to(DEV)
        pl = torch.empty(cap, dtype=torch.uint8, device=DEV)
        sizes.append(dc.compress(conf, t.data_ptr(), pl.data_ptr(), cap, s))
        full = torch.empty_like(t)
        dc.decompress(pl.data_ptr(), sizes[-1], full.data_ptr(), s)
        torch.cuda.synchronize()
        pls.append(pl)
        fulls.append(full)
    assert not np.array_equal(raw(fulls[0]), raw(fulls[1]))
    scratch = torch.empty_like(fulls[0])
    for k in (0, 1, 2):
        boxes = tile_boxes(coarse_shape(shape, k))[1:]
        for first, second in ((1, 0), (0, 1)):  # the other container's full decode, then this one's tiles
            for lo, ext in boxes:
                dc.decompress(pls[first].data_ptr(), sizes[first], scratch.data_ptr(), s)
                d0, t0 = sz3_amd.debug_tile_units()
                got = ctx_tile(dc, pls[second], sizes[second], k, lo, ext)
                d1, t1 = sz3_amd.debug_tile_units()
                assert d1 - d0 == sz3_amd.tile_plan(conf, k, lo, ext)["units_needed"] < t1 - t0, "the case must leave units undecoded"
                assert np.array_equal(raw(got), raw(coarse_view(fulls[second], k)[box_slices(lo, ext)])), (k, lo, ext)
        # two different boxes of one container back to back, in both orders
        for x, y in ((boxes[0], boxes[2]), (boxes[2], boxes[1]), (boxes[3], boxes[0])):
            for lo, ext in (x, y):
                got = ctx_tile(dc, pls[0], sizes[0], k, lo, ext)
                assert np.array_equal(raw(got), raw(coarse_view(fulls[0], k)[box_slices(lo, ext)])), (k, lo, ext)


# ---- fallback containers: the full decode, then the strided gather of the view -------------------------------------------------
@pytest.mark.parametrize("name,kw", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_fallback_containers(name, kw):
    """(an anchor stride that is no power of two takes this path too, but no such container can be written here: the compressor refuses the
    stride. tests/test_tile_cpu.py checks the plan's SZ3HIP_EUNSUPPORTED, which is what sends the to-device call here)"""
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **kw))
    _, conf = check_fallback(blob)
    assert conf.cmprAlgo not in INTERP_IDS
    if name == "lossless":
        assert conf.cmprAlgo == sz3_amd.ALGO_LOSSLESS


def check_fallback(blob):
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    for k, lo, ext in ((0, (3, 7, 11), (20, 9, 30)), (1, (1, 3, 5), (10, 9, 20)), (2, (0, 0, 0), coarse_shape(conf.dims, 2)), (3, (4, 5, 6), (1, 1, 1))):
        before = L.sz3hip_debug_region_fast_calls()
        got, c2 = sz3_amd.decompress_tile(blob, np.float32, k, lo, ext, device=DEV)
        assert L.sz3hip_debug_region_fast_calls() == before, "the fallback is no fast call"
        assert c2.dims == conf.dims
        assert np.array_equal(raw(got), raw(coarse_view(full, k)[box_slices(lo, ext)])), (k, lo, ext)
    return full, conf


def test_fallback_openmp_slabs(monkeypatch):
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    shape = (50, 30, 40)
    blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, openmp=1))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.openmp
    for k, lo, ext in ((0, (11, 3, 5), (30, 20, 17)), (1, (5, 1, 2), (15, 10, 9)), (2, (0, 0, 0), coarse_shape(shape, 2))):
        before = L.sz3hip_debug_region_fast_calls()
        got, _ = sz3_amd.decompress_tile(blob, np.float32, k, lo, ext, device=DEV)
        assert L.sz3hip_debug_region_fast_calls() == before
        assert np.array_equal(raw(got), raw(coarse_view(full, k)[box_slices(lo, ext)])), (k, lo, ext)


# ---- views, streams, pointers --------------------------------------------------------------------------------------------------
TILE = (1, (3, 4, 14), (10, 6, 20))


@pytest.mark.parametrize("which", ["interp", "lorenzo"])
def test_out_is_a_strided_view(interp_case, which):
    if which == "interp":
        blob, full, conf = interp_case
    else:
        shape = (65, 47, 130)
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0))
        full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    k, lo, ext = TILE
    big = torch.full(tuple(d + 3 for d in ext), 77.0, dtype=torch.float32, device=DEV)
    inner = tuple(slice(1, 1 + d) for d in ext)
    out, _ = sz3_amd.decompress_tile(blob, np.float32, k, lo, ext, out=big[inner])
    assert out.data_ptr() == big[inner].data_ptr()
    got = big.cpu().numpy()
    assert np.array_equal(got[inner].reshape(-1).view(np.uint8), raw(coarse_view(full, k)[box_slices(lo, ext)]))
    mask = np.ones(got.shape, bool)
    mask[inner] = False
    assert (got[mask] == 77).all(), "elements outside the view were written"


def test_non_default_stream(interp_case):
    blob, full, conf = interp_case
    k, lo, ext = TILE
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = torch.empty(ext, dtype=torch.float32, device=DEV)
        out.fill_(77.0)
        sz3_amd.decompress_tile(blob, np.float32, k, lo, ext, out=out, stream=side)
    torch.cuda.synchronize()
    assert np.array_equal(raw(out), raw(coarse_view(full, k)[box_slices(lo, ext)]))


def test_host_pointer_and_bad_boxes_are_refused_before_any_launch(interp_case):
    blob, _, conf = interp_case
    k, lo, ext = TILE

    def call(level, lo, ext, ptr):
        c = sz3_amd.Config(1)
        return L.sz3hip_decompress_tile_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, level, (C.c_uint64 * 4)(*lo), (C.c_uint64 * 4)(*ext), ptr, None, None)

    host = np.full(ext, 77, np.float32)
    before = L.sz3hip_debug_region_fast_calls()
    assert call(k, lo, ext, host.ctypes.data) == CODES["SZ3HIP_EINVAL"] and "device memory" in L.sz3hip_last_error().decode()
    assert (host == 77).all()
    out = torch.full(ext, 77.0, dtype=torch.float32, device=DEV)
    assert call(k, (30, 0, 0), (4, 4, 4), out.data_ptr()) == CODES["SZ3HIP_EINVAL"] and "dimension 0" in L.sz3hip_last_error().decode()  # (33 coarse planes)
    assert call(31, lo, ext, out.data_ptr()) == CODES["SZ3HIP_EINVAL"] and "level" in L.sz3hip_last_error().decode()
    assert call(k, lo, (10, 0, 20), out.data_ptr()) == CODES["SZ3HIP_EINVAL"] and "dimension 1" in L.sz3hip_last_error().decode()
    assert L.sz3hip_debug_region_fast_calls() == before and bool((out == 77).all())
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.decompress_tile(blob, np.int32, k, lo, ext, out=torch.full(ext, 77, dtype=torch.int32, device=DEV))
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"]


# ---- device context ------------------------------------------------------------------------------------------------------------
def test_device_context_and_its_scratch():
    shape = (65, 47, 130)
    conf = conf_for(shape)
    dc, pl, size, full = device_payload(smooth(shape), conf)
    assert dc.region_scratch() == 0
    out = torch.full((4, 4, 4), 77.0, dtype=torch.float32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for k, lo, ext, what in ((1, (0, 0, 62), (4, 4, 4), "dimension 2"), (2, (17, 0, 0), (1, 4, 4), "dimension 0"), (1, (1, 1, 1), (4, 0, 4), "dimension 1"),
                             (31, (0, 0, 0), (1, 1, 1), "level"), (-1, (0, 0, 0), (1, 1, 1), "level")):
        with pytest.raises(sz3_amd.SZ3HipError) as e:
            dc.decompress_tile(pl.data_ptr(), size, k, lo, ext, out.data_ptr(), s)
        assert e.value.code == CODES["SZ3HIP_EINVAL"] and what in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and dc.region_scratch() == 0
    k, lo, ext = TILE
    plan = sz3_amd.tile_plan(conf, k, lo, ext)
    got = ctx_tile(dc, pl, size, k, lo, ext)
    assert np.array_equal(raw(got), raw(coarse_view(full, k)[box_slices(lo, ext)]))
    cap = dc.region_scratch()
    assert cap >= plan["region"]["scratch_elems"] > 0
    # the same plan again, then smaller ones at other levels: nothing is allocated
    for k2, lo2, ext2 in (TILE, (2, (8, 5, 16), (1, 1, 1)), (0, (31, 21, 63), (2, 2, 2)), (5, (0, 0, 0), coarse_shape(shape, 5))):
        assert sz3_amd.tile_plan(conf, k2, lo2, ext2)["region"]["scratch_elems"] <= cap
        got = ctx_tile(dc, pl, size, k2, lo2, ext2)
        assert np.array_equal(raw(got), raw(coarse_view(full, k2)[box_slices(lo2, ext2)])) and dc.region_scratch() == cap
    after = torch.empty_like(full)  # (the full decode of the same context is what it was)
    dc.decompress(pl.data_ptr(), size, after.data_ptr(), s)
    torch.cuda.synchronize()
    assert np.array_equal(raw(after), raw(full))


def test_device_context_refuses_a_lorenzo_payload():
    shape = (40, 48, 56)
    out = torch.full((4, 4, 4), 77.0, dtype=torch.float32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    dc, pl, size, _ = device_payload(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0))
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        dc.decompress_tile(pl.data_ptr(), size, 1, (1, 1, 1), (4, 4, 4), out.data_ptr(), s)
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"]
    torch.cuda.synchronize()
    assert bool((out == 77).all())


# ---- a failed partial call leaves nothing behind on its thread -----------------------------------------------------------------
def test_a_failed_partial_call_leaves_nothing_installed():
    """one thread. A coarse, a region and a tile call of a blob cut 40 bytes short each return an error (the trailer's: the call ends at
    its peek). The same three calls of a blob whose trailer is intact and whose lossless block states one byte more than it holds: the peek
    passes and the call fails inside the decode, in libzstd's check, where the thread's output view and partial request are installed.
    After all six, the full decode of the intact blob on that thread — into device memory and into a host array — is the reference full
    decode, bit for bit, and a tile call of it its slice"""
    shape = (33, 20, 17)
    blob = container(smooth(shape), conf_for(shape))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo in INTERP_IDS
    k, lo, ext = 1, (3, 2, 1), (9, 5, 6)

    def calls(b):
        return (lambda: sz3_amd.decompress_coarse(b, np.float32, 1, device=DEV),
                lambda: sz3_amd.decompress_region(b, np.float32, lo, ext, device=DEV),
                lambda: sz3_amd.decompress_tile(b, np.float32, k, lo, ext, device=DEV))

    for call in calls(blob[:-40].copy()):
        with pytest.raises(sz3_amd.SZ3HipError) as e:
            call()
        assert e.value.code < 0
    bad = blob.copy()  # [magic, version][u64 payload bytes][u64 length of the lossless block's content][zstd frames][Config]
    bad[16:24] = np.array([int(bad[16:24].view(np.uint64)[0]) + 1], np.uint64).view(np.uint8)
    c = sz3_amd.Config(1)
    assert L.sz3hip_peek_config(C.byref(c._c), bad.ctypes.data, bad.size) == 0 and c.dims == conf.dims, "the peek must pass: the decode is what fails"
    for call in calls(bad):
        before = L.sz3hip_debug_region_fast_calls()
        with pytest.raises(sz3_amd.SZ3HipError) as e:
            call()
        assert e.value.code == CODES["SZ3HIP_EZSTD"] and "ZSTD_decompress" in str(e.value), "the error must be the decode's, not the peek's"
        assert L.sz3hip_debug_region_fast_calls() == before
    again, c2 = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert tuple(again.shape) == shape == c2.dims and np.array_equal(raw(again), raw(full))
    host, _ = sz3_amd.decompress(blob, np.float32, shape)
    assert np.array_equal(host.reshape(-1).view(np.uint8), raw(full)), "a host decode on this thread must land in its host array"
    got, _ = sz3_amd.decompress_tile(blob, np.float32, k, lo, ext, device=DEV)
    assert np.array_equal(raw(got), raw(coarse_view(full, k)[box_slices(lo, ext)]))

"""Several tiles of one stream in one call on the MI355X: every box of decompress_tiles(blob, dtype, k, boxes) — and of the
device context's call — is, bit for bit, decompress(blob, dtype)[::2**k, ...][box]. One call carries boxes of very different sizes (the whole
grid and a single point share every launch), so a workgroup that runs past its own box's total, or skips a box that has points, shows.
The one assertion on values everywhere is raw-byte identity with the full decode's slice; there are no tolerances. Fields, bound and the 1024
quantisation bins are partial_cases.py's, the shapes test_gpu_tile.py's."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, boxes_of, conf_for, container, device_payload, raw, smooth, spiky  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
DEF_ANCHOR = (4096, 128, 32, 16)
SENTINEL = 77.0


def coarse_shape(shape, k):
    return tuple(((d - 1) >> k) + 1 for d in shape)


def coarse_view(full, k):
    return full[tuple(slice(None, None, 1 << k) for _ in full.shape)]


def tile_boxes(shape):
    """boxes_of(shape) clipped to the grid (test_gpu_tile.py's): whole, point, origin, far, straddle, slab"""
    out = []
    for lo, ext in boxes_of(shape):
        lo = tuple(min(max(a, 0), d - 1) for a, d in zip(lo, shape))
        out.append((lo, tuple(max(1, min(e, d - a)) for e, d, a in zip(ext, shape, lo))))
    return out


def request(shape):
    """all six boxes of the grid and the point box a second time"""
    b = tile_boxes(shape)
    return b + [b[1]]


def same(outs, full, k, boxes, what=""):
    cv = coarse_view(full, k)
    assert len(outs) == len(boxes)
    for i, (got, (lo, ext)) in enumerate(zip(outs, boxes)):
        want = cv[box_slices(lo, ext)]
        assert tuple(got.shape) == tuple(ext) == tuple(want.shape)
        assert np.array_equal(raw(got), raw(want)), "%s level %d: box %d (lo %s shape %s) differs from the full decode's slice" % (what, k, i, lo, ext)


def ctx_tiles(dc, pl, size, k, boxes, dtype=torch.float32, sync=True):
    outs = [torch.full(tuple(ext), SENTINEL, dtype=dtype, device=DEV) for _, ext in boxes]
    dc.decompress_tiles(pl.data_ptr(), size, k, boxes, [o.data_ptr() for o in outs], torch.cuda.current_stream().cuda_stream)
    if sync:
        torch.cuda.synchronize()
    return outs


def check_container(blob, dtype, levels, algos=None, full=None, boxes=request):
    if full is None:
        full, conf = sz3_amd.decompress(blob, dtype, device=DEV)
    else:
        conf = sz3_amd.Config(1)
        assert L.sz3hip_peek_config(C.byref(conf._c), blob.ctypes.data, blob.size) == 0
    if algos is not None:
        assert conf.cmprAlgo in algos, "the case must be a lossy interpolation stream (cmprAlgo %d)" % conf.cmprAlgo
    fast = conf.cmprAlgo in INTERP_IDS and not conf.openmp
    for k in levels:
        bx = boxes(coarse_shape(conf.dims, k))
        before = L.sz3hip_debug_region_fast_calls()
        outs, c2 = sz3_amd.decompress_tiles(blob, dtype, k, bx, device=DEV)
        assert L.sz3hip_debug_region_fast_calls() - before == (1 if fast else 0), "one fast call per multi-box call, none on the fallback"
        assert c2.dims == conf.dims, "conf must stay the full array's"
        same(outs, full, k, bx, "container")
    return full, conf


def check_context(a, conf, levels, boxes=request):
    dc, pl, size, full = device_payload(a, conf)
    for k in levels:
        bx = boxes(coarse_shape(a.shape, k))
        same(ctx_tiles(dc, pl, size, k, bx, dtype=getattr(torch, a.dtype.name)), full, k, bx, "context")
    return dc, pl, size, full


# ---- 1. bit identity ---------------------------------------------------------------------------------------------------------------
SHAPES = [(65, 47, 130), (33, 70), (1000,), (9, 12, 17, 20), (5, 9, 1100)]


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bit_identity(shape, dtype, interp):
    """k = 0 .. 3 and the k whose stride is the default anchor stride, through the container call and through the device context"""
    a = smooth(shape, dtype)
    conf = conf_for(shape, interpAlgo=interp)
    levels = (0, 1, 2, 3, int(np.log2(DEF_ANCHOR[len(shape) - 1])))
    check_container(container(a, conf), np.dtype(dtype), levels, algos=None if shape == (1000,) else (sz3_amd.ALGO_HIP_INTERP,))
    check_context(a, conf, levels)


# ---- 2. paths inside the tile decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("direction", [3, 5])
def test_direction(direction, interp):
    shape = (65, 47, 130)
    a, conf = smooth(shape), conf_for(shape, interpAlgo=interp, interpDirection=direction)
    check_container(container(a, conf), np.float32, (0, 1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))
    check_context(a, conf, (0, 2))


@pytest.mark.parametrize("shape", [(65, 47, 130), (5, 9, 1100)], ids=["65x47x130", "5x9x1100"])
@pytest.mark.parametrize("anchor", [0, 4], ids=["stride0", "stride4"])
def test_anchor_strides(anchor, shape):
    """stride 4: from k = 2 on every coarse point is an anchor and no level runs; stride 0: the first point"""
    a, conf = smooth(shape), conf_for(shape, interpAnchorStride=anchor)
    check_container(container(a, conf), np.float32, (0, 1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))
    check_context(a, conf, (0, 1, 2, 3))


def test_first_point_for_some_boxes_only():
    """20^3 under the default stride of 32: the first-point path. The origin corner box and the far box in one call: the first-point launch
    runs, for some boxes only"""
    shape = (20, 20, 20)
    a, conf = smooth(shape), conf_for(shape)

    def boxes(cs):
        b = tile_boxes(cs)
        return [b[3], b[2], b[1], b[3], b[0]]  # far, origin, point, far again, whole

    check_container(container(a, conf), np.float32, (0, 1, 2, 4, 5), algos=(sz3_amd.ALGO_HIP_INTERP,), boxes=boxes)
    check_context(a, conf, (0, 1, 2, 4, 5), boxes=boxes)


@pytest.mark.parametrize("kw", [dict(interpAlpha=1.5, interpBeta=3.0), dict(interpAlpha=-1.0)], ids=["alpha1.5_beta3", "alpha-1"])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
def test_level_shift(kw, interp):
    shape = (65, 47, 130)
    a, conf = smooth(shape), conf_for(shape, interpAlgo=interp, **kw)
    check_container(container(a, conf), np.float32, (1, 2, 3), algos=(sz3_amd.ALGO_HIP_INTERP,))
    check_context(a, conf, (1, 2, 3))


# ---- 3. raw records ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stock", [0, 1], ids=["id17", "stock"])
def test_spikes(stock):
    """raw records inside some boxes' windows and outside others', on and off the coarse grid"""
    a, pos = spiky()
    sz3_amd.set_stock_format(stock)
    try:
        blob = container(a, conf_for(a.shape, algo=sz3_amd.ALGO_INTERP_LORENZO if stock else sz3_amd.ALGO_INTERP, quantbinCnt=256))
    finally:
        sz3_amd.set_stock_format(0)
    for k in (1, 2):
        on = (pos % (1 << k) == 0).all(axis=1)
        assert on.any() and (~on).any(), "spikes on and off the level-%d grid" % k
    full, _ = check_container(blob, np.float32, (0, 1, 2, 3), algos=(sz3_amd.ALGO_INTERP if stock else sz3_amd.ALGO_HIP_INTERP,))
    inside = [int((raw(full[box_slices(lo, ext)]).view(np.float32) == 1e6).sum()) for lo, ext in request(a.shape)]
    assert max(inside) > 0 and min(inside) == 0, "spikes inside some boxes and outside others (%s)" % inside
    if not stock:
        check_context(a, conf_for(a.shape, quantbinCnt=256), (0, 1, 2))


# ---- 4. stock ALGO_INTERP containers: every unit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 47, 130), (33, 70), (5, 9, 1100)], ids=["65x47x130", "33x70", "5x9x1100"])
def test_stock_format(shape):
    sz3_amd.set_stock_format(1)
    try:
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    full, conf = check_container(blob, np.float32, (0, 1, 2, 3, int(np.log2(DEF_ANCHOR[len(shape) - 1]))), algos=(sz3_amd.ALGO_INTERP,))
    total = -(-int(np.prod(shape)) // 512)
    bx = request(shape)[1:]
    d0, t0 = sz3_amd.debug_tile_units()
    outs, _ = sz3_amd.decompress_tiles(blob, np.float32, 0, bx, device=DEV)
    d1, t1 = sz3_amd.debug_tile_units()
    assert (d1 - d0, t1 - t0) == (total, total), "a stock stream's codes come through the stock decoder: every unit, once per call"
    same(outs, full, 0, bx)


# ---- 5. the union list ---------------------------------------------------------------------------------------------------------------
def small_boxes(shape):
    b = tile_boxes(shape)
    return [b[1], b[2], b[3], b[4], b[5]]  # point, origin, far, straddle, slab


def test_union_list():
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == sz3_amd.ALGO_HIP_INTERP
    total = -(-int(np.prod(shape)) // 512)
    assert total == 776 and sz3_amd.get_sparse_decode()
    for k, expect in ((0, 369), (1, 245), (2, 133)):
        bx = small_boxes(coarse_shape(shape, k))
        plan = sz3_amd.tiles_plan(conf, k, bx)
        union = set()
        for lo, ext in bx:
            union.update(int(u) for u in sz3_amd.tile_units(conf, k, lo, ext))
        assert plan["units_needed"] == len(union) == expect and plan["units_total"] == total
        assert 2 * plan["units_needed"] <= total, "the case must be one the list form takes"
        d0, t0 = sz3_amd.debug_tile_units()
        outs, _ = sz3_amd.decompress_tiles(blob, np.float32, k, bx, device=DEV)
        d1, t1 = sz3_amd.debug_tile_units()
        assert (d1 - d0, t1 - t0) == (plan["units_needed"], total), "one list launch over the union"
        same(outs, full, k, bx)
        sz3_amd.set_sparse_decode(0)
        try:
            dense, _ = sz3_amd.decompress_tiles(blob, np.float32, k, bx, device=DEV)
        finally:
            sz3_amd.set_sparse_decode(1)
        d2, t2 = sz3_amd.debug_tile_units()
        assert (d2 - d1, t2 - t1) == (total, total), "switched off: every unit"
        for x, y in zip(outs, dense):
            assert np.array_equal(raw(x), raw(y))


def test_union_beyond_the_limit_is_dense():
    """(5, 9, 1100), k = 0: origin and far need 40 / 41 of 97 units, each within the limit of 48 — their union, 71, is not"""
    shape = (5, 9, 1100)
    blob = container(smooth(shape), conf_for(shape))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == sz3_amd.ALGO_HIP_INTERP
    b = tile_boxes(shape)
    bx = [b[2], b[3]]
    total = 97
    singles = [sz3_amd.tile_plan(conf, 0, lo, ext)["units_needed"] for lo, ext in bx]
    plan = sz3_amd.tiles_plan(conf, 0, bx)
    assert singles == [40, 41] and plan["units_needed"] == 71 and plan["units_total"] == total
    for (lo, ext), need in zip(bx, singles):
        d0, t0 = sz3_amd.debug_tile_units()
        got, _ = sz3_amd.decompress_tile(blob, np.float32, 0, lo, ext, device=DEV)
        d1, t1 = sz3_amd.debug_tile_units()
        assert (d1 - d0, t1 - t0) == (need, total), "alone, each box is sparse"
    d0, t0 = sz3_amd.debug_tile_units()
    outs, _ = sz3_amd.decompress_tiles(blob, np.float32, 0, bx, device=DEV)
    d1, t1 = sz3_amd.debug_tile_units()
    assert (d1 - d0, t1 - t0) == (total, total), "dense by the union"
    same(outs, full, 0, bx)


# ---- 6. stale codes on the context ---------------------------------------------------------------------------------------------------
def test_stale_codes():
    """one context, two containers of one shape: a full decode of A, then the five-box call on B. A union list that misses a read shows A's codes"""
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
        bx = small_boxes(coarse_shape(shape, k))
        need = sz3_amd.tiles_plan(conf, k, bx)["units_needed"]
        for first, second in ((1, 0), (0, 1)):
            dc.decompress(pls[first].data_ptr(), sizes[first], scratch.data_ptr(), s)
            d0, t0 = sz3_amd.debug_tile_units()
            outs = ctx_tiles(dc, pls[second], sizes[second], k, bx)
            d1, t1 = sz3_amd.debug_tile_units()
            assert d1 - d0 == need < t1 - t0, "the case must leave units undecoded"
            same(outs, fulls[second], k, bx, "after the other container's full decode,")


# ---- 7. the launch count does not grow with n ------------------------------------------------------------------------------------------
def test_launch_count():
    shape = (65, 47, 130)
    dc, pl, size, full = device_payload(smooth(shape), conf_for(shape, interpAlgo=0))  # (linear, N = 3: two launches per pass)
    for k in (0, 1):
        straddle = tile_boxes(coarse_shape(shape, k))[4]
        l0 = L.sz3hip_debug_region_launches()
        one = ctx_tiles(dc, pl, size, k, [straddle])
        l1 = L.sz3hip_debug_region_launches()
        nine = ctx_tiles(dc, pl, size, k, [straddle] * 9)
        l2 = L.sz3hip_debug_region_launches()
        assert l1 - l0 > 0 and l2 - l1 == l1 - l0, "nine boxes: %d launches, one box: %d" % (l2 - l1, l1 - l0)
        same(one, full, k, [straddle])
        same(nine, full, k, [straddle] * 9)
        out = torch.empty(straddle[1], dtype=torch.float32, device=DEV)
        dc.decompress_tile(pl.data_ptr(), size, k, straddle[0], straddle[1], out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert L.sz3hip_debug_region_launches() - l2 == l1 - l0, "the single-box call counts its launches too: one box's sequence"


# ---- 8. the context's scratch and table ------------------------------------------------------------------------------------------------
def test_context_scratch_and_back_to_back_calls():
    shape = (65, 47, 130)
    conf = conf_for(shape)
    dc, pl, size, full = device_payload(smooth(shape), conf)
    assert dc.region_scratch() == 0
    k = 1
    b = tile_boxes(coarse_shape(shape, k))
    nine = [b[4], b[2], b[3], b[5], b[1], b[4], b[2], b[3], b[5]]
    plan = sz3_amd.tiles_plan(conf, k, nine)
    outs = ctx_tiles(dc, pl, size, k, nine)
    same(outs, full, k, nine)
    cap = dc.region_scratch()
    assert cap >= plan["scratch_elems"] > max(sz3_amd.tile_plan(conf, k, lo, ext)["region"]["scratch_elems"] for lo, ext in nine)
    three = [b[1], b[3], b[2]]
    assert sz3_amd.tiles_plan(conf, k, three)["scratch_elems"] <= cap
    outs3 = ctx_tiles(dc, pl, size, k, three)
    assert dc.region_scratch() == cap, "a request that fits allocates nothing: the scratch is kept as it is"
    same(outs3, full, k, three)
    # two calls back to back on one stream, no host synchronisation in between, different boxes: the second call's table must not reach the
    # pinned array before the first call's copy has read it
    for _ in range(3):
        x = ctx_tiles(dc, pl, size, k, nine, sync=False)
        y = ctx_tiles(dc, pl, size, 0, tile_boxes(shape)[1:], sync=False)
        z = ctx_tiles(dc, pl, size, k, three, sync=False)
        torch.cuda.synchronize()
        same(x, full, k, nine)
        same(y, full, 0, tile_boxes(shape)[1:])
        same(z, full, k, three)


# ---- 9. fallback containers: one full decode, n gathers ----------------------------------------------------------------------------
FB_BOXES = {0: [((3, 7, 11), (20, 9, 30)), ((0, 0, 0), (1, 1, 1)), ((3, 7, 11), (20, 9, 30))], 1: [((1, 3, 5), (10, 9, 20)), ((19, 23, 27), (1, 1, 1))],
            2: [((0, 0, 0), (10, 12, 14)), ((4, 5, 6), (1, 1, 1))], 3: [((4, 5, 6), (1, 1, 1)), ((0, 0, 0), (5, 6, 7))]}


@pytest.mark.parametrize("name,kw", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_fallback_containers(name, kw):
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **kw))
    _, conf = check_container(blob, np.float32, (0, 1, 2, 3), boxes=lambda cs: FB_BOXES[{40: 0, 20: 1, 10: 2, 5: 3}[cs[0]]])
    assert conf.cmprAlgo not in INTERP_IDS


def test_fallback_openmp_slabs(monkeypatch):
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    shape = (50, 30, 40)
    blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, openmp=1))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.openmp
    check_container(blob, np.float32, (0, 1, 2), full=full)


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------
def test_a_bad_box_refuses_the_whole_call():
    shape = (65, 47, 130)
    conf = conf_for(shape)
    a = smooth(shape)
    blob = container(a, conf)
    dc, pl, size, full = device_payload(a, conf)
    k = 1
    b = tile_boxes(coarse_shape(shape, k))
    good = [b[2], b[4], b[1], b[3]]
    bad = list(good)
    bad[2] = ((30, 0, 0), (4, 4, 4))  # (33 coarse planes)
    outs = [torch.full(tuple(ext), SENTINEL, dtype=torch.float32, device=DEV) for _, ext in bad]
    before = L.sz3hip_debug_region_fast_calls()
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.decompress_tiles(blob, np.float32, k, bad, out=outs)
    assert e.value.code == CODES["SZ3HIP_EINVAL"] and "box 2" in str(e.value) and "dimension 0" in str(e.value)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        dc.decompress_tiles(pl.data_ptr(), size, k, bad, [o.data_ptr() for o in outs], torch.cuda.current_stream().cuda_stream)
    assert e.value.code == CODES["SZ3HIP_EINVAL"] and "box 2" in str(e.value) and "dimension 0" in str(e.value)
    with pytest.raises(sz3_amd.SZ3HipError) as e:  # outputs that overlap one another
        dc.decompress_tiles(pl.data_ptr(), size, k, good, [outs[0].data_ptr(), outs[1].data_ptr(), outs[0].data_ptr() + 4, outs[3].data_ptr()],
                            torch.cuda.current_stream().cuda_stream)
    assert e.value.code == CODES["SZ3HIP_EINVAL"] and "overlap" in str(e.value)
    torch.cuda.synchronize()
    assert L.sz3hip_debug_region_fast_calls() == before
    assert all(bool((o == SENTINEL).all()) for o in outs), "a refused call writes nothing"
    # after the refused calls the next good ones are right
    got, _ = sz3_amd.decompress_tiles(blob, np.float32, k, good, device=DEV)
    same(got, full, k, good)
    same(ctx_tiles(dc, pl, size, k, good), full, k, good)


def test_device_context_refuses_a_lorenzo_payload():
    shape = (40, 48, 56)
    dc, pl, size, full = device_payload(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0))
    bx = [((1, 1, 1), (4, 4, 4)), ((0, 0, 0), (2, 2, 2))]
    outs = [torch.full(ext, SENTINEL, dtype=torch.float32, device=DEV) for _, ext in bx]
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        dc.decompress_tiles(pl.data_ptr(), size, 1, bx, [o.data_ptr() for o in outs], torch.cuda.current_stream().cuda_stream)
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"]
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)
    after = torch.empty_like(full)
    dc.decompress(pl.data_ptr(), size, after.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(raw(after), raw(full))


# ---- 11. a stream that is not the default ------------------------------------------------------------------------------------------
def test_non_default_stream():
    shape = (65, 47, 130)
    blob = container(smooth(shape), conf_for(shape))
    full, _ = sz3_amd.decompress(blob, np.float32, device=DEV)
    k = 1
    bx = request(coarse_shape(shape, k))[1:]
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        outs = [torch.empty(ext, dtype=torch.float32, device=DEV) for _, ext in bx]
        for o in outs:
            o.fill_(SENTINEL)
        sz3_amd.decompress_tiles(blob, np.float32, k, bx, out=outs, stream=side)
    torch.cuda.synchronize()
    same(outs, full, k, bx)

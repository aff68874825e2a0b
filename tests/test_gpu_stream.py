"""The opened stream on the MI355X: a handle does the Huffman stage once, at open, and every box of every later request —
through open_stream(blob) and through DeviceCompressor.open_stream(payload) — is, bit for bit, decompress(...)[::2**k, ...][box]. The one
assertion on values everywhere is raw-byte identity with the full decode's slice; there are no tolerances. Fields, bound and the 1024
quantisation bins are partial_cases.py's, the shapes and the request (the six boxes plus the point twice: the whole grid and a single point share
every launch) test_gpu_multibox.py's."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, boxes_of, conf_for, container, device_payload, raw, smooth, spiky  # noqa: E402
from sink_models import coarse_shape, coarse_view  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
SENTINEL = 77.0
CHAIN_DEFAULT = sz3_amd.get_chain_points()
SHAPES = [(65, 47, 130), (33, 70), (1000,), (9, 12, 17, 20), (5, 9, 1100)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def tile_boxes(shape):
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


@functools.lru_cache(maxsize=None)
def case(shape, dtype="float32", kw=()):
    """one field, its container and the container's full decode — made once, shared, never written"""
    a = smooth(shape, dtype)
    conf = conf_for(shape, **dict(kw))
    blob = container(a, conf)
    full, c2 = sz3_amd.decompress(blob, np.dtype(dtype), device=DEV)
    return a, blob, full, c2


def opens(shape, dtype="float32", kw=(), payload=True):
    """(name, Stream, the full decode it must match): the container's handle and the handle of a device context's payload of the same field"""
    a, blob, full, conf = case(shape, dtype, kw)
    yield "open_stream", sz3_amd.open_stream(blob, np.dtype(dtype), device=DEV), full
    if payload:
        dc, pl, size, pfull = device_payload(a, conf_for(shape, **dict(kw)))
        st = dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream)
        pl.zero_()  # (the handle owns what it reads)
        dc.close()
        yield "open_payload", st, pfull


def ask(st, k, boxes, sync=True, stream=None):
    outs = [torch.full(tuple(ext), SENTINEL, dtype=getattr(torch, st.dtype.name), device=DEV) for _, ext in boxes]
    st.tiles(k, boxes, out=outs, stream=stream)
    if sync:
        torch.cuda.synchronize()
    return outs


def check(shape, dtype="float32", kw=(), levels=(0, 1, 2), payload=True):
    algo = case(shape, dtype, kw)[3].cmprAlgo
    assert shape == (1000,) or algo == sz3_amd.ALGO_HIP_INTERP, "the case must be a lossy interpolation stream (cmprAlgo %d)" % algo
    for name, st, full in opens(shape, dtype, kw, payload):
        fast = name == "open_payload" or algo in INTERP_IDS  # (a context's payload of these Configs is an interpolation payload)
        with st:
            assert st.conf.dims == tuple(shape)
            for k in levels:
                bx = request(coarse_shape(shape, k))
                same(ask(st, k, bx), full, k, bx, name)
            s = st.stats()
            assert s["fast"] == (1 if fast else 0) and s["requests"] == len(levels)
            assert s["huffman_stages"] == (1 if fast else 0) and s["units_total"] == -(-int(np.prod(shape)) // 512)


# ---- 1. bit identity, through both opens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bit_identity(shape, dtype, interp):
    check(shape, dtype, (("interpAlgo", interp),))


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("direction", [3, 5])
def test_direction(direction, interp):
    check((65, 47, 130), kw=(("interpAlgo", interp), ("interpDirection", direction)))


@pytest.mark.parametrize("shape", [(65, 47, 130), (5, 9, 1100)], ids=["65x47x130", "5x9x1100"])
@pytest.mark.parametrize("anchor", [0, 4], ids=["stride0", "stride4"])
def test_anchor_strides(anchor, shape):
    """stride 4: at k = 2 every coarse point is an anchor and no level runs; stride 0: the first point"""
    check(shape, kw=(("interpAnchorStride", anchor),))


@pytest.mark.parametrize("kw", [(("interpAlpha", 1.5), ("interpBeta", 3.0)), (("interpAlpha", -1.0),)], ids=["alpha1.5_beta3", "alpha-1"])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
def test_level_shift(kw, interp):
    check((65, 47, 130), kw=(("interpAlgo", interp),) + kw)


def spiky_blob(stock):
    a, pos = spiky()
    sz3_amd.set_stock_format(stock)
    try:
        blob = container(a, conf_for(a.shape, algo=sz3_amd.ALGO_INTERP_LORENZO if stock else sz3_amd.ALGO_INTERP, quantbinCnt=256))
    finally:
        sz3_amd.set_stock_format(0)
    return a, pos, blob


@pytest.mark.parametrize("stock", [0, 1], ids=["id17", "stock"])
def test_spikes(stock):
    """raw records inside some boxes' windows and outside others', on and off every coarse grid"""
    a, pos, blob = spiky_blob(stock)
    for k in (1, 2):
        on = (pos % (1 << k) == 0).all(axis=1)
        assert on.any() and (~on).any(), "spikes on and off the level-%d grid" % k
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == (sz3_amd.ALGO_INTERP if stock else sz3_amd.ALGO_HIP_INTERP)
    inside = [int((raw(full[box_slices(lo, ext)]).view(np.float32) == 1e6).sum()) for lo, ext in request(a.shape)]
    assert max(inside) > 0 and min(inside) == 0, "spikes inside some boxes and outside others (%s)" % inside
    handles = [("open_stream", sz3_amd.open_stream(blob, np.float32, device=DEV), full)]
    if not stock:
        dc, pl, size, pfull = device_payload(a, conf_for(a.shape, quantbinCnt=256))
        handles.append(("open_payload", dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream), pfull))
    for name, st, ref in handles:
        with st:
            assert st.stats()["fast"] == 1
            for k in (0, 1, 2):
                bx = request(coarse_shape(a.shape, k))
                same(ask(st, k, bx), ref, k, bx, name)


# ---- 2. the chain at every split -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def chain():
    """sets the chain's threshold for the test's body and puts back what was in force"""
    before = sz3_amd.get_chain_points()
    yield sz3_amd.set_chain_points
    sz3_amd.set_chain_points(before)


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [(65, 47, 130), (5, 9, 1100)], ids=["65x47x130", "5x9x1100"])
def test_chain_at_every_split(shape, dtype, interp, chain):
    """threshold 0, 64, the default and 2^31 — the last puts every level, the finest included, into the chain: identical values at each, and the
    chained level count goes from 0 to n_levels"""
    kw = (("interpAlgo", interp),)
    conf = case(shape, dtype, kw)[3]
    for name, st, full in opens(shape, dtype, kw):
        with st:
            for k in (0, 1, 2):
                cs = coarse_shape(shape, k)
                bx = request(cs)
                n_levels = sz3_amd.tiles_plan(conf, k, bx)["n_levels"]
                assert n_levels > 0
                cs_seen = []
                for points in (0, 64, CHAIN_DEFAULT, 1 << 31):
                    chain(points)
                    same(ask(st, k, bx), full, k, bx, "%s, chain_points %d," % (name, points))
                    s = st.stats()
                    assert s["chain_points"] == points and s["n_levels_last_request"] == n_levels
                    cs_seen.append(s["chain_levels_last_request"])
                assert cs_seen[0] == 0 and cs_seen[3] == n_levels and cs_seen[1] <= cs_seen[3], cs_seen
                # single points only: every pass is a handful of points, every level fits (3-D: below 13^3 / 2 points a pass)
                chain(8192)
                pts = [tile_boxes(cs)[1]] * 3
                same(ask(st, k, pts), full, k, pts, "%s, points only," % name)
                assert st.stats()["chain_levels_last_request"] == n_levels
                # the mixed request: the whole-grid box decides
                whole = [tile_boxes(cs)[0]]
                same(ask(st, k, whole), full, k, whole, "%s, the whole grid," % name)
                c_whole = st.stats()["chain_levels_last_request"]
                same(ask(st, k, bx), full, k, bx, "%s, mixed," % name)
                assert st.stats()["chain_levels_last_request"] == c_whole
                if k == 0:
                    assert c_whole < n_levels, "the finest level of the whole grid has more than 8192 points in a pass"


FORMS = [(shape, dtype, (("interpAlgo", interp),)) for shape, dtype in (((1000,), "float32"), ((33, 70), "float64"), ((9, 12, 17, 20), "float32")) for interp in (0, 1)]
FORMS.append(((33, 70), "float32", (("quantbinCnt", 256), ("interpAnchorStride", 0))))  # (spiky: raw records, and no anchors: the first point)
FORM_IDS = ["%s-%s-%s" % ("x".join(map(str, f[0])), f[1], "-".join("%s%s" % q for q in f[2])) for f in FORMS]


@pytest.mark.parametrize("shape,dtype,kw", FORMS, ids=FORM_IDS)
def test_four_forms_of_one_request(shape, dtype, kw, chain):
    """The box reconstruction's three kernel forms run one device body per step; the same request through all four ways to reach them — the
    context's single-box call box by box, its multi-box call, the handle with the chain off, the handle with every level in the chain — gives
    the same bytes, the full decode's, in 1-D, 2-D and 4-D (the chain's other tests are 3-D). The spiky 2-D case has raw records inside and
    outside the boxes and no anchors: the scatter and the first-point body."""
    spikes = "interpAnchorStride" in dict(kw)
    a = spiky(shape=shape)[0] if spikes else smooth(shape, dtype)
    conf = conf_for(a.shape, **dict(kw))
    dc, pl, size, full = device_payload(a, conf)
    s = torch.cuda.current_stream().cuda_stream
    dt = getattr(torch, a.dtype.name)
    if spikes:
        assert int((raw(full).view(np.float32) == 1e6).sum()) > 0, "the field's spikes are raw records"
    with dc.open_stream(pl.data_ptr(), size, s) as st:
        assert st.stats()["fast"] == 1
        for k in (0, 1):
            bx = request(coarse_shape(a.shape, k))
            n_levels = sz3_amd.tiles_plan(conf, k, bx)["n_levels"]
            forms = {}
            single = [torch.full(tuple(ext), SENTINEL, dtype=dt, device=DEV) for _, ext in bx]
            for (lo, ext), o in zip(bx, single):
                dc.decompress_tile(pl.data_ptr(), size, k, lo, ext, o.data_ptr(), s)
            forms["single-box calls"] = single
            multi = [torch.full(tuple(ext), SENTINEL, dtype=dt, device=DEV) for _, ext in bx]
            dc.decompress_tiles(pl.data_ptr(), size, k, bx, [o.data_ptr() for o in multi], s)
            forms["multi-box call"] = multi
            chain(0)
            forms["handle, chain off"] = ask(st, k, bx)
            assert st.stats()["chain_levels_last_request"] == 0
            chain(1 << 31)
            forms["handle, all in the chain"] = ask(st, k, bx)
            assert st.stats()["chain_levels_last_request"] == n_levels == st.stats()["n_levels_last_request"]
            torch.cuda.synchronize()
            for name, outs in forms.items():
                same(outs, full, k, bx, name)
            for name, outs in forms.items():
                for i, (got, want) in enumerate(zip(outs, single)):
                    assert np.array_equal(raw(got), raw(want)), "%s, level %d: box %d differs from the single-box call's" % (name, k, i)
    dc.close()


# ---- 3. the launch count -------------------------------------------------------------------------------------------------------------------
def test_launch_count(chain):
    shape = (65, 47, 130)
    kw = (("interpAlgo", 0),)  # (linear, N = 3: two launches per pass)
    a, blob, full, conf = case(shape, "float32", kw)
    dc, pl, size, pfull = device_payload(a, conf_for(shape, **dict(kw)))
    with dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream) as st:
        for k in (0, 1):
            straddle = tile_boxes(coarse_shape(shape, k))[4]
            outs = [torch.empty(straddle[1], dtype=torch.float32, device=DEV)]
            l0 = L.sz3hip_debug_region_launches()
            dc.decompress_tiles(pl.data_ptr(), size, k, [straddle], [o.data_ptr() for o in outs], torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ctx_launches = L.sz3hip_debug_region_launches() - l0
            chain(0)
            l0 = L.sz3hip_debug_region_launches()
            same(ask(st, k, [straddle]), pfull, k, [straddle])
            off = L.sz3hip_debug_region_launches() - l0
            assert off == ctx_launches == st.stats()["launches_last_request"], "chain off: the launches sz3hip_decompress_device_tiles issues"
            chain(2048)
            l0 = L.sz3hip_debug_region_launches()
            same(ask(st, k, [straddle]), pfull, k, [straddle])
            one = L.sz3hip_debug_region_launches() - l0
            assert st.stats()["chain_levels_last_request"] > 0 and one < off and one == st.stats()["launches_last_request"], "chain on: strictly fewer (%d, %d)" % (one, off)
            l0 = L.sz3hip_debug_region_launches()
            same(ask(st, k, [straddle] * 9), pfull, k, [straddle] * 9)
            assert L.sz3hip_debug_region_launches() - l0 == one, "nine boxes issue as many launches as one"
            chain(0)
            l0 = L.sz3hip_debug_region_launches()
            same(ask(st, k, [straddle] * 9), pfull, k, [straddle] * 9)
            assert L.sz3hip_debug_region_launches() - l0 == off
    dc.close()


# ---- 4. one Huffman stage for the handle's life ----------------------------------------------------------------------------------------------
def test_one_huffman_stage():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    d0, t0 = sz3_amd.debug_tile_units()
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["huffman_stages"] == 1 and st.stats()["requests"] == 0
        for i in range(10):
            k = i % 4
            bx = request(coarse_shape(shape, k))[1 + i % 3:]
            same(ask(st, k, bx), full, k, bx)
        s = st.stats()
        assert s["huffman_stages"] == 1 and s["requests"] == 10
        assert s["scratch_elems"] > 0 and s["resident_bytes"] >= 2 * a.size + 4 * s["scratch_elems"]
    assert sz3_amd.debug_tile_units() == (d0, t0), "no request ran a tile decode's Huffman stage"


# ---- 5. stock ALGO_INTERP containers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 47, 130), (33, 70), (5, 9, 1100)], ids=["65x47x130", "33x70", "5x9x1100"])
def test_stock_format(shape):
    sz3_amd.set_stock_format(1)
    try:
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo == sz3_amd.ALGO_INTERP
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 1 and st.stats()["huffman_stages"] == 1
        for k in (0, 1, 2, 3):
            bx = request(coarse_shape(shape, k))
            same(ask(st, k, bx), full, k, bx, "stock")


# ---- 6. fallbacks: one full decode at open, gathers afterwards -------------------------------------------------------------------------------
FB_BOXES = {0: [((3, 7, 11), (20, 9, 30)), ((0, 0, 0), (1, 1, 1)), ((3, 7, 11), (20, 9, 30))], 1: [((1, 3, 5), (10, 9, 20)), ((19, 23, 27), (1, 1, 1))],
            2: [((0, 0, 0), (10, 12, 14)), ((4, 5, 6), (1, 1, 1))], 3: [((4, 5, 6), (1, 1, 1)), ((0, 0, 0), (5, 6, 7))]}


@pytest.mark.parametrize("name,kw", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_fallback_containers(name, kw):
    shape = (40, 48, 56)
    a = smooth(shape)
    blob = container(a, conf_for(shape, **kw))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo not in INTERP_IDS
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        s = st.stats()
        assert s["fast"] == 0 and s["resident_bytes"] >= 4 * a.size
        for k in (0, 1, 2, 3):
            same(ask(st, k, FB_BOXES[k]), full, k, FB_BOXES[k], name)
        whole = [((0, 0, 0), coarse_shape(shape, 1))]
        same(ask(st, 1, whole), full, 1, whole, name)
        assert st.stats()["fast"] == 0 and st.stats()["requests"] == 5


def test_fallback_payload_of_a_device_context():
    shape = (40, 48, 56)
    dc, pl, size, full = device_payload(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0))
    with dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream) as st:
        pl.zero_()
        assert st.stats()["fast"] == 0 and st.conf.dims == shape
        for k in (0, 1, 2, 3):
            same(ask(st, k, FB_BOXES[k]), full, k, FB_BOXES[k], "payload")
    dc.close()


def test_fallback_openmp_slabs(monkeypatch):
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    shape = (50, 30, 40)
    blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, openmp=1))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.openmp
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 0
        for k in (0, 1, 2):
            bx = request(coarse_shape(shape, k))
            same(ask(st, k, bx), full, k, bx, "slabs")


# ---- 7. ownership ----------------------------------------------------------------------------------------------------------------------------
def test_the_handle_owns_what_it_reads():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    mine = blob.copy()
    st = sz3_amd.open_stream(mine, np.float32, device=DEV)
    mine[:] = np.random.default_rng(3).integers(0, 256, mine.size, dtype=np.uint8)  # the blob, overwritten with noise
    dc, pl, size, pfull = device_payload(a, conf_for(shape))
    sp = dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream)
    pl.zero_()  # the payload, zeroed
    dc.close()  # ... and its context gone
    del pl
    torch.cuda.synchronize()
    with st, sp:
        for k in (0, 1, 2):
            bx = request(coarse_shape(shape, k))
            same(ask(st, k, bx), full, k, bx, "after the blob was overwritten,")
            same(ask(sp, k, bx), pfull, k, bx, "after the payload was zeroed,")


# ---- 8. requests back to back, on two streams, and a second handle ---------------------------------------------------------------------------
def test_back_to_back_requests():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        b1 = tile_boxes(coarse_shape(shape, 1))
        nine = [b1[4], b1[2], b1[3], b1[5], b1[1], b1[4], b1[2], b1[3], b1[5]]
        three = [b1[1], b1[3], b1[2]]
        for _ in range(3):  # different boxes, no host synchronisation in between: a request's table must not reach the pinned array too early
            x = ask(st, 1, nine, sync=False)
            y = ask(st, 0, tile_boxes(shape)[1:], sync=False)
            z = ask(st, 1, three, sync=False)
            torch.cuda.synchronize()
            same(x, full, 1, nine)
            same(y, full, 0, tile_boxes(shape)[1:])
            same(z, full, 1, three)


def test_two_streams():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        b0, b1 = request(shape), request(coarse_shape(shape, 1))
        torch.cuda.synchronize()
        for _ in range(3):  # the second request shares the scratch and the tables with the first: it is ordered behind it by an event
            x = ask(st, 0, b0, sync=False, stream=s1)
            y = ask(st, 1, b1, sync=False, stream=s2)
            z = ask(st, 0, b0[1:], sync=False, stream=s1)
            torch.cuda.synchronize()
            same(x, full, 0, b0)
            same(y, full, 1, b1)
            same(z, full, 0, b0[1:])


def test_a_second_handle_meanwhile():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    a2, blob2, full2, conf2 = case(shape, "float32", (("interpAlgo", 0), ("interpDirection", 5)))
    assert not np.array_equal(raw(full), raw(full2))
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        b1 = request(coarse_shape(shape, 1))
        torch.cuda.synchronize()
        x = ask(st, 1, b1, sync=False, stream=s1)
        with sz3_amd.open_stream(blob2, np.float32, device=DEV) as other:  # opened while the first handle's request may still run
            y = ask(other, 1, b1, sync=False, stream=s2)
            z = ask(st, 0, request(shape), sync=False, stream=s1)
            w = ask(other, 2, request(coarse_shape(shape, 2)), sync=False, stream=s2)
            torch.cuda.synchronize()
        same(x, full, 1, b1)
        same(y, full2, 1, b1)
        same(z, full, 0, request(shape))
        same(w, full2, 2, request(coarse_shape(shape, 2)))
        same(ask(st, 1, b1), full, 1, b1, "after the other handle was closed,")


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    k = 1
    b = tile_boxes(coarse_shape(shape, k))
    good = [b[2], b[4], b[1], b[3]]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        same(ask(st, k, good), full, k, good)
        before = st.stats()["requests"]
        for place in (0, 2, 3):  # a bad box at the first, a middle and the last place
            bad = list(good)
            bad[place] = ((30, 0, 0), (4, 4, 4))  # (33 coarse planes)
            outs = [torch.full(tuple(ext), SENTINEL, dtype=torch.float32, device=DEV) for _, ext in bad]
            with pytest.raises(sz3_amd.SZ3HipError) as e:
                st.tiles(k, bad, out=outs)
            assert e.value.code == CODES["SZ3HIP_EINVAL"] and "box %d: " % place in str(e.value) and "dimension 0" in str(e.value)
            torch.cuda.synchronize()
            assert all(bool((o == SENTINEL).all()) for o in outs), "a refused request writes nothing"
        outs = [torch.full(tuple(ext), SENTINEL, dtype=torch.float32, device=DEV) for _, ext in good]
        arr, shapes = sz3_amd._boxes(3, good)

        def call(level, n, ptrs):
            return L.sz3hip_stream_tiles(st._h, level, arr, n, (C.c_void_p * 4)(*ptrs), torch.cuda.current_stream().cuda_stream)

        ptrs = [o.data_ptr() for o in outs]
        assert call(k, 4, [ptrs[0], ptrs[1], ptrs[0] + 4, ptrs[3]]) == CODES["SZ3HIP_EINVAL"] and "overlap" in L.sz3hip_last_error().decode()
        assert call(k, 4, [ptrs[0], None, ptrs[2], ptrs[3]]) == CODES["SZ3HIP_EINVAL"] and "box 1" in L.sz3hip_last_error().decode()
        assert call(k, 0, ptrs) == CODES["SZ3HIP_EINVAL"] and "1 .. 256 boxes" in L.sz3hip_last_error().decode()
        assert call(k, 257, ptrs) == CODES["SZ3HIP_EINVAL"] and "1 .. 256 boxes" in L.sz3hip_last_error().decode()
        assert call(31, 4, ptrs) == CODES["SZ3HIP_EINVAL"] and "tile level 31 is outside 0 .. 30" in L.sz3hip_last_error().decode()
        assert call(-1, 4, ptrs) == CODES["SZ3HIP_EINVAL"]
        assert L.sz3hip_stream_tiles(None, k, arr, 4, (C.c_void_p * 4)(*ptrs), None) == CODES["SZ3HIP_EINVAL"] and "no handle" in L.sz3hip_last_error().decode()
        torch.cuda.synchronize()
        assert all(bool((o == SENTINEL).all()) for o in outs), "a refused request writes nothing"
        assert st.stats()["requests"] == before
        same(ask(st, k, good), full, k, good, "after the refusals,")  # the handle still serves the next request
    with pytest.raises(sz3_amd.SZ3HipError) as e:  # a closed handle
        st.tiles(k, good, out=outs)
    assert e.value.code == CODES["SZ3HIP_EINVAL"] and "no handle" in str(e.value)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        st.stats()
    assert e.value.code == CODES["SZ3HIP_EINVAL"]
    assert all(bool((o == SENTINEL).all()) for o in outs)
    with pytest.raises(sz3_amd.SZ3HipError) as e:  # an integer element type at open: the partial calls' code and wording
        sz3_amd.open_stream(blob, np.int32, device=DEV)
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"] and "integer element types are not supported yet" in str(e.value)


def test_refusals_on_a_fallback_handle():
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **dict(FALLBACKS[0][1])))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 0
        bad = [FB_BOXES[1][0], ((20, 0, 0), (1, 1, 1)), FB_BOXES[1][1]]  # (20 coarse planes)
        outs = [torch.full(tuple(ext), SENTINEL, dtype=torch.float32, device=DEV) for _, ext in bad]
        with pytest.raises(sz3_amd.SZ3HipError) as e:
            st.tiles(1, bad, out=outs)
        assert e.value.code == CODES["SZ3HIP_EINVAL"] and "box 1: " in str(e.value) and "dimension 0" in str(e.value)
        torch.cuda.synchronize()
        assert all(bool((o == SENTINEL).all()) for o in outs)
        same(ask(st, 1, FB_BOXES[1]), full, 1, FB_BOXES[1])


# ---- 10. different sinks interleaved on one handle: the one submit path orders request after reduce after map ... ----------------------------------
def sink_calls(items, level1_box, lo, hi, lut):
    """(name, extra launches beyond the request's own, call(st, stream)): every request call of a handle on the same three boxes, then tiles"""
    a, b = lo + 0.25 * (hi - lo), lo + 0.5 * (hi - lo)
    lattice = ((0.4, 0.6, 0.3), [(0.7, 0.5, 1.3)], (5,))  # five points along a line, nearest: the points' bytes
    return [
        ("request", 0, lambda st, s: st.request(items, stream=s)),
        ("reduce", 1, lambda st, s: st.reduce(items, bins=8, lo=lo, hi=hi, stream=s)),
        ("map", 0, lambda st, s: st.map(items, "u8", lo, hi, stream=s)),
        ("select", 2, lambda st, s: st.select(items, a, b, 64, stream=s)),
        ("sample", 0, lambda st, s: st.sample(items, [lattice] * len(items), mode="nearest", stream=s)),
        ("project", 0, lambda st, s: st.project(items, "max", 1, stream=s)),
        ("gradient", 0, lambda st, s: st.gradient(items, "mag", stream=s)),
        ("composite", 0, lambda st, s: st.composite(items, 1, lut, lo, hi, out_type="rgba8", stream=s)),
        ("tiles", None, lambda st, s: st.tiles(1, [level1_box], stream=s)),
    ]


def result_bytes(res):
    """a call's result as bytes, after the device was waited for: tensors as they are, a reduction's records and histogram, a selection's counts
    and its written indices and values (the rest of a selection's arrays is not set)"""
    if isinstance(res, sz3_amd.ReduceResult):
        return [x.tobytes() for x in res.numpy()]
    if isinstance(res, sz3_amd.SelectResult):
        return [np.int64(count).tobytes() + ix.tobytes() + v.tobytes() for count, ix, v in res.numpy()]
    return [raw(t).tobytes() for t in res]


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "full_array"])
def test_sinks_interleaved_on_two_streams(fast):
    from test_gpu_request import mixed  # (that module imports this one)
    shape = (65, 47, 130) if fast else (40, 48, 56)
    if fast:
        a, blob, full, conf = case(shape)
    else:
        blob = container(smooth(shape), conf_for(shape, **dict(FALLBACKS[0][1])))
        full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    items = mixed(shape, (0, 1, 2))[6:9]  # the origin-corner boxes of levels 0, 1 and 2: every extent is above 2
    assert [it[0] for it in items] == [0, 1, 2] and all(e > 2 for it in items for e in it[2])
    lo, hi = float(full.min()), float(full.max())
    lut = torch.linspace(0.05, 0.6, 64, device=DEV).reshape(16, 4).contiguous()
    calls = sink_calls(items, tile_boxes(coarse_shape(shape, 1))[2], lo, hi, lut)
    alone = []
    for name, extra, call in calls:  # every call alone on a fresh handle, with a synchronise behind it
        with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
            res = call(st, None)
            torch.cuda.synchronize()
            alone.append(result_bytes(res))
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == (1 if fast else 0)
        before = st.stats()["requests"]
        torch.cuda.synchronize()
        got, own = [], None
        for turn in range(2):  # the whole sequence twice, the streams alternating, no host synchronisation anywhere
            for i, (name, extra, call) in enumerate(calls):
                got.append(call(st, s1 if (turn * len(calls) + i) % 2 == 0 else s2))
                launches = st.stats()["launches_last_request"]
                if name == "request":
                    own = launches
                    assert own >= 1 and (fast or own == 1)
                elif extra is not None:
                    assert launches == own + extra, "%s: %d launches, the request's own are %d" % (name, launches, own)
        assert st.stats()["requests"] == before + 2 * len(calls)
        torch.cuda.synchronize()
        for j, res in enumerate(got):
            name = calls[j % len(calls)][0]
            assert result_bytes(res) == alone[j % len(calls)], "%s (call %d of the interleaved sequence) differs from the call alone on a fresh handle" % (name, j)

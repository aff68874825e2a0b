"""The opened stream's mixed-level request on the MI355X: boxes of several levels, into contiguous arrays and strided
views, in ONE launch sequence. The one assertion on values everywhere is raw-byte identity with the slice of the full decode's [::2**k] view —
there are no tolerances —, every output buffer is filled with a sentinel beforehand and checked outside the views. Fields, bound, Configs and
boxes are partial_cases.py's; the cached cases and the two opens are test_gpu_stream.py's, so both files share one set of full decodes."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, conf_for, container, device_payload, raw, smooth  # noqa: E402
from sink_models import SENTINEL, atlas_for, tdt, untouched  # noqa: E402
from test_gpu_stream import SHAPES, IDS, case, coarse_shape, coarse_view, opens, spiky_blob, tile_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
LEVELS = (2, 0, 3, 1)  # interleaved: no two neighbours of a request share a level


@pytest.fixture
def chain():
    before = sz3_amd.get_chain_points()
    yield sz3_amd.set_chain_points
    sz3_amd.set_chain_points(before)


def mixed(shape, levels=LEVELS):
    """(level, lo, ext) items: the six boxes of every level's grid, the levels interleaved; then a repeated box (the first point box again) and two
    more that overlap each other (the origin box of the finest level and the whole of the coarsest grid lie over it too)"""
    per = {k: tile_boxes(coarse_shape(shape, k)) for k in levels}
    items = [(k,) + per[k][j] for j in range(6) for k in levels]
    k0 = min(levels)
    lo, ext = per[k0][2]
    return items + [(levels[0],) + per[levels[0]][1], (k0, lo, ext), (k0, tuple(a + (e > 1) for a, e in zip(lo, ext)), tuple(max(1, e - 1) for e in ext))]


def same(outs, full, items, what=""):
    assert len(outs) == len(items)
    for i, (got, (k, lo, ext)) in enumerate(zip(outs, items)):
        want = coarse_view(full, k)[box_slices(lo, ext)]
        assert tuple(got.shape) == tuple(ext) == tuple(want.shape)
        assert np.array_equal(raw(got), raw(want)), "%s box %d (level %d, lo %s shape %s) differs from the full decode's slice" % (what, i, k, lo, ext)


def alloc(st, items):
    return [torch.full(tuple(ext), SENTINEL, dtype=tdt(st), device=DEV) for _, _, ext in items]


def ask(st, items, sync=True, stream=None, outs=None):
    """the request into contiguous sentinel-filled arrays"""
    outs = alloc(st, items) if outs is None else outs
    got = st.request([it + (o,) for it, o in zip(items, outs)], stream=stream)
    assert all(g is o for g, o in zip(got, outs))
    if sync:
        torch.cuda.synchronize()
    return outs


def by_tiles(st, items):
    """the same boxes through Stream.tiles, level by level"""
    outs = [None] * len(items)
    for k in sorted({it[0] for it in items}):
        idx = [i for i, it in enumerate(items) if it[0] == k]
        for i, o in zip(idx, st.tiles(k, [items[i][1:] for i in idx])):
            outs[i] = o
    torch.cuda.synchronize()
    return outs


@contextlib.contextmanager
def chain_off():
    before = sz3_amd.get_chain_points()
    sz3_amd.set_chain_points(0)
    try:
        yield
    finally:
        sz3_amd.set_chain_points(before)


def merged_sequence(st, shape, items, exact=True):
    """Holds the mixed request the handle served last (chain off) to the ONE merged sequence, through its launch count: it is the count of a
    tiles request of the whole grid at the finest requested level — exactly, where the request holds that box; at most, otherwise — and
    strictly less than the sum of the per-level tiles requests of the same boxes, which is what the route level group by level group issues."""
    m = st.stats()["launches_last_request"]
    levels = sorted({it[0] for it in items})
    assert len(levels) > 1
    k0, N = levels[0], len(shape)
    st.tiles(k0, [((0,) * N, coarse_shape(shape, k0))])
    whole = st.stats()["launches_last_request"]
    assert st.stats()["n_levels_last_request"] > 0, "the finest requested level runs levels"
    per_level = 0
    for k in levels:
        st.tiles(k, [it[1:] for it in items if it[0] == k])
        per_level += st.stats()["launches_last_request"]
    torch.cuda.synchronize()
    assert (m == whole if exact else m <= whole) and m < per_level, "launches: the mixed request %d, the whole grid at level %d %d, per level %d" % (m, k0, whole, per_level)


def check_mixed(shape, dtype="float32", kw=(), levels=LEVELS, payload=True, tiles_too=True):
    items = mixed(shape, levels)
    algo = case(shape, dtype, kw)[3].cmprAlgo
    assert shape == (1000,) or algo == sz3_amd.ALGO_HIP_INTERP, "the case must be a lossy interpolation stream (cmprAlgo %d)" % algo
    for name, st, full in opens(shape, dtype, kw, payload):
        fast = name == "open_payload" or algo in INTERP_IDS  # (a 1-D container may be no interpolation stream: the resident array's gathers)
        with st, chain_off():
            assert st.stats()["fast"] == (1 if fast else 0)
            outs = ask(st, items)
            same(outs, full, items, name)
            s = st.stats()
            assert s["requests"] == 1 and s["chain_levels_last_request"] == 0 and s["huffman_stages"] == (1 if fast else 0)
            if fast:
                # (the Config the field was compressed with: a container's trailer does not carry the anchor stride)
                assert s["n_levels_last_request"] == sz3_amd.request_plan(conf_for(shape, **dict(kw)), dtype, items)["n_levels"] > 0
                merged_sequence(st, shape, items)  # (the request holds the whole grid of its finest level)
            else:
                assert s["launches_last_request"] == 1
            if tiles_too:
                for i, (a, b) in enumerate(zip(outs, by_tiles(st, items))):
                    assert np.array_equal(raw(a), raw(b)), "%s box %d differs from Stream.tiles'" % (name, i)
            # the same boxes as rectangles of one atlas
            atlas, views = atlas_for(st, items)
            st.request([it + (v,) for it, v in zip(items, views)])
            torch.cuda.synchronize()
            same(views, full, items, name + ", atlas,")
            assert untouched(atlas, views)
            if fast:
                merged_sequence(st, shape, items)


# ---- 1. mixed levels, both opens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mixed_levels(shape, dtype, interp):
    check_mixed(shape, dtype, (("interpAlgo", interp),))


@pytest.mark.parametrize("anchor", [0, 4], ids=["stride0", "stride4"])
def test_anchors(anchor):
    """stride 4: at levels 2 and 3 every grid point is an anchor and no level runs for those boxes, beside boxes that run two levels and one;
    stride 0: the first point, for the boxes whose coarsest window holds the origin"""
    shape = (65, 47, 130)
    kw = (("interpAnchorStride", anchor),)
    if anchor == 4:
        conf = conf_for(shape, **dict(kw))
        assert [sz3_amd.tile_plan(conf, k, (0, 0, 0), coarse_shape(shape, k))["region"]["n_levels"] for k in range(4)] == [2, 1, 0, 0]
    check_mixed(shape, kw=kw)


@pytest.mark.parametrize("shape,top", [((1000,), 10), ((65, 47, 130), 8)], ids=["1000", "65x47x130"])
def test_a_grid_of_one_point(shape, top):
    assert coarse_shape(shape, top) == (1,) * len(shape)
    for name, st, full in opens(shape):
        fast = st.stats()["fast"] == 1
        with st, chain_off():
            N = len(shape)
            items = [(top, (0,) * N, (1,) * N), (0,) + tile_boxes(shape)[4], (top - 1, (0,) * N, coarse_shape(shape, top - 1)), (0,) + tile_boxes(shape)[1],
                     (top, (0,) * N, (1,) * N)]
            same(ask(st, items), full, items, name)
            if fast:
                merged_sequence(st, shape, items, exact=False)  # (no box of the request is the whole grid of level 0)
            alone = [items[0], items[4]]  # no level runs at all: one level, the tiles request's own sequence
            same(ask(st, alone), full, alone, name)
            if fast:
                m = st.stats()["launches_last_request"]
                st.tiles(top, [it[1:] for it in alone])
                assert st.stats()["launches_last_request"] == m and st.stats()["n_levels_last_request"] == 0


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("direction", [3, 5])
def test_direction(direction, interp):
    check_mixed((65, 47, 130), kw=(("interpAlgo", interp), ("interpDirection", direction)), tiles_too=False)


@pytest.mark.parametrize("kw", [(("interpAlpha", 1.5), ("interpBeta", 3.0)), (("interpAlpha", -1.0),)], ids=["alpha1.5_beta3", "alpha-1"])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
def test_level_shift(kw, interp):
    """the error bound of a pass is its ARRAY level's: what the boxes of different levels share in one launch"""
    check_mixed((65, 47, 130), kw=(("interpAlgo", interp),) + kw, tiles_too=False)


@pytest.mark.parametrize("stock", [0, 1], ids=["id17", "stock"])
def test_spikes(stock):
    """raw records inside some boxes' windows and outside others', on and off every coarse grid"""
    a, pos, blob = spiky_blob(stock)
    for k in (1, 2):
        on = (pos % (1 << k) == 0).all(axis=1)
        assert on.any() and (~on).any(), "spikes on and off the level-%d grid" % k
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    items = mixed(a.shape)
    inside = [int((raw(coarse_view(full, k)[box_slices(lo, ext)]).view(np.float32) == 1e6).sum()) for k, lo, ext in items]
    assert max(inside) > 0 and min(inside) == 0
    assert all(max(n for n, it in zip(inside, items) if it[0] == k) > 0 for k in (0, 1, 2)), "the levels 0, 1 and 2 have a box that holds a spike (%s)" % inside
    handles = [("open_stream", sz3_amd.open_stream(blob, np.float32, device=DEV), full)]
    if not stock:
        dc, pl, size, pfull = device_payload(a, conf_for(a.shape, quantbinCnt=256))
        handles.append(("open_payload", dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream), pfull))
    for name, st, ref in handles:
        with st, chain_off():
            assert st.stats()["fast"] == 1
            same(ask(st, items), ref, items, name)
            merged_sequence(st, a.shape, items)
            atlas, views = atlas_for(st, items, pad=1)
            st.request([it + (v,) for it, v in zip(items, views)])
            torch.cuda.synchronize()
            same(views, ref, items, name + ", atlas,")
            assert untouched(atlas, views)


# ---- 2. strided views ------------------------------------------------------------------------------------------------------------------------
def test_strided_views():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    items = mixed(shape)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        # x stride 2, a step along y too, and contiguous outputs between them
        bufs, views = [], []
        for i, (k, lo, ext) in enumerate(items):
            form = i % 3
            dims = {0: ext, 1: ext[:-1] + (2 * ext[-1],), 2: (ext[0] + 1, 2 * ext[1] + 1, ext[2] + 3)}[form]
            b = torch.full(dims, SENTINEL, dtype=torch.float32, device=DEV)
            bufs.append(b)
            views.append({0: b, 1: b[..., ::2], 2: b[1:, 1::2, 2:-1]}[form])
            assert tuple(views[-1].shape) == tuple(ext)
        assert any(not v.is_contiguous() for v in views) and any(v.is_contiguous() for v in views)
        got = st.request([it + (v,) for it, v in zip(items, views)])
        torch.cuda.synchronize()
        same(got, full, items, "views,")
        assert all(untouched(b, [v]) for b, v in zip(bufs, views)), "nothing outside a view is written"
    # a 4-D atlas
    shape = (9, 12, 17, 20)
    a, blob, full, conf = case(shape)
    items = mixed(shape)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        atlas, views = atlas_for(st, items, pad=1)
        assert atlas.dim() == 4
        st.request([it + (v,) for it, v in zip(items, views)])
        torch.cuda.synchronize()
        same(views, full, items, "4-D atlas,")
        assert untouched(atlas, views)


# ---- 3. the launch count ---------------------------------------------------------------------------------------------------------------------
def test_launch_count(chain):
    shape = (65, 47, 130)
    kw = (("interpAlgo", 0),)  # (linear, N = 3: two launches per pass)
    a, blob, full, conf = case(shape, "float32", kw)
    three = [(k,) + tile_boxes(coarse_shape(shape, k))[4] for k in (1, 0, 2)]
    twelve = three + [(k,) + tile_boxes(coarse_shape(shape, k))[j] for j in (2, 3, 5) for k in (2, 0, 1)]

    def launches(f):
        l0 = L.sz3hip_debug_region_launches()
        f()
        n = L.sz3hip_debug_region_launches() - l0
        assert n == st.stats()["launches_last_request"]
        return n

    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        chain(0)
        m3 = launches(lambda: same(ask(st, three), full, three))
        assert st.stats()["chain_levels_last_request"] == 0 and st.stats()["n_levels_last_request"] == sz3_amd.tile_plan(conf, 0, (0, 0, 0), shape)["region"]["n_levels"]
        whole = launches(lambda: st.tiles(0, [((0, 0, 0), shape)]))
        per_level = [launches(lambda: st.tiles(k, [(lo, ext)])) for k, lo, ext in three]
        print("launches: mixed request of levels {0, 1, 2}: %d; tiles of the whole grid at level 0: %d; the three tiles requests: %s" % (m3, whole, per_level))
        assert m3 <= whole, "the merged sequence is the finest level's own: no more launches than a level-0 request (%d, %d)" % (m3, whole)
        assert m3 < sum(per_level), "strictly fewer launches than the three requests of one level each (%d, %s)" % (m3, per_level)
        m12 = launches(lambda: same(ask(st, twelve), full, twelve))
        assert m12 == m3, "twelve boxes issue as many launches as three (%d, %d)" % (m12, m3)
        for points in (0, 2048):  # one level through the new call: exactly tiles' launches, the chain included
            chain(points)
            for k in (0, 1):
                bx = [tile_boxes(coarse_shape(shape, k))[j] for j in (4, 1, 4)]
                t = launches(lambda: st.tiles(k, bx))
                ct = st.stats()["chain_levels_last_request"]
                one = [(k,) + b for b in bx]
                r = launches(lambda: same(ask(st, one), full, one))
                assert r == t and st.stats()["chain_levels_last_request"] == ct and (ct > 0) == (points > 0), (points, k, r, t, ct)
        chain(2048)  # two or more levels never take the chain
        outs = ask(st, twelve)
        assert st.stats()["chain_levels_last_request"] == 0 and st.stats()["chain_points"] == 2048 and st.stats()["launches_last_request"] == m3
        same(outs, full, twelve, "threshold 2048,")


def test_level_group_by_level_group(chain):
    """the route of a request whose boxes do not align by array level — none does — behind its development switch: level group by level group
    over the one-level sequence; the same bytes, the launches of the per-level tiles requests"""
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, "float32", (("interpAlgo", 0),))
    items = mixed(shape)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for points in (0, 2048):
            chain(points)
            merged = ask(st, items)
            m, levels = st.stats()["launches_last_request"], st.stats()["n_levels_last_request"]
            with sz3_amd.debug_flags2(sz3_amd.Dbg2.REQUEST_BY_LEVEL):
                grouped = ask(st, items)
                s = st.stats()
                atlas, views = atlas_for(st, items, pad=1)
                st.request([it + (v,) for it, v in zip(items, views)])
                torch.cuda.synchronize()
            same(grouped, full, items, "by level,")
            same(views, full, items, "by level, atlas,")
            assert untouched(atlas, views)
            assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(merged, grouped))
            chain(0)  # (the groups never take the chain)
            per_level = 0
            for k in sorted(set(LEVELS)):
                st.tiles(k, [it[1:] for it in items if it[0] == k])
                per_level += st.stats()["launches_last_request"]
            assert s["launches_last_request"] == per_level > m and s["chain_levels_last_request"] == 0 and s["n_levels_last_request"] == levels
            same(ask(st, items), full, items, "merged again,")
            assert st.stats()["launches_last_request"] == m


def test_one_huffman_stage():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    d0, t0 = sz3_amd.debug_tile_units()
    items = mixed(shape)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for i in range(10):
            sub = items[i % 5:len(items) - i]
            same(ask(st, sub), full, sub)
        s = st.stats()
        assert s["huffman_stages"] == 1 and s["requests"] == 10
    assert sz3_amd.debug_tile_units() == (d0, t0), "no request ran a tile decode's Huffman stage"


# ---- 4. fallback handles: one gather launch out of the resident array ------------------------------------------------------------------------
FB_ITEMS = [(2, (0, 0, 0), (10, 12, 14)), (0, (3, 7, 11), (20, 9, 30)), (3, (4, 5, 6), (1, 1, 1)), (1, (1, 3, 5), (10, 9, 20)), (0, (0, 0, 0), (1, 1, 1)),
            (3, (0, 0, 0), (5, 6, 7)), (1, (19, 23, 27), (1, 1, 1)), (0, (3, 7, 11), (20, 9, 30)), (2, (4, 5, 6), (1, 1, 1))]


def check_fallback(st, full, name):
    assert st.stats()["fast"] == 0
    atlas, views = atlas_for(st, FB_ITEMS, pad=1)
    views[1] = torch.full((20, 9, 60), SENTINEL, dtype=torch.float32, device=DEV)[..., ::2]  # (x stride 2, an array of its own)
    st.request([it + (v,) for it, v in zip(FB_ITEMS, views)])
    torch.cuda.synchronize()
    same(views, full, FB_ITEMS, name)
    assert untouched(atlas, views[:1] + views[2:]) and untouched(views[1]._base, [views[1]])
    same(ask(st, FB_ITEMS), full, FB_ITEMS, name)
    s = st.stats()
    assert s["fast"] == 0 and s["requests"] == 2 and s["launches_last_request"] == 1 and s["chain_levels_last_request"] == 0


@pytest.mark.parametrize("name,kw", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_fallback_containers(name, kw):
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **kw))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo not in INTERP_IDS
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        check_fallback(st, full, name)


def test_fallback_payload_of_a_device_context():
    shape = (40, 48, 56)
    dc, pl, size, full = device_payload(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0))
    with dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream) as st:
        pl.zero_()
        check_fallback(st, full, "payload")
    dc.close()


def test_fallback_openmp_slabs(monkeypatch):
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, openmp=1))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.openmp
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        check_fallback(st, full, "slabs")


# ---- 5. refusals on an open handle -----------------------------------------------------------------------------------------------------------
def refusals(st, full, good):
    """every refusal leaves every output as it was and the handle able to serve the next request"""
    N = len(good[0][1])
    before = st.stats()["requests"]
    outs = [torch.full(tuple(ext), SENTINEL, dtype=torch.float32, device=DEV) for _, _, ext in good]
    atlas, views = atlas_for(st, good)

    def refused(items, code, *words):
        with pytest.raises(sz3_amd.SZ3HipError) as e:
            st.request(items)
        assert e.value.code == CODES[code] and all(w in str(e.value) for w in words), str(e.value)

    def with_item(place, item):
        items = [it + (o,) for it, o in zip(good, outs)]
        if len(item) == 3:
            outs.append(torch.full(item[2], SENTINEL, dtype=torch.float32, device=DEV))
            item = item + (outs[-1],)
        items[place] = item
        return items

    for place in (0, 1, len(good) - 1):
        refused(with_item(place, (1, (30,) + (0,) * (N - 1), (4,) * N)), "SZ3HIP_EINVAL", "box %d: " % place, "dimension 0")  # (33 coarse planes)
        refused(with_item(place, (31, (0,) * N, (1,) * N)), "SZ3HIP_EINVAL", "box %d: tile level 31 is outside 0 .. 30" % place)
        k, lo, ext = good[place]
        wide = torch.full(tuple(ext[:-1]) + (ext[-1] + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        outs.append(wide)
        if ext[-1] > 1:
            refused(with_item(place, (k, lo, ext, wide.as_strided(tuple(ext), tuple(wide.stride()[:-1]) + (0,)))), "SZ3HIP_EINVAL", "box %d: " % place, "zero")
        if ext[-1] > 1 and ext[-2] > 1:
            t = torch.full(tuple(ext[:-2]) + (ext[-1], ext[-2]), SENTINEL, dtype=torch.float32, device=DEV)
            outs.append(t)
            refused(with_item(place, (k, lo, ext, t.transpose(-1, -2))), "SZ3HIP_EINVAL", "box %d: " % place, "permuted")
    # the C interface: what the Python class cannot say
    reqs = (sz3_amd._CTileReq * len(good))()
    arr, _ = sz3_amd._boxes(N, [it[1:] for it in good])

    def fill():
        for i, (it, o) in enumerate(zip(good, outs)):
            reqs[i].level, reqs[i].reserved, reqs[i].box, reqs[i].d_out = it[0], 0, arr[i], o.data_ptr()
            reqs[i].strides[:] = [0, 0, 0, 0]

    def call(n=len(good)):
        rc = L.sz3hip_stream_request(st._h, reqs, n, torch.cuda.current_stream().cuda_stream)
        return rc, L.sz3hip_last_error().decode()

    einval = CODES["SZ3HIP_EINVAL"]
    fill()
    reqs[1].reserved = 3
    assert call() == (einval, "box 1: the reserved word is 3, not 0")
    fill()
    reqs[2].d_out = None
    assert call() == (einval, "box 2: the output array is NULL")
    fill()
    reqs[1].strides[N - 1] = -1
    rc, msg = call()
    assert rc == einval and "box 1: " in msg and "negative" in msg
    fill()
    reqs[2].d_out = outs[0].data_ptr() + 4  # two contiguous outputs that overlap
    assert call() == (einval, "box 2: the output overlaps box 0's, or cannot be shown not to")
    fill()
    for i, v in enumerate(views):  # two rectangles of the atlas that meet
        reqs[i].d_out = v.data_ptr()
        reqs[i].strides[:N] = list(v.stride())
    reqs[1].d_out = views[1].data_ptr() - 4
    assert call() == (einval, "box 1: the output overlaps box 0's, or cannot be shown not to")
    reqs[1].d_out = views[1].data_ptr()
    reqs[1].strides[N - 1] = 2  # ... and two views of different strides whose hulls meet
    rc, msg = call()
    assert rc == einval and "cannot be shown not to" in msg
    fill()
    assert call(0)[0] == einval and "1 .. 256 boxes" in call(0)[1]
    assert call(257)[0] == einval and "1 .. 256 boxes" in call(257)[1]
    assert L.sz3hip_stream_request(st._h, None, 1, None) == einval
    assert L.sz3hip_stream_request(None, reqs, len(good), None) == einval and "no handle" in L.sz3hip_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs) and bool((atlas == SENTINEL).all()), "a refused request writes nothing"
    assert st.stats()["requests"] == before
    same(ask(st, good), full, good, "after the refusals,")


def test_refusals():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    good = [(k,) + tile_boxes(coarse_shape(shape, k))[j] for k, j in ((2, 2), (0, 4), (1, 3), (3, 0))]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        same(ask(st, good), full, good)
        refusals(st, full, good)
    with pytest.raises(sz3_amd.SZ3HipError) as e:  # a closed handle
        st.request(good)
    assert e.value.code == CODES["SZ3HIP_EINVAL"] and "no handle" in str(e.value)


def test_refusals_on_a_fallback_handle():
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **dict(FALLBACKS[0][1])))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 0
        refusals(st, full, FB_ITEMS[:4])


# ---- 6. ordering -----------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_and_two_streams():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    a2, blob2, full2, conf2 = case(shape, "float32", (("interpAlgo", 0), ("interpDirection", 5)))
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    items = mixed(shape)
    x_items, y_items = items[:9], items[5:]
    b1 = tile_boxes(coarse_shape(shape, 1))
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st, sz3_amd.open_stream(blob2, np.float32, device=DEV) as other:
        for _ in range(2):  # no host synchronisation in between: the table, the scratch and the streams' order
            bufs = [alloc(st, its) for its in (x_items, y_items, x_items, y_items, y_items, x_items)]
            tb = [[torch.full(ext, SENTINEL, dtype=torch.float32, device=DEV) for _, ext in b1] for _ in range(2)]
            torch.cuda.synchronize()  # (the outputs are filled on the default stream: before anything runs on s1 / s2)
            x = ask(st, x_items, sync=False, outs=bufs[0])
            y = ask(st, y_items, sync=False, outs=bufs[1])
            t = st.tiles(1, b1, out=tb[0])
            z = ask(st, x_items, sync=False, stream=s1, outs=bufs[2])
            w = ask(st, y_items, sync=False, stream=s2, outs=bufs[3])
            o = ask(other, y_items, sync=False, stream=s2, outs=bufs[4])
            t2 = st.tiles(1, b1, out=tb[1], stream=s1)
            v = ask(st, x_items, sync=False, stream=s2, outs=bufs[5])
            torch.cuda.synchronize()
            for got in (x, z, v):
                same(got, full, x_items)
            for got in (y, w):
                same(got, full, y_items)
            same(o, full2, y_items, "the second handle,")
            for got in (t, t2):
                same(got, full, [(1,) + b for b in b1], "tiles between the requests,")

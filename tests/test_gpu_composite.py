"""Boxes composited along an axis, on the MI355X: Stream.composite, composite_points.

Expected values come from numpy alone (composite_model.py: the rule as a Python loop over the axis index on whole slices, float64), over the
full decode's [::2**k] slice of the box. Equality is in BYTES; the only exception is a NaN output, checked with isnan. Every output lives in
a buffer filled with 0x4D, and every byte outside the views — and every byte of a refused call — must still be 0x4D afterwards.

The kernels' constants the extents below bracket (sz3hip_composite.hip): a workgroup is 256 output points; the body for an axis that is not
the fastest issues CMP_BATCH = 8 loads ahead of the fold (axis extents 1, 7, 8, 9, 17); the body for the fastest axis gives a wave 64 rows
and steps 128 / sizeof(T) columns at a time — 32 for f32, 16 for f64 (axis extents 1, 2, 31, 32, 33, 63, 64, 65, 129; 1, 63, 64, 65, 257
rows)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
import composite_model as cm  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, conf_for, container, device_payload, smooth  # noqa: E402
from sink_models import FILL, flat, project_filled as filled, project_host as host, project_untouched as untouched, same_bytes  # noqa: E402
from test_gpu_request import FB_ITEMS, ask, chain, mixed, same  # noqa: E402,F401
from test_gpu_stream import SHAPES, IDS, case, coarse_shape, coarse_view, opens, tile_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
INF = float("inf")
TYPES = (cm.RGBA32F, cm.RGBA8)


def make_lut(n, seed=7, scale=0.3):
    """colours in [0, 1], opacities in [0, scale]"""
    rng = np.random.default_rng(seed)
    lut = rng.random((n, 4)).astype(np.float32)
    lut[:, 3] *= np.float32(scale)
    return lut


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def out_shape(ext, axis, out_type):
    return flat(ext, axis) + ((4,) if out_type == cm.RGBA32F else ())


def out_filled(ext, axis, out_type):
    return filled(out_shape(ext, axis, out_type), "float32" if out_type == cm.RGBA32F else "int32")


def atlas4(shapes, out_type):
    """one atlas of OUTPUT elements and the collapsed shapes' rectangles in it, side by side along x with a gap of one element; odd pitch"""
    N = len(shapes[0])
    dims = [max(s[j] for s in shapes) + 1 for j in range(N - 1)] + [sum(s[-1] + 1 for s in shapes)]
    dims[-1] += 1 - dims[-1] % 2
    atlas = filled(tuple(dims) + ((4,) if out_type == cm.RGBA32F else ()), "float32" if out_type == cm.RGBA32F else "int32")
    views, slices, x = [], [], 0
    for s in shapes:
        sl = tuple(slice(0, e) for e in s[:-1]) + (slice(x, x + s[-1]),)
        slices.append(sl)
        views.append(atlas[sl])
        x += s[-1] + 1
    return atlas, views, slices


def slices_of(full, items):
    return [coarse_view(full, k)[box_slices(lo, ext)].cpu().numpy() for k, lo, ext in items]


def window(full):
    f = full.cpu().numpy().astype(np.float64)
    return [float(v) for v in np.quantile(f[np.isfinite(f)], [0.1, 0.9])]


def check_composite(st, items, slices, axis, lut, lo, hi, out_type, what="", atlas=True, level_opacity=False, **kw):
    """Stream.composite into contiguous outputs and into rectangles of one atlas, both against the model; returns the contiguous outputs' bytes"""
    d_lut = dev(lut)
    outs = [out_filled(ext, axis, out_type) for _, _, ext in items]
    got = st.composite([it + (o,) for it, o in zip(items, outs)], axis, d_lut, lo, hi, out_type, level_opacity=level_opacity, **kw)
    assert all(g is o for g, o in zip(got, outs))
    if atlas:
        at, views, where = atlas4([flat(ext, axis) for _, _, ext in items], out_type)
        st.composite([it + (v,) for it, v in zip(items, views)], axis, d_lut, lo, hi, out_type, level_opacity=level_opacity, **kw)
    torch.cuda.synchronize()
    res = []
    mk = {k: v for k, v in kw.items() if k in ("reverse", "cutoff")}
    for i, (it, s) in enumerate(zip(items, slices)):
        sq = kw.get("level_bias", 0) + (it[0] if level_opacity else 0)
        want = cm.expected(s, axis, lut, lo, hi, out_type, s=sq, **mk)
        w = "%s axis %d -> %s %s box %d %s:" % (what, axis, out_type, kw, i, it)
        same_bytes(host(outs[i]), want, w + " contiguous,")
        if atlas:
            same_bytes(host(views[i]), want, w + " atlas,")
        res.append(host(outs[i]).tobytes())
    assert not atlas or untouched(at, where), what + " a byte outside the rectangles was written"
    return res


COMBOS = [(cm.RGBA32F, False), (cm.RGBA32F, True), (cm.RGBA8, False), (cm.RGBA8, True)]


# ---- 1. shapes and opens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shapes_and_opens(shape, dtype, interp):
    kw = (("interpAlgo", interp),)
    items = mixed(shape)
    algo = case(shape, dtype, kw)[3].cmprAlgo
    lut = make_lut(256)
    for name, st, full in opens(shape, dtype, kw):
        fast = name == "open_payload" or algo in INTERP_IDS
        slices = slices_of(full, items)
        lo, hi = window(full)
        with st:
            assert st.stats()["fast"] == (1 if fast else 0)
            n0 = st.stats()["requests"]
            calls = 0
            for axis in range(len(shape)):
                for out_type, rev in COMBOS:
                    check_composite(st, items, slices, axis, lut, lo, hi, out_type, what=name, reverse=rev, cutoff=0.95 if rev else INF)
                    calls += 2
            assert st.stats()["requests"] == n0 + calls, "a compositing counts as a request"
            assert st.stats()["huffman_stages"] == (1 if fast else 0)


def test_stock_container():
    shape = (65, 47, 130)
    sz3_amd.set_stock_format(1)
    try:
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    items = mixed(shape)
    slices = slices_of(full, items)
    lo, hi = window(full)
    lut = make_lut(256)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 1
        for axis in range(3):
            for out_type, rev in COMBOS:
                check_composite(st, items, slices, axis, lut, lo, hi, out_type, what="stock", reverse=rev)


def test_level_opacity():
    """a level-0 and a level-2 box of one region: the coarse box's opacities are squared twice"""
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    items = [(0, (8, 4, 12), (40, 24, 64)), (2, (2, 1, 3), (10, 6, 16)), (1, (4, 2, 6), (20, 12, 32)), (3, (0, 0, 0), (9, 6, 17))]
    slices = slices_of(full, items)
    lo, hi = window(full)
    lut = make_lut(64, scale=0.2)
    assert (cm.corrected_alpha(lut, 2) != cm.corrected_alpha(lut, 0)).any()
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for axis in range(3):
            with_lvl = check_composite(st, items, slices, axis, lut, lo, hi, cm.RGBA32F, what="level opacity", level_opacity=True)
            without = check_composite(st, items, slices, axis, lut, lo, hi, cm.RGBA32F, what="no level opacity")
            assert with_lvl[0] == without[0] and with_lvl[1] != without[1], "level 0 is not corrected, level 2 is"
            check_composite(st, items, slices, axis, lut, lo, hi, cm.RGBA8, what="level opacity + bias", level_opacity=True, level_bias=3, reverse=True)
            check_composite(st, items, slices, axis, lut, lo, hi, cm.RGBA32F, what="bias", level_bias=30, atlas=False)


# ---- 2. extents, strides and dimensions, through composite_points ------------------------------------------------------------------------------
def check_points(src, ref, axis, lut, lo=-1.0, hi=1.0, what="", combos=COMBOS, **kw):
    """composite_points of the device view `src` (host values `ref`) into a rectangle of a 0x4D buffer, both output types, both directions"""
    d_lut = dev(lut)
    shape = flat(ref.shape, axis)
    sl = tuple(slice(1, 1 + e) for e in shape)
    calls = []
    for out_type, rev in combos:
        buf = out_filled([e + 2 for e in shape], None, out_type)
        got = sz3_amd.composite_points(src, axis, d_lut, lo, hi, out_type, reverse=rev, out=buf[sl], **kw)
        assert got.data_ptr() == buf[sl].data_ptr()
        calls.append((out_type, rev, buf))
    torch.cuda.synchronize()
    for out_type, rev, buf in calls:
        want = cm.expected(ref, axis, lut, lo, hi, out_type, reverse=rev, s=kw.get("level_bias", 0), cutoff=kw.get("cutoff", INF))
        same_bytes(host(buf[sl]), want, "%s -> %s reverse %s %s, shape %s axis %d:" % (what, out_type, rev, kw, ref.shape, axis))
        assert untouched(buf, [sl]), "%s: a byte outside the view was written" % what


def noisy(rng, shape, dtype):
    """normal values with a NaN, an Inf and a -Inf somewhere (where there is room)"""
    a = rng.normal(0.0, 0.6, shape).astype(dtype)
    v = a.reshape(-1)
    if v.size >= 8:
        v[rng.integers(0, v.size, 3)] = [np.nan, np.inf, -np.inf]
    return a


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fastest_axis_extents(dtype):
    rng = np.random.default_rng(31)
    lut = make_lut(256)
    for rows in (1, 63, 64, 65, 257):
        for ex in (1, 2, 31, 32, 33, 63, 64, 65, 129):
            a = noisy(rng, (rows, ex), dtype)
            check_points(dev(a), a, 1, lut, what="rows %d" % rows, cutoff=0.9)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_other_axis_extents(dtype):
    rng = np.random.default_rng(37)
    lut = make_lut(256)
    for outs in (1, 255, 256, 257):
        for ex in (1, 7, 8, 9, 17):
            a = noisy(rng, (ex, outs), dtype)
            check_points(dev(a), a, 0, lut, what="outputs %d" % outs, cutoff=0.9)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dimensions_strides_and_tables(dtype):
    rng = np.random.default_rng(41)
    lut = make_lut(256)
    short = [(cm.RGBA32F, False), (cm.RGBA8, True)]
    # 1-D .. 4-D, every axis; extent-1 dimensions in every place
    for shape in ((1,), (77,), (9, 70), (3, 5, 67), (3, 4, 5, 66), (1, 9, 1, 70), (9, 1, 70, 1), (1, 1, 40), (40, 1, 1), (5, 37, 1), (1, 1, 1, 1)):
        a = noisy(rng, shape, dtype)
        for axis in range(len(shape)):
            check_points(dev(a), a, axis, lut, what="dims", combos=short)
    a = noisy(rng, (6, 7, 140), dtype)
    src = dev(a)
    views = [("x stride 2", src[:, :, ::2], a[:, :, ::2]),
             ("broadcast rows", src[:, 2:3, :].expand(6, 5, 140), np.broadcast_to(a[:, 2:3, :], (6, 5, 140))),
             ("broadcast x", src[:, :, 9:10].expand(6, 7, 70), np.broadcast_to(a[:, :, 9:10], (6, 7, 70))),
             ("broadcast slowest", src[1:2].expand(9, 7, 140), np.broadcast_to(a[1:2], (9, 7, 140))),
             ("transposed", src.permute(2, 0, 1), a.transpose(2, 0, 1)),
             ("transposed 2", src.transpose(1, 2), a.transpose(0, 2, 1))]
    for what, v, ref in views:
        for axis in range(3):
            check_points(v, np.ascontiguousarray(ref), axis, lut, what=what, combos=short, level_bias=1)
    for n in (2, 3, 256, 1024):
        t = make_lut(n, seed=n)
        for axis in range(3):
            check_points(src, a, axis, t, what="lut_n %d" % n, combos=short)
    # negative axes and allocated outputs
    out = sz3_amd.composite_points(src, -1, dev(lut), -1.0, 1.0)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (6, 7, 1, 4) and out.dtype == torch.float32 and out.is_contiguous()
    same_bytes(host(out), cm.expected(a, 2, lut, -1.0, 1.0))
    out = sz3_amd.composite_points(src, 0, dev(lut), -1.0, 1.0, "rgba8")
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 7, 140) and out.dtype == torch.int32
    same_bytes(host(out), cm.expected(a, 0, lut, -1.0, 1.0, cm.RGBA8))


# ---- 3. crafted columns ----------------------------------------------------------------------------------------------------------------------
# the crafted table over the window [0, 8): entry k serves x in [k, k + 1)
#   0 clear, 1 opaque white, 2 .. 4 faint colours, 5 beyond [0, 1] (a = 1.5, colours 2 and -1), 6 a NaN opacity, 7 tiny (denormal weights)
CRAFT = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [0.9, 0.1, 0.2, 0.25], [0.1, 0.8, 0.3, 0.125], [0.2, 0.3, 0.7, 0.0625],
                  [2.0, -1.0, 0.5, 1.5], [0.5, 0.5, 0.5, np.nan], [1.0, 1e-30, 1e-38, 1e-40]], dtype=np.float32)


def crafted(dtype):
    """columns of 16 points, one per row; values are entry indices + 0.5 unless noted"""
    E = 16
    n, i = np.nan, np.inf
    faint = [2.5, 3.5, 4.5, 3.5, 2.5, 4.5, 2.5, 3.5, 4.5, 4.5, 3.5, 2.5, 2.5, 3.5, 4.5, 3.5]

    t = np.dtype(dtype).type

    def opaque_at(p):  # behind the opaque entry the column meets the NaN entry: a missed stop changes the bytes (0 * NaN)
        c = list(faint)
        c[p] = 1.5
        if p + 1 < E:
            c[p + 1] = 6.5
        return c
    cols = [[n] * E,
            [n, 2.5, n, n, 3.5, n, 4.5, n] * 2,
            [i, -i] * (E // 2),
            [-i, i, 2.5, -i] * 4,
            [0.0, 8.0, float(np.nextafter(t(8.0), t(0.0))), 2.0, float(np.nextafter(t(2.0), t(0.0))), 3.0, -0.0, 7.0] * 2,
            opaque_at(0), opaque_at(7), opaque_at(8), opaque_at(15),
            [5.5] + faint[1:],
            faint[:5] + [5.5] + faint[6:],
            [2.5, 6.5] + faint[2:],
            [6.5] * E,
            [7.5] * E,
            [7.5, 7.5, 2.5, 7.5] * 4,
            [0.5] * E,
            faint]
    return np.array(cols, dtype=np.float64).astype(dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_crafted_columns(dtype):
    a = crafted(dtype)
    m = cm.composite(a, 1, CRAFT, 0.0, 8.0)[:, 0]
    # what the cases are there for
    assert (m[0] == 0.0).all() and not np.signbit(m[0]).any(), "all NaN: +0.0"
    assert (m[1] == cm.composite(np.array([[2.5, 3.5, 4.5] * 2]), 1, CRAFT, 0.0, 8.0)[0, 0]).all(), "NaNs between finite points add nothing"
    assert list(cm.codes(a[2, :2].astype(np.float64), 0.0, 8.0, 8)) == [7, 0], "+-Inf: the end codes"
    assert list(cm.codes(a[4, :8].astype(np.float64), 0.0, 8.0, 8)) == [0, 7, 7, 2, 1, 3, 0, 7], "lo, hi, nextafter(hi, lo) and the entries' edges"
    stopped = cm.composite(a, 1, CRAFT, 0.0, 8.0, cutoff=1.0)[:, 0]
    for row, p in ((5, 0), (6, 7), (7, 8), (8, 15)):  # the opaque entry at the first, the eighth, the ninth and the last place
        assert stopped[row, 3] == 1.0 and (stopped[row] == cm.composite(a[row:row + 1, :p + 1], 1, CRAFT, 0.0, 8.0)[0, 0]).all()
        assert np.isnan(m[row]).all() == (p < 15), "without the stop the column runs into the NaN entry"
    assert np.isnan(m[11]).all() and np.isnan(m[12]).all(), "a NaN entry"
    assert 0.0 < m[13, 3] < 1e-38, "denormal weights"
    assert stopped[9, 3] == 1.5 and m[9, 3] != 1.5 and m[10, 3] != stopped[10, 3], "an opacity beyond 1"
    t = np.ascontiguousarray(a.T)
    for cutoff in (1.0, INF, 0.3):
        check_points(dev(a), a, 1, CRAFT, 0.0, 8.0, "crafted rows", cutoff=cutoff)
        check_points(dev(t), t, 0, CRAFT, 0.0, 8.0, "crafted columns", cutoff=cutoff)
    # the same columns 70 and 9 points long (several steps of both bodies): the column repeated, then cut
    for E in (70, 9):
        b = np.ascontiguousarray(np.tile(a, (1, 5))[:, :E])
        check_points(dev(b), b, 1, CRAFT, 0.0, 8.0, "crafted rows of %d" % E, cutoff=1.0)
        t = np.ascontiguousarray(b.T)
        check_points(dev(t), t, 0, CRAFT, 0.0, 8.0, "crafted columns of %d" % E, cutoff=1.0)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_one_lane_never_stops(dtype):
    """a wave in which 63 columns stop at the first point and one never does, at several places of the wave, along both kinds of axis"""
    E = 70
    faint = np.resize(np.array([2.5, 3.5, 4.5]), E)
    for lane in (0, 17, 63):
        a = np.empty((128, E), dtype=dtype)
        a[:] = faint
        a[:, 0] = 1.5  # opaque at once
        a[lane] = faint
        a[64 + (lane + 5) % 64] = faint
        check_points(dev(a), a, 1, CRAFT, 0.0, 8.0, "rows, lane %d" % lane, cutoff=1.0)
        t = np.ascontiguousarray(a.T)
        check_points(dev(t), t, 0, CRAFT, 0.0, 8.0, "columns, lane %d" % lane, cutoff=1.0)


# ---- 4. ACCUMULATE ---------------------------------------------------------------------------------------------------------------------------
def test_accumulate():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    lo, hi = window(full)
    lut = make_lut(256, scale=0.1)
    d_lut = dev(lut)
    f = full.cpu().numpy()
    rng = np.random.default_rng(5)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for axis, cut in ((0, 30), (1, 20), (2, 64)):
            for rev in (False, True):
                lo_a = [0, 0, 0]
                ext_a = list(shape)
                ext_a[axis] = cut
                lo_b = [0, 0, 0]
                lo_b[axis] = cut
                ext_b = list(shape)
                ext_b[axis] = shape[axis] - cut
                first, second = (0, tuple(lo_a), tuple(ext_a)), (0, tuple(lo_b), tuple(ext_b))
                if rev:
                    first, second = second, first
                out = out_filled(shape, axis, cm.RGBA32F)
                st.composite([first + (out,)], axis, d_lut, lo, hi, reverse=rev)
                st.composite([second + (out,)], axis, d_lut, lo, hi, reverse=rev, accumulate=True)
                torch.cuda.synchronize()
                s1, s2 = slices_of(full, [first, second])
                carry = cm.expected(s1, axis, lut, lo, hi, reverse=rev)
                want = cm.expected(s2, axis, lut, lo, hi, reverse=rev, carry=carry)
                same_bytes(host(out), want, "a column split in two, axis %d reverse %s:" % (axis, rev))
                whole = cm.expected(f, axis, lut, lo, hi, reverse=rev)
                assert np.allclose(want, whole, rtol=1e-5, atol=1e-7) and (want != whole).any(), "the carry passes through float: close, not byte-equal"
            # into a buffer pre-filled with known RGBA, through composite_points too
            known = (rng.random(out_shape(shape, axis, cm.RGBA32F)) * 0.5).astype(np.float32)
            for run in ("stream", "points"):
                out = dev(known)
                if run == "stream":
                    st.composite([(0, (0, 0, 0), shape, out)], axis, d_lut, lo, hi, accumulate=True, cutoff=0.9)
                else:
                    sz3_amd.composite_points(full, axis, d_lut, lo, hi, accumulate=True, cutoff=0.9, out=out)
                torch.cuda.synchronize()
                same_bytes(host(out), cm.expected(f, axis, lut, lo, hi, cutoff=0.9, carry=known), "%s into known RGBA, axis %d:" % (run, axis))


# ---- 5. against the project itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_against_request_and_composite_points(dtype):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, dtype)
    items = mixed(shape)
    lo, hi = window(full)
    d_lut = dev(make_lut(256))
    with sz3_amd.open_stream(blob, np.dtype(dtype), device=DEV) as st:
        delivered = ask(st, items)
        for axis in range(3):
            for out_type, rev in COMBOS:
                got = st.composite(items, axis, d_lut, lo, hi, out_type, reverse=rev, level_opacity=True, level_bias=1, cutoff=0.97)
                torch.cuda.synchronize()
                for i, (g, d) in enumerate(zip(got, delivered)):
                    p = sz3_amd.composite_points(d, axis, d_lut, lo, hi, out_type, reverse=rev, level_bias=1 + items[i][0], cutoff=0.97)
                    assert tuple(g.shape) == out_shape(items[i][2], axis, out_type) == tuple(p.shape) and g.dtype == p.dtype
                    torch.cuda.synchronize()
                    assert host(g).tobytes() == host(p).tobytes(), "axis %d box %d: Stream.composite and composite_points over the request's tensor differ" % (axis, i)


def test_position_and_number_of_boxes(chain):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    rng = np.random.default_rng(17)
    many = []
    for i in range(255):
        k = int(rng.integers(0, 4))
        cs = coarse_shape(shape, k)
        ext = tuple(int(min(d, rng.integers(1, 13))) for d in cs)
        many.append((k, tuple(int(rng.integers(0, d - e + 1)) for d, e in zip(cs, ext)), ext))
    target = (1, (3, 2, 7), (21, 19, 33))
    tslice = slices_of(full, [target])
    lo, hi = window(full)
    lut = make_lut(256)
    d_lut = dev(lut)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        chain(0)
        for axis, out_type, rev in ((2, cm.RGBA32F, False), (0, cm.RGBA8, True), (1, cm.RGBA32F, True)):
            kw = dict(reverse=rev, level_opacity=True, cutoff=0.9)
            alone = check_composite(st, [target], tslice, axis, lut, lo, hi, out_type, **kw)[0]
            for place, others in [(0, many[:2]), (2, many[:2]), (27, many[:27]), (255, many)]:
                items = list(others[:place]) + [target] + list(others[place:])
                got = st.composite(items, axis, d_lut, lo, hi, out_type, **kw)
                torch.cuda.synchronize()
                assert host(got[place]).tobytes() == alone, "%d boxes, place %d" % (len(items), place)
            chain(2048)
            got = st.composite([target], axis, d_lut, lo, hi, out_type, **kw)
            torch.cuda.synchronize()
            assert st.stats()["chain_levels_last_request"] > 0 and host(got[0]).tobytes() == alone, "the chain at 2048"
            chain(0)
            with sz3_amd.debug_flags2(int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                items = many[:27] + [target]
                got = st.composite(items, axis, d_lut, lo, hi, out_type, **kw)
                torch.cuda.synchronize()
                assert host(got[27]).tobytes() == alone, "level group by level group"
                mi = mixed(shape)
                check_composite(st, mi, slices_of(full, mi), axis, lut, lo, hi, out_type, what="by level", **kw)


def test_launch_count(chain):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, "float32", (("interpAlgo", 0),))
    three = [(k,) + tile_boxes(coarse_shape(shape, k))[4] for k in (1, 0, 2)]
    twelve = three + [(k,) + tile_boxes(coarse_shape(shape, k))[j] for j in (2, 3, 5) for k in (2, 0, 1)]
    one_level = [[(k,) + tile_boxes(coarse_shape(shape, k))[j] for j in (4, 1, 4)] for k in (0, 1)]
    lo, hi = window(full)
    d_lut = dev(make_lut(256))

    def launches(f):
        l0 = L.sz3hip_debug_region_launches()
        f()
        n = L.sz3hip_debug_region_launches() - l0
        assert n == st.stats()["launches_last_request"]
        return n

    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for points in (0, 2048):
            chain(points)
            for items in [three, twelve, mixed(shape)] + one_level:
                q = launches(lambda: ask(st, items))
                cq = st.stats()["chain_levels_last_request"]
                for axis, out_type in ((0, "rgba32f"), (2, "rgba8"), (1, "rgba32f")):
                    r = launches(lambda: st.composite(items, axis, d_lut, lo, hi, out_type, level_opacity=True))
                    s = st.stats()
                    assert r == q and s["chain_levels_last_request"] == cq and s["chain_points"] == points, "a compositing issues the request's launches (%d, %d; threshold %d)" % (r, q, points)
            assert points == 0 or st.stats()["chain_levels_last_request"] > 0, "one level at threshold 2048 takes the chain"
            items = mixed(shape)
            with sz3_amd.debug_flags2(int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                q = launches(lambda: ask(st, items))
                assert launches(lambda: st.composite(items, 2, d_lut, lo, hi)) == q and launches(lambda: st.composite(items, 0, d_lut, lo, hi, "rgba8")) == q
        torch.cuda.synchronize()


def check_fallback(st, full, name):
    assert st.stats()["fast"] == 0
    slices = slices_of(full, FB_ITEMS)
    lo, hi = window(full)
    lut = make_lut(256)
    for axis in range(3):
        for out_type, rev in COMBOS:
            check_composite(st, FB_ITEMS, slices, axis, lut, lo, hi, out_type, what=name, reverse=rev, level_opacity=True)
            s = st.stats()
            assert s["fast"] == 0 and s["launches_last_request"] == 1 and s["chain_levels_last_request"] == 0


@pytest.mark.parametrize("name,kw", FALLBACKS[:2], ids=[f[0] for f in FALLBACKS[:2]])
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


# ---- 6. refusals and the handle's health -------------------------------------------------------------------------------------------------------
def refusals(st, full, good):
    N = len(good[0][1])
    n = len(good)
    einval = CODES["SZ3HIP_EINVAL"]
    before = st.stats()["requests"]
    arr, shapes = sz3_amd._boxes(N, [it[1:] for it in good])
    d_lut = dev(make_lut(16))
    levels = [it[0] for it in good]

    def refused(fragment, axis=0, out_type=0, edit=None, null_opts=False, **fields):
        name = "float32" if out_type == 0 else "int32"
        ax = min(axis, N - 1)
        outs = [out_filled(ext, ax, cm.RGBA32F if out_type == 0 else cm.RGBA8) for _, _, ext in good]
        reqs, _ = sz3_amd._composite_reqs(N, [it + (o,) for it, o in zip(good, outs)], shapes, arr, name, ax, st.device, True)
        o = sz3_amd._CCompositeOpts()
        o.lo, o.hi, o.cutoff, o.axis, o.out_type, o.lut_n, o.d_lut = 0.0, 1.0, INF, axis, out_type, 16, d_lut.data_ptr()
        for k, v in fields.items():
            setattr(o, k, v)
        if edit:
            edit(reqs, o)
        rc = L.sz3hip_stream_composite(st._h, reqs, n, None if null_opts else C.byref(o), sz3_amd._stream_handle(st.device, None))
        msg = L.sz3hip_last_error().decode()
        assert rc == einval and fragment in msg, (rc, msg, fragment)
        torch.cuda.synchronize()
        assert all((t.view(torch.uint8) == FILL).all() for t in outs), "a refused call wrote (%s)" % fragment
        # the handle serves the next request with the full decode's bytes
        same(ask(st, good[:3]), full, good[:3], "after a refusal (%s)" % fragment)

    refused("NULL argument (opts)", null_opts=True)
    refused("out_type (2)", out_type=2)
    refused("flags (0x8)", flags=8)
    refused("reserved word is 1", reserved=1)
    refused("axis (%d)" % N, axis=N)
    refused("is not finite", lo=float("nan"))
    refused("is empty", hi=0.0)
    refused("cutoff", cutoff=0.0)
    refused("cutoff", cutoff=float("nan"))
    refused("the table has 1 entries", lut_n=1)
    refused("the table has 1025 entries", lut_n=1025)
    refused("the table (d_lut) is NULL", d_lut=None)
    refused("the table (d_lut) is not aligned", d_lut=d_lut.data_ptr() + 4)
    refused("level_bias is 31", level_bias=31)
    top = max(levels)
    assert top > 0
    refused("box %d: level_bias (%d)" % (levels.index(top), 31 - top), level_bias=31 - top, flags=sz3_amd.COMPOSITE_LEVEL_OPACITY)
    refused("SZ3HIP_COMPOSITE_ACCUMULATE", out_type=1, flags=sz3_amd.COMPOSITE_ACCUMULATE)
    for b in (0, n // 2, n - 1):  # a box's: at the first, a middle and the last box
        def misalign16(reqs, o, b=b):
            reqs[b].d_out = reqs[b].d_out + 4
        refused("box %d: the output is not aligned to its element size (16 bytes)" % b, edit=misalign16)

        def misalign4(reqs, o, b=b):
            reqs[b].d_out = reqs[b].d_out + 2
        refused("box %d: the output is not aligned to its element size (4 bytes)" % b, out_type=1, edit=misalign4)

        def leave(reqs, o, b=b):
            reqs[b].box.lo[N - 1] = 1 << 40
        refused("box %d: " % b, edit=leave)

        def no_out(reqs, o, b=b):
            reqs[b].d_out = None
        refused("box %d: the output array is NULL" % b, edit=no_out)

        def res(reqs, o, b=b):
            reqs[b].reserved = 3
        refused("box %d: the reserved word" % b, edit=res)

        def negative(reqs, o, b=b):
            reqs[b].strides[N - 1] = -1
        if good[b][2][N - 1] > 1:
            refused("box %d: the view's stride of dimension %d is negative" % (b, N - 1), edit=negative)
        if b:
            def overlap(reqs, o, b=b):
                reqs[b].d_out = reqs[0].d_out
            refused("box %d: the output overlaps box 0's" % b, edit=overlap)
            refused("box %d: the output overlaps box 0's" % b, out_type=1, edit=overlap)
    assert st.stats()["requests"] > before


def test_refusals():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    good = mixed(shape)[:9]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        refusals(st, full, good)


def test_refusals_on_a_fallback_handle():
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **dict(FALLBACKS[0][1])))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 0
        refusals(st, full, FB_ITEMS[:6])


def test_refusals_of_composite_points():
    a = torch.zeros((4, 6), dtype=torch.float32, device=DEV)
    d_lut = dev(make_lut(16))
    buf = filled((4, 8, 4), "float32")
    with pytest.raises(ValueError):
        sz3_amd.composite_points(a, 2, d_lut, 0.0, 1.0)
    with pytest.raises(ValueError):
        sz3_amd.composite_points(a, 1, d_lut, 0.0, 1.0, out=buf[:, :6])  # (the input's shape, not the collapsed one)
    with pytest.raises(ValueError):
        sz3_amd.composite_points(a, 1, d_lut, 0.0, 1.0, "rgba8", out=buf[:, :1])  # (float32, not int32)
    with pytest.raises(ValueError, match="divisible by the component count 4"):
        sz3_amd.composite_points(a, 1, d_lut, 0.0, 1.0, out=filled((4, 1, 6), "float32")[:, :, :4])
    with pytest.raises(ValueError, match="must be contiguous"):
        sz3_amd.composite_points(a, 1, d_lut, 0.0, 1.0, out=filled((4, 1, 8), "float32")[:, :, ::2])
    with pytest.raises(ValueError):
        sz3_amd.composite_points(a, 1, d_lut[:, :3], 0.0, 1.0)
    with pytest.raises(ValueError):
        sz3_amd.composite_points(a, 1, d_lut.cpu(), 0.0, 1.0)
    with pytest.raises(ValueError):
        sz3_amd.composite_points(a.cpu(), 1, d_lut, 0.0, 1.0)
    with pytest.raises(sz3_amd.SZ3HipError, match="cutoff"):
        sz3_amd.composite_points(a, 1, d_lut, 0.0, 1.0, cutoff=0.0, out=buf[:, :1])
    with pytest.raises(sz3_amd.SZ3HipError, match="SZ3HIP_COMPOSITE_ACCUMULATE"):
        sz3_amd.composite_points(a, 1, d_lut, 0.0, 1.0, "rgba8", accumulate=True, out=filled((4, 1), "int32"))
    torch.cuda.synchronize()
    assert (buf.view(torch.uint8) == FILL).all()
    # two boxes that differ only along the axis share their output: refused, nothing written
    shape = (65, 47, 130)
    blob, full = case(shape)[1], case(shape)[2]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        out = filled((1, 5, 6, 4), "float32")
        with pytest.raises(sz3_amd.SZ3HipError, match="box 1: the output overlaps box 0's"):
            st.composite([(0, (0, 0, 0), (4, 5, 6), out), (0, (4, 0, 0), (4, 5, 6), out)], 0, d_lut, 0.0, 1.0)
        torch.cuda.synchronize()
        assert (out.view(torch.uint8) == FILL).all()
        same(ask(st, mixed(shape)[:3]), full, mixed(shape)[:3], "after the refusal")


# ---- 7. ordering -----------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_and_two_streams():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    items = mixed(shape)
    x_items, y_items = items[:9], items[5:]
    lo, hi = window(full)
    lut = make_lut(256)
    d_lut = dev(lut)
    qx = [([0.0, 0.0, 0.0], [[0.0, 0.0, 0.5]], [2 * ext[2] - 1]) for _, _, ext in x_items]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        want_x = check_composite(st, x_items, slices_of(full, x_items), 0, lut, lo, hi, cm.RGBA32F, cutoff=0.9)
        want_y = check_composite(st, y_items, slices_of(full, y_items), 2, lut, lo, hi, cm.RGBA8, reverse=True, level_opacity=True)
        want_red = st.reduce(x_items, 7, -0.5, 0.75).stats.cpu().numpy().tobytes()
        sel = st.select(y_items, lo, hi, 64)
        want_sel = [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()]
        want_map = [m.cpu().numpy().tobytes() for m in st.map(x_items, "u8", lo=lo, hi=hi)]
        want_smp = [t.cpu().numpy().tobytes() for t in st.sample(x_items, qx, "linear")]
        want_prj = [t.cpu().numpy().tobytes() for t in st.project(y_items, "sum", 2, out_dtype="float64")]
        want_grd = [t.cpu().numpy().tobytes() for t in st.gradient(x_items, "mag")]
        torch.cuda.synchronize()
        for _ in range(2):  # no host synchronisation in between
            cx0 = st.composite(x_items, 0, d_lut, lo, hi, cutoff=0.9)
            x = ask(st, x_items, sync=False, stream=s1)
            cy0 = st.composite(y_items, 2, d_lut, lo, hi, "rgba8", reverse=True, level_opacity=True, stream=s2)
            red = st.reduce(x_items, 7, -0.5, 0.75, stream=s1)
            cx1 = st.composite(x_items, 0, d_lut, lo, hi, cutoff=0.9, stream=s2)
            sel = st.select(y_items, lo, hi, 64)
            mp = st.map(x_items, "u8", lo=lo, hi=hi, stream=s1)
            cy1 = st.composite(y_items, 2, d_lut, lo, hi, "rgba8", reverse=True, level_opacity=True, stream=s1)
            smp = st.sample(x_items, qx, "linear", stream=s2)
            prj = st.project(y_items, "sum", 2, out_dtype="float64", stream=s1)
            grd = st.gradient(x_items, "mag", stream=s2)
            y = ask(st, y_items, sync=False, stream=s2)
            torch.cuda.synchronize()
            for outs in (cx0, cx1):
                assert [host(o).tobytes() for o in outs] == want_x
            for outs in (cy0, cy1):
                assert [host(o).tobytes() for o in outs] == want_y
            assert red.stats.cpu().numpy().tobytes() == want_red
            assert [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()] == want_sel
            assert [m.cpu().numpy().tobytes() for m in mp] == want_map
            assert [t.cpu().numpy().tobytes() for t in smp] == want_smp
            assert [t.cpu().numpy().tobytes() for t in prj] == want_prj
            assert [t.cpu().numpy().tobytes() for t in grd] == want_grd
            same(x, full, x_items)
            same(y, full, y_items)

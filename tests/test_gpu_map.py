"""Texels out of a request, on the MI355X: Stream.map, map_points.

Expected values come from numpy alone, over the full decode's [::2**k] slice s of the box with x = s.astype(float64): the code rule written in
numpy (np_codes), f16 as s.astype(float32).astype(float16), LUT32 as lut[codes]. Equality is in BYTES; the only exception is a NaN point of a
float output, checked with isnan. Every output lives in a buffer filled with 0x4D, and every byte outside the boxes' views — and every byte of
a refused call — must still be 0x4D afterwards: that is what holds the packed stores to their rows. Both store forms (the product's and the one
behind Dbg2.MAP_PLAIN_STORES) are held to the same bytes."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, conf_for, container, device_payload, smooth  # noqa: E402
from sink_models import (FILL, LAST, NAN_TEXEL, NP_OUT, TORCH_OUT, make_lut, map_expected as expected, map_filled as filled, map_host as host,  # noqa: E402,F401
                         map_untouched as untouched, np_codes, opts_for, same_texels, texel_atlas)
from test_gpu_request import FB_ITEMS, ask, chain, mixed, same  # noqa: E402,F401
from test_gpu_stream import SHAPES, IDS, case, coarse_shape, coarse_view, opens, tile_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
TYPES = ["u8", "u16", "f16", "f32", "lut32"]


def slices_of(full, items):
    return [coarse_view(full, k)[box_slices(lo, ext)].cpu().numpy() for k, lo, ext in items]


def window(full):
    """a middle band of the field's own values"""
    q = np.quantile(full.cpu().numpy().astype(np.float64), [0.25, 0.75])
    return float(q[0]), float(q[1])


def check_map(st, full, items, out_type, lo=0.0, hi=0.0, nan_code=0, lut=None, what="", slices=None):
    """Stream.map into contiguous outputs and into rectangles of one atlas, both against numpy; returns the contiguous outputs' bytes"""
    slices = slices_of(full, items) if slices is None else slices
    kw = opts_for(out_type, lo, hi, nan_code, lut)
    outs = [filled(ext, out_type) for _, _, ext in items]
    got = st.map([it + (o,) for it, o in zip(items, outs)], out_type, **kw)
    assert all(g is o for g, o in zip(got, outs))
    atlas, views, where = texel_atlas(items, out_type)
    st.map([it + (v,) for it, v in zip(items, views)], out_type, **kw)
    torch.cuda.synchronize()
    res = []
    for i, (it, s) in enumerate(zip(items, slices)):
        want = expected(s, out_type, lo, hi, nan_code, lut)
        w = "%s %s box %d %s:" % (what, out_type, i, it)
        same_texels(host(outs[i], out_type), want, out_type, w + " contiguous,")
        same_texels(host(views[i], out_type), want, out_type, w + " atlas,")
        res.append(host(outs[i], out_type).tobytes())
    # (repeated and overlapping boxes of `mixed` share no output here: every view is its own rectangle)
    assert untouched(atlas, out_type, where), what + " a byte outside the rectangles was written"
    return res


FORMS = [0, int(sz3_amd.Dbg2.MAP_PLAIN_STORES)]


@pytest.fixture(params=FORMS, ids=["packed", "plain"])
def form(request):
    with sz3_amd.debug_flags2(request.param):
        yield request.param


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
        lo, hi = window(full)
        slices = slices_of(full, items)
        with st:
            assert st.stats()["fast"] == (1 if fast else 0)
            n0 = st.stats()["requests"]
            for flags in FORMS:
                with sz3_amd.debug_flags2(flags):
                    for t in TYPES:
                        check_map(st, full, items, t, lo, hi, 3, lut, what="%s form %d" % (name, flags), slices=slices)
            assert st.stats()["requests"] == n0 + 2 * 2 * len(TYPES), "a map counts as a request"
            assert st.stats()["huffman_stages"] == (1 if fast else 0)


def test_stock_container(form):
    shape = (65, 47, 130)
    sz3_amd.set_stock_format(1)
    try:
        blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    lo, hi = window(full)
    lut = make_lut(256)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 1
        for t in TYPES:
            check_map(st, full, mixed(shape), t, lo, hi, 0, lut, what="stock")


# ---- 2. windows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_type", ["u8", "u16", "lut32"])
def test_windows(out_type, form):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    f = full.cpu().numpy().astype(np.float64)
    q = np.quantile(f, [0.4, 0.6])
    mn, mx = float(f.min()), float(f.max())
    windows = {"middle": (float(q[0]), float(q[1])), "everything": (mn, float(np.nextafter(mx, np.inf))), "below": (mx + 1.0, mx + 2.0), "above": (mn - 2.0, mn - 1.0)}
    # the mixed boxes and two single points: the field's smallest and largest value
    items = mixed(shape) + [(0, tuple(int(v) for v in np.unravel_index(i, shape)), (1, 1, 1)) for i in (f.argmin(), f.argmax())]
    lut = make_lut(1000)
    M = lut[0].size - 1 if out_type == "lut32" else LAST[out_type]
    slices = slices_of(full, items)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for name, (lo, hi) in windows.items():
            check_map(st, full, items, out_type, lo, hi, 9, lut, what=name, slices=slices)
            codes = [np_codes(s, lo, hi, M, 0) for s in slices]
            if name == "below":
                assert all((c == 0).all() for c in codes)
            elif name == "above":
                assert all((c == M).all() for c in codes)
            else:  # boxes all 0, all M, and spread over many codes
                assert any((c == 0).all() for c in codes) and any((c == M).all() for c in codes) and any(np.unique(c).size > min(M, 8) for c in codes), name


# ---- 3. edges, through map_points ------------------------------------------------------------------------------------------------------------
def points_into(src, out_view, out_type, lo=0.0, hi=0.0, nan_code=0, lut=None):
    got = sz3_amd.map_points(src, out_type, out=out_view, **opts_for(out_type, lo, hi, nan_code, lut))
    assert got is out_view


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("out_type", TYPES)
def test_row_heads_and_tails(out_type, dtype, form):
    """x extents around the packed pieces and the workgroup, every destination offset inside a word, rows whose pitch is odd"""
    rng = np.random.default_rng(23)
    lut = make_lut(256)
    rows = 3
    for ex in (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257):
        a = rng.normal(0.0, 1.0, (rows, ex)).astype(dtype)
        a[rng.integers(0, rows), rng.integers(0, ex)] = np.nan
        src = torch.from_numpy(a).to(DEV)
        want = expected(a, out_type, -1.0, 1.5, 7, lut)
        pitch = ex + 9 - (ex % 2)  # odd
        buf = filled((4 * rows + 1, pitch), out_type)
        where = [(slice(off * rows, off * rows + rows), slice(off, off + ex)) for off in range(4)]  # (offsets of 0 .. 3 texels: every byte offset of a one-byte row)
        for sl in where:
            points_into(src, buf[sl], out_type, -1.0, 1.5, 7, lut)
        torch.cuda.synchronize()
        for off, sl in enumerate(where):
            same_texels(host(buf[sl], out_type), want, out_type, "%s x extent %d offset %d:" % (out_type, ex, off))
        assert untouched(buf, out_type, where), "%s x extent %d: a byte outside the rows was written" % (out_type, ex)


@pytest.mark.parametrize("out_type", TYPES)
def test_totals_strides_and_dimensions(out_type, form):
    rng = np.random.default_rng(29)
    lut = make_lut(2)
    args = (-0.5, 0.5, 1, lut)
    for total in (1, 255, 256, 257, 3 * 256 + 1):
        for off in range(4):
            a = rng.normal(0.0, 1.0, total).astype(np.float32)
            buf = filled((total + 8,), out_type)
            points_into(torch.from_numpy(a).to(DEV), buf[off:off + total], out_type, *args)
            torch.cuda.synchronize()
            same_texels(host(buf[off:off + total], out_type), expected(a, out_type, *args), out_type, "total %d offset %d:" % (total, off))
            assert untouched(buf, out_type, [(slice(off, off + total),)])
    a = rng.normal(0.0, 1.0, (5, 131)).astype(np.float64)
    src = torch.from_numpy(a).to(DEV)
    # x stride 2 in the output
    buf = filled((6, 2 * 131 + 1), out_type)
    sl = (slice(0, 5), slice(1, 1 + 2 * 131, 2))
    points_into(src, buf[sl], out_type, *args)
    torch.cuda.synchronize()
    same_texels(host(buf[sl], out_type), expected(a, out_type, *args), out_type, "output x stride 2:")
    assert untouched(buf, out_type, [sl])
    # x stride 2 and a stride-0 broadcast in the input
    for view, ref in ((src[:, ::2], a[:, ::2]), (src[2:3, :].expand(4, 131), np.broadcast_to(a[2:3, :], (4, 131))), (src[:, 5:6].expand(5, 9), np.broadcast_to(a[:, 5:6], (5, 9)))):
        buf = filled((ref.shape[0] + 1, ref.shape[1] + 4), out_type)
        sl = (slice(1, 1 + ref.shape[0]), slice(3, 3 + ref.shape[1]))
        points_into(view, buf[sl], out_type, *args)
        torch.cuda.synchronize()
        same_texels(host(buf[sl], out_type), expected(ref, out_type, *args), out_type, "input strides %s:" % (tuple(view.stride()),))
        assert untouched(buf, out_type, [sl])
    # 4-D, a rectangle of a 4-D atlas
    a4 = rng.normal(0.0, 1.0, (3, 4, 5, 7)).astype(np.float32)
    buf = filled((4, 5, 6, 11), out_type)
    sl = (slice(1, 4), slice(0, 4), slice(1, 6), slice(3, 10))
    points_into(torch.from_numpy(a4).to(DEV), buf[sl], out_type, *args)
    torch.cuda.synchronize()
    same_texels(host(buf[sl], out_type), expected(a4, out_type, *args), out_type, "4-D:")
    assert untouched(buf, out_type, [sl])


def crafted(lo, hi, M):
    scale = (M + 1) / (hi - lo)
    v = [lo, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), hi, np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf), 0.0, -0.0, np.inf, -np.inf, np.nan,
         5e-324, -5e-324, 1e-310, 1e-40, -1e-40, float(np.float32(0.1)), 0.1, 1e300, -1e300]
    v += [lo + j / scale for j in (1, 2, 3, 100, M // 2, M - 1, M, M + 1)]  # (x - lo) * scale exactly an integer (scale is a power of two below)
    v += [np.nextafter(lo + j / scale, -np.inf) for j in (1, 2, 100, M)]
    return np.array(v, dtype=np.float64)


@pytest.mark.parametrize("nan_code", [0, 7, "last"])
@pytest.mark.parametrize("out_type", ["u8", "u16", "lut32"])
def test_crafted_values(out_type, nan_code, form):
    lut = make_lut(256 if nan_code == 0 else 1024 if nan_code == 7 else 1000)
    M = lut[0].size - 1 if out_type == "lut32" else LAST[out_type]
    nc = M if nan_code == "last" else nan_code
    for lo, hi in ((-1.0, 3.0), (0.0, 1.0), (0.1, 1.1), (-0.0, 2.0 ** -1000)):
        x = crafted(lo, hi, M)
        with np.errstate(over="ignore"):
            x32 = x.astype(np.float32)
        for a in (x, x32):
            buf = filled((a.size + 3,), out_type)
            points_into(torch.from_numpy(a).to(DEV), buf[1:1 + a.size], out_type, lo, hi, nc, lut)
            torch.cuda.synchronize()
            want = expected(a, out_type, lo, hi, nc, lut)
            same_texels(host(buf[1:1 + a.size], out_type), want, out_type, "%s window [%r, %r) %s:" % (out_type, lo, hi, a.dtype))
            nan = np.isnan(a)
            assert (want[nan] == (NAN_TEXEL if out_type == "lut32" else nc)).all() and nan.any()
    # 0.1f lies above a double lo of 0.1: code 0 by the window, not by the under rule; one step below lo is under all the same
    assert np_codes(np.float64(np.float32(0.1)), 0.1, 1.1, M, 0) == 0 and np.float64(np.float32(0.1)) > 0.1


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_half_and_float_outputs(dtype, form):
    two_step = 1.0 + 2.0 ** -11 + 2.0 ** -30  # f64 -> f16 rounds up; through f32 it first becomes the tie 1 + 2^-11, which goes to even: 1.0
    with np.errstate(over="ignore"):
        assert np.float64(two_step).astype(np.float16) != np.float64(two_step).astype(np.float32).astype(np.float16)
    v = [65504.0, 65519.99, 65520.0, 65536.0, -65520.0, 1e38, 1e300, 6.103515625e-05, 6.1e-05, 5.960464477539063e-08, 2.9802322387695312e-08, 2.99e-08, 8.9e-08,
         two_step, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, 1e-45, 5e-324, 1.0 / 3.0, 0.1]
    with np.errstate(over="ignore"):
        a = np.concatenate([np.array(v, dtype=np.float64), np.random.default_rng(3).normal(0, 100, 1000)]).astype(dtype)
    src = torch.from_numpy(a).to(DEV)
    for t in ("f16", "f32"):
        buf = filled((a.size + 4,), t)
        points_into(src, buf[1:1 + a.size], t)
        torch.cuda.synchronize()
        got = host(buf[1:1 + a.size], t)
        same_texels(got, expected(a, t), t, "%s from %s:" % (t, dtype))
        assert untouched(buf, t, [(slice(1, 1 + a.size),)])
        if t == "f16" and dtype == "float64":
            assert got[v.index(two_step)] == np.float16(1.0), "the two-step rounding is the definition"
    if dtype == "float32":  # F32 of a float is the value's bytes, NaN payloads included
        bits = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001], dtype=np.uint32)
        out = sz3_amd.map_points(torch.from_numpy(bits.view(np.float32).copy()).to(DEV), "f32")
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), bits)


@pytest.mark.parametrize("lut_n", [2, 256, 1000, 1024])
def test_lut(lut_n, form):
    lut = make_lut(lut_n)
    a = np.random.default_rng(lut_n).normal(0.0, 1.0, (7, 301))
    a[3, 5] = a[0, 0] = np.nan
    a[1, 1], a[2, 2] = np.inf, -np.inf
    for arr in (a, a.astype(np.float32)):
        out = sz3_amd.map_points(torch.from_numpy(arr).to(DEV), "lut32", lo=-2.0, hi=2.0, nan_code=NAN_TEXEL, lut=lut[1])
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, expected(arr, "lut32", -2.0, 2.0, 0, lut))
        assert got[3, 5] == NAN_TEXEL and got[1, 1] == lut[0][-1] and got[2, 2] == lut[0][0] and NAN_TEXEL not in lut[0]


# ---- 4. against the project itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_against_request_and_map_points(dtype, form):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, dtype)
    items = mixed(shape)
    lo, hi = window(full)
    lut = make_lut(1000)
    with sz3_amd.open_stream(blob, np.dtype(dtype), device=DEV) as st:
        delivered = ask(st, items)
        for t in TYPES:
            kw = opts_for(t, lo, hi, 5, lut)
            got = st.map(items, t, **kw)
            torch.cuda.synchronize()
            for i, (g, d) in enumerate(zip(got, delivered)):
                p = sz3_amd.map_points(d, t, **kw)
                torch.cuda.synchronize()
                assert host(g, t).tobytes() == host(p, t).tobytes(), "%s box %d: Stream.map and map_points over the request's tensor differ" % (t, i)
                if t == "f32" and dtype == "float32":
                    assert host(g, t).tobytes() == d.cpu().numpy().tobytes(), "F32 from a float handle is the request's bytes"


def test_codes_are_the_reduce_bins(form):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    items = mixed(shape)
    lo, hi = window(full)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        got = st.map(items, "u8", lo=lo, hi=hi)
        st_np, hist = st.reduce(items, bins=256, lo=lo, hi=hi).numpy()
        torch.cuda.synchronize()
        assert int(st_np["n_nonfinite"].sum()) == 0
        for i, g in enumerate(got):
            h = hist[i].astype(np.int64)
            folded = h[1:257].copy()
            folded[0] += h[0]
            folded[255] += h[257]
            assert np.array_equal(np.bincount(g.cpu().numpy().reshape(-1), minlength=256), folded), "box %d" % i


def test_position_and_number_of_boxes(chain, form):
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
    lo, hi = window(full)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        chain(0)
        for t in ("u8", "f16"):
            kw = opts_for(t, lo, hi, 0, None)
            alone = check_map(st, full, [target], t, lo, hi)[0]
            for place, others in [(0, many[:2]), (2, many[:2]), (27, many[:27]), (255, many)]:
                items = list(others[:place]) + [target] + list(others[place:])
                got = st.map(items, t, **kw)
                torch.cuda.synchronize()
                assert host(got[place], t).tobytes() == alone, "%s: %d boxes, place %d" % (t, len(items), place)
            chain(2048)
            got = st.map([target], t, **kw)
            torch.cuda.synchronize()
            assert st.stats()["chain_levels_last_request"] > 0 and host(got[0], t).tobytes() == alone, "the chain at 2048"
            chain(0)
            with sz3_amd.debug_flags2(form | int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                items = many[:27] + [target]
                got = st.map(items, t, **kw)
                torch.cuda.synchronize()
                assert host(got[27], t).tobytes() == alone, "level group by level group"
                check_map(st, full, mixed(shape), t, lo, hi, what="by level")
            L.sz3hip_debug_flags2(form)  # (the inner block's exit left 0)


# ---- 5. launch counts, fallback handles ------------------------------------------------------------------------------------------------------
def test_launch_count(chain, form):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, "float32", (("interpAlgo", 0),))
    lo, hi = window(full)
    three = [(k,) + tile_boxes(coarse_shape(shape, k))[4] for k in (1, 0, 2)]
    twelve = three + [(k,) + tile_boxes(coarse_shape(shape, k))[j] for j in (2, 3, 5) for k in (2, 0, 1)]
    one_level = [[(k,) + tile_boxes(coarse_shape(shape, k))[j] for j in (4, 1, 4)] for k in (0, 1)]

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
                for t in ("u8", "lut32"):
                    r = launches(lambda: st.map(items, t, **opts_for(t, lo, hi, 0, make_lut(256))))
                    s = st.stats()
                    assert r == q and s["chain_levels_last_request"] == cq and s["chain_points"] == points, "a map issues the request's launches (%d, %d; threshold %d)" % (r, q, points)
            assert points == 0 or st.stats()["chain_levels_last_request"] > 0, "one level at threshold 2048 takes the chain"
            items = mixed(shape)
            with sz3_amd.debug_flags2(form | int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                q = launches(lambda: ask(st, items))
                assert launches(lambda: st.map(items, "u16", lo=lo, hi=hi)) == q
            L.sz3hip_debug_flags2(form)  # (the inner block's exit left 0)
        torch.cuda.synchronize()


def check_fallback(st, full, name):
    assert st.stats()["fast"] == 0
    lo, hi = window(full)
    lut = make_lut(256)
    for t in TYPES:
        check_map(st, full, FB_ITEMS, t, lo, hi, 2, lut, what=name)
        s = st.stats()
        assert s["fast"] == 0 and s["launches_last_request"] == 1 and s["chain_levels_last_request"] == 0
    # a view with an x stride of 2 among rectangles
    outs = [filled(ext, "u8") for _, _, ext in FB_ITEMS]
    wide = filled((20, 9, 60), "u8")
    outs[1] = wide[..., ::2]
    st.map([it + (o,) for it, o in zip(FB_ITEMS, outs)], "u8", lo=lo, hi=hi)
    torch.cuda.synchronize()
    for o, s in zip(outs, slices_of(full, FB_ITEMS)):
        same_texels(host(o, "u8"), expected(s, "u8", lo, hi), "u8", name)
    assert untouched(wide, "u8", [(slice(None), slice(None), slice(0, 60, 2))])


@pytest.mark.parametrize("name,kw", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_fallback_containers(name, kw, form):
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **kw))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo not in INTERP_IDS
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        check_fallback(st, full, name)


def test_fallback_payload_of_a_device_context(form):
    shape = (40, 48, 56)
    dc, pl, size, full = device_payload(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0))
    with dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream) as st:
        pl.zero_()
        check_fallback(st, full, "payload")
    dc.close()


def test_fallback_openmp_slabs(monkeypatch, form):
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, openmp=1))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.openmp
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        check_fallback(st, full, "slabs")


# ---- 6. refusals and the handle's health -------------------------------------------------------------------------------------------------------
def refusals(st, full, good):
    N = len(good[0][1])
    n = len(good)
    einval = CODES["SZ3HIP_EINVAL"]
    before = st.stats()["requests"]
    lut = make_lut(16)
    arr, shapes = sz3_amd._boxes(N, [it[1:] for it in good])

    def refused(out_type, fragment, lo=0.0, hi=1.0, nan_code=0, lut_n=0, d_lut=None, flags=0, reserved=0, edit=None, null_opts=False):
        code, name = sz3_amd._map_type(out_type)
        outs = [filled(ext, out_type) for _, _, ext in good]
        reqs, _ = sz3_amd._map_reqs(N, [it + (o,) for it, o in zip(good, outs)], shapes, arr, name, st.device, True)
        o = sz3_amd._CMapOpts()
        o.lo, o.hi, o.out_type, o.flags, o.nan_code, o.lut_n, o.d_lut, o.reserved = lo, hi, code, flags, nan_code, lut_n, d_lut, reserved
        if edit:
            edit(reqs, o)
        rc = L.sz3hip_stream_map(st._h, reqs, n, None if null_opts else C.byref(o), sz3_amd._stream_handle(st.device, None))
        msg = L.sz3hip_last_error().decode()
        assert rc == einval and fragment in msg, (rc, msg, fragment)
        torch.cuda.synchronize()
        assert all((t.view(torch.uint8) == FILL).all() for t in outs), "a refused call wrote (%s)" % fragment
        # the handle serves the next request with the full decode's bytes
        same(ask(st, good[:3]), full, good[:3], "after a refusal (%s)" % fragment)

    def set_type(v):
        def f(reqs, o):
            o.out_type = v
        return f

    refused("u8", "NULL argument (opts)", null_opts=True)
    refused("u8", "out_type", edit=set_type(0))
    refused("u8", "out_type", edit=set_type(6))
    refused("u8", "flags", flags=1)
    refused("u8", "reserved", reserved=1)
    for t in ("u8", "u16", "lut32"):
        kw = dict(lut_n=16, d_lut=lut[1].data_ptr()) if t == "lut32" else {}
        refused(t, "not finite", lo=float("nan"), **kw)
        refused(t, "not finite", hi=float("inf"), **kw)
        refused(t, "is empty", lo=1.0, hi=1.0, **kw)
        refused(t, "is empty", lo=2.0, hi=1.0, **kw)
        refused(t, "too wide", lo=-1.7e308, hi=1.7e308, **kw)
    refused("u8", "nan_code", nan_code=256)
    refused("u16", "nan_code", nan_code=65536)
    refused("u8", "hold a table", lut_n=16)
    refused("u16", "hold a table", d_lut=lut[1].data_ptr())
    refused("lut32", "entries", lut_n=1, d_lut=lut[1].data_ptr())
    refused("lut32", "entries", lut_n=1025, d_lut=lut[1].data_ptr())
    refused("lut32", "d_lut) is NULL", lut_n=16)
    refused("lut32", "not aligned", lut_n=8, d_lut=lut[1].data_ptr() + 2)
    for t in ("f16", "f32"):
        refused(t, "take none", lo=0.0, hi=1.0)
        refused(t, "take none", hi=0.0, nan_code=1)
        refused(t, "take none", hi=0.0, lut_n=16)
        refused(t, "take none", hi=0.0, d_lut=lut[1].data_ptr())
    for b in (0, n // 2, n - 1):  # a box's: at the first, a middle and the last box
        def misalign(reqs, o, b=b):
            reqs[b].d_out = reqs[b].d_out + 1
        refused("u16", "box %d: the output is not aligned" % b, edit=misalign)
        refused("lut32", "box %d: the output is not aligned" % b, lut_n=16, d_lut=lut[1].data_ptr(), edit=misalign)

        def leave(reqs, o, b=b):
            reqs[b].box.lo[N - 1] = 1 << 40
        refused("u8", "box %d: " % b, edit=leave)

        def no_out(reqs, o, b=b):
            reqs[b].d_out = None
        refused("u8", "box %d: the output array is NULL" % b, edit=no_out)

        def res(reqs, o, b=b):
            reqs[b].reserved = 3
        refused("f16", "box %d: the reserved word" % b, hi=0.0, edit=res)
        if b:
            def overlap(reqs, o, b=b):
                reqs[b].d_out = reqs[0].d_out
            refused("u8", "box %d: the output overlaps box 0's" % b, edit=overlap)
    assert st.stats()["requests"] > before


def test_refusals(form):
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


def test_output_overlap_is_in_output_elements():
    """two u8 rectangles back to back: the last byte of one against the first of the next is accepted, one byte earlier refused"""
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    lo, hi = window(full)
    items = [(0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6))]
    want = [expected(s, "u8", lo, hi) for s in slices_of(full, items)]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        buf = filled((400,), "u8")
        outs = [buf[0:120].view(4, 5, 6), buf[120:240].view(4, 5, 6)]  # (as f32 views these hulls would overlap)
        st.map([it + (o,) for it, o in zip(items, outs)], "u8", lo=lo, hi=hi)
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            same_texels(host(o, "u8"), w, "u8")
        assert untouched(buf, "u8", [(slice(0, 240),)])
        buf = filled((400,), "u8")
        outs = [buf[0:120].view(4, 5, 6), buf[119:239].view(4, 5, 6)]
        with pytest.raises(sz3_amd.SZ3HipError, match="box 1: the output overlaps box 0's"):
            st.map([it + (o,) for it, o in zip(items, outs)], "u8", lo=lo, hi=hi)
        torch.cuda.synchronize()
        assert (buf == FILL).all()


# ---- 7. ordering -----------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_and_two_streams(form):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    items = mixed(shape)
    x_items, y_items = items[:9], items[5:]
    lo, hi = window(full)
    lut = make_lut(256)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        want_x = check_map(st, full, x_items, "u8", lo, hi)
        want_y = check_map(st, full, y_items, "lut32", lo, hi, 0, lut)
        want_red = st.reduce(x_items, 7, -0.5, 0.75).stats.cpu().numpy().tobytes()
        sel = st.select(y_items, lo, hi, 64)
        want_sel = [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()]
        torch.cuda.synchronize()
        for _ in range(2):  # no host synchronisation in between
            bx = [[filled(ext, "u8") for _, _, ext in x_items] for _ in range(2)]
            by = [[filled(ext, "lut32") for _, _, ext in y_items] for _ in range(2)]
            torch.cuda.synchronize()
            st.map([it + (o,) for it, o in zip(x_items, bx[0])], "u8", lo=lo, hi=hi)
            x = ask(st, x_items, sync=False, stream=s1)
            st.map([it + (o,) for it, o in zip(y_items, by[0])], "lut32", stream=s2, **opts_for("lut32", lo, hi, 0, lut))
            red = st.reduce(x_items, 7, -0.5, 0.75, stream=s1)
            st.map([it + (o,) for it, o in zip(x_items, bx[1])], "u8", lo=lo, hi=hi, stream=s2)
            sel = st.select(y_items, lo, hi, 64)
            st.map([it + (o,) for it, o in zip(y_items, by[1])], "lut32", stream=s1, **opts_for("lut32", lo, hi, 0, lut))
            y = ask(st, y_items, sync=False, stream=s2)
            torch.cuda.synchronize()
            for outs in bx:
                assert [host(o, "u8").tobytes() for o in outs] == want_x
            for outs in by:
                assert [host(o, "lut32").tobytes() for o in outs] == want_y
            assert red.stats.cpu().numpy().tobytes() == want_red
            assert [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()] == want_sel
            same(x, full, x_items)
            same(y, full, y_items)

"""Boxes projected along an axis, on the MI355X: Stream.project, project_points.

Expected values come from numpy alone, over the full decode's [::2**k] slice of the box as float64: the rule written as a Python loop over the
axis index on whole slices (np_fold: s = s + x[i] — never np.sum, which sums pairwise). Equality is in BYTES; the only exception is a NaN
output, checked with isnan. Every output lives in a buffer filled with 0x4D, and every byte outside the views — and every byte of a refused
call — must still be 0x4D afterwards.

The kernels' constants the extents below bracket (sz3hip_project.hip): a workgroup is 256 output points; the body for an axis that is not the
fastest issues PRJ_BATCH = 8 loads ahead of the fold (axis extents 1, 7, 8, 9, 17); the body for the fastest axis gives a wave 64 rows and
steps 256 / sizeof(T) columns at a time — 64 for f32, 32 for f64 (axis extents 1, 2, 31, 32, 33, 63, 64, 65, 129; 1, 63, 64, 65, 257 rows) —
and loads its rows in batches of 8 (f32) or 16 (f64)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, conf_for, container, device_payload, smooth  # noqa: E402
from sink_models import (FILL, INDEX_OPS, NAN, OPS, OUTS, atlas_of, combos, flat, np_fold, out_name, project_expected as expected,  # noqa: E402,F401
                         project_filled as filled, project_host as host, project_untouched as untouched, same_bytes)
from test_gpu_request import FB_ITEMS, ask, chain, mixed, same  # noqa: E402,F401
from test_gpu_stream import SHAPES, IDS, case, coarse_shape, coarse_view, opens, tile_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()


def slices_of(full, items):
    return [coarse_view(full, k)[box_slices(lo, ext)].cpu().numpy() for k, lo, ext in items]


def check_project(st, items, folds, op, axis, out, fill=NAN, what="", atlas=True):
    """Stream.project into contiguous outputs and into rectangles of one atlas, both against numpy; returns the contiguous outputs' bytes"""
    name = out_name(op, out, st.dtype)
    shapes = [flat(ext, axis) for _, _, ext in items]
    outs = [filled(s, name) for s in shapes]
    got = st.project([it + (o,) for it, o in zip(items, outs)], op, axis, out_dtype=out, fill=fill)
    assert all(g is o for g, o in zip(got, outs))
    if atlas:
        at, views, where = atlas_of(shapes, name)
        st.project([it + (v,) for it, v in zip(items, views)], op, axis, out_dtype=out, fill=fill)
    torch.cuda.synchronize()
    res = []
    for i, (it, f) in enumerate(zip(items, folds)):
        want = expected(f, op, axis, name, fill)
        w = "%s %s axis %d -> %s box %d %s:" % (what, op, axis, name, i, it)
        same_bytes(host(outs[i]), want, w + " contiguous,")
        if atlas:
            same_bytes(host(views[i]), want, w + " atlas,")
        res.append(host(outs[i]).tobytes())
    assert not atlas or untouched(at, where), what + " a byte outside the rectangles was written"
    return res


# ---- 1. shapes and opens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shapes_and_opens(shape, dtype, interp):
    kw = (("interpAlgo", interp),)
    items = mixed(shape)
    algo = case(shape, dtype, kw)[3].cmprAlgo
    for name, st, full in opens(shape, dtype, kw):
        fast = name == "open_payload" or algo in INTERP_IDS
        slices = slices_of(full, items)
        with st:
            assert st.stats()["fast"] == (1 if fast else 0)
            n0 = st.stats()["requests"]
            calls = 0
            for axis in range(len(shape)):
                folds = [np_fold(s, axis) for s in slices]
                for op, out in combos():
                    check_project(st, items, folds, op, axis, out, what=name)
                    calls += 2
            assert st.stats()["requests"] == n0 + calls, "a projection counts as a request"
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
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 1
        for axis in range(3):
            folds = [np_fold(s, axis) for s in slices]
            for op, out in combos():
                check_project(st, items, folds, op, axis, out, what="stock")


# ---- 2. extents, strides and dimensions, through project_points --------------------------------------------------------------------------------
def check_points(src, ref, axis, what="", fill=NAN, ops=None):
    """project_points of the device view `src` (host values `ref`) into a rectangle of a 0x4D buffer, every op and output type"""
    f = np_fold(ref, axis)
    shape = flat(ref.shape, axis)
    sl = tuple(slice(1, 1 + e) for e in shape)
    calls = []
    for op, out in (ops or combos()):
        name = out_name(op, out, ref.dtype)
        buf = filled([e + 2 for e in shape], name)
        got = sz3_amd.project_points(src, op, axis, out_dtype=out, fill=fill, out=buf[sl])
        assert got.data_ptr() == buf[sl].data_ptr()
        calls.append((op, name, buf))
    torch.cuda.synchronize()
    for op, name, buf in calls:
        same_bytes(host(buf[sl]), expected(f, op, axis, name, fill), "%s %s -> %s, shape %s axis %d:" % (what, op, name, ref.shape, axis))
        assert untouched(buf, [sl]), "%s %s: a byte outside the view was written" % (what, op)


def noisy(rng, shape, dtype):
    """normal values with a NaN, an Inf and a -Inf somewhere (where there is room)"""
    a = rng.normal(0.0, 1.0, shape).astype(dtype)
    v = a.reshape(-1)
    if v.size >= 8:
        v[rng.integers(0, v.size, 3)] = [np.nan, np.inf, -np.inf]
    return a


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fastest_axis_extents(dtype):
    rng = np.random.default_rng(31)
    for rows in (1, 63, 64, 65, 257):
        for ex in (1, 2, 31, 32, 33, 63, 64, 65, 129):
            a = noisy(rng, (rows, ex), dtype)
            check_points(torch.from_numpy(a).to(DEV), a, 1, "rows %d" % rows)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_other_axis_extents(dtype):
    rng = np.random.default_rng(37)
    for outs in (1, 255, 256, 257):
        for ex in (1, 7, 8, 9, 17):
            a = noisy(rng, (ex, outs), dtype)
            check_points(torch.from_numpy(a).to(DEV), a, 0, "outputs %d" % outs)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dimensions_and_strides(dtype):
    rng = np.random.default_rng(41)
    short = [("max", None), ("sum", "float64"), ("argmin", None), ("mean", "float32")]
    # 1-D .. 4-D, every axis; extent-1 dimensions in every place
    for shape in ((1,), (77,), (9, 70), (3, 5, 67), (3, 4, 5, 66), (1, 9, 1, 70), (9, 1, 70, 1), (1, 1, 40), (40, 1, 1), (2, 1, 3, 1, 37), (5, 37, 1)):
        a = noisy(rng, shape, dtype)
        for axis in range(len(shape)):
            check_points(torch.from_numpy(a).to(DEV), a, axis, "dims", ops=short if len(shape) > 4 else None)
    a = noisy(rng, (6, 7, 140), dtype)
    src = torch.from_numpy(a).to(DEV)
    views = [("x stride 2", src[:, :, ::2], a[:, :, ::2]),
             ("broadcast rows", src[:, 2:3, :].expand(6, 5, 140), np.broadcast_to(a[:, 2:3, :], (6, 5, 140))),
             ("broadcast x", src[:, :, 9:10].expand(6, 7, 70), np.broadcast_to(a[:, :, 9:10], (6, 7, 70))),
             ("broadcast slowest", src[1:2].expand(9, 7, 140), np.broadcast_to(a[1:2], (9, 7, 140))),
             ("transposed", src.permute(2, 0, 1), a.transpose(2, 0, 1)),
             ("transposed 2", src.transpose(1, 2), a.transpose(0, 2, 1))]
    for what, v, ref in views:
        for axis in range(3):
            check_points(v, np.ascontiguousarray(ref), axis, what, fill=-7.25)
    # negative axes and allocated outputs
    out = sz3_amd.project_points(src, "sum", -1)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (6, 7, 1) and out.dtype == src.dtype and out.is_contiguous()
    same_bytes(host(out), expected(np_fold(a, 2), "sum", 2, dtype))
    out = sz3_amd.project_points(src, "argmax", 0)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 7, 140) and out.dtype == torch.int32
    same_bytes(host(out), expected(np_fold(a, 0), "argmax", 0, "int32"))


# ---- 3. crafted columns ----------------------------------------------------------------------------------------------------------------------
def cancellation(E):
    """a column whose sequential sum differs from numpy's pairwise sum: the case holds the fold's order"""
    for seed in range(100):
        rng = np.random.default_rng(seed)
        x = rng.normal(0.0, 1.0, E) * 10.0 ** rng.integers(-8, 9, E)
        s = 0.0
        for v in x:
            s = s + v
        if s != np.sum(x):
            return x
    raise AssertionError("no cancellation column found")


def crafted(dtype):
    """columns of 16 points, one per row"""
    E = 16
    f32 = np.dtype(dtype) == np.float32
    big, tiny = (3e38, 1e-45) if f32 else (1e308, 5e-324)
    n, i = np.nan, np.inf
    cols = [[n] * E,
            [i, -i] * (E // 2),
            [n, i] * (E // 2),
            [2.5] + [n] * (E - 1),
            [n] * (E - 1) + [-2.5],
            [i, n, 7.0] + [n, -i] * 6 + [n],
            [-0.0, 0.0] * (E // 2),
            [0.0, -0.0] * (E // 2),
            [n, -0.0, 0.0, -0.0] * (E // 4),
            [1.0, 5.0, 5.0, 2.0, 5.0, -3.0, -3.0, 5.0] * 2,
            [-4.0, -4.0, 3.0, 3.0] * 4,
            [tiny, -tiny, 2 * tiny, 1e-40, -1e-40, 0.0, tiny, tiny] * 2,
            [tiny] * E,
            [big, big] + [n] * (E - 2),
            [big, big, -big, -big] * 4,
            [-big, -big, 1.0] + [0.0] * (E - 3),
            list(cancellation(E).astype(dtype)),
            list(np.arange(E, dtype=np.float64) - 7.5)]
    if not f32:
        cols += [[1e300, -1e300, 1e39, -1e39] * 4, [n, 3.5e38, n, 1e-50] * 4, [2.0 ** -150, 2.0 ** -149, 2.0 ** -127] + [n] * (E - 3)]
    with np.errstate(over="ignore"):
        return np.array(cols, dtype=np.float64).astype(dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_crafted_columns(dtype):
    x = cancellation(16)
    seq = 0.0
    for v in x:
        seq = seq + v
    assert seq != np.sum(x), "the cancellation column tells the sequential fold from the pairwise one"
    a = crafted(dtype)
    f = np_fold(a, 1)
    # what the cases are there for
    assert (f["count"][:3] == 0).all() and f["argmin"][0] == 16 and f["argmax"][1] == 16 and f["sum"][2] == 0.0
    assert (f["argmin"][3], f["argmax"][3], f["argmin"][4], f["argmax"][4], f["argmin"][5]) == (0, 0, 15, 15, 2)
    assert (f["argmin"][6], f["argmax"][6], f["argmin"][7], f["argmax"][8]) == (0, 0, 0, 1), "-0.0 and +0.0 tie: the first wins"
    assert np.signbit(f["min"][6]) and np.signbit(f["max"][6]) and not np.signbit(f["min"][7]) and np.signbit(f["max"][8]), "the element's sign of zero is kept"
    assert (f["argmax"][9], f["argmin"][9], f["argmax"][10], f["argmin"][10]) == (1, 5, 2, 0), "equal extrema: the first index wins"
    if dtype == "float64":
        assert np.isinf(f["sum"][13]) and f["count"][13] == 2, "Inf out of finite points"
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(f["max"][-3])) and np.isinf(np.float32(f["min"][-3])), "beyond f32's range"
    for fill in (NAN, -7.25, np.inf):
        check_points(torch.from_numpy(a).to(DEV), a, 1, "crafted rows", fill=fill)
        t = np.ascontiguousarray(a.T)
        check_points(torch.from_numpy(t).to(DEV), t, 0, "crafted columns", fill=fill)
    # the same columns 70 and 9 points long (several steps of both bodies): the column repeated, then cut
    for E in (70, 9):
        b = np.ascontiguousarray(np.tile(a, (1, 5))[:, :E])
        check_points(torch.from_numpy(b).to(DEV), b, 1, "crafted rows of %d" % E)
        t = np.ascontiguousarray(b.T)
        check_points(torch.from_numpy(t).to(DEV), t, 0, "crafted columns of %d" % E)


def test_sum_keeps_the_order_whichever_axis():
    """long cancellation columns along every axis of a 3-D array: the sequential sum's bytes, which the pairwise sum misses"""
    rng = np.random.default_rng(43)
    a = rng.normal(0.0, 1.0, (150, 140, 130)) * 10.0 ** rng.integers(-8, 9, (150, 140, 130))
    src = torch.from_numpy(a).to(DEV)
    for axis in range(3):
        f = np_fold(a, axis)
        pairwise = np.sum(np.ascontiguousarray(np.moveaxis(a, axis, -1)), axis=-1)  # (numpy sums a contiguous last axis pairwise)
        assert (pairwise != f["sum"]).any(), "numpy's own sum differs from the sequential fold"
        for op in ("sum", "mean"):
            got = sz3_amd.project_points(src, op, axis)
            torch.cuda.synchronize()
            same_bytes(host(got), expected(f, op, axis, "float64"), "%s axis %d:" % (op, axis))


# ---- 4. against the project itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_against_request_and_project_points(dtype):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, dtype)
    items = mixed(shape)
    with sz3_amd.open_stream(blob, np.dtype(dtype), device=DEV) as st:
        delivered = ask(st, items)
        for axis in range(3):
            for op, out in combos():
                got = st.project(items, op, axis, out_dtype=out, fill=-1.5)
                torch.cuda.synchronize()
                for i, (g, d) in enumerate(zip(got, delivered)):
                    p = sz3_amd.project_points(d, op, axis, out_dtype=out, fill=-1.5)
                    assert tuple(g.shape) == flat(items[i][2], axis) == tuple(p.shape) and g.dtype == p.dtype
                    torch.cuda.synchronize()
                    assert host(g).tobytes() == host(p).tobytes(), "%s axis %d box %d: Stream.project and project_points over the request's tensor differ" % (op, axis, i)


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
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        chain(0)
        for op, axis, out in (("sum", 2, None), ("argmax", 0, None), ("mean", 1, "float64")):
            alone = check_project(st, [target], [np_fold(tslice[0], axis)], op, axis, out)[0]
            for place, others in [(0, many[:2]), (2, many[:2]), (27, many[:27]), (255, many)]:
                items = list(others[:place]) + [target] + list(others[place:])
                got = st.project(items, op, axis, out_dtype=out)
                torch.cuda.synchronize()
                assert host(got[place]).tobytes() == alone, "%s: %d boxes, place %d" % (op, len(items), place)
            chain(2048)
            got = st.project([target], op, axis, out_dtype=out)
            torch.cuda.synchronize()
            assert st.stats()["chain_levels_last_request"] > 0 and host(got[0]).tobytes() == alone, "the chain at 2048"
            chain(0)
            with sz3_amd.debug_flags2(int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                items = many[:27] + [target]
                got = st.project(items, op, axis, out_dtype=out)
                torch.cuda.synchronize()
                assert host(got[27]).tobytes() == alone, "level group by level group"
                mi = mixed(shape)
                check_project(st, mi, [np_fold(s, axis) for s in slices_of(full, mi)], op, axis, out, what="by level")


# ---- 5. launch counts, fallback handles ------------------------------------------------------------------------------------------------------
def test_launch_count(chain):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, "float32", (("interpAlgo", 0),))
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
                for op, axis in (("max", 0), ("sum", 2), ("count", 1)):
                    r = launches(lambda: st.project(items, op, axis))
                    s = st.stats()
                    assert r == q and s["chain_levels_last_request"] == cq and s["chain_points"] == points, "a projection issues the request's launches (%d, %d; threshold %d)" % (r, q, points)
            assert points == 0 or st.stats()["chain_levels_last_request"] > 0, "one level at threshold 2048 takes the chain"
            items = mixed(shape)
            with sz3_amd.debug_flags2(int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                q = launches(lambda: ask(st, items))
                assert launches(lambda: st.project(items, "mean", 2)) == q and launches(lambda: st.project(items, "argmin", 0)) == q
        torch.cuda.synchronize()


def check_fallback(st, full, name):
    assert st.stats()["fast"] == 0
    slices = slices_of(full, FB_ITEMS)
    for axis in range(3):
        folds = [np_fold(s, axis) for s in slices]
        for op, out in combos():
            check_project(st, FB_ITEMS, folds, op, axis, out, what=name)
            s = st.stats()
            assert s["fast"] == 0 and s["launches_last_request"] == 1 and s["chain_levels_last_request"] == 0
    # a view with an x stride of 2 among contiguous outputs
    outs = [filled(flat(ext, 0), "float32") for _, _, ext in FB_ITEMS]
    wide = filled((1, 9, 60), "float32")
    outs[1] = wide[..., ::2]
    st.project([it + (o,) for it, o in zip(FB_ITEMS, outs)], "max", 0)
    torch.cuda.synchronize()
    for o, s in zip(outs, slices):
        same_bytes(host(o), expected(np_fold(s, 0), "max", 0, "float32"), name)
    assert untouched(wide, [(slice(None), slice(None), slice(0, 60, 2))])


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


# ---- 6. refusals and the handle's health -------------------------------------------------------------------------------------------------------
def refusals(st, full, good):
    N = len(good[0][1])
    n = len(good)
    einval = CODES["SZ3HIP_EINVAL"]
    before = st.stats()["requests"]
    arr, _ = sz3_amd._boxes(N, [it[1:] for it in good])

    def refused(fragment, op="max", axis=0, out_type=0, reserved=0, edit=None, null_opts=False, name="float32"):
        shapes = [flat(ext, min(axis, N - 1)) for _, _, ext in good]
        outs = [filled(s, name) for s in shapes]
        reqs, _ = sz3_amd._map_reqs(N, [it + (o,) for it, o in zip(good, outs)], shapes, arr, name, st.device, True)
        o = sz3_amd._CProjectOpts()
        o.op, o.axis, o.out_type, o.reserved, o.fill = OPS.index(op) if isinstance(op, str) else op, axis, out_type, reserved, NAN
        if edit:
            edit(reqs, o)
        rc = L.sz3hip_stream_project(st._h, reqs, n, None if null_opts else C.byref(o), sz3_amd._stream_handle(st.device, None))
        msg = L.sz3hip_last_error().decode()
        assert rc == einval and fragment in msg, (rc, msg, fragment)
        torch.cuda.synchronize()
        assert all((t.view(torch.uint8) == FILL).all() for t in outs), "a refused call wrote (%s)" % fragment
        # the handle serves the next request with the full decode's bytes
        same(ask(st, good[:3]), full, good[:3], "after a refusal (%s)" % fragment)

    refused("NULL argument (opts)", null_opts=True)
    refused("op (7)", op=7)
    refused("op (4294967295)", op=0xFFFFFFFF)
    refused("axis (%d)" % N, axis=N)
    refused("axis (4294967295)", axis=0xFFFFFFFF)
    refused("out_type (2)", out_type=2)
    for op in INDEX_OPS:
        refused("an index op", op=op, out_type=1, name="int32")
    refused("reserved word is 1", reserved=1)
    for b in (0, n // 2, n - 1):  # a box's: at the first, a middle and the last box
        def misalign4(reqs, o, b=b):
            reqs[b].d_out = reqs[b].d_out + 2
        refused("box %d: the output is not aligned to its element size (4 bytes)" % b, edit=misalign4)
        refused("box %d: the output is not aligned to its element size (4 bytes)" % b, op="count", edit=misalign4, name="int32")

        def misalign8(reqs, o, b=b):
            reqs[b].d_out = reqs[b].d_out + 4
        refused("box %d: the output is not aligned to its element size (8 bytes)" % b, out_type=1, edit=misalign8, name="float64")

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


def test_refusals_of_project_points():
    a = torch.zeros((4, 6), dtype=torch.float32, device=DEV)
    buf = filled((4, 8), "float32")
    with pytest.raises(ValueError):
        sz3_amd.project_points(a, "max", 2)
    with pytest.raises(ValueError):
        sz3_amd.project_points(a, "max", 1, out=buf[:, :6])  # (the input's shape, not the collapsed one)
    with pytest.raises(ValueError):
        sz3_amd.project_points(a, "argmax", 1, out=buf[:, :1])  # (float32, not int32)
    with pytest.raises(ValueError):
        sz3_amd.project_points(a, "count", 1, out_dtype="float32")
    with pytest.raises(ValueError):
        sz3_amd.project_points(a.cpu(), "max", 1)
    with pytest.raises(sz3_amd.SZ3HipError, match="permuted or overlap"):
        sz3_amd.project_points(torch.zeros((4, 5, 6), dtype=torch.float32, device=DEV), "max", 0, out=filled((6, 5, 1), "float32").permute(2, 1, 0))
    o = sz3_amd._CProjectOpts()  # (torch makes no misaligned float64 view: the C call, an f64 output 4 bytes off)
    o.op, o.axis, o.out_type = sz3_amd.PROJECT_SUM, 1, 1
    dims, strides = (C.c_uint64 * 2)(4, 6), (C.c_int64 * 2)(6, 1)
    rc = L.sz3hip_project_device(0, 2, dims, a.data_ptr(), strides, C.byref(o), buf.data_ptr() + 4, None, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and "not aligned to its element size (8 bytes)" in L.sz3hip_last_error().decode()
    torch.cuda.synchronize()
    assert (buf.view(torch.uint8) == FILL).all()
    # two boxes that differ only along the axis share their output: refused, nothing written
    shape = (65, 47, 130)
    blob, full = case(shape)[1], case(shape)[2]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        out = filled((1, 5, 6), "float32")
        with pytest.raises(sz3_amd.SZ3HipError, match="box 1: the output overlaps box 0's"):
            st.project([(0, (0, 0, 0), (4, 5, 6), out), (0, (4, 0, 0), (4, 5, 6), out)], "sum", 0)
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
    f = full.cpu().numpy().astype(np.float64)
    lo, hi = [float(v) for v in np.quantile(f, [0.25, 0.75])]
    qx = [([0.0, 0.0, 0.0], [[0.0, 0.0, 0.5]], [2 * ext[2] - 1]) for _, _, ext in x_items]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        want_x = check_project(st, x_items, [np_fold(s, 0) for s in slices_of(full, x_items)], "max", 0, None)
        want_y = check_project(st, y_items, [np_fold(s, 2) for s in slices_of(full, y_items)], "sum", 2, "float64")
        want_red = st.reduce(x_items, 7, -0.5, 0.75).stats.cpu().numpy().tobytes()
        sel = st.select(y_items, lo, hi, 64)
        want_sel = [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()]
        want_map = [m.cpu().numpy().tobytes() for m in st.map(x_items, "u8", lo=lo, hi=hi)]
        want_smp = [t.cpu().numpy().tobytes() for t in st.sample(x_items, qx, "linear")]
        torch.cuda.synchronize()
        for _ in range(2):  # no host synchronisation in between
            px0 = st.project(x_items, "max", 0)
            x = ask(st, x_items, sync=False, stream=s1)
            py0 = st.project(y_items, "sum", 2, out_dtype="float64", stream=s2)
            red = st.reduce(x_items, 7, -0.5, 0.75, stream=s1)
            px1 = st.project(x_items, "max", 0, stream=s2)
            sel = st.select(y_items, lo, hi, 64)
            mp = st.map(x_items, "u8", lo=lo, hi=hi, stream=s1)
            py1 = st.project(y_items, "sum", 2, out_dtype="float64", stream=s1)
            smp = st.sample(x_items, qx, "linear", stream=s2)
            y = ask(st, y_items, sync=False, stream=s2)
            torch.cuda.synchronize()
            for outs in (px0, px1):
                assert [host(o).tobytes() for o in outs] == want_x
            for outs in (py0, py1):
                assert [host(o).tobytes() for o in outs] == want_y
            assert red.stats.cpu().numpy().tobytes() == want_red
            assert [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()] == want_sel
            assert [m.cpu().numpy().tobytes() for m in mp] == want_map
            assert [t.cpu().numpy().tobytes() for t in smp] == want_smp
            same(x, full, x_items)
            same(y, full, y_items)

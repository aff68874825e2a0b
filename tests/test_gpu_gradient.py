"""Gradients of boxes, on the MI355X: Stream.gradient, gradient_points.

Expected values come from numpy alone (gradient_model.py: the header's rule on float64 slices), over the full decode's [::2**k] slice of the
box. Equality is in BYTES; the only exception is a NaN output, checked with isnan. MAG is compared with np.sqrt of the model's MAG2: the ROCm
tree states no bound for the device's sqrt(double), so the allowance is ONE unit in the last place of the output type, and the results that
differ at all are counted and printed (test_mag_against_numpys_root; DESIGN.md section 23 holds the count). Stream.gradient against gradient_points stays byte
for byte for MAG too. Every output lives in a buffer filled with 0x4D, and every byte outside the views — and every byte of a refused call —
must still be 0x4D afterwards.

The kernel's constants the extents below bracket (sz3hip_gradient.hip): a workgroup is 256 OUTPUT points; along a differentiated axis the
extents 1 (no difference), 2 (two one-sided points), 3 (one central point) and above take the clamped neighbours."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import gradient_model as gm  # noqa: E402
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, conf_for, container, device_payload, smooth  # noqa: E402
from sink_models import FILL, atlas_of, project_filled as filled, project_host as host, project_untouched as untouched  # noqa: E402
from test_gpu_request import FB_ITEMS, ask, chain, mixed, same  # noqa: E402,F401
from test_gpu_stream import SHAPES, IDS, case, coarse_shape, coarse_view, opens, tile_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
OPS = ("deriv", "mag2", "mag", "vector")
OUTS = ("float32", "float64")
ANISO = (0.5, 1.25, 3.0, 7.0)


def combos(N):
    return [("deriv", a) for a in range(N)] + [("mag2", 0), ("mag", 0), ("vector", 0)]


def full_shape(ext, op, axis, interior=False):
    s = gm.out_shape(tuple(ext), op, axis, interior)
    return s + (len(ext),) if op == "vector" else s


def slices_of(full, items):
    return [coarse_view(full, k)[box_slices(lo, ext)].cpu().numpy() for k, lo, ext in items]


def expect(got, values, op, axis, spacing, level, name, interior=False, what=""):
    """one output against the model: bytes, or for MAG one unit in the last place of the output type around sqrt(model's MAG2)"""
    if op != "mag":
        want = gm.gradient(values, op, axis, spacing, level, name, interior)
        assert got.shape == want.shape and got.dtype == want.dtype, "%s %s %s / %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
        assert gm.same_bytes(got, want), "%s the bytes differ from the rule's: got %r want %r" % (what, got.reshape(-1)[:4], want.reshape(-1)[:4])
        return
    m = gm.gradient(values, "mag", axis, spacing, level, name, interior, sqrt=False)
    with np.errstate(all="ignore"):
        want = np.sqrt(m).astype(name)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    worst = gm.ulp_apart(got, want)[1]
    assert worst <= 1, "%s MAG lies %d units in the last place from sqrt(MAG2)" % (what, worst)


def check_gradient(st, items, slices, op, axis, out, spacing, interior=False, what="", atlas=True):
    """Stream.gradient into contiguous outputs and into rectangles of one atlas with an odd pitch, both against the model; returns the
    contiguous outputs' bytes"""
    name = out or st.dtype.name
    N = len(items[0][1])
    shapes = [full_shape(ext, op, axis, interior) for _, _, ext in items]
    outs = [filled(s, name) for s in shapes]
    got = st.gradient([it + (o,) for it, o in zip(items, outs)], op, axis, spacing, out, interior)
    assert all(g is o for g, o in zip(got, outs))
    if atlas:
        at, views, where = atlas_of([gm.out_shape(ext, op, axis, interior) for _, _, ext in items], name) if op != "vector" else vector_atlas(shapes, name)
        st.gradient([it + (v,) for it, v in zip(items, views)], op, axis, spacing, out, interior)
    torch.cuda.synchronize()
    res = []
    for i, (it, s) in enumerate(zip(items, slices)):
        w = "%s %s axis %d -> %s box %d %s:" % (what, op, axis, name, i, it)
        expect(host(outs[i]), s, op, axis, spacing, it[0], name, interior, w + " contiguous,")
        if atlas:
            expect(host(views[i]), s, op, axis, spacing, it[0], name, interior, w + " atlas,")
        res.append(host(outs[i]).tobytes())
    assert not atlas or untouched(at, where), what + " a byte outside the rectangles was written"
    return res


def vector_atlas(shapes, name):
    """atlas_of for outputs with a trailing dimension of N components: rectangles side by side along x, the components kept together"""
    N = shapes[0][-1]
    dims = [max(s[j] for s in shapes) + 1 for j in range(N - 1)] + [sum(s[N - 1] + 1 for s in shapes)]
    dims[-1] += 1 - dims[-1] % 2
    atlas = filled(dims + [N], name)
    views, slices, x = [], [], 0
    for s in shapes:
        sl = tuple(slice(0, e) for e in s[:N - 1]) + (slice(x, x + s[N - 1]),)
        slices.append(sl)
        views.append(atlas[sl])
        x += s[N - 1] + 1
    return atlas, views, slices


# ---- 1. shapes and opens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shapes_and_opens(shape, dtype, interp):
    kw = (("interpAlgo", interp),)
    items = mixed(shape)
    N = len(shape)
    algo = case(shape, dtype, kw)[3].cmprAlgo
    for name, st, full in opens(shape, dtype, kw):
        fast = name == "open_payload" or algo in INTERP_IDS
        slices = slices_of(full, items)
        with st:
            assert st.stats()["fast"] == (1 if fast else 0)
            n0 = st.stats()["requests"]
            calls = 0
            for op, axis in combos(N):
                for out in OUTS:
                    for spacing in (None, ANISO[:N]):
                        check_gradient(st, items, slices, op, axis, out, spacing, what=name)
                        calls += 2
            assert st.stats()["requests"] == n0 + calls, "a gradient counts as a request"
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
        for op, axis in combos(3):
            for out, spacing in ((None, ANISO[:3]), ("float64", None)):
                check_gradient(st, items, slices, op, axis, out, spacing, what="stock")


def test_a_coarse_box_uses_the_coarse_grid_step():
    """the same region at level 0 and at level 2: the coarse box's derivatives divide by 4 x the spacing"""
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    items = [(0, (8, 4, 16), (33, 29, 65)), (2, (2, 1, 4), (9, 8, 17))]
    slices = slices_of(full, items)
    assert np.array_equal(slices[0][::4, ::4, ::4], slices[1]), "one region"
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for op, axis in combos(3):
            check_gradient(st, items, slices, op, axis, "float64", ANISO[:3], what="two levels")
        got = st.gradient(items, "deriv", 2, 0.25, "float64")
        again = sz3_amd.gradient_points(torch.from_numpy(slices[1]).to(DEV), "deriv", 2, 1.0, "float64")
        torch.cuda.synchronize()
        assert host(got[1]).tobytes() == host(again).tobytes(), "0.25 * 2^2 is the grid step 1.0"
        level0 = gm.gradient(slices[1], "deriv", 2, 0.25, 0, np.float64)
        assert np.array_equal(host(got[1]) * 4.0, level0), "a power of two: exactly a quarter of the level-0 rule's result"


# ---- 2. extents, strides and dimensions, through gradient_points -------------------------------------------------------------------------------
def check_points(src, ref, what="", spacing=None, interior=False, ops=None, outs=OUTS, strided=True):
    """gradient_points of the device view `src` (host values `ref`) into a rectangle of a 0x4D buffer: every op, axis and output type"""
    N = ref.ndim
    calls = []
    for op, axis in (ops or combos(N)):
        if interior and any(ref.shape[j] < 3 for j in gm.differentiated(op, axis, N)):
            continue
        shape = gm.out_shape(ref.shape, op, axis, interior)
        sl = tuple(slice(1, 1 + e) for e in shape)
        for name in outs:
            buf = filled([e + 2 for e in shape] + ([N] if op == "vector" else []), name)
            view = buf[sl] if strided else None
            got = sz3_amd.gradient_points(src, op, axis, spacing, name, interior, out=view)
            assert view is None or got.data_ptr() == view.data_ptr()
            calls.append((op, axis, name, buf, got))
    torch.cuda.synchronize()
    for op, axis, name, buf, got in calls:
        shape = gm.out_shape(ref.shape, op, axis, interior)
        sl = tuple(slice(1, 1 + e) for e in shape)
        assert tuple(got.shape) == full_shape(ref.shape, op, axis, interior)
        expect(host(got), ref, op, axis, spacing, 0, name, interior, "%s %s axis %d -> %s, shape %s:" % (what, op, axis, name, ref.shape))
        assert untouched(buf, [sl] if strided else []), "%s %s: a byte outside the view was written" % (what, op)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_small_extents_along_every_axis(dtype):
    rng = np.random.default_rng(31)
    for e in (1, 2, 3, 4, 5):
        for other in (1, 255, 256, 257):  # with e: 1 .. 5 workgroups' worth of output points
            for shape in ((e, other), (other, e), (e, 3, other), (3, e, other)):
                a = rng.normal(0.0, 1.0, shape).astype(dtype)
                check_points(torch.from_numpy(a).to(DEV), a, "extent %d" % e, ANISO[:len(shape)], outs=(dtype,))
    for total in (1, 255, 256, 257):  # the output points themselves
        a = rng.normal(0.0, 1.0, (total,)).astype(dtype)
        check_points(torch.from_numpy(a).to(DEV), a, "%d points" % total, 0.75)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dimensions_and_strides(dtype):
    rng = np.random.default_rng(41)
    for shape in ((1,), (77,), (9, 70), (3, 5, 67), (3, 4, 5, 66), (1, 9, 1, 70), (9, 1, 70, 1), (1, 1, 40), (40, 1, 1), (1, 3, 37, 1), (5, 37, 1), (1, 1, 1, 1)):
        a = rng.normal(0.0, 1.0, shape).astype(dtype)
        check_points(torch.from_numpy(a).to(DEV), a, "dims", ANISO[:len(shape)])
    a = rng.normal(0.0, 1.0, (6, 7, 140)).astype(dtype)
    src = torch.from_numpy(a).to(DEV)
    views = [("x stride 2", src[:, :, ::2], a[:, :, ::2]),
             ("broadcast rows", src[:, 2:3, :].expand(6, 5, 140), np.broadcast_to(a[:, 2:3, :], (6, 5, 140))),
             ("broadcast x", src[:, :, 9:10].expand(6, 7, 70), np.broadcast_to(a[:, :, 9:10], (6, 7, 70))),
             ("broadcast slowest", src[1:2].expand(9, 7, 140), np.broadcast_to(a[1:2], (9, 7, 140))),
             ("transposed", src.permute(2, 0, 1), a.transpose(2, 0, 1)),
             ("transposed 2", src.transpose(1, 2), a.transpose(0, 2, 1))]
    for what, v, ref in views:
        check_points(v, np.ascontiguousarray(ref), what, (2.0, 0.3, 1.0))
    # allocated outputs, negative axes, the defaults
    out = sz3_amd.gradient_points(src, "deriv", -1)
    vec = sz3_amd.gradient_points(src, "vector", spacing=2.0, out_dtype=torch.float64)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (6, 7, 140) and out.dtype == src.dtype and out.is_contiguous()
    assert tuple(vec.shape) == (6, 7, 140, 3) and vec.dtype == torch.float64 and vec.is_contiguous()
    expect(host(out), a, "deriv", 2, None, 0, dtype)
    expect(host(vec), a, "vector", 0, 2.0, 0, "float64")
    # VECTOR into a strided tensor: every other row of a wider buffer, the components kept together
    wide = filled((6, 14, 141, 3), "float32")
    view = wide[:, ::2, 1:, :]
    sz3_amd.gradient_points(src, "vector", out_dtype="float32", out=view)
    torch.cuda.synchronize()
    expect(host(view), a, "vector", 0, None, 0, "float32", what="a strided vector output:")
    assert untouched(wide, [(slice(None), slice(0, 14, 2), slice(1, 141))])
    # a strided scalar output: x stride 2
    wide = filled((6, 7, 280), "float64")
    sz3_amd.gradient_points(src, "mag2", out_dtype="float64", out=wide[..., ::2])
    torch.cuda.synchronize()
    expect(host(wide[..., ::2]), a, "mag2", 0, None, 0, "float64")
    assert untouched(wide, [(slice(None), slice(None), slice(0, 280, 2))])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_interior(dtype):
    rng = np.random.default_rng(43)
    for shape in ((3,), (4,), (66,), (3, 3), (3, 66), (66, 4), (3, 3, 3), (4, 3, 66), (66, 4, 3), (5, 1, 66), (1, 4, 1, 66), (3, 4, 3, 5)):
        a = rng.normal(0.0, 1.0, shape).astype(dtype)
        check_points(torch.from_numpy(a).to(DEV), a, "interior", ANISO[:len(shape)], interior=True)
    one = sz3_amd.gradient_points(torch.from_numpy(np.arange(27.0).reshape(3, 3, 3)).to(DEV), "vector", interior=True)
    torch.cuda.synchronize()
    assert tuple(one.shape) == (1, 1, 1, 3) and host(one).reshape(-1).tolist() == [9.0, 3.0, 1.0], "extent 3: one output point, a central difference"
    # a tile with a halo of one point: the interior of the haloed box is the whole array's gradient at the tile's points — seamless
    a = rng.normal(0.0, 1.0, (20, 22, 70)).astype(dtype)
    src = torch.from_numpy(a).to(DEV)
    whole = sz3_amd.gradient_points(src, "vector")
    tile = sz3_amd.gradient_points(src[3:13, 0:9, 30:70], "vector", interior=True)
    torch.cuda.synchronize()
    assert host(tile).tobytes() == host(whole[4:12, 1:8, 31:69]).tobytes()


# ---- 3. crafted arrays -----------------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_reach_their_neighbours_alone():
    for dtype in ("float32", "float64"):
        a = np.random.default_rng(47).normal(0.0, 1.0, (9, 10, 11)).astype(dtype)
        a[4, 5, 6] = np.nan
        a[1, 2, 3] = np.inf
        a[7, 7, 2] = -np.inf
        src = torch.from_numpy(a).to(DEV)
        check_points(src, a, "non-finite")
        got = host(sz3_amd.gradient_points(src, "vector", out_dtype="float64"))
        finite = np.isfinite(got)
        touched = np.zeros(a.shape, bool)
        for p in ((4, 5, 6), (1, 2, 3), (7, 7, 2)):
            for j in range(3):
                for d in (-1, 1):
                    q = list(p)
                    q[j] += d
                    touched[tuple(q)] = True
                    assert not finite[tuple(q) + (j,)], "the neighbour along axis %d of %s" % (j, p)
        assert finite[~touched].all(), "nobody else"
        assert finite[4, 5, 6].all(), "the centre is not read"
        # Inf - Inf: two infinite neighbours
        b = np.ones((5,), dtype)
        b[1] = b[3] = np.inf
        got = host(sz3_amd.gradient_points(torch.from_numpy(b).to(DEV), "deriv"))
        assert np.isnan(got[2]) and np.isinf(got[0]) and np.isinf(got[4])


def test_overflow_denormals_ramp_and_negative_zero():
    # spikes of 1e30 in f32: the squares overflow f32, not the double arithmetic
    a = np.zeros((6, 7, 8), np.float32)
    a[2, 3, 4] = 1e30
    a[3, 3, 4] = -1e30
    src = torch.from_numpy(a).to(DEV)
    check_points(src, a, "spikes")
    m2 = host(sz3_amd.gradient_points(src, "mag2"))
    assert np.isinf(m2).any() and np.isfinite(host(sz3_amd.gradient_points(src, "mag2", out_dtype="float64"))).all()
    assert np.isfinite(host(sz3_amd.gradient_points(src, "mag"))).all(), "the root is taken in double"
    # differences of 1e308 in f64 into f32: Inf by the cast; 2e308 overflows the subtraction itself
    b = np.zeros((9,), np.float64)
    b[2], b[5], b[7] = 1e308, 1e308, -1e308
    srcb = torch.from_numpy(b).to(DEV)
    check_points(srcb, b, "1e308")
    d32, d64 = host(sz3_amd.gradient_points(srcb, "deriv", out_dtype="float32")), host(sz3_amd.gradient_points(srcb, "deriv"))
    assert np.isinf(d32[1]) and np.isfinite(d64[1]) and np.isinf(d64[6]), "Inf by the cast / by the subtraction"
    check_points(srcb, b, "1e308 over a tiny step", 1e-300)
    # denormal differences
    for dtype, tiny in (("float32", 1e-45), ("float64", 5e-324)):
        c = (np.arange(40, dtype=np.float64).reshape(5, 8) % 3 * tiny).astype(dtype)
        assert (c != 0).any()
        check_points(torch.from_numpy(c).to(DEV), c, "denormal")
        check_points(torch.from_numpy(c).to(DEV), c, "denormal over a large step", (4.0, 1e10))
    # a linear ramp with a spacing such that every derivative is exactly 1.0
    r = (np.arange(6)[:, None, None] * 0.5 + np.arange(7)[None, :, None] * 1.25 + np.arange(70)[None, None, :] * 3.0).astype(np.float64)
    srcr = torch.from_numpy(r).to(DEV)
    vec = host(sz3_amd.gradient_points(srcr, "vector", spacing=(0.5, 1.25, 3.0)))
    assert (vec == 1.0).all() and (host(sz3_amd.gradient_points(srcr, "mag2", spacing=(0.5, 1.25, 3.0), out_dtype="float32")) == 3.0).all()
    check_points(srcr, r, "ramp", (0.5, 1.25, 3.0))
    # -0.0 inputs: x - x is +0.0 whatever the sign, and (-0.0) - (+0.0) is -0.0
    z = np.zeros((4, 7), np.float32)
    z[:, ::2] = -0.0
    check_points(torch.from_numpy(z).to(DEV), z, "-0.0")
    got = host(sz3_amd.gradient_points(torch.from_numpy(z).to(DEV), "deriv", 1))
    assert np.signbit(got[:, 6]).all() and not np.signbit(got[:, :6]).any() and (got == 0.0).all()


# ---- 4. against the project itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_against_request_and_gradient_points(dtype):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, dtype)
    items = mixed(shape)
    with sz3_amd.open_stream(blob, np.dtype(dtype), device=DEV) as st:
        delivered = ask(st, items)
        for interior in (False, True):
            for op, axis in combos(3):
                sub = [i for i, it in enumerate(items) if not interior or all(it[2][j] >= 3 for j in gm.differentiated(op, axis, 3))]
                for out in OUTS:
                    got = st.gradient([items[i] for i in sub], op, axis, ANISO[:3], out, interior)
                    torch.cuda.synchronize()
                    for g, i in zip(got, sub):
                        pre = tuple(s * 2.0 ** items[i][0] for s in ANISO[:3])
                        p = sz3_amd.gradient_points(delivered[i], op, axis, pre, out, interior)
                        torch.cuda.synchronize()
                        assert tuple(g.shape) == full_shape(items[i][2], op, axis, interior) == tuple(p.shape) and g.dtype == p.dtype
                        assert host(g).tobytes() == host(p).tobytes(), "%s axis %d box %d: Stream.gradient and gradient_points over the request's tensor differ" % (op, axis, i)


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
        for op, axis, out in (("vector", 0, None), ("deriv", 0, "float64"), ("mag", 0, None)):
            alone = check_gradient(st, [target], tslice, op, axis, out, ANISO[:3])[0]
            for place, others in [(0, many[:2]), (2, many[:2]), (27, many[:27]), (255, many)]:
                items = list(others[:place]) + [target] + list(others[place:])
                got = st.gradient(items, op, axis, ANISO[:3], out)
                torch.cuda.synchronize()
                assert host(got[place]).tobytes() == alone, "%s: %d boxes, place %d" % (op, len(items), place)
            chain(2048)
            got = st.gradient([target], op, axis, ANISO[:3], out)
            torch.cuda.synchronize()
            assert st.stats()["chain_levels_last_request"] > 0 and host(got[0]).tobytes() == alone, "the chain at 2048"
            chain(0)
            with sz3_amd.debug_flags2(int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                items = many[:27] + [target]
                got = st.gradient(items, op, axis, ANISO[:3], out)
                torch.cuda.synchronize()
                assert host(got[27]).tobytes() == alone, "level group by level group"
                mi = mixed(shape)
                check_gradient(st, mi, slices_of(full, mi), op, axis, out, ANISO[:3], what="by level")


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
                for op, axis in (("deriv", 2), ("mag", 0), ("vector", 0)):
                    r = launches(lambda: st.gradient(items, op, axis))
                    s = st.stats()
                    assert r == q and s["chain_levels_last_request"] == cq and s["chain_points"] == points, "a gradient issues the request's launches (%d, %d; threshold %d)" % (r, q, points)
            assert points == 0 or st.stats()["chain_levels_last_request"] > 0, "one level at threshold 2048 takes the chain"
            items = mixed(shape)
            with sz3_amd.debug_flags2(int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                q = launches(lambda: ask(st, items))
                assert launches(lambda: st.gradient(items, "mag2")) == q and launches(lambda: st.gradient(items, "deriv", 0)) == q
        torch.cuda.synchronize()


def check_fallback(st, full, name):
    assert st.stats()["fast"] == 0
    slices = slices_of(full, FB_ITEMS)
    for op, axis in combos(3):
        for out, spacing in ((None, ANISO[:3]), ("float64", None)):
            check_gradient(st, FB_ITEMS, slices, op, axis, out, spacing, what=name)
            s = st.stats()
            assert s["fast"] == 0 and s["launches_last_request"] == 1 and s["chain_levels_last_request"] == 0
    # a view with an x stride of 2 among contiguous outputs
    outs = [filled(ext, "float32") for _, _, ext in FB_ITEMS]
    wide = filled((20, 9, 60), "float32")
    outs[1] = wide[..., ::2]
    st.gradient([it + (o,) for it, o in zip(FB_ITEMS, outs)], "mag2", 0, 2.0)
    torch.cuda.synchronize()
    for o, s, it in zip(outs, slices, FB_ITEMS):
        expect(host(o), s, "mag2", 0, 2.0, it[0], "float32", what=name)
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
    big = [it for it in good if min(it[2]) >= 3]

    def refused(fragment, op="deriv", axis=0, out_type=0, flags=0, spacing=(1.0,) * 4, edit=None, null_opts=False, good=good):
        n = len(good)
        arr, shapes = sz3_amd._boxes(N, [it[1:] for it in good])
        name = OUTS[min(out_type, 1)]
        o = sz3_amd._CGradientOpts()
        o.op, o.axis, o.out_type, o.flags = OPS.index(op) if isinstance(op, str) else op, axis, out_type, flags
        o.spacing[:] = spacing
        plain = sz3_amd._CGradientOpts()  # (the outputs' shapes: the boxes', with N components for VECTOR)
        plain.op = o.op if o.op <= 3 else 0
        outs = [filled(tuple(s) + ((N,) if plain.op == 3 else ()), name) for s in shapes]
        reqs, _ = sz3_amd._gradient_reqs(N, [it + (t,) for it, t in zip(good, outs)], shapes, arr, name, plain, st.device, True)
        if edit:
            edit(reqs, o)
        rc = L.sz3hip_stream_gradient(st._h, reqs, n, None if null_opts else C.byref(o), sz3_amd._stream_handle(st.device, None))
        msg = L.sz3hip_last_error().decode()
        assert rc == einval and fragment in msg, (rc, msg, fragment)
        torch.cuda.synchronize()
        assert all((t.view(torch.uint8) == FILL).all() for t in outs), "a refused call wrote (%s)" % fragment
        # the handle serves the next request with the full decode's bytes
        same(ask(st, good[:3]), full, good[:3], "after a refusal (%s)" % fragment)

    refused("NULL argument (opts)", null_opts=True)
    refused("op (4)", op=4)
    refused("op (4294967295)", op=0xFFFFFFFF)
    refused("axis (%d)" % N, axis=N)
    refused("axis (4294967295)", axis=0xFFFFFFFF)
    for op in ("mag2", "mag", "vector"):
        refused("axis is 1", op=op, axis=1)
    refused("out_type (2)", out_type=2)
    refused("flags (0x2)", flags=2)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("spacing[%d]" % (N - 1), spacing=(1.0,) * (N - 1) + (bad,) + (1.0,) * (4 - N))
    for b in (0, n // 2, n - 1):  # a box's: at the first, a middle and the last box
        k, _, ext = good[b]
        if k:
            def finest_but(reqs, o, b=b):  # (a box of a coarser grid lies inside the finer one)
                for i in range(n):
                    if i != b:
                        reqs[i].level = 0
            refused("box %d: the grid step of dimension 0" % b, spacing=(1.7e308, 1.0, 1.0, 1.0), edit=finest_but)

        def misalign4(reqs, o, b=b):
            reqs[b].d_out = reqs[b].d_out + 2
        refused("box %d: the output is not aligned to its element size (4 bytes)" % b, edit=misalign4)
        refused("box %d: the output is not aligned to its element size (4 bytes)" % b, op="vector", edit=misalign4)

        def misalign8(reqs, o, b=b):
            reqs[b].d_out = reqs[b].d_out + 4
        refused("box %d: the output is not aligned to its element size (8 bytes)" % b, out_type=1, edit=misalign8)

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
        if ext[N - 1] > 1:
            refused("box %d: the view's stride of dimension %d is negative" % (b, N - 1), edit=negative)
        if b:
            def overlap(reqs, o, b=b):
                reqs[b].d_out = reqs[0].d_out
            refused("box %d: the output overlaps box 0's" % b, edit=overlap)
            refused("box %d: the output overlaps box 0's" % b, op="vector", out_type=1, edit=overlap)
    assert len(big) >= 3
    for b in (0, len(big) // 2, len(big) - 1):  # INTERIOR: boxes of at least 3 points along every axis, one cut to 2 along the last
        def two(reqs, o, b=b):
            reqs[b].box.ext[N - 1] = 2
        for op, axis in (("mag", 0), ("vector", 0), ("deriv", N - 1)):
            refused("box %d: the extent of dimension %d is 2" % (b, N - 1), op=op, axis=axis, flags=1, edit=two, good=big)
    assert st.stats()["requests"] > before


def test_refusals():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    good = mixed(shape)[:9]
    assert all(it[0] for it in (good[0], good[4], good[8]))
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        refusals(st, full, good)


def test_refusals_on_a_fallback_handle():
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **dict(FALLBACKS[0][1])))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 0
        refusals(st, full, FB_ITEMS[:6])


def test_refusals_of_gradient_points():
    a = torch.zeros((4, 6), dtype=torch.float32, device=DEV)
    buf = filled((4, 8), "float32")
    with pytest.raises(ValueError):
        sz3_amd.gradient_points(a, "deriv", 2)
    with pytest.raises(ValueError):
        sz3_amd.gradient_points(a, "mag", 1)
    with pytest.raises(ValueError):
        sz3_amd.gradient_points(a, "deriv", 1, out=buf[:, :5])
    with pytest.raises(ValueError):
        sz3_amd.gradient_points(a, "deriv", 1, out_dtype="float64", out=buf[:, :6])
    with pytest.raises(ValueError):
        sz3_amd.gradient_points(a.cpu(), "deriv", 1)
    with pytest.raises(ValueError):
        sz3_amd.gradient_points(a, "deriv", 1, spacing=(1.0, 2.0, 3.0))
    with pytest.raises(sz3_amd.SZ3HipError, match=r"spacing\[1\]"):
        sz3_amd.gradient_points(a, "deriv", 1, spacing=(1.0, 0.0), out=buf[:, :6])
    with pytest.raises(ValueError, match="dimension 0 is 2"):
        sz3_amd.gradient_points(a[:2], "mag", interior=True)
    with pytest.raises(sz3_amd.SZ3HipError, match="the extent of dimension 0 is 2"):  # (the library's own refusal: the C call)
        o2 = sz3_amd._CGradientOpts()
        o2.op, o2.flags = sz3_amd.GRADIENT_MAG, sz3_amd.GRADIENT_INTERIOR
        o2.spacing[:] = (1.0,) * 4
        sz3_amd._check(L.sz3hip_gradient_device(0, 2, (C.c_uint64 * 2)(2, 6), a.data_ptr(), None, C.byref(o2), buf.data_ptr(), None, None))
    with pytest.raises(sz3_amd.SZ3HipError, match="permuted or overlap"):
        sz3_amd.gradient_points(torch.zeros((4, 5, 6), dtype=torch.float32, device=DEV), "mag", out=filled((6, 5, 4), "float32").permute(2, 1, 0))
    # a VECTOR output: the components contiguous, the other strides divisible by their count — said in the error
    v = filled((4, 6, 4), "float32")
    with pytest.raises(ValueError, match="must be contiguous"):
        sz3_amd.gradient_points(a, "vector", out=v[:, :, ::2])
    with pytest.raises(ValueError, match="divisible by the component count 2"):
        sz3_amd.gradient_points(a, "vector", out=torch.as_strided(filled((200,), "float32"), (4, 6, 2), (21, 3, 1)))
    o = sz3_amd._CGradientOpts()  # (torch makes no misaligned float64 view: the C call, an f64 output 4 bytes off)
    o.op, o.axis, o.out_type = sz3_amd.GRADIENT_DERIV, 1, 1
    o.spacing[:] = (1.0,) * 4
    dims, strides = (C.c_uint64 * 2)(4, 3), (C.c_int64 * 2)(6, 1)
    rc = L.sz3hip_gradient_device(0, 2, dims, a.data_ptr(), strides, C.byref(o), buf.data_ptr() + 4, None, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and "not aligned to its element size (8 bytes)" in L.sz3hip_last_error().decode()
    torch.cuda.synchronize()
    assert (buf.view(torch.uint8) == FILL).all() and (v.view(torch.uint8) == FILL).all()


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
        want_x = check_gradient(st, x_items, slices_of(full, x_items), "vector", 0, None, ANISO[:3])
        want_y = check_gradient(st, y_items, slices_of(full, y_items), "deriv", 2, "float64", None)
        want_red = st.reduce(x_items, 7, -0.5, 0.75).stats.cpu().numpy().tobytes()
        sel = st.select(y_items, lo, hi, 64)
        want_sel = [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()]
        want_map = [m.cpu().numpy().tobytes() for m in st.map(x_items, "u8", lo=lo, hi=hi)]
        want_smp = [t.cpu().numpy().tobytes() for t in st.sample(x_items, qx, "linear")]
        want_prj = [t.cpu().numpy().tobytes() for t in st.project(y_items, "sum", 1)]
        torch.cuda.synchronize()
        for _ in range(2):  # no host synchronisation in between
            gx0 = st.gradient(x_items, "vector", 0, ANISO[:3])
            x = ask(st, x_items, sync=False, stream=s1)
            gy0 = st.gradient(y_items, "deriv", 2, out_dtype="float64", stream=s2)
            red = st.reduce(x_items, 7, -0.5, 0.75, stream=s1)
            gx1 = st.gradient(x_items, "vector", 0, ANISO[:3], stream=s2)
            sel = st.select(y_items, lo, hi, 64)
            mp = st.map(x_items, "u8", lo=lo, hi=hi, stream=s1)
            gy1 = st.gradient(y_items, "deriv", 2, out_dtype="float64", stream=s1)
            smp = st.sample(x_items, qx, "linear", stream=s2)
            prj = st.project(y_items, "sum", 1, stream=s1)
            y = ask(st, y_items, sync=False, stream=s2)
            torch.cuda.synchronize()
            for outs in (gx0, gx1):
                assert [host(o).tobytes() for o in outs] == want_x
            for outs in (gy0, gy1):
                assert [host(o).tobytes() for o in outs] == want_y
            assert red.stats.cpu().numpy().tobytes() == want_red
            assert [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()] == want_sel
            assert [m.cpu().numpy().tobytes() for m in mp] == want_map
            assert [t.cpu().numpy().tobytes() for t in smp] == want_smp
            assert [t.cpu().numpy().tobytes() for t in prj] == want_prj
            same(x, full, x_items)
            same(y, full, y_items)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_mag_against_numpys_root(dtype, capsys):
    """a field of 48^3 normal values: MAG within one unit in the last place of sqrt(MAG2), the results that differ at all counted and printed"""
    a = np.random.default_rng(53).normal(0.0, 1.0, (48, 48, 48)).astype(dtype)
    src = torch.from_numpy(a).to(DEV)
    for name in OUTS:
        got = host(sz3_amd.gradient_points(src, "mag", 0, ANISO[:3], name))
        with np.errstate(all="ignore"):
            want = np.sqrt(gm.gradient(a, "mag", 0, ANISO[:3], 0, name, sqrt=False)).astype(name)
        differ, worst = gm.ulp_apart(got, want)
        with capsys.disabled():
            print("\nMAG %s -> %s: %d of %d results differ from sqrt(MAG2), at most %d ulp" % (dtype, name, differ, got.size, worst))
        assert worst <= 1

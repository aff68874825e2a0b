"""Boxes sampled at fractional positions, on the MI355X: Stream.sample, sample_points.

Expected values come from numpy float64 alone, over the full decode's [::2**k] slice of the box, with the header's rule written in numpy
(np_sample). Equality is in BYTES for outputs that are no NaN and by isnan otherwise. Every output lives in a buffer filled with 0x4D: the
bytes beyond n_points, and all bytes of a refused call, must still be 0x4D afterwards."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, conf_for, container, smooth  # noqa: E402
from sink_models import NAN, RAW, np_lattice, np_sample, same_values  # noqa: E402,F401
from test_gpu_request import FB_ITEMS, ask, chain, mixed, same  # noqa: E402,F401
from test_gpu_stream import SHAPES, IDS, case, coarse_shape, coarse_view, opens, tile_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
FILL = 0x4D
PAD = 5  # elements behind every output that must stay 0x4D
MODES = ["nearest", "linear"]
SIZES = (1, 255, 256, 257, 3 * 256 + 1)


# ---- the rule, in numpy ----------------------------------------------------------------------------------------------------------------------
# ---- buffers and calls -----------------------------------------------------------------------------------------------------------------------
def filled(n, tdtype):
    """n elements of the torch type, every byte 0x4D"""
    return torch.full((n * torch.empty((), dtype=tdtype).element_size(),), FILL, dtype=torch.uint8, device=DEV).view(tdtype)


def taken(buf, n, what=""):
    """the first n elements on the host; the PAD elements behind them still hold 0x4D"""
    a = buf.cpu().numpy()
    assert a.size == n + PAD and (a[n:].view(np.uint8) == FILL).all(), what + " a byte beyond n_points was written"
    return a[:n]


def dev(coords):
    return torch.from_numpy(np.ascontiguousarray(coords)).to(DEV)


def as_query(q):
    """a numpy coordinate array goes to the device; a lattice stays"""
    return dev(q) if isinstance(q, np.ndarray) else q


def coords_of(q):
    return q if isinstance(q, np.ndarray) else np_lattice(*q)


def stream_sample(st, items, queries, mode, clamp=False, fill=NAN, stream=None):
    """sz3hip_stream_sample into 0x4D-filled buffers with PAD elements of room behind: the buffers and the query counts (not synchronised)"""
    held = [as_query(q) for q in queries]
    reqs, n, cname, _ = sz3_amd._sample_reqs(st.conf.N, items, held)
    td = getattr(torch, st.dtype.name)
    counts = [int(reqs[i].n_points) for i in range(n)]
    bufs = [filled(c + PAD, td) for c in counts]
    for i, b in enumerate(bufs):
        reqs[i].d_out = b.data_ptr()
    opts = sz3_amd._sample_opts(mode, clamp, fill, cname)
    rc = L.sz3hip_stream_sample(st._h, reqs, n, C.byref(opts), sz3_amd._stream_handle(st.device, stream))
    assert rc == 0, L.sz3hip_last_error().decode()
    return bufs, counts, held


def points(t, q, mode, clamp=False, fill=NAN):
    """sz3hip_sample_device over the tensor's own view into a 0x4D-filled buffer: the results on the host"""
    N = t.dim()
    held = as_query(q)
    req = sz3_amd._CSampleReq()
    cname, _ = sz3_amd._sample_query(held, N, 0, req)
    n = int(req.n_points)
    buf = filled(n + PAD, t.dtype)
    req.d_out = buf.data_ptr()
    opts = sz3_amd._sample_opts(mode, clamp, fill, cname or "float64")
    rc = L.sz3hip_sample_device(0 if t.dtype == torch.float32 else 1, N, (C.c_uint64 * N)(*[int(d) for d in t.shape]), t.data_ptr(),
                                (C.c_int64 * N)(*[int(v) for v in t.stride()]), C.byref(opts), C.byref(req), sz3_amd._stream_handle(t.device, None))
    assert rc == 0, L.sz3hip_last_error().decode()
    torch.cuda.synchronize()
    return taken(buf, n)


def check_points(a, q, what="", t=None, modes=MODES, fills=(NAN, -7.25)):
    """sample_points' launch over the array, both filters, with and without the clamp, against numpy"""
    t = torch.from_numpy(a).to(DEV) if t is None else t
    for mode in modes:
        for clamp, fill in zip((False, True), fills):
            got = points(t, q, mode, clamp, fill)
            same_values(got, np_sample(a, coords_of(q), mode, clamp, fill), "%s %s clamp %d:" % (what, mode, clamp))


def slices_of(full, items):
    return [coarse_view(full, k)[box_slices(lo, ext)].cpu().numpy() for k, lo, ext in items]


# ---- the queries of a box --------------------------------------------------------------------------------------------------------------------
def grid_points(ext):
    return np.stack([g.reshape(-1) for g in np.meshgrid(*[np.arange(e, dtype=np.float64) for e in ext], indexing="ij")], axis=1)


def cell_centres(ext):
    """the centre of every cell; a dimension of extent 1 has the one coordinate 0"""
    return np.stack([g.reshape(-1) for g in np.meshgrid(*[np.arange(max(e - 1, 1), dtype=np.float64) + (0.5 if e > 1 else 0.0) for e in ext], indexing="ij")], axis=1)


def uniform(ext, n, seed, margin=0.0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-margin, e - 1 + margin, n) for e in ext], axis=1)


def oblique(ext, counts=(3, 17, 23)):
    """a lattice that starts outside the box, runs obliquely through it and leaves it through other faces"""
    N = len(ext)
    steps = [[(e + 1.5) / c * (1.0 if j % 3 == a else 0.37) for j, e in enumerate(ext)] for a, c in enumerate(counts)]
    return ([-0.75] * N, steps, counts)


def queries_for(items, shift=0):
    """one kind of queries per box, the kinds going round: every grid point, all cell centres, seeded uniform points (some outside), an
    oblique lattice crossing the box's faces, and uniform points in the counts around a workgroup"""
    qs = []
    for i, (_, _, ext) in enumerate(items):
        kind = (i + shift) % 5
        if kind == 0:
            qs.append(grid_points(ext))
        elif kind == 1:
            qs.append(cell_centres(ext))
        elif kind == 2:
            qs.append(uniform(ext, 1000, i, margin=0.5))
        elif kind == 3:
            qs.append(oblique(ext))
        else:
            qs.append(uniform(ext, SIZES[(i // 5) % len(SIZES)], i))
    return qs


def check_stream(st, full, items, queries, mode, clamp=False, fill=NAN, what="", slices=None):
    """one sz3hip_stream_sample against numpy; returns the results' bytes per box"""
    slices = slices_of(full, items) if slices is None else slices
    bufs, counts, _ = stream_sample(st, items, queries, mode, clamp, fill)
    torch.cuda.synchronize()
    res = []
    for i, (it, s, q) in enumerate(zip(items, slices, queries)):
        w = "%s %s clamp %d box %d %s:" % (what, mode, clamp, i, it)
        got = taken(bufs[i], counts[i], w)
        same_values(got, np_sample(s, coords_of(q), mode, clamp, fill), w)
        res.append(got.tobytes())
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
            for shift, mode in enumerate(MODES):
                for clamp, fill in ((False, NAN), (True, 3.5)):
                    qs = queries_for(items, shift + 2 * clamp)
                    check_stream(st, full, items, qs, mode, clamp, fill, name, slices)
                    calls += 1
                # every grid point: NEAREST is the request's bytes, LINEAR its values
                grids = [grid_points(it[2]) for it in items[:8]]
                got = check_stream(st, full, items[:8], grids, mode, what=name + " grid", slices=slices[:8])
                assert got == [np.ascontiguousarray(s).tobytes() for s in slices[:8]], "%s %s at the grid points is not the request's bytes" % (name, mode)
                # f32 coordinates: the f64 call on coords.astype(float64)
                q32 = [uniform(it[2], 700, 40 + i, margin=0.25).astype(np.float32) for i, it in enumerate(items)]
                a = check_stream(st, full, items, q32, mode, what=name + " f32 coordinates", slices=slices)
                b = check_stream(st, full, items, [q.astype(np.float64) for q in q32], mode, what=name + " f64 of f32", slices=slices)
                assert a == b
                calls += 3
            assert st.stats()["requests"] == n0 + calls, "a sample counts as a request"
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
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 1
        for shift, mode in enumerate(MODES):
            check_stream(st, full, items, queries_for(items, shift), mode, bool(shift), 0.0, "stock")


# ---- 2. crafted coordinates, through sample_points ---------------------------------------------------------------------------------------------
def crafted_coordinates(ext):
    e1 = float(ext - 1)
    v = []
    for x in (0.0, -0.0, e1):
        v += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    v += [k + 0.5 for k in range(ext)] + [np.nextafter(k + 0.5, -np.inf) for k in range(ext)] + [np.nextafter(k + 0.5, np.inf) for k in range(ext)]
    v += [0.49999999999999994, 1.4999999999999998, e1 - 0.5, e1 + 0.5, -0.5, -0.49999999999999994, 5e-324, -5e-324, 1e-300, e1 - 1e-13, e1 + 1e-9, 1e300, -1e300,
          np.nan, np.inf, -np.inf, 1.0, 2.0, 1.25, 1.75, 1.0 / 3.0]
    return np.array(v, dtype=np.float64)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_crafted_coordinates(dtype):
    rng = np.random.default_rng(31)
    ext = 9
    x = crafted_coordinates(ext)
    assert np.floor(np.float64(0.49999999999999994) + 0.5) == 1.0, "the tie the rule defines: c + 0.5 rounds up to 1"
    a1 = rng.normal(0.0, 1.0, ext).astype(dtype)
    with np.errstate(over="ignore"):
        forms = [("f64", x), ("f32", x.astype(np.float32))]
    for cname, c in forms:
        check_points(a1, c.reshape(-1, 1), "1-D %s" % cname)
        # 3-D: the crafted coordinate along one dimension, the others inside
        a3 = rng.normal(0.0, 1.0, (4, ext, 5)).astype(dtype)
        for j, e in ((1, ext),):
            q = np.full((c.size, 3), 1.25, dtype=c.dtype)
            q[:, j] = c
            check_points(a3, q, "3-D %s dimension %d" % (cname, j))
        a3 = rng.normal(0.0, 1.0, (ext, 3, 4)).astype(dtype)
        q = np.full((c.size, 3), 2.0, dtype=c.dtype)
        q[:, 0] = c
        check_points(a3, q, "3-D %s dimension 0" % cname)
        a3 = rng.normal(0.0, 1.0, (3, 4, ext)).astype(dtype)
        q = np.full((c.size, 3), 0.5, dtype=c.dtype)
        q[:, 2] = c
        check_points(a3, q, "3-D %s dimension 2" % cname)
    # what the rule says about the ends, spelled out: -0.0 is inside, one step outside is not, NaN is never answered
    t = torch.from_numpy(a1).to(DEV)
    got = points(t, np.array([[-0.0], [np.nextafter(0.0, -1.0)], [ext - 1.0], [np.nextafter(ext - 1.0, np.inf)], [np.nan]]), "linear", False, -1.0)
    assert got.tolist() == [a1[0], -1.0, a1[-1], -1.0, -1.0]
    got = points(t, np.array([[-np.inf], [np.inf], [np.nan], [-3.0], [1e9]]), "nearest", True, -1.0)
    assert got.tolist() == [a1[0], a1[-1], -1.0, a1[0], a1[-1]]
    got = points(t, np.array([[0.5], [1.5], [0.49999999999999994], [7.5]]), "nearest")
    assert got.tolist() == [a1[1], a1[2], a1[1], a1[8]]


# ---- 3. crafted values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_crafted_values(dtype):
    tiny = np.finfo(dtype).tiny
    sub = np.nextafter(np.zeros((), dtype), np.ones((), dtype))  # the smallest denormal
    row = np.array([1.0, np.inf, 2.0, np.nan, 3.0, -np.inf, 4.0, sub, 3 * sub, tiny / 2, -sub, 0.0, -0.0, np.finfo(dtype).max, np.finfo(dtype).max, 5.0], dtype=dtype)
    c = np.concatenate([np.arange(row.size, dtype=np.float64), np.arange(row.size - 1) + 0.5, np.arange(row.size - 1) + 0.25, np.arange(row.size - 1) + 2.0 ** -40])
    check_points(row, c.reshape(-1, 1), "1-D")
    t = torch.from_numpy(row).to(DEV)
    got = points(t, np.arange(row.size, dtype=np.float64).reshape(-1, 1), "linear")
    assert got.tobytes() == row.tobytes() or (np.isnan(got[3]) and np.delete(got, 3).tobytes() == np.delete(row, 3).tobytes()), "a grid point next to Inf / NaN is the point"
    got = points(t, np.array([[0.5], [2.5], [1.0], [5.5]]), "linear")
    assert got[0] == np.inf and np.isnan(got[1]) and got[2] == np.inf and got[3] == -np.inf
    # 2-D: the same row among ordinary rows, grid points and points between along either dimension
    a = np.random.default_rng(7).normal(0.0, 1.0, (3, row.size)).astype(dtype)
    a[1] = row
    q = np.concatenate([grid_points(a.shape), cell_centres(a.shape), np.stack([np.full(c.size, 1.0), c], axis=1), np.stack([np.full(c.size, 0.5), c], axis=1)])
    check_points(a, q, "2-D")
    # NaN payloads under NEAREST
    u = RAW[np.dtype(dtype)]
    bits = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001], dtype=np.uint64)
    if dtype == "float64":
        bits = np.array([0x7FF8000000000001, 0xFFF8123456789ABC, 0x7FF0000000000001, 0x8000000000000000, 1], dtype=np.uint64)
    vals = bits.astype(u).view(dtype)
    got = points(torch.from_numpy(vals.copy()).to(DEV), np.array([[0.0], [1.2], [1.6], [3.0], [3.5], [0.4]]), "nearest")
    assert got.view(u).tolist() == [int(bits[i]) for i in (0, 1, 2, 3, 4, 0)]


# ---- 4. geometries, through sample_points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_geometries(dtype):
    rng = np.random.default_rng(29)

    def queries(ext, seed):
        return [np.concatenate([grid_points(ext), cell_centres(ext), uniform(ext, 600, seed, margin=0.4)]), oblique(ext, (2, 9, 31))]

    for shape in ((257,), (19, 23), (5, 131), (3, 4, 5, 7), (6, 1, 9), (1, 1, 1), (1, 7), (4, 1, 1, 3)):
        a = rng.normal(0.0, 1.0, shape).astype(dtype)
        for q in queries(shape, len(shape)):
            check_points(a, q, "shape %s" % (shape,))
    for n in SIZES:  # the query counts around a workgroup
        a = rng.normal(0.0, 1.0, (7, 11, 13)).astype(dtype)
        check_points(a, uniform(a.shape, n, n), "n_points %d" % n, modes=["linear"])
    a = rng.normal(0.0, 1.0, (5, 131)).astype(dtype)
    src = torch.from_numpy(a).to(DEV)
    # x stride 2 and stride-0 broadcasts in the input; a transposed view
    for view, ref in ((src[:, ::2], a[:, ::2]), (src[2:3, :].expand(4, 131), np.broadcast_to(a[2:3, :], (4, 131))), (src[:, 5:6].expand(5, 9), np.broadcast_to(a[:, 5:6], (5, 9))),
                      (src.t(), a.T), (src[1:4, 3:100:3], a[1:4, 3:100:3])):
        ref = np.ascontiguousarray(ref)
        for q in queries(ref.shape, 3):
            check_points(ref, q, "input strides %s" % (tuple(view.stride()),), t=view)
    # the Python call: the same bytes, the lattice's shape
    q = uniform(a.shape, 333, 1)
    for mode in MODES:
        out = sz3_amd.sample_points(src, dev(q), mode=mode, clamp=True, fill=0.0)
        torch.cuda.synchronize()
        same_values(out.cpu().numpy(), np_sample(a, q, mode, True, 0.0), "sample_points %s" % mode)
    lat = ([0.25, -2.0], [[0.5, 0.0], [0.0, 1.5]], (9, 90))
    out = sz3_amd.sample_points(src, lat)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (9, 90)
    same_values(out.cpu().numpy().reshape(-1), np_sample(a, np_lattice(*lat), "linear"), "sample_points lattice")


# ---- 5. against the project itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_against_request_and_sample_points(dtype):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape, dtype)
    items = mixed(shape)
    with sz3_amd.open_stream(blob, np.dtype(dtype), device=DEV) as st:
        delivered = ask(st, items)
        for shift, mode in enumerate(MODES):
            for clamp in (False, True):
                qs = [as_query(q) for q in queries_for(items, shift)]
                got = st.sample(items, qs, mode=mode, clamp=clamp, fill=1.5)
                torch.cuda.synchronize()
                for i, (g, d, q) in enumerate(zip(got, delivered, qs)):
                    p = sz3_amd.sample_points(d, q, mode=mode, clamp=clamp, fill=1.5)
                    torch.cuda.synchronize()
                    assert tuple(g.shape) == tuple(p.shape) and g.dtype == d.dtype
                    assert g.cpu().numpy().tobytes() == p.cpu().numpy().tobytes(), "%s box %d: Stream.sample and sample_points over the request's tensor differ" % (mode, i)
                    same_values(g.cpu().numpy().reshape(-1), np_sample(d.cpu().numpy(), coords_of(queries_for(items, shift)[i]), mode, clamp, 1.5), "Stream.sample box %d" % i)


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
    many_q = [uniform(it[2], 1 + i % 40, i, margin=0.3) for i, it in enumerate(many)]
    target = (1, (3, 2, 7), (21, 19, 33))
    tq = np.concatenate([uniform(target[2], 2000, 99, margin=0.2), cell_centres(target[2])])
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        chain(0)
        for mode in MODES:
            alone = check_stream(st, full, [target], [tq], mode)[0]
            for place, others in [(0, 2), (2, 2), (27, 27), (255, 255)]:
                items = many[:place] + [target] + many[place:others]
                qs = many_q[:place] + [tq] + many_q[place:others]
                got = check_stream(st, full, items, qs, mode, what="%d boxes" % len(items))
                assert got[place] == alone, "%s: %d boxes, place %d" % (mode, len(items), place)
            chain(2048)
            got = check_stream(st, full, [target], [tq], mode, what="chain")
            assert st.stats()["chain_levels_last_request"] > 0 and got[0] == alone, "the chain at 2048"
            chain(0)
            with sz3_amd.debug_flags2(int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                got = check_stream(st, full, many[:27] + [target], many_q[:27] + [tq], mode, what="by level")
                assert got[27] == alone, "level group by level group"
                items = mixed(shape)
                check_stream(st, full, items, queries_for(items, 1), mode, True, 0.0, what="by level")


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
        for points_ in (0, 2048):
            chain(points_)
            for items in [three, twelve, mixed(shape)] + one_level:
                q = launches(lambda: ask(st, items))
                cq = st.stats()["chain_levels_last_request"]
                for mode in MODES:
                    r = launches(lambda: check_stream(st, full, items, queries_for(items, 2), mode))
                    s = st.stats()
                    assert r == q and s["chain_levels_last_request"] == cq and s["chain_points"] == points_, "a sample issues the request's launches (%d, %d; threshold %d)" % (r, q, points_)
            assert points_ == 0 or st.stats()["chain_levels_last_request"] > 0, "one level at threshold 2048 takes the chain"
            items = mixed(shape)
            with sz3_amd.debug_flags2(int(sz3_amd.Dbg2.REQUEST_BY_LEVEL)):
                q = launches(lambda: ask(st, items))
                assert launches(lambda: check_stream(st, full, items, queries_for(items), "linear")) == q
        torch.cuda.synchronize()


def check_fallback(st, full, name):
    assert st.stats()["fast"] == 0
    for shift, mode in enumerate(MODES):
        for clamp in (False, True):
            check_stream(st, full, FB_ITEMS, queries_for(FB_ITEMS, shift + clamp), mode, clamp, -2.0, what=name)
            s = st.stats()
            assert s["fast"] == 0 and s["launches_last_request"] == 1 and s["chain_levels_last_request"] == 0


@pytest.mark.parametrize("name,kw", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_fallback_containers(name, kw):
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **kw))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    assert conf.cmprAlgo not in INTERP_IDS
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        check_fallback(st, full, name)


def test_fallback_openmp_slabs(monkeypatch):
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
    td = getattr(torch, st.dtype.name)
    lattice = oblique(good[0][2], (2, 3, 4))

    def refused(fragment, edit=None, mode="linear", coord="float64", flags=0, reserved=0, null_opts=False, lattice_at=None):
        held = [dev(uniform(it[2], 50, i).astype(coord)) for i, it in enumerate(good)]
        qs = list(held)
        if lattice_at is not None:
            qs[lattice_at] = lattice
        reqs, _, cname, _ = sz3_amd._sample_reqs(N, good, qs)
        bufs = [filled(int(reqs[i].n_points) + PAD, td) for i in range(n)]
        for i, b in enumerate(bufs):
            reqs[i].d_out = b.data_ptr()
        o = sz3_amd._sample_opts(mode, False, NAN, cname)
        o.flags, o.reserved = flags, reserved
        if edit:
            edit(reqs, o)
        rc = L.sz3hip_stream_sample(st._h, reqs, n, None if null_opts else C.byref(o), sz3_amd._stream_handle(st.device, None))
        msg = L.sz3hip_last_error().decode()
        assert rc == einval and fragment in msg, (rc, msg, fragment)
        torch.cuda.synchronize()
        assert all((t.view(torch.uint8) == FILL).all() for t in bufs), "a refused call wrote (%s)" % fragment
        # the handle serves the next request with the full decode's bytes
        same(ask(st, good[:3]), full, good[:3], "after a refusal (%s)" % fragment)

    def opt(name, v):
        def f(reqs, o):
            setattr(o, name, v)
        return f

    def box(b, name, v, index=None):
        def f(reqs, o):
            if index is None:
                setattr(reqs[b], name, v(getattr(reqs[b], name)) if callable(v) else v)
            else:
                getattr(reqs[b], name)[index] = v
        return f

    refused("NULL argument (opts)", null_opts=True)
    refused("filter", edit=opt("filter", 2))
    refused("coord_type", edit=opt("coord_type", 2))
    refused("flags", flags=2)
    refused("reserved", reserved=1)
    for b in (0, n // 2, n - 1):  # a box's: at the first, a middle and the last box
        at = "box %d: " % b
        refused(at + "the reserved word", edit=box(b, "reserved", 3))
        refused(at + "the output array is NULL", edit=box(b, "d_out", None))
        refused(at + "the output is not aligned", edit=box(b, "d_out", lambda p: p + 2))
        refused(at + "n_points is 0", edit=box(b, "n_points", 0))
        refused(at + "n_points is", edit=box(b, "n_points", (1 << 31) + 1))
        refused(at + "d_coords is not aligned", edit=box(b, "d_coords", lambda p: p + 4))
        refused(at + "d_coords is not aligned", edit=box(b, "d_coords", lambda p: p + 2), coord="float32")
        refused(at + "d_coords is given with a lattice", edit=box(b, "counts", 1, 2))
        refused(at + "d_coords is given with a lattice", edit=box(b, "origin", 0.5, 0))
        refused(at + "the lattice's count of axis 1 is 0", edit=box(b, "counts", 0, 1), lattice_at=b)
        refused(at + "the lattice's counts (2 x 3 x 4) do not multiply to n_points (23)", edit=box(b, "n_points", 23), lattice_at=b)
        refused(at + "the lattice's origin[1] is not finite", edit=box(b, "origin", float("inf"), 1), lattice_at=b)

        def step(reqs, o, b=b):
            reqs[b].steps[2][N - 1] = NAN
        refused(at + "the lattice's steps[2][%d] is not finite" % (N - 1), edit=step, lattice_at=b)

        def leave(reqs, o, b=b):
            reqs[b].box.lo[N - 1] = 1 << 40
        refused(at, edit=leave)
        refused(at, edit=box(b, "level", 31))
        if b:
            def overlap(reqs, o, b=b):
                reqs[b].d_out = reqs[0].d_out + 4 * st.dtype.itemsize
            refused(at + "the output overlaps box 0's", edit=overlap)
    assert st.stats()["requests"] > before


def test_refusals():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        refusals(st, full, mixed(shape)[:9])


def test_refusals_on_a_fallback_handle():
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **dict(FALLBACKS[0][1])))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 0
        refusals(st, full, FB_ITEMS[:6])


def test_refusals_of_sample_points():
    t = torch.zeros((4, 5), dtype=torch.float32, device=DEV)
    q = dev(uniform((4, 5), 10, 0))
    with pytest.raises(sz3_amd.SZ3HipError, match="not finite"):
        sz3_amd.sample_points(t, ([0.0, float("nan")], [[0.0, 1.0]], (4,)))
    with pytest.raises(ValueError):
        sz3_amd.sample_points(t, q[:, :1].contiguous())
    with pytest.raises(ValueError):
        sz3_amd.sample_points(t, q.cpu())
    with pytest.raises(TypeError):
        sz3_amd.sample_points(t.to(torch.float16), q)
    with pytest.raises(sz3_amd.SZ3HipError, match="integer element types"):
        sz3_amd.sample_points(t.to(torch.int32), q)
    with pytest.raises(ValueError, match="mode"):
        sz3_amd.sample_points(t, q, mode="cubic")


# ---- 7. ordering -----------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_and_two_streams():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    items = mixed(shape)
    x_items, y_items = items[:9], items[5:]
    f = full.cpu().numpy().astype(np.float64)
    lo, hi = [float(v) for v in np.quantile(f, [0.25, 0.75])]
    qx, qy = queries_for(x_items, 0), queries_for(y_items, 3)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        want_x = check_stream(st, full, x_items, qx, "linear")
        want_y = check_stream(st, full, y_items, qy, "nearest", True, 0.0)
        want_red = st.reduce(x_items, 7, -0.5, 0.75).stats.cpu().numpy().tobytes()
        sel = st.select(y_items, lo, hi, 64)
        want_sel = [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()]
        want_map = [m.cpu().numpy().tobytes() for m in st.map(x_items, "u8", lo=lo, hi=hi)]
        torch.cuda.synchronize()
        for _ in range(2):  # no host synchronisation in between
            keep = []
            bx0, cx, h = stream_sample(st, x_items, qx, "linear")
            keep.append(h)
            x = ask(st, x_items, sync=False, stream=s1)
            by0, cy, h = stream_sample(st, y_items, qy, "nearest", True, 0.0, stream=s2)
            keep.append(h)
            red = st.reduce(x_items, 7, -0.5, 0.75, stream=s1)
            bx1, _, h = stream_sample(st, x_items, qx, "linear", stream=s2)
            keep.append(h)
            sel = st.select(y_items, lo, hi, 64)
            mp = st.map(x_items, "u8", lo=lo, hi=hi, stream=s1)
            by1, _, h = stream_sample(st, y_items, qy, "nearest", True, 0.0, stream=s1)
            keep.append(h)
            y = ask(st, y_items, sync=False, stream=s2)
            torch.cuda.synchronize()
            for bufs in (bx0, bx1):
                assert [taken(b, c).tobytes() for b, c in zip(bufs, cx)] == want_x
            for bufs in (by0, by1):
                assert [taken(b, c).tobytes() for b, c in zip(bufs, cy)] == want_y
            assert red.stats.cpu().numpy().tobytes() == want_red
            assert [(c, ix.tobytes(), v.tobytes()) for c, ix, v in sel.numpy()] == want_sel
            assert [m.cpu().numpy().tobytes() for m in mp] == want_map
            same(x, full, x_items)
            same(y, full, y_items)

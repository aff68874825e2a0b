"""Per-box statistics of an opened stream on the MI355X: Stream.reduce, reduce_stats.

Expected values come from the full decode's [::2**k] slice in numpy. Counts, indices and histogram counts must be EQUAL; min, max and shift
must have the RAW BYTES of the slice's elements; mean and variance must be bit-equal to the two formulas of the struct's comments evaluated
in numpy float64 from the reported shift, sum, sum_sq, n, n_nonfinite (with m = 0 both are NaN: a NaN's payload is not part of the contract).
sum and sum_sq are held to the exact rational sums (fractions.Fraction over the slice) by bounds derived from the arithmetic, not measured:
with u = 2**-53 and gamma(k) = k u / (1 - k u),
    |sum    - S1| <= gamma(n)     * sum |v - K|        each term v - K rounded once, at most n - 1 additions in any order
    |sum_sq - S2| <= gamma(n + 2) * sum (v - K)**2     each term rounded once, each square once, at most n - 1 additions
Boxes checked this way hold at most 20 000 points, so that the exact sums stay fast; larger boxes are held to everything else and — like all
boxes — to the feature itself: Stream.reduce must equal, in every byte of the 88 and of the histogram row, reduce_stats over the tensor
Stream.request delivers for that box."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, conf_for, container, device_payload, smooth  # noqa: E402
from sink_models import EXACT_POINTS, bits, gamma, hist_of, reduce_check_box as check_box  # noqa: E402,F401
from test_gpu_request import FB_ITEMS, alloc, ask, atlas_for, chain, chain_off, mixed, same  # noqa: E402,F401
from test_gpu_stream import SHAPES, IDS, case, coarse_shape, coarse_view, opens, spiky_blob, tile_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
FIELDS = list(sz3_amd.BOX_STATS_DTYPE.names)


def rows(res):
    """(stats as raw int64 rows, histogram rows or None): synchronises"""
    torch.cuda.synchronize()
    return res.stats.cpu().numpy().copy(), None if res.hist is None else res.hist.cpu().numpy().copy()


def check_items(res, full, items, bins=0, lo=0.0, hi=0.0, what=""):
    st, hist = res.numpy()
    assert len(st) == len(items)
    for i, (k, blo, ext) in enumerate(items):
        v = coarse_view(full, k)[box_slices(blo, ext)].cpu().numpy()
        check_box(st[i], None if hist is None else hist[i], v, bins, lo, hi, "%s box %d (level %d, lo %s shape %s)" % (what, i, k, blo, ext))


def same_rows(a, b, what=""):
    (sa, ha), (sb, hb) = a, b
    assert sa.tobytes() == sb.tobytes(), what + " the statistics' bytes differ"
    assert (ha is None) == (hb is None) and (ha is None or ha.tobytes() == hb.tobytes()), what + " the histograms differ"


def against_itself(st, items, got, bins, lo, hi, what=""):
    """Stream.reduce against reduce_stats over what Stream.request delivers: contiguous arrays, then rectangles of an atlas"""
    sg, hg = got
    atlas, views = atlas_for(st, items, pad=1)
    if atlas.dim() == 1:  # (a stretch of a 1-D atlas is contiguous: every second element of an array of its own instead)
        views = [torch.full((2 * ext[0],), 77.0, dtype=atlas.dtype, device=DEV)[::2] for _, _, ext in items]
    st.request([it + (v,) for it, v in zip(items, views)])
    for outs in (ask(st, items), views):
        for i, t in enumerate(outs):
            r = rows(sz3_amd.reduce_stats(t, bins, lo, hi))
            same_rows((sg[i:i + 1], None if hg is None else hg[i:i + 1]), r, "%s box %d (%s):" % (what, i, "contiguous" if t.is_contiguous() else "atlas"))
    assert any(not v.is_contiguous() for v in views), "strided views among them"


def check_stream(st, full, items, bins=7, lo=-0.5, hi=0.75, what=""):
    res = st.reduce(items, bins, lo, hi)
    check_items(res, full, items, bins, lo, hi, what)
    got = rows(res)
    same_rows(got, rows(st.reduce(items, bins, lo, hi)), what + " a second call:")
    against_itself(st, items, got, bins, lo, hi, what)
    return got


# ---- 1. mixed levels, both opens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mixed_levels(shape, dtype, interp):
    kw = (("interpAlgo", interp),)
    items = mixed(shape)
    algo = case(shape, dtype, kw)[3].cmprAlgo
    for name, st, full in opens(shape, dtype, kw):
        fast = name == "open_payload" or algo in INTERP_IDS
        with st, chain_off():
            assert st.stats()["fast"] == (1 if fast else 0)
            check_stream(st, full, items, what=name)
            s = st.stats()
            assert s["huffman_stages"] == (1 if fast else 0)


def test_stock_container():
    shape = (65, 47, 130)
    a = smooth(shape)
    sz3_amd.set_stock_format(1)
    try:
        blob = container(a, conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO))
    finally:
        sz3_amd.set_stock_format(0)
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 1
        check_stream(st, full, mixed(shape), what="stock")


@pytest.mark.parametrize("anchor", [0, 4], ids=["stride0", "stride4"])
def test_anchors(anchor):
    shape = (65, 47, 130)
    kw = (("interpAnchorStride", anchor),)
    for name, st, full in opens(shape, "float32", kw):
        with st, chain_off():
            check_stream(st, full, mixed(shape), what=name)


def test_a_grid_of_one_point():
    shape, top = (65, 47, 130), 8
    assert coarse_shape(shape, top) == (1, 1, 1)
    for name, st, full in opens(shape):
        with st:
            items = [(top, (0, 0, 0), (1, 1, 1)), (0,) + tile_boxes(shape)[4], (top - 1, (0, 0, 0), coarse_shape(shape, top - 1)), (top, (0, 0, 0), (1, 1, 1))]
            got = check_stream(st, full, items, what=name)
            one = rows(st.reduce([items[0]], 7, -0.5, 0.75))  # (no level runs at all)
            same_rows((got[0][:1], got[1][:1]), one, "alone:")
            r = got[0].view(sz3_amd.BOX_STATS_DTYPE).reshape(-1)[0]
            assert r["n"] == 1 and r["argmin"] == 0 and r["argmax"] == 0 and r["sum"] == 0.0 and r["variance"] == 0.0 and bits(r["mean"]) == bits(r["min"])


@pytest.mark.parametrize("stock", [0, 1], ids=["id17", "stock"])
def test_spikes(stock):
    """raw records inside some boxes' windows and outside others'"""
    a, pos, blob = spiky_blob(stock)
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    items = mixed(a.shape)
    handles = [("open_stream", sz3_amd.open_stream(blob, np.float32, device=DEV), full)]
    if not stock:
        dc, pl, size, pfull = device_payload(a, conf_for(a.shape, quantbinCnt=256))
        handles.append(("open_payload", dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream), pfull))
    for name, st, ref in handles:
        with st:
            assert st.stats()["fast"] == 1
            got = check_stream(st, ref, items, bins=256, lo=-2.0, hi=2e6, what=name)
            mx = got[0].view(np.float64)[:, FIELDS.index("max")]
            assert (mx == 1e6).any() and (mx < 1e6).any(), "spikes inside some boxes and outside others"


def test_non_finite_points():
    shape = (65, 47, 130)
    a = smooth(shape)
    for p, v in zip([(0, 0, 0), (8, 8, 16), (16, 24, 64), (33, 21, 77), (64, 40, 128)], [np.nan, np.inf, -np.inf, np.nan, np.inf]):
        a[p] = v
    conf = conf_for(shape)
    blob = container(a, conf)
    full, _ = sz3_amd.decompress(blob, np.float32, device=DEV)
    items = mixed(shape) + [(3, (1, 1, 2), (1, 1, 1)), (0, (0, 0, 0), (1, 1, 1)), (0, (0, 0, 0), (1, 1, 2))]
    nonfin = [int((~np.isfinite(coarse_view(full, k)[box_slices(lo, ext)].cpu().numpy())).sum()) for k, lo, ext in items]
    fin = [int(np.isfinite(coarse_view(full, k)[box_slices(lo, ext)].cpu().numpy()).sum()) for k, lo, ext in items]
    assert max(nonfin) > 0 and max(fin) > 0 and min(nonfin) == 0 and min(fin) == 0, "boxes with and without non-finite points, one with nothing finite"
    dc, pl, size, pfull = device_payload(a, conf_for(shape))
    handles = [("open_stream", sz3_amd.open_stream(blob, np.float32, device=DEV), full),
               ("open_payload", dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream), pfull)]
    for name, st, ref in handles:
        with st:
            got = check_stream(st, ref, items, what=name)
            r = got[0].view(sz3_amd.BOX_STATS_DTYPE).reshape(-1)
            assert int(r["n_nonfinite"].max()) > 0 and (r["n_nonfinite"] == r["n"]).any() and (r["shift"][r["n_nonfinite"] == r["n"]] == 0.0).all()
    dc.close()


# ---- 2. histograms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 7, 256, 1024])
def test_histograms(bins):
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    items = mixed(shape)[:12]
    flat = np.sort(full.cpu().numpy().reshape(-1))
    lo_v, hi_v = float(flat[flat.size // 5]), float(flat[4 * flat.size // 5])  # (values of the field: points exactly on lo and on hi)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for lo, hi in [(lo_v, hi_v), (-10.0, 10.0), (5.0, 6.0), (-7.0, -6.5), (lo_v, lo_v + 2.0 ** -20)]:
            res = st.reduce(items, bins, lo, hi)
            check_items(res, full, items, bins, lo, hi, "bins %d [%r, %r):" % (bins, lo, hi))
        s, h = st.reduce(items, bins, lo_v, hi_v).numpy()
        whole = full.cpu().numpy().astype(np.float64).reshape(-1)
        assert (whole == lo_v).any() and (whole == hi_v).any() and h[0, 0] > 0 and h[0, bins + 1] > 0 and h[0, 1:bins + 1].sum() > 0
    # an inner bin edge, exactly: [0, 8) in 8 bins, values on the integers and next to them
    t = torch.tensor([0.0, 1.0, 3.0, np.nextafter(3.0, 0.0), 7.0, 8.0, np.nextafter(8.0, 0.0), -0.0, np.nextafter(0.0, -1.0), 4.5, np.nan], dtype=torch.float64, device=DEV)
    s, h = sz3_amd.reduce_stats(t, 8, 0.0, 8.0).numpy()
    assert h[0].tolist() == [1, 2, 1, 1, 1, 1, 0, 0, 2, 1]
    check_box(s[0], h[0], t.cpu().numpy(), 8, 0.0, 8.0)


# ---- 3. reduce_stats on crafted tensors, no stream -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 1])
def test_partition_edges(total, dtype):
    rng = np.random.default_rng(total)
    v = (rng.normal(3.0, 2.0, total)).astype(dtype)
    t = torch.from_numpy(v).to(DEV)
    res = sz3_amd.reduce_stats(t, 7, 0.0, 6.0)
    s, h = res.numpy()
    check_box(s[0], h[0], v, 7, 0.0, 6.0, "total %d" % total)
    same_rows(rows(res), rows(sz3_amd.reduce_stats(t.clone(), 7, 0.0, 6.0)), "another array, the same values:")
    s0, h0 = sz3_amd.reduce_stats(t).numpy()  # (no histogram)
    assert h0 is None and s0.tobytes() == s.tobytes()


def test_crafted_values():
    def one(v, **kw):
        s, h = sz3_amd.reduce_stats(v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)).to(DEV), **kw).numpy()
        return s[0], None if h is None else h[0]

    c = np.full(9001, 2.5, dtype=np.float32)  # a constant field
    s, _ = one(c)
    check_box(s, None, c)
    assert s["argmin"] == 0 and s["argmax"] == 0 and s["sum"] == 0.0 and s["sum_sq"] == 0.0 and s["mean"] == 2.5 and s["variance"] == 0.0
    z = np.zeros(5000, dtype=np.float64)  # -0.0 / +0.0 tie: the earlier element's sign
    z[::2] = -0.0
    s, _ = one(z)
    check_box(s, None, z)
    assert s["argmin"] == 0 and s["argmax"] == 0 and np.signbit(s["min"]) and np.signbit(s["max"])
    s, _ = one(z[1:].copy())
    assert s["argmin"] == 0 and not np.signbit(s["min"]) and not np.signbit(s["max"])
    d = np.random.default_rng(3).normal(0.0, 1.0, 3 * 4096 + 100).astype(np.float32)  # the minimum twice, in two chunks; the maximum too
    d[[4096 + 17, 2 * 4096 + 5]] = -50.0
    d[[3 * 4096 + 3, 77]] = 60.0
    s, _ = one(d)
    check_box(s, None, d)
    assert s["argmin"] == 4096 + 17 and s["argmax"] == 77
    e = np.array([np.nan, np.inf, -np.inf] * 1500, dtype=np.float32)  # nothing finite
    s, h = one(e, bins=4, lo=0.0, hi=1.0)
    check_box(s, h, e, 4, 0.0, 1.0)
    assert s["n_nonfinite"] == 4500 and s["argmin"] == 4500 and h.sum() == 0
    f = d.copy()  # a non-finite element 0: the shift is 0.0
    f[0] = np.inf
    s, _ = one(f)
    check_box(s, None, f)
    assert s["shift"] == 0.0 and s["n_nonfinite"] == 1
    g = torch.from_numpy(np.random.default_rng(4).normal(1.0, 1.0, (7, 50, 66)).astype(np.float32)).to(DEV)
    v = g[:, 1:40, ::2]  # x stride 2, a step along y
    s, h = one(v, bins=16, lo=-1.0, hi=3.0)
    check_box(s, h, v.cpu().numpy(), 16, -1.0, 3.0, "x stride 2")
    b = g[0, 3].expand(9, 66)  # a stride-0 broadcast
    assert b.stride(0) == 0
    s, _ = one(b)
    check_box(s, None, b.cpu().numpy(), what="broadcast")
    q = torch.from_numpy(np.random.default_rng(5).normal(-2.0, 3.0, (5, 6, 7, 40)).astype(np.float64)).to(DEV)  # 4-D, a view of it
    for v in (q, q[1:, :, 2:6, 3:37]):
        s, h = one(v, bins=256, lo=-5.0, hi=1.0)
        check_box(s, h, v.cpu().numpy(), 256, -5.0, 1.0, "4-D")


# ---- 4. position in the request, number of boxes ---------------------------------------------------------------------------------------------
def test_position_and_number_of_boxes():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    rng = np.random.default_rng(17)
    many = []
    for i in range(255):  # mixed levels, mixed sizes
        k = int(rng.integers(0, 4))
        cs = coarse_shape(shape, k)
        ext = tuple(int(min(d, rng.integers(1, 13))) for d in cs)
        many.append((k, tuple(int(rng.integers(0, d - e + 1)) for d, e in zip(cs, ext)), ext))
    target = (1, (3, 2, 7), (21, 19, 33))  # 13167 points: four chunks
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        alone = rows(st.reduce([target], 256, -1.0, 1.0))
        check_items(st.reduce([target], 256, -1.0, 1.0), full, [target], 256, -1.0, 1.0)
        for place, others in [(0, many[:2]), (2, many[:2]), (5, mixed(shape)), (255, many), (100, many)]:
            items = list(others[:place]) + [target] + list(others[place:])
            assert len(items) <= 256
            s, h = rows(st.reduce(items, 256, -1.0, 1.0))
            same_rows(alone, (s[place:place + 1], h[place:place + 1]), "%d boxes, place %d:" % (len(items), place))
        res = st.reduce(many + [target], 7, -0.5, 0.75)
        assert st.stats()["requests"] == 8
        check_items(res, full, many + [target], 7, -0.5, 0.75, "256 boxes,")


# ---- 5. fallback handles: two launches out of the resident array -----------------------------------------------------------------------------
def check_fallback(st, full, name):
    assert st.stats()["fast"] == 0
    check_stream(st, full, FB_ITEMS, what=name)
    st.reduce(FB_ITEMS)
    s = st.stats()
    assert s["fast"] == 0 and s["launches_last_request"] == 2 and s["chain_levels_last_request"] == 0


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


# ---- 6. the launch count ---------------------------------------------------------------------------------------------------------------------
def test_launch_count(chain):
    shape = (65, 47, 130)
    kw = (("interpAlgo", 0),)
    a, blob, full, conf = case(shape, "float32", kw)
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
            counts = []
            for items in [three, twelve, mixed(shape)] + one_level:
                q = launches(lambda: ask(st, items))
                cq = st.stats()["chain_levels_last_request"]
                r = launches(lambda: st.reduce(items, 7, -0.5, 0.75))
                s = st.stats()
                assert r == q + 1, "a reduce is the request's launches plus one (%d, %d; threshold %d)" % (r, q, points)
                assert s["chain_levels_last_request"] == cq and s["chain_points"] == points
                counts.append(r)
            assert counts[0] == counts[1], "twelve boxes issue as many launches as three"
            assert points == 0 or st.stats()["chain_levels_last_request"] > 0, "one level at threshold 2048 takes the chain"
            with sz3_amd.debug_flags2(sz3_amd.Dbg2.REQUEST_BY_LEVEL):  # level group by level group: still ONE final
                items = mixed(shape)
                q = launches(lambda: ask(st, items))
                res = None

                def f():
                    nonlocal res
                    res = st.reduce(items, 7, -0.5, 0.75)
                assert launches(f) == q + 1
                grouped = rows(res)
            same_rows(grouped, rows(st.reduce(items, 7, -0.5, 0.75)), "by level against merged:")
        check_items(st.reduce(twelve, 7, -0.5, 0.75), full, twelve, 7, -0.5, 0.75, "threshold 2048,")


def test_one_huffman_stage():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    d0, t0 = sz3_amd.debug_tile_units()
    items = mixed(shape)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        for i in range(10):
            sub = items[i % 5:len(items) - i]
            res = st.reduce(sub, 7 if i % 2 else 0, -0.5, 0.75)
        check_items(res, full, sub, 7, -0.5, 0.75)
        s = st.stats()
        assert s["huffman_stages"] == 1 and s["requests"] == 10
    assert sz3_amd.debug_tile_units() == (d0, t0), "no reduce ran a tile decode's Huffman stage"


# ---- 7. ordering -----------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_and_two_streams():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    items = mixed(shape)
    x_items, y_items = items[:9], items[5:]
    b1 = tile_boxes(coarse_shape(shape, 1))
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        want_x, want_y = rows(st.reduce(x_items, 7, -0.5, 0.75)), rows(st.reduce(y_items, 7, -0.5, 0.75))
        check_items(st.reduce(x_items, 7, -0.5, 0.75), full, x_items, 7, -0.5, 0.75)
        for _ in range(2):  # no host synchronisation in between
            bufs = [alloc(st, its) for its in (x_items, y_items)]
            tb = [torch.full(ext, 77.0, dtype=torch.float32, device=DEV) for _, ext in b1]
            torch.cuda.synchronize()
            r = [st.reduce(x_items, 7, -0.5, 0.75), st.reduce(y_items, 7, -0.5, 0.75)]
            x = ask(st, x_items, sync=False, outs=bufs[0])
            r.append(st.reduce(x_items, 7, -0.5, 0.75, stream=s1))
            t = st.tiles(1, b1, out=tb, stream=s1)
            r.append(st.reduce(y_items, 7, -0.5, 0.75, stream=s2))
            y = ask(st, y_items, sync=False, stream=s1, outs=bufs[1])
            r.append(st.reduce(x_items, 7, -0.5, 0.75, stream=s2))
            r.append(st.reduce(y_items, 7, -0.5, 0.75))
            torch.cuda.synchronize()
            for got, want in zip(r, (want_x, want_y, want_x, want_y, want_x, want_y)):
                same_rows(rows(got), want, "back to back:")
            same(x, full, x_items)
            same(y, full, y_items)
            same(t, full, [(1,) + b for b in b1], "tiles between the reduces,")
    # reduce_stats on two streams shares the library's partial records: ordered by an event
    big = torch.from_numpy(np.random.default_rng(9).normal(0, 1, 300000).astype(np.float32)).to(DEV)
    small = big[:5000].clone()
    torch.cuda.synchronize()
    wb, ws = rows(sz3_amd.reduce_stats(big)), rows(sz3_amd.reduce_stats(small))
    rs = []
    for i in range(6):
        rs.append(sz3_amd.reduce_stats(big if i % 2 == 0 else small, stream=(s1, s2)[i % 2] if i % 3 else None))
    torch.cuda.synchronize()
    for i, got in enumerate(rs):
        same_rows(rows(got), wb if i % 2 == 0 else ws, "reduce_stats on two streams:")


# ---- 8. refusals on an open handle -----------------------------------------------------------------------------------------------------------
def refusals(st, full, good):
    N = len(good[0][1])
    before = st.stats()["requests"]
    bins = 5
    stats = torch.full((len(good), 11), 0x4D4D4D4D, dtype=torch.int64, device=DEV)
    hist = torch.full((len(good), bins + 2), 0x4D4D4D4D, dtype=torch.int64, device=DEV)
    reqs = (sz3_amd._CReduceReq * 300)()
    arr, _ = sz3_amd._boxes(N, [it[1:] for it in good])
    opts = sz3_amd._CReduceOpts()
    einval = CODES["SZ3HIP_EINVAL"]

    def fill():
        for i, it in enumerate(good):
            reqs[i].level, reqs[i].reserved, reqs[i].box = it[0], 0, arr[i]
        opts.nbins, opts.reserved, opts.lo, opts.hi = bins, 0, -0.5, 0.75

    def call(n=len(good), d_stats=stats.data_ptr(), d_hist=hist.data_ptr(), h=st._h, o=opts):
        rc = L.sz3hip_stream_reduce(h, reqs, n, C.byref(o) if o is not None else None, d_stats, d_hist, torch.cuda.current_stream().cuda_stream)
        return rc, L.sz3hip_last_error().decode()

    for place in (0, 1, len(good) - 1):
        fill()
        reqs[place].level = 31
        assert call() == (einval, "box %d: tile level 31 is outside 0 .. 30" % place)
        fill()
        reqs[place].level = -1
        rc, msg = call()
        assert rc == einval and "box %d: " % place in msg
        fill()
        reqs[place].level = 1
        reqs[place].box.lo[0], reqs[place].box.ext[0] = 30, 4
        rc, msg = call()
        assert rc == einval and "box %d: " % place in msg and "dimension 0" in msg
        fill()
        reqs[place].box.ext[N - 1] = 0
        rc, msg = call()
        assert rc == einval and "box %d: " % place in msg and "extent 0" in msg
        fill()
        reqs[place].reserved = 3
        assert call() == (einval, "box %d: the reserved word is 3, not 0" % place)
        reqs[place].box = arr[place]
    fill()
    opts.reserved = 1
    assert call()[0] == einval and "reserved" in call()[1]
    for nb, lo, hi, word in [(1025, 0.0, 1.0, "1025 bins"), (5, 1.0, 1.0, "above lo"), (5, 1.0, 0.0, "above lo"), (5, np.nan, 1.0, "not finite"), (5, 0.0, np.inf, "not finite")]:
        fill()
        opts.nbins, opts.lo, opts.hi = nb, lo, hi
        rc, msg = call()
        assert rc == einval and word in msg, msg
    fill()
    assert call(d_hist=None)[0] == einval and "d_hist" in call(d_hist=None)[1]
    assert call(d_stats=None)[0] == einval and "d_stats" in call(d_stats=None)[1]
    assert call(0)[0] == einval and "1 .. 256 boxes" in call(0)[1]
    assert call(257)[0] == einval and "1 .. 256 boxes" in call(257)[1]
    assert call(h=None)[0] == einval and "no handle" in call(h=None)[1]
    assert L.sz3hip_stream_reduce(st._h, None, 1, None, stats.data_ptr(), None, None) == einval
    torch.cuda.synchronize()
    assert bool((stats == 0x4D4D4D4D).all()) and bool((hist == 0x4D4D4D4D).all()), "a refused reduce writes nothing"
    assert st.stats()["requests"] == before
    # the handle serves the next requests: without options and without a histogram array, then with both
    fill()
    assert call(d_hist=None, o=None)[0] == 0
    opts.nbins = 0
    assert call(d_hist=None)[0] == 0
    torch.cuda.synchronize()
    assert bool((hist == 0x4D4D4D4D).all()), "no histogram asked for: the array is not touched"
    res = st.reduce(good, bins, -0.5, 0.75)
    check_items(res, full, good, bins, -0.5, 0.75, "after the refusals,")
    assert stats.cpu().numpy().tobytes() == rows(res)[0].tobytes()
    same(ask(st, good), full, good, "after the refusals,")


def test_refusals():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    good = [(k,) + tile_boxes(coarse_shape(shape, k))[j] for k, j in ((2, 2), (0, 4), (1, 3), (3, 0))]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        refusals(st, full, good)
    with pytest.raises(sz3_amd.SZ3HipError) as e:  # a closed handle
        st.reduce(good)
    assert e.value.code == CODES["SZ3HIP_EINVAL"] and "no handle" in str(e.value)
    with pytest.raises(TypeError):
        sz3_amd.reduce_stats(np.zeros(4, dtype=np.float32))
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.reduce_stats(torch.zeros(8, dtype=torch.int32, device=DEV))
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"] and "integer element types are not supported yet" in str(e.value)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.reduce_stats(torch.zeros(8, dtype=torch.float32, device=DEV), bins=4, lo=2.0, hi=1.0)
    assert e.value.code == CODES["SZ3HIP_EINVAL"]


def test_refusals_on_a_fallback_handle():
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **dict(FALLBACKS[0][1])))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 0
        refusals(st, full, FB_ITEMS[:4])

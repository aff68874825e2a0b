"""The points of boxes whose values lie in a range, on the MI355X: Stream.select, select_points.

Expected values come from numpy over the full decode's [::2**k] slice of the box, s, with x = s.astype(float64).ravel(): idx =
flatnonzero(pred(x)); count == idx.size; written == min(count, capacity); d_index[:written] EQUAL to idx[:written]; d_value[:written] equal in
RAW BYTES to s.ravel()[idx[:written]]; everything from `written` on, and every output of a refused call, still holds its sentinel. Ranges are
taken from the field's own quantiles. Every selection is also held to the feature itself: Stream.select must equal, in every byte of head,
index and value, select_points over the tensor Stream.request delivers for that box."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
from partial_cases import CODES, DEV, FALLBACKS, INTERP_IDS, box_slices, conf_for, container, device_payload, smooth  # noqa: E402
from sink_models import SENT, pred, raw_select, select_check_box as check_box, sentinels, t_size, utype  # noqa: E402,F401
from test_gpu_request import FB_ITEMS, alloc, ask, atlas_for, chain, chain_off, mixed, same  # noqa: E402,F401
from test_gpu_stream import SHAPES, IDS, case, coarse_shape, coarse_view, opens, spiky_blob, tile_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
CHUNK = 4096
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def raw_points(t, cap, lo, hi, invert=False, nan=False, values=True, stream=None):
    """select_points' call into sentinel-filled arrays"""
    keep = [i for i, d in enumerate(t.shape) if int(d) != 1]
    dims = [int(t.shape[i]) for i in keep] or [1]
    strides = [int(t.stride(i)) for i in keep] or [1]
    N = len(dims)
    heads = torch.full((1, 4), SENT, dtype=torch.int64, device=DEV)
    index, value = sentinels([cap], t.dtype, values)
    opts = sz3_amd._select_opts(lo, hi, invert, nan)
    rc = L.sz3hip_select_device(0 if t.dtype == torch.float32 else 1, N, (C.c_uint64 * N)(*dims), t.data_ptr(), (C.c_int64 * N)(*strides), C.byref(opts),
                                index[0].data_ptr() if cap else None, value[0].data_ptr() if values and cap else None, cap, heads.data_ptr(),
                                sz3_amd._stream_handle(DEV, stream))
    assert rc == 0, L.sz3hip_last_error().decode()
    return heads, index, value


def to_bytes(heads, index, value):
    """(heads, per-box index bytes, per-box value bytes) on the host: synchronises"""
    torch.cuda.synchronize()
    return (heads.cpu().numpy().tobytes(), [t.cpu().numpy().tobytes() for t in index], None if value is None else [t.cpu().numpy().tobytes() for t in value])


def slices_of(full, items):
    return [coarse_view(full, k)[box_slices(lo, ext)].cpu().numpy() for k, lo, ext in items]


def caps_for(slices, lo, hi, invert=False, nan=False):
    """per box, in turn: every point, count - 1, count + 1, half the count, nothing, the count itself"""
    caps = []
    for i, s in enumerate(slices):
        c = int(pred(s.astype(np.float64).reshape(-1), lo, hi, invert, nan).sum())
        caps.append([s.size, max(c - 1, 0), c + 1, c // 2, 0, c][i % 6])
    return caps


def check_select(st, full, items, lo, hi, invert=False, nan=False, values=True, what="", caps=None):
    slices = slices_of(full, items)
    caps = caps_for(slices, lo, hi, invert, nan) if caps is None else caps
    rc, heads, index, value = raw_select(st, items, caps, lo, hi, invert, nan, values)
    assert rc == 0, L.sz3hip_last_error().decode()
    torch.cuda.synchronize()
    h = heads.cpu().numpy()
    counts = []
    for i, (it, s) in enumerate(zip(items, slices)):
        counts.append(check_box(h[i], index[i].cpu().numpy(), None if value is None else value[i].cpu().numpy(), s, caps[i], lo, hi, invert, nan,
                                "%s box %d %s [%r, %r] invert %d nan %d:" % (what, i, it, lo, hi, invert, nan)))
    return caps, counts, to_bytes(heads, index, value)


def same_bytes(a, b, what=""):
    assert a[0] == b[0], what + " the heads differ"
    assert a[1] == b[1], what + " the indices' bytes differ"
    assert a[2] == b[2], what + " the values' bytes differ"


def against_itself(st, items, caps, got, lo, hi, invert=False, nan=False, what=""):
    """Stream.select against select_points over what Stream.request delivers: contiguous arrays, then rectangles of an atlas"""
    hg, ig, vg = got
    atlas, views = atlas_for(st, items, pad=1)
    if atlas.dim() == 1:  # (a stretch of a 1-D atlas is contiguous: every second element of an array of its own instead)
        views = [torch.full((2 * ext[0],), 77.0, dtype=atlas.dtype, device=DEV)[::2] for _, _, ext in items]
    st.request([it + (v,) for it, v in zip(items, views)])
    for outs in (ask(st, items), views):
        for i, t in enumerate(outs):
            r = to_bytes(*raw_points(t, caps[i], lo, hi, invert, nan))
            same_bytes((hg[32 * i:32 * i + 32], ig[i:i + 1], vg[i:i + 1]), r, "%s box %d (%s):" % (what, i, "contiguous" if t.is_contiguous() else "atlas"))
    assert any(not v.is_contiguous() for v in views), "strided views among them"


def quantile_ranges(full):
    """ranges from the field's own values: a band in the middle, the upper tail, everything, nothing (lo > hi)"""
    flat = np.sort(full.cpu().numpy().astype(np.float64).reshape(-1))
    flat = flat[np.isfinite(flat)]
    q = lambda f: float(flat[min(int(f * flat.size), flat.size - 1)])  # noqa: E731
    return [(q(0.45), q(0.55)), (q(0.9), float(flat[-1])), (float(flat[0]), float(flat[-1])), (q(0.6), q(0.4))]


def check_stream(st, full, items, what=""):
    """the quantile ranges over the items — the band, the upper tail inverted, everything (NaN too), nothing; every kind of box — no hit,
    some, all — must occur"""
    kinds = set()
    for j, (lo, hi) in enumerate(quantile_ranges(full)):
        invert, nan = [(False, False), (True, False), (False, True), (False, False)][j]
        caps, counts, got = check_select(st, full, items, lo, hi, invert, nan, what=what)
        sizes = [int(np.prod(it[2])) for it in items]
        kinds |= {"none" if c == 0 else "all" if c == n else "some" for c, n in zip(counts, sizes)}
        if j == 0:
            same_bytes(got, check_select(st, full, items, lo, hi, invert, nan, what=what + " a second call", caps=caps)[2], what + " a second call:")
            against_itself(st, items, caps, got, lo, hi, invert, nan, what)
            # the Python call: the same heads, the same first `written` entries
            res = st.select(items, lo, hi, caps, invert=invert, nan=nan)
            out = res.numpy()
            assert res.heads.cpu().numpy().tobytes() == got[0] and tuple(res.heads.shape) == (len(items), 4)
            for i, (c, ix, val) in enumerate(out):
                w = min(c, caps[i])
                assert c == counts[i] and ix.tobytes() == got[1][i][:8 * w] and val.tobytes() == got[2][i][:val.itemsize * w]
                assert tuple(res.index[i].shape) == (caps[i],) and res.value[i].dtype == getattr(torch, st.dtype.name)
    assert kinds == {"none", "some", "all"}, kinds
    check_select(st, full, items, *quantile_ranges(full)[1], values=False, what=what + " indices only")


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
            assert st.stats()["huffman_stages"] == (1 if fast else 0)


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
            check_stream(st, full, items, what=name)
            v = float(full[0, 0, 0])
            caps, counts, got = check_select(st, full, items, v, v, what=name, caps=[1, 5, 2, 0])
            assert counts[0] == 1 and counts[3] == 1
            alone = check_select(st, full, items[:1], v, v, what=name + " alone", caps=[1])[2]  # (no level runs at all)
            same_bytes((got[0][:32], got[1][:1], got[2][:1]), alone, "alone:")


@pytest.mark.parametrize("stock", [0, 1], ids=["id17", "stock"])
def test_spikes(stock):
    """raw records inside some boxes' windows and outside others': the spikes are what the upper range selects"""
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
            check_stream(st, ref, items, what=name)
            caps, counts, _ = check_select(st, ref, items, 1e6, 1e6, what=name + " the spikes")
            assert max(counts) > 0 and min(counts) == 0, "spikes inside some boxes and outside others"


def test_non_finite_points():
    """the reduce tests' NaN / +-Inf field under each of the four flag combinations; lo = hi = +Inf"""
    shape = (65, 47, 130)
    a = smooth(shape)
    for p, v in zip([(0, 0, 0), (8, 8, 16), (16, 24, 64), (33, 21, 77), (64, 40, 128)], [np.nan, np.inf, -np.inf, np.nan, np.inf]):
        a[p] = v
    conf = conf_for(shape)
    blob = container(a, conf)
    full, _ = sz3_amd.decompress(blob, np.float32, device=DEV)
    items = mixed(shape) + [(3, (1, 1, 2), (1, 1, 1)), (0, (0, 0, 0), (1, 1, 1)), (0, (0, 0, 0), (1, 1, 2))]
    dc, pl, size, pfull = device_payload(a, conf_for(shape))
    handles = [("open_stream", sz3_amd.open_stream(blob, np.float32, device=DEV), full),
               ("open_payload", dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream), pfull)]
    (qlo, qhi) = quantile_ranges(full)[0]
    for name, st, ref in handles:
        with st:
            for invert, nan in FLAGS:
                for lo, hi in [(qlo, qhi), (np.inf, np.inf), (-np.inf, -np.inf), (-np.inf, np.inf), (1.0, -1.0)]:
                    caps, counts, got = check_select(st, ref, items, lo, hi, invert, nan, what=name)
                if (invert, nan) == (False, True):  # (the last range, lo > hi: the NaNs alone)
                    nans = [int(np.isnan(s).sum()) for s in slices_of(ref, items)]
                    assert counts == nans and max(nans) > 0 and min(nans) == 0
            caps, counts, got = check_select(st, ref, items, np.inf, np.inf, what=name + " +Inf")
            assert sum(counts) > 0 and counts == [int(np.isposinf(s).sum()) for s in slices_of(ref, items)]
            against_itself(st, items, caps, got, np.inf, np.inf, what=name + " +Inf")
    dc.close()


# ---- 2. select_points on crafted tensors, no stream -------------------------------------------------------------------------------------------
def check_points(v, cap, lo, hi, invert=False, nan=False, values=True, t=None, what=""):
    """v: the numpy array of the values (its row-major order is the index order); t: the device tensor when it is a view"""
    t = torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if t is None else t
    heads, index, value = raw_points(t, cap, lo, hi, invert, nan, values)
    torch.cuda.synchronize()
    return check_box(heads.cpu().numpy()[0], index[0].cpu().numpy(), None if value is None else value[0].cpu().numpy(), v, cap, lo, hi, invert, nan, what)


def with_hits(total, hits, dtype=np.float32):
    v = np.full(total, -1.0, dtype=dtype)
    v[np.asarray(hits, dtype=np.int64)] = 1.0 + np.arange(len(hits)) / 1024.0  # (distinct values: a swapped pair shows)
    return v


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 * 4096, 3 * 4096 + 1])
def test_partition_edges(total, dtype):
    rng = np.random.default_rng(total)
    v = rng.normal(3.0, 2.0, total).astype(dtype)
    count = check_points(v, total, 2.0, 4.0, what="total %d" % total)
    for cap in sorted({0, 1, max(count - 1, 0), count, count + 1}):
        check_points(v, cap, 2.0, 4.0, what="total %d capacity %d" % (total, cap))
    check_points(v, total, 2.0, 4.0, invert=True, what="total %d inverted" % total)
    check_points(v, total, -1e30, 1e30, what="total %d, all points hit" % total)
    check_points(v, total, 100.0, 200.0, what="total %d, none hit" % total)
    # hits at the first and last index of a chunk, of a row of 256 and of a wave
    edges = sorted({i for c in range(0, total, CHUNK) for i in (c, c + 63, c + 64, c + 255, c + 256, c + CHUNK - 1) if i < total} | {total - 1})
    e = with_hits(total, edges, dtype)
    for cap in sorted({len(edges), len(edges) - 1, 1, 3}):
        assert check_points(e, cap, 0.0, 10.0, what="total %d, hits on the edges" % total) == len(edges)
    assert check_points(with_hits(total, [total - 1], dtype), 4, 0.0, 10.0, what="total %d, a lone hit at the end" % total) == 1
    res = sz3_amd.select_points(torch.from_numpy(e).to(DEV), 0.0, 10.0, len(edges) + 2)  # the Python call
    (c, ix, val), = res.numpy()
    assert c == len(edges) and ix.tolist() == edges and val.tobytes() == e[edges].tobytes() and tuple(res.heads.shape) == (1, 4)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_capacity_cuts(dtype):
    """all points hit (the rank is the index), then every second one: capacities inside a wave, between two waves, between two rows of 256 and
    exactly at a chunk boundary"""
    total = 3 * CHUNK + 1
    rng = np.random.default_rng(5)
    every = rng.normal(0.0, 1.0, total).astype(dtype)
    second = every.copy()
    second[1::2] = 50.0
    for cap in (37, 64, 100, 128, 256, 300, 512, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 64, total - 1, total, total + 1):
        assert check_points(every, cap, -40.0, 40.0, what="every point, capacity %d" % cap) == total
        check_points(second, cap // 2, -40.0, 40.0, what="every second point, capacity %d" % (cap // 2))
        check_points(second, cap // 2, -40.0, 40.0, values=False, what="every second point, indices only, capacity %d" % (cap // 2))


def test_crafted_values():
    z = np.zeros(5000, dtype=np.float64)  # -0.0 against lo = 0.0: equal, and the sign is kept in the value
    z[::2] = -0.0
    z[7::10] = -1.0
    assert check_points(z, 5000, 0.0, 0.0) == 4500
    assert check_points(z.astype(np.float32), 5000, 0.0, 1.0) == 4500
    assert check_points(z, 5000, -0.0, -0.0, invert=True) == 500
    f = np.full(300, np.float32(0.1), dtype=np.float32)  # the comparison is in double: 0.1f lies above the double 0.1
    f[::3] = 0.0
    up = float(np.float32(0.1))
    assert up > 0.1
    assert check_points(f, 300, 0.1, 1.0) == 200
    assert check_points(f, 300, up, 1.0) == 200
    assert check_points(f, 300, float(np.nextafter(up, 1.0)), 1.0) == 0
    assert check_points(f, 300, 0.0, 0.1) == 100
    n = np.arange(9000, dtype=np.float64)  # NaN payloads and signs are kept; NaN alone with lo > hi
    nans = np.array([0x7FF8000000000001, 0xFFF8000000000123, 0x7FF0000000000001], dtype=np.uint64).view(np.float64)
    n[[5, 4096, 8999]] = nans
    n[[6, 4097]] = [np.inf, -np.inf]
    for invert, nan in FLAGS:
        check_points(n, 9000, 1.0, 0.0, invert, nan)
        check_points(n, 9000, 100.0, 5000.0, invert, nan)
        check_points(n, 9000, -np.inf, np.inf, invert, nan)
    assert check_points(n, 9000, 1.0, 0.0, nan=True) == 3 and check_points(n, 9000, 1.0, 0.0) == 0
    assert check_points(n, 9000, np.inf, np.inf) == 1 and check_points(n, 9000, -np.inf, np.inf) == 8997
    n4 = np.arange(300, dtype=np.float32)
    n4[[3, 299]] = np.array([0x7FC00001, 0xFFC12345], dtype=np.uint32).view(np.float32)
    assert check_points(n4, 300, 1.0, 0.0, nan=True) == 2
    g = torch.from_numpy(np.random.default_rng(4).normal(1.0, 1.0, (7, 50, 66)).astype(np.float32)).to(DEV)
    v = g[:, 1:40, ::2]  # x stride 2, a step along y
    check_points(v.cpu().numpy(), 3000, 0.5, 1.5, t=v, what="x stride 2")
    b = g[0, 3].expand(9, 66)  # a stride-0 broadcast
    assert b.stride(0) == 0
    check_points(b.cpu().numpy(), 9 * 66, 0.5, 1.5, t=b, what="broadcast")
    q = torch.from_numpy(np.random.default_rng(5).normal(-2.0, 3.0, (5, 6, 7, 40)).astype(np.float64)).to(DEV)  # 4-D, a view of it
    for v in (q, q[1:, :, 2:6, 3:37]):
        check_points(v.cpu().numpy(), 2000, -3.0, 0.0, t=v, what="4-D")
        check_points(v.cpu().numpy(), 2000, -3.0, 0.0, invert=True, t=v, what="4-D")


def test_the_scan_carries_past_256_chunks():
    shape = (129, 96, 96)
    total = int(np.prod(shape))
    assert -(-total // CHUNK) == 291
    hits = sorted(c * CHUNK + o for c in (0, 255, 256, 290) for o in (0, 63, 64, 255, 256, 1000) if c * CHUNK + o < total) + [total - 1]
    v = with_hits(total, hits).reshape(shape)
    for cap in (len(hits), 7, 13, len(hits) - 1):
        assert check_points(v, cap, 0.0, 10.0, what="291 chunks, capacity %d" % cap) == len(hits)
    t = torch.from_numpy(np.random.default_rng(8).normal(0.0, 1.0, shape).astype(np.float32)).to(DEV)
    check_points(t.cpu().numpy(), total, 1.0, 5.0, t=t, what="291 chunks, a sixth of the points")
    check_points(t.cpu().numpy(), 1000, -5.0, 5.0, t=t, what="291 chunks, capacity 1000")


# ---- 3. position in the request, number of boxes, the chain ----------------------------------------------------------------------------------
def test_position_and_number_of_boxes(chain):
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
    flat = np.sort(slices_of(full, [target])[0].astype(np.float64).reshape(-1))  # (the target's own second quarter: about 3300 points)
    lo, hi = float(flat[flat.size // 4]), float(flat[flat.size // 2])
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        chain(0)
        caps, counts, alone = check_select(st, full, [target], lo, hi, caps=[4000])
        assert counts[0] > 0
        for place, others in [(0, many[:2]), (2, many[:2]), (5, mixed(shape)), (27, many[:27]), (255, many), (100, many)]:
            items = list(others[:place]) + [target] + list(others[place:])
            assert len(items) <= 256
            cs = [5] * len(items)
            cs[place] = 4000
            rc, heads, index, value = raw_select(st, items, cs, lo, hi)
            assert rc == 0
            h, ix, vv = to_bytes(heads, index, value)
            same_bytes(alone, (h[32 * place:32 * place + 32], ix[place:place + 1], vv[place:place + 1]), "%d boxes, place %d:" % (len(items), place))
        n0 = st.stats()["requests"]
        check_select(st, full, many + [target], lo, hi, what="256 boxes,")
        assert st.stats()["requests"] == n0 + 1
        chain(2048)
        same_bytes(alone, check_select(st, full, [target], lo, hi, caps=[4000])[2], "the chain at 2048:")
        assert st.stats()["chain_levels_last_request"] > 0


# ---- 4. fallback handles: three launches out of the resident array ---------------------------------------------------------------------------
def check_fallback(st, full, name):
    assert st.stats()["fast"] == 0
    check_stream(st, full, FB_ITEMS, what=name)
    st.select(FB_ITEMS, 0.0, 1.0, 16)
    s = st.stats()
    assert s["fast"] == 0 and s["launches_last_request"] == 3 and s["chain_levels_last_request"] == 0


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


# ---- 5. the launch count ---------------------------------------------------------------------------------------------------------------------
def test_launch_count(chain):
    shape = (65, 47, 130)
    kw = (("interpAlgo", 0),)
    a, blob, full, conf = case(shape, "float32", kw)
    lo, hi = quantile_ranges(full)[0]
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
                r = launches(lambda: st.select(items, lo, hi, 64))
                s = st.stats()
                assert r == q + 2, "a select is the request's launches plus two (%d, %d; threshold %d)" % (r, q, points)
                assert s["chain_levels_last_request"] == cq and s["chain_points"] == points
                counts.append(r)
            assert counts[0] == counts[1], "twelve boxes issue as many launches as three"
            assert points == 0 or st.stats()["chain_levels_last_request"] > 0, "one level at threshold 2048 takes the chain"
            items = mixed(shape)
            caps = caps_for(slices_of(full, items), lo, hi)
            with sz3_amd.debug_flags2(sz3_amd.Dbg2.REQUEST_BY_LEVEL):  # level group by level group: still plus two
                q = launches(lambda: ask(st, items))
                grouped = None

                def f():
                    nonlocal grouped
                    grouped = check_select(st, full, items, lo, hi, caps=caps, what="by level")[2]
                assert launches(f) == q + 2
            same_bytes(grouped, check_select(st, full, items, lo, hi, caps=caps)[2], "by level against merged:")
        check_select(st, full, twelve, lo, hi, what="threshold 2048,")


# ---- 6. ordering -----------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_and_two_streams():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    items = mixed(shape)
    x_items, y_items = items[:9], items[5:]
    lo, hi = quantile_ranges(full)[0]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        cx, _, want_x = check_select(st, full, x_items, lo, hi)
        cy, _, want_y = check_select(st, full, y_items, lo, hi)
        torch.cuda.synchronize()
        want_rx = st.reduce(x_items, 7, -0.5, 0.75).stats.cpu().numpy().tobytes()
        for _ in range(2):  # no host synchronisation in between
            bufs = [alloc(st, its) for its in (x_items, y_items)]
            torch.cuda.synchronize()
            r = [raw_select(st, x_items, cx, lo, hi), raw_select(st, y_items, cy, lo, hi)]
            x = ask(st, x_items, sync=False, outs=bufs[0])
            r.append(raw_select(st, x_items, cx, lo, hi, stream=s1))
            red = st.reduce(x_items, 7, -0.5, 0.75, stream=s2)
            r.append(raw_select(st, y_items, cy, lo, hi, stream=s2))
            y = ask(st, y_items, sync=False, stream=s1, outs=bufs[1])
            r.append(raw_select(st, x_items, cx, lo, hi, stream=s2))
            r.append(raw_select(st, y_items, cy, lo, hi))
            torch.cuda.synchronize()
            for got, want in zip(r, (want_x, want_y, want_x, want_y, want_x, want_y)):
                assert got[0] == 0
                same_bytes(to_bytes(*got[1:]), want, "back to back:")
            assert red.stats.cpu().numpy().tobytes() == want_rx
            same(x, full, x_items)
            same(y, full, y_items)
    # select_points on two streams shares the library's chunk records (and reduce_stats' partials): ordered by an event
    big = torch.from_numpy(np.random.default_rng(9).normal(0, 1, 300000).astype(np.float32)).to(DEV)
    small = big[:5000].clone()
    torch.cuda.synchronize()
    wb, ws = to_bytes(*raw_points(big, 50000, 0.5, 3.0)), to_bytes(*raw_points(small, 50000, 0.5, 3.0))
    wr = sz3_amd.reduce_stats(big).stats.cpu().numpy().tobytes()
    rs, reds = [], []
    for i in range(6):
        sx = (s1, s2)[i % 2] if i % 3 else None
        rs.append(raw_points(big if i % 2 == 0 else small, 50000, 0.5, 3.0, stream=sx))
        reds.append(sz3_amd.reduce_stats(big, stream=(s2, s1)[i % 2]))
    torch.cuda.synchronize()
    for i, got in enumerate(rs):
        same_bytes(to_bytes(*got), wb if i % 2 == 0 else ws, "select_points on two streams:")
        assert reds[i].stats.cpu().numpy().tobytes() == wr


# ---- 7. refusals on an open handle -----------------------------------------------------------------------------------------------------------
def refusals(st, full, good):
    N = len(good[0][1])
    n = len(good)
    before = st.stats()["requests"]
    einval = CODES["SZ3HIP_EINVAL"]
    caps = [16] * n
    heads = torch.full((n, 4), SENT, dtype=torch.int64, device=DEV)
    index, value = sentinels(caps, torch.float32)
    reqs = (sz3_amd._CSelectReq * 300)()
    arr, _ = sz3_amd._boxes(N, [it[1:] for it in good])
    opts = sz3_amd._CSelectOpts()

    def fill():
        for i, it in enumerate(good):
            reqs[i].level, reqs[i].reserved, reqs[i].box = it[0], 0, arr[i]
            reqs[i].d_index, reqs[i].d_value, reqs[i].capacity = index[i].data_ptr(), value[i].data_ptr(), caps[i]
        opts.lo, opts.hi, opts.flags, opts.reserved = -0.5, 0.75, 0, 0

    def call(cnt=n, d_heads=heads.data_ptr(), h=st._h, o=opts):
        rc = L.sz3hip_stream_select(h, reqs, cnt, C.byref(o) if o is not None else None, d_heads, torch.cuda.current_stream().cuda_stream)
        return rc, L.sz3hip_last_error().decode()

    for place in (0, 1, n - 1):
        at = "box %d: " % place
        fill()
        reqs[place].level = 31
        assert call() == (einval, at + "tile level 31 is outside 0 .. 30")
        fill()
        reqs[place].level = -1
        rc, msg = call()
        assert rc == einval and at in msg
        fill()
        reqs[place].level = 1
        reqs[place].box.lo[0], reqs[place].box.ext[0] = 30, 4
        rc, msg = call()
        assert rc == einval and at in msg and "dimension 0" in msg
        fill()
        reqs[place].box.ext[N - 1] = 0
        rc, msg = call()
        assert rc == einval and at in msg and "extent 0" in msg
        fill()
        reqs[place].reserved = 3
        assert call() == (einval, at + "the reserved word is 3, not 0")
        fill()
        reqs[place].d_index = None
        rc, msg = call()
        assert rc == einval and at in msg and "d_index is NULL" in msg
        fill()
        reqs[place].capacity = 0
        rc, msg = call()
        assert rc == einval and at in msg and "capacity of 0" in msg
        if place:
            fill()
            reqs[place].d_index = index[0].data_ptr() + 8 * 15
            rc, msg = call()
            assert rc == einval and msg.startswith("box %d: the output overlaps box 0's" % place), msg
            fill()
            reqs[place].d_value = value[0].data_ptr() + 4 * 15
            rc, msg = call()
            assert rc == einval and msg.startswith("box %d: the output overlaps box 0's" % place), msg
    for lo, hi, flags, reserved, word in [(np.nan, 1.0, 0, 0, "NaN"), (0.0, np.nan, 0, 0, "NaN"), (0.0, 1.0, 4, 0, "flags"), (0.0, 1.0, 0, 1, "reserved")]:
        fill()
        opts.lo, opts.hi, opts.flags, opts.reserved = lo, hi, flags, reserved
        rc, msg = call()
        assert rc == einval and word in msg, msg
    fill()
    assert call(o=None)[0] == einval and "opts" in call(o=None)[1]
    assert call(d_heads=None)[0] == einval and "d_heads" in call(d_heads=None)[1]
    assert call(0)[0] == einval and "1 .. 256 boxes" in call(0)[1]
    assert call(257)[0] == einval and "1 .. 256 boxes" in call(257)[1]
    assert call(h=None)[0] == einval and "no handle" in call(h=None)[1]
    torch.cuda.synchronize()
    assert bool((heads == SENT).all()) and all(bool((t == SENT).all()) for t in index) and all(bool((t.view(torch.uint8) == 0x4D).all()) for t in value), \
        "a refused select writes nothing"
    assert st.stats()["requests"] == before
    same(ask(st, good), full, good, "after the refusals,")
    # count > capacity is no error: the head says so, and the handle serves the next request
    lo, hi = float(full.min()), float(full.max())
    _, counts, _ = check_select(st, full, good, lo, hi, caps=[1] * n, what="every point against a capacity of 1")
    assert max(counts) > 1
    same(ask(st, good), full, good, "after count > capacity,")
    check_stream(st, full, good, what="after the refusals,")


def test_refusals():
    shape = (65, 47, 130)
    a, blob, full, conf = case(shape)
    good = [(k,) + tile_boxes(coarse_shape(shape, k))[j] for k, j in ((2, 2), (0, 4), (1, 3), (3, 0))]
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        refusals(st, full, good)
    with pytest.raises(sz3_amd.SZ3HipError) as e:  # a closed handle
        st.select(good, 0.0, 1.0, 4)
    assert e.value.code == CODES["SZ3HIP_EINVAL"] and "no handle" in str(e.value)
    with pytest.raises(TypeError):
        sz3_amd.select_points(np.zeros(4, dtype=np.float32), 0.0, 1.0, 4)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.select_points(torch.zeros(8, dtype=torch.int32, device=DEV), 0.0, 1.0, 4)
    assert e.value.code == CODES["SZ3HIP_EUNSUPPORTED"] and "integer element types are not supported yet" in str(e.value)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.select_points(torch.zeros(8, dtype=torch.float32, device=DEV), np.nan, 1.0, 4)
    assert e.value.code == CODES["SZ3HIP_EINVAL"]


def test_refusals_on_a_fallback_handle():
    shape = (40, 48, 56)
    blob = container(smooth(shape), conf_for(shape, **dict(FALLBACKS[0][1])))
    full, conf = sz3_amd.decompress(blob, np.float32, device=DEV)
    with sz3_amd.open_stream(blob, np.float32, device=DEV) as st:
        assert st.stats()["fast"] == 0
        refusals(st, full, FB_ITEMS[:4])

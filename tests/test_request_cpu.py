"""The opened stream's mixed-level request, without a GPU: the symbols, the two structs' layout against the header, the
plan — a pure host function — against the sums of the single boxes' tile plans, every refusal that comes before anything touches a device, the
accepted atlas views, and the Python names and signatures. Output pointers here are numbers: the plan never reads or writes them."""
import ctypes as C
import inspect
import os
import re

import pytest

import sz3_amd
from test_region_cpu import CODES

L = sz3_amd.lib()
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sz3hip.h")
SYMBOLS = ("sz3hip_stream_request", "sz3hip_request_plan_for")
SHAPES = [(65, 47, 130), (33, 70), (1000,), (9, 12, 17, 20)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
BASE = 1 << 40  # a made-up device address
EINVAL, EUNSUPPORTED = CODES["SZ3HIP_EINVAL"], CODES["SZ3HIP_EUNSUPPORTED"]


def err():
    return L.sz3hip_last_error().decode()


def coarse_shape(shape, k):
    return tuple(((d - 1) >> k) + 1 for d in shape)


def conf_for(shape, **kw):
    c = sz3_amd.Config(*shape)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def boxes_at(shape, k):
    """the whole coarse grid, a box with odd corners inside it, a single point"""
    cs = coarse_shape(shape, k)
    lo = tuple(min(d - 1, 1) for d in cs)
    return [((0,) * len(cs), cs), (lo, tuple(max(1, (d - a) // 2) for d, a in zip(cs, lo))), (tuple(d - 1 for d in cs), (1,) * len(cs))]


def reqs_of(items, N, esz=4):
    """items: (level, lo, shape[, ptr[, strides[, reserved]]]) -> the sz3hip_tile_req array; items without a pointer get contiguous outputs one
    after the other"""
    arr = (sz3_amd._CTileReq * max(len(items), 1))()
    at = BASE
    for i, it in enumerate(items):
        r = arr[i]
        r.level = it[0]
        r.box.lo[:N] = it[1]
        r.box.ext[:N] = it[2]
        n = 1
        for e in it[2]:
            n *= e
        if len(it) > 3 and it[3] is not None:
            r.d_out = it[3]
        else:
            r.d_out = at
            at += (n * esz + 255) & ~255
        if len(it) > 4 and it[4] is not None:
            r.strides[:N] = it[4]
        if len(it) > 5:
            r.reserved = it[5]
    return arr


def plan(conf, items, dtype=0, n=None):
    p = sz3_amd._CRequestPlan()
    rc = L.sz3hip_request_plan_for(C.byref(conf._c), dtype, reqs_of(items, conf.N, 4 if dtype == 0 else 8), len(items) if n is None else n, C.byref(p))
    return rc, p


def c_struct(name, txt):
    """the fields of a typedef'd struct of the header as (name, ctypes type), arrays included"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "sz3hip_box": sz3_amd._CBox, "void *": C.c_void_p}
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(void \*|\w+)\s*(.*)$", decl)
        t = ctype[m.group(1)]
        for var in m.group(2).split(","):
            a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", var)
            out.append((a.group(1), t * int(a.group(2)) if a.group(2) else t))
    return out


def test_symbols_exist():
    with open(HEADER) as f:
        txt = f.read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, txt), "%s is not declared in include/sz3hip.h" % sym


@pytest.mark.parametrize("name,cls,size", [("sz3hip_tile_req", "_CTileReq", 112), ("sz3hip_request_plan", "_CRequestPlan", 32)])
def test_struct_layout_matches_the_header(name, cls, size):
    with open(HEADER) as f:
        fields = c_struct(name, f.read())
    S = getattr(sz3_amd, cls)
    assert fields == list(S._fields_)
    assert C.sizeof(S) == size
    off = 0  # natural alignment, no hidden padding
    for n, t in S._fields_:
        assert getattr(S, n).offset == off, n
        off += C.sizeof(t)
    assert off == size


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plan_is_the_sum_of_the_tile_plans(shape, interp):
    conf = conf_for(shape, interpAlgo=interp)
    items = [(k, lo, ext) for k in (2, 0, 3, 1) for lo, ext in boxes_at(shape, k)]
    rc, p = plan(conf, items)
    assert rc == 0, err()
    singles = [sz3_amd.tile_plan(conf, k, lo, ext)["region"] for k, lo, ext in items]
    assert p.n == len(items) and p.finest_level == 0 and p.coarsest_level == 3
    assert p.points == sum(s["points"] for s in singles) and p.scratch_elems == sum(s["scratch_elems"] for s in singles)
    finest_whole = sz3_amd.tile_plan(conf, 0, (0,) * len(shape), shape)["region"]
    assert p.n_levels == finest_whole["n_levels"] == max(s["n_levels"] for s in singles) > 0
    # without the level-0 boxes the sequence is level 1's
    rc, p1 = plan(conf, [it for it in items if it[0] > 0])
    assert rc == 0 and p1.finest_level == 1 and p1.n_levels == sz3_amd.tile_plan(conf, 1, (0,) * len(shape), coarse_shape(shape, 1))["region"]["n_levels"]
    assert sz3_amd.request_plan(conf, "float32", items) == {k: getattr(p, k) for k, _ in sz3_amd._CRequestPlan._fields_}
    rc, p8 = plan(conf, items, dtype=1)
    assert rc == 0 and (p8.points, p8.scratch_elems, p8.n_levels) == (p.points, p.scratch_elems, p.n_levels)


def test_plan_with_anchors_aligns_by_array_level():
    """anchor stride 4: the boxes of levels 2 and 3 run no level at all (every grid point is an anchor), level 0 runs two, level 1 one"""
    shape = (65, 47, 130)
    conf = conf_for(shape, interpAnchorStride=4)
    per_level = [sz3_amd.tile_plan(conf, k, (0, 0, 0), coarse_shape(shape, k))["region"]["n_levels"] for k in range(4)]
    assert per_level == [2, 1, 0, 0]
    rc, p = plan(conf, [(k, (0, 0, 0), coarse_shape(shape, k)) for k in (2, 0, 3, 1)])
    assert rc == 0 and p.n_levels == 2


def test_refusals():
    shape = (65, 47, 130)
    conf = conf_for(shape)
    good = [(2, (0, 0, 0), (4, 4, 4)), (0, (1, 3, 5), (6, 5, 4)), (1, (0, 0, 0), (3, 3, 3))]
    assert plan(conf, good)[0] == 0
    out = sz3_amd._CRequestPlan()
    arr = reqs_of(good, 3)
    assert L.sz3hip_request_plan_for(None, 0, arr, 3, C.byref(out)) == EINVAL and "conf" in err()
    assert L.sz3hip_request_plan_for(C.byref(conf._c), 0, None, 3, C.byref(out)) == EINVAL and "NULL" in err()
    assert L.sz3hip_request_plan_for(C.byref(conf._c), 0, arr, 3, None) == EINVAL and "out" in err()
    assert plan(conf, good, n=0)[0] == EINVAL and "1 .. 256 boxes" in err()
    assert plan(conf, [good[0]] * 3, n=257)[0] == EINVAL and "1 .. 256 boxes" in err()
    for place in (0, 1, 2):
        bad = list(good)
        bad[place] = (31, (0, 0, 0), (1, 1, 1))
        assert plan(conf, bad)[0] == EINVAL and err() == "box %d: tile level 31 is outside 0 .. 30" % place
        bad[place] = (-1, (0, 0, 0), (1, 1, 1))
        assert plan(conf, bad)[0] == EINVAL and "box %d: " % place in err()
        bad[place] = (1, (30, 0, 0), (4, 4, 4))  # (33 coarse planes)
        assert plan(conf, bad)[0] == EINVAL and "box %d: " % place in err() and "leaves dimension 0 (extent 33)" in err()
        bad[place] = (3, (0, 0, 0), (9, 6, 18))  # (9 x 6 x 17 points at level 3)
        assert plan(conf, bad)[0] == EINVAL and "box %d: " % place in err() and "dimension 2" in err()
        bad[place] = (0, (0, 0, 0), (2, 0, 2))
        assert plan(conf, bad)[0] == EINVAL and "box %d: " % place in err() and "extent 0" in err()
        bad[place] = good[place] + (None, None, 7)
        assert plan(conf, bad)[0] == EINVAL and "box %d: " % place in err() and "reserved" in err()
    arr = reqs_of(good, 3)
    arr[1].d_out = None
    assert L.sz3hip_request_plan_for(C.byref(conf._c), 0, arr, 3, C.byref(out)) == EINVAL and err() == "box 1: the output array is NULL"
    for dt in range(2, 10):  # integer element types: the partial calls' code and wording
        assert plan(conf, good, dtype=dt)[0] == EUNSUPPORTED
        assert err() == "the region decode reads float / double arrays; integer element types are not supported yet"
    assert plan(conf, good, dtype=10)[0] == EUNSUPPORTED and "dataType" in err()
    assert plan(conf_for(shape, interpAnchorStride=24), good)[0] == EUNSUPPORTED and "power of two" in err()


def test_view_refusals():
    shape = (65, 47, 130)
    conf = conf_for(shape)
    box = (1, (0, 0, 0), (4, 5, 6))
    other = (0, (0, 0, 0), (2, 2, 2), BASE + (1 << 20))

    def one(strides, ext=(4, 5, 6)):
        return plan(conf, [other, (1, (0, 0, 0), ext, BASE, strides)])[0]

    assert one((30, 6, 1)) == 0 and one((1000, 100, 2)) == 0 and one((0, 0, 0)) == 0
    assert one((30, 6, -1)) == EINVAL and "box 1: " in err() and "dimension 2" in err() and "negative" in err()
    assert one((-30, 6, 1)) == EINVAL and "dimension 0" in err() and "negative" in err()
    assert one((30, 0, 1)) == EINVAL and "box 1: " in err() and "dimension 1" in err() and "zero" in err()
    assert one((30, 6, 0)) == EINVAL and "dimension 2" in err() and "zero" in err()
    assert one((1, 4, 20)) == EINVAL and "box 1: " in err() and "permuted" in err()  # (a transposed view)
    assert one((30, 5, 1)) == EINVAL and "permuted or overlap" in err()  # (rows of 6 elements 5 apart)
    assert one((29, 6, 1)) == EINVAL and "dimension 0" in err()
    # dimensions of extent 1 are ignored, whatever their strides say
    assert one((-7, 6, 1), ext=(1, 5, 6)) == 0 and one((0, 6, 1), ext=(1, 5, 6)) == 0 and one((30, -1, 1), ext=(4, 1, 6)) == 0
    assert one((6, 0, 1), ext=(4, 1, 6)) == 0 and one((5, 0, 1), ext=(4, 1, 6)) == EINVAL and "permuted or overlap" in err()
    # two contiguous outputs that overlap: today's rule
    a, b = (1, (0, 0, 0), (4, 5, 6), BASE), (0, (0, 0, 0), (2, 2, 2), BASE + 4 * 119)
    assert plan(conf, [a, b])[0] == EINVAL and err() == "box 1: the output overlaps box 0's, or cannot be shown not to"
    assert plan(conf, [a, (0, (0, 0, 0), (2, 2, 2), BASE + 4 * 120)])[0] == 0
    assert plan(conf, [a, box + (BASE,)])[0] == EINVAL and "overlaps box 0's" in err()  # (one array twice)
    assert plan(conf, [a, b], dtype=1)[0] == EINVAL and plan(conf, [a, (0, (0, 0, 0), (2, 2, 2), BASE + 4 * 120)], dtype=1)[0] == EINVAL  # (f64: twice the bytes)


def test_atlas_views():
    shape = (65, 47, 130)
    conf = conf_for(shape)
    W, H = 64, 40  # an atlas of 8 x 40 x 64 elements
    st = (H * W, W, 1)

    def at(z, y, x):
        return BASE + 4 * (z * H * W + y * W + x)

    def two(a, b):
        return plan(conf, [a, b])[0]

    left = (0, (0, 0, 0), (4, 10, 20), at(0, 0, 0), st)
    # side by side: the byte hulls interleave row by row, the rectangles do not meet
    assert two(left, (1, (1, 1, 1), (4, 10, 20), at(0, 0, 20), st)) == 0
    assert two((1, (1, 1, 1), (4, 10, 20), at(0, 0, 20), st), left) == 0
    assert two(left, (1, (0, 0, 0), (4, 10, 44), at(0, 0, 20), st)) == 0  # (to the row's end)
    assert two(left, (2, (0, 0, 0), (4, 12, 30), at(0, 10, 5), st)) == 0  # (below)
    assert two(left, (2, (0, 0, 0), (2, 12, 30), at(4, 3, 5), st)) == 0  # (behind)
    assert two((0, (0, 0, 0), (4, 10, 20), at(0, 12, 30), st), (1, (0, 0, 0), (4, 10, 20), at(0, 0, 5), st)) == 0  # (above and to the left)
    # (below and to the left: the origins' distance wraps around a row's end, the offsets are taken modulo the row)
    wrap = (0, (0, 0, 0), (4, 10, 20), at(0, 12, 30), st)
    assert two(wrap, (1, (0, 0, 0), (4, 10, 20), at(0, 14, 5), st)) == 0 and two(wrap, (1, (0, 0, 0), (4, 10, 26), at(0, 14, 5), st)) == EINVAL
    # ... and rectangles that meet, or run over the row's end into the next row
    for other in [(1, (0, 0, 0), (4, 10, 20), at(0, 0, 19), st), (1, (0, 0, 0), (4, 10, 20), at(0, 9, 19), st), (1, (0, 0, 0), (1, 1, 1), at(3, 9, 19), st),
                  (1, (0, 0, 0), (4, 10, 20), at(3, 9, 19), st), (1, (0, 0, 0), (4, 10, 45), at(0, 0, 20), st), (1, (0, 0, 0), (4, 10, 20), at(0, 35, 30), st)]:
        assert two(left, other) == EINVAL and err() == "box 1: the output overlaps box 0's, or cannot be shown not to", other
        assert two(other, left) == EINVAL and "box 1: the output overlaps box 0's" in err()
    # a third box is checked against both
    assert plan(conf, [left, (1, (1, 1, 1), (4, 10, 20), at(0, 0, 20), st), (2, (0, 0, 0), (4, 10, 20), at(0, 5, 30), st)])[0] == EINVAL and "box 2: the output overlaps box 1's" in err()
    # two views of different strides with meeting hulls cannot be shown apart
    assert two(left, (1, (0, 0, 0), (4, 10, 10), at(0, 0, 20), (H * W, W, 2))) == EINVAL and "cannot be shown not to" in err()
    assert two(left, (1, (0, 0, 0), (4, 10, 20), at(0, 0, 20), (H * W, 2 * W, 1))) == EINVAL
    # ... with disjoint hulls they are fine
    assert two(left, (1, (0, 0, 0), (4, 10, 10), at(4, 0, 0), (H * W, W, 2))) == 0
    # x stride 2: two tiles on the even elements side by side; one on the odd elements cannot be shown apart from one on the even ones
    st2 = (H * W, W, 2)
    a = (1, (0, 0, 0), (4, 10, 10), at(0, 0, 0), st2)
    assert two(a, (2, (0, 0, 0), (4, 10, 10), at(0, 0, 20), st2)) == 0 and two(a, (2, (0, 0, 0), (4, 10, 10), at(0, 0, 18), st2)) == EINVAL
    assert two(a, (2, (0, 0, 0), (4, 10, 10), at(0, 0, 1), st2)) == EINVAL and "cannot be shown not to" in err()
    # a 4-D atlas
    conf4 = conf_for((9, 12, 17, 20))
    s4 = (2 * 30 * 40, 30 * 40, 40, 1)
    a = (0, (0, 0, 0, 0), (2, 2, 10, 20), BASE, s4)
    assert plan(conf4, [a, (1, (0, 0, 0, 0), (2, 2, 9, 10), BASE + 4 * 20, s4)])[0] == 0
    assert plan(conf4, [a, (1, (0, 0, 0, 0), (2, 2, 9, 10), BASE + 4 * (10 * 40 + 3), s4)])[0] == 0
    assert plan(conf4, [a, (1, (0, 0, 0, 0), (2, 2, 9, 10), BASE + 4 * (9 * 40 + 3), s4)])[0] == EINVAL


def test_a_view_past_the_end_of_the_address_space():
    conf = conf_for((65, 47, 130))
    top = (1 << 64) - 64
    assert plan(conf, [(0, (0, 0, 0), (2, 2, 2), BASE), (1, (0, 0, 0), (4, 5, 6), top)])[0] == EINVAL and err() == "box 1: the view runs past the end of the address space"
    assert plan(conf, [(0, (0, 0, 0), (2, 2, 2), BASE), (1, (0, 0, 0), (4, 5, 6), top, (1 << 40, 1 << 20, 1))])[0] == EINVAL and "address space" in err()
    assert plan(conf, [(0, (0, 0, 0), (2, 2, 2), BASE), (1, (0, 0, 0), (1, 2, 4), top)])[0] == 0  # (32 bytes: they fit)


def test_request_plan_takes_the_items_of_stream_request():
    """(level, lo, shape[, out]): of a tensor the plan reads address and strides only — tensors in host memory serve"""
    torch = pytest.importorskip("torch")
    conf = conf_for((65, 47, 130))
    atlas = torch.zeros((8, 40, 64), dtype=torch.float32)
    left, right = atlas[:4, :10, :20], atlas[:4, :10, 20:40]
    items = [(0, (0, 0, 0), (4, 10, 20), left), (1, (1, 1, 1), (4, 10, 20), right), (2, (0, 0, 0), (3, 3, 3))]
    p = sz3_amd.request_plan(conf, "float32", items)
    assert p == sz3_amd.request_plan(conf, "float32", [it[:3] for it in items]) and p["n"] == 3 and p["coarsest_level"] == 2
    with pytest.raises(sz3_amd.SZ3HipError) as e:  # the rectangles meet
        sz3_amd.request_plan(conf, "float32", [items[0], (1, (1, 1, 1), (4, 10, 20), atlas[:4, :10, 19:39])])
    assert e.value.code == EINVAL and "box 1: the output overlaps box 0's" in str(e.value)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.request_plan(conf, "float32", [(1, (1, 1, 1), (4, 10, 20), torch.zeros((10, 4, 20), dtype=torch.float32).transpose(0, 1))])
    assert e.value.code == EINVAL and "permuted" in str(e.value)
    with pytest.raises(ValueError):
        sz3_amd.request_plan(conf, "float32", [(0, (0, 0, 0), (4, 10, 21), left)])
    with pytest.raises(ValueError):
        sz3_amd.request_plan(conf, "float64", [items[0]])
    with pytest.raises(ValueError):
        sz3_amd.request_plan(conf, "float32", [(0, (0, 0, 0), (4, 10, 20), 4096, (800, 20, 1))])


def test_request_refuses_a_null_handle():
    arr = reqs_of([(0, (0,), (1,))], 1)
    assert L.sz3hip_stream_request(None, arr, 1, None) == EINVAL and "no handle" in err()


def test_development_switch_is_listed():
    """the switch that sends a mixed request level group by level group: one bit of the second word, in the header and in sz3_amd.Dbg2"""
    with open(os.path.join(os.path.dirname(HEADER), "sz3hip_debug.h")) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"enum\s+sz3hip_dbg2\s*\{(.*?)\}", txt, flags=re.S).group(1)
    hdr = {m.group(1): int(m.group(2)) for m in re.finditer(r"SZ3HIP_DBG2_([A-Z0-9_]+)\s*=\s*(\d+)", body)}
    assert hdr == {name: int(v) for name, v in sz3_amd.Dbg2.__members__.items()} and hdr["REQUEST_BY_LEVEL"] == 2
    assert len(set(hdr.values())) == len(hdr) and all(v & (v - 1) == 0 for v in hdr.values())


def test_python_names_and_signatures():
    S = sz3_amd.Stream
    p = inspect.signature(S.request).parameters
    assert list(p) == ["self", "items", "stream"] and p["stream"].default is None
    assert list(inspect.signature(sz3_amd.request_plan).parameters) == ["conf", "dtype", "items"]
    for f in (S.tiles, S.tile, S.region, S.coarse):  # the convenience methods stay as they are
        q = inspect.signature(f).parameters
        assert q["out"].default is None and q["stream"].default is None

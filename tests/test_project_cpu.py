"""Boxes projected along an axis, without a GPU: the symbols and constants, the two structs' layout against the header,
the plan — a pure host function — against the request's plan, every refusal that comes before anything touches a device (the output overlap
on the COLLAPSED box in output elements among them), and the Python names and signatures. Output pointers here are numbers: the plan never
reads or writes them."""
import ctypes as C
import inspect
import re

import pytest

import sz3_amd
from test_map_cpu import c_struct
from test_request_cpu import BASE, EINVAL, EUNSUPPORTED, HEADER, IDS, SHAPES, boxes_at, conf_for, err, reqs_of

L = sz3_amd.lib()
SYMBOLS = ("sz3hip_stream_project", "sz3hip_project_plan_for", "sz3hip_project_device")
OPS = {"min": 0, "max": 1, "sum": 2, "mean": 3, "argmin": 4, "argmax": 5, "count": 6}
CONSTANTS = {"SZ3HIP_PROJECT_" + k.upper(): v for k, v in OPS.items()}
INDEX_OPS = ("argmin", "argmax", "count")
SHAPE = (65, 47, 130)
GOOD = [(0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6)), (2, (2, 1, 0), (3, 3, 8)), (0, (9, 9, 9), (1, 1, 1)), (3, (0, 0, 0), (2, 2, 2))]


def opts_of(op="max", axis=0, out_type=0, reserved=0, fill=float("nan")):
    o = sz3_amd._CProjectOpts()
    o.op = OPS[op] if isinstance(op, str) else op
    o.axis, o.out_type, o.reserved, o.fill = axis, out_type, reserved, fill
    return o


def out_bytes(op, out_type):
    return 4 if op in INDEX_OPS or out_type == 0 else 8


DEFAULT = object()


def plan(conf, items, dtype=0, n=None, opts=DEFAULT, esz=4):
    p = sz3_amd._CProjectPlan()
    o = opts_of() if opts is DEFAULT else opts
    rc = L.sz3hip_project_plan_for(C.byref(conf._c), dtype, reqs_of(items, conf.N, esz), len(items) if n is None else n, None if o is None else C.byref(o),
                                   C.byref(p))
    return rc, p


def refused(conf, items, fragment, code=EINVAL, **kw):
    rc, _ = plan(conf, items, **kw)
    assert rc == code and fragment in err(), (rc, err(), fragment)


def test_symbols_and_constants():
    with open(HEADER) as f:
        txt = f.read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, txt), "%s is not declared in include/sz3hip.h" % sym
    assert len(CONSTANTS) == 7
    for name, v in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%du\b" % (name, v), txt), name
    assert (sz3_amd.PROJECT_MIN, sz3_amd.PROJECT_MAX, sz3_amd.PROJECT_SUM, sz3_amd.PROJECT_MEAN, sz3_amd.PROJECT_ARGMIN, sz3_amd.PROJECT_ARGMAX,
            sz3_amd.PROJECT_COUNT) == (0, 1, 2, 3, 4, 5, 6)


@pytest.mark.parametrize("name,cls,size", [("sz3hip_project_opts", "_CProjectOpts", 24), ("sz3hip_project_plan", "_CProjectPlan", 48)])
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


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plan(shape, interp, dtype):
    conf = conf_for(shape, interpAlgo=interp)
    boxes = [(k, lo, ext) for k in (2, 0, 3, 1) for lo, ext in boxes_at(shape, k)]
    name = "float32" if dtype == 0 else "float64"
    want = sz3_amd.request_plan(conf, name, boxes)
    for axis in range(len(shape)):
        outs = 0
        for _, _, ext in boxes:
            n = 1
            for j, e in enumerate(ext):
                n *= 1 if j == axis else e
            outs += n
        for op in OPS:
            for out_type in ((0,) if op in INDEX_OPS else (0, 1)):
                rc, p = plan(conf, boxes, dtype=dtype, opts=opts_of(op, axis, out_type), esz=8)
                assert rc == 0, err()
                got = {k: getattr(p, k) for k, _ in sz3_amd._CProjectPlan._fields_}
                assert got == dict(want, out_points=outs, out_elem_bytes=out_bytes(op, out_type), reserved=0), (axis, op, out_type)
                got.pop("reserved")
                assert sz3_amd.project_plan(conf, name, boxes, op, axis, None if op in INDEX_OPS else ("float32", "float64")[out_type]) == got
        assert sz3_amd.project_plan(conf, name, boxes, "sum", axis)["out_elem_bytes"] == (4, 8)[dtype], "the handle's type is the default"


def test_refusals_of_the_options():
    conf = conf_for(SHAPE)
    refused(conf, GOOD, "NULL argument (opts)", opts=None)
    for bad in (7, 8, 255, 0xFFFFFFFF):
        refused(conf, GOOD, "op (%u)" % bad, opts=opts_of(bad))
    for bad in (3, 4, 0xFFFFFFFF):
        refused(conf, GOOD, "axis (%u)" % bad, opts=opts_of(axis=bad))
    refused(conf_for((33, 70)), [(0, (0, 0), (4, 5))], "axis (2)", opts=opts_of(axis=2))
    refused(conf_for((1000,)), [(0, (0,), (40,))], "axis (1)", opts=opts_of(axis=1))
    for bad in (2, 3, 9):
        refused(conf, GOOD, "out_type (%u)" % bad, opts=opts_of(out_type=bad))
    for op in INDEX_OPS:
        refused(conf, GOOD, "an index op", opts=opts_of(op, out_type=1))
        assert plan(conf, GOOD, opts=opts_of(op))[0] == 0, err()
    for bad in (1, 1 << 31):
        refused(conf, GOOD, "reserved word is %u" % bad, opts=opts_of(reserved=bad))
    for fill in (float("nan"), float("inf"), -0.0, 1e308):  # any double, not checked
        assert plan(conf, GOOD, opts=opts_of(fill=fill))[0] == 0, err()
    for op in OPS:
        for axis in range(3):
            assert plan(conf, GOOD, dtype=1, opts=opts_of(op, axis, 0 if op in INDEX_OPS else 1), esz=8)[0] == 0, err()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_refusals_of_the_boxes_and_views(axis):
    """sz3hip_stream_request's own, with its wording, on the collapsed box: each at the first, a middle and the last box"""
    conf = conf_for(SHAPE)
    n = len(GOOD)
    o = opts_of("sum", axis)
    o8 = opts_of("sum", axis, 1)
    refused(conf, [], "", n=0, opts=o)
    refused(conf, GOOD * 60, "", n=257, opts=o)
    for b in (0, n // 2, n - 1):
        def edit(item):
            items = list(GOOD)
            items[b] = item
            return items
        k, lo, ext = GOOD[b]
        flat = tuple(1 if j == axis else e for j, e in enumerate(ext))
        s1 = flat[2] + 1
        s0 = s1 * flat[1]
        good = (s0, s1, 1)
        assert plan(conf, edit((k, lo, ext, BASE + (1 << 30), good)), opts=o)[0] == 0, err()
        refused(conf, edit((31, lo, ext)), "box %d: " % b, opts=o)
        refused(conf, edit((k, (1 << 40, 0, 0), ext)), "box %d: " % b, opts=o)
        for j in range(3):  # an extent of 0, at the axis too
            refused(conf, edit((k, lo, tuple(0 if i == j else e for i, e in enumerate(ext)))), "box %d: " % b, opts=o)
        refused(conf, edit((k, lo, ext, None, None, 7)), "box %d: the reserved word is 7" % b, opts=o)
        for j in range(3):
            if flat[j] == 1:  # the stride at the axis, as that of any extent-1 dimension, is not read: garbage is accepted
                for junk in (-5, 0, 1 << 60, 3):
                    assert plan(conf, edit((k, lo, ext, BASE + (1 << 30), tuple(junk if i == j else v for i, v in enumerate(good)))), opts=o)[0] == 0, err()
                continue
            refused(conf, edit((k, lo, ext, BASE + (1 << 30), tuple(-v if i == j else v for i, v in enumerate(good)))),
                    "box %d: the view's stride of dimension %d is negative" % (b, j), opts=o)
            refused(conf, edit((k, lo, ext, BASE + (1 << 30), tuple(0 if i == j else v for i, v in enumerate(good)))),
                    "box %d: the view's stride of dimension %d is zero" % (b, j), opts=o)
        counted = [j for j in range(3) if flat[j] > 1]
        if len(counted) == 2:
            swapped = list(good)
            swapped[counted[0]], swapped[counted[1]] = good[counted[1]], good[counted[0]]
            refused(conf, edit((k, lo, ext, BASE + (1 << 30), tuple(swapped))), "box %d: the view's strides are permuted or overlap" % b, opts=o)
        # an output not aligned to its element: 4 bytes (float, uint32_t) and 8 (double)
        for off in (1, 2, 3):
            for oo in (o, opts_of("argmax", axis), opts_of("count", axis)):
                refused(conf, edit((k, lo, ext, BASE + (1 << 30) + off)), "box %d: the output is not aligned to its element size (4 bytes)" % b, opts=oo)
        for off in (1, 4, 7):
            refused(conf, edit((k, lo, ext, BASE + (1 << 30) + off)), "box %d: the output is not aligned to its element size (8 bytes)" % b, opts=o8)
        assert plan(conf, edit((k, lo, ext, BASE + (1 << 30) + 4)), dtype=1, opts=o)[0] == 0, "an f64 handle's f32 output is aligned to 4 bytes"
        arr = reqs_of(edit((k, lo, ext)), 3)
        arr[b].d_out = None
        p = sz3_amd._CProjectPlan()
        assert L.sz3hip_project_plan_for(C.byref(conf._c), 0, arr, n, C.byref(o), C.byref(p)) == EINVAL and "box %d: the output array is NULL" % b in err()


def test_index_ops_refuse_an_extent_beyond_uint32():
    conf = conf_for(((1 << 32) + 8,))
    box = [(0, (0,), ((1 << 32),))]
    for op in ("argmin", "argmax", "count"):
        refused(conf, box, "box 0: the extent along the axis (4294967296)", opts=opts_of(op))
        assert plan(conf, [(0, (0,), ((1 << 32) - 1,))], opts=opts_of(op))[0] == 0, err()
    assert plan(conf, box, opts=opts_of("max"))[0] == 0, err()


@pytest.mark.parametrize("out_type", [0, 1], ids=["4B", "8B"])
def test_output_overlap_is_counted_on_the_collapsed_box(out_type):
    conf = conf_for(SHAPE)
    e = 4 << out_type
    a, b = (0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6))
    at = BASE + (1 << 20)
    for axis, outs in ((0, 30), (1, 24), (2, 20)):
        opts = opts_of("mean", axis, out_type)
        # contiguous outputs of `outs` elements: the second may start right behind the first's last element, and not one element earlier
        assert plan(conf, [a + (at,), b + (at + outs * e,)], opts=opts)[0] == 0, err()
        refused(conf, [a + (at,), b + (at + outs * e - e,)], "box 1: the output overlaps box 0's", opts=opts)
        refused(conf, [b + (at + outs * e - e,), a + (at,)], "box 1: the output overlaps box 0's", opts=opts)
        # (the whole boxes' hulls, 120 elements, would overlap here: the collapsed box is the one laid out)
        p = sz3_amd._CRequestPlan()
        assert L.sz3hip_request_plan_for(C.byref(conf._c), 0, reqs_of([a + (at,), b + (at + outs * 4,)], 3), 2, C.byref(p)) == EINVAL
    # rectangles of one atlas of pitch 13 (axis 0 folded: 5 x 6 images): side by side along x they are shown apart; one column closer they meet
    opts = opts_of("max", 0, out_type)
    st = (5 * 13, 13, 1)
    assert plan(conf, [a + (at, st), b + (at + 6 * e, st)], opts=opts)[0] == 0, err()
    refused(conf, [a + (at, st), b + (at + 5 * e, st)], "box 1: the output overlaps box 0's", opts=opts)
    # two boxes that differ only along the axis share their output: refused. Repeated BOXES into outputs apart are allowed
    for axis in range(3):
        lo2 = tuple(4 if j == axis else 0 for j in range(3))
        refused(conf, [a + (at,), (0, lo2, (4, 5, 6), at)], "box 1: the output overlaps box 0's", opts=opts_of("sum", axis, out_type))
        refused(conf, [a + (at, st), (0, lo2, (4, 5, 6), at, st)], "box 1: the output overlaps box 0's", opts=opts_of("sum", axis, out_type))
    assert plan(conf, [a + (at,), a + (at + 30 * e,)], opts=opts)[0] == 0, err()


def test_integer_types_and_null_arguments():
    conf = conf_for(SHAPE)
    for dt in range(2, 10):
        rc, _ = plan(conf, GOOD, dtype=dt)
        assert rc == EUNSUPPORTED and "integer element types are not supported yet" in err()
    refused(conf, GOOD, "dataType", code=EUNSUPPORTED, dtype=10)
    p = sz3_amd._CProjectPlan()
    o = opts_of()
    arr = reqs_of(GOOD, 3)
    assert L.sz3hip_project_plan_for(None, 0, arr, len(GOOD), C.byref(o), C.byref(p)) == EINVAL and "NULL argument (conf)" in err()
    assert L.sz3hip_project_plan_for(C.byref(conf._c), 0, arr, len(GOOD), C.byref(o), None) == EINVAL and "NULL argument (out)" in err()
    assert L.sz3hip_project_plan_for(C.byref(conf._c), 0, None, len(GOOD), C.byref(o), C.byref(p)) == EINVAL
    assert L.sz3hip_stream_project(None, arr, len(GOOD), C.byref(o), None) == EINVAL and "no handle" in err()
    dims = (C.c_uint64 * 1)(8)
    for dt in range(2, 10):  # sz3hip_project_device refuses integers before it looks at a pointer
        assert L.sz3hip_project_device(dt, 1, dims, BASE, None, C.byref(o), BASE + 4096, None, None) == EUNSUPPORTED
        assert "integer element types are not supported yet" in err()
    assert L.sz3hip_project_device(0, 5, dims, BASE, None, C.byref(o), BASE + 4096, None, None) == EINVAL and "dimension count" in err()
    assert L.sz3hip_project_device(0, 1, dims, BASE, None, C.byref(o), None, None, None) == EINVAL and "d_out" in err()
    assert L.sz3hip_project_device(0, 1, dims, BASE, None, None, BASE + 4096, None, None) == EINVAL and "opts" in err()
    for bad in (opts_of(7), opts_of(axis=1), opts_of(out_type=2), opts_of("count", out_type=1), opts_of(reserved=1)):
        assert L.sz3hip_project_device(0, 1, dims, BASE, None, C.byref(bad), BASE + 4096, None, None) == EINVAL, "the options come before any pointer"


def test_python_names_and_signatures():
    p = inspect.signature(sz3_amd.Stream.project).parameters
    assert list(p) == ["self", "items", "op", "axis", "out_dtype", "fill", "stream"]
    assert p["out_dtype"].default is None and p["fill"].default != p["fill"].default and p["stream"].default is None
    p = inspect.signature(sz3_amd.project_plan).parameters
    assert list(p) == ["conf", "dtype", "items", "op", "axis", "out_dtype"] and p["out_dtype"].default is None
    p = inspect.signature(sz3_amd.project_points).parameters
    assert list(p) == ["tensor", "op", "axis", "out_dtype", "fill", "out", "stream"]
    assert p["out_dtype"].default is None and p["fill"].default != p["fill"].default and p["out"].default is None and p["stream"].default is None
    conf = conf_for(SHAPE)
    for name in OPS:
        for spelled in (name, name.upper()):
            got = sz3_amd.project_plan(conf, "float64", GOOD, spelled, -1)
            assert got["out_elem_bytes"] == (4 if name in INDEX_OPS else 8) and got["n"] == len(GOOD)
            assert got["out_points"] == 4 * 5 + 4 * 5 + 3 * 3 + 1 + 2 * 2, "axis -1 is the last one"
    with pytest.raises(ValueError):
        sz3_amd.project_plan(conf, "float32", GOOD, "median", 0)
    with pytest.raises(ValueError):
        sz3_amd.project_plan(conf, "float32", GOOD, "max", 3)
    with pytest.raises(ValueError):
        sz3_amd.project_plan(conf, "float32", GOOD, "argmax", 0, "float32")
    with pytest.raises(ValueError):
        sz3_amd.project_plan(conf, "float32", GOOD, "max", 0, "float16")
    with pytest.raises(ValueError):
        sz3_amd.project_plan(conf, "float32", [(0, (0, 0, 0))], "max", 0)
    with pytest.raises(TypeError):
        sz3_amd.project_points([1.0, 2.0], "max", 0)

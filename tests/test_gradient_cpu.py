"""Gradients of boxes, without a GPU: the symbols and constants, the two structs' layout against the header, the plan —
a pure host function — against the request's plan, every refusal that comes before anything touches a device (the spacing, INTERIOR's
extents and the output overlap on the OUTPUT box in output elements among them), the Python names and signatures, and the tests' numpy model
against numpy's own gradient where both are exact. Output pointers here are numbers: the plan never reads or writes them."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import gradient_model as gm
import sz3_amd
from test_request_cpu import BASE, EINVAL, EUNSUPPORTED, HEADER, IDS, SHAPES, boxes_at, conf_for, err, reqs_of

L = sz3_amd.lib()
SYMBOLS = ("sz3hip_stream_gradient", "sz3hip_gradient_plan_for", "sz3hip_gradient_device")
OPS = gm.OPS
CONSTANTS = dict({"SZ3HIP_GRADIENT_" + k.upper(): v for k, v in OPS.items()}, SZ3HIP_GRADIENT_INTERIOR=1)
SHAPE = (65, 47, 130)
GOOD = [(0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6)), (2, (2, 1, 0), (3, 3, 8)), (0, (9, 9, 9), (1, 1, 1)), (3, (0, 0, 0), (2, 2, 2))]
WIDE = [(0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6)), (2, (2, 1, 0), (3, 3, 8)), (0, (9, 9, 9), (3, 4, 3)), (3, (0, 0, 0), (5, 3, 3))]


def opts_of(op="deriv", axis=0, out_type=0, flags=0, spacing=(1.0, 1.0, 1.0, 1.0)):
    o = sz3_amd._CGradientOpts()
    o.op = OPS[op] if isinstance(op, str) else op
    o.axis, o.out_type, o.flags = axis, out_type, flags
    o.spacing[:len(spacing)] = spacing
    return o


def c_struct(name, txt):
    """the fields of a typedef'd struct of the header as (name, ctypes type), arrays of scalars included"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "double": C.c_double}
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(\w+)\s*(.*)$", decl)
        for var in m.group(2).split(","):
            a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", var)
            out.append((a.group(1), ctype[m.group(1)] * int(a.group(2)) if a.group(2) else ctype[m.group(1)]))
    return out


DEFAULT = object()


def plan(conf, items, dtype=0, n=None, opts=DEFAULT, esz=4):
    p = sz3_amd._CGradientPlan()
    o = opts_of() if opts is DEFAULT else opts
    rc = L.sz3hip_gradient_plan_for(C.byref(conf._c), dtype, reqs_of(items, conf.N, esz), len(items) if n is None else n, None if o is None else C.byref(o),
                                    C.byref(p))
    return rc, p


def refused(conf, items, fragment, code=EINVAL, **kw):
    rc, p = plan(conf, items, **kw)
    assert rc == code and fragment in err(), (rc, err(), fragment)


def test_symbols_and_constants():
    with open(HEADER) as f:
        txt = f.read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, txt), "%s is not declared in include/sz3hip.h" % sym
    assert len(CONSTANTS) == 5
    for name, v in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%du\b" % (name, v), txt), name
    assert (sz3_amd.GRADIENT_DERIV, sz3_amd.GRADIENT_MAG2, sz3_amd.GRADIENT_MAG, sz3_amd.GRADIENT_VECTOR, sz3_amd.GRADIENT_INTERIOR) == (0, 1, 2, 3, 1)


@pytest.mark.parametrize("name,cls,size", [("sz3hip_gradient_opts", "_CGradientOpts", 48), ("sz3hip_gradient_plan", "_CGradientPlan", 48)])
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
    N = len(shape)
    every = [(k, lo, ext) for k in (2, 0, 3, 1) for lo, ext in boxes_at(shape, k)]
    name = "float32" if dtype == 0 else "float64"
    spacing = (0.5, 1.25, 3.0, 7.0)[:N]
    for op in OPS:
        for axis in (range(N) if op == "deriv" else (0,)):
            for interior in (False, True):
                axes = gm.differentiated(op, axis, N)
                boxes = [b for b in every if not interior or all(b[2][j] >= 3 for j in axes)]
                assert {b[0] for b in boxes} >= {0, 1} and len(boxes) >= 2
                want = sz3_amd.request_plan(conf, name, boxes)
                outs = sum(int(np.prod(gm.out_shape(b[2], op, axis, interior))) for b in boxes)
                for out_type in (0, 1):
                    rc, p = plan(conf, boxes, dtype=dtype, opts=opts_of(op, axis, out_type, int(interior), spacing), esz=8 * N)
                    assert rc == 0, err()
                    got = {k: getattr(p, k) for k, _ in sz3_amd._CGradientPlan._fields_}
                    elem = (4, 8)[out_type] * (N if op == "vector" else 1)
                    assert got == dict(want, out_points=outs, out_elem_bytes=elem, reserved=0), (op, axis, interior, out_type)
                    got.pop("reserved")
                    assert sz3_amd.gradient_plan(conf, name, boxes, op, axis, spacing, ("float32", "float64")[out_type], interior) == got
    assert sz3_amd.gradient_plan(conf, name, every, "mag")["out_elem_bytes"] == (4, 8)[dtype], "the handle's type is the default"
    assert {b[0] for b in every} == {0, 1, 2, 3}, "levels 0 - 3 in one request"


def test_refusals_of_the_options():
    conf = conf_for(SHAPE)
    refused(conf, GOOD, "NULL argument (opts)", opts=None)
    for bad in (4, 5, 255, 0xFFFFFFFF):
        refused(conf, GOOD, "op (%u)" % bad, opts=opts_of(bad))
    for bad in (3, 4, 0xFFFFFFFF):
        refused(conf, GOOD, "axis (%u)" % bad, opts=opts_of(axis=bad))
    refused(conf_for((33, 70)), [(0, (0, 0), (4, 5))], "axis (2)", opts=opts_of(axis=2))
    refused(conf_for((1000,)), [(0, (0,), (40,))], "axis (1)", opts=opts_of(axis=1))
    for op in ("mag2", "mag", "vector"):
        for bad in (1, 2, 7):
            refused(conf, GOOD, "axis is %u" % bad, opts=opts_of(op, axis=bad))
        assert plan(conf, GOOD, opts=opts_of(op), esz=32)[0] == 0, err()
    for bad in (2, 3, 9):
        refused(conf, GOOD, "out_type (%u)" % bad, opts=opts_of(out_type=bad))
    for bad in (2, 3, 1 << 31, 0xFFFFFFFE):
        refused(conf, GOOD, "flags (0x%x)" % bad, opts=opts_of(flags=bad))
    for op in OPS:
        for axis in (range(3) if op == "deriv" else (0,)):
            for out_type in (0, 1):
                assert plan(conf, GOOD, dtype=1, opts=opts_of(op, axis, out_type), esz=32)[0] == 0, err()


def test_refusals_of_the_spacing():
    conf = conf_for(SHAPE)
    for a in range(3):
        for bad in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            sp = [1.0, 2.0, 0.5, 1.0]
            sp[a] = bad
            for op in OPS:
                refused(conf, GOOD, "spacing[%d]" % a, opts=opts_of(op, spacing=sp))
    # entries at and beyond N are not read
    for junk in (0.0, -3.0, float("nan"), float("inf")):
        assert plan(conf, GOOD, opts=opts_of(spacing=(1.0, 1.0, 1.0, junk)))[0] == 0, err()
        assert plan(conf_for((33, 70)), [(0, (0, 0), (4, 5))], opts=opts_of(spacing=(1.0, 1.0, junk, junk)))[0] == 0, err()
        assert plan(conf_for((1000,)), [(1, (0,), (40,))], opts=opts_of(spacing=(2.0, junk, junk, junk)))[0] == 0, err()
    # the grid step of a box: spacing * 2^level must stay finite — 1e308 holds at level 0 and leaves the doubles at level 4
    big = conf_for((70, 70, 70))
    for a in range(3):
        sp = [1.0, 1.0, 1.0]
        sp[a] = 1e308
        box4 = (4, (0, 0, 0), (3, 3, 3))
        assert plan(big, [(0, (0, 0, 0), (3, 3, 3))] * 3, opts=opts_of(spacing=sp))[0] == 0, err()
        for b in (0, 1, 2):
            items = [(0, (0, 0, 0), (3, 3, 3))] * 3
            items[b] = box4
            refused(big, items, "box %d: the grid step of dimension %d" % (b, a), opts=opts_of(spacing=sp))
    assert plan(big, [(4, (0, 0, 0), (3, 3, 3))], opts=opts_of(spacing=(1e307, 1e307, 1e307)))[0] == 0, "1e307 * 16 is finite"
    # denormal spacings are finite and above 0
    assert plan(conf, GOOD, opts=opts_of(spacing=(5e-324, 1.0, 1.0)))[0] == 0, err()


def test_interior_needs_three_points_along_a_differentiated_axis():
    conf = conf_for(SHAPE)
    n = len(WIDE)
    for b in (0, n // 2, n - 1):
        k, lo, ext = WIDE[b]
        for j in range(3):
            for e in (1, 2, 3):
                items = list(WIDE)
                items[b] = (k, lo, tuple(e if i == j else v for i, v in enumerate(ext)))
                for op in OPS:
                    for axis in (range(3) if op == "deriv" else (0,)):
                        o = opts_of(op, axis, flags=1)
                        if e < 3 and j in gm.differentiated(op, axis, 3):
                            refused(conf, items, "box %d: the extent of dimension %d is %d" % (b, j, e), opts=o, esz=32)
                        else:
                            rc, p = plan(conf, items, opts=o, esz=32)
                            assert rc == 0, err()
                            assert p.out_points == sum(int(np.prod(gm.out_shape(it[2], op, axis, True))) for it in items)
                        assert plan(conf, items, opts=opts_of(op, axis), esz=32)[0] == 0, "without INTERIOR any extent is served"
    # extent 3 leaves ONE point
    rc, p = plan(conf, [(0, (0, 0, 0), (3, 3, 3))], opts=opts_of("mag", flags=1))
    assert rc == 0 and p.out_points == 1


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_refusals_of_the_boxes_and_views(axis):
    """sz3hip_stream_request's own, with its wording, on the output box: each at the first, a middle and the last box"""
    conf = conf_for(SHAPE)
    n = len(GOOD)
    o = opts_of("deriv", axis)
    o8 = opts_of("deriv", axis, 1)
    refused(conf, [], "", n=0, opts=o)
    refused(conf, GOOD * 60, "", n=257, opts=o)
    for b in (0, n // 2, n - 1):
        def edit(item):
            items = list(GOOD)
            items[b] = item
            return items
        k, lo, ext = GOOD[b]
        s1 = ext[2] + 1
        s0 = s1 * ext[1]
        good = (s0, s1, 1)
        assert plan(conf, edit((k, lo, ext, BASE + (1 << 30), good)), opts=o)[0] == 0, err()
        refused(conf, edit((31, lo, ext)), "box %d: " % b, opts=o)
        refused(conf, edit((k, (1 << 40, 0, 0), ext)), "box %d: " % b, opts=o)
        for j in range(3):
            refused(conf, edit((k, lo, tuple(0 if i == j else e for i, e in enumerate(ext)))), "box %d: " % b, opts=o)
        refused(conf, edit((k, lo, ext, None, None, 7)), "box %d: the reserved word is 7" % b, opts=o)
        for j in range(3):
            if ext[j] == 1:
                continue
            refused(conf, edit((k, lo, ext, BASE + (1 << 30), tuple(-v if i == j else v for i, v in enumerate(good)))),
                    "box %d: the view's stride of dimension %d is negative" % (b, j), opts=o)
            refused(conf, edit((k, lo, ext, BASE + (1 << 30), tuple(0 if i == j else v for i, v in enumerate(good)))),
                    "box %d: the view's stride of dimension %d is zero" % (b, j), opts=o)
        if all(e > 1 for e in ext):
            refused(conf, edit((k, lo, ext, BASE + (1 << 30), (1, s1, s0))), "box %d: the view's strides are permuted or overlap" % b, opts=o)
        # an output not aligned to sizeof(Tout): 4 bytes and 8, for VECTOR's N-fold element too
        for off in (1, 2, 3):
            for oo in (o, opts_of("mag"), opts_of("vector")):
                refused(conf, edit((k, lo, ext, BASE + (1 << 30) + off)), "box %d: the output is not aligned to its element size (4 bytes)" % b, opts=oo)
        for off in (1, 4, 7):
            for oo in (o8, opts_of("vector", out_type=1)):
                refused(conf, edit((k, lo, ext, BASE + (1 << 30) + off)), "box %d: the output is not aligned to its element size (8 bytes)" % b, opts=oo)
        assert plan(conf, edit((k, lo, ext, BASE + (1 << 30) + 4)), dtype=1, opts=o)[0] == 0, "an f64 handle's f32 output is aligned to 4 bytes"
        assert plan(conf, edit((k, lo, ext, BASE + (1 << 30) + 4)), opts=opts_of("vector"), esz=32)[0] == 0, "a vector element of 12 bytes is aligned to 4"
        arr = reqs_of(edit((k, lo, ext)), 3)
        arr[b].d_out = None
        p = sz3_amd._CGradientPlan()
        assert L.sz3hip_gradient_plan_for(C.byref(conf._c), 0, arr, n, C.byref(o), C.byref(p)) == EINVAL and "box %d: the output array is NULL" % b in err()


@pytest.mark.parametrize("op,out_type", [("deriv", 0), ("deriv", 1), ("mag", 0), ("mag2", 1), ("vector", 0), ("vector", 1)])
def test_output_overlap_is_counted_in_output_elements(op, out_type):
    conf = conf_for(SHAPE)
    e = (4 << out_type) * (3 if op == "vector" else 1)  # the output element's bytes
    a, b = (0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6))
    at = BASE + (1 << 20)
    for interior in (0, 1):
        opts = opts_of(op, 1 if op == "deriv" else 0, out_type, interior)
        outs = int(np.prod(gm.out_shape((4, 5, 6), op, 1, bool(interior))))
        # contiguous outputs of `outs` elements: the second may start right behind the first's last element, and not one element earlier
        assert plan(conf, [a + (at,), b + (at + outs * e,)], opts=opts)[0] == 0, err()
        refused(conf, [a + (at,), b + (at + outs * e - e,)], "box 1: the output overlaps box 0's", opts=opts)
        refused(conf, [b + (at + outs * e - e,), a + (at,)], "box 1: the output overlaps box 0's", opts=opts)
    # rectangles of one atlas of pitch 13 (4 x 5 x 6 boxes): side by side along x they are shown apart; one column closer they meet
    opts = opts_of(op, 0, out_type)
    st = (5 * 13, 13, 1)
    assert plan(conf, [a + (at, st), b + (at + 6 * e, st)], opts=opts)[0] == 0, err()
    refused(conf, [a + (at, st), b + (at + 5 * e, st)], "box 1: the output overlaps box 0's", opts=opts)
    # under INTERIOR the rectangles are the trimmed boxes': (2 x 3 x 4) for the ops over every axis — four columns apart is enough then
    if op != "deriv":
        opts = opts_of(op, 0, out_type, 1)
        assert plan(conf, [a + (at, st), b + (at + 4 * e, st)], opts=opts)[0] == 0, err()
        refused(conf, [a + (at, st), b + (at + 3 * e, st)], "box 1: the output overlaps box 0's", opts=opts)
    # repeated boxes into outputs apart are allowed; into one output they are refused
    assert plan(conf, [a + (at,), a + (at + 120 * e,)], opts=opts_of(op, 0, out_type))[0] == 0, err()
    refused(conf, [a + (at,), a + (at,)], "box 1: the output overlaps box 0's", opts=opts_of(op, 0, out_type))


def test_integer_types_and_null_arguments():
    conf = conf_for(SHAPE)
    for dt in range(2, 10):
        rc, _ = plan(conf, GOOD, dtype=dt)
        assert rc == EUNSUPPORTED and "integer element types are not supported yet" in err()
    refused(conf, GOOD, "dataType", code=EUNSUPPORTED, dtype=10)
    p = sz3_amd._CGradientPlan()
    o = opts_of()
    arr = reqs_of(GOOD, 3)
    assert L.sz3hip_gradient_plan_for(None, 0, arr, len(GOOD), C.byref(o), C.byref(p)) == EINVAL and "NULL argument (conf)" in err()
    assert L.sz3hip_gradient_plan_for(C.byref(conf._c), 0, arr, len(GOOD), C.byref(o), None) == EINVAL and "NULL argument (out)" in err()
    assert L.sz3hip_gradient_plan_for(C.byref(conf._c), 0, None, len(GOOD), C.byref(o), C.byref(p)) == EINVAL
    assert L.sz3hip_stream_gradient(None, arr, len(GOOD), C.byref(o), None) == EINVAL and "no handle" in err()
    dims = (C.c_uint64 * 1)(8)
    for dt in range(2, 10):  # sz3hip_gradient_device refuses integers before it looks at a pointer
        assert L.sz3hip_gradient_device(dt, 1, dims, BASE, None, C.byref(o), BASE + 4096, None, None) == EUNSUPPORTED
        assert "integer element types are not supported yet" in err()
    assert L.sz3hip_gradient_device(0, 5, dims, BASE, None, C.byref(o), BASE + 4096, None, None) == EINVAL and "dimension count" in err()
    assert L.sz3hip_gradient_device(0, 1, dims, BASE, None, C.byref(o), None, None, None) == EINVAL and "d_out" in err()
    assert L.sz3hip_gradient_device(0, 1, dims, BASE, None, None, BASE + 4096, None, None) == EINVAL and "opts" in err()
    for bad in (opts_of(4), opts_of(axis=1), opts_of("mag", axis=1), opts_of(out_type=2), opts_of(flags=2), opts_of(spacing=(0.0,)),
                opts_of(spacing=(float("nan"),))):
        assert L.sz3hip_gradient_device(0, 1, dims, None, None, C.byref(bad), None, None, None) == EINVAL, "the options come before any pointer"
        assert "options" in err()


def test_python_names_and_signatures():
    p = inspect.signature(sz3_amd.Stream.gradient).parameters
    assert list(p) == ["self", "items", "op", "axis", "spacing", "out_dtype", "interior", "stream"]
    assert p["axis"].default == 0 and p["spacing"].default is None and p["out_dtype"].default is None and p["interior"].default is False and p["stream"].default is None
    p = inspect.signature(sz3_amd.gradient_plan).parameters
    assert list(p) == ["conf", "dtype", "items", "op", "axis", "spacing", "out_dtype", "interior"]
    assert p["axis"].default == 0 and p["spacing"].default is None and p["out_dtype"].default is None and p["interior"].default is False
    p = inspect.signature(sz3_amd.gradient_points).parameters
    assert list(p) == ["tensor", "op", "axis", "spacing", "out_dtype", "interior", "out", "stream"]
    assert p["axis"].default == 0 and p["spacing"].default is None and p["out"].default is None and p["stream"].default is None
    conf = conf_for(SHAPE)
    for name in OPS:
        for spelled in (name, name.upper()):
            got = sz3_amd.gradient_plan(conf, "float64", GOOD, spelled)
            assert got["out_elem_bytes"] == (24 if name == "vector" else 8) and got["n"] == len(GOOD)
            assert got["out_points"] == 120 + 120 + 72 + 1 + 8
    assert sz3_amd.gradient_plan(conf, "float32", GOOD, "deriv", -1, 2.0)["out_points"] == 321, "axis -1 is the last one; a scalar spacing holds for every axis"
    assert sz3_amd.gradient_plan(conf, "float32", WIDE, "deriv", 2, (1, 2, 3), "float64", True)["out_points"] == 4 * 5 * 4 * 2 + 3 * 3 * 6 + 3 * 4 + 5 * 3
    with pytest.raises(ValueError):
        sz3_amd.gradient_plan(conf, "float32", GOOD, "laplace")
    with pytest.raises(ValueError):
        sz3_amd.gradient_plan(conf, "float32", GOOD, "deriv", 3)
    with pytest.raises(ValueError):
        sz3_amd.gradient_plan(conf, "float32", GOOD, "mag", 1)
    with pytest.raises(ValueError):
        sz3_amd.gradient_plan(conf, "float32", GOOD, "mag", 0, (1.0, 2.0))
    with pytest.raises(ValueError):
        sz3_amd.gradient_plan(conf, "float32", GOOD, "mag", 0, None, "float16")
    with pytest.raises(ValueError):
        sz3_amd.gradient_plan(conf, "float32", [(0, (0, 0, 0))], "mag")
    with pytest.raises(sz3_amd.SZ3HipError):
        sz3_amd.gradient_plan(conf, "float32", GOOD, "mag", 0, 0.0)
    with pytest.raises(TypeError):
        sz3_amd.gradient_points([1.0, 2.0], "mag")


@pytest.mark.parametrize("shape", [(7,), (1,), (2, 5), (4, 1, 6), (3, 4, 5, 2)])
def test_the_model_is_numpys_gradient_where_both_are_exact(shape):
    """small integers, spacings that are powers of two: every difference and quotient is exact, so numpy's edge_order=1 gradient and the rule
    agree in every bit"""
    rng = np.random.default_rng(5)
    x = rng.integers(-64, 64, size=shape).astype(np.float32)
    N = len(shape)
    spacing = (0.5, 2.0, 1.0, 4.0)[:N]
    for level in (0, 2):
        steps = [s * 2.0 ** level for s in spacing]
        want = []
        for a in range(N):
            g = np.gradient(x.astype(np.float64), steps[a], axis=a, edge_order=1) if shape[a] > 1 else np.zeros(shape)
            want.append(g)
            got = gm.gradient(x, "deriv", a, spacing, level, np.float64)
            assert got.dtype == np.float64 and gm.same_bytes(got, g), a
        assert gm.same_bytes(gm.gradient(x, "vector", 0, spacing, level, np.float64), np.stack(want, axis=-1))
        m2 = sum(g * g for g in want)
        assert np.array_equal(gm.gradient(x, "mag2", 0, spacing, level, np.float64), m2)
        assert np.array_equal(gm.gradient(x, "mag", 0, spacing, level, np.float32), np.sqrt(m2).astype(np.float32))
        if all(e >= 3 for e in shape):
            inner = tuple(slice(1, -1) for _ in shape)
            assert np.array_equal(gm.gradient(x, "mag2", 0, spacing, level, np.float64, interior=True), m2[inner])
            assert gm.gradient(x, "vector", 0, spacing, level, interior=True).shape == tuple(e - 2 for e in shape) + (N,)
        if shape[0] >= 3:
            assert np.array_equal(gm.gradient(x, "deriv", 0, spacing, level, np.float64, interior=True), want[0][1:-1])

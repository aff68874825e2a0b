"""Boxes composited along an axis, without a GPU: the symbols and constants, the two structs' layout against the header,
the plan — a pure host function — against the request's plan, every refusal that comes before anything touches a device (the output overlap
on the COLLAPSED box in output elements among them), the Python names and signatures, and the numpy model (composite_model.py) against
closed forms where both are exact. Output and table pointers here are numbers: the plan never reads or writes them."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

import sz3_amd
import composite_model as cm
from test_map_cpu import c_struct
from test_request_cpu import BASE, EINVAL, EUNSUPPORTED, HEADER, IDS, SHAPES, boxes_at, conf_for, err, reqs_of

L = sz3_amd.lib()
SYMBOLS = ("sz3hip_stream_composite", "sz3hip_composite_plan_for", "sz3hip_composite_device")
CONSTANTS = {"SZ3HIP_COMPOSITE_RGBA32F": 0, "SZ3HIP_COMPOSITE_RGBA8": 1, "SZ3HIP_COMPOSITE_REVERSE": 1, "SZ3HIP_COMPOSITE_LEVEL_OPACITY": 2,
             "SZ3HIP_COMPOSITE_ACCUMULATE": 4}
REV, LVL, ACC = 1, 2, 4
SHAPE = (65, 47, 130)
GOOD = [(0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6)), (2, (2, 1, 0), (3, 3, 8)), (0, (9, 9, 9), (1, 1, 1)), (3, (0, 0, 0), (2, 2, 2))]
LUT = 1 << 39  # a made-up, 16-byte aligned device address
INF, NAN = float("inf"), float("nan")


def opts_of(axis=0, out_type=0, flags=0, lo=0.0, hi=1.0, cutoff=INF, lut_n=256, d_lut=LUT, level_bias=0, reserved=0):
    o = sz3_amd._CCompositeOpts()
    o.lo, o.hi, o.cutoff, o.axis, o.out_type, o.flags, o.lut_n, o.level_bias, o.reserved, o.d_lut = lo, hi, cutoff, axis, out_type, flags, lut_n, level_bias, reserved, d_lut
    return o


def flag_sets(out_type):
    """every flag combination the output type allows"""
    return [f for f in range(8) if out_type == 0 or not f & ACC]


DEFAULT = object()


def plan(conf, items, dtype=0, n=None, opts=DEFAULT, esz=16):
    p = sz3_amd._CCompositePlan()
    o = opts_of() if opts is DEFAULT else opts
    rc = L.sz3hip_composite_plan_for(C.byref(conf._c), dtype, reqs_of(items, conf.N, esz), len(items) if n is None else n, None if o is None else C.byref(o),
                                     C.byref(p))
    return rc, p


def refused(conf, items, fragment, code=EINVAL, **kw):
    rc, p = plan(conf, items, **kw)
    assert rc == code and fragment in err(), (rc, err(), fragment)
    assert bytes(p) == bytes(C.sizeof(p)), "a refused plan is zero"


def test_symbols_and_constants():
    with open(HEADER) as f:
        txt = f.read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, txt), "%s is not declared in include/sz3hip.h" % sym
    for name, v in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%du\b" % (name, v), txt), name
    assert (sz3_amd.COMPOSITE_RGBA32F, sz3_amd.COMPOSITE_RGBA8) == (0, 1)
    assert (sz3_amd.COMPOSITE_REVERSE, sz3_amd.COMPOSITE_LEVEL_OPACITY, sz3_amd.COMPOSITE_ACCUMULATE) == (REV, LVL, ACC)
    assert re.search(r"#define\s+SZ3HIP_MAX_LUT\s+1024\b", txt)


@pytest.mark.parametrize("name,cls,size", [("sz3hip_composite_opts", "_CCompositeOpts", 56), ("sz3hip_composite_plan", "_CCompositePlan", 48)])
def test_struct_layout_matches_the_header(name, cls, size):
    with open(HEADER) as f:
        txt = f.read()
    fields = c_struct(name, txt)
    assert re.search(r"typedef struct %s \{\s*/\* %d bytes \*/" % (name, size), txt), "the struct's comment states its size"
    S = getattr(sz3_amd, cls)
    assert fields == list(S._fields_)
    assert C.sizeof(S) == size
    off = 0  # natural alignment, no hidden padding
    for n, t in S._fields_:
        assert getattr(S, n).offset == off, n
        off += C.sizeof(t)
    assert off == size
    if cls == "_CCompositeOpts":
        assert sorted(n for n, _ in fields) == sorted(["lo", "hi", "cutoff", "axis", "out_type", "flags", "lut_n", "level_bias", "d_lut", "reserved"])


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plan(shape, dtype):
    conf = conf_for(shape)
    boxes = [(k, lo, ext) for k in (2, 0, 3, 1) for lo, ext in boxes_at(shape, k)]  # levels 0 - 3 in one request
    name = "float32" if dtype == 0 else "float64"
    want = sz3_amd.request_plan(conf, name, boxes)
    for axis in range(len(shape)):
        outs = 0
        for _, _, ext in boxes:
            n = 1
            for j, e in enumerate(ext):
                n *= 1 if j == axis else e
            outs += n
        for out_type in (0, 1):
            for flags in flag_sets(out_type):
                rc, p = plan(conf, boxes, dtype=dtype, opts=opts_of(axis, out_type, flags))
                assert rc == 0, err()
                got = {k: getattr(p, k) for k, _ in sz3_amd._CCompositePlan._fields_}
                assert got == dict(want, out_points=outs, out_elem_bytes=(16, 4)[out_type], reserved=0), (axis, out_type, flags)
                got.pop("reserved")
                assert sz3_amd.composite_plan(conf, name, boxes, axis, 256, 0.0, 1.0, ("rgba32f", "rgba8")[out_type], reverse=bool(flags & REV),
                                              level_opacity=bool(flags & LVL), accumulate=bool(flags & ACC)) == got


def test_refusals_of_the_options():
    conf = conf_for(SHAPE)
    refused(conf, GOOD, "NULL argument (opts)", opts=None)
    for bad in (2, 3, 255, 0xFFFFFFFF):
        refused(conf, GOOD, "out_type (%u)" % bad, opts=opts_of(out_type=bad))
    for bad in (8, 16, 0x80000000, 0xFFFFFFF8):
        refused(conf, GOOD, "flags (0x%x)" % bad, opts=opts_of(flags=bad))
    for bad in (1, 1 << 31):
        refused(conf, GOOD, "reserved word is %u" % bad, opts=opts_of(reserved=bad))
    for bad in (3, 4, 0xFFFFFFFF):
        refused(conf, GOOD, "axis (%u)" % bad, opts=opts_of(axis=bad))
    refused(conf_for((33, 70)), [(0, (0, 0), (4, 5))], "axis (2)", opts=opts_of(axis=2))
    refused(conf_for((1000,)), [(0, (0,), (40,))], "axis (1)", opts=opts_of(axis=1))
    for lo, hi in ((NAN, 1.0), (0.0, NAN), (-INF, 1.0), (0.0, INF)):
        refused(conf, GOOD, "is not finite", opts=opts_of(lo=lo, hi=hi))
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, -0.0)):
        refused(conf, GOOD, "is empty", opts=opts_of(lo=lo, hi=hi))
    refused(conf, GOOD, "too wide", opts=opts_of(lo=-1.7e308, hi=1.7e308))
    for bad in (0.0, -0.0, -1.0, NAN, -INF):
        refused(conf, GOOD, "cutoff", opts=opts_of(cutoff=bad))
    for ok in (INF, 1e-300, 1.0, 0.99, 5e-324):
        assert plan(conf, GOOD, opts=opts_of(cutoff=ok))[0] == 0, err()
    for bad in (0, 1, 1025, 0xFFFFFFFF):
        refused(conf, GOOD, "the table has %u entries" % bad, opts=opts_of(lut_n=bad))
    for ok in (2, 3, 1024):
        assert plan(conf, GOOD, opts=opts_of(lut_n=ok))[0] == 0, err()
    refused(conf, GOOD, "the table (d_lut) is NULL", opts=opts_of(d_lut=None))
    for off in (1, 4, 8, 12):
        refused(conf, GOOD, "the table (d_lut) is not aligned", opts=opts_of(d_lut=LUT + off))
    for out_type in (0, 1):
        for flags in flag_sets(out_type):
            assert plan(conf, GOOD, opts=opts_of(out_type=out_type, flags=flags))[0] == 0, err()
    for flags in (ACC, ACC | REV, ACC | LVL, 7):
        refused(conf, GOOD, "SZ3HIP_COMPOSITE_ACCUMULATE", opts=opts_of(out_type=1, flags=flags))


def test_squarings_are_at_most_30():
    conf = conf_for(SHAPE)
    # by level_bias alone
    assert plan(conf, GOOD, opts=opts_of(level_bias=30))[0] == 0, err()
    for bad in (31, 32, 0xFFFFFFFF):
        refused(conf, GOOD, "level_bias is %u" % bad, opts=opts_of(level_bias=bad))
    # by bias + level: GOOD's levels are 0, 1, 2, 0, 3 — without LEVEL_OPACITY the level does not count
    assert plan(conf, GOOD, opts=opts_of(level_bias=30))[0] == 0, err()
    assert plan(conf, GOOD, opts=opts_of(level_bias=27, flags=LVL))[0] == 0, err()
    refused(conf, GOOD, "box 4: level_bias (28) and the box's level (3) make 31 squarings", opts=opts_of(level_bias=28, flags=LVL))
    refused(conf, GOOD, "box 2: level_bias (29) and the box's level (2) make 31 squarings", opts=opts_of(level_bias=29, flags=LVL))
    refused(conf, GOOD, "box 1: level_bias (30) and the box's level (1) make 31 squarings", opts=opts_of(level_bias=30, flags=LVL | REV))
    first = [(2, (0, 0, 0), (2, 2, 2))] + GOOD[:2]
    refused(conf, first, "box 0: level_bias (29) and the box's level (2) make 31 squarings", opts=opts_of(level_bias=29, flags=LVL))
    assert plan(conf, first, opts=opts_of(level_bias=28, flags=LVL))[0] == 0, err()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_refusals_of_the_boxes_and_views(axis):
    """sz3hip_stream_request's own, with its wording, on the collapsed box: each at the first, a middle and the last box"""
    conf = conf_for(SHAPE)
    n = len(GOOD)
    o = opts_of(axis)
    o8 = opts_of(axis, 1)
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
        at = BASE + (1 << 30)
        assert plan(conf, edit((k, lo, ext, at, good)), opts=o)[0] == 0, err()
        refused(conf, edit((31, lo, ext)), "box %d: " % b, opts=o)
        refused(conf, edit((k, (1 << 40, 0, 0), ext)), "box %d: " % b, opts=o)
        for j in range(3):  # an extent of 0, at the axis too
            refused(conf, edit((k, lo, tuple(0 if i == j else e for i, e in enumerate(ext)))), "box %d: " % b, opts=o)
        refused(conf, edit((k, lo, ext, None, None, 7)), "box %d: the reserved word is 7" % b, opts=o)
        for j in range(3):
            if flat[j] == 1:  # the stride at the axis, as that of any extent-1 dimension, is not read: garbage is accepted
                for junk in (-5, 0, 1 << 60, 3):
                    for oo in (o, o8):
                        assert plan(conf, edit((k, lo, ext, at, tuple(junk if i == j else v for i, v in enumerate(good)))), opts=oo)[0] == 0, err()
                continue
            refused(conf, edit((k, lo, ext, at, tuple(-v if i == j else v for i, v in enumerate(good)))),
                    "box %d: the view's stride of dimension %d is negative" % (b, j), opts=o)
            refused(conf, edit((k, lo, ext, at, tuple(0 if i == j else v for i, v in enumerate(good)))),
                    "box %d: the view's stride of dimension %d is zero" % (b, j), opts=o)
        counted = [j for j in range(3) if flat[j] > 1]
        if len(counted) == 2:
            swapped = list(good)
            swapped[counted[0]], swapped[counted[1]] = good[counted[1]], good[counted[0]]
            refused(conf, edit((k, lo, ext, at, tuple(swapped))), "box %d: the view's strides are permuted or overlap" % b, opts=o)
        # an output not aligned to its element: 16 bytes (four floats) and 4 (RGBA8)
        for off in (1, 4, 8, 12):
            refused(conf, edit((k, lo, ext, at + off)), "box %d: the output is not aligned to its element size (16 bytes)" % b, opts=o)
        for off in (1, 2, 3):
            refused(conf, edit((k, lo, ext, at + off)), "box %d: the output is not aligned to its element size (4 bytes)" % b, opts=o8)
        assert plan(conf, edit((k, lo, ext, at + 4)), opts=o8)[0] == 0, err()
        arr = reqs_of(edit((k, lo, ext)), 3, 16)
        arr[b].d_out = None
        p = sz3_amd._CCompositePlan()
        assert L.sz3hip_composite_plan_for(C.byref(conf._c), 0, arr, n, C.byref(o), C.byref(p)) == EINVAL and "box %d: the output array is NULL" % b in err()


@pytest.mark.parametrize("out_type", [0, 1], ids=["16B", "4B"])
def test_output_overlap_is_counted_on_the_collapsed_box(out_type):
    conf = conf_for(SHAPE)
    e = (16, 4)[out_type]
    a, b = (0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6))
    at = BASE + (1 << 20)
    for axis, outs in ((0, 30), (1, 24), (2, 20)):
        opts = opts_of(axis, out_type)
        # contiguous outputs of `outs` elements: the second may start right behind the first's last element, and not one element earlier
        assert plan(conf, [a + (at,), b + (at + outs * e,)], opts=opts)[0] == 0, err()
        refused(conf, [a + (at,), b + (at + outs * e - e,)], "box 1: the output overlaps box 0's", opts=opts)
        refused(conf, [b + (at + outs * e - e,), a + (at,)], "box 1: the output overlaps box 0's", opts=opts)
    # rectangles of one atlas of pitch 13 (axis 0 folded: 5 x 6 images): side by side along x they are apart; one column closer they meet
    opts = opts_of(0, out_type)
    st = (5 * 13, 13, 1)
    assert plan(conf, [a + (at, st), b + (at + 6 * e, st)], opts=opts)[0] == 0, err()
    refused(conf, [a + (at, st), b + (at + 5 * e, st)], "box 1: the output overlaps box 0's", opts=opts)
    # two boxes that differ only along the axis share their output: refused (ACCUMULATE goes call by call). Repeated BOXES apart are allowed
    for axis in range(3):
        lo2 = tuple(4 if j == axis else 0 for j in range(3))
        for flags in ((0, ACC) if out_type == 0 else (0,)):
            refused(conf, [a + (at,), (0, lo2, (4, 5, 6), at)], "box 1: the output overlaps box 0's", opts=opts_of(axis, out_type, flags))
            refused(conf, [a + (at, st), (0, lo2, (4, 5, 6), at, st)], "box 1: the output overlaps box 0's", opts=opts_of(axis, out_type, flags))
    assert plan(conf, [a + (at,), a + (at + 30 * e,)], opts=opts)[0] == 0, err()


def test_integer_types_and_null_arguments():
    conf = conf_for(SHAPE)
    for dt in range(2, 10):
        rc, _ = plan(conf, GOOD, dtype=dt)
        assert rc == EUNSUPPORTED and "integer element types are not supported yet" in err()
    refused(conf, GOOD, "dataType", code=EUNSUPPORTED, dtype=10)
    p = sz3_amd._CCompositePlan()
    o = opts_of()
    arr = reqs_of(GOOD, 3, 16)
    assert L.sz3hip_composite_plan_for(None, 0, arr, len(GOOD), C.byref(o), C.byref(p)) == EINVAL and "NULL argument (conf)" in err()
    assert L.sz3hip_composite_plan_for(C.byref(conf._c), 0, arr, len(GOOD), C.byref(o), None) == EINVAL and "NULL argument (out)" in err()
    assert L.sz3hip_composite_plan_for(C.byref(conf._c), 0, None, len(GOOD), C.byref(o), C.byref(p)) == EINVAL
    assert L.sz3hip_stream_composite(None, arr, len(GOOD), C.byref(o), None) == EINVAL and "no handle" in err()
    dims = (C.c_uint64 * 1)(8)
    for dt in range(2, 10):  # sz3hip_composite_device refuses integers before it looks at a pointer
        assert L.sz3hip_composite_device(dt, 1, dims, BASE, None, C.byref(o), BASE + 4096, None, None) == EUNSUPPORTED
        assert "integer element types are not supported yet" in err()
    assert L.sz3hip_composite_device(0, 5, dims, BASE, None, C.byref(o), BASE + 4096, None, None) == EINVAL and "dimension count" in err()
    assert L.sz3hip_composite_device(0, 1, dims, BASE, None, C.byref(o), None, None, None) == EINVAL and "d_out" in err()
    assert L.sz3hip_composite_device(0, 1, dims, BASE, None, None, BASE + 4096, None, None) == EINVAL and "opts" in err()
    bad = (opts_of(out_type=2), opts_of(axis=1), opts_of(flags=8), opts_of(reserved=1), opts_of(hi=0.0), opts_of(cutoff=0.0), opts_of(lut_n=1), opts_of(d_lut=None),
           opts_of(d_lut=LUT + 4), opts_of(level_bias=31), opts_of(out_type=1, flags=ACC), opts_of(lo=NAN))
    for b in bad:
        assert L.sz3hip_composite_device(0, 1, dims, None, None, C.byref(b), None, None, None) == EINVAL, "the options come before any pointer"
        assert "d_out" not in err() and "NULL argument" not in err(), err()


def test_python_names_and_signatures():
    p = inspect.signature(sz3_amd.Stream.composite).parameters
    assert list(p) == ["self", "items", "axis", "lut", "lo", "hi", "out_type", "reverse", "level_opacity", "accumulate", "cutoff", "level_bias", "stream"]
    assert (p["out_type"].default, p["reverse"].default, p["level_opacity"].default, p["accumulate"].default, p["cutoff"].default, p["level_bias"].default,
            p["stream"].default) == ("rgba32f", False, False, False, INF, 0, None)
    p = inspect.signature(sz3_amd.composite_plan).parameters
    assert list(p)[:7] == ["conf", "dtype", "items", "axis", "lut", "lo", "hi"] and p["out_type"].default == "rgba32f" and p["cutoff"].default == INF
    p = inspect.signature(sz3_amd.composite_points).parameters
    assert list(p)[:5] == ["tensor", "axis", "lut", "lo", "hi"] and p["out_type"].default == "rgba32f" and p["out"].default is None and p["stream"].default is None
    conf = conf_for(SHAPE)
    for spelled, b in (("rgba32f", 16), ("RGBA32F", 16), ("rgba8", 4), ("RGBA8", 4)):
        got = sz3_amd.composite_plan(conf, "float64", GOOD, -1, 256, 0.0, 1.0, spelled)
        assert got["out_elem_bytes"] == b and got["n"] == len(GOOD)
        assert got["out_points"] == 4 * 5 + 4 * 5 + 3 * 3 + 1 + 2 * 2, "axis -1 is the last one"
    with pytest.raises(ValueError):
        sz3_amd.composite_plan(conf, "float32", GOOD, 0, 256, 0.0, 1.0, "rgb")
    with pytest.raises(ValueError):
        sz3_amd.composite_plan(conf, "float32", GOOD, 3, 256, 0.0, 1.0)
    with pytest.raises(ValueError):
        sz3_amd.composite_plan(conf, "float32", [(0, (0, 0, 0))], 0, 256, 0.0, 1.0)
    with pytest.raises(sz3_amd.SZ3HipError, match="SZ3HIP_COMPOSITE_ACCUMULATE"):
        sz3_amd.composite_plan(conf, "float32", GOOD, 0, 256, 0.0, 1.0, "rgba8", accumulate=True)
    with pytest.raises(TypeError):
        sz3_amd.composite_points([1.0, 2.0], 0, None, 0.0, 1.0)


# ---- the model against closed forms where both are exact -------------------------------------------------------------------------------------
HALF = np.array([[1.0, 1.0, 1.0, 0.5]] * 4, dtype=np.float32)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 31, 52])
def test_model_half_opacity_column(n):
    v = np.linspace(0.0, 0.99, n).reshape(n, 1)
    got = cm.composite(v, 0, HALF, 0.0, 1.0)
    want = 1.0 - 2.0 ** -n  # (exact in double up to n = 53)
    assert got.shape == (1, 1, 4) and (got == want).all()
    assert (cm.expected(v, 0, HALF, 0.0, 1.0) == np.float32(want)).all()
    # with one squaring the opacity is 0.75: A = 1 - 4^-n
    assert (cm.corrected_alpha(HALF, 1) == 0.75).all() and (cm.corrected_alpha(HALF, 2) == 1.0 - 2.0 ** -4).all()
    if 2 * n <= 53:
        assert (cm.composite(v, 0, HALF, 0.0, 1.0, s=1) == 1.0 - 4.0 ** -n).all()
    # NaN points are skipped: they add nothing and stop nothing
    w = np.full((2 * n + 1, 1), np.nan)
    w[1::2] = v
    assert (cm.composite(w, 0, HALF, 0.0, 1.0) == want).all()


def test_model_cutoff_reverse_and_codes():
    # entry 0 is opaque red, entry 1 half-transparent green: x < 0.5 picks 0
    lut = np.array([[1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 0.5]], dtype=np.float32)
    v = np.array([[0.1, 0.9, 0.9], [0.9, 0.1, 0.9], [0.9, 0.9, 0.1]])
    got = cm.composite(v, 1, lut, 0.0, 1.0, cutoff=1.0)
    assert got.shape == (3, 1, 4)
    assert (got[0, 0] == [1.0, 0.0, 0.0, 1.0]).all(), "a = 1 stops at the first point for cutoff 1"
    assert (got[1, 0] == [0.5, 0.5, 0.0, 1.0]).all() and (got[2, 0] == [0.25, 0.75, 0.0, 1.0]).all()
    # without a cutoff an opaque column goes on folding with weight 0: the same sums here
    assert (cm.composite(v, 1, lut, 0.0, 1.0) == got).all()
    # a cutoff below the first weight stops every column at once
    one = cm.composite(v, 1, lut, 0.0, 1.0, cutoff=0.5)
    assert (one[1, 0] == [0.0, 0.5, 0.0, 0.5]).all() and (one[0, 0] == [1.0, 0.0, 0.0, 1.0]).all()
    # REVERSE on a reversed column equals the forward fold
    rng = np.random.default_rng(3)
    lut = rng.random((16, 4)).astype(np.float32)
    v = rng.random((5, 23, 3))
    for axis in range(3):
        fwd = cm.composite(v, axis, lut, 0.0, 1.0, cutoff=0.9, s=1)
        assert (cm.composite(np.flip(v, axis), axis, lut, 0.0, 1.0, reverse=True, cutoff=0.9, s=1) == fwd).all()
    assert (cm.composite(v, 1, lut, 0.0, 1.0, reverse=True) != cm.composite(v, 1, lut, 0.0, 1.0)).any(), "the order matters"
    # the codes: the mapping's rule
    x = np.array([-INF, -1.0, 0.0, 0.4999, 0.5, np.nextafter(1.0, 0.0), 1.0, 7.0, INF])
    assert list(cm.codes(x, 0.0, 1.0, 2)) == [0, 0, 0, 0, 1, 1, 1, 1, 1]
    assert list(cm.codes(x, 0.0, 1.0, 1024)) == [0, 0, 0, 511, 512, 1023, 1023, 1023, 1023]
    # the carry: a column split in two, the second starting from the first's float32 image, is the model's carried form — and differs
    # from the one-box result where the float32 rounding bites
    v = rng.random((40, 6))
    lut = rng.random((64, 4)).astype(np.float32) * np.float32(0.2)
    first = cm.expected(v[:17], 0, lut, 0.0, 1.0)
    carried = cm.composite(v[17:], 0, lut, 0.0, 1.0, carry=first)
    whole = cm.composite(v, 0, lut, 0.0, 1.0)
    assert np.allclose(carried, whole, rtol=1e-6) and (carried != whole).any()
    # all NaN: +0.0
    z = cm.composite(np.full((4, 3), np.nan), 0, lut, 0.0, 1.0)
    assert (z == 0.0).all() and not np.signbit(z).any()


def test_model_rgba8_packing():
    c = np.array([0.0, 1.0, 0.5, NAN, -1.0, 2.0, 1.0 / 255.0, 0.5 / 255.0 - 1e-12, 254.6 / 255.0, INF, -INF])
    assert list(cm.pack8(c)) == [0, 255, 128, 0, 0, 255, 1, 0, 255, 255, 0]
    state = np.array([[0.0, 1.0, 0.5, NAN], [-1.0, 2.0, 0.25, 1.0]])
    assert list(cm.store(state, cm.RGBA8)) == [0 | 255 << 8 | 128 << 16 | 0 << 24, 0 | 255 << 8 | 64 << 16 | 255 << 24]
    assert cm.store(state, cm.RGBA8).dtype == np.uint32 and cm.store(state, cm.RGBA32F).dtype == np.float32
    assert math.isnan(cm.store(state, cm.RGBA32F)[0, 3])
    assert all(cm.pack8(np.float64(i) / 255.0) == i for i in range(256))

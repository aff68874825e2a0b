"""Texels out of a request, without a GPU: the symbols and constants, the two structs' layout against the header, the
plan — a pure host function — against the request's plan, every refusal that comes before anything touches a device (the output overlap in
OUTPUT elements among them), and the Python names and signatures. Output pointers here are numbers: the plan never reads or writes them."""
import ctypes as C
import inspect
import re

import pytest

import sz3_amd
from test_request_cpu import BASE, EINVAL, EUNSUPPORTED, HEADER, IDS, SHAPES, boxes_at, conf_for, err, reqs_of

L = sz3_amd.lib()
SYMBOLS = ("sz3hip_stream_map", "sz3hip_map_plan_for", "sz3hip_map_device")
CONSTANTS = {"SZ3HIP_MAP_U8": 1, "SZ3HIP_MAP_U16": 2, "SZ3HIP_MAP_F16": 3, "SZ3HIP_MAP_F32": 4, "SZ3HIP_MAP_LUT32": 5, "SZ3HIP_MAX_LUT": 1024}
TYPES = {"u8": (1, 1), "u16": (2, 2), "f16": (3, 2), "f32": (4, 4), "lut32": (5, 4)}  # name -> (SZ3HIP_MAP_*, bytes of a texel)
LUT = 1 << 39  # a made-up device address of a table
SHAPE = (65, 47, 130)
GOOD = [(0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6)), (2, (2, 1, 0), (3, 3, 8)), (0, (9, 9, 9), (1, 1, 1)), (3, (0, 0, 0), (2, 2, 2))]


def c_struct(name, txt):
    """the fields of a typedef'd struct of the header as (name, ctypes type); a pointer of any type is a c_void_p"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "double": C.c_double}
    out = []
    for decl in body.split(";"):
        decl = re.sub(r"\bconst\b", "", decl).strip()
        if not decl:
            continue
        m = re.match(r"(\w+)\s*(.*)$", decl)
        for var in m.group(2).split(","):
            a = re.match(r"\s*(\*?)\s*(\w+)\s*$", var)
            out.append((a.group(2), C.c_void_p if a.group(1) else ctype[m.group(1)]))
    return out


def opts_of(out_type="u8", lo=0.0, hi=1.0, nan_code=0, lut_n=0, d_lut=None, flags=0, reserved=0):
    o = sz3_amd._CMapOpts()
    o.out_type = TYPES[out_type][0] if isinstance(out_type, str) else out_type
    if out_type in ("f16", "f32") and (lo, hi) == (0.0, 1.0):
        hi = 0.0
    if out_type == "lut32" and lut_n == 0 and d_lut is None:
        lut_n, d_lut = 16, LUT
    o.lo, o.hi, o.nan_code, o.lut_n, o.d_lut, o.flags, o.reserved = lo, hi, nan_code, lut_n, d_lut, flags, reserved
    return o


DEFAULT = object()


def plan(conf, items, dtype=0, n=None, opts=DEFAULT, esz=1):
    p = sz3_amd._CMapPlan()
    o = opts_of() if opts is DEFAULT else opts
    rc = L.sz3hip_map_plan_for(C.byref(conf._c), dtype, reqs_of(items, conf.N, esz), len(items) if n is None else n, None if o is None else C.byref(o), C.byref(p))
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
    for name, v in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, v), txt), name
    assert (sz3_amd.MAP_U8, sz3_amd.MAP_U16, sz3_amd.MAP_F16, sz3_amd.MAP_F32, sz3_amd.MAP_LUT32, sz3_amd.MAX_LUT) == (1, 2, 3, 4, 5, 1024)


@pytest.mark.parametrize("name,cls,size", [("sz3hip_map_opts", "_CMapOpts", 48), ("sz3hip_map_plan", "_CMapPlan", 40)])
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


@pytest.mark.parametrize("out_type", list(TYPES))
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plan(shape, interp, dtype, out_type):
    conf = conf_for(shape, interpAlgo=interp)
    boxes = [(k, lo, ext) for k in (2, 0, 3, 1) for lo, ext in boxes_at(shape, k)]
    rc, p = plan(conf, boxes, dtype=dtype, opts=opts_of(out_type), esz=TYPES[out_type][1])
    assert rc == 0, err()
    want = sz3_amd.request_plan(conf, "float32" if dtype == 0 else "float64", boxes)
    got = {k: getattr(p, k) for k, _ in sz3_amd._CMapPlan._fields_}
    assert got == dict(want, out_elem_bytes=TYPES[out_type][1])
    assert sz3_amd.map_plan(conf, "float32" if dtype == 0 else "float64", boxes, out_type, 0.0, 0.0 if out_type in ("f16", "f32") else 1.0,
                            lut=16 if out_type == "lut32" else None) == got


def test_refusals_of_the_options():
    conf = conf_for(SHAPE)
    refused(conf, GOOD, "NULL argument (opts)", opts=None)
    for bad in (0, 6, 255):
        refused(conf, GOOD, "out_type", opts=opts_of(bad))
    refused(conf, GOOD, "flags", opts=opts_of(flags=1))
    refused(conf, GOOD, "reserved", opts=opts_of(reserved=1 << 40))
    for t in ("u8", "u16", "lut32"):
        e = TYPES[t][1]
        for lo, hi in ((float("nan"), 1.0), (0.0, float("nan")), (float("-inf"), 1.0), (0.0, float("inf"))):
            refused(conf, GOOD, "not finite", opts=opts_of(t, lo, hi), esz=e)
        refused(conf, GOOD, "is empty", opts=opts_of(t, 1.0, 1.0), esz=e)
        refused(conf, GOOD, "is empty", opts=opts_of(t, 1.0, -1.0), esz=e)
        refused(conf, GOOD, "hi - lo is not finite", opts=opts_of(t, -1.7e308, 1.7e308), esz=e)
    refused(conf, GOOD, "nan_code (256)", opts=opts_of("u8", nan_code=256))
    refused(conf, GOOD, "nan_code (65536)", opts=opts_of("u16", nan_code=65536), esz=2)
    assert plan(conf, GOOD, opts=opts_of("u8", nan_code=255))[0] == 0 and plan(conf, GOOD, opts=opts_of("u16", nan_code=65535), esz=2)[0] == 0
    assert plan(conf, GOOD, opts=opts_of("lut32", nan_code=0xFFFFFFFF), esz=4)[0] == 0, "LUT32's nan_code is the raw texel"
    for n in (1, 1025, 0):
        refused(conf, GOOD, "entries", opts=opts_of("lut32", lut_n=n, d_lut=LUT), esz=4)
    for n in (2, 1024):
        assert plan(conf, GOOD, opts=opts_of("lut32", lut_n=n, d_lut=LUT), esz=4)[0] == 0, err()
    refused(conf, GOOD, "(d_lut) is NULL", opts=opts_of("lut32", lut_n=16, d_lut=None), esz=4)
    for off in (1, 2, 3):
        refused(conf, GOOD, "(d_lut) is not aligned", opts=opts_of("lut32", lut_n=16, d_lut=LUT + off), esz=4)
    for t in ("u8", "u16"):
        refused(conf, GOOD, "hold a table", opts=opts_of(t, lut_n=16), esz=TYPES[t][1])
        refused(conf, GOOD, "hold a table", opts=opts_of(t, d_lut=LUT), esz=TYPES[t][1])
    for t in ("f16", "f32"):
        e = TYPES[t][1]
        for kw in (dict(lo=-1.0, hi=0.0), dict(lo=0.0, hi=2.0), dict(hi=0.0, nan_code=1), dict(hi=0.0, lut_n=2), dict(hi=0.0, d_lut=LUT)):
            refused(conf, GOOD, "take none", opts=opts_of(t, **kw), esz=e)
        assert plan(conf, GOOD, opts=opts_of(t), esz=e)[0] == 0, err()


def test_refusals_of_the_boxes_and_views():
    """sz3hip_stream_request's own, with its wording: each at the first, a middle and the last box"""
    conf = conf_for(SHAPE)
    n = len(GOOD)
    refused(conf, [], "", n=0)
    refused(conf, GOOD * 60, "", n=257)
    for b in (0, n // 2, n - 1):
        def edit(item):
            items = list(GOOD)
            items[b] = item
            return items
        k, lo, ext = GOOD[b]
        s1 = ext[2] + 1
        s0 = s1 * ext[1]
        refused(conf, edit((31, lo, ext)), "box %d: " % b)
        refused(conf, edit((k, (1 << 40, 0, 0), ext)), "box %d: " % b)
        refused(conf, edit((k, lo, (0, 1, 1))), "box %d: " % b)
        refused(conf, edit((k, lo, ext, None, None, 7)), "box %d: the reserved word is 7" % b)
        refused(conf, edit((k, lo, ext, BASE + (1 << 30), (-s0, s1, 1))), "box %d: the view's stride of dimension 0 is negative" % b)
        refused(conf, edit((k, lo, ext, BASE + (1 << 30), (0, s1, 1))), "box %d: the view's stride of dimension 0 is zero" % b)
        refused(conf, edit((k, lo, ext, BASE + (1 << 30), (s1, s0, 1))), "box %d: the view's strides are permuted or overlap" % b)
        # an output not aligned to its element: two- and four-byte texels
        for t, off in (("u16", 1), ("f16", 1), ("f32", 2), ("lut32", 1), ("lut32", 2)):
            refused(conf, edit((k, lo, ext, BASE + (1 << 30) + off)), "box %d: the output is not aligned to its element size (%d bytes)" % (b, TYPES[t][1]),
                    opts=opts_of(t), esz=TYPES[t][1])
        assert plan(conf, edit((k, lo, ext, BASE + (1 << 30) + 3)))[0] == 0, "a one-byte texel has no alignment"
        items = edit((k, lo, ext))
        arr = reqs_of(items, 3, 1)
        arr[b].d_out = None
        p = sz3_amd._CMapPlan()
        o = opts_of()
        assert L.sz3hip_map_plan_for(C.byref(conf._c), 0, arr, n, C.byref(o), C.byref(p)) == EINVAL and "box %d: the output array is NULL" % b in err()


@pytest.mark.parametrize("out_type", ["u8", "u16"])
def test_output_overlap_is_counted_in_output_elements(out_type):
    conf = conf_for(SHAPE)
    e = TYPES[out_type][1]
    a, b = (0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6))  # 120 texels each
    at = BASE + (1 << 20)
    opts = opts_of(out_type)
    # contiguous outputs: the second may start right behind the first's last byte, and not one element earlier
    assert plan(conf, [a + (at,), b + (at + 120 * e,)], opts=opts, esz=e)[0] == 0, err()
    refused(conf, [a + (at,), b + (at + 120 * e - e,)], "box 1: the output overlaps box 0's", opts=opts, esz=e)
    refused(conf, [b + (at + 120 * e - e,), a + (at,)], "box 1: the output overlaps box 0's", opts=opts, esz=e)
    # (with the handle's f32 / f64 element size these hulls would overlap: the output's size is the one used)
    rc, _ = plan(conf, [a + (at,), b + (at + 120 * e,)], dtype=1, opts=opts, esz=e)
    assert rc == 0, err()
    p = sz3_amd._CRequestPlan()
    assert L.sz3hip_request_plan_for(C.byref(conf._c), 0, reqs_of([a + (at,), b + (at + 120 * e,)], 3), 2, C.byref(p)) == EINVAL
    # rectangles of one atlas of pitch 13: side by side along x they interleave and are shown apart; one column closer they meet
    st = (5 * 13, 13, 1)
    assert plan(conf, [a + (at, st), b + (at + 6 * e, st)], opts=opts, esz=e)[0] == 0, err()
    refused(conf, [a + (at, st), b + (at + 5 * e, st)], "box 1: the output overlaps box 0's", opts=opts, esz=e)
    # repeated and overlapping BOXES are allowed
    assert plan(conf, [a + (at,), a + (at + 120 * e,)], opts=opts, esz=e)[0] == 0, err()


def test_integer_types_and_null_arguments():
    conf = conf_for(SHAPE)
    for dt in range(2, 10):
        rc, _ = plan(conf, GOOD, dtype=dt)
        assert rc == EUNSUPPORTED and "integer element types are not supported yet" in err()
    refused(conf, GOOD, "dataType", code=EUNSUPPORTED, dtype=10)
    p = sz3_amd._CMapPlan()
    o = opts_of()
    arr = reqs_of(GOOD, 3, 1)
    assert L.sz3hip_map_plan_for(None, 0, arr, len(GOOD), C.byref(o), C.byref(p)) == EINVAL and "NULL argument (conf)" in err()
    assert L.sz3hip_map_plan_for(C.byref(conf._c), 0, arr, len(GOOD), C.byref(o), None) == EINVAL and "NULL argument (out)" in err()
    assert L.sz3hip_map_plan_for(C.byref(conf._c), 0, None, len(GOOD), C.byref(o), C.byref(p)) == EINVAL
    assert L.sz3hip_stream_map(None, arr, len(GOOD), C.byref(o), None) == EINVAL and "no handle" in err()
    dims = (C.c_uint64 * 1)(8)
    for dt in range(2, 10):  # sz3hip_map_device refuses integers before it looks at a pointer
        assert L.sz3hip_map_device(dt, 1, dims, BASE, None, C.byref(o), BASE + 4096, None, None) == EUNSUPPORTED
        assert "integer element types are not supported yet" in err()
    assert L.sz3hip_map_device(0, 5, dims, BASE, None, C.byref(o), BASE + 4096, None, None) == EINVAL and "dimension count" in err()
    assert L.sz3hip_map_device(0, 1, dims, BASE, None, C.byref(o), None, None, None) == EINVAL and "d_out" in err()
    assert L.sz3hip_map_device(0, 1, dims, BASE, None, None, BASE + 4096, None, None) == EINVAL and "opts" in err()


def test_python_names_and_signatures():
    p = inspect.signature(sz3_amd.Stream.map).parameters
    assert list(p) == ["self", "items", "out_type", "lo", "hi", "nan_code", "lut", "stream"]
    assert (p["lo"].default, p["hi"].default, p["nan_code"].default, p["lut"].default, p["stream"].default) == (0.0, 0.0, 0, None, None)
    p = inspect.signature(sz3_amd.map_plan).parameters
    assert list(p) == ["conf", "dtype", "items", "out_type", "lo", "hi", "nan_code", "lut"]
    p = inspect.signature(sz3_amd.map_points).parameters
    assert list(p) == ["tensor", "out_type", "lo", "hi", "nan_code", "lut", "out", "stream"] and p["out"].default is None
    conf = conf_for(SHAPE)
    for name, (code, size) in TYPES.items():
        for spelled in (name, name.upper(), code):
            got = sz3_amd.map_plan(conf, "float32", GOOD, spelled, 0.0, 0.0 if name in ("f16", "f32") else 1.0, lut=16 if name == "lut32" else None)
            assert got["out_elem_bytes"] == size and got["n"] == len(GOOD)
    with pytest.raises(ValueError):
        sz3_amd.map_plan(conf, "float32", GOOD, "bf16")
    with pytest.raises(ValueError):
        sz3_amd.map_plan(conf, "float32", [(0, (0, 0, 0))], "u8", 0.0, 1.0)
    with pytest.raises(sz3_amd.SZ3HipError):
        sz3_amd.map_plan(conf, "float32", GOOD, "u8", 1.0, 1.0)
    with pytest.raises(TypeError):
        sz3_amd.map_points([1.0, 2.0], "u8", 0.0, 1.0)
    assert int(sz3_amd.Dbg2.MAP_PLAIN_STORES) == 4

"""The points of boxes whose values lie in a range, without a GPU: the symbols and flags, the four structs' layout
against the header, the plan — a pure host function — against the request's plan and the partition rule, every refusal that comes before
anything touches a device, and the Python names and signatures."""
import ctypes as C
import inspect
import math
import re

import pytest

import sz3_amd
from test_request_cpu import EINVAL, EUNSUPPORTED, HEADER, IDS, SHAPES, boxes_at, conf_for, err

L = sz3_amd.lib()
SYMBOLS = ("sz3hip_stream_select", "sz3hip_select_plan_for", "sz3hip_select_device")
CHUNK = 4096  # the partition rule: a chunk record per 4096 consecutive row-major indices of a box
BASE = 1 << 40  # a made-up device address


def c_struct(name, txt):
    """the fields of a typedef'd struct of the header as (name, ctypes type); a pointer of any type is a c_void_p"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "double": C.c_double, "sz3hip_box": sz3_amd._CBox}
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(\w+)\s*(.*)$", decl)
        for var in m.group(2).split(","):
            a = re.match(r"\s*(\*?)\s*(\w+)\s*$", var)
            out.append((a.group(2), C.c_void_p if a.group(1) else ctype[m.group(1)]))
    return out


def reqs_of(items, N, esz=4):
    """items: (level, lo, shape[, capacity[, d_index[, d_value[, reserved]]]]) -> the sz3hip_select_req array; an item with a capacity and no
    pointers gets index and value arrays of its own, one after the other"""
    arr = (sz3_amd._CSelectReq * max(len(items), 1))()
    at = BASE
    for i, it in enumerate(items):
        it = tuple(it) + (None,) * (7 - len(it))
        r = arr[i]
        r.level = it[0]
        r.box.lo[:N] = it[1]
        r.box.ext[:N] = it[2]
        r.capacity = it[3] or 0
        if it[4] is None and it[5] is None and r.capacity:
            r.d_index, r.d_value = at, at + r.capacity * 8
            at += (r.capacity * (8 + esz) + 7) & ~7
        else:
            r.d_index, r.d_value = it[4], it[5]
        r.reserved = it[6] or 0
    return arr


def opts_of(lo=0.0, hi=1.0, flags=0, reserved=0):
    o = sz3_amd._CSelectOpts()
    o.lo, o.hi, o.flags, o.reserved = lo, hi, flags, reserved
    return o


DEFAULT = object()


def plan(conf, items, dtype=0, n=None, opts=DEFAULT):
    p = sz3_amd._CSelectPlan()
    o = opts_of() if opts is DEFAULT else opts
    rc = L.sz3hip_select_plan_for(C.byref(conf._c), dtype, reqs_of(items, conf.N, 4 if dtype == 0 else 8), len(items) if n is None else n,
                                  None if o is None else C.byref(o), C.byref(p))
    return rc, p


def test_symbols_and_flags():
    with open(HEADER) as f:
        txt = f.read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, txt), "%s is not declared in include/sz3hip.h" % sym
    assert re.search(r"#define\s+SZ3HIP_SELECT_INVERT\s+1u\b", txt) and sz3_amd.SELECT_INVERT == 1
    assert re.search(r"#define\s+SZ3HIP_SELECT_NAN\s+2u\b", txt) and sz3_amd.SELECT_NAN == 2


@pytest.mark.parametrize("name,cls,size", [("sz3hip_select_req", "_CSelectReq", 96), ("sz3hip_select_opts", "_CSelectOpts", 24),
                                           ("sz3hip_select_head", "_CSelectHead", 32), ("sz3hip_select_plan", "_CSelectPlan", 40)])
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
def test_plan(shape, interp):
    conf = conf_for(shape, interpAlgo=interp)
    boxes = [(k, lo, ext) for k in (2, 0, 3, 1) for lo, ext in boxes_at(shape, k)]
    items = [b + (cap,) for b, cap in zip(boxes, [0, 1, 5, 4096, 7, 0, 100000, 3, 1, 2, 0, 9])]
    rc, p = plan(conf, items)
    assert rc == 0, err()
    want = sz3_amd.request_plan(conf, "float32", boxes)
    assert (p.n, p.finest_level, p.coarsest_level, p.n_levels, p.points) == tuple(want[k] for k in ("n", "finest_level", "coarsest_level", "n_levels", "points"))
    chunks = sum(-(-math.prod(ext) // CHUNK) for _, _, ext in boxes)
    assert p.partials == chunks
    # the level buffers, then the chunk records (8 bytes each) on an 8-byte boundary
    assert p.scratch_elems == ((want["scratch_elems"] + 1) & ~1) + 2 * chunks
    rc, p8 = plan(conf, items, dtype=1)
    assert rc == 0 and p8.scratch_elems == want["scratch_elems"] + chunks and p8.partials == chunks
    for flags in (1, 2, 3):  # (the plan does not depend on the range)
        rc, pf = plan(conf, items, opts=opts_of(2.0, -2.0, flags))
        assert rc == 0 and bytes(pf) == bytes(p)
    caps = [it[3] for it in items]
    assert sz3_amd.select_plan(conf, "float32", boxes, 0.0, 1.0, caps) == {k: getattr(p, k) for k, _ in sz3_amd._CSelectPlan._fields_}
    assert sz3_amd.select_plan(conf, "float32", boxes, capacity=0)["partials"] == chunks  # (count only)


def test_refusals():
    shape = (65, 47, 130)
    conf = conf_for(shape)
    good = [(2, (0, 0, 0), (4, 4, 4), 8), (0, (1, 3, 5), (6, 5, 4), 16), (1, (0, 0, 0), (3, 3, 3), 4)]
    assert plan(conf, good)[0] == 0
    out = sz3_amd._CSelectPlan()
    arr = reqs_of(good, 3)
    o = opts_of()
    assert L.sz3hip_select_plan_for(None, 0, arr, 3, C.byref(o), C.byref(out)) == EINVAL and "conf" in err()
    assert L.sz3hip_select_plan_for(C.byref(conf._c), 0, None, 3, C.byref(o), C.byref(out)) == EINVAL and "NULL" in err()
    assert L.sz3hip_select_plan_for(C.byref(conf._c), 0, arr, 3, C.byref(o), None) == EINVAL and "out" in err()
    assert plan(conf, good, n=0)[0] == EINVAL and "1 .. 256 boxes" in err()
    assert plan(conf, [good[0][:3]] * 3, n=257)[0] == EINVAL and "1 .. 256 boxes" in err()
    for place in (0, 1, 2):
        at = "box %d: " % place
        bad = list(good)
        bad[place] = (31, (0, 0, 0), (1, 1, 1))
        assert plan(conf, bad)[0] == EINVAL and err() == at + "tile level 31 is outside 0 .. 30"
        bad[place] = (-1, (0, 0, 0), (1, 1, 1))
        assert plan(conf, bad)[0] == EINVAL and at in err()
        bad[place] = (1, (30, 0, 0), (4, 4, 4))  # (33 coarse planes)
        assert plan(conf, bad)[0] == EINVAL and at in err() and "leaves dimension 0 (extent 33)" in err()
        bad[place] = (0, (0, 0, 0), (2, 0, 2))
        assert plan(conf, bad)[0] == EINVAL and at in err() and "extent 0" in err()
        bad[place] = good[place] + (None, None, 7)
        assert plan(conf, bad)[0] == EINVAL and at in err() and "reserved" in err()
        # the outputs' rules
        bad[place] = good[place][:3] + (5, None, BASE - 4096)
        assert plan(conf, bad)[0] == EINVAL and at in err() and "d_index is NULL" in err()
        bad[place] = good[place][:3] + (0, None, BASE - 4096)
        assert plan(conf, bad)[0] == EINVAL and at in err() and "d_value" in err() and "capacity of 0" in err()
        bad[place] = good[place][:3] + (0, BASE - 4096, None)  # (an index array that is not used is no error)
        assert plan(conf, bad)[0] == 0, err()
        bad[place] = good[place][:3] + (5, BASE - 4096, None)  # (indices only)
        assert plan(conf, bad)[0] == 0, err()
        bad[place] = good[place][:3] + (5, BASE - 4096 + 4, None)
        assert plan(conf, bad)[0] == EINVAL and at in err() and "aligned" in err()
        bad[place] = good[place][:3] + (5, BASE - 4096, BASE - 2048 + 2)
        assert plan(conf, bad)[0] == EINVAL and at in err() and "aligned" in err()
    # two boxes' outputs: index against index, value against value, ranges of non-zero capacity only
    far = 1 << 41
    a = good[0][:3] + (8, far, far + 4096)
    for place in (1, 2):
        bad = [a] + list(good[1:])
        bad[place] = good[place][:3] + (4, far + 56, far + 8192)  # (the last index word of box 0)
        assert plan(conf, bad)[0] == EINVAL and err().startswith("box %d: the output overlaps box 0's" % place) and "d_index" in err()
        bad[place] = good[place][:3] + (4, far + 64, far + 8192)
        assert plan(conf, bad)[0] == 0, err()
        bad[place] = good[place][:3] + (4, far + 1024, far + 4096 + 28)  # (the last value of box 0, 4 bytes each)
        assert plan(conf, bad)[0] == EINVAL and err().startswith("box %d: the output overlaps box 0's" % place) and "d_value" in err()
        assert plan(conf, bad, dtype=1)[0] == EINVAL
        bad[place] = good[place][:3] + (4, far + 1024, far + 4096 + 32)
        assert plan(conf, bad)[0] == 0, err()
        assert plan(conf, bad, dtype=1)[0] == EINVAL and "d_value" in err()  # (8 bytes each: box 0's values reach 64 bytes)
        bad[place] = good[place][:3] + (0, far, None)  # (capacity 0: not compared)
        assert plan(conf, bad)[0] == 0, err()
        bad[place] = good[place][:3] + (4, far + 4096, far + 1024)  # (an index array over a value array is not this check's business)
        assert plan(conf, bad)[0] == 0, err()
    # the options
    assert plan(conf, good, opts=None)[0] == EINVAL and "opts" in err()
    assert plan(conf, good, opts=opts_of(math.nan, 1.0))[0] == EINVAL and "lo is NaN" in err()
    assert plan(conf, good, opts=opts_of(0.0, math.nan))[0] == EINVAL and "hi is NaN" in err()
    assert plan(conf, good, opts=opts_of(0.0, 1.0, flags=4))[0] == EINVAL and "flags" in err()
    assert plan(conf, good, opts=opts_of(0.0, 1.0, flags=7))[0] == EINVAL and "flags" in err()
    assert plan(conf, good, opts=opts_of(0.0, 1.0, reserved=1))[0] == EINVAL and "reserved" in err()
    for lo, hi, flags in [(1.0, 0.0, 0), (math.inf, math.inf, 0), (-math.inf, math.inf, 3), (2.0, 1.0, 2)]:  # (valid: empty ranges, infinite ends)
        assert plan(conf, good, opts=opts_of(lo, hi, flags))[0] == 0, err()
    for dt in range(2, 10):  # integer element types: the partial calls' code and wording
        assert plan(conf, good, dtype=dt)[0] == EUNSUPPORTED
        assert err() == "the region decode reads float / double arrays; integer element types are not supported yet"
    assert plan(conf, good, dtype=10)[0] == EUNSUPPORTED and "dataType" in err()
    assert plan(conf_for(shape, interpAnchorStride=24), good)[0] == EUNSUPPORTED and "power of two" in err()


def test_select_refuses_a_null_handle_and_null_heads():
    arr = reqs_of([(0, (0,), (1,))], 1)
    heads = (sz3_amd._CSelectHead * 1)()  # (never written: the handle is refused first)
    o = opts_of()
    assert L.sz3hip_stream_select(None, arr, 1, C.byref(o), C.byref(heads), None) == EINVAL and "no handle" in err()
    assert L.sz3hip_stream_select(None, arr, 1, C.byref(o), None, None) == EINVAL and "d_heads" in err()
    dims = (C.c_uint64 * 1)(4)
    assert L.sz3hip_select_device(0, 1, dims, None, None, C.byref(o), None, None, 0, None, None) == EINVAL and "d_head" in err()
    assert L.sz3hip_select_device(7, 1, dims, None, None, C.byref(o), None, None, 0, C.byref(heads), None) == EUNSUPPORTED
    assert L.sz3hip_select_device(0, 5, dims, None, None, C.byref(o), None, None, 0, C.byref(heads), None) == EINVAL and "dimension count" in err()
    assert L.sz3hip_select_device(0, 1, dims, None, None, None, None, None, 0, C.byref(heads), None) == EINVAL and "opts" in err()
    assert L.sz3hip_select_device(0, 1, dims, None, None, C.byref(o), None, None, 3, C.byref(heads), None) == EINVAL and "d_index is NULL" in err()
    assert L.sz3hip_select_device(0, 1, dims, None, None, C.byref(o), None, BASE, 0, C.byref(heads), None) == EINVAL and "capacity of 0" in err()
    assert bytes(heads) == bytes(32)


def test_python_names_and_signatures():
    p = inspect.signature(sz3_amd.Stream.select).parameters
    assert list(p) == ["self", "items", "lo", "hi", "capacity", "invert", "nan", "values", "stream"]
    assert (p["invert"].default, p["nan"].default, p["values"].default, p["stream"].default) == (False, False, True, None)
    p = inspect.signature(sz3_amd.select_points).parameters
    assert list(p) == ["tensor", "lo", "hi", "capacity", "invert", "nan", "values", "stream"]
    assert (p["invert"].default, p["nan"].default, p["values"].default, p["stream"].default) == (False, False, True, None)
    p = inspect.signature(sz3_amd.select_plan).parameters
    assert list(p)[:3] == ["conf", "dtype", "items"]
    assert callable(sz3_amd.SelectResult.numpy)
    with pytest.raises(ValueError):
        sz3_amd.select_plan(conf_for((9, 9)), "float32", [(0, (0, 0), (2, 2), None)])  # (a select item names no output)
    with pytest.raises(ValueError):
        sz3_amd.select_plan(conf_for((9, 9)), "float32", [(0, (0, 0), (2, 2))], capacity=[1, 2])
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.select_plan(conf_for((9, 9)), "float32", [(0, (0, 0), (2, 2))], lo=math.nan)
    assert e.value.code == EINVAL
    with pytest.raises(TypeError):
        sz3_amd.select_points([1.0, 2.0], 0.0, 1.0, 4)

"""Boxes sampled at fractional positions, without a GPU: the symbols and constants, the three structs' layout against
the header, the plan — a pure host function — against the request's plan, every refusal that comes before anything touches a device, and
the Python names and signatures. Pointers here are numbers: the plan never reads or writes them."""
import ctypes as C
import inspect
import math
import re

import pytest

import sz3_amd
from test_request_cpu import BASE, EINVAL, EUNSUPPORTED, HEADER, IDS, SHAPES, boxes_at, conf_for, err

L = sz3_amd.lib()
SYMBOLS = ("sz3hip_stream_sample", "sz3hip_sample_plan_for", "sz3hip_sample_device")
CONSTANTS = {"SZ3HIP_SAMPLE_NEAREST": 0, "SZ3HIP_SAMPLE_LINEAR": 1, "SZ3HIP_SAMPLE_CLAMP": 1}
COORDS = 1 << 38  # a made-up device address of coordinates
SHAPE = (65, 47, 130)
GOOD = [(0, (0, 0, 0), (4, 5, 6)), (1, (1, 1, 1), (4, 5, 6)), (2, (2, 1, 0), (3, 3, 8)), (0, (9, 9, 9), (1, 1, 1)), (3, (0, 0, 0), (2, 2, 2))]
LATTICE = dict(counts=(2, 3, 4), origin=(0.5, 0.25, 0.0), steps=((0.5, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.5)))


def c_struct(name, txt):
    """the fields of a typedef'd struct of the header as (name, ctypes type), pointers as c_void_p, arrays of one and two dimensions included"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "double": C.c_double, "sz3hip_box": sz3_amd._CBox,
             "void": None}
    out = []
    for decl in body.split(";"):
        decl = re.sub(r"\bconst\b", "", decl).strip()
        if not decl:
            continue
        m = re.match(r"(\w+)\s*(.*)$", decl)
        for var in m.group(2).split(","):
            a = re.match(r"\s*(\*?)\s*(\w+)\s*((?:\[\d+\])*)\s*$", var)
            t = C.c_void_p if a.group(1) else ctype[m.group(1)]
            for d in reversed(re.findall(r"\[(\d+)\]", a.group(3))):
                t = t * int(d)
            out.append((a.group(2), t))
    return out


def reqs_of(items, N, esz=4, queries=None):
    """items: (level, lo, shape) -> the sz3hip_sample_req array: 7 points at COORDS each, contiguous outputs one after the other; queries[i]
    (a dict of fields) overrides box i's"""
    arr = (sz3_amd._CSampleReq * max(len(items), 1))()
    at = BASE
    for i, it in enumerate(items):
        r = arr[i]
        r.level = it[0]
        r.box.lo[:N] = it[1]
        r.box.ext[:N] = it[2]
        over = (queries or {}).get(i, {})
        q = dict(d_coords=COORDS + 4096 * i, n_points=7)
        if "counts" in over:  # (the lattice form, unless the override says otherwise)
            q = dict(d_coords=None, n_points=over["counts"][0] * over["counts"][1] * over["counts"][2])
        q.update(over)
        r.d_coords = q["d_coords"]
        r.n_points = q["n_points"]
        r.reserved = q.get("reserved", 0)
        if "counts" in q:
            r.counts[:] = q["counts"]
        if "origin" in q:
            r.origin[:len(q["origin"])] = q["origin"]
        for a, st in enumerate(q.get("steps", ())):
            r.steps[a][:len(st)] = st
        r.d_out = q["d_out"] if "d_out" in q else at
        at += (r.n_points * esz + 255) & ~255 if r.n_points < (1 << 32) else 256
    return arr


def opts_of(filter=1, coord_type=1, flags=0, reserved=0, fill=float("nan")):
    o = sz3_amd._CSampleOpts()
    o.filter, o.coord_type, o.flags, o.reserved, o.fill = filter, coord_type, flags, reserved, fill
    return o


DEFAULT = object()


def plan(conf, items, dtype=0, n=None, opts=DEFAULT, queries=None):
    p = sz3_amd._CSamplePlan()
    o = opts_of() if opts is DEFAULT else opts
    arr = reqs_of(items, conf.N, 4 if dtype == 0 else 8, queries)
    rc = L.sz3hip_sample_plan_for(C.byref(conf._c), dtype, arr, len(items) if n is None else n, None if o is None else C.byref(o), C.byref(p))
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
        assert re.search(r"#define\s+%s\s+%du\b" % (name, v), txt), name
    assert (sz3_amd.SAMPLE_NEAREST, sz3_amd.SAMPLE_LINEAR, sz3_amd.SAMPLE_CLAMP) == (0, 1, 1)


@pytest.mark.parametrize("name,cls,size", [("sz3hip_sample_req", "_CSampleReq", 248), ("sz3hip_sample_opts", "_CSampleOpts", 24),
                                           ("sz3hip_sample_plan", "_CSamplePlan", 40)])
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
    N = len(shape)
    lattice = dict(counts=(2, 3, 4), origin=(0.0,) * N, steps=((0.0,) * N,) * 3)
    queries = {i: (lattice if i % 3 == 1 else dict(n_points=1 + 100 * i)) for i in range(len(boxes))}
    for filt, ct, flags in ((0, 0, 0), (1, 1, 1)):
        rc, p = plan(conf, boxes, dtype=dtype, opts=opts_of(filt, ct, flags), queries=queries)
        assert rc == 0, err()
        name = "float32" if dtype == 0 else "float64"
        want = sz3_amd.request_plan(conf, name, boxes)
        got = {k: getattr(p, k) for k, _ in sz3_amd._CSamplePlan._fields_}
        n_queries = sum(24 if i % 3 == 1 else 1 + 100 * i for i in range(len(boxes)))
        assert got == dict(want, queries=n_queries)
        py = [((0.0,) * N, ((0.0,) * N,) * 3, (2, 3, 4)) if i % 3 == 1 else 1 + 100 * i for i in range(len(boxes))]
        assert sz3_amd.sample_plan(conf, name, boxes, py, mode="nearest" if filt == 0 else "linear", clamp=bool(flags)) == got


def test_refusals_of_the_options():
    conf = conf_for(SHAPE)
    assert plan(conf, GOOD)[0] == 0, err()
    refused(conf, GOOD, "NULL argument (opts)", opts=None)
    for bad in (2, 255):
        refused(conf, GOOD, "filter", opts=opts_of(filter=bad))
        refused(conf, GOOD, "coord_type", opts=opts_of(coord_type=bad))
    for bad in (2, 3, 1 << 31):
        refused(conf, GOOD, "flags", opts=opts_of(flags=bad))
    refused(conf, GOOD, "reserved", opts=opts_of(reserved=1))
    for fill in (float("nan"), float("inf"), -float("inf"), 1e308, -0.0, 5e-324):  # fill is any double
        assert plan(conf, GOOD, opts=opts_of(fill=fill))[0] == 0, err()
    for filt in (0, 1):
        for ct in (0, 1):
            for flags in (0, 1):
                assert plan(conf, GOOD, opts=opts_of(filt, ct, flags))[0] == 0, err()


def test_refusals_of_the_boxes_and_queries():
    """sz3hip_stream_request's own, with its wording, and the queries': each at the first, a middle and the last box"""
    conf = conf_for(SHAPE)
    n = len(GOOD)
    refused(conf, [], "", n=0)
    refused(conf, GOOD * 60, "", n=257)
    inf, nan = float("inf"), float("nan")
    for b in (0, n // 2, n - 1):
        def edit(item):
            items = list(GOOD)
            items[b] = item
            return items
        k, lo, ext = GOOD[b]
        at = "box %d: " % b
        refused(conf, edit((31, lo, ext)), at)
        refused(conf, edit((-1, lo, ext)), at)
        refused(conf, edit((k, (1 << 40, 0, 0), ext)), at)
        refused(conf, edit((k, lo, (0, 1, 1))), at)
        refused(conf, edit((k, lo, (66, 1, 1))), at)
        refused(conf, GOOD, at + "the reserved word is 7", queries={b: dict(reserved=7)})
        # the output
        refused(conf, GOOD, at + "the output array is NULL", queries={b: dict(d_out=None)})
        for dtype, offs in ((0, (1, 2, 3)), (1, (1, 2, 4, 7))):
            for off in offs:
                refused(conf, GOOD, at + "the output is not aligned to its element size (%d bytes)" % (4 if dtype == 0 else 8), dtype=dtype,
                        queries={b: dict(d_out=BASE + (1 << 30) + off)})
        assert plan(conf, GOOD, dtype=0, queries={b: dict(d_out=BASE + (1 << 30) + 4)})[0] == 0, err()
        # n_points
        refused(conf, GOOD, at + "n_points is 0", queries={b: dict(n_points=0)})
        refused(conf, GOOD, at + "n_points is %d" % ((1 << 31) + 1), queries={b: dict(n_points=(1 << 31) + 1, d_out=BASE + (1 << 50))})
        assert plan(conf, GOOD, queries={b: dict(n_points=1 << 31, d_out=BASE + (1 << 50))})[0] == 0, err()
        assert plan(conf, GOOD, queries={b: dict(n_points=1)})[0] == 0, err()
        # the points form: the coordinates' alignment is their type's; nothing of a lattice beside them
        for ct, offs in ((0, (1, 2, 3)), (1, (1, 2, 4))):
            for off in offs:
                refused(conf, GOOD, at + "d_coords is not aligned to its coordinate size (%d bytes)" % (4 if ct == 0 else 8), opts=opts_of(coord_type=ct),
                        queries={b: dict(d_coords=COORDS + off)})
        assert plan(conf, GOOD, opts=opts_of(coord_type=0), queries={b: dict(d_coords=COORDS + 4)})[0] == 0, err()
        for extra in (dict(counts=(1, 0, 0)), dict(counts=(0, 0, 7)), dict(origin=(0.0, 0.0, 1.0)), dict(origin=(0.0, 0.0, 0.0, 1.0)), dict(origin=(nan,)),
                      dict(steps=((0.0, 1.0, 0.0),)), dict(steps=((0.0,), (0.0,), (0.0, 0.0, 0.0, 0.5)))):
            refused(conf, GOOD, at + "d_coords is given with a lattice", queries={b: dict(extra, d_coords=COORDS, n_points=7)})
        # the lattice form
        assert plan(conf, GOOD, queries={b: LATTICE})[0] == 0, err()
        for a in range(3):
            counts = list(LATTICE["counts"])
            counts[a] = 0
            refused(conf, GOOD, at + "the lattice's count of axis %d is 0" % a, queries={b: dict(LATTICE, counts=tuple(counts), n_points=24)})
        refused(conf, GOOD, at + "the lattice's counts (2 x 3 x 4) do not multiply to n_points (23)", queries={b: dict(LATTICE, n_points=23)})
        refused(conf, GOOD, at + "the lattice's counts (2147483648 x 2147483648 x 4) do not multiply to n_points (4)", queries={b: dict(LATTICE, counts=(1 << 31, 1 << 31, 4), n_points=4)})
        refused(conf, GOOD, at + "the lattice's counts", queries={b: dict(LATTICE, counts=(1 << 63, 2, 1), n_points=1)})
        for bad in (inf, -inf, nan):
            for j in range(3):
                origin = list(LATTICE["origin"])
                origin[j] = bad
                refused(conf, GOOD, at + "the lattice's origin[%d] is not finite" % j, queries={b: dict(LATTICE, origin=tuple(origin))})
                for a in range(3):
                    steps = [list(s) for s in LATTICE["steps"]]
                    steps[a][j] = bad
                    refused(conf, GOOD, at + "the lattice's steps[%d][%d] is not finite" % (a, j), queries={b: dict(LATTICE, steps=steps)})
        # (an entry beyond the N used is not looked at)
        assert plan(conf, GOOD, queries={b: dict(LATTICE, origin=LATTICE["origin"] + (nan,))})[0] == 0, err()
    arr = reqs_of(GOOD, 3)
    p = sz3_amd._CSamplePlan()
    o = opts_of()
    assert L.sz3hip_sample_plan_for(C.byref(conf._c), 0, None, n, C.byref(o), C.byref(p)) == EINVAL
    assert L.sz3hip_sample_plan_for(C.byref(conf._c), 0, arr, n, C.byref(o), C.byref(p)) == 0


def test_output_overlap():
    conf = conf_for(SHAPE)
    at = BASE + (1 << 20)
    n = len(GOOD)
    for dtype, e in ((0, 4), (1, 8)):
        for i, j in ((1, 0), (n // 2, 1), (n - 1, n // 2), (n - 1, 0)):
            def q(pi, pj):
                return {i: dict(n_points=10, d_out=pi), j: dict(n_points=7, d_out=pj)}
            # box j's 7 elements right in front of box i's 10, and the other way round: apart; one element closer: they meet
            assert plan(conf, GOOD, dtype=dtype, queries=q(at + 7 * e, at))[0] == 0, err()
            assert plan(conf, GOOD, dtype=dtype, queries=q(at, at + 10 * e))[0] == 0, err()
            refused(conf, GOOD, "box %d: the output overlaps box %d's" % (i, j), dtype=dtype, queries=q(at + 6 * e, at))
            refused(conf, GOOD, "box %d: the output overlaps box %d's" % (i, j), dtype=dtype, queries=q(at, at + 9 * e))
            refused(conf, GOOD, "box %d: the output overlaps box %d's" % (i, j), dtype=dtype, queries=q(at, at))
    # repeated and overlapping BOXES are allowed
    assert plan(conf, [GOOD[0], GOOD[0], GOOD[1], GOOD[0]])[0] == 0, err()


def test_integer_types_and_null_arguments():
    conf = conf_for(SHAPE)
    for dt in range(2, 10):
        rc, _ = plan(conf, GOOD, dtype=dt)
        assert rc == EUNSUPPORTED and "integer element types are not supported yet" in err()
    refused(conf, GOOD, "dataType", code=EUNSUPPORTED, dtype=10)
    p = sz3_amd._CSamplePlan()
    o = opts_of()
    arr = reqs_of(GOOD, 3)
    assert L.sz3hip_sample_plan_for(None, 0, arr, len(GOOD), C.byref(o), C.byref(p)) == EINVAL and "NULL argument (conf)" in err()
    assert L.sz3hip_sample_plan_for(C.byref(conf._c), 0, arr, len(GOOD), C.byref(o), None) == EINVAL and "NULL argument (out)" in err()
    assert L.sz3hip_stream_sample(None, arr, len(GOOD), C.byref(o), None) == EINVAL and "no handle" in err()
    dims = (C.c_uint64 * 1)(8)
    one = reqs_of([(0, (0,), (0,))], 1)
    for dt in range(2, 10):  # sz3hip_sample_device refuses integers before it looks at a pointer
        assert L.sz3hip_sample_device(dt, 1, dims, BASE, None, C.byref(o), one, None) == EUNSUPPORTED
        assert "integer element types are not supported yet" in err()
    assert L.sz3hip_sample_device(0, 5, dims, BASE, None, C.byref(o), one, None) == EINVAL and "dimension count" in err()
    assert L.sz3hip_sample_device(0, 1, dims, BASE, None, C.byref(o), None, None) == EINVAL and "query" in err()
    assert L.sz3hip_sample_device(0, 1, dims, BASE, None, None, one, None) == EINVAL and "opts" in err()
    # the view is the box: level, reserved and box stay zero
    for field, v in (("level", 1), ("reserved", 1)):
        q = reqs_of([(0, (0,), (0,))], 1)
        setattr(q[0], field, v)
        assert L.sz3hip_sample_device(0, 1, dims, BASE, None, C.byref(o), q, None) == EINVAL and "must be 0" in err()
    for item in ((0, (1,), (0,)), (0, (0,), (8,))):
        assert L.sz3hip_sample_device(0, 1, dims, BASE, None, C.byref(o), reqs_of([item], 1), None) == EINVAL and "must be 0" in err()
    # ... and the query's own rules hold, without "box <i>: " in front
    for q, fragment in ((dict(n_points=0), "n_points is 0"), (dict(d_out=None), "the output array is NULL"), (dict(d_out=BASE + 2), "not aligned"),
                        (dict(d_coords=COORDS + 4), "d_coords is not aligned"), (dict(counts=(1, 2, 3), n_points=7), "do not multiply"),
                        (dict(counts=(1, 1, 7), origin=(float("inf"),)), "origin[0] is not finite")):
        assert L.sz3hip_sample_device(0, 1, dims, BASE, None, C.byref(o), reqs_of([(0, (0,), (0,))], 1, queries={0: q}), None) == EINVAL
        assert fragment in err() and not err().startswith("box"), err()


def test_python_names_and_signatures():
    p = inspect.signature(sz3_amd.Stream.sample).parameters
    assert list(p) == ["self", "items", "queries", "mode", "clamp", "fill", "stream"]
    assert (p["mode"].default, p["clamp"].default, p["stream"].default) == ("linear", False, None) and math.isnan(p["fill"].default)
    p = inspect.signature(sz3_amd.sample_points).parameters
    assert list(p) == ["tensor", "query", "mode", "clamp", "fill", "stream"] and p["mode"].default == "linear" and math.isnan(p["fill"].default)
    p = inspect.signature(sz3_amd.sample_plan).parameters
    assert list(p)[:4] == ["conf", "dtype", "items", "queries"]
    conf = conf_for(SHAPE)
    lattice = ((0.0, 0.0, 0.0), ((0.0, 0.5, 0.0), (0.0, 0.0, 0.25)), (5, 9))  # two axes: rows and columns
    got = sz3_amd.sample_plan(conf, "float32", GOOD, [3, lattice, 1, 1, 1])
    assert got["n"] == len(GOOD) and got["queries"] == 3 + 45 + 3
    for mode in ("nearest", "LINEAR", 0, 1):
        assert sz3_amd.sample_plan(conf, "float64", GOOD, [1] * len(GOOD), mode=mode)["queries"] == len(GOOD)
    with pytest.raises(ValueError):
        sz3_amd.sample_plan(conf, "float32", GOOD, [1] * len(GOOD), mode="cubic")
    with pytest.raises(ValueError):
        sz3_amd.sample_plan(conf, "float32", GOOD, [1])
    with pytest.raises(ValueError):
        sz3_amd.sample_plan(conf, "float32", GOOD[:1], [((0.0, 0.0), ((0.0, 0.0, 1.0),), (4,))])
    with pytest.raises(sz3_amd.SZ3HipError):
        sz3_amd.sample_plan(conf, "float32", GOOD[:1], [0])
    with pytest.raises(TypeError):
        sz3_amd.sample_points([1.0, 2.0], None)

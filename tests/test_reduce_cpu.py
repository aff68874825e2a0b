"""Per-box statistics of an opened stream, without a GPU: the symbols, the four structs' layout against the header, the
plan — a pure host function — against the request's plan and the partition rule, every refusal that comes before anything touches a device,
and the Python names and signatures."""
import ctypes as C
import inspect
import math
import re

import pytest

import sz3_amd
from test_request_cpu import EINVAL, EUNSUPPORTED, HEADER, IDS, SHAPES, boxes_at, conf_for, err

L = sz3_amd.lib()
SYMBOLS = ("sz3hip_stream_reduce", "sz3hip_reduce_plan_for", "sz3hip_reduce_device")
CHUNK = 4096  # the partition rule: a partial record per 4096 consecutive row-major indices of a box


def c_struct(name, txt):
    """the fields of a typedef'd struct of the header as (name, ctypes type) (test_request_cpu.c_struct, with double)"""
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
            a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", var)
            out.append((a.group(1), ctype[m.group(1)] * int(a.group(2)) if a.group(2) else ctype[m.group(1)]))
    return out


def reqs_of(items, N):
    """items: (level, lo, shape[, reserved]) -> the sz3hip_reduce_req array"""
    arr = (sz3_amd._CReduceReq * max(len(items), 1))()
    for i, it in enumerate(items):
        arr[i].level = it[0]
        arr[i].box.lo[:N] = it[1]
        arr[i].box.ext[:N] = it[2]
        if len(it) > 3:
            arr[i].reserved = it[3]
    return arr


def opts_of(nbins=0, lo=0.0, hi=0.0, reserved=0):
    o = sz3_amd._CReduceOpts()
    o.nbins, o.lo, o.hi, o.reserved = nbins, lo, hi, reserved
    return o


def plan(conf, items, dtype=0, n=None, opts=None):
    p = sz3_amd._CReducePlan()
    rc = L.sz3hip_reduce_plan_for(C.byref(conf._c), dtype, reqs_of(items, conf.N), len(items) if n is None else n, None if opts is None else C.byref(opts), C.byref(p))
    return rc, p


def test_symbols_exist():
    with open(HEADER) as f:
        txt = f.read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert re.search(r"\b%s\(" % sym, txt), "%s is not declared in include/sz3hip.h" % sym
    assert re.search(r"#define\s+SZ3HIP_MAX_BINS\s+1024\b", txt)


@pytest.mark.parametrize("name,cls,size", [("sz3hip_box_stats", "_CBoxStats", 88), ("sz3hip_reduce_req", "_CReduceReq", 72), ("sz3hip_reduce_opts", "_CReduceOpts", 24),
                                           ("sz3hip_reduce_plan", "_CReducePlan", 48)])
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


def test_the_structured_dtype_is_the_struct():
    assert sz3_amd.BOX_STATS_DTYPE.itemsize == 88
    assert list(sz3_amd.BOX_STATS_DTYPE.names) == [n for n, _ in sz3_amd._CBoxStats._fields_]


@pytest.mark.parametrize("nbins", [0, 7, 1024])
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "cubic"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plan(shape, interp, nbins):
    conf = conf_for(shape, interpAlgo=interp)
    items = [(k, lo, ext) for k in (2, 0, 3, 1) for lo, ext in boxes_at(shape, k)]
    rc, p = plan(conf, items, opts=opts_of(nbins, -1.0, 1.0))
    assert rc == 0, err()
    want = sz3_amd.request_plan(conf, "float32", items)
    assert (p.n, p.finest_level, p.coarsest_level, p.n_levels, p.points) == tuple(want[k] for k in ("n", "finest_level", "coarsest_level", "n_levels", "points"))
    chunks = sum(-(-math.prod(ext) // CHUNK) for _, _, ext in items)
    assert p.partials == chunks
    assert p.hist_words == (len(items) * (nbins + 2) if nbins else 0)
    # the level buffers, then the partial records (64 bytes each) on an 8-byte boundary
    assert want["scratch_elems"] + 16 * chunks <= p.scratch_elems <= want["scratch_elems"] + 16 * chunks + 1
    rc, p8 = plan(conf, items, dtype=1, opts=opts_of(nbins, -1.0, 1.0))
    assert rc == 0 and p8.scratch_elems == want["scratch_elems"] + 8 * chunks and p8.partials == chunks
    rc, p0 = plan(conf, items)  # (no options: no histogram)
    assert rc == 0 and p0.hist_words == 0 and p0.partials == chunks
    assert sz3_amd.reduce_plan(conf, "float32", items, bins=nbins, lo=-1.0, hi=1.0) == {k: getattr(p, k) for k, _ in sz3_amd._CReducePlan._fields_}


def test_refusals():
    shape = (65, 47, 130)
    conf = conf_for(shape)
    good = [(2, (0, 0, 0), (4, 4, 4)), (0, (1, 3, 5), (6, 5, 4)), (1, (0, 0, 0), (3, 3, 3))]
    assert plan(conf, good)[0] == 0
    out = sz3_amd._CReducePlan()
    arr = reqs_of(good, 3)
    assert L.sz3hip_reduce_plan_for(None, 0, arr, 3, None, C.byref(out)) == EINVAL and "conf" in err()
    assert L.sz3hip_reduce_plan_for(C.byref(conf._c), 0, None, 3, None, C.byref(out)) == EINVAL and "NULL" in err()
    assert L.sz3hip_reduce_plan_for(C.byref(conf._c), 0, arr, 3, None, None) == EINVAL and "out" in err()
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
        bad[place] = good[place] + (7,)
        assert plan(conf, bad)[0] == EINVAL and "box %d: " % place in err() and "reserved" in err()
    # the options
    assert plan(conf, good, opts=opts_of(0, 0.0, 0.0))[0] == 0  # (no histogram: the range is not read)
    assert plan(conf, good, opts=opts_of(1024, 0.0, 1.0))[0] == 0
    assert plan(conf, good, opts=opts_of(0, 0.0, 0.0, reserved=1))[0] == EINVAL and "reserved" in err()
    assert plan(conf, good, opts=opts_of(8, 0.0, 1.0, reserved=1))[0] == EINVAL and "reserved" in err()
    assert plan(conf, good, opts=opts_of(1025, 0.0, 1.0))[0] == EINVAL and "1025 bins" in err()
    assert plan(conf, good, opts=opts_of(8, 1.0, 1.0))[0] == EINVAL and "hi must be above lo" in err()
    assert plan(conf, good, opts=opts_of(8, 1.0, 0.5))[0] == EINVAL and "hi must be above lo" in err()
    for lo, hi in [(math.nan, 1.0), (0.0, math.nan), (-math.inf, 1.0), (0.0, math.inf)]:
        assert plan(conf, good, opts=opts_of(8, lo, hi))[0] == EINVAL and "not finite" in err()
    for dt in range(2, 10):  # integer element types: the partial calls' code and wording
        assert plan(conf, good, dtype=dt)[0] == EUNSUPPORTED
        assert err() == "the region decode reads float / double arrays; integer element types are not supported yet"
    assert plan(conf, good, dtype=10)[0] == EUNSUPPORTED and "dataType" in err()
    assert plan(conf_for(shape, interpAnchorStride=24), good)[0] == EUNSUPPORTED and "power of two" in err()


def test_reduce_refuses_a_null_handle_and_null_stats():
    arr = reqs_of([(0, (0,), (1,))], 1)
    stats = (sz3_amd._CBoxStats * 1)()  # (never written: the handle is refused first)
    assert L.sz3hip_stream_reduce(None, arr, 1, None, C.byref(stats), None, None) == EINVAL and "no handle" in err()
    assert L.sz3hip_stream_reduce(None, arr, 1, None, None, None, None) == EINVAL and "d_stats" in err()
    dims = (C.c_uint64 * 1)(4)
    assert L.sz3hip_reduce_device(0, 1, dims, None, None, None, None, None, None) == EINVAL and "d_stats" in err()
    assert L.sz3hip_reduce_device(7, 1, dims, None, None, None, C.byref(stats), None, None) == EUNSUPPORTED
    assert L.sz3hip_reduce_device(0, 5, dims, None, None, None, C.byref(stats), None, None) == EINVAL and "dimension count" in err()


def test_python_names_and_signatures():
    p = inspect.signature(sz3_amd.Stream.reduce).parameters
    assert list(p) == ["self", "items", "bins", "lo", "hi", "stream"]
    assert (p["bins"].default, p["lo"].default, p["hi"].default, p["stream"].default) == (0, 0.0, 0.0, None)
    p = inspect.signature(sz3_amd.reduce_plan).parameters
    assert list(p) == ["conf", "dtype", "items", "bins", "lo", "hi"] and p["bins"].default == 0
    p = inspect.signature(sz3_amd.reduce_stats).parameters
    assert list(p)[:2] == ["tensor", "bins"] and p["bins"].default == 0 and p["stream"].default is None
    assert callable(sz3_amd.ReduceResult.numpy)
    with pytest.raises(ValueError):
        sz3_amd.reduce_plan(conf_for((9, 9)), "float32", [(0, (0, 0), (2, 2), None)])  # (a reduce item names no output)
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.reduce_plan(conf_for((9, 9)), "float32", [(0, (0, 0), (2, 2))], bins=4, lo=1.0, hi=1.0)
    assert e.value.code == EINVAL

#!/usr/bin/env python3
"""Generates tests/golden/stream_errors.json: what the opened stream's calls answer to faulty arguments — the return code and the whole
sz3hip_last_error text — for every call that fails before it touches a device: the eight *_plan_for, the eight sz3hip_stream_* and
sz3hip_stream_tiles with a NULL handle, and the seven *_device calls for the faults up to the input view's strides. Single faults, and
pairs of faults whose precedence the table pins. tests/test_stream_errors_cpu.py replays every case against the current build.

One conf, (40, 48, 56) float32 with the default interpolation; output addresses are placeholders from 1 << 40 upward (no call here reads
or writes them). LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the committed table is the answer of the commit BEFORE a
change of these calls, made from a build of that commit; regenerated from the changed tree it must come out byte-identical.

    LAB_PKG=<dir of the build to record> python tests/golden/make_stream_errors.py          # writes tests/golden/stream_errors.json
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "stream_errors.json")

SHAPE = (40, 48, 56)
BASE = 1 << 40   # placeholder output addresses, 4096 apart
LUT = 1 << 39    # a placeholder table
INF, NAN = float("inf"), float("nan")
KINDS = ("request", "reduce", "select", "map", "sample", "project", "gradient", "composite")
TILE_KINDS = ("request", "map", "project", "gradient", "composite")  # their boxes are sz3hip_tile_req with a view each

# ---- the faults: the options' (a dict of fields over the valid options; None: no options at all) ... ------------------------------------
OPTS = {
    "reduce": dict(nbins=8, lo=0.0, hi=1.0),
    "select": dict(lo=0.25, hi=0.75),
    "map": dict(out_type=2, lo=0.0, hi=1.0),  # U16: an output element of two bytes can be misaligned
    "sample": dict(filter=1, coord_type=0),
    "project": dict(op=1, axis=1),
    "gradient": dict(op=2, spacing=(1.0, 1.0, 1.0, 1.0)),
    "composite": dict(lo=0.0, hi=1.0, cutoff=INF, axis=1, lut_n=16, d_lut=LUT),
}
OPT_FAULTS = {  # every refusal of every *_opts check; the first one of a kind is its "bad options" in the pairs
    "reduce": [("reserved", dict(reserved=3)), ("bins", dict(nbins=1 << 20)), ("not_finite", dict(hi=INF)), ("nan", dict(lo=NAN)), ("empty", dict(hi=0.0))],
    "select": [("reserved", dict(reserved=3)), ("null", None), ("flags", dict(flags=4)), ("lo_nan", dict(lo=NAN)), ("hi_nan", dict(hi=NAN))],
    "map": [("flags", dict(flags=1)), ("null", None), ("type_0", dict(out_type=0)), ("type_6", dict(out_type=6)), ("reserved", dict(reserved=1)),
            ("f16_window", dict(out_type=3)), ("f32_table", dict(out_type=4, lo=0.0, hi=0.0, lut_n=4)), ("not_finite", dict(lo=-INF)), ("empty", dict(hi=0.0)),
            ("too_wide", dict(lo=-1.5e308, hi=1.5e308)), ("lut_1", dict(out_type=5, lut_n=1, d_lut=LUT)), ("lut_many", dict(out_type=5, lut_n=1025, d_lut=LUT)),
            ("lut_null", dict(out_type=5, lut_n=16)), ("lut_misaligned", dict(out_type=5, lut_n=16, d_lut=LUT + 2)), ("table_not_taken", dict(lut_n=4)),
            ("nan_code", dict(nan_code=65536))],
    "sample": [("filter", dict(filter=2)), ("null", None), ("coord_type", dict(coord_type=2)), ("flags", dict(flags=2)), ("reserved", dict(reserved=1))],
    "project": [("op", dict(op=7)), ("null", None), ("out_type", dict(out_type=2)), ("index_out_type", dict(op=4, out_type=1)), ("reserved", dict(reserved=1))],
    "gradient": [("op", dict(op=4)), ("null", None), ("axis_not_read", dict(axis=1)), ("out_type", dict(out_type=2)), ("flags", dict(flags=2))],
    "composite": [("out_type", dict(out_type=2)), ("null", None), ("flags", dict(flags=8)), ("reserved", dict(reserved=1)), ("not_finite", dict(hi=INF)),
                  ("empty", dict(hi=-1.0)), ("too_wide", dict(lo=-1.5e308, hi=1.5e308)), ("cutoff", dict(cutoff=0.0)), ("lut_1", dict(lut_n=1)),
                  ("lut_many", dict(lut_n=1025)), ("lut_null", dict(d_lut=0)), ("lut_misaligned", dict(d_lut=LUT + 8)), ("level_bias", dict(level_bias=31)),
                  ("accumulate_rgba8", dict(flags=4, out_type=1))],
}
# ... what needs the dimension count (checked behind the geometry in a plan call, with the options in a _device call) ...
AXIS_FAULTS = {
    "project": [("axis", dict(axis=3))],
    "gradient": [("axis", dict(op=0, axis=3)), ("spacing_0", dict(spacing=(1.0, 0.0, 1.0, 1.0))), ("spacing_inf", dict(spacing=(INF, 1.0, 1.0, 1.0))),
                 ("spacing_nan", dict(spacing=(1.0, 1.0, NAN, 1.0)))],
    "composite": [("axis", dict(axis=3))],
}
# ... and the arguments' and boxes' (a name the builders below know)
ARG_FAULTS = ("null_conf", "null_out", "null_reqs", "dtype_12", "dtype_int32", "n_0", "n_over", "reserved", "level_31", "level_neg", "ext_0", "off_grid")
BOX_FAULTS = {  # per kind, behind the shared ones
    "request": ("null_d_out", "stride_negative", "stride_zero", "stride_permuted", "stride_huge", "overlap", "past_address_space"),
    "reduce": (),
    "select": ("index_null", "value_without_capacity", "capacity_huge", "misaligned", "overlap", "overlap_value"),
    "map": ("null_d_out", "misaligned", "stride_negative", "stride_zero", "stride_permuted", "overlap"),
    "sample": ("null_d_out", "misaligned", "n_points_0", "coords_misaligned", "coords_with_lattice", "lattice_count_0", "lattice_product", "lattice_origin",
               "lattice_step", "overlap"),
    "project": ("null_d_out", "misaligned", "stride_negative", "stride_zero", "stride_permuted", "overlap", "index_extent"),
    "gradient": ("null_d_out", "misaligned", "stride_negative", "stride_zero", "stride_permuted", "overlap", "interior_ext_2", "grid_step"),
    "composite": ("null_d_out", "misaligned", "stride_negative", "stride_zero", "stride_permuted", "overlap", "squarings"),
}
PAIRS = (("dtype_12", "null_reqs"), ("reserved", "opts"), ("opts", "off_grid"), ("off_grid", "overlap"), ("axis", "misaligned"), ("interior_ext_2", "overlap"),
         ("n_0", "null_reqs"), ("level_31", "ext_0"), ("null_d_out", "reserved"), ("opts", "axis"))
DEVICE_FAULTS = ("N_0", "N_5", "dims_null", "ext_0", "null_output", "opts", "stride_negative", "dtype_12")
DEVICE_PAIRS = (("null_output", "opts"), ("opts", "N_5"), ("null_output", "axis"), ("dtype_12", "N_0"), ("null_output", "stride_negative"), ("ext_0", "opts"))


def load(pkg=None):
    sys.path.insert(0, pkg or os.environ.get("LAB_PKG") or ROOT)
    import sz3_amd
    return sz3_amd


def cases():
    """every case's id, in the table's order: "<call>[<fault>]" or "<call>[<fault>+<fault>]" """
    ids = []
    for kind in KINDS:
        call = "sz3hip_%s_plan_for" % kind
        singles = list(ARG_FAULTS) + list(BOX_FAULTS[kind])
        singles += ["opts:" + name for name, _ in OPT_FAULTS.get(kind, ())] + ["axis:" + name for name, _ in AXIS_FAULTS.get(kind, ())]
        ids += ["%s[%s]" % (call, f) for f in singles]
        ids += ["%s[%s+%s]" % (call, a, b) for a, b in PAIRS if applies(kind, a) and applies(kind, b)]
    for kind in KINDS + ("tiles",):
        call = "sz3hip_stream_%s" % kind
        ids.append("%s[null_handle]" % call)
        ids += ["%s[null_handle+%s]" % (call, f) for f in ("null_reqs", "n_0", "null_result", "opts") if applies(kind, f) or (f == "null_result" and kind in ("reduce", "select"))]
    for kind in KINDS[1:]:
        call = "sz3hip_%s_device" % kind
        singles = list(DEVICE_FAULTS) + ["axis:" + name for name, _ in AXIS_FAULTS.get(kind, ())]
        ids += ["%s[%s]" % (call, f) for f in singles]
        ids += ["%s[%s+%s]" % (call, a, b) for a, b in DEVICE_PAIRS if a != "axis" and b != "axis" or kind in AXIS_FAULTS]
    return ids


def applies(kind, fault):
    if fault == "opts":
        return kind in OPT_FAULTS
    if fault == "axis":
        return kind in AXIS_FAULTS
    return fault in ARG_FAULTS or fault in BOX_FAULTS.get(kind, ())


def fill(struct, fields):
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(struct, k)[j] = x
        else:
            setattr(struct, k, v)
    return struct


def options(sz, kind, faults):
    """the kind's options struct with the faults' fields over the valid ones (None: the fault is to pass none)"""
    if kind not in OPTS:
        return None
    fields = dict(OPTS[kind])
    for f in faults:
        table = dict(OPT_FAULTS[kind]) if f == "opts" or f.startswith("opts:") else dict(AXIS_FAULTS.get(kind, ())) if f == "axis" or f.startswith("axis:") else None
        if table is None:
            continue
        over = table[f.split(":", 1)[1]] if ":" in f else next(iter(table.values()))
        if over is None:
            return None
        fields.update(over)
    if kind == "gradient" and "interior_ext_2" in faults:
        fields["flags"] = 1
    if kind == "gradient" and "grid_step" in faults:
        fields["spacing"] = (1.0, 1.5e308, 1.0, 1.0)
    if kind == "project" and "index_extent" in faults:
        fields.update(op=5, axis=0)
    if kind == "composite" and "squarings" in faults:
        fields.update(flags=2, level_bias=30)
    struct = {"reduce": sz._CReduceOpts, "select": sz._CSelectOpts, "map": sz._CMapOpts, "sample": sz._CSampleOpts, "project": sz._CProjectOpts,
              "gradient": sz._CGradientOpts, "composite": sz._CCompositeOpts}[kind]()
    return fill(struct, fields)


def boxes(sz, kind, faults):
    """two valid boxes of levels 0 and 1 with the faults worked in (box 1 carries them); returns the array, n and whether it is passed"""
    n = 257 if "n_over" in faults else 2
    struct = {"reduce": sz._CReduceReq, "select": sz._CSelectReq, "sample": sz._CSampleReq}.get(kind, sz._CTileReq)
    reqs = (struct * n)()
    for i in range(n):
        q = reqs[i]
        q.level = i % 2
        lo, ext = ((0, 0, 0), (8, 8, 8)) if i % 2 == 0 else ((2, 2, 2), (6, 5, 4))
        for j in range(3):
            q.box.lo[j], q.box.ext[j] = lo[j], ext[j]
        at = BASE + 4096 * i
        if kind in TILE_KINDS:
            q.d_out = at
        elif kind == "select":
            q.d_index, q.d_value, q.capacity = at, at + (1 << 30), 16
        elif kind == "sample":
            q.d_coords, q.d_out, q.n_points = at + (1 << 30), at, 10
    b = reqs[1]
    for f in faults:
        if f == "reserved":
            b.reserved = 7
        elif f == "level_31":
            b.level = 31
        elif f == "level_neg":
            b.level = -1
        elif f == "ext_0":
            b.box.ext[1] = 0
        elif f == "off_grid":
            b.box.lo[2] = 27  # level 1's grid has 28 points along z: [27, 27 + 4) leaves it
        elif f == "null_d_out":
            b.d_out = 0
        elif f == "misaligned":
            if kind == "select":
                b.d_index += 4
            else:
                b.d_out += 1
        elif f == "stride_negative":
            b.strides[0], b.strides[1], b.strides[2] = -20, 4, 1
        elif f == "stride_zero":
            b.strides[0], b.strides[1], b.strides[2] = 0, 4, 1
        elif f == "stride_permuted":
            b.strides[0], b.strides[1], b.strides[2] = 1, 4, 24
        elif f == "stride_huge":
            b.strides[0], b.strides[1], b.strides[2] = 1 << 60, 4, 1
        elif f == "past_address_space":
            b.d_out = (1 << 64) - 64
        elif f == "overlap":
            if kind == "select":
                b.d_index = reqs[0].d_index + 8
            else:
                b.d_out = reqs[0].d_out
        elif f == "overlap_value":
            b.d_value = reqs[0].d_value
        elif f == "index_null":
            b.d_index = 0
        elif f == "value_without_capacity":
            b.capacity = 0
        elif f == "capacity_huge":
            b.capacity = (1 << 56) + 1
        elif f == "n_points_0":
            b.n_points = 0
        elif f == "coords_misaligned":
            b.d_coords += 2
        elif f == "coords_with_lattice":
            b.counts[0] = 10
        elif f.startswith("lattice_"):
            b.d_coords, b.n_points = 0, 10
            b.counts[0], b.counts[1], b.counts[2] = 10, 1, 1
            if f == "lattice_count_0":
                b.counts[1] = 0
            elif f == "lattice_product":
                b.counts[1] = 2
            elif f == "lattice_origin":
                b.origin[1] = INF
            elif f == "lattice_step":
                b.steps[2][0] = NAN
        elif f == "interior_ext_2":
            b.box.ext[1] = 2
    return reqs, (0 if "n_0" in faults else n)


def run_plan(sz, kind, faults):
    L = sz.lib()
    conf = sz.Config(*SHAPE)
    reqs, n = boxes(sz, kind, faults)
    plan = {"request": sz._CRequestPlan, "reduce": sz._CReducePlan, "select": sz._CSelectPlan, "map": sz._CMapPlan, "sample": sz._CSamplePlan,
            "project": sz._CProjectPlan, "gradient": sz._CGradientPlan, "composite": sz._CCompositePlan}[kind]()
    dtype = 12 if "dtype_12" in faults else 7 if "dtype_int32" in faults else 0
    if "index_extent" in faults:  # the one fault no box of (40, 48, 56) can hold: an index op along 2^32 points, on a conf of its own
        conf = sz.Config(1 << 33, 2)
        reqs, n = (sz._CTileReq * 1)(), 1
        reqs[0].box.ext[0], reqs[0].box.ext[1], reqs[0].d_out = 1 << 32, 2, BASE
    args = [None if "null_conf" in faults else C.byref(conf._c), dtype, None if "null_reqs" in faults else reqs, n]
    if kind != "request":
        opts = options(sz, kind, faults)
        args.append(None if opts is None else C.byref(opts))
    args.append(None if "null_out" in faults else C.byref(plan))
    return getattr(L, "sz3hip_%s_plan_for" % kind)(*args)


def run_stream(sz, kind, faults):
    """the call with a NULL handle; everything else valid unless a second fault says otherwise"""
    L = sz.lib()
    if kind == "tiles":
        bx = (sz._CBox * 2)()
        for i in range(2):
            for j in range(3):
                bx[i].ext[j] = 4
        outs = (C.c_void_p * 2)(BASE, BASE + 4096)
        return L.sz3hip_stream_tiles(None, 0, None if "null_reqs" in faults else bx, 0 if "n_0" in faults else 2, outs, None)
    reqs, n = boxes(sz, kind, faults)
    args = [None, None if "null_reqs" in faults else reqs, n]
    if kind != "request":
        opts = options(sz, kind, faults)
        args.append(None if opts is None else C.byref(opts))
    if kind == "reduce":
        args += [None if "null_result" in faults else BASE + (1 << 32), BASE + (1 << 33)]
    if kind == "select":
        args.append(None if "null_result" in faults else BASE + (1 << 32))
    args.append(None)
    return getattr(L, "sz3hip_stream_%s" % kind)(*args)


def run_device(sz, kind, faults):
    """a (6, 5, 4) view of device memory at a placeholder address; every case fails before the address is looked at"""
    L = sz.lib()
    N = 0 if "N_0" in faults else 5 if "N_5" in faults else 3
    dims = (C.c_uint64 * 5)(6, 0 if "ext_0" in faults else 5, 4, 3, 2)
    strides = (C.c_int64 * 5)(20, -4 if "stride_negative" in faults else 4, 1, 1, 1)
    opts = options(sz, kind, faults)
    out = None if "null_output" in faults else BASE + 4096
    args = [12 if "dtype_12" in faults else 0, N, None if "dims_null" in faults else dims, BASE, strides, None if opts is None else C.byref(opts)]
    if kind == "reduce":
        args += [out, BASE + 8192]
    elif kind == "select":
        args += [BASE + 8192, BASE + 12288, 16, out]
    elif kind == "sample":
        q = sz._CSampleReq()
        q.d_coords, q.d_out, q.n_points = BASE + 8192, BASE + 4096, 10
        args.append(None if out is None else C.byref(q))
    else:
        args += [out, None]
    args.append(None)
    return getattr(L, "sz3hip_%s_device" % kind)(*args)


def run(sz, case):
    """one case against the package `sz`: (return code, sz3hip_last_error's text)"""
    call, faults = case[:-1].split("[")
    faults = faults.split("+")
    kind = call.split("_")[2] if call.startswith("sz3hip_stream_") else call.split("_")[1]
    runner = run_plan if call.endswith("_plan_for") else run_stream if call.startswith("sz3hip_stream_") else run_device
    rc = runner(sz, kind, faults)
    return int(rc), sz.lib().sz3hip_last_error().decode()


def table(sz):
    rows = []
    for case in cases():
        rc, text = run(sz, case)
        if rc == 0:
            raise SystemExit("%s: the call succeeded — not a case of this table" % case)
        rows.append({"id": case, "rc": rc, "error": text})
    return rows


def dumps(rows):
    return "[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n"


if __name__ == "__main__":
    rows = table(load())
    with open(OUT, "w") as f:
        f.write(dumps(rows))
    print("%d cases -> %s" % (len(rows), OUT))

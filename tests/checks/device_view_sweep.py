#!/usr/bin/env python3
"""seeded sweep over the DEVICE-MEMORY calls: sz3hip_compress_from_device, sz3hip_decompress_to_device and the coarse
call's strided output over drawn views of drawn base allocations — the kernel family k_strided in every form the draws reach. Every reference
is numpy's as_strided view of a host copy of the same allocation (tests/view_model.py); the host API delivers the container bytes and the
decoded values. Everything is compared for equality of bytes; the one tolerance is the Config's error bound.
Per case (np.random.default_rng(SEED); every draw is made before anything runs on a device and depends on no device result): an element type
of the ten, a rank 1 .. 4, a shape whose inner extent is one of the row walker's edges, an input view and another output view of it (per axis
whole / sub-range / step 2 / step 3, a permuted memory order, a stride-0 axis for inputs, one field of interleaved records, a base offset that is
misaligned, 8- or 16-byte aligned; half the cases aim at the wide units), an algorithm, an error-bound mode (the float types; integers take
the absolute bound, the one the project defines for them), stock format 0 / 1, a route (plain, conf.openmp slabs, pipelined pieces) and the data.
  1  sz3hip_debug_gather of the input view equals numpy's view (integers widened to f64);
  2  the container from the view == the container from a contiguous device copy == the host API's;
  3  the input allocation is unchanged;
  4  the decode into the output view: the WHOLE allocation (random bytes before) equals view_model.expected_after_scatter of the host decode;
  5  the bound of the mode holds for the host decode against numpy;
  6  float cases under an interpolation algorithm, and the first other float case of a seed: the coarse call at a drawn level into a drawn view.
No case is skipped; an exception is a failure; a container that fell back to lossless passes the same identities.
Environment: SEED, N, CASES=3,17 (only those run; all draws are still made), VERBOSE, DRY=1 (no device call: the draws, their premises — every
view inside its allocation, every output accepted by view_model.dev_view_rule — and the tallies). One line per failure, a line TALLY <json>, a
last line "cases ... failures K"; exit status 1 if K > 0, 2 after an error of the HIP runtime (nothing more runs on the device then)."""
import json, os, sys
from collections import Counter
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (before sz3_amd: one HIP runtime)
import sz3_amd
import view_model as M
from view_model import View
from partial_cases import CODES, smooth

SEED = int(os.environ.get("SEED", "1"))
N_CASES = int(os.environ.get("N", "24"))
SEL = set(int(x) for x in os.environ["CASES"].split(",")) if os.environ.get("CASES") else None
VERBOSE = bool(os.environ.get("VERBOSE"))
DRY = bool(os.environ.get("DRY"))
rng = np.random.default_rng(SEED)
EHIP = CODES["SZ3HIP_EHIP"]

MAX_VIEW, MAX_BASE = 40000, 300000  # elements of the array, of a base allocation
OUTER = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 50, 64, 70]
WIDE_INNERS = (32, 64, 256)  # whole 16-byte units in every element type
INNER_P = np.array([1.0] * (len(M.INNERS) - 2) + [3.0, 3.0]) / (len(M.INNERS) + 4)  # (rows of several passes, 257 and 1025, three times as often)
FLOATS = ("float32", "float64")
SETS = {1: [(1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1), (0, 0, 1)], 2: [(1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)],
        3: [(1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)], 4: [(1, 0, 0), (1, 0, 1)]}
ALGOS = ["lorenzo", "lorenzo", "interp_lorenzo", "interp", "nopred", "lossless"]
ALGO_ID = {"lorenzo": sz3_amd.ALGO_LORENZO_REG, "interp_lorenzo": sz3_amd.ALGO_INTERP_LORENZO, "interp": sz3_amd.ALGO_INTERP,
           "nopred": sz3_amd.ALGO_NOPRED, "lossless": sz3_amd.ALGO_LOSSLESS}
MODES = [sz3_amd.EB_ABS, sz3_amd.EB_REL, sz3_amd.EB_ABS_AND_REL, sz3_amd.EB_ABS_OR_REL, sz3_amd.EB_PSNR, sz3_amd.EB_L2NORM]


def r(a, b):
    return int(rng.integers(a, b + 1))  # inclusive


# ---- the draws ---------------------------------------------------------------------------------------------------------------------------------
def draw_shape(rank, wide, route):
    while True:
        inner = int(rng.choice(WIDE_INNERS)) if wide else int(rng.choice(M.INNERS, p=INNER_P))
        outer = [int(rng.choice(OUTER)) for _ in range(rank - 1)]
        if route[0] == "pieces" and rank >= 2:  # (a piece has at least 32 planes)
            outer[0] = 32 * route[1] + r(0, 31)
        elif route[0] == "slabs" and rank >= 2:  # (slabs of at least two rows, cut at no convenient multiple)
            outer[0] = max(outer[0], 2 * route[1] + r(0, 40))
        shape = tuple(outer) + (inner,)
        if 2 <= int(np.prod(shape)) <= MAX_VIEW:
            return shape


def draw_view(dtype, shape, output, wide):
    """a view of extents `shape` of a base allocation -> (View, base elements, facts)"""
    es = np.dtype(dtype).itemsize
    n = len(shape)
    g = max(1, 16 // es)  # elements per 16 bytes
    while True:
        modes = [str(rng.choice(["whole", "sub", "step2", "step3"])) for _ in range(n)]
        permute = n > 1 and not wide and rng.random() < 0.4
        order = [int(i) for i in rng.permutation(n)] if permute else list(range(n - 1, -1, -1))  # logical axes, fastest first
        cand = [i for i in range(n) if shape[i] > 1]
        zero = int(rng.choice(cand)) if (not output and cand and rng.random() < 0.2) else None
        if wide and zero == n - 1:
            zero = None
        nf = r(2, 4) if (not wide and rng.random() < 0.2) else 1
        k = r(0, nf - 1)
        align = [16, 8, "mis"][int(rng.choice(3, p=[0.45, 0.45, 0.1] if wide else [0.25, 0.25, 0.5]))]
        if wide:
            modes[n - 1] = str(rng.choice(["whole", "sub"]))
        lo, step, ext = [0] * n, [1] * n, [0] * n
        for i, d in enumerate(shape):
            if i == zero:
                ext[i] = 1
                continue
            if modes[i] == "whole":
                ext[i] = d
            elif modes[i] == "sub":
                lo[i], hi_pad = r(0, 5), r(0, 5)
                if wide and i == n - 1:
                    lo[i], hi_pad = g * r(0, 3), g * r(0, 3)
                ext[i] = lo[i] + d + hi_pad
            else:
                step[i] = int(modes[i][-1])
                lo[i] = r(0, step[i] - 1)
                ext[i] = lo[i] + (d - 1) * step[i] + 1 + r(0, step[i] - 1)
        run, off, strides = nf, k, [0] * n
        for i in order:
            strides[i] = 0 if i == zero else run * step[i]
            off += run * lo[i]
            run *= ext[i]
        if run > MAX_BASE:
            continue
        boff = g * r(0, 3) if align == 16 else (max(1, 8 // es) + g * r(0, 2)) if align == 8 else 1 + g * r(0, 2)
        v = View(np.dtype(dtype).name, off + boff, tuple(shape), tuple(strides))
        facts = dict(permuted=order != list(range(n - 1, -1, -1)), stepped=any(s > 1 for i, s in enumerate(step) if shape[i] > 1), zero=zero, field=nf > 1, align=align,
                     contiguous=M.dev_view_rule(v.dropped().shape, v.dropped().strides, False) == M.CONTIGUOUS)
        if output and M.dev_view_rule(v.shape, v.strides, True) not in (M.CONTIGUOUS, M.STRIDED):
            continue  # (cannot happen: an output draws no stride 0 and its axes nest)
        return v, boff + run + r(1, 9), facts


def coarse_shape(shape, k):
    return tuple(((d - 1) >> k) + 1 for d in shape)


def draw_case(k, seen_fallback_coarse):
    c = {"k": k}
    wide = c["wide"] = bool(k % 2)  # half the cases aim at the wide units
    c["dtype"] = dtype = str(rng.choice(FLOATS)) if (wide and rng.random() < 0.5) else M.DTYPES[int(rng.integers(0, 10))]
    is_int = dtype in M.INT_TYPES
    rank = c["rank"] = int(rng.choice([1, 2, 2, 3, 3, 4]))
    route = [("plain", 0), ("slabs", r(2, 4)), ("pieces", r(2, 3))][int(rng.choice(3, p=[0.45, 0.35, 0.2]))]
    if rank == 1 and route[0] == "pieces":  # (a 1-D piece has 65536 elements: beyond this sweep's arrays)
        route = ("slabs", route[1])
    c["shape"] = shape = draw_shape(rank, wide, route)
    if route[0] == "slabs" and shape[0] < 2 * route[1]:
        route = ("plain", 0)
    c["route"] = route
    c["vin"], c["n_in"], c["f_in"] = draw_view(dtype, shape, False, wide)
    c["vout"], c["n_out"], c["f_out"] = draw_view(dtype, shape, True, wide)
    algo = ALGOS[int(rng.integers(0, len(ALGOS)))]
    if not is_int and rng.random() < 0.3:
        algo = "interp"
    pset = SETS[max(1, len([d for d in shape if d > 1]))]
    c["set"] = pset[int(rng.integers(0, len(pset)))]
    mode = MODES[int(rng.integers(0, len(MODES)))]
    c["stock"] = int(rng.random() < 0.25)
    kinds = ["smooth", "step", "ends"] if is_int else ["smooth", "step", "nonfinite"]
    c["kind"] = kinds[int(rng.choice(3, p=[0.4, 0.2, 0.4] if is_int else [0.5, 0.25, 0.25]))]
    if route[0] == "pieces":  # what a call needs to be cut into pieces: Lorenzo or no predictor, an absolute bound, this library's own format
        algo = algo if algo in ("lorenzo", "nopred") else "lorenzo"
        mode, c["stock"] = sz3_amd.EB_ABS, 0
    if is_int or c["kind"] == "nonfinite":  # (integers: the bound the project defines for them; the range of a field with NaN is NaN)
        mode = sz3_amd.EB_ABS
    c["algo"], c["mode"] = algo, mode
    c["eb"] = float(rng.choice([1.0, 2.5, 10.0])) if is_int else float(rng.choice([1e-2, 1e-3]))
    c["field_seed"] = r(1, 1 << 30)
    c["base_seed"] = r(1, 1 << 30)
    # the coarse call: float interpolation algorithms, and the first other float case of the seed
    c["coarse"] = None
    dropped = tuple(d for d in shape if d > 1)
    level = min(r(1, 2), max((d - 1).bit_length() for d in dropped))  # (at most the level whose grid is one point)
    cs = coarse_shape(dropped, level)
    cv, cn, cf = draw_view(dtype, cs, True, False)
    if not is_int and (algo in ("interp", "interp_lorenzo") or not seen_fallback_coarse[0]):
        if algo not in ("interp", "interp_lorenzo"):
            seen_fallback_coarse[0] = True
        c["coarse"] = dict(level=level, view=cv, n=cn, facts=cf)
    return c


def tag_of(c):
    return "case %d (SEED %d) %s %s %s set %s mode %d eb %g stock %d route %s %s data; in %s %s; out %s %s%s" % (
        c["k"], SEED, c["dtype"], "x".join(map(str, c["shape"])), c["algo"], c["set"], c["mode"], c["eb"], c["stock"], "%s %d" % c["route"], c["kind"],
        tuple(c["vin"][1:]), c["f_in"]["align"], tuple(c["vout"][1:]), c["f_out"]["align"], "; coarse level %d" % c["coarse"]["level"] if c["coarse"] else "")


def conf_of(c):
    conf = sz3_amd.Config(*c["shape"])
    conf.cmprAlgo = ALGO_ID[c["algo"]]
    if c["algo"] == "lorenzo":
        conf.lorenzo, conf.lorenzo2, conf.regression = c["set"]
    conf.errorBoundMode = c["mode"]
    conf.absErrorBound = c["eb"]
    conf.relErrorBound = 1e-3
    conf.psnrErrorBound = 60.0
    conf.l2normErrorBound = c["eb"] * float(np.sqrt(np.prod(c["shape"])))
    conf.quantbinCnt = 1024
    conf.openmp = 1 if c["route"][0] == "slabs" else 0
    return conf


def data_of(c, shape):
    dtype, kind = c["dtype"], c["kind"]
    q = np.random.default_rng(c["field_seed"])
    f = smooth(shape, "float64", seed=c["field_seed"])
    if kind == "step":
        f = f + 3.0 * (np.indices(shape)[int(np.argmax(shape))] > max(shape) // 2)
    if dtype in FLOATS:
        a = f.astype(dtype)
        if kind == "nonfinite":
            pos = q.integers(0, a.size, max(1, min(8, a.size // 50)))
            a.reshape(-1)[pos] = q.choice([np.nan, np.inf, -np.inf], pos.size)
        return a
    info = np.iinfo(dtype)
    amp = min(10000, (int(info.max) - int(info.min)) // 12)
    mid = (int(info.max) + int(info.min) + 1) // 2 if info.bits < 64 else 0 if info.min < 0 else 100000
    a = (np.rint(f * amp / 4.5).astype(np.int64) + mid).astype(dtype)
    if kind == "ends":  # runs at both ends of the type: under a bound >= 1 the reconstruction leaves the range and the narrowing clamps
        flat = a.reshape(-1)
        for end in (info.min, info.max, info.max, info.min):
            p0 = int(q.integers(0, flat.size))
            flat[p0:p0 + int(q.integers(1, 40))] = end
        flat[0], flat[-1] = info.max, info.min
    return a


# ---- the tallies (from the draws alone) ----------------------------------------------------------------------------------------------------------
def tally_case(c, T):
    dtype, is_int = c["dtype"], c["dtype"] in M.INT_TYPES
    T["dtype_in"][dtype] += 1
    T["dtype_out"][dtype] += 1
    T["rank"][str(c["rank"])] += 1
    T["algo"][c["algo"]] += 1
    T["kind"][c["kind"]] += 1
    T["route"][c["route"][0]] += 1
    for side, v, converts in (("gather", c["vin"], is_int), ("scatter", c["vout"], is_int and c["algo"] != "lossless")):
        d = v.dropped()
        form, inner = M.launch_form(d, d.offset * d.itemsize, 0, converts)  # (allocations and the library's dense buffers are aligned beyond 16 bytes)
        T[side + "_form"][str(form)] += 1
        if form is not None:
            T[side + "_convert"] += int(converts)
            T[side + "_packed"] += int(M.rows_per_wave(inner) > 1)
            T[side + "_one_row"] += int(M.rows_per_wave(inner) == 1)
            T[side + "_passes"] += int(M.row_passes(inner) > 1)
    strided_in = not c["f_in"]["contiguous"]
    T["permuted_out"] += int(c["f_out"]["permuted"])
    T["stepped_out"] += int(c["f_out"]["stepped"])
    T["permuted_in"] += int(c["f_in"]["permuted"])
    T["field_in"] += int(c["f_in"]["field"])
    T["zero_in"] += int(c["f_in"]["zero"] is not None)
    T["slabs_strided_in"] += int(c["route"][0] == "slabs" and strided_in)
    T["pieces_strided_in"] += int(c["route"][0] == "pieces" and strided_in)
    T["stock"] += c["stock"]
    T["coarse_strided_out"] += int(c["coarse"] is not None and not c["coarse"]["facts"]["contiguous"])
    T["clamp"] += int(c["kind"] == "ends" and c["algo"] != "lossless" and np.dtype(dtype).itemsize < 8)


def dry(c):
    bad = []
    for name, v, n, output in (("input", c["vin"], c["n_in"], False), ("output", c["vout"], c["n_out"], True)) + (
            (("coarse output", c["coarse"]["view"], c["coarse"]["n"], True),) if c["coarse"] else ()):
        if not (v.offset >= 0 and v.last < n):
            bad.append("the %s view leaves its allocation" % name)
        want = (M.CONTIGUOUS, M.STRIDED)
        if M.dev_view_rule(v.shape, v.strides, output) not in want:
            bad.append("the %s view is refused by the rule" % name)
        if output and len(set(M.touched_offsets(v.shape, v.strides))) != v.numel:
            bad.append("the %s view's elements overlap" % name)
    if c["vin"].shape != c["vout"].shape or c["vin"].numel > MAX_VIEW:
        bad.append("shapes")
    if c["route"][0] == "pieces" and not (c["shape"][0] >= 32 * c["route"][1] and c["algo"] in ("lorenzo", "nopred") and c["mode"] == sz3_amd.EB_ABS and not c["stock"]):
        bad.append("a pieces draw that the library would not cut")
    return bad


# ---- the device legs ---------------------------------------------------------------------------------------------------------------------------
def bound_holds(c, a, dec):
    """the guarantee of the Config's mode for the host decode (the rules of tests/checks/host_sweep.py; integers: |x - x^| <= floor(eb))"""
    if dec.dtype != a.dtype or dec.shape != a.shape:
        return "dtype or shape changed"
    if c["dtype"] in M.INT_TYPES:
        if a.itemsize == 8:
            err = max(abs(int(x) - int(y)) for x, y in zip(a.reshape(-1), dec.reshape(-1)))
        else:
            err = int(np.abs(a.astype(np.int64) - dec.astype(np.int64)).max())
        return None if err <= int(np.floor(c["eb"])) else "integer error %d beyond floor(%g)" % (err, c["eb"])
    af, df = a.astype(np.float64), dec.astype(np.float64)
    fin = np.isfinite(af)
    if not (np.array_equal(np.isnan(df), np.isnan(af)) and np.array_equal(df[~fin & ~np.isnan(af)], af[~fin & ~np.isnan(af)])):
        return "non-finite values moved"
    if not fin.any():
        return None
    err = float(np.abs(df[fin] - af[fin]).max())
    rngv = float(af[fin].max() - af[fin].min())
    mode, eb, rel = c["mode"], c["eb"], 1e-3
    bound = {sz3_amd.EB_ABS: eb, sz3_amd.EB_REL: rel * rngv, sz3_amd.EB_ABS_AND_REL: min(eb, rel * rngv), sz3_amd.EB_ABS_OR_REL: max(eb, rel * rngv)}.get(mode)
    if bound is not None:
        if a.dtype == np.float32:
            bound = bound * (1 + 1e-6) + 1e-30  # (the range is taken in float32, as the reference takes it)
        return None if err <= bound * (1 + 1e-9) else "error %.6g beyond the bound %.6g" % (err, bound)
    if mode == sz3_amd.EB_PSNR:
        mse = float(np.mean((df[fin] - af[fin]) ** 2))
        psnr = 20 * np.log10(rngv) - 10 * np.log10(mse) if mse > 0 and rngv > 0 else np.inf
        return None if psnr >= 60.0 - 4.8 else "PSNR %.2f below the target's guarantee" % psnr
    l2 = float(np.sqrt(np.sum((df[fin] - af[fin]) ** 2)))
    target = eb * float(np.sqrt(a.size))
    return None if l2 <= target * 1.1 else "L2 norm %.6g beyond %.6g" % (l2, target)


def run_case(c, T):
    import device_views as D
    bad = []
    dtype, vin, vout = c["dtype"], c["vin"], c["vout"]
    npdt = np.dtype(dtype)
    # the input allocation: random bytes, the field written through the view (a stride-0 axis: through its one layer)
    host = np.random.default_rng(c["base_seed"]).integers(0, 256, c["n_in"] * npdt.itemsize, dtype=np.uint8)
    z = c["f_in"]["zero"]
    layer = vin if z is None else View(vin.dtype, vin.offset, tuple(1 if i == z else d for i, d in enumerate(vin.shape)), vin.strides)
    M.view_of(host, layer)[...] = data_of(c, layer.shape)
    a = np.ascontiguousarray(M.view_of(host, vin))
    alloc = D.Alloc(host)
    # 1 the gather alone
    d = vin.dropped()
    if not D.same_bytes(D.gather(alloc, d), D.gather_expected(alloc, d)):
        bad.append("1: sz3hip_debug_gather of the input view differs from numpy's view")
    # 2, 3 the three containers, the input unchanged
    sz3_amd.set_stock_format(c["stock"])
    if c["route"][0] == "slabs":
        os.environ["SZ3HIP_SLABS"] = str(c["route"][1])
    if c["route"][0] == "pieces":
        os.environ["SZ3HIP_PIECES"] = str(c["route"][1])
    try:
        b_view = sz3_amd.compress(alloc.tensor(vin), conf_of(c))[0].tobytes()
        b_cont = sz3_amd.compress(torch.from_numpy(a).to(D.DEV), conf_of(c))[0].tobytes()
        b_host = sz3_amd.compress(a, conf_of(c))[0].tobytes()
    finally:
        os.environ.pop("SZ3HIP_SLABS", None)
        os.environ.pop("SZ3HIP_PIECES", None)
        sz3_amd.set_stock_format(0)
    if b_view != b_cont:
        bad.append("2: the container of the view (%d bytes) is not the container of its contiguous device copy (%d)" % (len(b_view), len(b_cont)))
    if b_view != b_host:
        bad.append("2: the container of the view (%d bytes) is not the host API's (%d)" % (len(b_view), len(b_host)))
    if not alloc.unchanged():
        bad.append("3: the input allocation was written")
    # 4 the decode into the output view, the whole allocation
    want, c2 = sz3_amd.decompress(b_host, npdt)
    want = want.reshape(c["shape"])
    T["lossless_containers"] += int(c2.cmprAlgo == sz3_amd.ALGO_LOSSLESS)
    if c["route"][0] != "plain" and c2.openmp != 1:
        bad.append("the route %s was drawn and the container is no multi-slab one" % (c["route"],))
    out = D.Alloc.random(dtype, c["n_out"], np.random.default_rng(c["base_seed"] + 1))
    sz3_amd.decompress(b_view, npdt, out=out.tensor(vout))
    got, exp = out.now(), M.expected_after_scatter(out.host, vout, want)
    if not np.array_equal(got, exp):
        bad.append("4: the decode into the output view: %s" % D.first_difference(got, exp, vout))
    # 5 the bound
    why = bound_holds(c, a, want)
    if why:
        bad.append("5: %s" % why)
    # 6 the coarse call
    if c["coarse"]:
        k, cv = c["coarse"]["level"], c["coarse"]["view"]
        full = want.reshape(tuple(dd for dd in c["shape"] if dd > 1))
        coarse = np.ascontiguousarray(full[tuple(slice(None, None, 1 << k) for _ in full.shape)])
        co = D.Alloc.random(dtype, c["coarse"]["n"], np.random.default_rng(c["base_seed"] + 2))
        sz3_amd.decompress_coarse(b_view, npdt, k, out=co.tensor(cv))
        got, exp = co.now(), M.expected_after_scatter(co.host, cv, coarse)
        if not np.array_equal(got, exp):
            bad.append("6: the coarse call at level %d into %s: %s" % (k, tuple(cv[1:]), D.first_difference(got, exp, cv)))
    return bad


def main():
    T = {k: Counter() for k in ("dtype_in", "dtype_out", "rank", "algo", "kind", "route", "gather_form", "scatter_form")}
    for k in ("gather_convert", "scatter_convert", "gather_packed", "gather_one_row", "gather_passes", "scatter_packed", "scatter_one_row", "scatter_passes", "permuted_out",
              "stepped_out", "permuted_in", "field_in", "zero_in", "slabs_strided_in", "pieces_strided_in", "stock", "coarse_strided_out", "clamp", "lossless_containers"):
        T[k] = 0
    failures = n_run = 0
    down = None
    seen = [False]
    for k in range(N_CASES):
        c = draw_case(k, seen)
        if SEL and k not in SEL:
            continue
        n_run += 1
        tally_case(c, T)
        tag = tag_of(c)
        if VERBOSE:
            print(tag, flush=True)
        bad = dry(c)
        if not DRY and not bad:
            try:
                bad = run_case(c, T)
            except sz3_amd.SZ3HipError as e:
                bad = ["exception: %s" % str(e)[:300]]
                if e.code == EHIP:
                    down = e
            except RuntimeError as e:  # (torch's: a fault of an earlier launch surfaces there)
                bad, down = ["exception: %s" % str(e)[:300]], e
            except Exception as e:  # noqa: BLE001  (an exception is a failure)
                bad = ["exception: %s: %s" % (type(e).__name__, str(e)[:300])]
            finally:
                os.environ.pop("SZ3HIP_SLABS", None)
                os.environ.pop("SZ3HIP_PIECES", None)
        for b in bad:
            failures += 1
            print("FAIL %s: %s" % (tag, b), flush=True)
        if down is not None:
            print("an error of the HIP runtime — the sweep ends here", flush=True)
            break
    show = lambda cn: ", ".join("%s %d" % (k, cn[k]) for k in sorted(cn, key=str))  # noqa: E731
    print("dtype: %s | rank: %s" % (show(T["dtype_in"]), show(T["rank"])))
    print("algo: %s | data: %s | route: %s | stock %d" % (show(T["algo"]), show(T["kind"]), show(T["route"]), T["stock"]))
    print("gather forms: %s | scatter forms: %s" % (show(T["gather_form"]), show(T["scatter_form"])))
    print("TALLY " + json.dumps({k: (dict(v) if isinstance(v, Counter) else v) for k, v in T.items()}, sort_keys=True))
    print("cases %d (SEED %d, %s) failures %d" % (n_run, SEED, "DRY: draws only" if DRY else "on the device", failures))
    sys.exit(2 if down is not None else 1 if failures else 0)


main()

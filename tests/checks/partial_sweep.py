#!/usr/bin/env python3
"""seeded sweep over the PARTIAL decodes (DESIGN.md sections 12 - 21): random shapes, boxes, interpolation orders, anchor strides, routes and
sinks, every result held byte for byte to an expected array that one of three sources delivers:
  own      sz3_amd.compress's container                         — expected: this library's full decode
  payload  a DeviceCompressor payload, opened by dc.open_stream — expected: that context's full decode
  oracle   a container the ORACLE wrote on the CPU              — expected: the oracle's own decode (the library wrote neither the stream nor
           the expected values; its full decode is held to the oracle's array too)
Per case (np.random.default_rng(SEED); every draw is made before anything runs on a device and depends on no device result):
  A  three of the boxes through decompress_region / _tile / _tiles / _coarse on the container (sparse decode on and off), a payload's through
     DeviceCompressor.decompress_region / _tile / _tiles;
  B  Stream.request of all items three times (contiguous outputs, rectangles of one atlas, views with a step of 2 along x), single-level
     requests through Stream.tiles too, and the handle's stats;
  C  two of the five sinks (reduce, select, map, sample, project) against the numpy rules of tests/sink_models.py, then again under a second
     route (the other chain setting, or the by-level switch flipped), byte for byte.
A case whose anchor stride is no power of two (one in twenty) cannot be written as an interpolation stream (the compressor refuses the stride,
as the reference does): the sweep holds it to that refusal, then the field goes through the Lorenzo predictor with the same Config and the case
runs over the fallback handle (stats()["fast"] == 0).
Environment: SEED, N, CASES=3,17 (only those run; all draws are still made), VERBOSE, DRY=1 (no device call: every drawn request goes through
the pure host plan functions, which must accept it). One line per failure with the case's tag, a tally, a line TALLY <json>, a last line
"cases ... failures K"; exit status 1 if K > 0, 2 after an error of the HIP runtime (nothing more runs on the device then)."""
import contextlib, io, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (before sz3_amd: one HIP runtime)
import sz3_amd
from partial_cases import CODES, DEV, box_slices, conf_for, container, device_payload, raw, smooth

SEED = int(os.environ.get("SEED", "1"))
N_CASES = int(os.environ.get("N", "15"))
SEL = set(int(x) for x in os.environ["CASES"].split(",")) if os.environ.get("CASES") else None
VERBOSE = bool(os.environ.get("VERBOSE"))
DRY = bool(os.environ.get("DRY"))
L = sz3_amd.lib()
rng = np.random.default_rng(SEED)

MIN_ELEMS, MAX_ELEMS = 2000, 150000  # (below ~2000 elements a stream's fixed part outweighs the array and the dispatcher writes it lossless)
EDGE = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 47, 63, 64, 65, 66, 96, 97, 127, 128, 129, 130]
EDGE4 = list(range(1, 21)) + [31, 32, 33]
# rank 1: the 512-code units of the sparse tile decode. (511 .. 1025 lie under MIN_ELEMS and are always redrawn; the same edges further up stay)
EDGE1 = [511, 512, 513, 1024, 1025, 2047, 2048, 2049, 2559, 2560, 2561, 4095, 4096, 4097]
ALPHAS, BETAS = [-1.0, 1.0, 1.25, 1.5, 2.0], [1.0, 2.0, 3.0, 4.0]
ANCHORS = [None, 0, 2, 4, 8, 16, 32, 64]
DEF_ANCHOR = {1: 4096, 2: 128, 3: 32, 4: 16}
SINKS = ["reduce", "select", "map", "sample", "project"]
BOX_KINDS = ["whole", "point", "slab", "low", "far", "rows", "interior", "straddle"]
CHAIN_DEFAULT = sz3_amd.get_chain_points()
BY_LEVEL, PLAIN = int(sz3_amd.Dbg2.REQUEST_BY_LEVEL), int(sz3_amd.Dbg2.MAP_PLAIN_STORES)
EUNSUPPORTED, EHIP, EOUTLIERS = CODES["SZ3HIP_EUNSUPPORTED"], CODES["SZ3HIP_EHIP"], CODES["SZ3HIP_EOUTLIERS"]


class HipDown(Exception):
    """an error of the HIP runtime: the sweep ends, nothing more is started on the device"""


def coarse_shape(shape, k):
    return tuple(((d - 1) >> k) + 1 for d in shape)


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------------
def draw_shape():
    nd = int(rng.choice([1, 2, 3, 3, 4]))
    while True:
        if nd == 1:
            drawn = (int(rng.choice(EDGE1)) if rng.random() < 0.5 else int(rng.integers(300, 5001)),)
        else:
            drawn = tuple(int(rng.choice(EDGE4 if nd == 4 else EDGE)) for _ in range(nd))
        n = int(np.prod(drawn))
        if MIN_ELEMS <= n <= MAX_ELEMS and max(drawn) > 1:
            return drawn, tuple(d for d in drawn if d > 1)  # (a Config drops extents of one: the array's rank is what is left)


def draw_box(cs, kind):
    """a box (lo, ext) of the grid cs"""
    N = len(cs)
    r = lambda a, b: int(rng.integers(a, b + 1))  # noqa: E731  (inclusive)
    lo_i = [r(0, d - 1) for d in cs]
    inner = (tuple(lo_i), tuple(r(1, d - a) for d, a in zip(cs, lo_i)))
    ax = r(0, N - 1)
    pt, ext_low, ext_far = [r(0, d - 1) for d in cs], [r(1, d) for d in cs], [r(1, d) for d in cs]
    wide = [j for j in range(N) if cs[j] >= 35]
    pick = r(0, max(len(wide), 1) - 1)
    m, back, fwd = r(1, 1 << 20), 2 * r(0, 15) + 1, r(1, 40)
    if kind == "whole":
        return (0,) * N, tuple(cs)
    if kind == "point":
        return tuple(pt), (1,) * N
    if kind == "slab":
        return tuple(pt[j] if j == ax else 0 for j in range(N)), tuple(1 if j == ax else cs[j] for j in range(N))
    if kind == "low":
        return (0,) * N, tuple(ext_low)
    if kind == "far":
        return tuple(d - e for d, e in zip(cs, ext_far)), tuple(ext_far)
    if kind == "rows":
        return inner[0][:-1] + (0,), inner[1][:-1] + (cs[-1],)
    if kind == "straddle" and wide:  # odd lo below a multiple of 32 of this grid, the box's end above it
        j = wide[pick]
        mult = 32 * (1 + m % ((cs[j] - 2) // 32))  # 32 <= mult <= cs[j] - 2
        lo_j = mult - min(back, 31)                 # odd, < mult, >= 1
        hi_j = min(cs[j], mult + fwd)               # > mult
        lo, ext = list(inner[0]), list(inner[1])
        lo[j], ext[j] = lo_j, hi_j - lo_j
        return tuple(lo), tuple(ext)
    return inner  # interior; a grid too short to straddle a multiple of 32


def draw_case(k):
    c = {"k": k}
    c["drawn"], shape = draw_shape()
    c["shape"] = shape
    N = len(shape)
    n = int(np.prod(shape))
    c["dtype"] = "float64" if rng.random() < 0.5 else "float32"
    c["interp"] = int(rng.integers(0, 2))
    c["direction"] = int(rng.integers(0, math.factorial(N)))
    c["alpha"], c["beta"] = float(rng.choice(ALPHAS)), float(rng.choice(BETAS))
    a = ANCHORS[int(rng.integers(0, len(ANCHORS)))]
    odd = rng.random() < 0.05
    odd_stride = int(rng.choice([12, 24]))
    c["anchor"] = odd_stride if odd else a
    c["odd"] = bool(odd)
    c["field_seed"] = int(rng.integers(1, 1 << 30))
    spikes, n_spikes = rng.random() < 1 / 3, int(rng.integers(20, 201))
    c["spikes"] = rng.integers(0, n, n_spikes) if spikes else None
    nonfinite, n_nf = rng.random() < 0.2, int(rng.integers(3, 9))
    pos, val = rng.integers(0, n, n_nf), rng.choice([np.nan, np.inf, -np.inf], n_nf)
    c["nonfinite"] = (pos, val) if nonfinite else None
    u = rng.random()
    c["kind"] = (("own", "payload")[u < 0.5] if odd else "oracle" if u < (0.45 if N >= 2 else 0.3) else "own" if u < 0.75 else "payload")
    # the items
    top = max((d - 1).bit_length() for d in shape)  # the level whose grid is one point
    kmax = min(4, top)
    n_items = int(rng.integers(1, 25))
    single = rng.random() < 0.25
    one_level = int(rng.integers(0, kmax + 1))
    levels = [int(v) for v in rng.integers(0, kmax + 1, n_items)]
    kinds = [BOX_KINDS[int(v)] for v in rng.integers(0, len(BOX_KINDS), n_items)]
    eff = DEF_ANCHOR[N] if c["anchor"] is None else c["anchor"]
    all_anchor_level = (eff - 1).bit_length() if (eff > 0 and not odd and max(shape) > eff) else None
    c["all_anchor"] = c["one_point"] = 0
    if single:
        levels = [one_level] * n_items
    elif n_items >= 3:
        levels[1] = top
        if all_anchor_level is not None and all_anchor_level <= top:
            levels[0] = all_anchor_level
    items = []
    for lv, kd in zip(levels, kinds):
        cs = coarse_shape(shape, lv)
        lo, ext = draw_box(cs, kd)
        items.append((lv, lo, ext))
        c["all_anchor"] += int(all_anchor_level is not None and lv >= all_anchor_level and lv > 0)
        c["one_point"] += int(lv >= top)
    c["items"], c["single"], c["top"] = items, len(set(levels)) == 1, top
    # the route
    c["chain"] = [0, CHAIN_DEFAULT, 1 << 20][int(rng.integers(0, 3))]
    c["by_level"] = bool(rng.random() < 0.25)
    c["route"] = "by_level" if c["by_level"] else "chain" if (c["single"] and c["chain"] > 0) else "merged"
    # the sinks and their options (all drawn, whichever two run)
    c["sinks"] = [SINKS[int(i)] for i in rng.choice(5, 2, replace=False)]
    second = "by_level" if rng.random() < 0.5 else "chain"
    c["second"] = "chain" if c["single"] else second  # (a request of one level has no level groups: its other route is the other chain setting)
    c["bins"] = int(rng.choice([0, 7, 1024]))
    c["sel_range"], c["invert"], c["nan"], c["cap_shift"] = int(rng.integers(0, 4)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.integers(0, 6))
    c["nan_code"] = int(rng.integers(0, 256))
    c["coord"], c["clamp"], c["q_seed"] = ("float32", "float64")[int(rng.integers(0, 2))], bool(rng.integers(0, 2)), int(rng.integers(1, 1 << 30))
    return c


def tag_of(c):
    return ("case %d (SEED %d) %s%s %s %s interp %d direction %d alpha %g beta %g anchor %s%s%s; %d items%s, chain %d%s, sinks %s then %s" % (
        c["k"], SEED, "x".join(map(str, c["shape"])), "" if c["drawn"] == c["shape"] else " (drawn %s)" % "x".join(map(str, c["drawn"])), c["dtype"], c["kind"],
        c["interp"], c["direction"], c["alpha"], c["beta"], c["anchor"], " spikes %d" % len(c["spikes"]) if c["spikes"] is not None else "",
        " nonfinite %d" % len(c["nonfinite"][0]) if c["nonfinite"] else "", len(c["items"]), " of one level" if c["single"] else "", c["chain"],
        " by level" if c["by_level"] else "", "+".join(c["sinks"]), c["second"]))


def conf_of(c, algo=sz3_amd.ALGO_INTERP):
    kw = dict(interpAlgo=c["interp"], interpDirection=c["direction"], interpAlpha=c["alpha"], interpBeta=c["beta"])
    if c["anchor"] is not None:
        kw["interpAnchorStride"] = c["anchor"]
    if algo != sz3_amd.ALGO_INTERP:
        kw.update(lorenzo=1, lorenzo2=0, regression=0)
    return conf_for(c["shape"], algo=algo, **kw)


def field_of(c):
    a = smooth(c["shape"], c["dtype"], seed=c["field_seed"])
    if c["spikes"] is not None:
        a.reshape(-1)[c["spikes"]] = 1e6
    if c["nonfinite"]:
        a.reshape(-1)[c["nonfinite"][0]] = c["nonfinite"][1]
    return a


def sample_queries(c):
    """per item a query, from the case's own seed: a lattice that crosses the box's faces for every third box, else coordinates (some outside, one
    NaN row, the first grid point) in the drawn type"""
    q = np.random.default_rng(c["q_seed"])
    out = []
    for i, (_, _, ext) in enumerate(c["items"]):
        N = len(ext)
        if i % 3 == 0:
            counts = (2, 3, 5)
            out.append(([-0.75] * N, [[(e + 1.5) / cn * (1.0 if j % 3 == ax else 0.37) for j, e in enumerate(ext)] for ax, cn in enumerate(counts)], counts))
        else:
            n = int(q.integers(1, 300))
            co = np.stack([q.uniform(-0.5, e - 0.5, n) for e in ext], axis=1)
            co[0] = 0.0
            if n > 2:
                co[n // 2, int(q.integers(0, N))] = np.nan
                co[n - 1] = [e - 1 for e in ext]
            out.append(np.ascontiguousarray(co.astype(c["coord"])))
    return out


# ---- DRY: every drawn request through the pure host functions ----------------------------------------------------------------------------------
def dry(c):
    """-> the list of plan calls that did not answer as they must (success; SZ3HIP_EUNSUPPORTED for a stride that is no power of two)"""
    import sink_models as M
    conf, dt, items = conf_of(c), c["dtype"], c["items"]
    calls = []
    for lv, lo, ext in items[:3]:
        calls.append(("region_plan", lambda lo=lo, ext=ext: sz3_amd.region_plan(conf, lo, ext)))
        calls.append(("tile_plan", lambda lv=lv, lo=lo, ext=ext: sz3_amd.tile_plan(conf, lv, lo, ext)))
    for lv in sorted({it[0] for it in items}):
        calls.append(("tiles_plan", lambda lv=lv: sz3_amd.tiles_plan(conf, lv, [it[1:] for it in items if it[0] == lv])))
    calls.append(("request_plan", lambda: sz3_amd.request_plan(conf, dt, items)))
    calls.append(("reduce_plan", lambda: sz3_amd.reduce_plan(conf, dt, items, c["bins"], -0.5, 0.75)))
    calls.append(("select_plan", lambda: sz3_amd.select_plan(conf, dt, items, -0.5, 0.75, [int(np.prod(it[2])) for it in items], c["invert"], c["nan"])))
    for t, lut in (("u8", None), ("u16", None), ("f16", None), ("f32", None), ("lut32", 2), ("lut32", 1024)):
        kw = {} if t in ("f16", "f32") else dict(lo=-0.5, hi=0.75, nan_code=c["nan_code"], lut=lut)  # (a float output takes no window)
        calls.append(("map_plan " + t, lambda t=t, kw=kw: sz3_amd.map_plan(conf, dt, items, t, **kw)))
    qs = [int(np.prod(q[2])) if isinstance(q, tuple) else len(q) for q in sample_queries(c)]
    for mode in ("nearest", "linear"):
        calls.append(("sample_plan " + mode, lambda mode=mode: sz3_amd.sample_plan(conf, dt, items, qs, mode, c["clamp"])))
    for axis in range(len(c["shape"])):
        for op, out in M.combos():
            calls.append(("project_plan %s axis %d" % (op, axis), lambda op=op, out=out, axis=axis: sz3_amd.project_plan(conf, dt, items, op, axis, out)))
    bad = []
    for name, f in calls:
        try:
            f()
            if c["odd"]:
                bad.append("%s accepted an anchor stride that is no power of two" % name)
        except sz3_amd.SZ3HipError as e:
            if not (c["odd"] and e.code == EUNSUPPORTED):
                bad.append("%s refused the draw: %s" % (name, str(e)[:120]))
    return bad


# ---- the device legs ---------------------------------------------------------------------------------------------------------------------------
def set_route(chain, by_level, extra=0):
    sz3_amd.set_chain_points(chain)
    L.sz3hip_debug_flags2((BY_LEVEL if by_level else 0) | extra)


def second_route(c):
    if c["second"] == "by_level":
        return c["chain"], not c["by_level"]
    return (0 if c["chain"] > 0 else CHAIN_DEFAULT), c["by_level"]


def finite_sorted(full_np):
    flat = np.sort(full_np.astype(np.float64).reshape(-1))
    return flat[np.isfinite(flat)]


def window_of(flat):
    q = lambda f: float(flat[min(int(f * flat.size), flat.size - 1)])  # noqa: E731
    lo, hi = q(0.25), q(0.75)
    return lo, (hi if hi > lo else lo + 1.0)


def run_sink(name, st, c, slices, flat, chain, by_level, check, what):
    """one sink over the case's items under the route (chain, by_level); check: against the numpy rule. -> the results' bytes"""
    import sink_models as M
    items = c["items"]
    sig = []
    lo, hi = window_of(flat)
    set_route(chain, by_level)
    if name == "reduce":
        stt, hist = st.reduce(items, c["bins"], lo, hi).numpy()
        if check:
            with contextlib.redirect_stdout(io.StringIO()):
                for i, s in enumerate(slices):
                    M.reduce_check_box(stt[i], None if hist is None else hist[i], s, c["bins"], lo, hi, "%s reduce box %d %s" % (what, i, items[i]))
        sig = [stt.tobytes(), b"" if hist is None else hist.tobytes()]
    elif name == "select":
        q = lambda f: float(flat[min(int(f * flat.size), flat.size - 1)])  # noqa: E731
        lo, hi = [(q(0.45), q(0.55)), (q(0.9), float(flat[-1])), (float(flat[0]), float(flat[-1])), (q(0.6), q(0.4))][c["sel_range"]]
        caps = []
        for i, s in enumerate(slices):  # capacities below and above the hit count, in turn
            n = int(M.pred(s.astype(np.float64).reshape(-1), lo, hi, c["invert"], c["nan"]).sum())
            caps.append([s.size, max(n - 1, 0), n + 1, n // 2, 0, n][(i + c["cap_shift"]) % 6])
        rc, heads, index, value = M.raw_select(st, items, caps, lo, hi, c["invert"], c["nan"])
        assert rc == 0, L.sz3hip_last_error().decode()
        torch.cuda.synchronize()
        h = heads.cpu().numpy()
        ix, vl = [t.cpu().numpy() for t in index], [t.cpu().numpy() for t in value]
        if check:
            for i, s in enumerate(slices):
                M.select_check_box(h[i], ix[i], vl[i], s, caps[i], lo, hi, c["invert"], c["nan"], "%s select box %d %s [%r, %r]:" % (what, i, items[i], lo, hi))
        sig = [h.tobytes()] + [t.tobytes() for t in ix] + [t.tobytes() for t in vl]
    elif name == "map":
        for out_type, lut_n in (("u8", 0), ("u16", 0), ("f16", 0), ("f32", 0), ("lut32", 2), ("lut32", 1024)):
            lut = M.make_lut(lut_n) if lut_n else None
            kw = M.opts_for(out_type, lo, hi, c["nan_code"], lut)
            for form in (0, PLAIN):
                set_route(chain, by_level, form)
                outs = [M.map_filled(ext, out_type) for _, _, ext in items]
                st.map([it + (o,) for it, o in zip(items, outs)], out_type, **kw)
                atlas, views, where = M.texel_atlas(items, out_type)
                st.map([it + (v,) for it, v in zip(items, views)], out_type, **kw)
                torch.cuda.synchronize()
                for i, s in enumerate(slices):
                    got = M.map_host(outs[i], out_type)
                    if check:
                        want = M.map_expected(s, out_type, lo, hi, c["nan_code"], lut)
                        w = "%s map %s lut %d form %d box %d %s:" % (what, out_type, lut_n, form, i, items[i])
                        M.same_texels(got, want, out_type, w + " contiguous,")
                        M.same_texels(M.map_host(views[i], out_type), want, out_type, w + " atlas,")
                    sig.append(got.tobytes())
                assert M.map_untouched(atlas, out_type, where), "%s map %s form %d: a byte outside the rectangles was written" % (what, out_type, form)
        set_route(chain, by_level)
    elif name == "sample":
        qs = sample_queries(c)
        held = [torch.from_numpy(q).to(DEV) if isinstance(q, np.ndarray) else q for q in qs]
        for mode in ("nearest", "linear"):
            fill = -7.25 if c["clamp"] else M.NAN
            outs = st.sample(items, held, mode, c["clamp"], fill)
            torch.cuda.synchronize()
            for i, (s, q) in enumerate(zip(slices, qs)):
                got = outs[i].cpu().numpy().reshape(-1)
                if check:
                    M.same_values(got, M.np_sample(s, q if isinstance(q, np.ndarray) else M.np_lattice(*q), mode, c["clamp"], fill),
                                  "%s sample %s clamp %d %s coordinates box %d %s:" % (what, mode, c["clamp"], c["coord"], i, items[i]))
                sig.append(got.tobytes())
    elif name == "project":
        for axis in range(len(c["shape"])):
            folds = [M.np_fold(s, axis) for s in slices] if check else None
            shapes = [M.flat(ext, axis) for _, _, ext in items]
            for op, out in M.combos():
                oname = M.out_name(op, out, st.dtype)
                outs = [M.project_filled(s, oname) for s in shapes]
                st.project([it + (o,) for it, o in zip(items, outs)], op, axis, out_dtype=out)
                at, views, where = M.atlas_of(shapes, oname)
                st.project([it + (v,) for it, v in zip(items, views)], op, axis, out_dtype=out)
                torch.cuda.synchronize()
                for i in range(len(items)):
                    got = M.project_host(outs[i])
                    if check:
                        want = M.project_expected(folds[i], op, axis, oname)
                        w = "%s project %s axis %d -> %s box %d %s:" % (what, op, axis, oname, i, items[i])
                        M.same_bytes(got, want, w + " contiguous,")
                        M.same_bytes(M.project_host(views[i]), want, w + " atlas,")
                    sig.append(got.tobytes())
                assert M.project_untouched(at, where), "%s project %s axis %d: a byte outside the rectangles was written" % (what, op, axis)
    return sig, st.stats()["chain_levels_last_request"]


def same_box(got, full, lv, lo, ext, what):
    import sink_models as M
    want = M.coarse_view(full, lv)[box_slices(lo, ext)]
    assert tuple(got.shape) == tuple(ext) == tuple(want.shape), what
    assert np.array_equal(raw(got), raw(want)), what + " differs from the expected array's slice"


def leg_a(c, blob, payload, full, fast):
    """three of the boxes through the calls that are no Stream"""
    import sink_models as M
    dt = np.dtype(c["dtype"])
    td = getattr(torch, dt.name)
    three = c["items"][:3]
    if blob is not None:
        before = sz3_amd.get_sparse_decode()
        try:
            for sparse in (True, False):
                sz3_amd.set_sparse_decode(sparse)
                w = "sparse %d" % sparse
                for lv, lo, ext in three:
                    same_box(sz3_amd.decompress_tile(blob, dt, lv, lo, ext, device=DEV)[0], full, lv, lo, ext, "%s decompress_tile level %d %s %s" % (w, lv, lo, ext))
                    same_box(sz3_amd.decompress_region(blob, dt, lo, ext, device=DEV)[0], full, 0, lo, ext, "%s decompress_region %s %s" % (w, lo, ext))
                for lv in sorted({it[0] for it in three}):
                    bx = [it[1:] for it in three if it[0] == lv]
                    for t, (lo, ext) in zip(sz3_amd.decompress_tiles(blob, dt, lv, bx, device=DEV)[0], bx):
                        same_box(t, full, lv, lo, ext, "%s decompress_tiles level %d %s %s" % (w, lv, lo, ext))
                lv = three[0][0]
                cs = M.coarse_shape(c["shape"], lv)
                same_box(sz3_amd.decompress_coarse(blob, dt, lv, device=DEV)[0], full, lv, (0,) * len(cs), cs, "%s decompress_coarse level %d" % (w, lv))
        finally:
            sz3_amd.set_sparse_decode(before)
    elif fast:  # (the context's partial decodes take interpolation payloads)
        dc, pl, size = payload
        s = torch.cuda.current_stream().cuda_stream
        for lv, lo, ext in three:
            o = torch.full(tuple(ext), M.SENTINEL, dtype=td, device=DEV)
            dc.decompress_tile(pl.data_ptr(), size, lv, lo, ext, o.data_ptr(), s)
            same_box(o, full, lv, lo, ext, "DeviceCompressor.decompress_tile level %d %s %s" % (lv, lo, ext))
            o = torch.full(tuple(ext), M.SENTINEL, dtype=td, device=DEV)
            dc.decompress_region(pl.data_ptr(), size, lo, ext, o.data_ptr(), s)
            same_box(o, full, 0, lo, ext, "DeviceCompressor.decompress_region %s %s" % (lo, ext))
        for lv in sorted({it[0] for it in three}):
            bx = [it[1:] for it in three if it[0] == lv]
            outs = [torch.full(tuple(ext), M.SENTINEL, dtype=td, device=DEV) for _, ext in bx]
            dc.decompress_tiles(pl.data_ptr(), size, lv, bx, [o.data_ptr() for o in outs], s)
            for o, (lo, ext) in zip(outs, bx):
                same_box(o, full, lv, lo, ext, "DeviceCompressor.decompress_tiles level %d %s %s" % (lv, lo, ext))


def leg_b(c, st, full, fast):
    """Stream.request three times, Stream.tiles for a request of one level, the handle's stats -> chain levels of the first request"""
    import sink_models as M
    items = c["items"]
    td = M.tdt(st)
    set_route(c["chain"], c["by_level"])
    outs = [torch.full(tuple(ext), M.SENTINEL, dtype=td, device=DEV) for _, _, ext in items]
    st.request([it + (o,) for it, o in zip(items, outs)])
    torch.cuda.synchronize()
    s = st.stats()
    for o, (lv, lo, ext) in zip(outs, items):
        same_box(o, full, lv, lo, ext, "request, contiguous, level %d %s %s" % (lv, lo, ext))
    assert s["fast"] == (1 if fast else 0)
    assert s["huffman_stages"] == (1 if fast else 0), "huffman_stages %d" % s["huffman_stages"]
    if not c["single"] or not fast:
        assert s["chain_levels_last_request"] == 0, "a request of %s took the chain" % ("several levels" if fast else "a fallback handle")
    atlas, views = M.atlas_for(st, items, pad=1)
    st.request([it + (v,) for it, v in zip(items, views)])
    torch.cuda.synchronize()
    for v, (lv, lo, ext) in zip(views, items):
        same_box(v, full, lv, lo, ext, "request, atlas, level %d %s %s" % (lv, lo, ext))
    assert M.untouched(atlas, views), "request, atlas: an element outside the rectangles was written"
    bufs = [torch.full(tuple(ext[:-1]) + (2 * ext[-1],), M.SENTINEL, dtype=td, device=DEV) for _, _, ext in items]
    views = [b[..., ::2] for b in bufs]
    st.request([it + (v,) for it, v in zip(items, views)])
    torch.cuda.synchronize()
    for b, v, (lv, lo, ext) in zip(bufs, views, items):
        same_box(v, full, lv, lo, ext, "request, step 2 along x, level %d %s %s" % (lv, lo, ext))
        assert M.untouched(b, [v]), "request, step 2 along x: an element between the view's was written"
    if c["single"]:
        lv = items[0][0]
        for t, (_, lo, ext) in zip(st.tiles(lv, [it[1:] for it in items]), items):
            same_box(t, full, lv, lo, ext, "tiles level %d %s %s" % (lv, lo, ext))
    assert st.stats()["huffman_stages"] == (1 if fast else 0)
    return s["chain_levels_last_request"]


def open_case(c, a, T):
    """-> (Stream, expected array on the device, blob or None, payload triple or None, the failures met on the way)"""
    bad = []
    conf = conf_of(c)
    if c["odd"]:  # no interpolation stream of this stride can be written: the refusal, then the fallback container of the same Config
        try:
            container(a, conf)
            bad.append("the compressor took an anchor stride that is no power of two")
        except sz3_amd.SZ3HipError as e:
            if "Anchor stride" not in str(e):
                bad.append("the refusal of the stride reads: %s" % str(e)[:100])
        conf = conf_of(c, sz3_amd.ALGO_LORENZO_REG)
    if c["kind"] == "oracle":
        from oracle_binding import ALGO_INTERP, make_config, oracle_compress, oracle_decompress
        kw = dict(algo=ALGO_INTERP, abs_eb=1e-2, quantbinCnt=1024, interp_algo=c["interp"], interpDirection=c["direction"], interpAlpha=c["alpha"], interpBeta=c["beta"])
        if c["anchor"] is not None:
            kw["interpAnchorStride"] = c["anchor"]
        blob = oracle_compress(a, make_config(c["shape"], **kw))
        want, _ = oracle_decompress(blob, a.dtype, a.shape)
        full = torch.from_numpy(want).to(DEV)
        mine, _ = sz3_amd.decompress(blob, a.dtype, device=DEV)
        if not np.array_equal(raw(mine), raw(full)):
            neq = int((raw(mine).view("u%d" % a.itemsize) != raw(full).view("u%d" % a.itemsize)).sum())
            bad.append("oracle leg: the full decode differs from the oracle's array in %d of %d values" % (neq, a.size))
        return sz3_amd.open_stream(blob, a.dtype, device=DEV), full, blob, None, bad
    if c["kind"] == "payload":
        # A context's lists hold max(1024, n / 32) raw records each; a draw with more of them (a dense anchor grid, spikes and what they spoil)
        # ends in SZ3HIP_EOUTLIERS, the context's documented answer. The case then runs on the host API's container of the same draw, which
        # writes such an array lossless: a fallback handle, counted in the fast share like every other.
        try:
            dc, pl, size, full = device_payload(a, conf)
            return dc.open_stream(pl.data_ptr(), size, torch.cuda.current_stream().cuda_stream), full, None, (dc, pl, size), bad
        except sz3_amd.SZ3HipError as e:
            if e.code != EOUTLIERS:
                raise
            T["payload_refused"] += 1
            c["kind"] = "own (the context's lists cannot hold the payload)"
    blob = container(a, conf)
    full, _ = sz3_amd.decompress(blob, a.dtype, device=DEV)
    return sz3_amd.open_stream(blob, a.dtype, device=DEV), full, blob, None, bad


def guard(bad, leg, f):
    """runs a leg; an assertion or a refusal is a failure of that leg, an error of the HIP runtime ends the sweep"""
    try:
        return f()
    except AssertionError as e:
        bad.append("leg %s: %s" % (leg, str(e)[:300]))
    except sz3_amd.SZ3HipError as e:
        if e.code == EHIP:
            raise HipDown("leg %s: %s" % (leg, e))
        bad.append("leg %s: %s" % (leg, str(e)[:300]))
    except RuntimeError as e:  # (torch's: a fault of an earlier launch surfaces here)
        raise HipDown("leg %s: %s" % (leg, str(e)[:300]))
    return None


def run_case(c, T):
    import sink_models as M
    bad = []
    a = field_of(c)
    st, full, blob, payload, b0 = open_case(c, a, T)
    bad += b0
    with st:
        fast = st.stats()["fast"] == 1
        if c["odd"]:
            if fast:
                bad.append("a stride that is no power of two, and the handle is fast")
        else:
            T["interp_cases"] += 1
            T["fallback"] += int(not fast)
            if c["kind"] == "payload" and not fast:
                bad.append("a context's interpolation payload opened as a fallback handle")
        T["fast" if fast else "slow"] += 1
        full_np = full.cpu().numpy()
        slices = [M.coarse_view(full_np, lv)[box_slices(lo, ext)] for lv, lo, ext in c["items"]]
        flat = finite_sorted(full_np)
        guard(bad, "A", lambda: leg_a(c, blob, payload, full, fast))
        ch = guard(bad, "B", lambda: leg_b(c, st, full, fast))
        route = lambda chain_levels, by_level: "chain" if chain_levels else "by_level" if (by_level and fast and not c["single"]) else "merged"  # noqa: E731
        if ch is not None:
            T["routes"][route(ch, c["by_level"])] += 1
        for name in c["sinks"]:
            first = guard(bad, "C " + name, lambda: run_sink(name, st, c, slices, flat, c["chain"], c["by_level"], True, "route 1"))
            if first is None:
                continue
            T["sink_routes"]["%s/%s" % (name, route(first[1], c["by_level"]))] += 1
            ch2, by2 = second_route(c)
            again = guard(bad, "C %s, second route" % name, lambda: run_sink(name, st, c, slices, flat, ch2, by2, False, "route 2"))
            if again is not None:
                T["sink_routes"]["%s/%s" % (name, route(again[1], by2))] += 1
                if again[0] != first[0]:
                    bad.append("leg C %s: chain %d by level %d and chain %d by level %d give other bytes" % (name, c["chain"], c["by_level"], ch2, by2))
    if payload is not None:
        payload[0].close()
    return bad


def main():
    from collections import Counter
    T = {"rank": Counter(), "direction": Counter(), "anchor": Counter(), "kind": Counter(), "route_drawn": Counter(), "sink_route_drawn": Counter(), "sink": Counter(),
         "routes": Counter(), "sink_routes": Counter(), "all_anchor": 0, "one_point": 0, "odd": 0, "rank2plus": 0, "oracle2plus": 0, "fast": 0, "slow": 0,
         "interp_cases": 0, "fallback": 0, "payload_refused": 0}
    failures = n_run = 0
    down = None
    for k in range(N_CASES):
        c = draw_case(k)
        if SEL and k not in SEL:
            continue
        n_run += 1
        N = len(c["shape"])
        T["rank"][N] += 1
        T["direction"]["%dD:%d" % (N, c["direction"])] += 1
        T["anchor"][str(c["anchor"])] += 1
        T["kind"][c["kind"]] += 1
        T["route_drawn"][c["route"]] += 1
        for s in c["sinks"]:
            T["sink"][s] += 1
            T["sink_route_drawn"]["%s/%s" % (s, c["route"])] += 1
        T["all_anchor"] += c["all_anchor"]
        T["one_point"] += c["one_point"]
        T["odd"] += int(c["odd"])
        T["rank2plus"] += int(N >= 2)
        T["oracle2plus"] += int(N >= 2 and c["kind"] == "oracle")
        tag = tag_of(c)
        if VERBOSE:
            print(tag, flush=True)
        if DRY:
            bad = dry(c)
        else:
            try:
                bad = run_case(c, T)
            except HipDown as e:
                bad, down = ["%s — the sweep ends here" % e], e
            except (sz3_amd.SZ3HipError, RuntimeError) as e:
                if getattr(e, "code", EHIP) == EHIP:  # (torch's RuntimeError: a fault of an earlier launch surfaces there)
                    bad, down = ["%s — the sweep ends here" % str(e)[:300]], e
                else:
                    bad = ["opening the case: %s" % str(e)[:300]]
            finally:
                sz3_amd.set_chain_points(CHAIN_DEFAULT)
                L.sz3hip_debug_flags2(0)
        for b in bad:
            failures += 1
            print("FAIL %s: %s" % (tag, b), flush=True)
        if down is not None:
            break
    if not DRY and T["fallback"] * 10 > T["interp_cases"]:
        failures += 1
        print("FAIL fast share: %d of the %d cases drawn as interpolation streams of a power-of-two stride came back with fast == 0 (at most one in ten may)"
              % (T["fallback"], T["interp_cases"]), flush=True)
    show = lambda cn: ", ".join("%s %d" % (k, cn[k]) for k in sorted(cn, key=str))  # noqa: E731
    print("rank: %s | kind: %s | strides no power of two: %d" % (show(T["rank"]), show(T["kind"]), T["odd"]))
    print("direction: %s" % show(T["direction"]))
    print("anchor: %s" % show(T["anchor"]))
    print("routes as drawn: %s | sinks: %s | sink x route as drawn: %s" % (show(T["route_drawn"]), show(T["sink"]), show(T["sink_route_drawn"])))
    print("all-anchor items %d, one-point grids %d, oracle among rank >= 2: %d of %d" % (T["all_anchor"], T["one_point"], T["oracle2plus"], T["rank2plus"]))
    if not DRY:
        print("handles: fast %d, fallback %d; fallback among the %d interpolation cases of a power-of-two stride: %d; payloads a context's lists could not hold: %d"
              % (T["fast"], T["slow"], T["interp_cases"], T["fallback"], T["payload_refused"]))
        print("requests per route (leg B): %s | sink x route (leg C): %s" % (show(T["routes"]), show(T["sink_routes"])))
    print("TALLY " + json.dumps({k: (dict(v) if isinstance(v, Counter) else v) for k, v in T.items()}, sort_keys=True))
    print("cases %d (SEED %d, %s) failures %d" % (n_run, SEED, "DRY: plans only" if DRY else "on the device", failures))
    sys.exit(2 if down is not None else 1 if failures else 0)


main()

"""The tile decode without a GPU: the symbols and Python names, the argument checks, the geometry at a level against the region plan of the
coarse grid (DESIGN.md section 13's identity), and the list of decoder units — against a Python model of its definition (row-runs of the
pass windows, walked with the schedule model of test_region_cpu.py) and against a brute-force walk over every predicted point."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import sz3_amd
import test_region_cpu as R

L = sz3_amd.lib()
CODES = R.CODES
DEF_ANCHOR = R.DEF_ANCHOR
UNIT = 512


def test_symbols_and_names_exist():
    for sym in ("sz3hip_tile_plan_for", "sz3hip_tile_units_for", "sz3hip_decompress_tile_to_device", "sz3hip_decompress_device_tile",
                "sz3hip_set_sparse_decode", "sz3hip_get_sparse_decode", "sz3hip_debug_tile_units"):
        assert hasattr(L, sym), sym
    for name in ("tile_plan", "tile_units", "decompress_tile", "set_sparse_decode", "get_sparse_decode"):
        assert callable(getattr(sz3_amd, name)), name
    assert callable(sz3_amd.DeviceCompressor.decompress_tile)


def _box(v):
    return (C.c_uint64 * 4)(*v)


def _tplan(c, level, lo, ext):
    plan = sz3_amd._CTilePlan()
    rc = L.sz3hip_tile_plan_for(C.byref(c), level, _box(lo), _box(ext), C.byref(plan))
    return rc, plan


def _units(c, level, lo, ext):
    n = C.c_uint64(0)
    rc = L.sz3hip_tile_units_for(C.byref(c), level, _box(lo), _box(ext), None, 0, C.byref(n))
    assert rc in (0, CODES["SZ3HIP_ECAPACITY"]), L.sz3hip_last_error().decode()
    u = np.zeros(int(n.value), np.uint32)
    if u.size:
        assert L.sz3hip_tile_units_for(C.byref(c), level, _box(lo), _box(ext), u.ctypes.data, u.size, C.byref(n)) == 0
        assert n.value == u.size
    return u


def _coarse(dims, k):
    return tuple(((d - 1) >> k) + 1 for d in dims)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_level_range():
    c = R._cconf((20, 30, 40))
    for level in (-1, 31, 1000):
        rc, _ = _tplan(c, level, (0, 0, 0), (1, 1, 1))
        assert rc == CODES["SZ3HIP_EINVAL"] and "level" in L.sz3hip_last_error().decode()
        n = C.c_uint64(0)
        assert L.sz3hip_tile_units_for(C.byref(c), level, _box((0, 0, 0)), _box((1, 1, 1)), None, 0, C.byref(n)) == CODES["SZ3HIP_EINVAL"]
    assert _tplan(c, 30, (0, 0, 0), (1, 1, 1))[0] == 0


def test_box_is_checked_against_the_coarse_grid():
    c = R._cconf((20, 30, 40))  # level 2: the grid is 5 x 8 x 10
    assert _tplan(c, 2, (0, 0, 0), (5, 8, 10))[0] == 0
    rc, _ = _tplan(c, 2, (0, 0, 0), (5, 8, 11))
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 2" in L.sz3hip_last_error().decode()
    rc, _ = _tplan(c, 2, (5, 0, 0), (1, 1, 1))
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 0" in L.sz3hip_last_error().decode()
    rc, _ = _tplan(c, 2, (0, 0, 0), (5, 0, 10))
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 1" in L.sz3hip_last_error().decode()
    rc, _ = _tplan(c, 2, (0, 2 ** 64 - 1, 0), (1, 2, 1))  # (lo + ext wraps)
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 1" in L.sz3hip_last_error().decode()


def test_null_arguments():
    c = R._cconf((20, 30))
    plan = sz3_amd._CTilePlan()
    box = _box((1, 1, 0, 0))
    n = C.c_uint64(0)
    for args in ((None, 1, box, box, C.byref(plan)), (C.byref(c), 1, None, box, C.byref(plan)), (C.byref(c), 1, box, None, C.byref(plan)),
                 (C.byref(c), 1, box, box, None)):
        assert L.sz3hip_tile_plan_for(*args) == CODES["SZ3HIP_EINVAL"] and "NULL" in L.sz3hip_last_error().decode()
    for args in ((None, 1, box, box, None, 0, C.byref(n)), (C.byref(c), 1, None, box, None, 0, C.byref(n)), (C.byref(c), 1, box, None, None, 0, C.byref(n)),
                 (C.byref(c), 1, box, box, None, 0, None), (C.byref(c), 1, box, box, None, 4, C.byref(n))):
        assert L.sz3hip_tile_units_for(*args) == CODES["SZ3HIP_EINVAL"] and "NULL" in L.sz3hip_last_error().decode()
    assert L.sz3hip_decompress_device_tile(None, 0x1000, 4096, 1, box, box, 0x2000, None) == CODES["SZ3HIP_EINVAL"]


def test_anchor_stride_no_power_of_two_is_unsupported():
    c = R._cconf((50, 60, 70), anchor=12)
    rc, _ = _tplan(c, 1, (1, 1, 1), (4, 4, 4))
    assert rc == CODES["SZ3HIP_EUNSUPPORTED"] and "power of two" in L.sz3hip_last_error().decode()
    n = C.c_uint64(0)
    assert L.sz3hip_tile_units_for(C.byref(c), 1, _box((1, 1, 1)), _box((4, 4, 4)), None, 0, C.byref(n)) == CODES["SZ3HIP_EUNSUPPORTED"]


def _tile_call(blob, dt, level, lo, ext, ptr, strides=None):
    c = sz3_amd.Config(1)
    rc = L.sz3hip_decompress_tile_to_device(C.byref(c._c), dt, blob.ctypes.data, blob.size, level, _box(lo) if lo else None, _box(ext) if ext else None, ptr,
                                            strides, None)
    return rc, c


def test_to_device_call_checks_before_anything_else():
    blob = R._lossless_container()  # 6 x 10; level 1: 3 x 5
    rc, c = _tile_call(blob, 0, 1, (0, 0), (3, 6), 0x1000)
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 1" in L.sz3hip_last_error().decode()
    assert tuple(c.dims) == (6, 10), "conf stays the full array's"
    rc, _ = _tile_call(blob, 0, 1, (0, 0), (0, 5), 0x1000)
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 0" in L.sz3hip_last_error().decode()
    rc, _ = _tile_call(blob, 0, 31, (0, 0), (1, 1), 0x1000)
    assert rc == CODES["SZ3HIP_EINVAL"] and "level" in L.sz3hip_last_error().decode()
    rc, _ = _tile_call(blob, 0, 1, None, None, 0x1000)
    assert rc == CODES["SZ3HIP_EINVAL"] and "NULL" in L.sz3hip_last_error().decode()
    rc, _ = _tile_call(blob, 7, 1, (0, 0), (2, 2), 0x1000)
    assert rc == CODES["SZ3HIP_EUNSUPPORTED"] and "integer" in L.sz3hip_last_error().decode()
    out = np.zeros(15, np.float32)  # (a host pointer: an error, never a host path)
    rc, _ = _tile_call(blob, 0, 1, (0, 0), (3, 5), out.ctypes.data)
    assert rc == CODES["SZ3HIP_EINVAL"] and "device memory" in L.sz3hip_last_error().decode() and not out.any()
    with pytest.raises(ValueError):
        sz3_amd.decompress_tile(blob, np.float32, 1, (0, 0), (3, 5))  # (neither device= nor out=)


def test_sparse_switch():
    before = sz3_amd.get_sparse_decode()
    try:
        sz3_amd.set_sparse_decode(0)
        assert sz3_amd.get_sparse_decode() is False
        sz3_amd.set_sparse_decode(1)
        assert sz3_amd.get_sparse_decode() is True
    finally:
        sz3_amd.set_sparse_decode(before)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
def _same_plan(a, b):
    assert a.n_levels == b.n_levels and a.points == b.points and a.scratch_elems == b.scratch_elems
    assert list(a.stride) == list(b.stride)
    for i in range(32):
        assert list(a.win_lo[i]) == list(b.win_lo[i]) and list(a.win_hi[i]) == list(b.win_hi[i]), i


def test_level_0_is_the_region_plan():
    rng = np.random.default_rng(13)
    for _ in range(300):
        dims, interp, direction, anchor, lo, ext = R._random_case(rng)
        c = R._cconf(dims, interp, direction, anchor)
        rc, tp = _tplan(c, 0, lo, ext)
        rc2, rp = R._plan(c, lo, ext)
        assert rc == 0 and rc2 == 0
        _same_plan(tp.region, rp)
        num = int(np.prod(dims))
        assert tp.units_total == -(-num // UNIT)


def _random_box(rng, dims):
    lo, ext = [], []
    for D in dims:
        kind = rng.random()
        if kind < 0.2:
            a, e = int(rng.integers(0, D)), 1
        elif kind < 0.35:
            a, e = 0, int(rng.integers(1, D + 1))
        elif kind < 0.5:
            e = int(rng.integers(1, D + 1))
            a = D - e
        else:
            a = int(rng.integers(0, D))
            e = int(rng.integers(1, D - a + 1))
        lo.append(a)
        ext.append(e)
    return lo, ext


def _random_tile(rng, max_shift_of_anchor=None):
    """(dims, interp, direction, anchor argument, anchor in force, k, lo, ext) with the box on the level-k grid"""
    dims, interp, direction, anchor, _, _ = R._random_case(rng)
    anchor = int(rng.choice([-1, 4, 8, 16, 32]))
    a = DEF_ANCHOR[len(dims) - 1] if anchor < 0 else anchor
    kmax = int(math.log2(a)) - 2
    k = int(rng.integers(0, kmax + 1))
    lo, ext = _random_box(rng, _coarse(dims, k))
    return dims, interp, direction, anchor, a, k, lo, ext


def test_identity_with_the_coarse_grids_region_plan():
    """the tile of level k is the region of the grid of every 2^k-th point: extents ((D - 1) >> k) + 1, anchor stride A >> k"""
    rng = np.random.default_rng(20261019)
    seen_k, seen_n = set(), set()
    for _ in range(600):
        dims, interp, direction, anchor, a, k, lo, ext = _random_tile(rng)
        rc, tp = _tplan(R._cconf(dims, interp, direction, anchor), k, lo, ext)
        assert rc == 0, L.sz3hip_last_error().decode()
        rc, rp = R._plan(R._cconf(_coarse(dims, k), interp, direction, a >> k), lo, ext)
        assert rc == 0
        _same_plan(tp.region, rp)
        assert tp.units_total == -(-int(np.prod(dims)) // UNIT), "the units are the FULL code array's"
        seen_k.add(k)
        seen_n.add(len(dims))
    assert seen_n == {1, 2, 3, 4} and {0, 1, 2, 3} <= seen_k


@pytest.mark.parametrize("dims,anchor,k", [((65, 47, 130), 4, 2), ((65, 47, 130), 4, 3), ((65, 47, 130), -1, 5), ((65, 47, 130), -1, 6), ((33, 70), 8, 3),
                                           ((5000,), 4, 2), ((9, 12, 17, 20), -1, 4)])
def test_every_coarse_point_is_an_anchor(dims, anchor, k):
    cd = _coarse(dims, k)
    c = R._cconf(dims, 1, 0, anchor)
    for lo, ext in (((0,) * len(dims), cd), (tuple(d - 1 for d in cd), (1,) * len(dims))):
        rc, tp = _tplan(c, k, lo, ext)
        assert rc == 0
        assert tp.region.n_levels == 0 and tp.region.points == 0
        assert tp.units_needed == 0 and _units(c, k, lo, ext).size == 0, "raw records alone: no code is read, the first point is none"
        assert tp.region.scratch_elems >= int(np.prod(ext))


def test_first_point_path_at_a_level():
    """no extent above the anchor stride: the first point is predicted by 0 from codes[0], at every level"""
    dims = (20, 20, 20)
    c = R._cconf(dims, 1, 0, -1)
    for k in (0, 1, 2, 4, 5):
        cd = _coarse(dims, k)
        rc, tp = _tplan(c, k, (0, 0, 0), cd)
        assert rc == 0 and tp.region.n_levels == max(0, 5 - k)
        u = _units(c, k, (0, 0, 0), cd)
        assert u.size >= 1 and u[0] == 0


# ---- the unit list -----------------------------------------------------------------------------------------------------------------------
def _pass_lattices(dims, interp, direction, anchor_eff, lo, ext, plan):
    """the pass windows' lattices, from the plan's windows (coordinates of the grid `dims`): yields one list of per-dimension coordinate arrays
    per pass — test_region_cpu._walk's loop without the stencils"""
    N = len(dims)
    nl = plan.n_levels
    perm = list(itertools.permutations(range(N)))[direction]
    pos = {perm[k]: k for k in range(N)}
    box = [(lo[j], lo[j] + ext[j] - 1) for j in range(N)]
    for b in range(nl):
        s = 1 << (nl - 1 - b)
        win = [(int(plan.win_lo[b][j]), int(plan.win_hi[b][j])) for j in range(N)]
        out = [(int(plan.win_lo[b + 1][j]), int(plan.win_hi[b + 1][j])) for j in range(N)] if b + 1 < nl else box
        for k in range(N):
            d = perm[k]
            defers = interp == 0 and N >= 3
            cl = []
            for j in range(N):
                start = s if j == d else 0
                step = 2 * s if (j == d or pos[j] > k) else s
                wl, wh = win[j] if pos[j] > k else out[j]
                if j == d and defers:
                    wl = max(0, wl - 2 * s)
                cl.append(R._lattice(start, step, wl, wh))
            if all(len(c) for c in cl):
                yield cl


def _full_offsets(dims):
    off = [1] * len(dims)
    for j in range(len(dims) - 2, -1, -1):
        off[j] = off[j + 1] * dims[j + 1]
    return off


def _model_units(dims, interp, direction, a, k, lo, ext, plan):
    """section 13's definition: per row-run the units from its first lattice point's code to its last's; unit 0 where the first point is read"""
    N = len(dims)
    cd = _coarse(dims, k)
    off = _full_offsets(dims)
    anchor_eff = a if any(d > a for d in dims) else 0
    marked = set()
    if anchor_eff == 0:
        marked.add(0)  # (the coarsest window always holds the first point: its stride is at least half the largest extent)
    for cl in _pass_lattices(cd, interp, direction, anchor_eff >> k, lo, ext, plan):
        x = cl[N - 1]
        rows = np.zeros(1, np.int64)
        for j in range(N - 1):
            rows = (rows[:, None] + (cl[j].astype(np.int64) << k)[None, :] * off[j]).reshape(-1)
        i0 = rows + (int(x[0]) << k)
        i1 = rows + (int(x[-1]) << k)
        for u0, u1 in zip(i0 // UNIT, i1 // UNIT):
            marked.update(range(int(u0), int(u1) + 1))
    return np.array(sorted(marked), np.uint32)


def _read_units(dims, interp, direction, a, k, lo, ext, plan):
    """brute force: the unit of the full code index of every predicted point of every pass (and of the first point)"""
    N = len(dims)
    cd = _coarse(dims, k)
    off = _full_offsets(dims)
    anchor_eff = a if any(d > a for d in dims) else 0
    units = {0} if anchor_eff == 0 else set()
    for cl in _pass_lattices(cd, interp, direction, anchor_eff >> k, lo, ext, plan):
        idx = np.zeros(1, np.int64)
        for j in range(N):
            idx = (idx[:, None] + (cl[j].astype(np.int64) << k)[None, :] * off[j]).reshape(-1)
        assert idx.max() < int(np.prod(dims))
        units.update(np.unique(idx // UNIT).tolist())
    return units


FIXED_TILES = [
    # rows longer than a unit, rows shorter than one, 1-D, 4-D, single points, far edges
    ((5, 9, 1100), 1, 0, -1, 0, (0, 0, 0), (5, 9, 1100)),
    ((5, 9, 1100), 0, 3, -1, 1, (1, 2, 300), (2, 3, 250)),
    ((5, 9, 1100), 1, 0, 4, 0, (4, 8, 1099), (1, 1, 1)),
    ((5, 9, 1100), 1, 5, -1, 2, (0, 0, 200), (2, 3, 75)),
    ((65, 47, 130), 1, 0, -1, 0, (32, 23, 65), (1, 1, 1)),
    ((65, 47, 130), 0, 0, -1, 0, (0, 0, 0), (22, 16, 44)),
    ((65, 47, 130), 1, 2, -1, 1, (17, 12, 33), (16, 12, 32)),
    ((65, 47, 130), 0, 0, 0, 2, (12, 9, 24), (5, 3, 9)),
    ((65, 47, 130), 1, 0, 4, 1, (0, 0, 0), (33, 24, 65)),
    ((200000,), 1, 0, -1, 0, (100001,), (1,)),
    ((200000,), 0, 0, -1, 3, (24000,), (1000,)),
    ((200000,), 1, 0, 32, 2, (0,), (50000,)),
    ((9, 12, 17, 20), 1, 0, -1, 0, (8, 11, 16, 19), (1, 1, 1, 1)),
    ((9, 12, 17, 20), 0, 7, -1, 1, (1, 1, 2, 3), (3, 4, 5, 6)),
    ((9, 12, 17, 20), 1, 23, 4, 0, (2, 0, 11, 3), (7, 12, 6, 17)),
    ((33, 70), 1, 1, -1, 3, (1, 2), (4, 7)),
    ((33, 70), 0, 0, 0, 0, (32, 69), (1, 1)),
    ((300, 700), 1, 0, -1, 1, (100, 0), (50, 350)),
]


def _check_units(dims, interp, direction, anchor, k, lo, ext):
    a = DEF_ANCHOR[len(dims) - 1] if anchor < 0 else anchor
    c = R._cconf(dims, interp, direction, anchor)
    rc, tp = _tplan(c, k, lo, ext)
    assert rc == 0, L.sz3hip_last_error().decode()
    u = _units(c, k, lo, ext)
    assert tp.units_needed == u.size
    assert (np.diff(u.astype(np.int64)) > 0).all(), "strictly ascending"
    assert u.size == 0 or int(u[-1]) < tp.units_total
    all_anchor = k > 0 and a > 0 and any(d > a for d in dims) and (1 << k) >= a
    if all_anchor:
        assert u.size == 0
        return u, set()
    model = _model_units(dims, interp, direction, a, k, lo, ext, tp.region)
    assert np.array_equal(u, model), ("the list is not the definition's", dims, interp, direction, anchor, k, lo, ext)
    reads = _read_units(dims, interp, direction, a, k, lo, ext, tp.region)
    assert reads <= set(u.tolist()), ("a pass reads a code in a unit that is not listed", sorted(reads - set(u.tolist()))[:8])
    return u, reads


@pytest.mark.parametrize("case", FIXED_TILES, ids=["%s-k%d-%d" % ("x".join(map(str, t[0])), t[4], i) for i, t in enumerate(FIXED_TILES)])
def test_unit_list_fixed_cases(case):
    dims, interp, direction, anchor, k, lo, ext = case
    u, reads = _check_units(dims, interp, direction, anchor, k, lo, ext)
    assert u.size >= 1 and reads


def test_unit_list_random_cases():
    rng = np.random.default_rng(20261020)
    sparse = 0
    for case in range(400):
        dims, interp, direction, anchor, _, _ = R._random_case(rng)
        a = DEF_ANCHOR[len(dims) - 1] if anchor < 0 else anchor
        k = int(rng.integers(0, 4))
        lo, ext = _random_box(rng, _coarse(dims, k))
        try:
            u, reads = _check_units(dims, interp, direction, anchor, k, lo, ext)
        except AssertionError as e:
            raise AssertionError("case %d: dims %s interp %d direction %d anchor %d k %d lo %s ext %s: %s" % (case, dims, interp, direction, anchor, k, lo, ext, e))
        sparse += 2 * u.size <= -(-int(np.prod(dims)) // UNIT)
    assert sparse >= 20, "the cases must include boxes that need few of the units"


def test_the_closure_test_looks():
    """removing any one listed unit that holds a read makes the closure fail"""
    dims, interp, direction, anchor, k, lo, ext = (65, 47, 130), 1, 0, -1, 1, (17, 12, 33), (6, 5, 12)
    u, reads = _check_units(dims, interp, direction, anchor, k, lo, ext)
    assert len(reads) >= 4
    for r in sorted(reads):
        assert r in u
        assert not reads <= set(u.tolist()) - {r}


def test_capacity():
    c = R._cconf((65, 47, 130), 1, 0, -1)
    lo, ext = (3, 5, 7), (20, 20, 40)
    u = _units(c, 0, lo, ext)
    assert u.size > 4
    part = np.full(u.size, 0xFFFFFFFF, np.uint32)
    n = C.c_uint64(0)
    rc = L.sz3hip_tile_units_for(C.byref(c), 0, _box(lo), _box(ext), part.ctypes.data, 3, C.byref(n))
    assert rc == CODES["SZ3HIP_ECAPACITY"] and n.value == u.size
    assert np.array_equal(part[:3], u[:3]) and (part[3:] == 0xFFFFFFFF).all(), "nothing is written past cap"
    assert np.array_equal(sz3_amd.tile_units(sz3_amd.Config(65, 47, 130), 0, lo, ext), u)
    p = sz3_amd.tile_plan(sz3_amd.Config(65, 47, 130), 0, lo, ext)
    assert p["units_needed"] == u.size and p["units_total"] == -(-65 * 47 * 130 // UNIT) and p["region"] == sz3_amd.region_plan(sz3_amd.Config(65, 47, 130), lo, ext)

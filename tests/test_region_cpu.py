"""The region decode without a GPU: the symbols and Python names, the box's argument checks, a loud failure (never a fallback) where a device
would be needed, and the plan closure test — a brute-force model of the level / pass schedule and of the stencils' read offsets walks the
passes over the windows sz3hip_region_plan_for hands out and asserts that no read leaves a window and that every point of the box is
computed from valid inputs."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import sz3_amd

L = sz3_amd.lib()
L.sz3hip_last_error_code.restype = C.c_int


def _codes():  # the error enum of include/sz3hip.h
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sz3hip.h")) as f:
        txt = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SZ3HIP_E[A-Z]+) = (-?\d+)", txt)}


CODES = _codes()
DEF_ANCHOR = (4096, 128, 32, 16)


def test_symbols_and_names_exist():
    for sym in ("sz3hip_region_plan_for", "sz3hip_decompress_region_to_device", "sz3hip_decompress_device_region", "sz3hip_debug_region_scratch",
                "sz3hip_debug_region_fast_calls"):
        assert hasattr(L, sym), sym
    assert callable(sz3_amd.region_plan) and callable(sz3_amd.decompress_region)
    assert callable(sz3_amd.DeviceCompressor.decompress_region)


def _cconf(dims, interp=1, direction=0, anchor=-1):
    c = sz3_amd._CConfig()  # (the raw struct: extents of 1 stay)
    c.N = len(dims)
    for i, d in enumerate(dims):
        c.dims[i] = d
    c.interpAlgo = interp
    c.interpDirection = direction
    c.interpAnchorStride = anchor
    return c


def _plan(c, lo, ext):
    plan = sz3_amd._CRegionPlan()
    rc = L.sz3hip_region_plan_for(C.byref(c), (C.c_uint64 * 4)(*lo), (C.c_uint64 * 4)(*ext), C.byref(plan))
    return rc, plan


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_box_checks_name_the_extent():
    c = _cconf((20, 30, 40))
    rc, _ = _plan(c, (0, 0, 0), (20, 0, 40))
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 1" in L.sz3hip_last_error().decode()
    rc, _ = _plan(c, (0, 0, 38), (1, 1, 3))
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 2" in L.sz3hip_last_error().decode()
    rc, _ = _plan(c, (20, 0, 0), (1, 1, 1))
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 0" in L.sz3hip_last_error().decode()
    rc, _ = _plan(c, (2 ** 64 - 1, 0, 0), (2, 1, 1))  # (lo + ext wraps)
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 0" in L.sz3hip_last_error().decode()
    rc, _ = _plan(c, (19, 29, 39), (1, 1, 1))
    assert rc == 0


def test_null_arguments():
    c = _cconf((20, 30))
    plan = sz3_amd._CRegionPlan()
    box = (C.c_uint64 * 4)(1, 1, 0, 0)
    for args in ((None, box, box, C.byref(plan)), (C.byref(c), None, box, C.byref(plan)), (C.byref(c), box, None, C.byref(plan)), (C.byref(c), box, box, None)):
        assert L.sz3hip_region_plan_for(*args) == CODES["SZ3HIP_EINVAL"]
        assert "NULL" in L.sz3hip_last_error().decode()


def test_anchor_stride_no_power_of_two_is_unsupported():
    rc, _ = _plan(_cconf((50, 60, 70), anchor=12), (1, 1, 1), (4, 4, 4))
    assert rc == CODES["SZ3HIP_EUNSUPPORTED"] and "power of two" in L.sz3hip_last_error().decode()


def test_python_region_plan():
    conf = sz3_amd.Config(65, 47, 130)
    p = sz3_amd.region_plan(conf, (3, 5, 7), (4, 4, 4))
    assert p["n_levels"] == 5 and p["strides"] == (16, 8, 4, 2, 1) and len(p["windows"]) == 5
    assert p["windows"][-1] == ((0, 2, 4), (9, 11, 13))  # the box grown by 3 below and above
    assert p["points"] > 0 and p["scratch_elems"] > 0
    with pytest.raises(sz3_amd.SZ3HipError):
        sz3_amd.region_plan(conf, (3, 5, 7), (4, 4, 200))
    with pytest.raises(ValueError):
        sz3_amd.region_plan(conf, (3, 5), (4, 4))


def _lossless_container(shape=(6, 10)):
    """a container this machine can write without a device: ALGO_LOSSLESS is zstd alone"""
    a = np.arange(np.prod(shape), dtype=np.float32).reshape(shape)
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = sz3_amd.ALGO_LOSSLESS
    blob, _ = sz3_amd.compress(a, c)
    return np.ascontiguousarray(blob)


def _region_call(blob, dt, lo, ext, ptr, strides=None):
    c = sz3_amd.Config(1)
    rc = L.sz3hip_decompress_region_to_device(C.byref(c._c), dt, blob.ctypes.data, blob.size, (C.c_uint64 * 4)(*lo), (C.c_uint64 * 4)(*ext), ptr, strides, None)
    return rc, c


def test_to_device_call_checks_the_box_before_anything_else():
    blob = _lossless_container()
    rc, c = _region_call(blob, 0, (0, 0), (6, 11), 0x1000)
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 1" in L.sz3hip_last_error().decode()
    assert tuple(c.dims) == (6, 10), "conf stays the full array's"
    rc, _ = _region_call(blob, 0, (0, 0), (0, 5), 0x1000)
    assert rc == CODES["SZ3HIP_EINVAL"] and "dimension 0" in L.sz3hip_last_error().decode()
    c = sz3_amd.Config(1)
    rc = L.sz3hip_decompress_region_to_device(C.byref(c._c), 0, blob.ctypes.data, blob.size, None, None, 0x1000, None, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and "NULL" in L.sz3hip_last_error().decode()


def test_integer_types_are_unsupported():
    blob = _lossless_container()
    rc, _ = _region_call(blob, 7, (0, 0), (2, 2), 0x1000)
    assert rc == CODES["SZ3HIP_EUNSUPPORTED"] and "integer" in L.sz3hip_last_error().decode()


def test_truncated_container():
    blob = _lossless_container()
    part = np.ascontiguousarray(blob[:blob.size - 5])
    rc, _ = _region_call(part, 0, (0, 0), (2, 2), 0x1000)
    assert rc == CODES["SZ3HIP_EFORMAT"]


def test_overlapping_output_strides_refused():
    blob = _lossless_container()
    rc, _ = _region_call(blob, 0, (1, 1), (3, 5), 0x1000, (C.c_int64 * 2)(1, 1))
    assert rc == CODES["SZ3HIP_EINVAL"] and "overlap" in L.sz3hip_last_error().decode()


def test_without_a_device_the_calls_fail_loudly():
    """a host pointer (or no device at all) is an error; nothing falls back to a host path"""
    blob = _lossless_container()
    out = np.zeros(15, np.float32)
    rc, _ = _region_call(blob, 0, (1, 2), (3, 5), out.ctypes.data)
    assert rc == CODES["SZ3HIP_EINVAL"] and "device memory" in L.sz3hip_last_error().decode()
    assert not out.any()
    with pytest.raises(ValueError):
        sz3_amd.decompress_region(blob, np.float32, (1, 2), (3, 5))  # (neither device= nor out=)
    with pytest.raises(ValueError):
        sz3_amd.decompress_region(blob, np.float32, (1, 2), (3, 5), out=out)  # (a host array)


def test_device_context_call_fails_loudly_without_a_context():
    box = (C.c_uint64 * 4)(1, 1, 1, 1)
    rc = L.sz3hip_decompress_device_region(None, 0x1000, 4096, box, box, 0x2000, None)
    assert rc == CODES["SZ3HIP_EINVAL"] and L.sz3hip_last_error().decode()
    assert L.sz3hip_debug_region_scratch(None) == 0


# ---- the model: InterpolationDecomposition's schedule and the stencils' read offsets -----------------------------------------------------
def _levels(dims, anchor_stride):
    """(number of levels that run, anchor stride in effect) — init(), InterpolationDecomposition.hpp:176-213"""
    lv = max(math.ceil(math.log2(d)) for d in dims)
    anchor = anchor_stride if any(d > anchor_stride for d in dims) else 0
    if anchor > 0:
        lv = min(lv, int(math.log2(anchor)) + 1) - 1
    return lv, anchor


def _reads(i, n, old_api, interp):
    """(offsets along the pass axis in units of the level's stride, deferred) of point i of a line of n points"""
    if old_api:
        if interp == 0 or n < 5:
            if i + 1 < n:
                return (-1, 1), False
            return ((-1,) if n < 4 else (-3, -1)), False
        if i == 1:
            return (-1, 1, 3), False
        if i + 3 < n:
            return (-3, -1, 1, 3), False
        if i + 1 < n:
            return (-3, -1, 1), False
        return (-5, -3, -1), False
    if interp == 0:
        if i + 1 < n:
            return (-1, 1), False
        if n < 3:
            return (-1,), False
        return (-2, -1), True
    if i >= 3:
        if i + 3 < n:
            return (-3, -1, 1, 3), False
        if i + 1 < n:
            return (-3, -1, 1), False
        return (-3, -1), False
    if i + 3 < n:
        return (-1, 1, 3), False
    if i + 1 < n:
        return (-1, 1), False
    return (-1,), False


def _lattice(start, step, wl, wh):
    q0 = 0 if wl <= start else -(-(wl - start) // step)
    first = start + q0 * step
    return np.arange(first, wh + 1, step, dtype=np.int64) if first <= wh else np.zeros(0, np.int64)


def _walk(dims, interp, direction, anchor_stride, lo, ext, plan):
    """walks the passes over the plan's windows; returns (points predicted, sum of the level buffers the windows imply)"""
    N = len(dims)
    nl, anchor = _levels(dims, anchor_stride)
    assert plan.n_levels == nl
    perm = list(itertools.permutations(range(N)))[direction]
    pos = {perm[k]: k for k in range(N)}
    old_api = N <= 2
    box = [(lo[j], lo[j] + ext[j] - 1) for j in range(N)]
    valid = np.zeros(dims, bool)  # the points a buffer holds with their final value
    if anchor:
        valid[tuple(slice(0, None, anchor) for _ in range(N))] = True  # the anchor grid: raw records
    else:
        valid[(0,) * N] = True  # the first point
    points = 0
    buffers = 0
    for b in range(nl):
        s = 1 << (nl - 1 - b)
        assert plan.stride[b] == s
        win = [(int(plan.win_lo[b][j]), int(plan.win_hi[b][j])) for j in range(N)]
        out = [(int(plan.win_lo[b + 1][j]), int(plan.win_hi[b + 1][j])) for j in range(N)] if b + 1 < nl else box
        for j in range(N):
            assert 0 <= win[j][0] <= out[j][0] <= out[j][1] <= win[j][1] < dims[j], (b, j, win, out)
        buf = 1
        for j in range(N):
            buf *= (win[j][1] - win[j][0] // (2 * s) * (2 * s)) // s + 1
        buffers += buf
        # the buffer of this level holds what lies in its window and nothing else
        inside = np.zeros(dims, bool)
        inside[tuple(slice(win[j][0], win[j][1] + 1) for j in range(N))] = True
        valid &= inside
        for k in range(N):
            d = perm[k]
            D = dims[d]
            defers = interp == 0 and N >= 3
            cl = []
            for j in range(N):
                start = s if j == d else 0
                step = 2 * s if (j == d or pos[j] > k) else s
                wl, wh = win[j] if pos[j] > k else out[j]
                if j == d and defers:
                    wl = max(0, wl - 2 * s)
                cl.append(_lattice(start, step, wl, wh))
            cnt = 1
            for j in range(N):
                cnt *= len(cl[j])
            points += cnt
            if cnt == 0:
                continue
            late = []
            for cd in cl[d]:
                cd = int(cd)
                begin = cd // (32 * s) * (32 * s)
                end = min(begin + 32 * s, D - 1)
                n, i = (end - begin) // s + 1, (cd - begin) // s
                assert i % 2 == 1 and 1 <= i <= n - 1
                offs, deferred = _reads(i, n, old_api, interp)
                if deferred:
                    late.append((cd, offs))
                    continue
                for o in offs:
                    rc = cd + o * s
                    assert win[d][0] <= rc <= win[d][1] and 0 <= rc < D, ("read leaves the window", b, k, cd, o, win[d])
                    assert valid[np.ix_(*[cl[j] if j != d else [rc] for j in range(N)])].all(), ("read of a point nobody computed", b, k, cd, o)
                valid[np.ix_(*[cl[j] if j != d else [cd] for j in range(N)])] = True
            for cd, offs in late:  # the pass's second launch
                for o in offs:
                    rc = cd + o * s
                    assert win[d][0] <= rc <= win[d][1] and 0 <= rc < D, ("read leaves the window", b, k, cd, o, win[d])
                    assert valid[np.ix_(*[cl[j] if j != d else [rc] for j in range(N)])].all(), ("read of a point nobody computed", b, k, cd, o)
                valid[np.ix_(*[cl[j] if j != d else [cd] for j in range(N)])] = True
    assert valid[tuple(slice(box[j][0], box[j][1] + 1) for j in range(N))].all(), "a point of the box was not computed"
    return points, buffers


def _random_case(rng):
    N = int(rng.integers(1, 5))
    top = (700, 150, 70, 22)[N - 1]
    dims = []
    for _ in range(N):
        r = rng.random()
        if r < 0.08:
            dims.append(1)
        elif r < 0.35:
            e = int(rng.integers(1, int(math.log2(top)) + 1))
            dims.append(min(top, max(1, 2 ** e + int(rng.integers(-1, 2)))))
        else:
            dims.append(int(rng.integers(2, top + 1)))
    interp = int(rng.integers(0, 2))
    direction = int(rng.integers(0, math.factorial(N)))
    anchor = int(rng.choice([-1, 0, 4, 8, 16, 32]))
    lo, ext = [], []
    for D in dims:
        kind = rng.random()
        if kind < 0.2:  # a single point
            a = int(rng.integers(0, D))
            e = 1
        elif kind < 0.35:  # at the origin
            a = 0
            e = int(rng.integers(1, D + 1))
        elif kind < 0.5:  # ending at the far edge
            e = int(rng.integers(1, D + 1))
            a = D - e
        else:
            a = int(rng.integers(0, D))
            e = int(rng.integers(1, D - a + 1))
        lo.append(a)
        ext.append(e)
    return dims, interp, direction, anchor, lo, ext


def test_plan_closure():
    rng = np.random.default_rng(20261018)
    seen = {"N": set(), "interp": set(), "anchor": set(), "first_point": False, "single": False, "no_level": False}
    for case in range(2400):
        dims, interp, direction, anchor, lo, ext = _random_case(rng)
        rc, plan = _plan(_cconf(dims, interp, direction, anchor), lo, ext)
        assert rc == 0, (dims, lo, ext, L.sz3hip_last_error().decode())
        a = DEF_ANCHOR[len(dims) - 1] if anchor < 0 else anchor
        try:
            points, buffers = _walk(dims, interp, direction, a, lo, ext, plan)
        except AssertionError as e:
            raise AssertionError("case %d: dims %s interp %d direction %d anchor %d lo %s ext %s: %s" % (case, dims, interp, direction, anchor, lo, ext, e))
        assert plan.points == points, (dims, interp, direction, anchor, lo, ext)
        assert plan.scratch_elems >= max(buffers, 1), (dims, lo, ext)
        seen["N"].add(len(dims))
        seen["interp"].add(interp)
        seen["anchor"].add(anchor)
        seen["first_point"] |= _levels(dims, a)[1] == 0
        seen["single"] |= all(e == 1 for e in ext)
        seen["no_level"] |= plan.n_levels == 0
    assert seen["N"] == {1, 2, 3, 4} and seen["interp"] == {0, 1} and seen["anchor"] == {-1, 0, 4, 8, 16, 32}
    assert seen["first_point"] and seen["single"]


def _schedule_points(dims, anchor_stride):
    """the full schedule's predicted points: build_schedule's cnt per pass, summed"""
    N = len(dims)
    nl, _ = _levels(dims, anchor_stride)
    total = 0
    for level in range(nl, 0, -1):
        s = 1 << (level - 1)
        for k in range(N):  # (the count of a pass does not depend on the order: pass k has k axes at every multiple of s)
            c = 1
            for j in range(N):
                g = (dims[j] - 1) // s + 1
                c *= g // 2 if j == k else (g if j < k else (dims[j] - 1) // (2 * s) + 1)
            total += c
    return total


@pytest.mark.parametrize("dims", [(300,), (129, 200), (65, 47, 130), (9, 12, 17, 20), (64, 64, 64), (33, 1, 40)])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("anchor", [-1, 0, 4])
def test_whole_array_box(dims, interp, anchor):
    N = len(dims)
    rc, plan = _plan(_cconf(dims, interp, 0, anchor), (0,) * N, dims)
    assert rc == 0
    a = DEF_ANCHOR[N - 1] if anchor < 0 else anchor
    assert plan.n_levels == _levels(dims, a)[0]
    for b in range(plan.n_levels):
        assert [int(plan.win_lo[b][j]) for j in range(N)] == [0] * N
        assert [int(plan.win_hi[b][j]) for j in range(N)] == [d - 1 for d in dims]
    assert plan.points == _schedule_points(dims, a)
    _walk(dims, interp, 0, a, (0,) * N, dims, plan)

"""Several tiles of one stream in one call, without a GPU: the symbols and Python names, the plan of a request against
the single-box plans and unit lists (test_tile_cpu.py's helpers, themselves checked there against the Python models), and the refusals —
which must name the box they refuse and come before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import sz3_amd
import test_region_cpu as R
import test_tile_cpu as T

L = sz3_amd.lib()
CODES = R.CODES
MAX_BOXES = 256


def _carr(boxes):
    arr = (sz3_amd._CBox * max(len(boxes), 1))()
    for i, (lo, ext) in enumerate(boxes):
        arr[i].lo[:len(lo)] = [int(v) for v in lo]
        arr[i].ext[:len(ext)] = [int(v) for v in ext]
    return arr


def _mplan(c, level, boxes, n=None):
    plan = sz3_amd._CTilesPlan()
    rc = L.sz3hip_tiles_plan_for(C.byref(c), level, _carr(boxes), len(boxes) if n is None else n, C.byref(plan))
    return rc, plan


def test_symbols_and_names_exist():
    for sym in ("sz3hip_tiles_plan_for", "sz3hip_decompress_device_tiles", "sz3hip_decompress_tiles_to_device", "sz3hip_debug_region_launches"):
        assert hasattr(L, sym), sym
    for name in ("tiles_plan", "decompress_tiles"):
        assert callable(getattr(sz3_amd, name)), name
    assert callable(sz3_amd.DeviceCompressor.decompress_tiles)
    assert C.sizeof(sz3_amd._CBox) == 64 and C.sizeof(sz3_amd._CTilesPlan) == 40
    assert isinstance(L.sz3hip_debug_region_launches(), int)


# ---- the plan of a request ----------------------------------------------------------------------------------------------------------------
def _random_request(rng):
    """one grid, one level, 1 .. 9 boxes of it: random ones, duplicates of earlier ones and boxes that overlap an earlier one"""
    dims, interp, direction, anchor, a, k, lo, ext = T._random_tile(rng)
    k = min(k, 3)
    cd = T._coarse(dims, k)
    boxes = [T._random_box(rng, cd)]
    for _ in range(int(rng.integers(0, 9))):
        kind = rng.random()
        if kind < 0.2:
            boxes.append(boxes[int(rng.integers(0, len(boxes)))])  # a duplicate
        elif kind < 0.45:  # one that shares its low corner with an earlier box: the two overlap
            lo0, ext0 = boxes[int(rng.integers(0, len(boxes)))]
            boxes.append((list(lo0), [int(rng.integers(1, D - l + 1)) for l, D in zip(lo0, cd)]))
        else:
            boxes.append(T._random_box(rng, cd))
    return dims, interp, direction, anchor, k, boxes


def test_plan_of_random_requests():
    rng = np.random.default_rng(20261019)
    seen_n, seen_k, seen_boxes, saw_shared = set(), set(), set(), False
    for _ in range(150):
        dims, interp, direction, anchor, k, boxes = _random_request(rng)
        c = R._cconf(dims, interp, direction, anchor)
        rc, mp = _mplan(c, k, boxes)
        assert rc == 0, L.sz3hip_last_error().decode()
        singles = []
        union = set()
        for lo, ext in boxes:
            rc, tp = T._tplan(c, k, lo, ext)
            assert rc == 0
            singles.append(tp)
            union.update(int(u) for u in T._units(c, k, lo, ext))
        assert mp.n_boxes == len(boxes) and mp.n_levels == singles[0].region.n_levels
        assert all(tp.region.n_levels == mp.n_levels for tp in singles), "one level of one grid: every box has the grid's level count"
        assert mp.points == sum(tp.region.points for tp in singles)
        # the implementation places box i's buffers at the sum of the scratch of the boxes before it: the last base plus the last box's own
        # scratch is the sum, which the plan must cover
        assert mp.scratch_elems >= sum(tp.region.scratch_elems for tp in singles)
        assert mp.units_total == singles[0].units_total == -(-int(np.prod(dims)) // T.UNIT)
        assert mp.units_needed == len(union)
        saw_shared = saw_shared or len(union) < sum(tp.units_needed for tp in singles)
        seen_n.add(len(dims))
        seen_k.add(k)
        seen_boxes.add(len(boxes))
    assert seen_n == {1, 2, 3, 4} and {0, 1, 2, 3} <= seen_k and {1, 9} <= seen_boxes
    assert saw_shared, "some request's boxes must share units, or the union is not what is checked"


def test_one_box_is_the_tile_plan():
    rng = np.random.default_rng(5)
    for _ in range(100):
        dims, interp, direction, anchor, a, k, lo, ext = T._random_tile(rng)
        c = R._cconf(dims, interp, direction, anchor)
        rc, mp = _mplan(c, k, [(lo, ext)])
        assert rc == 0, L.sz3hip_last_error().decode()
        rc, tp = T._tplan(c, k, lo, ext)
        assert rc == 0
        assert (mp.n_boxes, mp.n_levels, mp.points, mp.scratch_elems, mp.units_total, mp.units_needed) == \
            (1, tp.region.n_levels, tp.region.points, tp.region.scratch_elems, tp.units_total, tp.units_needed)


def test_python_tiles_plan():
    conf = sz3_amd.Config(65, 47, 130)
    boxes = [((3, 5, 7), (4, 4, 4)), ((0, 0, 0), (9, 9, 9)), ((3, 5, 7), (4, 4, 4))]
    p = sz3_amd.tiles_plan(conf, 1, boxes)
    singles = [sz3_amd.tile_plan(conf, 1, lo, ext) for lo, ext in boxes]
    assert p["n_boxes"] == 3 and p["points"] == sum(s["region"]["points"] for s in singles)
    assert p["scratch_elems"] == sum(s["region"]["scratch_elems"] for s in singles)
    assert p["units_needed"] == np.union1d(sz3_amd.tile_units(conf, 1, *boxes[0]), sz3_amd.tile_units(conf, 1, *boxes[1])).size
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.tiles_plan(conf, 1, boxes + [((0, 0, 60), (1, 1, 10))])
    assert e.value.code == CODES["SZ3HIP_EINVAL"] and "box 3" in str(e.value)
    with pytest.raises(ValueError):
        sz3_amd.tiles_plan(conf, 1, [((3, 5), (4, 4))])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_plan_refusals():
    c = R._cconf((20, 30, 40))  # level 2: the grid is 5 x 8 x 10
    good = ((1, 1, 1), (2, 2, 2))
    assert _mplan(c, 2, [good] * 4)[0] == 0
    rc, _ = _mplan(c, 2, [])
    assert rc == CODES["SZ3HIP_EINVAL"] and "boxes" in L.sz3hip_last_error().decode()
    assert _mplan(c, 2, [good] * MAX_BOXES)[0] == 0
    rc, _ = _mplan(c, 2, [good] * (MAX_BOXES + 1))
    assert rc == CODES["SZ3HIP_EINVAL"] and "257" in L.sz3hip_last_error().decode()
    plan = sz3_amd._CTilesPlan()
    arr = _carr([good])
    for args in ((None, 2, arr, 1, C.byref(plan)), (C.byref(c), 2, None, 1, C.byref(plan)), (C.byref(c), 2, arr, 1, None)):
        assert L.sz3hip_tiles_plan_for(*args) == CODES["SZ3HIP_EINVAL"] and "NULL" in L.sz3hip_last_error().decode()
    for level in (-1, 31, 1000):
        rc, _ = _mplan(c, level, [good])
        assert rc == CODES["SZ3HIP_EINVAL"] and "level" in L.sz3hip_last_error().decode()
    # a bad box at the first, a middle and the last index: the single-box call's wording, with the index
    bads = [(((0, 0, 0), (5, 8, 11)), "dimension 2"), (((5, 0, 0), (1, 1, 1)), "dimension 0"), (((0, 0, 0), (5, 0, 10)), "dimension 1"),
            (((0, 2 ** 64 - 1, 0), (1, 2, 1)), "dimension 1")]
    for bad, what in bads:
        rc, _ = T._tplan(c, 2, *bad)
        single = L.sz3hip_last_error().decode()
        assert rc == CODES["SZ3HIP_EINVAL"] and what in single
        for at in (0, 3, 6):
            boxes = [good] * 7
            boxes[at] = bad
            rc, _ = _mplan(c, 2, boxes)
            msg = L.sz3hip_last_error().decode()
            assert rc == CODES["SZ3HIP_EINVAL"] and msg == "box %d: %s" % (at, single), msg
    # the FIRST bad box is the one refused
    boxes = [good, bads[1][0], good, bads[0][0]]
    rc, _ = _mplan(c, 2, boxes)
    assert rc == CODES["SZ3HIP_EINVAL"] and "box 1:" in L.sz3hip_last_error().decode() and "dimension 0" in L.sz3hip_last_error().decode()


def test_anchor_stride_no_power_of_two_is_unsupported():
    c = R._cconf((50, 60, 70), anchor=12)
    rc, _ = _mplan(c, 1, [((1, 1, 1), (4, 4, 4)), ((2, 2, 2), (4, 4, 4))])
    assert rc == CODES["SZ3HIP_EUNSUPPORTED"] and "power of two" in L.sz3hip_last_error().decode()


def _tiles_call(blob, dt, level, boxes, ptrs, n=None):
    c = sz3_amd.Config(1)
    arr = _carr(boxes) if boxes is not None else None
    outs = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
    n = (len(boxes) if boxes is not None else 1) if n is None else n
    rc = L.sz3hip_decompress_tiles_to_device(C.byref(c._c), dt, blob.ctypes.data, blob.size, level, arr, n, outs, None)
    return rc, c


def test_to_device_call_checks_before_anything_else():
    """test_tile_cpu.py's pattern: every refusal comes before the library looks for a device, so this machine sees them all"""
    blob = R._lossless_container()  # 6 x 10; level 1: 3 x 5
    good = ((0, 0), (3, 5))
    far = [0x100000 * (i + 1) for i in range(4)]
    rc, c = _tiles_call(blob, 0, 1, [good, good, ((0, 0), (3, 6)), good], far)
    assert rc == CODES["SZ3HIP_EINVAL"] and "box 2" in L.sz3hip_last_error().decode() and "dimension 1" in L.sz3hip_last_error().decode()
    assert tuple(c.dims) == (6, 10), "conf stays the full array's"
    rc, _ = _tiles_call(blob, 0, 1, [((0, 0), (0, 5)), good], far[:2])
    assert rc == CODES["SZ3HIP_EINVAL"] and "box 0" in L.sz3hip_last_error().decode() and "dimension 0" in L.sz3hip_last_error().decode()
    rc, _ = _tiles_call(blob, 0, 1, [good, ((3, 0), (1, 1))], far[:2])
    assert rc == CODES["SZ3HIP_EINVAL"] and "box 1" in L.sz3hip_last_error().decode() and "dimension 0" in L.sz3hip_last_error().decode()
    rc, _ = _tiles_call(blob, 0, 31, [good], far[:1])
    assert rc == CODES["SZ3HIP_EINVAL"] and "level" in L.sz3hip_last_error().decode()
    rc, _ = _tiles_call(blob, 0, 1, None, far[:1])
    assert rc == CODES["SZ3HIP_EINVAL"] and "NULL" in L.sz3hip_last_error().decode()
    rc, _ = _tiles_call(blob, 0, 1, [good], None)
    assert rc == CODES["SZ3HIP_EINVAL"] and "NULL" in L.sz3hip_last_error().decode()
    rc, _ = _tiles_call(blob, 0, 1, [good], far[:1], n=0)
    assert rc == CODES["SZ3HIP_EINVAL"]
    rc, _ = _tiles_call(blob, 0, 1, [good] * (MAX_BOXES + 1), [0x100000 * (i + 1) for i in range(MAX_BOXES + 1)])
    assert rc == CODES["SZ3HIP_EINVAL"] and "257" in L.sz3hip_last_error().decode()
    rc, _ = _tiles_call(blob, 7, 1, [good], far[:1])
    assert rc == CODES["SZ3HIP_EUNSUPPORTED"] and "integer" in L.sz3hip_last_error().decode()
    # outputs that overlap one another: box 0's 15 floats reach 60 bytes past its pointer
    rc, _ = _tiles_call(blob, 0, 1, [good, good], [0x100000, 0x100000 + 56])
    assert rc == CODES["SZ3HIP_EINVAL"] and "overlap" in L.sz3hip_last_error().decode()
    rc, _ = _tiles_call(blob, 0, 1, [good, good], [0x100000, 0x100000])
    assert rc == CODES["SZ3HIP_EINVAL"] and "overlap" in L.sz3hip_last_error().decode()
    rc, _ = _tiles_call(blob, 0, 1, [good, good], [0x100000, 0])
    assert rc == CODES["SZ3HIP_EINVAL"] and "box 1" in L.sz3hip_last_error().decode() and "NULL" in L.sz3hip_last_error().decode()
    # a host pointer among the outputs: an error, never a host path (the arrays end to end, not overlapping)
    out = np.zeros(30, np.float32)
    rc, _ = _tiles_call(blob, 0, 1, [good, good], [out.ctypes.data, out.ctypes.data + 60])
    assert rc == CODES["SZ3HIP_EINVAL"] and "device memory" in L.sz3hip_last_error().decode() and not out.any()
    with pytest.raises(ValueError):
        sz3_amd.decompress_tiles(blob, np.float32, 1, [good])  # (neither device= nor out=)


def test_device_context_call_fails_loudly_without_a_context():
    arr = _carr([((0, 0), (1, 1))])
    outs = (C.c_void_p * 1)(0x2000)
    assert L.sz3hip_decompress_device_tiles(None, 0x1000, 4096, 1, arr, 1, outs, None) == CODES["SZ3HIP_EINVAL"]
    assert "context" in L.sz3hip_last_error().decode()

"""tests/view_model.py held to numpy itself and to Python integers (no device): the views, the narrowing, and dev_view's overlap answer
against a brute-force set of touched offsets."""
import itertools
import math

import numpy as np
import pytest

import view_model as M
from view_model import View


def base_of(n, dtype="int32"):
    return np.arange(1, n + 1).astype(dtype)


def same(view, base, want):
    got = M.view_of(base, view)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert view.numel == want.size and (want.size == 0 or base[view.last] == want.reshape(-1)[-1])


# ---- host_view against plain numpy, for every kind of view the sweep draws ---------------------------------------------------------
def test_whole_and_offset():
    b = base_of(5 * 6 * 7 + 3)
    same(View.whole("int32", (5, 6, 7)), b, b[:210].reshape(5, 6, 7))
    same(View.whole("int32", (5, 6, 7), offset=3), b, b[3:].reshape(5, 6, 7))
    same(View.whole("int32", (210,), offset=1), b, b[1:211])


@pytest.mark.parametrize("slices", [
    (slice(1, 4), slice(0, 6), slice(2, 7)), (slice(None, None, 2),) * 3, (slice(None, None, 3),) * 3,
    (slice(1, 5, 2), slice(2, 3), slice(0, 7, 3)), (slice(4, 5), slice(5, 6), slice(6, 7))])
def test_sub_ranges_and_steps(slices):
    b = base_of(5 * 6 * 7 + 2)
    same(View.whole("int32", (5, 6, 7), offset=2).sliced(*slices), b, b[2:].reshape(5, 6, 7)[slices])


@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))))
def test_permutations(perm):
    b = base_of(4 * 5 * 6)
    v = View.whole("int32", (4, 5, 6)).sliced(slice(1, 4), slice(None, None, 2), slice(0, 5)).permuted(perm)
    same(v, b, b.reshape(4, 5, 6)[1:4, ::2, 0:5].transpose(perm))


def test_rank_4_permuted_and_stepped():
    b = base_of(3 * 4 * 5 * 6)
    v = View.whole("int32", (3, 4, 5, 6)).sliced(slice(0, 3), slice(1, 4), slice(None, None, 2), slice(None, None, 3)).permuted((2, 0, 3, 1))
    same(v, b, b.reshape(3, 4, 5, 6)[:, 1:4, ::2, ::3].transpose(2, 0, 3, 1))


def test_interleaved_field():
    b = base_of(4 * 5 * 3)
    for k in range(3):
        same(View.whole("int32", (4, 5, 3)).field(k), b, b.reshape(4, 5, 3)[..., k])
    same(View.whole("int32", (4, 5, 3)).field(1).sliced(slice(1, 3), slice(None, None, 2)), b, b.reshape(4, 5, 3)[1:3, ::2, 1])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_stride_zero(axis):
    shape = [4, 5, 6]
    shape[axis] = 1
    b = base_of(int(np.prod(shape)) + 1)
    v = View.whole("int32", shape, offset=1).expanded(axis, 3)
    want_shape = list(shape)
    want_shape[axis] = 3
    same(v, b, np.broadcast_to(b[1:].reshape(shape), want_shape))
    assert v.strides[axis] == 0


def test_dropped_extents_of_one():
    v = View.whole("int32", (3, 1, 4, 1))
    assert v.dropped().shape == (3, 4) and v.dropped().strides == (4, 1)
    assert View.whole("int32", (1, 1)).dropped().shape == (1,)


def test_expected_after_scatter():
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, 6 * 7 * 2, dtype=np.uint8)
    v = View.whole("int16", (6, 7)).sliced(slice(1, 6, 2), slice(0, 7, 3)).permuted((1, 0))
    vals = np.arange(-4, 5, dtype=np.int16)
    out = M.expected_after_scatter(raw, v, vals)
    want = raw.copy().view(np.int16).reshape(6, 7)
    want[1:6:2, 0:7:3] = vals.reshape(3, 3).T
    assert np.array_equal(out, want.reshape(-1).view(np.uint8))
    assert not np.shares_memory(out, raw) and int((out != raw).sum()) <= 2 * 9


# ---- narrow against Python integers ---------------------------------------------------------------------------------------------------
def py_narrow(x, dtype):
    info = np.iinfo(dtype)
    if math.isnan(x):
        return int(info.min)
    if math.isinf(x):
        return int(info.min) if x < 0 else int(M.clamp_ends(dtype)[1])
    fl = math.floor(x)
    d = x - fl  # (exact: the inputs below are halves and integers)
    r = fl if d < 0.5 else fl + 1 if d > 0.5 else fl + (fl & 1)
    return max(int(info.min), min(r, int(M.clamp_ends(dtype)[1])))


@pytest.mark.parametrize("dtype", M.INT_TYPES)
def test_narrow(dtype):
    v = M.narrowing_probe(dtype)
    got = M.narrow(v, dtype)
    assert got.dtype == np.dtype(dtype)
    for x, g in zip(v, got):
        assert int(g) == py_narrow(float(x), dtype), (dtype, float(x), int(g))


def test_clamp_ends_of_the_64_bit_types():
    assert M.clamp_ends("int64") == (-9223372036854775808.0, 9223372036854774784.0)
    assert M.clamp_ends("uint64") == (0.0, 18446744073709549568.0)
    assert M.clamp_ends("uint8") == (0.0, 255.0) and M.clamp_ends("int16") == (-32768.0, 32767.0)
    assert int(M.narrow(np.array([2.0 ** 64]), "uint64")[0]) == 18446744073709549568
    assert int(M.narrow(np.array([2.0 ** 63]), "int64")[0]) == 9223372036854774784


def test_widen_and_the_flag():
    for dt in M.INT_TYPES:
        info = np.iinfo(dt)
        a = np.array([info.min, info.max, 0, 1], dtype=dt)
        assert M.widen(a).dtype == np.float64 and [float(int(x)) for x in a] == list(M.widen(a))
    for dt in ("int64", "uint64"):
        assert not M.beyond_2_53(np.array([1 << 53, 0], dtype=dt)) and M.beyond_2_53(np.array([0, (1 << 53) + 1], dtype=dt))
    assert not M.beyond_2_53(np.array([-(1 << 53)], dtype="int64")) and M.beyond_2_53(np.array([-(1 << 53) - 1], dtype="int64"))
    assert not M.beyond_2_53(np.array([2 ** 31 - 1], dtype="int32"))


# ---- dev_view_rule ------------------------------------------------------------------------------------------------------------------
def test_dev_view_rule_named_cases():
    R = M.dev_view_rule
    assert R((4, 5, 6), None, True) == R((4, 5, 6), (30, 6, 1), True) == M.CONTIGUOUS
    assert R((4, 1, 6), (6, 999, 1), True) == M.CONTIGUOUS  # (an extent of one: its stride does not count)
    assert R((4, 5, 6), (60, 12, 2), True) == R((6, 4, 5), (1, 30, 6), True) == M.STRIDED
    assert R((4, 5), (-5, 1), False) == R((4, 5), (5, -1), True) == R((1, 5), (-1, 1), False) == M.NEGATIVE
    assert R((3, 5, 6), (0, 6, 1), False) == M.STRIDED and R((3, 5, 6), (0, 6, 1), True) == M.OVERLAP
    assert R((5, 4), (2, 1), True) == M.OVERLAP and R((5, 4), (2, 1), False) == M.STRIDED  # windows of 4 every 2
    assert R((2, 3), (3, 2), True) == M.OVERLAP  # (no two elements coincide, yet the sufficient test refuses: allowed)
    assert len(set(M.touched_offsets((2, 3), (3, 2)))) == 6


def test_overlap_answer_against_brute_force():
    rng = np.random.default_rng(5)
    accepted = refused_free = refused = 0
    for _ in range(400):
        n = int(rng.integers(1, 5))
        dims = [int(rng.integers(1, 5)) for _ in range(n)]
        strides = [int(rng.integers(0, 13)) for _ in range(n)]
        ans = M.dev_view_rule(dims, strides, True)
        offs = M.touched_offsets(dims, strides)
        distinct = len(set(offs)) == len(offs)
        if ans in (M.CONTIGUOUS, M.STRIDED):
            accepted += 1
            assert distinct, "accepted an output whose elements overlap: dims %s strides %s" % (dims, strides)
        else:
            assert ans == M.OVERLAP
            refused += 1
            refused_free += int(distinct)
        assert M.dev_view_rule(dims, strides, False) in (M.CONTIGUOUS, M.STRIDED)  # (an input may overlap)
    assert accepted >= 40 and refused - refused_free >= 100  # (the draw reaches both answers; refused_free: refusals the test need not make)


# ---- the forms ------------------------------------------------------------------------------------------------------------------------
def test_unit_form_and_walker_counts():
    A = 4096  # an aligned base address
    rect = View.whole("float32", (10, 64)).sliced(slice(2, 9), slice(8, 40))  # offset 136 elements, rows of 32, stride 64: whole 16-byte units
    assert M.unit_form(rect, A + rect.offset * 4, A, 4) == 16
    assert M.unit_form(rect, A + rect.offset * 4, A + 8, 4) == 8  # (the dense side is only 8-aligned)
    moved = rect._replace(offset=rect.offset + 1)
    assert M.unit_form(moved, A + moved.offset * 4, A, 4) == M.ELEMENT
    r8 = View.whole("float32", (10, 62)).sliced(slice(2, 9), slice(8, 40))  # row stride 62 elements = 248 bytes: 8-byte units only
    assert M.unit_form(r8, A + r8.offset * 4, A, 4) == 8
    assert M.unit_form(View.whole("float64", (10, 64)).sliced(slice(0, 10), slice(0, 32)), A, A, 8) == 16
    assert M.unit_form(View.whole("float32", (10, 64)), A, A, 4) == M.ELEMENT  # contiguous: the plain loop
    assert M.unit_form(rect.permuted((1, 0)), A + rect.offset * 4, A, 4) == M.ELEMENT  # innermost stride is not 1
    assert M.launch_form(rect, A + rect.offset * 4, A, False) == (16, 8) and M.launch_form(rect, A + rect.offset * 4, A, True) == (M.ELEMENT, 32)
    assert M.launch_form(View.whole("float32", (10, 64)), A, A, False) == (None, None)
    assert [M.rows_per_wave(i) for i in (1, 2, 5, 31, 32, 33, 1025)] == [64, 32, 12, 2, 1, 1, 1]
    assert [M.row_passes(i) for i in (1, 31, 32, 256, 257, 1024, 1025)] == [1, 1, 1, 1, 2, 4, 5]

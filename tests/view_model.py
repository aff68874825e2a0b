"""The rules of the device-memory calls' strided views, restated in numpy: which elements of a base allocation a
view names, what the allocation holds after a decode into the view, what sz3hip_host.cpp's dev_view answers for a view, which form of
k_strided (sz3hip_kernels.hip) a launch takes, and the widening / narrowing between the integer types and f64. No device, no library: a
plain module that tests/test_view_model_cpu.py holds to numpy itself, and that the fixed cases (tests/test_gpu_device_views.py) and the
sweep (tests/checks/device_view_sweep.py) take their expected arrays and their tallies from.
A view is a View: element type, element offset into the base allocation, extents and element strides (>= 0; 0 is a broadcast)."""
import itertools
from collections import namedtuple

import numpy as np

DTYPES = ("float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64")  # (index = SZ3HIP_FLOAT .. SZ3HIP_INT64)
INT_TYPES = DTYPES[2:]
INNERS = (1, 2, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025)  # the row walker's edges: packed waves, one wave, ragged rows, several passes
ELEMENT = "element"


class View(namedtuple("View", "dtype offset shape strides")):
    """the view of a base allocation of `dtype` elements: offset, extents and strides in elements"""
    __slots__ = ()

    @staticmethod
    def whole(dtype, shape, offset=0):
        shape = tuple(int(d) for d in shape)
        run, st = 1, []
        for d in reversed(shape):
            st.append(run)
            run *= d
        return View(np.dtype(dtype).name, int(offset), shape, tuple(reversed(st)))

    def sliced(self, *slices):
        """per axis a slice (start, stop, step > 0), as numpy slices"""
        off, shape, st = self.offset, [], []
        for d, s, sl in zip(self.shape, self.strides, slices):
            lo, hi, step = sl.indices(d)
            assert step > 0
            shape.append(max(0, (hi - lo + step - 1) // step))
            st.append(s * step)
            off += lo * s
        return View(self.dtype, off, tuple(shape), tuple(st))

    def permuted(self, perm):
        return View(self.dtype, self.offset, tuple(self.shape[p] for p in perm), tuple(self.strides[p] for p in perm))

    def field(self, k):
        """element k of the last axis (one field of interleaved records): the axis goes"""
        assert 0 <= k < self.shape[-1]
        return View(self.dtype, self.offset + k * self.strides[-1], self.shape[:-1], self.strides[:-1])

    def expanded(self, axis, n):
        """an axis of extent 1 read n times: stride 0 (torch's expand)"""
        assert self.shape[axis] == 1
        shape, st = list(self.shape), list(self.strides)
        shape[axis], st[axis] = int(n), 0
        return View(self.dtype, self.offset, tuple(shape), tuple(st))

    def dropped(self):
        """without the extents of one, the way a Config and the Python face drop them"""
        keep = [i for i, d in enumerate(self.shape) if d != 1]
        if not keep:
            return View(self.dtype, self.offset, (1,), (1,))
        return View(self.dtype, self.offset, tuple(self.shape[i] for i in keep), tuple(self.strides[i] for i in keep))

    @property
    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))

    @property
    def itemsize(self):
        return np.dtype(self.dtype).itemsize

    @property
    def last(self):
        """the largest element offset the view names"""
        return self.offset + sum((d - 1) * s for d, s in zip(self.shape, self.strides))


def host_view(base, offset, shape, strides):
    """the as_strided view of the 1-D array `base`: element offset, extents, element strides"""
    base = np.asarray(base).reshape(-1)
    shape, strides = tuple(int(d) for d in shape), tuple(int(s) for s in strides)
    assert offset >= 0 and all(s >= 0 for s in strides)
    if all(d > 0 for d in shape):
        assert offset + sum((d - 1) * s for d, s in zip(shape, strides)) < base.size, "the view leaves the allocation"
    return np.lib.stride_tricks.as_strided(base[offset:], shape, tuple(s * base.itemsize for s in strides))


def view_of(base, view):
    return host_view(np.asarray(base).reshape(-1).view(view.dtype), view.offset, view.shape, view.strides)


def expected_after_scatter(base_bytes, view, values):
    """the whole base allocation (uint8) after `values` were decoded into the view: a new array"""
    out = np.array(base_bytes, dtype=np.uint8, copy=True).reshape(-1)
    values = np.asarray(values)
    assert values.dtype == np.dtype(view.dtype) and values.size == view.numel
    view_of(out, view)[...] = values.reshape(view.shape)
    return out


# ---- dev_view ----------------------------------------------------------------------------------------------------------------------
CONTIGUOUS, STRIDED, NEGATIVE, OVERLAP = "contiguous", "strided", "negative", "overlap"


def dev_view_rule(dims, strides, output):
    """dev_view's answer for N extents and their element strides (None: contiguous): CONTIGUOUS / STRIDED, or the refusal NEGATIVE (any
    negative stride) / OVERLAP (outputs; the sufficient test: the strides of the extents > 1 in increasing order, each beyond what the smaller
    ones reach)"""
    dims = [int(d) for d in dims]
    if strides is None:
        return CONTIGUOUS
    strides = [int(s) for s in strides]
    contig, run = True, 1
    for d, s in zip(reversed(dims), reversed(strides)):
        if s < 0:
            return NEGATIVE
        if d > 1 and s != run:
            contig = False
        run *= d
    if contig:
        return CONTIGUOUS
    if output:
        reach = 0
        for s, d in sorted((s, d) for d, s in zip(dims, strides) if d > 1):
            if s <= reach:
                return OVERLAP
            reach += s * (d - 1)
    return STRIDED


def touched_offsets(dims, strides):
    """brute force: every element offset the view names, with repeats"""
    return [sum(i * s for i, s in zip(idx, strides)) for idx in itertools.product(*[range(d) for d in dims])]


# ---- the forms of k_strided ----------------------------------------------------------------------------------------------------------
def _padded(view):
    n = len(view.shape)
    assert 1 <= n <= 4
    return (1,) * (4 - n) + tuple(view.shape), (0,) * (4 - n) + tuple(view.strides)


def unit_form(view, strided_base_addr, dense_base_addr, itemsize):
    """launch_copy's choice for a copy (no widening, no narrowing) between the view at strided_base_addr and the dense buffer at
    dense_base_addr: 16, 8 (view_in_units: bytes per unit) or ELEMENT. The view's extents are those the call is given (View.dropped() for
    the Python face)."""
    dims, st = _padded(view)
    if dev_view_rule(view.shape, view.strides, False) == CONTIGUOUS:
        return ELEMENT
    for unit in (16, 8):
        if itemsize >= unit or st[3] != 1 or strided_base_addr % unit or dense_base_addr % unit:
            continue
        if (dims[3] * itemsize) % unit:
            continue
        if any(dims[d] > 1 and (st[d] * itemsize) % unit for d in range(3)):
            continue
        return unit
    return ELEMENT


def launch_form(view, strided_base_addr, dense_base_addr, converts):
    """-> (form, inner): the unit form of a launch over the view (a widening or narrowing launch is always element-wide; None for the
    contiguous loop) and the row length the walker sees, in units"""
    if dev_view_rule(view.shape, view.strides, False) == CONTIGUOUS:
        return None, None
    form = ELEMENT if converts else unit_form(view, strided_base_addr, dense_base_addr, view.itemsize)
    inner = view.shape[-1] if form == ELEMENT else view.shape[-1] * view.itemsize // form
    return form, inner


def rows_per_wave(inner):
    return 64 // inner if inner < 32 else 1


def row_passes(inner):
    """trips of the walker's `x += 4 * xstep` loop over one row (its busiest lane's)"""
    return 1 if inner < 32 else (inner + 255) // 256


# ---- widening and narrowing ----------------------------------------------------------------------------------------------------------
def widen(a):
    return np.asarray(a).astype(np.float64)


def clamp_ends(dtype):
    """(lo, hi) of the narrowing as doubles: the type's ends; for the 64-bit types hi is the largest double below 2^63 / 2^64"""
    info = np.iinfo(dtype)
    lo = float(info.min)
    hi = float(info.max) if info.bits < 64 else float(np.nextafter(np.float64(2.0 ** (63 if info.min < 0 else 64)), 0.0))
    return lo, hi


def narrow(v, dtype):
    """clip(rint(v), lo, hi), ties to even, NaN to lo — fmin(fmax(rint(v), lo), hi) — as the integer type"""
    dtype = np.dtype(dtype)
    lo, hi = clamp_ends(dtype)
    r = np.fmin(np.fmax(np.rint(np.asarray(v, dtype=np.float64)), lo), hi)
    if dtype == np.uint64:  # (through two halves: every double from 2^63 on is a multiple of 2048, the difference is exact)
        top = r >= 2.0 ** 63
        out = np.where(top, r - 2.0 ** 63, r).astype(np.uint64)
        return out + np.where(top, np.uint64(1 << 63), np.uint64(0))
    return r.astype(dtype)


def narrowing_probe(dtype):
    """ties, one below / at / above both ends of the type (the doubles next to them where the end itself is no double's neighbour by 1),
    signed zeros, NaN, infinities"""
    info = np.iinfo(dtype)
    v = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.0, -0.0, float("nan"), float("inf"), float("-inf"), 0.49999999999999994, 3.0, -3.0, 126.5, 127.5]
    for end in (float(info.min), float(info.max)):
        v += [end, end - 1.0, end + 1.0, end - 0.5, end + 0.5, float(np.nextafter(end, -np.inf)), float(np.nextafter(end, np.inf))]
    return np.array(v, dtype=np.float64)


def beyond_2_53(a):
    """the flag of the widening: an element of a 64-bit integer array strictly beyond 2^53 in magnitude"""
    a = np.asarray(a)
    if a.dtype == np.uint64:
        return bool((a > np.uint64(1 << 53)).any())
    if a.dtype == np.int64:
        return bool(((a > (1 << 53)) | (a < -(1 << 53))).any())
    return False

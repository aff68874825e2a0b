"""The gradient's rule in numpy float64, written as the header states it, and the helpers of the gradient's tests: output
shapes and comparisons in bytes and in units in the last place. Along axis a, with extent E and index i:

    ip = min(i + 1, E - 1), im = max(i, 1) - 1, s = spacing[a] * 2^level
    d_a = E == 1 ? +0.0 : (x[ip] - x[im]) / ((double)(ip - im) * s)

— clamped index arrays, one subtraction, one division by (ip - im) * s; the magnitude is m = m + d * d in a loop over the axes. Nothing here
calls numpy's own gradient or norm."""
import numpy as np

OPS = {"deriv": 0, "mag2": 1, "mag": 2, "vector": 3}


def scale_of(spacing, N, level=0):
    """the grid steps s_a = ldexp(spacing[a], level); spacing: None (1.0), a scalar or one value per axis"""
    if spacing is None:
        spacing = (1.0,) * N
    elif np.ndim(spacing) == 0:
        spacing = (float(spacing),) * N
    assert len(spacing) == N
    return tuple(float(np.ldexp(np.float64(s), level)) for s in spacing)


def deriv(values, a, s):
    """the derivative along axis `a` of the whole box, float64"""
    x = np.asarray(values).astype(np.float64)
    E = x.shape[a]
    if E == 1:
        return np.zeros(x.shape, np.float64)
    i = np.arange(E)
    ip = np.minimum(i + 1, E - 1)
    im = np.maximum(i, 1) - 1
    shape = [1] * x.ndim
    shape[a] = E
    den = (ip - im).astype(np.float64) * np.float64(s)
    with np.errstate(all="ignore"):
        diff = np.take(x, ip, axis=a) - np.take(x, im, axis=a)
        return diff / den.reshape(shape)


def differentiated(op, axis, N):
    return (axis % N,) if op == "deriv" else tuple(range(N))


def out_shape(shape, op, axis=0, interior=False):
    axes = differentiated(op, axis, len(shape)) if interior else ()
    return tuple(e - 2 if j in axes else e for j, e in enumerate(shape))


def trim(arr, op, axis, N, interior):
    """the box without its first and last point along every differentiated axis (arr may carry a trailing component dimension)"""
    if not interior:
        return arr
    sl = [slice(None)] * arr.ndim
    for j in differentiated(op, axis, N):
        sl[j] = slice(1, arr.shape[j] - 1)
    return arr[tuple(sl)]


def gradient(values, op, axis=0, spacing=None, level=0, out_dtype=None, interior=False, sqrt=True):
    """the output of a box with values `values` (what a request delivers): an array of out_dtype (default: the values') of the output box's
    shape, for "vector" with a last dimension N. sqrt=False: "mag" stops at the float64 sum m (the caller takes the root)"""
    values = np.asarray(values)
    N = values.ndim
    s = scale_of(spacing, N, level)
    T = np.dtype(values.dtype if out_dtype is None else out_dtype)
    with np.errstate(all="ignore"):
        if op == "deriv":
            r = deriv(values, axis % N, s[axis % N])
        elif op == "vector":
            r = np.stack([deriv(values, a, s[a]) for a in range(N)], axis=-1)
        else:
            m = np.zeros(values.shape, np.float64)
            for a in range(N):
                d = deriv(values, a, s[a])
                m = m + d * d
            r = np.sqrt(m) if op == "mag" and sqrt else m
        r = trim(r, op, axis, N, interior)
        return r if op == "mag" and not sqrt else r.astype(T)


def same_bytes(got, want):
    """byte equality, a NaN matching any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    U = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    g, w = np.ascontiguousarray(got).view(U), np.ascontiguousarray(want).view(U)
    return bool(np.all((g == w) | nan))


def ulp_apart(got, want):
    """the count of elements that differ at all and the largest distance in units in the last place (NaNs must agree; equal values: 0)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    I = np.int32 if got.dtype.itemsize == 4 else np.int64
    g, w = got.view(I).astype(np.int64), want.view(I).astype(np.int64)
    d = np.where(nan | (got == want), 0, np.abs(g - w))  # (non-negative results: the integer order is the floating one)
    return int(np.count_nonzero(d)), int(d.max()) if d.size else 0

"""The compositing rule (include/sz3hip.h) in numpy float64, exactly as written: a Python loop over the axis index on
whole slices, an `active` mask for the cutoff, the table's squarings in a loop. No cumprod, no pow, no np.sum: every operation is one
IEEE double operation rounded on its own, in the rule's order.

    corrected_alpha(lut, s)                    the opacities after s squarings (float64)
    codes(x, lo, hi, lut_n)                    the window's codes of values that are no NaN
    composite(v, axis, lut, lo, hi, ...)       the state (R, G, B, A) as float64, shape = v's with 1 at `axis`, plus a last dimension 4
    store(state, out_type)                     the output element's bytes: float32 (..., 4) or uint32 (...)
    expected(v, axis, lut, lo, hi, out_type, ...)   composite + store; `carry` is the float32 image an ACCUMULATE call starts from"""
import numpy as np

RGBA32F, RGBA8 = "rgba32f", "rgba8"


def corrected_alpha(lut, s):
    a = np.asarray(lut, dtype=np.float32)[:, 3].astype(np.float64)
    if s == 0:
        return a
    with np.errstate(all="ignore"):
        t = 1.0 - a
        for _ in range(s):
            t = t * t
        return 1.0 - t


def codes(x, lo, hi, lut_n):
    """x: float64 without NaN"""
    M = lut_n - 1
    scale = float(M + 1) / (hi - lo)
    with np.errstate(all="ignore"):
        inside = (x >= lo) & (x < hi)
        k = np.where(inside, (x - lo) * scale, 0.0).astype(np.uint64)  # (truncation, as the C cast)
    k = np.minimum(k, np.uint64(M))
    return np.where(x < lo, 0, np.where(x >= hi, M, k)).astype(np.int64)


def composite(v, axis, lut, lo, hi, reverse=False, s=0, cutoff=np.inf, carry=None):
    v = np.asarray(v)
    lut = np.asarray(lut, dtype=np.float32)
    E = v.shape[axis]
    flat = tuple(1 if j == axis else e for j, e in enumerate(v.shape))
    rgb = lut[:, :3].astype(np.float64)
    alpha = corrected_alpha(lut, s)
    if carry is None:
        R, G, B, A = (np.zeros(flat, dtype=np.float64) for _ in range(4))
    else:
        c = np.asarray(carry, dtype=np.float32).reshape(flat + (4,)).astype(np.float64)
        R, G, B, A = (c[..., j].copy() for j in range(4))
    active = np.ones(flat, dtype=bool)
    order = range(E - 1, -1, -1) if reverse else range(E)
    with np.errstate(all="ignore"):
        for i in order:
            x = np.take(v, [i], axis=axis).astype(np.float64)
            nan = np.isnan(x)
            c = codes(np.where(nan, lo, x), lo, hi, lut.shape[0])
            a, r, g, b = alpha[c], rgb[c, 0], rgb[c, 1], rgb[c, 2]
            fold = active & ~nan
            w = (1.0 - A) * a
            R = np.where(fold, R + w * r, R)
            G = np.where(fold, G + w * g, G)
            B = np.where(fold, B + w * b, B)
            A = np.where(fold, A + w, A)
            active = active & ~(fold & (A >= cutoff))
    return np.stack([R, G, B, A], axis=-1)


def pack8(c):
    """one channel's byte: q = c * 255.0 + 0.5; q > 0 ? (q >= 255 ? 255 : (uint8_t)q) : 0 — a NaN gives 0"""
    with np.errstate(all="ignore"):
        q = np.asarray(c, dtype=np.float64) * 255.0 + 0.5
        pos = q > 0
        return np.where(pos, np.where(q >= 255, 255, np.where(pos & (q < 255), q, 0.0).astype(np.uint8)), 0).astype(np.uint32)


def store(state, out_type):
    if out_type == RGBA32F:
        with np.errstate(all="ignore"):
            return state.astype(np.float32)
    b = pack8(state)
    return b[..., 0] | b[..., 1] << np.uint32(8) | b[..., 2] << np.uint32(16) | b[..., 3] << np.uint32(24)


def expected(v, axis, lut, lo, hi, out_type=RGBA32F, reverse=False, s=0, cutoff=np.inf, carry=None):
    return store(composite(v, axis, lut, lo, hi, reverse, s, cutoff, carry), out_type)

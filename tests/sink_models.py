"""The numpy rules the GPU tests of the opened stream hold its sinks to — Stream.request (test_gpu_request.py), reduce (test_gpu_reduce.py),
select (test_gpu_select.py), map (test_gpu_map.py), sample (test_gpu_sample.py), project (test_gpu_project.py) — and the buffers they check
them in, in one place: those test files and tests/checks/partial_sweep.py share them. A plain module: it holds no test and no fixture. Where
two files had a helper of one name (check_box, expected, filled, host, untouched) the name carries its sink here; the bodies are unchanged."""
import ctypes as C
from fractions import Fraction

import numpy as np
import torch

import sz3_amd
from partial_cases import DEV

L = sz3_amd.lib()


# ---- the coarse grid (test_gpu_stream.py) ------------------------------------------------------------------------------------------------------
def coarse_shape(shape, k):
    return tuple(((d - 1) >> k) + 1 for d in shape)


def coarse_view(full, k):
    return full[tuple(slice(None, None, 1 << k) for _ in full.shape)]


# ---- Stream.request's outputs (test_gpu_request.py) --------------------------------------------------------------------------------------------
SENTINEL = 77.0


def tdt(st):
    return getattr(torch, st.dtype.name)


def atlas_for(st, items, pad=0):
    """one atlas tensor and the items' rectangles in it, side by side along x (their byte hulls interleave): (atlas, views)"""
    N = len(items[0][2])
    dims = [max(it[2][j] for it in items) + pad for j in range(N - 1)] + [sum(it[2][-1] + pad for it in items)]
    atlas = torch.full(dims, SENTINEL, dtype=tdt(st), device=DEV)
    views, x = [], 0
    for _, _, ext in items:
        views.append(atlas[tuple(slice(0, e) for e in ext[:-1]) + (slice(x, x + ext[-1]),)])
        x += ext[-1] + pad
    return atlas, views


def untouched(buf, views):
    """everything of buf outside the views still holds the sentinel"""
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    base = buf.data_ptr()
    for v in views:
        off = (v.data_ptr() - base) // buf.element_size()
        mask.view(-1).as_strided(tuple(v.shape), tuple(v.stride()), off).fill_(True)
    return bool((buf[~mask] == SENTINEL).all())


# ---- reduce (test_gpu_reduce.py) ---------------------------------------------------------------------------------------------------------------
EXACT_POINTS = 20000
U = Fraction(1, 2 ** 53)


def gamma(k):
    return k * U / (1 - k * U)


def bits(x):
    return np.float64(x).tobytes()


def hist_of(x, bins, lo, hi):
    """the header's rule in numpy float64: slot 0 under, slot bins + 1 over, else 1 + min((uint64)((x - lo) * scale), bins - 1)"""
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(bins) / (hi - lo)
    x = x[np.isfinite(x)]
    want = np.zeros(bins + 2, dtype=np.uint64)
    want[0] = (x < lo).sum()
    want[bins + 1] = (x >= hi).sum()
    mid = x[(x >= lo) & (x < hi)]
    k = np.minimum(((mid - lo) * scale).astype(np.uint64), np.uint64(bins - 1))
    want[1:bins + 1] = np.bincount(k.astype(np.int64), minlength=bins)
    return want


def reduce_check_box(s, h, v, bins=0, lo=0.0, hi=0.0, what=""):
    """one sz3hip_box_stats record (a row of the structured array) and its histogram row against the numpy array v (the box's values)"""
    x = np.asarray(v).astype(np.float64).reshape(-1)  # ((double)v: exact)
    fin = np.isfinite(x)
    n, nf = x.size, int(fin.sum())
    assert int(s["n"]) == n and int(s["n_nonfinite"]) == n - nf, what
    if nf:
        amin, amax = int(np.where(fin, x, np.inf).argmin()), int(np.where(fin, x, -np.inf).argmax())
        assert (int(s["argmin"]), int(s["argmax"])) == (amin, amax), what
        assert bits(s["min"]) == bits(x[amin]) and bits(s["max"]) == bits(x[amax]), what
    else:
        assert int(s["argmin"]) == n and int(s["argmax"]) == n and np.isnan(s["min"]) and np.isnan(s["max"]), what
    K = x[0] if fin[0] else np.float64(0.0)
    assert bits(s["shift"]) == bits(K), what
    with np.errstate(all="ignore"):
        m = np.float64(int(s["n"]) - int(s["n_nonfinite"]))
        mean = s["shift"] + s["sum"] / m
        var = (s["sum_sq"] - s["sum"] * s["sum"] / m) / m
    if nf:
        assert bits(s["mean"]) == bits(mean) and bits(s["variance"]) == bits(var), what
    else:
        assert np.isnan(s["mean"]) and np.isnan(s["variance"]) and s["sum"] == 0.0 and s["sum_sq"] == 0.0, what
    if n <= EXACT_POINTS:
        d = [Fraction(float(t)) - Fraction(float(K)) for t in x[fin]]
        s1, a1, s2 = sum(d, Fraction(0)), sum((abs(t) for t in d), Fraction(0)), sum((t * t for t in d), Fraction(0))
        e1, e2 = abs(Fraction(float(s["sum"])) - s1), abs(Fraction(float(s["sum_sq"])) - s2)
        print("%s n %d: |sum - exact| %.3e (bound %.3e), |sum_sq - exact| %.3e (bound %.3e)" % (what, n, e1, gamma(n) * a1, e2, gamma(n + 2) * s2))
        assert e1 <= gamma(n) * a1, what
        assert e2 <= gamma(n + 2) * s2, what
    if bins:
        want = hist_of(x, bins, lo, hi)
        assert np.array_equal(h.view(np.uint64), want), what
        assert int(h.sum()) == nf, what
    else:
        assert h is None


# ---- select (test_gpu_select.py) ---------------------------------------------------------------------------------------------------------------
SENT = 0x4D4D4D4D4D4D4D4D


def pred(x, lo, hi, invert=False, nan=False):
    """the header's rule over float64 values"""
    with np.errstate(invalid="ignore"):
        inside = (lo <= x) & (x <= hi)
    return np.where(np.isnan(x), bool(nan), inside != bool(invert))


def utype(dt):
    return np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64


def sentinels(caps, tdtype, values=True):
    """index and value arrays of the capacities (at least one element each, so that a capacity of 0 has something to leave alone), every byte 0x4D"""
    index = [torch.full((max(c, 1),), SENT, dtype=torch.int64, device=DEV) for c in caps]
    value = [torch.full((max(c, 1) * t_size(tdtype),), 0x4D, dtype=torch.uint8, device=DEV).view(tdtype) for c in caps] if values else None
    return index, value


def t_size(tdtype):
    return 4 if tdtype == torch.float32 else 8


def raw_select(st, items, caps, lo, hi, invert=False, nan=False, values=True, stream=None, n=None):
    """sz3hip_stream_select into sentinel-filled arrays: (rc, heads, index, value) — nothing waits"""
    tdtype = getattr(torch, st.dtype.name)
    heads = torch.full((max(len(items), 1), 4), SENT, dtype=torch.int64, device=DEV)
    index, value = sentinels(caps, tdtype, values)
    reqs, cnt = sz3_amd._select_reqs(st.conf.N, items, caps, index, value)
    opts = sz3_amd._select_opts(lo, hi, invert, nan)
    rc = L.sz3hip_stream_select(st._h, reqs, cnt if n is None else n, C.byref(opts), heads.data_ptr(), sz3_amd._stream_handle(DEV, stream))
    return rc, heads, index, value


def select_check_box(head, index, value, s, cap, lo, hi, invert=False, nan=False, what=""):
    """one head row, one sentinel-filled index array and value array (host copies) against the numpy array s (the box's values)"""
    s = np.asarray(s)
    x = s.astype(np.float64).reshape(-1)
    idx = np.flatnonzero(pred(x, lo, hi, invert, nan))
    written = min(idx.size, cap)
    assert [int(v) for v in head] == [x.size, idx.size, written, cap], "%s head %s, expected n %d count %d written %d capacity %d" % (what, head, x.size, idx.size, written, cap)
    assert np.array_equal(index[:written], idx[:written]), what + " the indices differ"
    assert (index[written:].view(np.uint64) == SENT).all(), what + " an index behind `written` was touched"
    if value is not None:
        u = utype(s.dtype)
        assert np.array_equal(value.view(u)[:written], s.reshape(-1)[idx[:written]].view(u)), what + " the values' bytes differ"
        assert (value.view(np.uint8)[written * s.dtype.itemsize:] == 0x4D).all(), what + " a value behind `written` was touched"
    return idx.size


# ---- map (test_gpu_map.py) ---------------------------------------------------------------------------------------------------------------------
FILL = 0x4D
NP_OUT = {"u8": np.uint8, "u16": np.uint16, "f16": np.float16, "f32": np.float32, "lut32": np.uint32}
TORCH_OUT = {"u8": torch.uint8, "u16": torch.int16, "f16": torch.float16, "f32": torch.float32, "lut32": torch.int32}
LAST = {"u8": 255, "u16": 65535}
NAN_TEXEL = 0xDEADBEEF


def np_codes(x, lo, hi, M, nan_code):
    """the header's rule over float64 values: scale once, NaN -> nan_code, x < lo -> 0, x >= hi -> M, else min(uint64((x - lo) * scale), M)"""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(M + 1) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (x >= lo) & (x < hi)
        k = np.minimum(np.where(inside, (x - lo) * scale, 0.0).astype(np.uint64), np.uint64(M))
        c = np.where(x < lo, np.uint64(0), np.where(x >= hi, np.uint64(M), k))
    return np.where(np.isnan(x), np.uint64(nan_code), c)


def make_lut(n, seed=5):
    """a seeded random table of n 32-bit texels that does not hold NAN_TEXEL: (host uint32 array, device int32 tensor)"""
    t = np.random.default_rng(seed + n).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    t[t == NAN_TEXEL] = 1
    return t, torch.from_numpy(t.view(np.int32).copy()).to(DEV)


def opts_for(out_type, lo=0.0, hi=0.0, nan_code=0, lut=None):
    """keyword arguments of Stream.map / map_points for one output type (a float output takes no window)"""
    if out_type in ("f16", "f32"):
        return {}
    if out_type == "lut32":
        return dict(lo=lo, hi=hi, nan_code=NAN_TEXEL, lut=lut[1])
    return dict(lo=lo, hi=hi, nan_code=nan_code)


def map_expected(s, out_type, lo=0.0, hi=0.0, nan_code=0, lut=None):
    s = np.asarray(s)
    if out_type == "f32":
        with np.errstate(over="ignore"):
            return s.astype(np.float32)
    if out_type == "f16":
        with np.errstate(over="ignore"):
            return s.astype(np.float32).astype(np.float16)
    x = s.astype(np.float64)
    if out_type == "lut32":
        codes = np_codes(x, lo, hi, lut[0].size - 1, 0)
        return np.where(np.isnan(x), np.uint32(NAN_TEXEL), lut[0][codes.astype(np.int64)])
    return np_codes(x, lo, hi, LAST[out_type], nan_code).astype(NP_OUT[out_type])


def map_filled(shape, out_type):
    """a contiguous tensor of the output type, every byte 0x4D"""
    td = TORCH_OUT[out_type]
    n = int(np.prod(shape))
    return torch.full((n * torch.empty((), dtype=td).element_size(),), FILL, dtype=torch.uint8, device=DEV).view(td).reshape(tuple(shape))


def map_host(t, out_type):
    """a tensor's elements on the host, in the numpy type of the output"""
    return t.contiguous().cpu().numpy().view(NP_OUT[out_type])


def same_texels(got, want, out_type, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if out_type in ("f16", "f32"):
        nan = np.isnan(want)
        assert np.isnan(got[nan]).all(), what + " a NaN point is no NaN"
        u = np.uint16 if out_type == "f16" else np.uint32
        assert np.array_equal(got.view(u)[~nan], want.view(u)[~nan]), what + " the texels' bytes differ"
    else:
        assert np.array_equal(got, want), what + " the texels differ"


def map_untouched(buf, out_type, slices):
    """every byte of buf outside the slices still holds 0x4D"""
    a = buf.cpu().numpy()
    mask = np.zeros(a.shape, dtype=bool)
    for sl in slices:
        mask[sl] = True
    by = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return bool((by[~mask] == FILL).all())


def texel_atlas(items, out_type):
    """one atlas of the output type and the items' rectangles in it, side by side along x with a gap of one texel; the row pitch is odd (in
    texels), so that the rows of a one-byte atlas start on all four byte alignments: (atlas, views, slices)"""
    N = len(items[0][2])
    dims = [max(it[2][j] for it in items) + 1 for j in range(N - 1)] + [sum(it[2][-1] + 1 for it in items)]
    dims[-1] += 1 - dims[-1] % 2
    atlas = map_filled(dims, out_type)
    views, slices, x = [], [], 0
    for _, _, ext in items:
        sl = tuple(slice(0, e) for e in ext[:-1]) + (slice(x, x + ext[-1]),)
        slices.append(sl)
        views.append(atlas[sl])
        x += ext[-1] + 1
    return atlas, views, slices


# ---- sample (test_gpu_sample.py) ---------------------------------------------------------------------------------------------------------------
NAN = float("nan")
RAW = {np.dtype("float32"): np.uint32, np.dtype("float64"): np.uint64}


def np_sample(s, coords, mode, clamp=False, fill=NAN):
    """s: the box's values (a numpy array of the stream's type); coords: (n, N) float32 / float64. The header's rule, in float64."""
    s = np.asarray(s)
    N = s.ndim
    c = np.asarray(coords).astype(np.float64)  # (exact)
    assert c.ndim == 2 and c.shape[1] == N
    last = np.array(s.shape, dtype=np.int64) - 1
    hi = last.astype(np.float64)
    nan = np.isnan(c).any(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        if clamp:
            c = np.where(np.isnan(c), c, np.where(c < 0.0, 0.0, np.where(c > hi, hi, c)))
            inside = ~nan
        else:
            inside = ((0.0 <= c) & (c <= hi)).all(axis=1)
        out = np.full(c.shape[0], fill, dtype=np.float64).astype(s.dtype)
        ci = c[inside]
        if mode == "nearest":
            i = np.minimum(np.floor(ci + 0.5).astype(np.int64), last)
            u = RAW[s.dtype]
            out.view(u)[inside] = s.view(u)[tuple(i.T)]  # raw bytes
            return out
        fl = np.floor(ci)
        i = fl.astype(np.int64)
        f = ci - fl
        i1 = np.minimum(i + 1, last)
        # corner k: bit d of k picks i + 1 along dimension N - 1 - d
        w = [s[tuple((i1 if (k >> (N - 1 - j)) & 1 else i)[:, j] for j in range(N))].astype(np.float64) for k in range(1 << N)]
        for d in range(N):  # the fastest dimension first
            fd = f[:, N - 1 - d]
            gd = 1.0 - fd
            w = [np.where(fd == 0.0, w[2 * m], gd * w[2 * m] + fd * w[2 * m + 1]) for m in range(len(w) // 2)]
        out[inside] = w[0].astype(s.dtype)  # one rounding
    return out


def np_lattice(origin, steps, counts):
    """the lattice's coordinates by the header's formula: ((origin + i0 * s0) + i1 * s1) + i2 * s2 in float64, query-major"""
    counts = (1,) * (3 - len(counts)) + tuple(counts)
    steps = [(0.0,) * len(origin)] * (3 - len(steps)) + [tuple(st) for st in steps]
    i0, i1, i2 = [g.reshape(-1).astype(np.float64) for g in np.meshgrid(*[np.arange(c) for c in counts], indexing="ij")]
    cols = []
    for j, o in enumerate(origin):
        cols.append(((np.float64(o) + i0 * np.float64(steps[0][j])) + i1 * np.float64(steps[1][j])) + i2 * np.float64(steps[2][j]))
    return np.stack(cols, axis=1)


def same_values(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what + " a NaN result is no NaN"
    u = RAW[want.dtype]
    bad = np.flatnonzero(got.view(u)[~nan] != want.view(u)[~nan])
    assert bad.size == 0, "%s %d results differ in their bytes, the first at %d: %r, not %r" % (what, bad.size, bad[0], got[~nan][bad[0]], want[~nan][bad[0]])


# ---- project (test_gpu_project.py) -------------------------------------------------------------------------------------------------------------
OPS = ["min", "max", "sum", "mean", "argmin", "argmax", "count"]
INDEX_OPS = ("argmin", "argmax", "count")
OUTS = ["float32", "float64"]


def combos():
    """(op, out_dtype name or None): every op, the value ops into both output types"""
    return [(op, None) for op in INDEX_OPS] + [(op, o) for op in OPS[:4] for o in OUTS]


def np_fold(s, axis):
    """the header's rule over a slice: one pass over the axis index, ascending, every column at once"""
    x = np.moveaxis(np.asarray(s).astype(np.float64), axis, 0)
    E, shape = x.shape[0], x.shape[1:]
    ssum, cnt = np.zeros(shape), np.zeros(shape, dtype=np.int64)
    amin, amax = np.full(shape, E, dtype=np.int64), np.full(shape, E, dtype=np.int64)
    vmin, vmax = np.zeros(shape), np.zeros(shape)
    with np.errstate(all="ignore"):
        for i in range(E):
            xi = x[i]
            fin = np.abs(xi) < np.inf
            ssum = np.where(fin, ssum + xi, ssum)
            cnt = cnt + fin
            lower = fin & ((amin == E) | (xi < vmin))  # (strictly smaller: of equal values, -0.0 and +0.0 among them, the first stays)
            vmin, amin = np.where(lower, xi, vmin), np.where(lower, i, amin)
            upper = fin & ((amax == E) | (xi > vmax))
            vmax, amax = np.where(upper, xi, vmax), np.where(upper, i, amax)
    return dict(E=E, sum=ssum, count=cnt, argmin=amin, argmax=amax, min=vmin, max=vmax)


def project_expected(f, op, axis, out_name, fill=NAN):
    """the output of a fold: fill and the one rounding, the axis kept with extent 1"""
    with np.errstate(all="ignore"):
        if op in INDEX_OPS:
            r = f[op].astype(np.uint32)
        else:
            t = np.dtype(out_name).type
            if op == "sum":
                r = f["sum"].astype(t)
            elif op == "mean":
                r = np.where(f["count"] > 0, f["sum"] / f["count"].astype(np.float64), np.float64(fill)).astype(t)
            else:
                r = np.where(f["arg" + op] < f["E"], f[op], np.float64(fill)).astype(t)
    return np.expand_dims(r, axis)


def out_name(op, out, dtype):
    return "int32" if op in INDEX_OPS else (out or np.dtype(dtype).name)


def project_filled(shape, name):
    """a contiguous tensor of the output's torch type (int32 for the index ops), every byte 0x4D"""
    td = getattr(torch, name)
    n = int(np.prod(shape))
    return torch.full((n * torch.empty((), dtype=td).element_size(),), FILL, dtype=torch.uint8, device=DEV).view(td).reshape(tuple(shape))


def project_host(t):
    a = t.contiguous().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def same_bytes(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, "%s %s %s / %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if want.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.isnan(got[nan]).all(), what + " a NaN output is no NaN"
        u = np.uint32 if want.dtype.itemsize == 4 else np.uint64
        bad = got.view(u)[~nan] != want.view(u)[~nan]
        assert not bad.any(), "%s %d outputs' bytes differ, first: got %r want %r" % (what, int(bad.sum()), got[~nan][bad][:3], want[~nan][bad][:3])
    else:
        assert np.array_equal(got, want), what + " the indices differ"


def project_untouched(buf, slices):
    """every byte of buf outside the slices still holds 0x4D"""
    a = buf.cpu().numpy()
    mask = np.zeros(a.shape, dtype=bool)
    for sl in slices:
        mask[sl] = True
    by = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return bool((by[~mask] == FILL).all())


def flat(ext, axis):
    return tuple(1 if j == axis else e for j, e in enumerate(ext))


def atlas_of(shapes, name):
    """one atlas of the output type and the shapes' rectangles in it, side by side along x with a gap of one element; the row pitch is odd"""
    N = len(shapes[0])
    dims = [max(s[j] for s in shapes) + 1 for j in range(N - 1)] + [sum(s[-1] + 1 for s in shapes)]
    dims[-1] += 1 - dims[-1] % 2
    atlas = project_filled(dims, name)
    views, slices, x = [], [], 0
    for s in shapes:
        sl = tuple(slice(0, e) for e in s[:-1]) + (slice(x, x + s[-1]),)
        slices.append(sl)
        views.append(atlas[sl])
        x += s[-1] + 1
    return atlas, views, slices

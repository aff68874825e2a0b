"""The device-memory calls' strided views on the MI355X: the kernel family k_strided behind
sz3hip_compress_from_device, sz3hip_decompress_to_device and the coarse call's outputs, held case by case to numpy's as_strided view of a
host copy of the same allocation (tests/view_model.py). Everything is compared for equality of bytes — the gathered array, the container
(the host API's), and after a decode the WHOLE allocation, which was filled with random bytes: every byte outside the view counts."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402
import view_model as M  # noqa: E402
from device_views import DEV, Alloc, L, first_difference, gather, gather_expected, same_bytes, scatter_rc  # noqa: E402
from partial_cases import CODES, smooth  # noqa: E402
from view_model import View  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = CODES["SZ3HIP_EINVAL"]
FLOATS = ("float32", "float64")
ROWS = (3, 70)
PERMS3 = list(itertools.permutations(range(3)))


def data_for(shape, dtype, seed=7):
    """a smooth field of the type: floats of amplitude ~1, integers over a sixth of the type's range (at most +-10000) around its middle"""
    f = smooth(shape, "float64", seed=seed) if int(np.prod(shape)) > 1 else np.zeros(shape)
    if dtype in FLOATS:
        return f.astype(dtype)
    info = np.iinfo(dtype)
    amp = min(10000, (int(info.max) - int(info.min)) // 6)
    mid = (int(info.max) + int(info.min) + 1) // 2 if info.bits < 64 else 0 if info.min < 0 else 20000
    return (np.rint(f * amp / 1.3).astype(np.int64) + mid).astype(dtype)


def conf_for(shape, dtype, algo=sz3_amd.ALGO_LORENZO_REG, eb=None, **kw):
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = algo
    c.errorBoundMode = sz3_amd.EB_ABS
    c.absErrorBound = (1e-2 if dtype in FLOATS else 1.0) if eb is None else eb
    c.quantbinCnt = 1024
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def host_container(a, conf):
    return sz3_amd.compress(np.ascontiguousarray(a), conf)[0].tobytes()


@functools.lru_cache(maxsize=None)
def stream_of(dtype, shape, algo=sz3_amd.ALGO_LORENZO_REG):
    """-> (the host API's container of the type's field of this shape, the host API's decode of it): computed once, never written"""
    a = data_for(shape, dtype)
    blob = host_container(a, conf_for(shape, dtype, algo=algo))
    want, _ = sz3_amd.decompress(blob, np.dtype(dtype))
    want.setflags(write=False)
    return blob, want


def permuted_base(shape, perm):
    """the view of extents `shape` that is the permutation `perm` of a contiguous array"""
    base = [0] * len(shape)
    for i, p in enumerate(perm):
        base[p] = shape[i]
    return View.whole("uint8", base).permuted(perm)


def typed(view, dtype, offset=0):
    return View(np.dtype(dtype).name, view.offset + offset, view.shape, view.strides)


def rect(dtype, shape2or3, unit):
    """a rectangle of rows of shape[-1] elements inside rows of twice that, its offset, row length and strides whole `unit`-byte units (and, for 8,
    not whole 16-byte ones): shape[-1] * itemsize must be a multiple of 16"""
    es = np.dtype(dtype).itemsize
    inner = shape2or3[-1]
    assert (inner * es) % 16 == 0 and (inner // 2 * es) % 16 == 0
    base = tuple(d + 2 for d in shape2or3[:-1]) + (2 * inner,)
    v = View.whole(dtype, base).sliced(*([slice(1, 1 + d) for d in shape2or3[:-1]] + [slice(inner // 2, inner // 2 + inner)]))
    return v if unit == 16 else v._replace(offset=v.offset + 8 // es)


def span(view, pad=3):
    return view.last + 1 + pad


# =============================================================================================================================================
# the gather alone
# =============================================================================================================================================
def check_gather(alloc, view, what=""):
    got = gather(alloc, view)
    want = gather_expected(alloc, view)
    assert same_bytes(got, want), "%s gather of %s differs from numpy's view in %d of %d elements" % (
        what, (view,), int((got.reshape(-1).view("u%d" % got.itemsize) != want.reshape(-1).view("u%d" % want.itemsize)).sum()), want.size)


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_gather_inner_extents(dtype):
    """every inner extent at which the row walker changes its form (packed waves below 32, one wave per row, ragged last passes), with 3 and
    with 70 rows, as a sub-box at an odd offset of a base of random bytes (integers over their whole range, the 64-bit ones beyond 2^53)"""
    rng = np.random.default_rng(M.DTYPES.index(dtype))
    for inner in M.INNERS:
        for rows in ROWS:
            v = View.whole(dtype, (rows + 2, inner + 3)).sliced(slice(1, rows + 1), slice(2, inner + 2))
            alloc = Alloc.random(dtype, span(v), rng)
            check_gather(alloc, v, "rows %d inner %d" % (rows, inner))
            assert alloc.unchanged(), "the gather wrote its input (rows %d inner %d)" % (rows, inner)


@pytest.mark.parametrize("dtype", ["float32", "uint8", "int64"])
def test_gather_ranks(dtype):
    rng = np.random.default_rng(3)
    views = [View.whole(dtype, (9000,), offset=1).sliced(slice(5, 8990, 3)),
             View.whole(dtype, (70, 130)).sliced(slice(1, 69, 2), slice(3, 100)),
             View.whole(dtype, (20, 30, 70)).sliced(slice(1, 19), slice(0, 30, 3), slice(2, 67)),
             View.whole(dtype, (6, 9, 11, 40)).sliced(slice(1, 6, 2), slice(2, 9), slice(0, 11, 2), slice(3, 36)),
             View.whole(dtype, (6, 9, 11, 40)).sliced(slice(0, 6), slice(2, 9), slice(0, 11), slice(3, 36)).permuted((3, 1, 0, 2))]
    for v in views:
        alloc = Alloc.random(dtype, span(v), rng)
        check_gather(alloc, v, "rank %d" % len(v.shape))
        assert alloc.unchanged()


def gather_view_kinds(dtype):
    es = np.dtype(dtype).itemsize
    B = (12, 20, 64)
    whole = View.whole(dtype, B)
    sub = whole.sliced(slice(2, 10), slice(3, 17), slice(4, 44))
    kinds = {"subbox": sub}
    for ax in range(3):
        for step in (2, 3):
            kinds["step%d_axis%d" % (step, ax)] = whole.sliced(*[slice(1, None, step) if a == ax else slice(1, d - 1) for a, d in enumerate(B)])
    kinds["step2_every_axis"] = whole.sliced(*[slice(None, None, 2)] * 3)
    kinds["step3_every_axis"] = whole.sliced(*[slice(1, None, 3)] * 3)
    for p in PERMS3:
        kinds["permuted_%d%d%d" % p] = sub.permuted(p)
    kinds["interleaved_field"] = View.whole(dtype, (12, 20, 16, 4)).field(2)
    kinds["stride0_slowest"] = View.whole(dtype, (1, 20, 64), offset=1).expanded(0, 5)
    kinds["stride0_middle"] = View.whole(dtype, (12, 1, 64)).expanded(1, 7).sliced(slice(1, 11), slice(0, 7), slice(3, 60))
    kinds["stride0_fastest"] = View.whole(dtype, (12, 20, 1)).expanded(2, 33)
    r16 = rect(dtype, (10, 16, 32), 16)
    kinds["units16"] = r16
    kinds["units8"] = rect(dtype, (10, 16, 32), 8)
    kinds["units16_moved_by_one"] = r16._replace(offset=r16.offset + 1)
    kinds["contiguous_offset_1"] = View.whole(dtype, B, offset=1)
    return kinds, es


VIEW_KINDS = sorted(gather_view_kinds("float32")[0])


@pytest.mark.parametrize("dtype", ["float32", "float64", "uint8", "int16"])
@pytest.mark.parametrize("kind", VIEW_KINDS)
def test_gather_views(kind, dtype):
    kinds, es = gather_view_kinds(dtype)
    v = kinds[kind]
    alloc = Alloc.random(dtype, span(v), np.random.default_rng(VIEW_KINDS.index(kind)))
    if dtype in FLOATS:  # (the copy has the unit forms: the cases named for them take them)
        form = M.unit_form(v, alloc.addr(v), 0, es)
        want = {"units16": 16, "units8": 8 if es < 8 else M.ELEMENT, "units16_moved_by_one": M.ELEMENT}.get(kind)
        assert want is None or form == want, (kind, form)
    check_gather(alloc, v, kind)
    assert alloc.unchanged(), "the gather wrote its input"


# =============================================================================================================================================
# the scatter: decompress(blob, dtype, out=view), the whole allocation against expected_after_scatter of the host API's decode
# =============================================================================================================================================
def decode_into(blob, want, view, rng, what=""):
    alloc = Alloc.random(view.dtype, span(view), rng)
    out, _ = sz3_amd.decompress(blob, np.dtype(view.dtype), out=alloc.tensor(view))
    assert out.data_ptr() == alloc.addr(view)
    got, exp = alloc.now(), M.expected_after_scatter(alloc.host, view, want)
    assert np.array_equal(got, exp), "%s decode into %s: %s" % (what, (view,), first_difference(got, exp, view))
    return alloc


S3 = (6, 10, 32)


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_scatter_permuted_and_stepped_outputs(dtype):
    rng = np.random.default_rng(11)
    blob, want = stream_of(dtype, S3)
    for p in PERMS3[1:]:
        decode_into(blob, want, typed(permuted_base(S3, p), dtype, offset=1), rng, "permutation %s" % (p,))
    a, b, c = S3
    decode_into(blob, want, View.whole(dtype, (2 * a, b, 3 * c)).sliced(slice(None, None, 2), slice(None), slice(None, None, 3)), rng, "steps 2, 1, 3")
    decode_into(blob, want, View.whole(dtype, (3 * a, 2 * b, c + 1)).sliced(slice(2, None, 3), slice(1, None, 2), slice(1, None)), rng, "steps 3, 2, 1")
    decode_into(blob, want, View.whole(dtype, (a, 3 * b, 2 * c), offset=1).sliced(slice(None), slice(None, None, 3), slice(None, None, 2)), rng, "steps 1, 3, 2")


@pytest.mark.parametrize("algo", [sz3_amd.ALGO_LORENZO_REG, sz3_amd.ALGO_LOSSLESS], ids=["lorenzo", "lossless"])
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_scatter_rectangles_in_wide_units(dtype, algo):
    """rows, offset and strides in whole 16-byte units, in whole 8-byte units, and the first rectangle moved by one element. A float array is
    copied into its view, and so is an integer array that was stored lossless: those launches take the wide forms (view_model.unit_form; the
    library's dense buffer comes from hipMalloc, aligned beyond 16 bytes). A lossy integer stream is narrowed from f64: element-wide."""
    rng = np.random.default_rng(12)
    es = np.dtype(dtype).itemsize
    copied = dtype in FLOATS or algo == sz3_amd.ALGO_LOSSLESS
    for shape in ((6, 10, 32), (70, 32), (3, 64)):
        blob, want = stream_of(dtype, shape, algo)
        for unit in (16, 8):
            v = rect(dtype, shape, unit)
            alloc = decode_into(blob, want, v, rng, "%d-byte units, %s" % (unit, shape))
            if copied:
                form = M.unit_form(v.dropped(), alloc.addr(v), 0, es)
                assert form == (unit if es < unit else M.ELEMENT), (unit, form)
        v = rect(dtype, shape, 16)
        v = v._replace(offset=v.offset + 1)
        alloc = decode_into(blob, want, v, rng, "16-byte units moved by one element, %s" % (shape,))
        assert M.unit_form(v.dropped(), alloc.addr(v), 0, es) == M.ELEMENT


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_scatter_inner_extents(dtype):
    rng = np.random.default_rng(13)
    for inner in M.INNERS:
        for rows in ROWS:
            blob, want = stream_of(dtype, (rows, inner))
            v = View.whole(dtype, (rows + 1, inner + 5)).sliced(slice(1, None), slice(3, inner + 3))
            decode_into(blob, want, v, rng, "rows %d inner %d" % (rows, inner))


@pytest.mark.parametrize("dtype", ["float32", "float64", "int16", "uint64"])
def test_scatter_rank_4(dtype):
    rng = np.random.default_rng(14)
    shape = (4, 5, 7, 33)
    blob, want = stream_of(dtype, shape)
    decode_into(blob, want, View.whole(dtype, (6, 5, 14, 40)).sliced(slice(1, 5), slice(None), slice(None, None, 2), slice(3, 36)), rng, "sub-box with a step")
    decode_into(blob, want, typed(permuted_base(shape, (2, 0, 3, 1)), dtype), rng, "permuted")
    decode_into(blob, want, View.whole(dtype, (4, 5, 7, 33, 3)).field(1), rng, "one field of interleaved records")


# =============================================================================================================================================
# integer edges in strided views
# =============================================================================================================================================
def as_ints(a):
    return [int(x) for x in np.asarray(a).reshape(-1)]


@pytest.mark.parametrize("dtype", M.INT_TYPES)
def test_integer_ends_through_strided_views(dtype):
    """runs at the type's minimum and maximum under a bound of 2.5: the reconstruction of an end may leave the type's range, and the narrowing
    into the view clamps it. Compressed from a stepped view, decoded into a permuted one: the host API's container, the host API's values,
    |x - x^| <= floor(eb), dtype kept."""
    info = np.iinfo(dtype)
    shape = (20, 37)
    a = data_for(shape, dtype)
    a[3, :] = info.min
    a[7, 5:30] = info.max
    a[12, ::2] = info.max
    a[12, 1::2] = info.min
    a[19, 36] = info.max
    a[0, 0] = info.min
    src = View.whole(dtype, (40, 3 * 37 + 1), offset=1).sliced(slice(None, None, 2), slice(1, None, 3))
    base = np.zeros(span(src), dtype=dtype)
    M.view_of(base, src)[...] = a
    alloc = Alloc.of(base)
    conf = conf_for(shape, dtype, eb=2.5)
    blob = sz3_amd.compress(alloc.tensor(src), conf)[0].tobytes()
    assert blob == host_container(a, conf_for(shape, dtype, eb=2.5)), "the container of the strided view is not the host API's"
    assert alloc.unchanged()
    want, _ = sz3_amd.decompress(blob, np.dtype(dtype))
    assert want.dtype == np.dtype(dtype) and max(abs(x - y) for x, y in zip(as_ints(want), as_ints(a))) <= 2
    dst = typed(permuted_base(shape, (1, 0)), dtype, offset=3)
    decode_into(blob, want, dst, np.random.default_rng(21), "permuted")


BIG_SPOTS = {  # name -> (shape, position of the one value beyond 2^53)
    "first_element": ((120, 33), (0, 0)),
    "last_of_a_ragged_row": ((120, 33), (4, 32)),
    "second_pass_of_a_long_row": ((20, 300), (2, 299)),
    "packed_wave_row": ((800, 5), (27, 3)),
    "packed_wave_last_lane": ((800, 5), (611, 4)),
    "last_row": ((120, 33), (119, 17)),
    "last_element": ((70, 65), (69, 64)),
}


def strided_source(a, seed):
    """the array as a stepped sub-box at an odd offset of a base of random bytes"""
    r, c = a.shape
    v = View.whole(a.dtype.name, (2 * r + 1, c + 4), offset=1).sliced(slice(1, None, 2), slice(3, c + 3))
    host = np.random.default_rng(seed).integers(0, 256, span(v) * a.itemsize, dtype=np.uint8)
    M.view_of(host, v)[...] = a
    return Alloc(host), v


@pytest.mark.parametrize("spot", sorted(BIG_SPOTS))
@pytest.mark.parametrize("dtype", ["int64", "uint64"])
def test_one_value_beyond_2_53(dtype, spot):
    """the flag travels from any lane of the walker: whichever element lies beyond 2^53, the container is the host API's — lossless, which
    the same field without that value is not — and the decode into a view is exact"""
    shape, pos = BIG_SPOTS[spot]
    a = data_for(shape, dtype)
    _, c0 = sz3_amd.decompress(host_container(a, conf_for(shape, dtype)), np.dtype(dtype))
    assert c0.cmprAlgo != sz3_amd.ALGO_LOSSLESS, "the premise: this field without the value is a lossy stream"
    a[pos] = (1 << 53) + 1
    alloc, v = strided_source(a, 31)
    conf = conf_for(shape, dtype)
    blob = sz3_amd.compress(alloc.tensor(v), conf)[0].tobytes()
    assert blob == host_container(a, conf_for(shape, dtype))
    assert alloc.unchanged()
    want, c2 = sz3_amd.decompress(blob, np.dtype(dtype))
    assert c2.cmprAlgo == sz3_amd.ALGO_LOSSLESS and same_bytes(want, a)
    decode_into(blob, want, typed(permuted_base(shape, (1, 0)), dtype, offset=1), np.random.default_rng(32), spot)
    if dtype == "int64":
        a[pos] = -(1 << 53) - 1
        alloc, v = strided_source(a, 33)
        blob = sz3_amd.compress(alloc.tensor(v), conf_for(shape, dtype))[0].tobytes()
        want, c2 = sz3_amd.decompress(blob, np.dtype(dtype))
        assert c2.cmprAlgo == sz3_amd.ALGO_LOSSLESS and same_bytes(want, a) and blob == host_container(a, conf_for(shape, dtype))


@pytest.mark.parametrize("dtype,value", [("int64", 1 << 53), ("int64", -(1 << 53)), ("uint64", 1 << 53)])
def test_exactly_2_53_does_not_raise_the_flag(dtype, value):
    """strictly beyond: an array whose largest magnitude is 2^53 itself stays lossy (and the same array with that value one further out
    does not)"""
    shape = (64, 100)
    a = data_for(shape, dtype)
    alloc, v = strided_source(a, 41)
    _, c0 = sz3_amd.decompress(sz3_amd.compress(alloc.tensor(v), conf_for(shape, dtype))[0], np.dtype(dtype))
    assert c0.cmprAlgo != sz3_amd.ALGO_LOSSLESS, "the premise: this field without the value is a lossy stream"
    a[33, 77] = value
    alloc, v = strided_source(a, 42)
    blob = sz3_amd.compress(alloc.tensor(v), conf_for(shape, dtype))[0].tobytes()
    assert blob == host_container(a, conf_for(shape, dtype))
    want, c1 = sz3_amd.decompress(blob, np.dtype(dtype))
    assert c1.cmprAlgo != sz3_amd.ALGO_LOSSLESS, "a value of exactly %d raised the 2^53 flag" % value
    assert max(abs(x - y) for x, y in zip(as_ints(want), as_ints(a))) <= 1
    a[33, 77] = value + (1 if value > 0 else -1)
    alloc, v = strided_source(a, 43)
    _, c2 = sz3_amd.decompress(sz3_amd.compress(alloc.tensor(v), conf_for(shape, dtype))[0], np.dtype(dtype))
    assert c2.cmprAlgo == sz3_amd.ALGO_LOSSLESS


# =============================================================================================================================================
# the narrowing alone: sz3hip_debug_scatter of prescribed doubles
# =============================================================================================================================================
@pytest.mark.parametrize("dtype", M.INT_TYPES)
def test_narrowing_of_prescribed_doubles(dtype):
    """ties, both ends of the type with their neighbours, signed zeros, NaN and the infinities, narrowed into a contiguous array, a stepped
    row, packed rows of 5 and a permuted view: view_model.narrow, element for element, and no other byte of the allocation written"""
    probe = M.narrowing_probe(dtype)
    rng = np.random.default_rng(51)
    n = 5 * 33
    v = np.concatenate([probe, rng.choice(probe, n - probe.size)])  # (every prescribed value once, then drawn repeats up to 5 rows of 33)
    assert v.size == n
    vd = torch.from_numpy(v).to(DEV)
    views = [View.whole(dtype, (n,), offset=1), View.whole(dtype, (3 * n,)).sliced(slice(1, None, 3)),
             View.whole(dtype, (33, 9), offset=1).sliced(slice(None), slice(2, 7)), typed(permuted_base((5, 33), (1, 0)), dtype),
             View.whole(dtype, (5, 40)).sliced(slice(None), slice(4, 37))]
    for view in views:
        alloc = Alloc.random(dtype, span(view), rng)
        sz3_amd._check(scatter_rc(vd, alloc, view))
        got, exp = alloc.now(), M.expected_after_scatter(alloc.host, view, M.narrow(v, dtype))
        assert np.array_equal(got, exp), "narrowing into %s: %s" % ((view,), first_difference(got, exp, view))


@pytest.mark.parametrize("dtype", FLOATS)
def test_scatter_hook_copies_floats(dtype):
    rng = np.random.default_rng(52)
    view = rect(dtype, (7, 32), 16)
    vals = rng.integers(0, 256, view.numel * np.dtype(dtype).itemsize, dtype=np.uint8).view(dtype)  # (any bit pattern, NaNs included)
    alloc = Alloc.random(dtype, span(view), rng)
    sz3_amd._check(scatter_rc(torch.from_numpy(vals.copy()).to(DEV), alloc, view))
    assert np.array_equal(alloc.now(), M.expected_after_scatter(alloc.host, view, vals))


# =============================================================================================================================================
# refusals, all before any launch
# =============================================================================================================================================
def last_error():
    return L.sz3hip_last_error().decode()


def test_negative_strides_are_refused():
    rng = np.random.default_rng(61)
    shape = (8, 12)
    alloc = Alloc.random("float32", 8 * 12 * 2, rng)
    mid = alloc.dev.data_ptr() + 4 * 96  # (the middle of the allocation: the refused view would lie inside it)
    conf = conf_for(shape, "float32")
    blob, _ = stream_of("float32", shape)
    blob = np.frombuffer(blob, dtype=np.uint8)
    out = np.empty(sz3_amd.compress_bound(conf, np.float32), dtype=np.uint8)
    dense = torch.zeros(96, dtype=torch.float32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    dims = (C.c_uint64 * 2)(*shape)
    for strides in ((-12, 1), (12, -1)):
        st = (C.c_int64 * 2)(*strides)
        assert L.sz3hip_compress_from_device(C.byref(conf._c), 0, mid, st, out.ctypes.data, out.size, s) == 0
        assert L.sz3hip_last_error_code() == EINVAL and "negative" in last_error()
        c2 = sz3_amd.Config(1)
        assert L.sz3hip_decompress_to_device(C.byref(c2._c), 0, blob.ctypes.data, blob.size, mid, st, s) == EINVAL and "negative" in last_error()
        assert L.sz3hip_debug_gather(0, mid, 2, dims, st, dense.data_ptr(), s) == EINVAL and "negative" in last_error()
        assert L.sz3hip_debug_scatter(0, dense.data_ptr(), 2, dims, st, mid, s) == EINVAL and "negative" in last_error()
    assert alloc.unchanged() and float(dense.abs().sum()) == 0.0


OVERLAPS = {  # name -> the output view of extents (8, 12)
    "expand_slowest": View.whole("float32", (1, 12)).expanded(0, 8),
    "expand_fastest": View.whole("float32", (8, 1)).expanded(1, 12),
    "windows_every_5": View("float32", 1, (8, 12), (5, 1)),
    "windows_transposed": View("float32", 0, (8, 12), (1, 3)),
    "rows_one_short": View("float32", 2, (8, 12), (11, 1)),
}


@pytest.mark.parametrize("name", sorted(OVERLAPS))
def test_overlapping_outputs_are_refused(name):
    view = OVERLAPS[name]
    assert M.dev_view_rule(view.shape, view.strides, True) == M.OVERLAP and len(set(M.touched_offsets(view.shape, view.strides))) < view.numel
    blob, _ = stream_of("float32", (8, 12))
    alloc = Alloc.random("float32", span(view), np.random.default_rng(62))
    with pytest.raises(sz3_amd.SZ3HipError) as e:
        sz3_amd.decompress(blob, np.float32, out=alloc.tensor(view))
    assert e.value.code == EINVAL and "the output strides make elements overlap" in str(e.value)
    dense = torch.ones(view.numel, dtype=torch.float32, device=DEV)
    assert scatter_rc(dense, alloc, view) == EINVAL and "the output strides make elements overlap" in last_error()
    assert alloc.unchanged(), "a refused output was written"


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_stride_0_input_is_accepted(axis):
    """a broadcast axis is an input like any other: the container is the host API's for the expanded array"""
    shape = [18, 24, 40]
    shape[axis] = 1
    small = data_for(tuple(shape), "float32")
    alloc = Alloc.of(small)
    view = View.whole("float32", shape).expanded(axis, 21)
    a = np.ascontiguousarray(M.view_of(alloc.host, view))
    assert a.shape[axis] == 21 and view.strides[axis] == 0
    conf = conf_for(a.shape, "float32")
    assert sz3_amd.compress(alloc.tensor(view), conf)[0].tobytes() == host_container(a, conf_for(a.shape, "float32"))
    assert alloc.unchanged()
    check_gather(alloc, view, "stride 0 on axis %d" % axis)


# =============================================================================================================================================
# routes over strided views: conf.openmp slabs, pipelined pieces
# =============================================================================================================================================
def route_views(kind, rows):
    """-> (dtype, the input view of `rows` rows, the output view)"""
    if kind == "subbox":
        src = View.whole("float32", (rows + 3, 30, 44)).sliced(slice(2, rows + 2), slice(3, 27), slice(4, 41))
        return "float32", src, typed(permuted_base(src.shape, (2, 0, 1)), "float32", offset=1)
    if kind == "permuted":
        src = typed(permuted_base((rows, 24, 37), (1, 2, 0)), "float32")
        return "float32", src, View.whole("float32", (rows, 2 * 24, 3 * 37)).sliced(slice(None), slice(None, None, 2), slice(None, None, 3))
    src = View.whole("int16", (rows + 2, 2 * 24, 45)).sliced(slice(1, rows + 1), slice(None, None, 2), slice(5, 42))
    return "int16", src, typed(permuted_base(src.shape, (1, 0, 2)), "int16", offset=1)


def check_route(kind, rows, conf_kw):
    dtype, src, dst = route_views(kind, rows)
    a = data_for(src.shape, dtype)
    host = Alloc.random(dtype, span(src), np.random.default_rng(71)).host
    M.view_of(host, src)[...] = a
    alloc = Alloc(host)
    blob = sz3_amd.compress(alloc.tensor(src), conf_for(src.shape, dtype, **conf_kw))[0].tobytes()
    assert blob == host_container(a, conf_for(src.shape, dtype, **conf_kw)), "the container of the strided view is not the host API's for its contiguous copy"
    assert alloc.unchanged()
    want, c2 = sz3_amd.decompress(blob, np.dtype(dtype))
    assert c2.openmp == 1, "the route was not taken"
    decode_into(blob, want, dst, np.random.default_rng(72), kind)


@pytest.mark.parametrize("kind", ["subbox", "permuted", "int16_stepped"])
def test_openmp_slabs_over_strided_views(kind, monkeypatch):
    """50 rows over 3 slabs: the bounds 16 and 33 are multiples of nothing; each slab's base is the view's plus lo * stride[0]"""
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    check_route(kind, 50, dict(openmp=1))


@pytest.mark.parametrize("kind", ["subbox", "permuted", "int16_stepped"])
def test_pieces_over_strided_views(kind, monkeypatch):
    """three pieces need 32 planes each: 100 rows, cut at 33 and 66"""
    monkeypatch.setenv("SZ3HIP_PIECES", "3")
    check_route(kind, 100, dict(regression=0))


# =============================================================================================================================================
# the coarse call into strided outputs
# =============================================================================================================================================
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("algo", [sz3_amd.ALGO_INTERP, sz3_amd.ALGO_LORENZO_REG], ids=["interp_fast_path", "lorenzo_fallback"])
@pytest.mark.parametrize("dtype", FLOATS)
def test_coarse_into_strided_outputs(dtype, algo, level):
    """every 2^level-th point into a stepped and into a permuted output: decompress(...)[::2^k, ...], every other byte of the allocation
    unchanged. The interpolation stream takes the fast path through the strided scatter, the Lorenzo container the full decode and then the
    gather whose strides are multiplied by 2^level."""
    shape = (37, 45, 50)
    blob, want = stream_of(dtype, shape, algo)
    st = 1 << level
    coarse = np.ascontiguousarray(want[::st, ::st, ::st])
    cs = coarse.shape
    rng = np.random.default_rng(81)
    outs = [View.whole(dtype, (2 * cs[0], cs[1] + 2, 3 * cs[2]), offset=1).sliced(slice(None, None, 2), slice(1, cs[1] + 1), slice(None, None, 3)),
            typed(permuted_base(cs, (2, 0, 1)), dtype), typed(permuted_base(cs, (1, 0, 2)), dtype, offset=1)]
    for view in outs:
        alloc = Alloc.random(dtype, span(view), rng)
        sz3_amd.decompress_coarse(blob, np.dtype(dtype), level, out=alloc.tensor(view))
        got, exp = alloc.now(), M.expected_after_scatter(alloc.host, view, coarse)
        assert np.array_equal(got, exp), "coarse level %d into %s: %s" % (level, (view,), first_difference(got, exp, view))

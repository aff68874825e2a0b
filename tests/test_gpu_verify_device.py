"""sz3hip_verify_device on the MI355X: the error statistics of two arrays in device memory against a numpy model of the kernel's rules
(sz3_amd/csrc/sz3hip_verify.hip). Extremes, maxima, indices and counts do not depend on the summation order and are compared for
equality; the four sums against math.fsum of the exact terms with the bound any f64 summation order obeys; acEff against the two-pass
value in np.longdouble."""
import math
import os
import subprocess
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = "cuda:0"
INT_TYPES = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64"]
ALL_TYPES = ["float32", "float64"] + INT_TYPES
U = 2.0 ** -53


def field(shape, dtype="float32", seed=0):  # (tests/test_gpu_device_container.py's generator)
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = np.linspace(0, 6.0, n)
    a = np.sin(x) * 10 + np.cumsum(rng.standard_normal(n)) * 0.05
    if dtype in INT_TYPES:
        info = np.iinfo(dtype)
        a = np.clip(np.round(a * 7), info.min, info.max)
    return a.reshape(shape).astype(dtype)


def field_offset(shape, seed=0):
    """the same field 1000 above zero, in f64: the one-pass second moments must not lose it to cancellation"""
    return field(shape, "float64", seed) + 1000.0


def noisy(a, seed=1, amp=1e-3):
    rng = np.random.default_rng(seed)
    if a.dtype.kind == "f":
        return (a.astype(np.float64) + rng.uniform(-amp, amp, a.shape)).astype(a.dtype)
    info = np.iinfo(a.dtype)
    return np.clip(a.astype(np.float64) + rng.integers(-2, 3, a.shape), info.min, info.max).astype(a.dtype)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return np.ascontiguousarray(t.cpu().numpy())


# ---- the model ---------------------------------------------------------------------------------------------------
def model(o, d, bound=None):
    """the rules of sz3hip_verify.hip on two host arrays of the same shape; indices are row-major ones"""
    o = np.ascontiguousarray(o).ravel()
    d = np.ascontiguousarray(d).ravel()
    n = o.size
    a = o.astype(np.float64)
    b = d.astype(np.float64)
    if o.dtype.kind == "f":
        fin = np.isfinite(a) & np.isfinite(b)
        with np.errstate(invalid="ignore"):
            e = np.abs(b - a)
            same = (np.isnan(a) & np.isnan(b)) | (a == b)
        mismatch = int(np.count_nonzero(~fin & ~same))
    else:
        fin = np.ones(n, bool)
        mismatch = 0
        if o.dtype.itemsize == 8:  # exact magnitudes in Python integers, then the nearest double
            e = np.array([float(abs(int(x) - int(y))) for x, y in zip(o, d)], dtype=np.float64)
        else:
            e = np.abs(o.astype(np.int64) - d.astype(np.int64)).astype(np.float64)
    idx = np.flatnonzero(fin)
    af, bf, ef = a[idx], b[idx], e[idx]
    m = idx.size
    r = dict(n=n, n_nonfinite=n - m, n_nonfinite_mismatch=mismatch)
    if m:
        r.update(min=float(af.min()), max=float(af.max()), max_diff=float(ef.max()), argmax=int(idx[np.argmax(ef)]))
        nz = af != 0
        r["max_pw_rel"] = float((ef[nz] / np.abs(af[nz])).max()) if nz.any() else 0.0
    else:
        r.update(min=float("nan"), max=float("nan"), max_diff=0.0, argmax=n, max_pw_rel=0.0)
    over = ef > bound if bound is not None and bound >= 0 else np.zeros(m, bool)
    r["n_over"] = int(np.count_nonzero(over))
    r["first_over"] = int(idx[np.argmax(over)]) if over.any() else n
    r["terms"] = dict(sum_ori=af, sum_dec=bf, sum_sq_err=ef * ef, sum_sq_dec=bf * bf)
    r["a"], r["b"] = af, bf
    return r


def same_value(x, y, rel=0.0):
    if math.isnan(x) or math.isnan(y):
        return math.isnan(x) and math.isnan(y)
    if math.isinf(x) or math.isinf(y):
        return x == y
    return abs(x - y) <= rel * max(abs(x), abs(y))


def derived(st):
    """section 2's formulas from the struct's own sums, in IEEE double (numpy scalars: a division by zero is inf or nan, not an exception)"""
    with np.errstate(all="ignore"):
        m = np.float64(st.n - st.n_nonfinite)
        mse = np.float64(st.sum_sq_err) / m
        rng = np.float64(st.max) - np.float64(st.min)
        l2 = np.sqrt(np.float64(st.sum_sq_err))
        return dict(psnr=float(20 * np.log10(rng) - 10 * np.log10(mse)), nrmse=float(np.sqrt(mse) / rng), l2_err=float(l2),
                    l2_err_norm=float(l2 / np.sqrt(np.float64(st.sum_sq_dec))))


def aceff_truth(a, b):
    """-> (two-pass Pearson coefficient in long double, tolerance 8 n 2^-53 kappa) or None when ori has no variance (undefined)"""
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    ma, mb = al.mean(), bl.mean()
    va, vb, cab = ((al - ma) ** 2).sum(), ((bl - mb) ** 2).sum(), ((al - ma) * (bl - mb)).sum()
    if va == 0 or vb == 0:
        return None
    K = np.longdouble(a[0])  # the first finite element of ori's view
    kappa = float(1 + (ma - K) ** 2 / (va / a.size))
    tol = 8 * a.size * U * kappa
    assert tol < 1e-6, "the input makes the acEff tolerance loose (%g)" % tol
    return float(cab / np.sqrt(va * vb)), tol


def check(to, td, bound=None, stream=None, truth=None):
    """verify_stats of two device tensors against the model on their contiguous host copies; returns the stats"""
    st = sz3_amd.verify_stats(to, td, bound=bound, stream=stream)
    ho, hd = truth if truth is not None else (host(to), host(td))
    r = model(ho, hd, bound)
    for k in ("n", "n_nonfinite", "n_nonfinite_mismatch", "n_over", "first_over", "argmax"):
        assert st[k] == r[k], (k, st[k], r[k])
    for k in ("min", "max", "max_diff", "max_pw_rel"):
        assert same_value(st[k], r[k]), (k, st[k], r[k])
    for k, t in r["terms"].items():
        m = t.size
        exact = math.fsum(t)
        lim = m * U * math.fsum(np.abs(t)) / (1 - m * U)
        print("%s: device %.17g, fsum %.17g, |difference| %.3g, bound %.3g" % (k, st[k], exact, abs(st[k] - exact), lim))
        assert abs(st[k] - exact) <= lim, (k, st[k], exact, lim)
    for k, v in derived(st).items():
        assert same_value(st[k], v, 1e-14), (k, st[k], v)
    if r["a"].size:
        ac = aceff_truth(r["a"], r["b"])
        if ac is not None:
            print("acEff: device %.17g, two-pass %.17g, |difference| %.3g, tolerance %.3g" % (st.acEff, ac[0], abs(st.acEff - ac[0]), ac[1]))
            assert abs(st.acEff - ac[0]) <= ac[1], (st.acEff, ac)
    return st


# ---- lengths, misaligned bases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097, (1 << 20) + 3])
def test_lengths_f32(n):
    a = field((n,))
    check(dev(a), dev(noisy(a)), bound=5e-4)


@pytest.mark.parametrize("n", [4097, (1 << 20) + 3])
def test_lengths_f64_offset(n):
    a = field_offset((n,))
    check(dev(a), dev(noisy(a)), bound=5e-4)


@pytest.mark.parametrize("cut", [1, 3])
def test_base_misalignment(cut):
    a = field((4097,))
    to, td = dev(a)[cut:], dev(noisy(a))[cut:]
    assert to.data_ptr() % 16 != 0 and td.data_ptr() % 16 != 0
    check(to, td, bound=5e-4)


def test_bases_misaligned_differently():
    a = field((4097,))
    to, td = dev(a)[1:-2], dev(noisy(a))[3:]
    assert to.data_ptr() % 16 != td.data_ptr() % 16
    check(to, td, bound=5e-4)


@pytest.mark.parametrize("dtype", ["float64", "int16", "uint8"])
def test_base_misalignment_other_widths(dtype):
    a = field((4099,), dtype)
    check(dev(a)[1:], dev(noisy(a))[1:], bound=1.0 if dtype != "float64" else 5e-4)


# ---- strided views -------------------------------------------------------------------------------------------------
def strided_pair(kind):
    if kind == "subbox_2d":  # rows of 19: packed three to a wave
        big = dev(field((40, 32)))
        o = big[1:38, 2:21]
        return o, dev(noisy(host(o)))
    if kind == "rows_of_5":
        big = dev(field((300, 8)))
        o = big[:, 1:6]
        return o, dev(noisy(host(o)))
    if kind == "subbox_3d":
        big = dev(field((9, 12, 70)))
        o = big[1:8, 2:11, 3:68]
        return o, dev(noisy(host(o)))
    if kind == "view_4d":
        big = dev(field((4, 5, 6, 40)))
        o = big[1:, 1:, 1:, 2:35]
        assert tuple(o.shape) == (3, 4, 5, 33)
        return o, dev(noisy(host(o)))
    if kind == "transposed":
        o = dev(field((45, 70))).t()
        return o, dev(noisy(host(o)))
    if kind == "both_strided":
        o = dev(field((50, 80)))[3:43, 5:75]
        d = dev(noisy(host(o)).T.copy()).t()  # the same values, column-major
        return o, d
    if kind == "broadcast":
        o = dev(field((1, 300))).expand(7, 300)
        d = dev(noisy(host(o)))
        return o, d
    if kind == "interleaved":  # field 1 of a 4-way interleaved array
        big = dev(field((30, 40, 4)))
        o = big[..., 1]
        return o, dev(noisy(host(o)))
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["subbox_2d", "rows_of_5", "subbox_3d", "view_4d", "transposed", "both_strided", "broadcast", "interleaved"])
def test_strided_views(kind):
    o, d = strided_pair(kind)
    assert not o.is_contiguous()
    st = check(o, d, bound=5e-4)
    assert st.n == o.numel()


def test_size_one_dimensions_are_dropped():
    a = field((3, 1, 5, 1, 7, 1, 4))
    st = check(dev(a), dev(noisy(a)))
    assert st.n == a.size
    t = dev(field((2, 2, 2, 2, 2)))
    with pytest.raises(ValueError, match="at most 4"):
        sz3_amd.verify_stats(t, t)


# ---- the ten element types -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_all_types(dtype):
    shape = (37, 19)
    a = field(shape, dtype)
    b = noisy(a)
    if dtype in INT_TYPES:
        info = np.iinfo(dtype)
        a[5, 7], b[5, 7] = info.max, info.min  # the widest difference of the type
        a[30, 2], b[30, 2] = info.min, info.max
    st = check(dev(a), dev(b), bound=1.0, truth=(a, b))
    if dtype in INT_TYPES:
        info = np.iinfo(dtype)
        assert st.max_diff == float(info.max - info.min) and st.argmax == 5 * 19 + 7


@pytest.mark.parametrize("dtype", ["int64", "uint64"])
def test_64_bit_pairs_beyond_2_53_differ_by_exactly_one(dtype):
    a = np.zeros((37, 19), dtype)
    b = a.copy()
    a[3, 4], b[3, 4] = (1 << 60) + 7, (1 << 60) + 8
    a[20, 0], b[20, 0] = (1 << 53) + 3, (1 << 53) + 2
    if dtype == "uint64":
        a[36, 18], b[36, 18] = (1 << 63) + 5, (1 << 63) + 4
    else:
        a[36, 18], b[36, 18] = -(1 << 62) - 1, -(1 << 62) - 2
    st = check(dev(a), dev(b), bound=0.5, truth=(a, b))
    assert st.max_diff == 1.0 and st.argmax == 3 * 19 + 4 and st.n_over == 3 and st.first_over == 3 * 19 + 4


# ---- indices ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, where", [(4097, [0]), (4097, [4096]), (4102, [4101]), (70000, [1234, 60001]), (70000, [60001, 99]), (300, [299, 7])])
def test_planted_maximum(n, where):
    """one planted error at index 0, at n - 1, inside the scalar tail; two equal maxima report the smaller index"""
    a = field((n,))
    b = a.copy()
    for i in where:
        a[i], b[i] = 1.25, 1.75  # (exactly 0.5 apart, every time)
    st = check(dev(a), dev(b), bound=0.25)
    assert st.max_diff == 0.5 and st.argmax == st.first_over == min(where) and st.n_over == len(where)


def test_index_in_a_strided_view_is_row_major_over_the_view():
    big = field((40, 32))
    big[1 + 17, 2 + 11] = big[1 + 30, 2 + 3] = 2.0
    d = np.ascontiguousarray(big[1:38, 2:21]).copy()
    d[17, 11] = d[30, 3] = 2.75  # two equal maxima
    o = dev(big)[1:38, 2:21]
    st = check(o, dev(d), bound=0.1)
    assert st.max_diff == 0.75 and st.argmax == st.first_over == 17 * 19 + 11 and st.n_over == 2
    st = check(o.t(), dev(d).t(), bound=0.1)  # the transposed views: the index runs over (19, 37)
    assert st.argmax == st.first_over == 3 * 37 + 30 and st.n_over == 2


# ---- bound -----------------------------------------------------------------------------------------------------------
def test_bound_is_strict():
    n = 5000
    a = np.round(field((n,), "float64") * 8) / 8  # multiples of 1/8: the planted differences are exact in f64
    b = a.copy()
    bound = 0.25
    planted = [4999, 77, 2048, 640]
    for i in planted:
        b[i] = a[i] + 0.375
    b[5] = a[5] + bound  # exactly the bound: not above it
    b[4000] = a[4000] - bound
    st = check(dev(a), dev(b), bound=bound)
    assert st.n_over == len(planted) and st.first_over == 77 and st.max_diff == 0.375
    st = check(dev(a), dev(b), bound=None)
    assert st.n_over == 0 and st.first_over == n
    for none in (-1.0, float("nan")):
        st = sz3_amd.verify_stats(dev(a), dev(b), bound=none)
        assert st.n_over == 0 and st.first_over == n


# ---- positions that are not finite -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_nonfinite_at_the_same_places(dtype):
    a = field((3001,), dtype)
    b = noisy(a)
    for i, v in [(0, np.nan), (64, np.inf), (1500, -np.inf), (3000, np.nan), (2999, np.inf)]:
        a[i] = b[i] = v
    st = check(dev(a), dev(b), bound=5e-4)
    assert st.n_nonfinite == 5 and st.n_nonfinite_mismatch == 0 and math.isfinite(st.psnr)


def test_nonfinite_mismatches():
    a = field((3001,))
    b = noisy(a)
    a[10] = np.nan            # NaN against a number
    b[20] = np.nan            # a number against NaN
    a[30], b[30] = np.inf, -np.inf
    a[40] = np.inf            # an infinity against a number
    a[50], b[50] = np.nan, np.inf
    a[60] = b[60] = np.inf    # the same infinity: no mismatch
    a[70] = b[70] = np.nan    # NaN with NaN: no mismatch
    st = check(dev(a), dev(b))
    assert st.n_nonfinite == 7 and st.n_nonfinite_mismatch == 5


def test_all_nan_ori():
    a = np.full((1000,), np.nan, np.float32)
    b = field((1000,))
    st = check(dev(a), dev(b), bound=1.0)
    assert st.n_nonfinite == 1000 and st.n_nonfinite_mismatch == 1000 and st.n_over == 0 and st.max_diff == 0.0 and st.argmax == 1000
    st = check(dev(a), dev(a))
    assert st.n_nonfinite == 1000 and st.n_nonfinite_mismatch == 0


# ---- degenerate inputs ---------------------------------------------------------------------------------------------------
def test_identical_arrays():
    a = field((37, 19, 11))
    t = dev(a)
    st = check(t, t.clone(), bound=0.0)
    assert st.max_diff == 0.0 and st.psnr == float("inf") and st.nrmse == 0.0 and st.n_over == 0 and st.argmax == 0
    assert abs(st.acEff - 1.0) <= aceff_truth(a.ravel().astype(np.float64), a.ravel().astype(np.float64))[1]
    assert sz3_amd.verify(t, t) == (0.0, float("inf"), 0.0)


def test_constant_ori():
    a = np.full((50, 60), 3.0, np.float32)
    b = a + field((50, 60)) * np.float32(0.01)
    to, td = dev(a), dev(b)
    check(to, td)
    got = sz3_amd.verify(to, td)
    want = sz3_amd.verify(a, b)
    assert got[0] == want[0] and got[1:] == want[1:] == (float("inf"), 0.0)


# ---- sz3_amd.verify on tensors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, dtype", [((64, 64, 64), "float32"), ((1 << 20,), "float32"), ((100, 333), "float64")])
def test_verify_on_tensors_equals_verify_on_host_copies(shape, dtype):
    a = field(shape, dtype)
    to, td = dev(a), dev(noisy(a))
    got = sz3_amd.verify(to, td)
    want = sz3_amd.verify(to.cpu().numpy(), td.cpu().numpy())
    print("tensors", got, "host copies", want)
    assert got[0] == want[0]
    assert abs(got[1] - want[1]) <= 1e-9 * abs(want[1])
    assert abs(got[2] - want[2]) <= 1e-9 * abs(want[2])


def test_python_face_refusals():
    t = dev(field((8, 8)))
    with pytest.raises(TypeError):
        sz3_amd.verify_stats(t.cpu().numpy(), t)
    with pytest.raises(ValueError, match="HIP device"):
        sz3_amd.verify_stats(t, t.cpu())
    with pytest.raises(ValueError, match="shapes"):
        sz3_amd.verify_stats(t, t[:4])
    with pytest.raises(TypeError, match="dtypes"):
        sz3_amd.verify_stats(t, t.double())
    with pytest.raises(TypeError, match="float32 / float64"):
        sz3_amd.verify_stats(t.half(), t.half())
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="different devices"):
            sz3_amd.verify_stats(t, t.to("cuda:1"))


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _conf(shape, algo, mode, eb, rel=1e-3):
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = algo
    c.errorBoundMode = mode
    c.absErrorBound = eb
    c.relErrorBound = rel
    return c


@pytest.mark.parametrize("case", ["lorenzo_abs", "default_rel", "int32"])
def test_end_to_end(case):
    shape = (64, 64, 64)
    if case == "int32":
        t = dev(field(shape, "int32"))
        conf = _conf(shape, sz3_amd.ALGO_LORENZO_REG, sz3_amd.EB_ABS, 2.0)
    else:
        t = dev(field(shape))
        conf = (_conf(shape, sz3_amd.ALGO_LORENZO_REG, sz3_amd.EB_ABS, 1e-3) if case == "lorenzo_abs" else
                _conf(shape, sz3_amd.ALGO_INTERP_LORENZO, sz3_amd.EB_REL, 1e-3))
    blob, _ = sz3_amd.compress(t, conf)
    dec, conf2 = sz3_amd.decompress(blob, t.dtype, device=DEV)
    st = check(t, dec.reshape(shape), bound=conf2.absErrorBound)
    print(case, "bound", conf2.absErrorBound, "max_diff", st.max_diff, "psnr", st.psnr)
    assert st.n_over == 0 and st.first_over == st.n and st.max_diff <= conf2.absErrorBound


# ---- stream ordering, threads ------------------------------------------------------------------------------------------------
def test_stream_ordering():
    """the producer is still at work on its stream when the call is made: the library waits for it on the device, not the host"""
    a = field((64, 128, 128))
    b = noisy(a)
    src, td = dev(a), dev(b)
    x = torch.randn((4096, 4096), device=DEV)
    side = torch.cuda.Stream(device=DEV)
    t = torch.zeros_like(src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(6):
            x = torch.matmul(x, x) * 1e-2
        t.copy_(src)
        st = sz3_amd.verify_stats(t, td, bound=5e-4, stream=side)
    want = sz3_amd.verify_stats(src, td, bound=5e-4)
    assert st == want and st.max_diff > 0
    r = model(a, b, 5e-4)
    assert st.max_diff == r["max_diff"] and st.argmax == r["argmax"] and st.n_over == r["n_over"] and st.min == r["min"]


def test_threads():
    shapes = [(40, 50, 60), (1 << 18,), (300, 90), (7, 9, 11, 13)]
    pairs = []
    for i, s in enumerate(shapes):
        a = field(s, seed=i)
        b = noisy(a, seed=10 + i, amp=1e-3 * (i + 1))
        pairs.append((dev(a), dev(b)))
    torch.cuda.synchronize()
    want = [sz3_amd.verify_stats(o, d, bound=1e-3, stream=0) for o, d in pairs]
    assert len({w.max_diff for w in want}) == 4
    got = [None] * 4

    def run(i):
        for _ in range(5):
            got[i] = sz3_amd.verify_stats(pairs[i][0], pairs[i][1], bound=1e-3, stream=0)

    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert got == want


# ---- the C++ face -----------------------------------------------------------------------------------------------------------
CXX = r"""
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <vector>
#include "SZ3/api/sz.hpp"
int main(int argc, char **argv) {
    const size_t n = (size_t)atol(argv[3]);
    std::vector<float> o(n), d(n);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(o.data(), 4, n, f) != n) return 2;
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f || fread(d.data(), 4, n, f) != n) return 2;
    fclose(f);
    float *d_o = nullptr, *d_d = nullptr;
    if (hipMalloc((void **)&d_o, n * 4) != hipSuccess || hipMalloc((void **)&d_d, n * 4) != hipSuccess) return 3;
    if (hipMemcpy(d_o, o.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_d, d.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return 3;
    const sz3hip_verify_stats st = SZ3::hip_verify_device<float>(d_o, d_d, n, atof(argv[4]));
    printf("%.17g %llu %llu %.17g\n", st.max_diff, (unsigned long long)st.n_over, (unsigned long long)st.argmax, st.psnr);
    try {  // a host pointer: the face's exception, not a host loop
        SZ3::hip_verify_device<float>(o.data(), d_d, n);
        return 4;
    } catch (const std::invalid_argument &e) {
        printf("invalid_argument: %s\n", e.what());
    }
    (void)hipFree(d_o);
    (void)hipFree(d_d);
    return 0;
}
"""


def test_cxx_face(tmp_path):
    n = 10007
    a = field((n,))
    b = noisy(a)
    b[4321] = a[4321] + np.float32(0.5)
    a.tofile(tmp_path / "ori.f32")
    b.tofile(tmp_path / "dec.f32")
    src = tmp_path / "verify_face.cpp"
    src.write_text(CXX)
    exe = str(tmp_path / "verify_face")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe, "-L" + os.path.join(ROOT, "sz3_amd"), "-lsz3hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "sz3_amd"), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([exe, str(tmp_path / "ori.f32"), str(tmp_path / "dec.f32"), str(n), "5e-4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    max_diff, n_over, argmax, psnr = lines[0].split()
    want = model(a, b, 5e-4)
    assert float(max_diff) == want["max_diff"] and int(n_over) == want["n_over"] and int(argmax) == want["argmax"] == 4321
    assert abs(float(psnr) - sz3_amd.verify(a, b)[1]) <= 1e-9 * float(psnr)
    assert lines[1].startswith("invalid_argument") and "device memory" in lines[1]

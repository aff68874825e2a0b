"""sz3hip_compress_from_device / sz3hip_decompress_to_device on the MI355X: the container of a device array is, byte for byte, what
sz3hip_compress writes for its host copy; the array decoded into device memory is, bit for bit, what sz3hip_decompress writes."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sz3_amd  # noqa: E402

pytestmark = pytest.mark.gpu
L = sz3_amd.lib()
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
INT_TYPES = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64"]


def field(shape, dtype="float32", seed=0):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = np.linspace(0, 6.0, n)
    a = np.sin(x) * 10 + np.cumsum(rng.standard_normal(n)) * 0.05
    if dtype in INT_TYPES:
        info = np.iinfo(dtype)
        a = np.clip(np.round(a * 7), info.min, info.max)
    return a.reshape(shape).astype(dtype)


def conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, mode=sz3_amd.EB_ABS, eb=1e-3, rel=1e-3, **kw):
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = algo
    c.errorBoundMode = mode
    c.absErrorBound = eb
    c.relErrorBound = rel
    c.psnrErrorBound = 60.0
    c.l2normErrorBound = 1.0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def host_container(a, conf):
    return sz3_amd.compress(np.ascontiguousarray(a), conf)[0].tobytes()


def device_container(t, conf, stream=None):
    return sz3_amd.compress(t, conf, stream=stream)[0].tobytes()


def check_roundtrip(a, conf, dtype):
    """compression byte identity, then decompression bit identity: contiguous and into a sub-box of a sentinel-filled tensor"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    before = t.clone()
    hb = host_container(a, conf)
    db = device_container(t, conf)
    assert db == hb, "device container differs from the host API's (%d vs %d bytes)" % (len(db), len(hb))
    assert torch.equal(t, before), "the input tensor was written"
    check_decode(hb, dtype, a.shape)


def check_decode(blob, dtype, shape):
    host, _ = sz3_amd.decompress(blob, dtype)
    dev, _ = sz3_amd.decompress(blob, dtype, device=DEV)
    assert dev.device.type == "cuda" and sz3_amd._np_dtype(dev.dtype) == np.dtype(dtype)
    assert np.array_equal(dev.cpu().numpy().view(np.uint8), host.view(np.uint8)), "device decode differs from the host API's"
    # a sub-box of a larger tensor, its other elements untouched
    big_shape = tuple(int(d) + 3 for d in host.shape)
    sentinel = torch.full(big_shape, 77, dtype=dev.dtype, device=DEV)
    box = sentinel[tuple(slice(1, 1 + int(d)) for d in host.shape)]
    out, _ = sz3_amd.decompress(blob, dtype, out=box)
    assert out.data_ptr() == box.data_ptr()
    got = sentinel.cpu().numpy()
    inner = tuple(slice(1, 1 + int(d)) for d in host.shape)
    assert np.array_equal(got[inner].view(np.uint8), host.view(np.uint8))
    mask = np.ones(big_shape, bool)
    mask[inner] = False
    assert (got[mask] == 77).all(), "elements outside the view were written"


ALGOS = [
    ("lorenzo", dict(algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0)),
    ("lorenzo_reg_default", dict(algo=sz3_amd.ALGO_LORENZO_REG)),
    ("lorenzo2", dict(algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=1, regression=0)),
    ("interp", dict(algo=sz3_amd.ALGO_INTERP)),
    ("interp_lorenzo", dict(algo=sz3_amd.ALGO_INTERP_LORENZO)),
    ("nopred", dict(algo=sz3_amd.ALGO_NOPRED)),
    ("lossless", dict(algo=sz3_amd.ALGO_LOSSLESS)),
]


@pytest.mark.parametrize("name,kw", ALGOS, ids=[a[0] for a in ALGOS])
@pytest.mark.parametrize("stock", [0, 1])
def test_algorithms(name, kw, stock):
    shape = (40, 36, 44)
    kw = dict(kw)
    algo = kw.pop("algo")
    sz3_amd.set_stock_format(stock)
    try:
        check_roundtrip(field(shape), conf_for(shape, algo=algo, **kw), np.float32)
    finally:
        sz3_amd.set_stock_format(0)


@pytest.mark.parametrize("mode", range(6))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_bound_modes(mode, dtype):
    shape = (30, 50, 20)
    check_roundtrip(field(shape, dtype), conf_for(shape, mode=mode, eb=1e-2, rel=1e-3), np.dtype(dtype))


@pytest.mark.parametrize("dtype", INT_TYPES)
def test_integer_types(dtype):
    shape = (24, 33, 17)
    check_roundtrip(field(shape, dtype), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, eb=2.0), np.dtype(dtype))


def test_int64_beyond_2_53_goes_lossless():
    a = field((20, 30), "int64")
    a[3, 4] = (1 << 60) + 7
    conf = conf_for(a.shape, algo=sz3_amd.ALGO_LORENZO_REG, eb=1.0)
    check_roundtrip(a, conf, np.int64)


@pytest.mark.parametrize("shape", [(5000,), (3, 1000), (1, 257, 3), (7, 5, 9, 11), (2, 3, 4, 5), (4097,), (130, 1, 3)])
@pytest.mark.parametrize("algo", [sz3_amd.ALGO_LORENZO_REG, sz3_amd.ALGO_INTERP_LORENZO])
def test_ranks_and_thin_extents(shape, algo):
    check_roundtrip(field(shape), conf_for(shape, algo=algo), np.float32)


@pytest.mark.parametrize("algo", [sz3_amd.ALGO_LORENZO_REG, sz3_amd.ALGO_INTERP_LORENZO, sz3_amd.ALGO_NOPRED])
def test_stock_1d(algo):
    """the stock 1-D ALGO_LORENZO_REG chain is walked on the host: the device call copies the array there for it"""
    sz3_amd.set_stock_format(1)
    try:
        check_roundtrip(field((20000,)), conf_for((20000,), algo=algo), np.float32)
        check_roundtrip(field((9000,), "float64"), conf_for((9000,), algo=algo), np.float64)
    finally:
        sz3_amd.set_stock_format(0)


def test_eb_zero_and_white_noise():
    shape = (32, 32, 32)
    check_roundtrip(field(shape), conf_for(shape, eb=0.0), np.float32)
    noise = np.random.default_rng(3).random(shape, dtype=np.float32)
    check_roundtrip(noise, conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, eb=1e-6), np.float32)


def test_interp_lorenzo_pretuned_size():
    """>= 16 MB under an absolute bound: the host API pre-tunes from its host copy, the device call tunes in stage 1"""
    shape = (96, 128, 384)
    check_roundtrip(field(shape), conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO, eb=1e-3), np.float32)


def test_openmp_slabs(monkeypatch):
    monkeypatch.setenv("SZ3HIP_SLABS", "3")
    shape = (45, 40, 30)
    for algo in (sz3_amd.ALGO_LORENZO_REG, sz3_amd.ALGO_INTERP_LORENZO):
        check_roundtrip(field(shape), conf_for(shape, algo=algo, openmp=1), np.float32)
    check_roundtrip(field(shape, "int16"), conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, eb=1.0, openmp=1), np.int16)


def test_pieces():
    shape = (128, 512, 512)
    conf = conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG, eb=1e-3)
    a = field(shape)
    check_roundtrip(a, conf, np.float32)


# ---- strided input -------------------------------------------------------------------------------------------
def strided_case(kind):
    base = torch.from_numpy(field((24, 40, 52))).to(DEV)
    if kind == "subbox":
        return base[2:20, 3:37, 4:48]
    if kind == "field":
        inter = torch.from_numpy(field((20, 30, 36, 4))).to(DEV)
        return inter[..., 2]
    if kind == "permuted":
        return base.permute(2, 0, 1)
    if kind == "int16":
        t = torch.from_numpy(field((24, 40, 52), "int16")).to(DEV)
        return t[1:23, ::2, 5:50]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["subbox", "field", "permuted", "int16"])
@pytest.mark.parametrize("algo", [sz3_amd.ALGO_LORENZO_REG, sz3_amd.ALGO_INTERP_LORENZO])
def test_strided_input(kind, algo):
    v = strided_case(kind)
    assert not v.is_contiguous()
    conf = conf_for(tuple(v.shape), algo=algo, eb=1.0 if kind == "int16" else 1e-3)
    before = v.clone()
    assert device_container(v, conf) == device_container(v.contiguous(), conf) == host_container(v.cpu().numpy(), conf)
    assert torch.equal(v, before)


# ---- reference containers --------------------------------------------------------------------------------------
REF_CASES = [
    ("default_3d", (30, 34, 38), dict(algo=1)),
    ("lorenzo_reg_1d", (6000,), dict(algo=0, regression=True)),
    ("lorenzo_reg_2d", (70, 90), dict(algo=0, regression=True)),
    ("lorenzo_reg_3d", (30, 34, 38), dict(algo=0, regression=True)),
    ("nopred", (30, 34, 38), dict(algo=3)),
    ("lossless", (30, 34, 38), dict(algo=4)),
    ("openmp", (40, 34, 38), dict(algo=0, openmp=True)),
]


@pytest.mark.ref
@pytest.mark.parametrize("name,shape,kw", REF_CASES, ids=[c[0] for c in REF_CASES])
def test_reference_containers(name, shape, kw):
    from oracle_binding import have_ref
    if not have_ref():
        pytest.skip("oracle/_ref not built")
    a = field(shape)
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "a.bin"), os.path.join(d, "c.sz")
        a.tofile(src)
        r = subprocess.run([sys.executable, os.path.join(HERE, "checks", "_ref_write.py"), src, "float32", ",".join(map(str, shape)),
                            json.dumps(dict(abs_eb=1e-3, **kw)), dst], capture_output=True, timeout=300)
        if r.returncode != 0:
            pytest.skip("the reference's writer failed on this case (%d)" % r.returncode)
        blob = np.fromfile(dst, dtype=np.uint8).tobytes()
    check_decode(blob, np.float32, shape)


# ---- stream ordering, threads, Python face -------------------------------------------------------------------
def test_stream_ordering():
    shape = (64, 128, 128)
    conf = conf_for(shape, algo=sz3_amd.ALGO_LORENZO_REG)
    a = field(shape)
    want = host_container(a, conf)
    src = torch.from_numpy(a).to(DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t = torch.empty_like(src)
        torch.cuda._sleep(20_000_000)  # (the producer is still busy when the call is made)
        t.copy_(src)
        got = device_container(t, conf, stream=side)
    assert got == want


def test_threads():
    shapes = [(40, 50, 60), (64, 64, 64), (30, 90, 45), (100, 100, 10)]
    arrays = [field(s, seed=i) for i, s in enumerate(shapes)]
    confs = [conf_for(s, algo=sz3_amd.ALGO_LORENZO_REG if i % 2 else sz3_amd.ALGO_INTERP_LORENZO) for i, s in enumerate(shapes)]
    want = [host_container(a, c) for a, c in zip(arrays, confs)]
    tensors = [torch.from_numpy(a).to(DEV) for a in arrays]
    torch.cuda.synchronize()
    got = [None] * 4

    def run(i):
        for _ in range(3):
            got[i] = sz3_amd.compress(tensors[i], confs[i], stream=0)[0].tobytes()

    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert got == want


def test_python_face():
    shape = (33, 47, 29)
    conf = conf_for(shape, algo=sz3_amd.ALGO_INTERP_LORENZO)
    t = torch.from_numpy(field(shape)).to(DEV)
    b_dev, ratio = sz3_amd.compress(t, conf)
    b_host, ratio_h = sz3_amd.compress(t.cpu().numpy(), conf)
    assert b_dev.tobytes() == b_host.tobytes() and ratio == ratio_h
    host, _ = sz3_amd.decompress(b_host, np.float32, shape)
    dev, c2 = sz3_amd.decompress(b_host, torch.float32, shape, device=DEV)
    assert dev.dtype == torch.float32 and tuple(dev.shape) == shape and dev.is_cuda
    assert np.array_equal(dev.cpu().numpy(), host)
    big = torch.zeros((40, 50, 30), device=DEV)
    out, _ = sz3_amd.decompress(b_host, torch.float32, out=big[3:36, 1:48, :29])
    assert np.array_equal(out.cpu().numpy(), host) and float(big[0].abs().sum()) == 0.0

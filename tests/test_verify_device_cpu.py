"""sz3hip_verify_device without a GPU: the symbol, the struct's layout, the argument checks that need no device, a loud failure (never a
host loop) where a device would be needed, and the numpy branch of sz3_amd.verify as it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sz3_amd

L = sz3_amd.lib()
L.sz3hip_last_error_code.restype = C.c_int


def _codes():  # the error enum of include/sz3hip.h
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sz3hip.h")) as f:
        txt = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SZ3HIP_E[A-Z]+) = (-?\d+)", txt)}


CODES = _codes()
SENTINEL = 0xA5


def _verify(dt=0, dims=(8, 8), ori=0x1000, dec=0x2000, so=None, sd=None, bound=-1.0, out=True, N=None):
    """-> (rc, code, message, the bytes of *out afterwards)"""
    N = len(dims) if N is None else N
    d = (C.c_uint64 * max(len(dims), 1))(*dims)
    st = sz3_amd._CVerifyStats()
    C.memset(C.byref(st), SENTINEL, C.sizeof(st))
    arr = lambda s: (C.c_int64 * len(s))(*s) if s else None  # noqa: E731
    rc = L.sz3hip_verify_device(dt, N, d, ori, arr(so), dec, arr(sd), bound, C.byref(st) if out else None, None)
    return rc, L.sz3hip_last_error_code(), L.sz3hip_last_error().decode(), bytes(st)


def test_symbol_exported():
    assert hasattr(L, "sz3hip_verify_device")
    assert hasattr(sz3_amd, "verify_stats")


def test_struct_size():
    assert C.sizeof(sz3_amd._CVerifyStats) == 6 * 8 + 13 * 8
    names = [k for k, _ in sz3_amd._CVerifyStats._fields_]
    assert names[:6] == ["n", "n_nonfinite", "n_nonfinite_mismatch", "n_over", "first_over", "argmax"]
    assert names[6:] == ["min", "max", "max_diff", "max_pw_rel", "sum_ori", "sum_dec", "sum_sq_err", "sum_sq_dec", "psnr", "nrmse", "l2_err",
                         "l2_err_norm", "acEff"]


def test_struct_matches_header():
    """the Python mirror names the header's fields in the header's order"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sz3hip.h")) as f:
        body = re.search(r"typedef struct sz3hip_verify_stats \{(.*?)\}", f.read(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [x.strip() for x in decl.split(None, 1)[1].split(",")]
    assert fields == [k for k, _ in sz3_amd._CVerifyStats._fields_]


def test_unknown_data_type():
    for dt in (10, -1):
        rc, code, msg, _ = _verify(dt=dt)
        assert rc == code == CODES["SZ3HIP_EUNSUPPORTED"] and "dataType" in msg


@pytest.mark.parametrize("N", [0, 5, -1])
def test_rank_outside_1_to_4(N):
    rc, code, msg, _ = _verify(dims=(2, 2, 2, 2, 2), N=N)
    assert rc == code == CODES["SZ3HIP_EINVAL"] and "dimension" in msg


def test_extent_of_zero():
    rc, code, msg, _ = _verify(dims=(4, 0, 3))
    assert rc == code == CODES["SZ3HIP_EINVAL"] and "dimension" in msg


@pytest.mark.parametrize("which", ["ori", "dec"])
def test_negative_stride_refused(which):
    kw = {"so" if which == "ori" else "sd": [8, -1]}
    rc, code, msg, _ = _verify(**kw)
    assert rc == code == CODES["SZ3HIP_EINVAL"] and "negative" in msg


def test_out_null():
    rc, code, msg, _ = _verify(out=False)
    assert rc == code == CODES["SZ3HIP_EINVAL"] and "out" in msg


def test_overlapping_and_broadcast_strides_pass_the_stride_check():
    """both arrays are only read: what an output view refuses is accepted here, and the call stops at the pointer check"""
    for st in ([0, 1], [1, 1], [0, 0]):
        rc, code, msg, _ = _verify(so=st)
        assert rc == code == CODES["SZ3HIP_EINVAL"] and "overlap" not in msg and "device memory" in msg


def test_host_pointer_fails_and_leaves_out_untouched():
    """a host pointer (or no device at all) is an error; nothing falls back to a host loop"""
    a = np.random.default_rng(0).random((8, 8), dtype=np.float32)
    b = a + 1
    rc, code, msg, raw = _verify(ori=a.ctypes.data, dec=b.ctypes.data)
    assert rc == code == CODES["SZ3HIP_EINVAL"] and "device memory" in msg
    assert raw == bytes([SENTINEL]) * C.sizeof(sz3_amd._CVerifyStats)


def test_python_face_refuses_what_is_not_two_gpu_tensors():
    a = np.zeros((4, 4), np.float32)
    with pytest.raises(TypeError):
        sz3_amd.verify_stats(a, a)
    torch = pytest.importorskip("torch")
    t = torch.zeros((4, 4))
    with pytest.raises(TypeError):
        sz3_amd.verify_stats(a, t)
    with pytest.raises(ValueError, match="HIP device"):
        sz3_amd.verify_stats(t, t)


def test_numpy_verify_unchanged():
    """the numpy branch of sz3_amd.verify returns what it returned before the tensor branch was added"""
    o = np.array([[0.0, 1.0, 2.0, 4.0], [-3.0, 0.5, 0.25, 8.0]], dtype=np.float32)
    d = o + np.array([[0.5, -0.25, 0.0, 0.125], [0.0, 0.0, -1.0, 0.0]], dtype=np.float32)
    max_diff, psnr, nrmse = sz3_amd.verify(o, d)
    mse = (0.25 + 0.0625 + 0.015625 + 1.0) / 8  # exact in binary
    assert max_diff == 1.0
    assert psnr == 20 * np.log10(11.0) - 10 * np.log10(mse)
    assert nrmse == np.sqrt(mse) / 11.0
    assert sz3_amd.verify(o, o) == (0.0, float("inf"), 0.0)
    c = np.full(5, 3.0)
    assert sz3_amd.verify(c, c + 2) == (2.0, float("inf"), 0.0)

"""What tests/test_gpu_device_views.py and tests/checks/device_view_sweep.py share on the device: a base allocation with its host copy, a
view_model.View of it as a tensor, and the two hooks that run the strided kernels alone (sz3hip_debug_gather / sz3hip_debug_scatter).
A plain module: it holds no test and no fixture."""
import ctypes as C

import numpy as np
import torch

import sz3_amd
import view_model as M

DEV = "cuda:0"
L = sz3_amd.lib()
for _f in (L.sz3hip_debug_gather, L.sz3hip_debug_scatter):
    _f.restype = C.c_int
    _f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]


class Alloc:
    """a base allocation: `dev` (uint8 tensor on the device) and `host`, the bytes it was filled with"""

    def __init__(self, host_bytes):
        self.host = np.ascontiguousarray(host_bytes, dtype=np.uint8).reshape(-1).copy()
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0

    @staticmethod
    def random(dtype, n_elems, rng):
        return Alloc(rng.integers(0, 256, int(n_elems) * np.dtype(dtype).itemsize, dtype=np.uint8))

    @staticmethod
    def of(array):
        return Alloc(np.ascontiguousarray(array).reshape(-1).view(np.uint8))

    def now(self):
        """the allocation's bytes as the device holds them"""
        torch.cuda.synchronize()
        return self.dev.cpu().numpy()

    def unchanged(self):
        return np.array_equal(self.now(), self.host)

    def addr(self, view):
        return self.dev.data_ptr() + view.offset * view.itemsize

    def inside(self, view):
        return view.numel == 0 or (view.last + 1) * view.itemsize <= self.host.size

    def tensor(self, view):
        assert self.inside(view), "the view leaves the allocation"
        typed = self.dev.view(getattr(torch, view.dtype))
        return torch.as_strided(typed, view.shape, view.strides, view.offset)


def _dims(view):
    n = len(view.shape)
    return n, (C.c_uint64 * n)(*view.shape), (C.c_int64 * n)(*view.strides)


def gather_rc(alloc, view, out):
    assert alloc.inside(view) and out.numel() == view.numel
    n, dims, strides = _dims(view)
    return L.sz3hip_debug_gather(M.DTYPES.index(view.dtype), alloc.addr(view), n, dims, strides, out.data_ptr(), torch.cuda.current_stream().cuda_stream)


def gather(alloc, view):
    """sz3hip_debug_gather of the view -> the dense array on the host (f64 for the integer types)"""
    odt = torch.float64 if view.dtype in M.INT_TYPES else getattr(torch, view.dtype)
    out = torch.empty(view.numel, dtype=odt, device=DEV)
    sz3_amd._check(gather_rc(alloc, view, out))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(view.shape)


def gather_expected(alloc, view):
    a = np.ascontiguousarray(M.view_of(alloc.host, view))
    return M.widen(a) if view.dtype in M.INT_TYPES else a


def scatter_rc(values_dev, alloc, view):
    """sz3hip_debug_scatter of the dense device array (f64 for the integer types) into the view"""
    assert alloc.inside(view) and values_dev.numel() == view.numel
    n, dims, strides = _dims(view)
    return L.sz3hip_debug_scatter(M.DTYPES.index(view.dtype), values_dev.data_ptr(), n, dims, strides, alloc.addr(view), torch.cuda.current_stream().cuda_stream)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def first_difference(got, want, view):
    """where two allocations differ, for a message: byte offsets, and whether they lie inside the view's elements"""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return "equal"
    es = view.itemsize
    mine = np.zeros(got.size // es + 1, bool)
    if all(s > 0 for s in view.strides) or view.numel < 1 << 22:
        mine[np.unique(np.asarray(M.touched_offsets(view.shape, view.strides)) + view.offset)] = True
    inside = mine[bad // es]
    return "%d bytes differ (%d inside the view's elements, %d outside); first at byte %d (element %d)" % (bad.size, int(inside.sum()), int((~inside).sum()), int(bad[0]), int(bad[0]) // es)

"""What the GPU tests of the partial decodes (test_gpu_coarse.py, test_gpu_region.py, test_gpu_tile.py) share: the fields, the Config, the
container and the device context's payload. A plain module: it holds no test and no fixture."""
import os
import re

import numpy as np
import torch

import sz3_amd

DEV = "cuda:0"
EB = 1e-2
INTERP_IDS = (sz3_amd.ALGO_INTERP, sz3_amd.ALGO_HIP_INTERP)


def _codes():  # the error enum of include/sz3hip.h
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sz3hip.h")) as f:
        txt = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SZ3HIP_E[A-Z]+) = (-?\d+)", txt)}


CODES = _codes()


def smooth(shape, dtype="float32", seed=7):
    """a smooth N-D field (periods of 37 .. 61 points, four times that in 1-D; amplitude ~1) with noise of sigma 1e-3: at the bound 1e-2
    most codes are the central one"""
    ix = np.indices(shape, dtype=np.float64)
    w = 4.0 if len(shape) == 1 else 1.0  # (a 1-D array of a few thousand points has no other extent to pay for the stream's fixed part)
    f = np.ones(shape)
    for i, x in enumerate(ix):
        f = f * np.sin(2 * np.pi * x / (w * (61 - 7 * i)) + 0.4 * i)
    f = f + 0.25 * np.sin(2 * np.pi * sum((i + 1) * x for i, x in enumerate(ix)) / (w * 37))
    f = f + np.random.default_rng(seed).normal(0.0, 1e-3, size=shape)
    return f.astype(dtype)


def spiky(shape=(65, 47, 130), n_spikes=200, seed=11):
    """the 3-D field with spikes of 1e6 at seeded positions: unpredictable values on and off every coarse grid"""
    a = smooth(shape)
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.integers(0, d, n_spikes) for d in shape], axis=1)
    a[tuple(pos.T)] = 1e6
    return a, pos


def conf_for(shape, algo=sz3_amd.ALGO_INTERP, eb=EB, **kw):
    """quantbinCnt 1024: the payload stores a code length per symbol from the smallest to the largest in use, and symbol 0 (anchors,
    unpredictable points) is always in use — under the default 65536 bins that table alone is 32 KB, more than the smallest arrays here
    hold, and the dispatcher then writes them lossless (payload >= array). +-512 bins at this bound cover the fields' residuals."""
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = algo
    c.errorBoundMode = sz3_amd.EB_ABS
    c.absErrorBound = eb
    c.quantbinCnt = 1024
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def container(a, conf):
    return sz3_amd.compress(np.ascontiguousarray(a), conf)[0].copy()


def raw(t):
    return t.contiguous().cpu().numpy().reshape(-1).view(np.uint8)


def box_slices(lo, ext):
    return tuple(slice(a, a + e) for a, e in zip(lo, ext))


def boxes_of(shape):
    """the boxes of the geometry cases: the whole array; one interior point with odd coordinates; a box at the origin corner; one ending at the
    far corner; one with odd lo that straddles the coordinates 32 and 64 along x (where x is shorter: odd lo, to the row's end); one of extent 1
    in the slowest dimension"""
    N = len(shape)
    whole = ((0,) * N, tuple(shape))
    point = (tuple(min(d - 1, (d // 2) | 1) for d in shape), (1,) * N)
    origin = ((0,) * N, tuple(max(1, min(d, d // 3 + 1)) for d in shape))
    far_ext = tuple(max(1, min(d, d // 4 + 2)) for d in shape)
    far = (tuple(d - e for d, e in zip(shape, far_ext)), far_ext)
    x = shape[-1]
    xlo = 29 if x > 69 else 3
    lo = tuple(min(d - 1, 1) for d in shape[:-1]) + (xlo,)
    straddle = (lo, tuple(max(1, min(5, d - a)) for d, a in zip(shape[:-1], lo)) + (min(40, x - xlo),))
    slab_lo = (min(shape[0] - 1, 5),) + tuple(min(d - 1, 2) for d in shape[1:])
    slab = (slab_lo, (1,) + tuple(d - a for d, a in zip(shape[1:], slab_lo[1:])))
    return [whole, point, origin, far, straddle, slab]


# the containers that are no single interpolation stream: the partial decodes take the full decode, then the strided gather
FALLBACKS = [
    ("lorenzo", dict(algo=sz3_amd.ALGO_LORENZO_REG, lorenzo=1, lorenzo2=0, regression=0)),
    ("blocks_default", dict(algo=sz3_amd.ALGO_LORENZO_REG)),
    ("nopred", dict(algo=sz3_amd.ALGO_NOPRED)),
    ("lossless", dict(algo=sz3_amd.ALGO_INTERP_LORENZO, eb=0.0)),
]


def device_payload(a, conf):
    dc = sz3_amd.DeviceCompressor(a.size, a.dtype)
    cap = dc.payload_bound(a.size, worst_case=True)
    t = torch.from_numpy(a).to(DEV)
    pl = torch.empty(cap, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    size = dc.compress(conf, t.data_ptr(), pl.data_ptr(), cap, s)
    full = torch.empty_like(t)
    dc.decompress(pl.data_ptr(), size, full.data_ptr(), s)
    torch.cuda.synchronize()
    return dc, pl, size, full

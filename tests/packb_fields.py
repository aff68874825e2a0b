"""Fields built on the device for the tests of k_pack_b's unit loop (tests/test_gpu_packb_units.py, tools/record_packb_golden.py,
tools/bench_rough.py): arrays of tens of millions of elements that are a pure function of their indices — products of 1-D sine
factors (numpy, float64, rounded to float32 once) broadcast on the device, plus an integer-hash "noise" (exact integer arithmetic, four
bytes of a 32-bit hash summed: bounded, bell-shaped, standard deviation 1 after scaling). No random generator, no host array."""
import numpy as np

BASE_SIGMA = 2e-3  # the grain of the C2 field (tests/fields.py): chunks of ~128 words at abs 1e-3
_HASH_STD = 147.79715  # sqrt(4 * (256^2 - 1) / 12): four uniform bytes summed


def _hash_noise(torch, idx, salt):
    """idx: int64 tensor of element indices -> float32 in (-3.46, 3.46), mean 0, standard deviation 1"""
    m = 0xFFFFFFFF
    h = (idx * 0x9E3779B1 + salt) & m
    h = h ^ (h >> 15)
    h = (h * 0x85EBCA77) & m  # (wraps in int64: the low 32 bits are what they are)
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE3D) & m
    h = h ^ (h >> 16)
    s = (h & 255) + ((h >> 8) & 255) + ((h >> 16) & 255) + ((h >> 24) & 255) - 510
    return s.to(torch.float32) * np.float32(1.0 / _HASH_STD)


def device_field(torch, dev, shape, rough=None, sigma=0.03):
    """(z, y, x) float32 on dev. rough: None (the smooth field), "all", "rows5" (every fifth row of x gets the rough noise) or
    "chunks5" (every fifth run of 1024 elements does: with the spill of the Lorenzo stencil into the next row and plane, chunks
    0, 1, 2 mod 5 of the code stream are rough and chunks 3, 4 mod 5 are not — every order of the two inside a unit of four)."""
    nz, ny, nx = shape

    def fac(n, period, fn):
        return torch.from_numpy(fn(2 * np.pi * np.arange(n, dtype=np.float64) / period).astype(np.float32)).to(dev)

    f = fac(nz, 128, np.sin)[:, None, None] * fac(ny, 96, np.cos)[None, :, None] * fac(nx, 64, np.sin)[None, None, :]
    f = f + np.float32(0.25) * (fac(nz, 37, np.cos)[:, None, None] * fac(ny, 53, np.sin)[None, :, None] * fac(nx, 41, np.cos)[None, None, :])
    idx = torch.arange(nz * ny * nx, dtype=torch.int64, device=dev).reshape(nz, ny, nx)
    f = f + np.float32(BASE_SIGMA) * _hash_noise(torch, idx, 1)
    if rough is not None:
        r = np.float32(sigma) * _hash_noise(torch, idx, 2)
        if rough == "rows5":
            r = r * ((idx // nx) % 5 == 0).to(torch.float32)
        elif rough == "chunks5":
            r = r * ((idx >> 10) % 5 == 0).to(torch.float32)
        elif rough != "all":
            raise ValueError(rough)
        f = f + r
    return f.contiguous()


def spike(torch, f, count=4000):
    """steps of hundreds of lattice units at `count` distinct places (listed deltas: byte 255 of a one-byte stream); in place"""
    n = f.numel()
    k = torch.arange(count, dtype=torch.int64, device=f.device)
    pos = k * (n // count) + ((k * 0x9E3779B1) & 0xFFFFFFFF) % (n // count)  # one place in each of `count` equal runs
    amp = np.float32(0.3) + np.float32(0.25) * (_hash_noise(torch, k, 3) + np.float32(3.5))  # 0.3 .. 2.05
    sign = ((k & 1) * 2 - 1).to(torch.float32)
    flat = f.reshape(-1)
    flat[pos] = flat[pos] + sign * amp
    return f

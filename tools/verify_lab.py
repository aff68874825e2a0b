#!/usr/bin/env python3
"""Timings of sz3_amd.verify_stats (sz3hip_verify_device) on one GPU, as one JSON line: python tools/verify_lab.py
Per case the median wall-clock ms of 20 synchronous calls after 3 warm-ups and GB/s = bytes of both arrays / time; beside it, from the
same run, DeviceCompressor.minmax on the ori array (the existing one-array reduction: bytes of that array / time; contiguous cases) and
the route a caller had before: .cpu() of both tensors plus the numpy sz3_amd.verify (LAB_HOST_ROUTE=0 leaves it out)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sz3_amd  # noqa: E402

DEV = torch.device("cuda:0")


def make(shape, dtype):
    n = int(np.prod(shape))
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.linspace(0, 6.0, n, device=DEV, dtype=torch.float64)
    a = torch.sin(x) * 10 + torch.cumsum(torch.randn(n, device=DEV, dtype=torch.float64, generator=g), 0) * 0.05
    ori = a.to(dtype).reshape(shape)
    dec = (a + (torch.rand(n, device=DEV, dtype=torch.float64, generator=g) - 0.5) * 2e-3).to(dtype).reshape(shape)
    return ori, dec


def median_ms(f, reps=20, warm=3):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def case(name, shape, dtype, interleave=False):
    ori, dec = make(shape, dtype)
    if interleave:  # ori as field 1 of a 4-way interleaved array (inner stride 4)
        big = torch.zeros(tuple(shape) + (4,), dtype=dtype, device=DEV)
        big[..., 1] = ori
        ori = big[..., 1]
    nbytes = ori.numel() * ori.element_size()
    st = sz3_amd.verify_stats(ori, dec, bound=1e-3)
    ms = median_ms(lambda: sz3_amd.verify_stats(ori, dec, bound=1e-3))
    r = {"case": name, "shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "ori_strides": list(ori.stride()),
         "verify_ms": round(ms, 4), "verify_GBps": round(2 * nbytes / ms / 1e6, 1), "max_diff": st.max_diff, "psnr": st.psnr, "n_over": st.n_over}
    if ori.is_contiguous():
        dc = sz3_amd.DeviceCompressor(ori.numel(), sz3_amd._np_dtype(dtype))
        stream = torch.cuda.current_stream().cuda_stream
        mm = median_ms(lambda: dc.minmax(ori.data_ptr(), ori.numel(), stream))
        r.update(minmax_ms=round(mm, 4), minmax_GBps=round(nbytes / mm / 1e6, 1))
        r["verify_over_minmax_GBps"] = round(r["verify_GBps"] / r["minmax_GBps"], 3)
        assert dc.minmax(ori.data_ptr(), ori.numel(), stream) == (st.min, st.max)
        dc.close()
    if os.environ.get("LAB_HOST_ROUTE", "1") != "0":
        def host_route():
            return sz3_amd.verify(ori.cpu().numpy(), dec.cpu().numpy())
        hm = median_ms(host_route, reps=3, warm=1)
        got = sz3_amd.verify(ori, dec)
        want = host_route()
        assert got[0] == want[0] and abs(got[1] - want[1]) <= 1e-9 * abs(want[1]), (got, want)
        r.update(host_route_ms=round(hm, 2), host_route_over_verify=round(hm / ms, 1))
    return r


if __name__ == "__main__":
    out = {"device": torch.cuda.get_device_name(0), "cases": [
        case("f32_512^3_contiguous", (512, 512, 512), torch.float32),
        case("f32_512^3_ori_field_1_of_4", (512, 512, 512), torch.float32, interleave=True),
        case("f64_256^3_contiguous", (256, 256, 256), torch.float64),
        case("f32_2^20_contiguous", (1 << 20,), torch.float32),
    ]}
    print(json.dumps(out))

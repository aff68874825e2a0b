#!/usr/bin/env python3
"""Device-container calls against the host API, one JSON line on stdout.

  C2: 512^3 f32 (tests/fields.py field3d), ALGO_LORENZO_REG, abs 1e-3;  C3: the same array, ALGO_INTERP_LORENZO, abs 1e-4.
  compress:   sz3hip_compress_from_device(tensor)  vs  sz3hip_compress(host copy)      (same container, checked)
  decompress: sz3hip_decompress_to_device(tensor)  vs  sz3hip_decompress(host array)   (same bits, checked)
One process, warmed up, the two calls alternating, median of --reps. The strided gather kernel on two views of a 512^3 f32 array
(a sub-box, innermost stride 1; one field of a 4-field interleaved array) beside a device-to-device hipMemcpy of the same byte count.
SZ3HIP_TIMING=1 in the environment adds the host API's breakdown on stderr.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (before the library: one HIP runtime)
import numpy as np  # noqa: E402
import sz3_amd  # noqa: E402
from fields import field3d  # noqa: E402


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def leg(name, a, t, algo, eb, reps):
    conf = sz3_amd.Config(*a.shape)
    conf.cmprAlgo = algo
    conf.absErrorBound = eb
    cap = sz3_amd.compress_bound(conf, np.float32)
    out_h = np.empty(cap, np.uint8)
    out_d = np.empty(cap, np.uint8)
    dec_h = np.empty(a.size, np.float32)
    dec_d = torch.empty(a.shape, dtype=torch.float32, device=t.device)
    hb = sz3_amd.compress(a, conf, out=out_h)[0].tobytes()
    db = sz3_amd.compress(t, conf, out=out_d)[0].tobytes()
    assert hb == db, "containers differ"
    sz3_amd.decompress(hb, np.float32, out=dec_h)
    sz3_amd.decompress(hb, np.float32, out=dec_d)
    assert np.array_equal(dec_d.cpu().numpy().ravel(), dec_h), "decoded arrays differ"
    res = {"bytes": a.nbytes, "container_bytes": len(hb)}
    ch, cd, dh, dd = [], [], [], []
    for _ in range(reps):  # alternating
        ch.append(median_ms(lambda: sz3_amd.compress(a, conf, out=out_h), 1)[0])
        cd.append(median_ms(lambda: sz3_amd.compress(t, conf, out=out_d), 1)[0])
        dh.append(median_ms(lambda: sz3_amd.decompress(hb, np.float32, out=dec_h), 1)[0])
        dd.append(median_ms(lambda: sz3_amd.decompress(hb, np.float32, out=dec_d), 1)[0])
    for k, v in (("compress_host_ms", ch), ("compress_device_ms", cd), ("decompress_host_ms", dh), ("decompress_device_ms", dd)):
        res[k] = round(float(np.median(v)), 3)
        res[k + "_all"] = [round(x, 3) for x in v]
    res["compress_speedup"] = round(res["compress_host_ms"] / res["compress_device_ms"], 3)
    res["decompress_speedup"] = round(res["decompress_host_ms"] / res["decompress_device_ms"], 3)
    return res


def gather_leg(reps):
    L = sz3_amd.lib()
    dev = torch.device("cuda:0")
    base = torch.randn((512, 512, 512), device=dev)
    cases = {}
    views = {"subbox_inner_stride1": base[8:504, 8:504, 8:504],
             "field_of_4_interleaved": torch.randn((256, 256, 512, 4), device=dev)[..., 1]}
    for name, v in views.items():
        n = v.numel()
        dst = torch.empty(n, device=dev)
        cpy = torch.empty(n, device=dev)
        src = torch.empty(n, device=dev)
        # the gather alone (sz3hip_debug_gather: the kernel the compress call runs first on a strided view)
        fn = L.sz3hip_debug_gather
        fn.restype = C.c_int
        fn.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
        dims = (C.c_uint64 * 3)(*v.shape)
        st = (C.c_int64 * 3)(*v.stride())
        sid = torch.cuda.current_stream().cuda_stream
        g = lambda: fn(0, v.data_ptr(), 3, dims, st, dst.data_ptr(), sid)  # noqa: E731
        m = lambda: cpy.copy_(src)  # noqa: E731 (hipMemcpy device-to-device of the same byte count)
        assert g() == 0
        assert torch.equal(dst.view(v.shape), v)
        for _ in range(3):
            g(), m()
        gt, mt = [], []
        for _ in range(reps):
            gt.append(median_ms(g, 1)[0])
            mt.append(median_ms(m, 1)[0])
        gms, mms = float(np.median(gt)), float(np.median(mt))
        useful = 2 * n * 4  # read + write
        inner = v.stride()[-1]
        read_lines = n * 4 * (inner if inner > 1 and inner * 4 <= 128 else 1)  # bytes of the cache lines the reads touch
        cases[name] = {"elements": n, "gather_ms": round(gms, 4), "copy_ms": round(mms, 4),
                       "gather_GBps_useful": round(useful / gms / 1e6, 1), "copy_GBps": round(useful / mms / 1e6, 1),
                       "gather_over_copy": round(mms / gms, 3), "read_line_bytes": read_lines, "useful_read_bytes": n * 4}
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="c2,c3,gather")
    ap.add_argument("--once", action="store_true", help="one compress + one decompress of C2 on the device (the copy trace run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.once:  # (the array is made on the device: any copy of its size in the trace would be the library's)
        x = torch.linspace(0, 40, 512, device=dev)
        t = (torch.sin(x)[:, None, None] * torch.cos(x)[None, :, None] + torch.sin(2 * x)[None, None, :]).contiguous()
        conf = sz3_amd.Config(*t.shape)
        conf.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
        conf.absErrorBound = 1e-3
        b = sz3_amd.compress(t, conf)[0]
        out = torch.empty_like(t)
        sz3_amd.decompress(b, np.float32, out=out)
        torch.cuda.synchronize()
        print(json.dumps({"once": True, "container_bytes": int(b.size)}))
        return
    a = field3d((512, 512, 512)).astype(np.float32)
    t = torch.from_numpy(a).to(dev)
    torch.cuda.synchronize()
    res = {"tool": "device_container_lab", "gpu": torch.cuda.get_device_name(0), "reps": args.reps}
    legs = args.legs.split(",")
    if "c2" in legs:
        res["C2"] = leg("C2", a, t, sz3_amd.ALGO_LORENZO_REG, 1e-3, args.reps)
    if "c3" in legs:
        res["C3"] = leg("C3", a, t, sz3_amd.ALGO_INTERP_LORENZO, 1e-4, args.reps)
    if "gather" in legs:
        res["gather"] = gather_leg(args.reps * 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Boxes composited along an axis at C3 (512^3 f32, default algorithm, abs 1e-4) through an opened stream, on section
15's three screens (tools/stream_lab.py). Every box's RGBA32F image goes into a contiguous array of its own; the table has 256 entries:
  (a) composite_z, composite_z_cut, composite_x, composite_x_cut
                               one sz3hip_stream_composite along z (axis 0: a thread per output point) and along x (axis 2, the fastest:
                               the body that stages through LDS), with cutoff +Inf and with cutoff 0.99
  (b) request_torch_z, request_torch_x
                               what a caller issues without it: sz3hip_stream_request into contiguous f32 arrays, then per box the torch
                               chain — window, clamp, cast, table lookup, 1 - a, exclusive cumprod, multiply, sum
  (c) request                  sz3hip_stream_request alone: the existing path
One JSON line (LAB_WRITE=<file> appends it there: profiles/r29_composite.txt holds the lines of the measurement in section 26), with its
`series` (LAB_SERIES) and `build` (LAB_TAG). Protocol: tools/stream_lab.py's — a run is CALLS calls between two device synchronisations,
the variants alternate, seven runs each, the figure is the median (us per call) with the runs' min and max; the chain is off. Every image of
(a) without a cutoff is compared with the torch chain's f32 result (the largest difference is reported: no equality, the tests hold the
bytes). LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: a package without the call runs (b) and (c) alone. Run it under a time
limit of its own (timeout -k 10 400 python tools/composite_lab.py); LAB_SIZE=<n> takes n^3."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("LAB_PKG") or ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sz3_amd  # noqa: E402
from fields import field3d  # noqa: E402
from reduce_lab import requests  # noqa: E402

S = int(os.environ.get("LAB_SIZE", "512"))
RUNS, CALLS = 7, 10
LUT_N = 256
HAVE = hasattr(sz3_amd.Stream, "composite") and os.environ.get("LAB_COMPOSITE", "1") != "0"
CASES = (("z", 0, float("inf")), ("z_cut", 0, 0.99), ("x", 2, float("inf")), ("x_cut", 2, 0.99))


def main():
    dev = torch.device("cuda:0")
    a = field3d((S, S, S))
    d_in = torch.from_numpy(a).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    conf = sz3_amd.Config(S, S, S)
    conf.cmprAlgo = sz3_amd.ALGO_INTERP_LORENZO
    conf.absErrorBound = 1e-4
    dc = sz3_amd.DeviceCompressor(a.size, np.float32)
    cap = dc.payload_bound(a.size)
    pl = torch.empty(cap, dtype=torch.uint8, device=dev)
    size = dc.compress(conf, d_in.data_ptr(), pl.data_ptr(), cap, s)
    torch.cuda.synchronize()
    st = dc.open_stream(pl.data_ptr(), size, s)
    assert st.stats()["fast"] == 1
    sz3_amd.set_chain_points(0)
    lo, hi = [float(v) for v in np.quantile(a, [0.05, 0.95])]
    rng = np.random.default_rng(11)
    lut_h = rng.random((LUT_N, 4)).astype(np.float32)
    lut_h[:, 3] *= np.float32(0.08)  # (a 64-point column reaches an opacity of about 0.9: the cutoff bites on some columns, not on all)
    lut = torch.from_numpy(lut_h).to(dev)
    scale = LUT_N / (hi - lo)

    screens = {n: items for n, items in requests().items() if n != "frame"}
    variants, info, images, kept = {}, {}, {}, []
    # every variant calls the C face over structs built once: the figures are the calls', not the Python wrappers'
    L, C, handle = sz3_amd.lib(), sz3_amd.C, sz3_amd._stream_handle(dev, None)

    def tile_reqs(items, outs):
        reqs = (sz3_amd._CTileReq * len(items))()
        for r, it, o in zip(reqs, items, outs):
            r.level = it[0]
            r.box.lo[:3], r.box.ext[:3] = it[1], it[2]
            r.d_out = o.data_ptr()
        return reqs

    def chain(o, axis):
        code = ((o - lo) * scale).clamp_(0, LUT_N - 1).to(torch.int64)
        e = lut[code]
        al = e[..., 3]
        t = torch.cumprod(1.0 - al, dim=axis)
        t = torch.cat([torch.ones_like(t.narrow(axis, 0, 1)), t.narrow(axis, 0, t.shape[axis] - 1)], dim=axis)
        w = t * al
        return torch.cat([(w.unsqueeze(-1) * e[..., :3]).sum(dim=axis, keepdim=True), w.sum(dim=axis, keepdim=True).unsqueeze(-1)], dim=-1)

    for name, items in screens.items():
        n = len(items)
        outs = [torch.empty(it[2], dtype=torch.float32, device=dev) for it in items]
        treqs = tile_reqs(items, outs)
        kept.append((outs, treqs))

        def request(treqs=treqs, n=n):
            assert L.sz3hip_stream_request(st._h, treqs, n, handle) == 0
        variants["request_%s" % name] = request
        for ax, axis in (("z", 0), ("x", 2)):
            def request_torch(f=request, outs=outs, axis=axis):
                f()
                return [chain(o, axis) for o in outs]
            variants["request_torch_%s_%s" % (ax, name)] = request_torch
        if not HAVE:
            continue
        for tag, axis, cutoff in CASES:
            imgs = [torch.empty(tuple(1 if j == axis else e for j, e in enumerate(it[2])) + (4,), dtype=torch.float32, device=dev) for it in items]
            images["composite_%s_%s" % (tag, name)] = imgs
            creqs = tile_reqs(items, imgs)
            opts = sz3_amd._CCompositeOpts()
            opts.lo, opts.hi, opts.cutoff, opts.axis, opts.out_type, opts.lut_n, opts.d_lut = lo, hi, cutoff, axis, sz3_amd.COMPOSITE_RGBA32F, LUT_N, lut.data_ptr()
            kept.append((creqs, opts))

            def composite(creqs=creqs, opts=opts, n=n):
                assert L.sz3hip_stream_composite(st._h, creqs, n, C.byref(opts), handle) == 0
            variants["composite_%s_%s" % (tag, name)] = composite

    for f in variants.values():  # warm-up: code objects, the handle's scratch and table
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    diff = 0.0
    for name, items in screens.items():
        for v in [n for n in variants if n.endswith("_" + name) and not n.startswith("request_torch")]:
            l0 = L.sz3hip_debug_region_launches()
            variants[v]()
            info[v] = {"launches": int(L.sz3hip_debug_region_launches() - l0)}
        torch.cuda.synchronize()
        if not HAVE:
            continue
        for ax, axis in (("z", 0), ("x", 2)):
            want = variants["request_torch_%s_%s" % (ax, name)]()
            for img, w in zip(images["composite_%s_%s" % (ax, name)], want):
                diff = max(diff, float((img - w).abs().max()))
    times = {n: [] for n in variants}
    for _ in range(RUNS):
        for n, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / CALLS * 1e6)
    device = {}
    for n, f in variants.items():  # the device's share, in runs of its own: a pair of events around one call
        d = []
        for _ in range(RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            d.append(1e3 * e0.elapsed_time(e1))
        device[n] = round(float(np.median(d)), 1)
    res = {"series": os.environ.get("LAB_SERIES", "1"), "build": os.environ.get("LAB_TAG", "this"), "case": "C3", "shape": [S, S, S], "dtype": "float32",
           "abs_eb": 1e-4, "ratio": round(a.nbytes / size, 3), "lut_n": LUT_N, "window": [lo, hi],
           "points": {n: int(sum(np.prod(it[2]) for it in items)) for n, items in screens.items()},
           "runs": RUNS, "calls_per_run": CALLS, "composite_call": HAVE, "composite_max_abs_difference_to_the_torch_chain": diff if HAVE else None,
           "us_per_call": {n: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in times.items()},
           "device_us": device, "requests": info}
    st.close()
    line = json.dumps(res)
    print(line)
    if os.environ.get("LAB_WRITE"):
        with open(os.environ["LAB_WRITE"], "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Boxes projected along an axis at C3 (512^3 f32, default algorithm, abs 1e-4) through an opened stream, on section
15's three screens (tools/stream_lab.py). Every box's image goes into a contiguous array of its own:
  (a) project_max_z, project_sum_z, project_max_x, project_sum_x
                               one sz3hip_stream_project: MAX and SUM along z (axis 0: a thread per output point) and along x (axis 2, the
                               fastest: the body that stages through LDS)
  (b) request_torch_max_z, ... what a caller issues without it: sz3hip_stream_request into contiguous f32 arrays, then per box torch.amax /
                               torch.sum over the axis (keepdim)
  (c) request                  sz3hip_stream_request alone: the existing path, to set against the parent commit's package
One JSON line (LAB_WRITE=<file> appends it there: profiles/r24_project.txt holds the lines of the measurement in section 21). Protocol:
tools/stream_lab.py's — a run is CALLS calls between two device synchronisations, the variants alternate, seven runs each, the figure is the
median (us per call) with the runs' min and max; the chain is off. Every MAX image is compared with torch.amax over the full decode's slice
(equal, the field has no NaN); for SUM the largest difference to torch.sum's f32 result is reported.
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package has no projection and runs (b) and (c) alone. Run it
under a time limit of its own (timeout -k 10 400 python tools/project_lab.py); LAB_SIZE=<n> takes n^3; LAB_TAG=<name> goes into the line as
"build"; LAB_PROJECT=0 leaves the projecting variants out of this tree's run too: a process with the parent's variants, for the comparison
of (c)."""
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
HAVE = hasattr(sz3_amd.Stream, "project") and os.environ.get("LAB_PROJECT", "1") != "0"
CASES = (("max", "z", 0), ("sum", "z", 0), ("max", "x", 2), ("sum", "x", 2))


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
    full = torch.empty_like(d_in)
    dc.decompress(pl.data_ptr(), size, full.data_ptr(), s)
    torch.cuda.synchronize()
    st = dc.open_stream(pl.data_ptr(), size, s)
    assert st.stats()["fast"] == 1
    sz3_amd.set_chain_points(0)

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

    for name, items in screens.items():
        n = len(items)
        outs = [torch.empty(it[2], dtype=torch.float32, device=dev) for it in items]
        treqs = tile_reqs(items, outs)
        kept.append((outs, treqs))

        def request(treqs=treqs, n=n):
            assert L.sz3hip_stream_request(st._h, treqs, n, handle) == 0
        variants["request_%s" % name] = request
        for op, ax, axis in CASES:
            fn = torch.amax if op == "max" else torch.sum

            def request_torch(f=request, outs=outs, fn=fn, axis=axis):
                f()
                return [fn(o, dim=axis, keepdim=True) for o in outs]
            variants["request_torch_%s_%s_%s" % (op, ax, name)] = request_torch
            if HAVE:
                imgs = [torch.empty(tuple(1 if j == axis else e for j, e in enumerate(it[2])), dtype=torch.float32, device=dev) for it in items]
                images["project_%s_%s_%s" % (op, ax, name)] = imgs
                preqs = tile_reqs(items, imgs)
                opts = sz3_amd._CProjectOpts()
                opts.op, opts.axis, opts.fill = sz3_amd._PROJECT_OPS[op], axis, float("nan")
                kept.append((preqs, opts))

                def project(preqs=preqs, opts=opts, n=n):
                    assert L.sz3hip_stream_project(st._h, preqs, n, C.byref(opts), handle) == 0
                variants["project_%s_%s_%s" % (op, ax, name)] = project

    for f in variants.values():  # warm-up: code objects, the handle's scratch and table
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    agrees, sum_diff = True, 0.0
    for name, items in screens.items():
        for v in [n for n in variants if n.endswith("_" + name) and not n.startswith("request_torch")]:
            l0 = sz3_amd.lib().sz3hip_debug_region_launches()
            variants[v]()
            info[v] = {"launches": int(sz3_amd.lib().sz3hip_debug_region_launches() - l0)}
        torch.cuda.synchronize()
        if not HAVE:
            continue
        for op, ax, axis in CASES:
            for (k, lo, ext), img in zip(items, images["project_%s_%s_%s" % (op, ax, name)]):
                want = full[tuple(slice(None, None, 1 << k) for _ in range(3))][tuple(slice(l, l + e) for l, e in zip(lo, ext))]
                if op == "max":
                    agrees = agrees and bool((img == torch.amax(want, dim=axis, keepdim=True)).all())
                else:
                    sum_diff = max(sum_diff, float((img - torch.sum(want, dim=axis, keepdim=True)).abs().max()))
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
    res = {"build": os.environ.get("LAB_TAG", "this"), "case": "C3", "shape": [S, S, S], "dtype": "float32", "abs_eb": 1e-4, "ratio": round(a.nbytes / size, 3),
           "points": {n: int(sum(np.prod(it[2]) for it in items)) for n, items in screens.items()},
           "runs": RUNS, "calls_per_run": CALLS, "project_call": HAVE, "project_max_equals_torch_amax": agrees if HAVE else None,
           "project_sum_max_abs_difference_to_torch_sum": sum_diff if HAVE else None,
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

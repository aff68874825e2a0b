#!/usr/bin/env python3
"""Gradients of boxes at C3 (512^3 f32, default algorithm, abs 1e-4) through an opened stream, on section 15's three
screens (tools/stream_lab.py). Every box's output goes into a contiguous array of its own:
  (a) gradient_deriv_z, gradient_deriv_x, gradient_mag, gradient_vector
                               one sz3hip_stream_gradient: the derivative along z (axis 0) and along x (axis 2, the fastest), the magnitude
                               and the vector, f32 outputs, spacing 1 (a box of level k: 2^k)
  (b) request_torch_deriv_z, ... what a caller issues without it: sz3hip_stream_request into contiguous f32 arrays, then per box
                               torch.gradient (edge_order=1, the spacing 2^level) along the axis — along all three with torch.stack for the
                               vector, and torch.linalg.vector_norm over the stack for the magnitude
  (c) request                  sz3hip_stream_request alone: the existing path, to set against the parent commit's package
One JSON line (LAB_WRITE=<file> appends it there: profiles/r26_gradient.txt holds the lines of the measurement in section 23). Protocol:
tools/stream_lab.py's — a run is CALLS calls between two device synchronisations, the variants alternate, seven runs each, the figure is the
median (us per call) with the runs' min and max; the chain is off. Every output is compared with torch.gradient over the full decode's slice:
the largest absolute difference is reported (torch computes in f32; the call in double, rounded once).
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package has no gradient and runs (b) and (c) alone. Run it
under a time limit of its own (timeout -k 10 400 python tools/gradient_lab.py); LAB_SIZE=<n> takes n^3; LAB_TAG=<name> goes into the line as
"build"; LAB_GRADIENT=0 leaves the differentiating variants out of this tree's run too: a process with the parent's variants, for the
comparison of (c); LAB_REQUEST_ONLY=1 times (c) alone, without (a) and (b): a short process, for comparing builds of the library over many
alternating processes (each build a directory with a copy of sz3_amd/*.py and its libsz3hip.so, given as LAB_PKG)."""
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
HAVE = hasattr(sz3_amd.Stream, "gradient") and os.environ.get("LAB_GRADIENT", "1") != "0"
CASES = (("deriv_z", "deriv", 0), ("deriv_x", "deriv", 2), ("mag", "mag", 0), ("vector", "vector", 0))
if os.environ.get("LAB_REQUEST_ONLY") == "1":
    HAVE, CASES = False, ()


def torch_gradient(o, case, k):
    """what a caller computes from a request's tensor `o` of level k"""
    step = float(1 << k)
    if case.startswith("deriv"):
        return torch.gradient(o, spacing=step, dim=0 if case == "deriv_z" else 2, edge_order=1)[0]
    g = torch.stack(torch.gradient(o, spacing=step, dim=(0, 1, 2), edge_order=1), dim=-1)
    return g if case == "vector" else torch.linalg.vector_norm(g, dim=-1)


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

    # (torch.gradient needs two points along every axis it differentiates: the screens' boxes have them)
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
        assert all(min(it[2]) >= 2 for it in items)
        outs = [torch.empty(it[2], dtype=torch.float32, device=dev) for it in items]
        treqs = tile_reqs(items, outs)
        kept.append((outs, treqs))

        def request(treqs=treqs, n=n):
            assert L.sz3hip_stream_request(st._h, treqs, n, handle) == 0
        variants["request_%s" % name] = request
        for case, op, axis in CASES:
            def request_torch(f=request, outs=outs, items=items, case=case):
                f()
                return [torch_gradient(o, case, it[0]) for o, it in zip(outs, items)]
            variants["request_torch_%s_%s" % (case, name)] = request_torch
            if HAVE:
                imgs = [torch.empty(tuple(it[2]) + ((3,) if op == "vector" else ()), dtype=torch.float32, device=dev) for it in items]
                images["gradient_%s_%s" % (case, name)] = imgs
                greqs = tile_reqs(items, imgs)
                opts = sz3_amd._CGradientOpts()
                opts.op, opts.axis = sz3_amd._GRADIENT_OPS[op], axis
                opts.spacing[:] = (1.0, 1.0, 1.0, 1.0)
                kept.append((greqs, opts))

                def gradient(greqs=greqs, opts=opts, n=n):
                    assert L.sz3hip_stream_gradient(st._h, greqs, n, C.byref(opts), handle) == 0
                variants["gradient_%s_%s" % (case, name)] = gradient

    for f in variants.values():  # warm-up: code objects, the handle's scratch and table, torch's allocator
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    diff = 0.0
    for name, items in screens.items():
        for v in [n for n in variants if n.endswith("_" + name) and not n.startswith("request_torch")]:
            l0 = sz3_amd.lib().sz3hip_debug_region_launches()
            variants[v]()
            info[v] = {"launches": int(sz3_amd.lib().sz3hip_debug_region_launches() - l0)}
        torch.cuda.synchronize()
        if not HAVE:
            continue
        for case, op, axis in CASES:
            for (k, lo, ext), img in zip(items, images["gradient_%s_%s" % (case, name)]):
                want = full[tuple(slice(None, None, 1 << k) for _ in range(3))][tuple(slice(l, l + e) for l, e in zip(lo, ext))]
                diff = max(diff, float((img - torch_gradient(want, case, k)).abs().max()))
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
           "runs": RUNS, "calls_per_run": CALLS, "gradient_call": HAVE, "gradient_max_abs_difference_to_torch_gradient": diff if HAVE else None,
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

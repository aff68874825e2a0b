#!/usr/bin/env python3
"""Boxes sampled at fractional positions at C3 (512^3 f32, default algorithm, abs 1e-4) through an opened stream, on
section 15's three screens (tools/stream_lab.py). Every screen's boxes share 512 x 512 lattice queries (an oblique plane through each box:
rows along y, columns along x, z rising with both) and 2^20 seeded random points inside the boxes:
  (a) sample_lattice, sample_points   one sz3hip_stream_sample, linear, of the lattices / of the points (f32 coordinates on the device);
      sample_nearest_points           the points with the nearest filter
  (b) request_grid_lattice, ..._points what a caller issues without it: sz3hip_stream_request into contiguous f32 arrays, then per box
                                       torch.nn.functional.grid_sample (bilinear, align_corners) over normalised coordinates made in front
  (c) request                         sz3hip_stream_request alone: the existing path, to set against the parent commit's package
One JSON line (LAB_WRITE=<file> appends it there: profiles/r23_sample.txt holds the lines of the measurement in section 20). Protocol:
tools/stream_lab.py's — a run is CALLS calls between two device synchronisations, the variants alternate, seven runs each, the figure is the
median (us per call) with the runs' min and max; the chain is off. Every variant calls the C face over structs and outputs made once, so
that a figure is the call's and not a Python wrapper's. The results of (a) are compared with (b)'s: grid_sample works in f32, so the line
holds the largest difference, not an equality.
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package has no sample and runs (b) and (c) alone. Run it
under a time limit of its own (timeout -k 10 400 python tools/sample_lab.py); LAB_SIZE=<n> takes n^3; LAB_TAG=<name> goes into the line as
"build"; LAB_SAMPLE=0 leaves the sample variants out of this tree's run too: a process with the parent's variants, for the comparison of (c)."""
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
HAVE_SAMPLE = hasattr(sz3_amd.Stream, "sample") and os.environ.get("LAB_SAMPLE", "1") != "0"
SIDE, POINTS = 512, 1 << 20


def lattice_of(ext, side):
    """an oblique side x side plane through a box: (origin, steps, counts), rows along y, columns along x, z rising along both"""
    e = [float(v - 1) for v in ext]
    return ([0.1 * e[0], 0.0, 0.0], [[0.35 * e[0] / (side - 1), e[1] / (side - 1), 0.0], [0.45 * e[0] / (side - 1), 0.0, e[2] / (side - 1)]], (side, side))


def lattice_coords(lat, dev):
    origin, steps, counts = lat
    i = torch.arange(counts[0], dtype=torch.float64, device=dev).reshape(-1, 1, 1)
    j = torch.arange(counts[1], dtype=torch.float64, device=dev).reshape(1, -1, 1)
    o, s0, s1 = [torch.tensor(v, dtype=torch.float64, device=dev) for v in (origin, steps[0], steps[1])]
    return (o + i * s0) + j * s1  # (rows, columns, 3), in box points


def normalised(c, ext):
    """grid_sample's coordinates of box-local points c (..., 3) in (z, y, x): x, y, z in [-1, 1], align_corners"""
    e = torch.tensor([float(v - 1) for v in ext], dtype=torch.float64, device=c.device)
    return (c / e * 2.0 - 1.0).flip(-1).to(torch.float32)


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
    grid_sample = torch.nn.functional.grid_sample

    variants, info, checks, kept = {}, {}, {}, []
    for name, items in requests().items():
        if name == "frame":
            continue
        n = len(items)
        m = int(round(n ** 0.5))
        side, per = SIDE // m, POINTS // n
        outs = [torch.empty(it[2], dtype=torch.float32, device=dev) for it in items]
        lats = [lattice_of(it[2], side) for it in items]
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        pts = [torch.rand((per, 3), generator=gen, device=dev, dtype=torch.float32) * torch.tensor([float(v - 1) for v in it[2]], device=dev) for it in items]
        g_lat = [normalised(lattice_coords(lat, dev), it[2]).reshape(1, 1, side, side, 3) for lat, it in zip(lats, items)]
        g_pts = [normalised(p.double(), it[2]).reshape(1, 1, 1, per, 3) for p, it in zip(pts, items)]

        # every variant calls the C face over structs built once: the figures are the calls', not the Python wrappers'
        L, C, handle = sz3_amd.lib(), sz3_amd.C, sz3_amd._stream_handle(dev, None)
        treqs = (sz3_amd._CTileReq * n)()
        for r, it, o in zip(treqs, items, outs):
            r.level = it[0]
            r.box.lo[:3], r.box.ext[:3] = it[1], it[2]
            r.d_out = o.data_ptr()
        kept.append((outs, pts, g_lat, g_pts, treqs))

        def request(treqs=treqs, n=n):
            assert L.sz3hip_stream_request(st._h, treqs, n, handle) == 0

        def request_grid(grids, f=request, outs=outs):
            f()
            return [grid_sample(o[None, None], g, mode="bilinear", padding_mode="zeros", align_corners=True) for o, g in zip(outs, grids)]
        variants["request_%s" % name] = request
        variants["request_grid_lattice_%s" % name] = lambda g=g_lat, f=request_grid: f(g)
        variants["request_grid_points_%s" % name] = lambda g=g_pts, f=request_grid: f(g)
        if HAVE_SAMPLE:
            for kind, queries, mode in (("lattice", lats, "linear"), ("points", pts, "linear"), ("nearest_points", pts, "nearest")):
                sreqs, _, cname, shapes = sz3_amd._sample_reqs(3, items, queries)
                souts = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in shapes]
                for r, o in zip(sreqs, souts):
                    r.d_out = o.data_ptr()
                opts = sz3_amd._sample_opts(mode, False, float("nan"), cname)
                kept.append((sreqs, souts, opts))

                def sample(sreqs=sreqs, souts=souts, opts=opts, n=n):
                    assert L.sz3hip_stream_sample(st._h, sreqs, n, C.byref(opts), handle) == 0
                    return souts
                variants["sample_%s_%s" % (kind, name)] = sample

    for f in variants.values():  # warm-up: code objects, the handle's scratch and table
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    for v, f in variants.items():
        if "_grid_" in v:
            continue
        l0 = sz3_amd.lib().sz3hip_debug_region_launches()
        f()
        info[v] = {"launches": int(sz3_amd.lib().sz3hip_debug_region_launches() - l0)}
    torch.cuda.synchronize()
    if HAVE_SAMPLE:
        for name in [n[len("sample_lattice_"):] for n in variants if n.startswith("sample_lattice_")]:
            for kind in ("lattice", "points"):
                got = variants["sample_%s_%s" % (kind, name)]()
                ref = variants["request_grid_%s_%s" % (kind, name)]()
                torch.cuda.synchronize()
                checks["%s_%s" % (kind, name)] = max(float((g.reshape(-1).double() - r.reshape(-1).double()).abs().max()) for g, r in zip(got, ref))
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
           "queries": {"lattice": SIDE * SIDE, "points": POINTS}, "runs": RUNS, "calls_per_run": CALLS, "sample_call": HAVE_SAMPLE,
           "max_abs_difference_to_grid_sample": checks if HAVE_SAMPLE else None,
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

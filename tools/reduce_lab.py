#!/usr/bin/env python3
"""Numbers about boxes at C3 (512^3 f32, default algorithm, abs 1e-4) through an opened stream, on section 15's three
screens (tools/stream_lab.py) and section 16's frame (tools/request_lab.py):
  (a) reduce, reduce_hist256   one sz3hip_stream_reduce, without and with a 256-bin histogram
  (b) request_torch            what an analysis issues without it: sz3hip_stream_request into contiguous arrays, then torch amin / amax / sum
                               per box (three framework reductions per box; no variance, no indices, no histogram — the cheapest stand-in)
  (c) request                  sz3hip_stream_request alone: the existing path, to set against the parent commit's package
One JSON line (LAB_WRITE=<file> appends it there: profiles/r18_reduce.txt holds the lines of the measurement in section 17). Protocol:
tools/stream_lab.py's — a run is CALLS calls between two device synchronisations, the variants alternate, seven runs each, the figure is the
median (us per call) with the runs' min and max; the chain is off. The reduce's min / max of every box are compared with torch's over the
full decode's slice, its counts with the box's size.
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package has no reduce and runs (b) and (c) alone. Run it under
a time limit of its own (timeout -k 10 400 python tools/reduce_lab.py); LAB_SIZE=<n> takes n^3; LAB_TAG=<name> goes into the line as "build"."""
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

S = int(os.environ.get("LAB_SIZE", "512"))
RUNS, CALLS = 7, 10
HAVE_REDUCE = hasattr(sz3_amd.Stream, "reduce")


def requests():
    """name -> (level, lo, shape) items: the three screens of section 15, the frame of section 16"""
    out = {}
    for name, k, e, m in (("L0_4x4_64", 0, S // 8, 4), ("L1_4x4_64", 1, S // 8, 4), ("L0_2x2_128", 0, S // 4, 2)):
        G = ((S - 1) >> k) + 1
        z = (G - e) // 2 + 1
        o = (G - m * e) // 2
        out[name] = [(k, (z, o + i * e, o + j * e), (e, e, e)) for i in range(m) for j in range(m)]
    e0, e1 = S // 4, S // 8
    c0 = (S - e0) // 2 + 1
    G1 = ((S - 1) >> 1) + 1
    c1 = (G1 - 2 * e1) // 2 + 1
    G3 = ((S - 1) >> 3) + 1
    frame = [(0, (c0, c0, c0), (e0, e0, e0))]
    frame += [(1, (c1, c1 + i * e1, c1 + j * e1), (e1, e1, e1)) for i in range(2) for j in range(2)]
    frame.append((3, (0, 0, 0), (G3, G3, G3)))
    out["frame"] = frame
    return out


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
    lo_h, hi_h = float(full.min()), float(full.max())

    variants, info, kept = {}, {}, {}
    for name, items in requests().items():
        outs = [torch.empty(it[2], dtype=torch.float32, device=dev) for it in items]
        with_outs = [it + (o,) for it, o in zip(items, outs)]

        def request(with_outs=with_outs):
            st.request(with_outs)

        def request_torch(with_outs=with_outs, outs=outs, name=name):
            st.request(with_outs)
            kept[name] = [(o.amin(), o.amax(), o.sum()) for o in outs]
        variants["request_%s" % name] = request
        variants["request_torch_%s" % name] = request_torch
        if HAVE_REDUCE:
            def reduce(items=items, name=name):
                kept["reduce_" + name] = st.reduce(items)

            def reduce_hist(items=items, name=name):
                kept["hist_" + name] = st.reduce(items, 256, lo_h, hi_h)
            variants["reduce_%s" % name] = reduce
            variants["reduce_hist256_%s" % name] = reduce_hist

    for f in variants.values():  # warm-up: code objects, the handle's scratch and table
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    agrees = True
    for name, items in requests().items():
        l0 = sz3_amd.lib().sz3hip_debug_region_launches()
        variants["request_%s" % name]()
        info["request_%s" % name] = {"launches": int(sz3_amd.lib().sz3hip_debug_region_launches() - l0)}
        if not HAVE_REDUCE:
            continue
        for v in ("reduce_%s" % name, "reduce_hist256_%s" % name):
            l0 = sz3_amd.lib().sz3hip_debug_region_launches()
            variants[v]()
            info[v] = {"launches": int(sz3_amd.lib().sz3hip_debug_region_launches() - l0)}
        torch.cuda.synchronize()
        stt, hist = kept["hist_" + name].numpy()
        for i, (k, lo, ext) in enumerate(items):
            want = full[tuple(slice(None, None, 1 << k) for _ in range(3))][tuple(slice(l, l + e) for l, e in zip(lo, ext))]
            agrees = agrees and float(stt[i]["min"]) == float(want.min()) and float(stt[i]["max"]) == float(want.max())
            agrees = agrees and int(stt[i]["n"]) == want.numel() == int(hist[i].sum()) and int(stt[i]["n_nonfinite"]) == 0
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
           "runs": RUNS, "calls_per_run": CALLS, "reduce_call": HAVE_REDUCE, "reduce_agrees_with_full_slice": agrees if HAVE_REDUCE else None,
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

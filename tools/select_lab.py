#!/usr/bin/env python3
"""The points of boxes in a range at C3 (512^3 f32, default algorithm, abs 1e-4) through an opened stream, on section
15's three screens (tools/stream_lab.py) and section 16's frame (tools/request_lab.py). The range is the field's upper decile:
  (a) select, select_index     one sz3hip_stream_select with capacity = the box's points, with and without the values
  (b) request_nonzero          what an analysis issues without it: sz3hip_stream_request into contiguous arrays, then per box torch.nonzero over
                               the flattened mask and an indexed gather (a host synchronisation inside every nonzero)
  (c) request                  sz3hip_stream_request alone: the existing path, to set against the parent commit's package
  (d) reduce                   sz3hip_stream_reduce: the other existing sink, at both commits
One JSON line (LAB_WRITE=<file> appends it there: profiles/r19_select.txt holds the lines of the measurement in section 18). Protocol:
tools/stream_lab.py's — a run is CALLS calls between two device synchronisations, the variants alternate, seven runs each, the figure is the
median (us per call) with the runs' min and max; the chain is off. Every box's count, indices and values are compared with torch's over the
full decode's slice.
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package has no select and runs (b), (c) and (d) alone. Run it
under a time limit of its own (timeout -k 10 400 python tools/select_lab.py); LAB_SIZE=<n> takes n^3; LAB_TAG=<name> goes into the line as
"build"."""
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
HAVE_SELECT = hasattr(sz3_amd.Stream, "select")


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
    lo_r = float(torch.quantile(full.reshape(-1)[::97].double(), 0.9))  # the upper decile (of every 97th point: quantile's input is bounded)
    hi_r = float(full.max())

    variants, info, kept = {}, {}, {}
    for name, items in requests().items():
        outs = [torch.empty(it[2], dtype=torch.float32, device=dev) for it in items]
        with_outs = [it + (o,) for it, o in zip(items, outs)]
        caps = [int(np.prod(it[2])) for it in items]

        def request(with_outs=with_outs):
            st.request(with_outs)

        def request_nonzero(with_outs=with_outs, outs=outs, name=name):
            st.request(with_outs)
            res = []
            for o in outs:
                flat = o.reshape(-1)
                idx = torch.nonzero((flat >= lo_r) & (flat <= hi_r)).reshape(-1)
                res.append((idx, flat[idx]))
            kept["nonzero_" + name] = res

        def reduce(items=items, name=name):
            kept["reduce_" + name] = st.reduce(items)
        variants["request_%s" % name] = request
        variants["request_nonzero_%s" % name] = request_nonzero
        variants["reduce_%s" % name] = reduce
        if HAVE_SELECT:
            def select(items=items, name=name, caps=caps):
                kept["select_" + name] = st.select(items, lo_r, hi_r, caps)

            def select_index(items=items, name=name, caps=caps):
                kept["index_" + name] = st.select(items, lo_r, hi_r, caps, values=False)
            variants["select_%s" % name] = select
            variants["select_index_%s" % name] = select_index

    for f in variants.values():  # warm-up: code objects, the handle's scratch and table
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    agrees, selected = True, {}
    for name, items in requests().items():
        for v in ("request_%s" % name, "reduce_%s" % name) + (("select_%s" % name, "select_index_%s" % name) if HAVE_SELECT else ()):
            l0 = sz3_amd.lib().sz3hip_debug_region_launches()
            variants[v]()
            info[v] = {"launches": int(sz3_amd.lib().sz3hip_debug_region_launches() - l0)}
        variants["request_nonzero_%s" % name]()
        torch.cuda.synchronize()
        selected[name] = int(sum(ix.numel() for ix, _ in kept["nonzero_" + name]))
        if not HAVE_SELECT:
            continue
        got = kept["select_" + name].numpy()
        for i, (k, lo, ext) in enumerate(items):
            want = full[tuple(slice(None, None, 1 << k) for _ in range(3))][tuple(slice(l, l + e) for l, e in zip(lo, ext))].reshape(-1)
            idx = torch.nonzero((want >= lo_r) & (want <= hi_r)).reshape(-1)
            c, ix, val = got[i]
            agrees = agrees and c == idx.numel() and np.array_equal(ix, idx.cpu().numpy()) and val.tobytes() == want[idx].cpu().numpy().tobytes()
            ix2, val2 = kept["nonzero_" + name][i]
            agrees = agrees and np.array_equal(ix, ix2.cpu().numpy()) and val.tobytes() == val2.cpu().numpy().tobytes()
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
           "range": [lo_r, hi_r], "selected_points": selected, "points": {n: int(sum(np.prod(it[2]) for it in items)) for n, items in requests().items()},
           "runs": RUNS, "calls_per_run": CALLS, "select_call": HAVE_SELECT, "select_agrees_with_full_slice": agrees if HAVE_SELECT else None,
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

#!/usr/bin/env python3
"""Texels out of a request at C3 (512^3 f32, default algorithm, abs 1e-4) through an opened stream, on section 15's
three screens (tools/stream_lab.py) and section 16's frame (tools/request_lab.py). The window is the field's 5 % .. 95 % band; every box goes
into its rectangle of one atlas, the rectangles side by side along x:
  (a) map_u8, map_lut32        one sz3hip_stream_map into a uint8 / an int32 atlas (lut32: a 256-entry table); map_u16, map_f16 likewise;
      ..._plain                the same with the thread-per-point stores (Dbg2.MAP_PLAIN_STORES): the plain against the packed form
  (b) request_chain            what a caller issues without it: sz3hip_stream_request into contiguous f32 arrays, then per box the framework's
                               chain — subtract, multiply, clamp, NaN mask, cast to uint8, copy into the atlas rectangle
  (c) request                  sz3hip_stream_request alone: the existing path, to set against the parent commit's package
One JSON line (LAB_WRITE=<file> appends it there: profiles/r22_map.txt holds the lines of the measurement in section 19). Protocol:
tools/stream_lab.py's — a run is CALLS calls between two device synchronisations, the variants alternate, seven runs each, the figure is the
median (us per call) with the runs' min and max; the chain is off. Every u8 texel is compared with the rule in float64 over the full
decode's slice.
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package has no map and runs (b) and (c) alone. Run it under a
time limit of its own (timeout -k 10 400 python tools/map_lab.py); LAB_SIZE=<n> takes n^3; LAB_TAG=<name> goes into the line as "build";
LAB_MAP=0 leaves the map variants out of this tree's run too: a process with the parent's variants, for the comparison of (c)."""
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
HAVE_MAP = hasattr(sz3_amd.Stream, "map") and os.environ.get("LAB_MAP", "1") != "0"
OUT = {"u8": torch.uint8, "u16": torch.int16, "f16": torch.float16, "lut32": torch.int32}


def atlas_views(items, dtype, dev):
    dims = [max(it[2][0] for it in items), max(it[2][1] for it in items), sum(it[2][2] for it in items)]
    atlas = torch.zeros(dims, dtype=dtype, device=dev)
    views, x = [], 0
    for _, _, ext in items:
        views.append(atlas[:ext[0], :ext[1], x:x + ext[2]])
        x += ext[2]
    return atlas, views


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
    q = torch.quantile(full.reshape(-1)[::97].double(), torch.tensor([0.05, 0.95], dtype=torch.float64, device=dev))
    lo_w, hi_w = float(q[0]), float(q[1])
    scale32 = 256.0 / (hi_w - lo_w)
    lut = torch.from_numpy(np.random.default_rng(1).integers(0, 2 ** 31, 256).astype(np.int32)).to(dev)

    variants, info, kept = {}, {}, {}
    for name, items in requests().items():
        outs = [torch.empty(it[2], dtype=torch.float32, device=dev) for it in items]
        with_outs = [it + (o,) for it, o in zip(items, outs)]
        chain_atlas, chain_views = atlas_views(items, torch.uint8, dev)
        kept["chain_" + name] = chain_atlas

        def request(with_outs=with_outs):
            st.request(with_outs)

        def request_chain(with_outs=with_outs, outs=outs, views=chain_views):
            st.request(with_outs)
            for o, v in zip(outs, views):
                c = ((o - lo_w) * scale32).clamp_(0.0, 255.0)
                c.masked_fill_(torch.isnan(o), 0.0)
                v.copy_(c.to(torch.uint8))
        variants["request_%s" % name] = request
        variants["request_chain_%s" % name] = request_chain
        if HAVE_MAP:
            for t in ("u8", "u16", "f16", "lut32"):
                atlas, views = atlas_views(items, OUT[t], dev)
                kept["%s_%s" % (t, name)] = atlas
                kw = {} if t == "f16" else dict(lo=lo_w, hi=hi_w, lut=lut if t == "lut32" else None)
                mapped = [it + (v,) for it, v in zip(items, views)]
                for flags, suffix in ((0, ""), (int(sz3_amd.Dbg2.MAP_PLAIN_STORES), "_plain")):
                    if t == "lut32" and flags:
                        continue  # (a four-byte texel has one form)

                    def run(mapped=mapped, t=t, kw=kw, flags=flags):
                        sz3_amd.lib().sz3hip_debug_flags2(flags)
                        st.map(mapped, t, **kw)
                        sz3_amd.lib().sz3hip_debug_flags2(0)
                    variants["map_%s%s_%s" % (t, suffix, name)] = run

    for f in variants.values():  # warm-up: code objects, the handle's scratch and table
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    agrees = True
    for name, items in requests().items():
        for v in [n for n in variants if n.endswith("_" + name) and not n.startswith("request_chain")]:
            l0 = sz3_amd.lib().sz3hip_debug_region_launches()
            variants[v]()
            info[v] = {"launches": int(sz3_amd.lib().sz3hip_debug_region_launches() - l0)}
        torch.cuda.synchronize()
        if not HAVE_MAP:
            continue
        for form in ("map_u8_%s" % name, "map_u8_plain_%s" % name):
            kept["u8_" + name].zero_()
            variants[form]()
            torch.cuda.synchronize()
            x0 = 0
            for k, lo, ext in items:
                want = full[tuple(slice(None, None, 1 << k) for _ in range(3))][tuple(slice(l, l + e) for l, e in zip(lo, ext))].double()
                code = ((want - lo_w) * (256.0 / (hi_w - lo_w))).clamp(0.0, 255.0).to(torch.uint8)  # (truncation: the floor of a value that is not negative)
                code = torch.where(want < lo_w, torch.zeros_like(code), torch.where(want >= hi_w, torch.full_like(code, 255), code))
                agrees = agrees and bool((kept["u8_" + name][:ext[0], :ext[1], x0:x0 + ext[2]] == code).all())
                x0 += ext[2]
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
           "window": [lo_w, hi_w], "points": {n: int(sum(np.prod(it[2]) for it in items)) for n, items in requests().items()},
           "runs": RUNS, "calls_per_run": CALLS, "map_call": HAVE_MAP, "map_u8_agrees_with_full_slice": agrees if HAVE_MAP else None,
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

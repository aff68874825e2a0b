#!/usr/bin/env python3
"""Region decode against the full decode at C3 (512^3 f32, default algorithm, abs 1e-4), through the device context. One JSON line.

Variants: the full decode (sz3hip_decompress_device) and the region decode (sz3hip_decompress_device_region) of centred and corner boxes of
64^3, 128^3 and 256^3 and of one full x-y plane. A run is CALLS calls between two device synchronisations; the variants alternate, seven
runs each, and the figure is the median (us per call) with the runs' min and max beside it. Beside each box: the plan's predicted points and
scratch elements, and the stage split (Huffman stage, reconstruction) from sz3hip_get_stage_times in runs of its own, with the Huffman
stage's share of the two. Run it under a time limit of its own (timeout -k 10 300 python tools/region_lab.py); LAB_SIZE=<n> takes n^3."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sz3_amd  # noqa: E402
from fields import field3d  # noqa: E402

S = int(os.environ.get("LAB_SIZE", "512"))
RUNS, CALLS = 7, 10


def boxes():
    out = {}
    for e in (S // 8, S // 4, S // 2):
        c = (S - e) // 2 + 1  # (odd where S / 2 is even: the box's faces are not on the coarse lattices)
        out["centre_%d" % e] = ((c, c, c), (e, e, e))
        out["corner_%d" % e] = ((0, 0, 0), (e, e, e))
    out["plane_xy"] = ((S // 2 + 1, 0, 0), (1, S, S))
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

    variants = {"full": lambda: dc.decompress(pl.data_ptr(), size, full.data_ptr(), s)}
    outs, plans = {}, {}
    bx = boxes()
    for n, (lo, ext) in bx.items():
        outs[n] = torch.empty(ext, dtype=torch.float32, device=dev)
        p = sz3_amd.region_plan(conf, lo, ext)
        plans[n] = {"lo": list(lo), "shape": list(ext), "points": p["points"], "scratch_elems": p["scratch_elems"], "n_levels": p["n_levels"]}
        variants[n] = (lambda n=n, lo=lo, ext=ext: dc.decompress_region(pl.data_ptr(), size, lo, ext, outs[n].data_ptr(), s))

    for f in variants.values():  # warm-up: code objects, the context's lazy buffers
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    identical = all(bool(torch.equal(outs[n], full[tuple(slice(l, l + e) for l, e in zip(*bx[n]))])) for n in bx)
    times = {n: [] for n in variants}
    for _ in range(RUNS):
        for n, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / CALLS * 1e6)
    stages = {}
    dc.set_profiling(True)
    for n, f in variants.items():
        h, r = [], []
        for _ in range(RUNS):
            f()
            torch.cuda.synchronize()
            t = dc.stage_times()
            h.append(1e3 * t.get("huffman_decode", 0.0))
            r.append(1e3 * t.get("reconstruct", 0.0))
        hm, rm = float(np.median(h)), float(np.median(r))
        stages[n] = {"huffman_decode_us": round(hm, 1), "reconstruct_us": round(rm, 1), "huffman_share": round(hm / (hm + rm), 3) if hm + rm > 0 else None}
    dc.set_profiling(False)
    res = {"case": "C3", "shape": [S, S, S], "dtype": "float32", "abs_eb": 1e-4, "ratio": round(a.nbytes / size, 3), "runs": RUNS, "calls_per_run": CALLS,
           "bit_identical_to_full_slice": identical, "region_scratch_elems": dc.region_scratch(),
           "us_per_call": {n: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in times.items()},
           "stages": stages, "plans": plans}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

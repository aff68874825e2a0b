#!/usr/bin/env python3
"""Tile decode at C3 (512^3 f32, default algorithm, abs 1e-4), through the device context. One JSON line (LAB_WRITE=<file> appends it there:
profiles/r10_tile_decode.txt holds the lines of the measurement in DESIGN.md section 13).

Variants: the full decode; centred and corner boxes of 64^3, 128^3 and 256^3 at level 0, each with sparse decode on and off
(sz3hip_set_sparse_decode); the same boxes' coarse counterparts at levels 1 and 2 (a 64^3 tile of the level-1 grid, and so on); the
whole-array box. A run is CALLS calls between two device synchronisations; the variants alternate, seven runs each, and the figure is the
median (us per call) with the runs' min and max beside it. Beside each box: units needed and total, the host time of the list build alone
(sz3hip_tile_units_for, median of seven), and the stage split (Huffman stage, reconstruction) from sz3hip_get_stage_times in runs of its own.
A library without the tile calls (the parent commit's) runs the level-0 boxes through sz3hip_decompress_device_region: the A side of an A/B.
Run it under a time limit of its own (timeout -k 10 400 python tools/tile_lab.py); LAB_SIZE=<n> takes n^3."""
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
HAVE_TILE = hasattr(sz3_amd, "decompress_tile")


def boxes():
    out = {}
    for k in ((0, 1, 2) if HAVE_TILE else (0,)):
        G = ((S - 1) >> k) + 1
        for e in (S // 8, S // 4, S // 2):
            if e > G:
                continue
            c = (G - e) // 2 + 1 if e < G else 0  # (odd where G / 2 is even: the box's faces are not on the coarse lattices)
            out["L%d_centre_%d" % (k, e)] = (k, (c, c, c), (e, e, e))
            if e < G:
                out["L%d_corner_%d" % (k, e)] = (k, (0, 0, 0), (e, e, e))
        if k == 0:
            out["L0_whole"] = (0, (0, 0, 0), (S, S, S))  # (behind the largest boxes in either library's run: the same load in front of it)
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

    def sparse(on):
        if HAVE_TILE:
            sz3_amd.set_sparse_decode(on)

    variants = {"full": lambda: dc.decompress(pl.data_ptr(), size, full.data_ptr(), s)}
    outs, plans, build_us = {}, {}, {}
    bx = boxes()
    for n, (k, lo, ext) in bx.items():
        outs[n] = torch.empty(ext, dtype=torch.float32, device=dev)
        if HAVE_TILE:
            p = sz3_amd.tile_plan(conf, k, lo, ext)
            plans[n] = {"level": k, "lo": list(lo), "shape": list(ext), "points": p["region"]["points"], "units_needed": p["units_needed"], "units_total": p["units_total"]}
            t = []
            for _ in range(RUNS):
                t0 = time.perf_counter()
                sz3_amd.tile_units(conf, k, lo, ext)
                t.append((time.perf_counter() - t0) * 1e6)
            build_us[n] = round(float(np.median(t)), 1)
            variants[n] = (lambda n=n, k=k, lo=lo, ext=ext: dc.decompress_tile(pl.data_ptr(), size, k, lo, ext, outs[n].data_ptr(), s))
            if k == 0:
                def dense(n=n, lo=lo, ext=ext):
                    sparse(0)
                    dc.decompress_tile(pl.data_ptr(), size, 0, lo, ext, outs[n].data_ptr(), s)
                    sparse(1)
                variants[n + "_dense"] = dense
        else:
            variants[n] = (lambda n=n, lo=lo, ext=ext: dc.decompress_region(pl.data_ptr(), size, lo, ext, outs[n].data_ptr(), s))

    for f in variants.values():  # warm-up: code objects, the context's lazy buffers
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    identical = True
    for n, (k, lo, ext) in bx.items():  # (after a full decode of the context: the stale codes are this container's own — the tests cover the rest)
        variants[n]()
        torch.cuda.synchronize()
        cv = full[tuple(slice(None, None, 1 << k) for _ in range(3))]
        identical = identical and bool(torch.equal(outs[n], cv[tuple(slice(l, l + e) for l, e in zip(lo, ext))]))
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
        stages[n] = {"huffman_decode_us": round(float(np.median(h)), 1), "reconstruct_us": round(float(np.median(r)), 1)}
    dc.set_profiling(False)
    res = {"case": "C3", "shape": [S, S, S], "dtype": "float32", "abs_eb": 1e-4, "ratio": round(a.nbytes / size, 3), "runs": RUNS, "calls_per_run": CALLS,
           "tile_calls": HAVE_TILE, "bit_identical_to_full_slice": identical,
           "us_per_call": {n: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in times.items()},
           "stages": stages, "list_build_us": build_us, "plans": plans}
    line = json.dumps(res)
    print(line)
    if os.environ.get("LAB_WRITE"):
        with open(os.environ["LAB_WRITE"], "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Several tiles in one call at C3 (512^3 f32, default algorithm, abs 1e-4): a screenful of tiles through n single-box calls against one
multi-box call. One JSON line (LAB_WRITE=<file> appends it there: profiles/r14_tiles.txt holds the lines of the
measurement in section 14).

Screens: 4 x 4 tiles of 64^3 at level 0 and at level 1, 2 x 2 tiles of 128^3 at level 0 — one plane of tiles, centred in the slowest
dimension. Through the device context (sz3hip_decompress_device_tile n times / sz3hip_decompress_device_tiles once) and through the container
calls (sz3hip_decompress_tile_to_device n times / sz3hip_decompress_tiles_to_device once). Beside them the single-box variants of
tools/tile_lab.py (section 13's table), which this change must leave where they were. A run is CALLS calls (of a whole screen, where the
variant is one) between two device synchronisations; the variants alternate, seven runs each; the figure is the median (us per call) with
the runs' min and max. The stage split (Huffman stage, reconstruction; summed over a screen's calls) comes from sz3hip_get_stage_times in
runs of its own. Every box is compared with the full decode's slice.
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package is the A side of an A/B; a package without the
multi-box call runs the single-box variants alone. Run it under a time limit of its own (timeout -k 10 500 python tools/tiles_lab.py);
LAB_SIZE=<n> takes n^3; LAB_TAG=<name> goes into the line as "build"."""
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
HAVE_MULTI = hasattr(sz3_amd, "decompress_tiles")


def screens():
    out = {}
    for name, k, e, m in (("L0_4x4_64", 0, S // 8, 4), ("L1_4x4_64", 1, S // 8, 4), ("L0_2x2_128", 0, S // 4, 2)):
        G = ((S - 1) >> k) + 1
        z = (G - e) // 2 + 1
        o = (G - m * e) // 2
        out[name] = (k, [((z, o + i * e, o + j * e), (e, e, e)) for i in range(m) for j in range(m)])
    return out


def single_boxes():
    out = {}
    for k in (0, 1, 2):
        G = ((S - 1) >> k) + 1
        for e in (S // 8, S // 4, S // 2):
            if e > G:
                continue
            c = (G - e) // 2 + 1 if e < G else 0
            out["L%d_centre_%d" % (k, e)] = (k, (c, c, c), (e, e, e))
            if e < G:
                out["L%d_corner_%d" % (k, e)] = (k, (0, 0, 0), (e, e, e))
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
    blob = sz3_amd.compress(a, conf)[0].copy()

    variants = {"full": lambda: dc.decompress(pl.data_ptr(), size, full.data_ptr(), s)}
    checks, plans = [], {}
    for n, (k, lo, ext) in single_boxes().items():
        out = torch.empty(ext, dtype=torch.float32, device=dev)
        variants[n] = (lambda k=k, lo=lo, ext=ext, out=out: dc.decompress_tile(pl.data_ptr(), size, k, lo, ext, out.data_ptr(), s))
        checks.append((n, k, [(lo, ext)], [out]))
    for n, (k, bx) in screens().items():
        for path in ("ctx", "blob"):
            outs = [torch.empty(ext, dtype=torch.float32, device=dev) for _, ext in bx]
            if path == "ctx":
                def singles(k=k, bx=bx, outs=outs):
                    for (lo, ext), o in zip(bx, outs):
                        dc.decompress_tile(pl.data_ptr(), size, k, lo, ext, o.data_ptr(), s)
            else:
                def singles(k=k, bx=bx, outs=outs):
                    for (lo, ext), o in zip(bx, outs):
                        sz3_amd.decompress_tile(blob, np.float32, k, lo, ext, out=o)
            variants["%s_%s_singles" % (path, n)] = singles
            checks.append(("%s_%s_singles" % (path, n), k, bx, outs))
            if HAVE_MULTI:
                mouts = [torch.empty(ext, dtype=torch.float32, device=dev) for _, ext in bx]
                ptrs = [o.data_ptr() for o in mouts]
                if path == "ctx":
                    variants["ctx_%s_multi" % n] = (lambda k=k, bx=bx, ptrs=ptrs: dc.decompress_tiles(pl.data_ptr(), size, k, bx, ptrs, s))
                else:
                    variants["blob_%s_multi" % n] = (lambda k=k, bx=bx, mouts=mouts: sz3_amd.decompress_tiles(blob, np.float32, k, bx, out=mouts))
                checks.append(("%s_%s_multi" % (path, n), k, bx, mouts))
        if HAVE_MULTI:
            p = sz3_amd.tiles_plan(conf, k, bx)
            plans[n] = dict(p, level=k, units_needed_summed=sum(sz3_amd.tile_plan(conf, k, lo, ext)["units_needed"] for lo, ext in bx))

    for f in variants.values():  # warm-up: code objects, the context's lazy buffers
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    identical = True
    for n, k, bx, outs in checks:
        for o in outs:
            o.fill_(77.0)
        variants[n]()
        torch.cuda.synchronize()
        cv = full[tuple(slice(None, None, 1 << k) for _ in range(3))]
        for (lo, ext), o in zip(bx, outs):
            identical = identical and bool(torch.equal(o, cv[tuple(slice(l, l + e) for l, e in zip(lo, ext))]))
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
    tmp = torch.empty((S // 4,) * 3, dtype=torch.float32, device=dev)
    dc.set_profiling(True)
    for n, f in variants.items():
        if not n.startswith("ctx_"):
            continue
        k, bx = screens()[n[4:].rsplit("_", 1)[0]]
        h, r = [], []
        for _ in range(RUNS):
            hs = rs = 0.0
            if n.endswith("_multi"):
                f()
                torch.cuda.synchronize()
                t = dc.stage_times()
                hs, rs = t.get("huffman_decode", 0.0), t.get("reconstruct", 0.0)
            else:  # (the stage times are the last call's: one call at a time, summed over the screen)
                for lo, ext in bx:
                    dc.decompress_tile(pl.data_ptr(), size, k, lo, ext, tmp.data_ptr(), s)
                    torch.cuda.synchronize()
                    t = dc.stage_times()
                    hs += t.get("huffman_decode", 0.0)
                    rs += t.get("reconstruct", 0.0)
            h.append(1e3 * hs)
            r.append(1e3 * rs)
        stages[n] = {"huffman_decode_us": round(float(np.median(h)), 1), "reconstruct_us": round(float(np.median(r)), 1)}
    dc.set_profiling(False)
    res = {"build": os.environ.get("LAB_TAG", "this"), "case": "C3", "shape": [S, S, S], "dtype": "float32", "abs_eb": 1e-4, "ratio": round(a.nbytes / size, 3), "runs": RUNS, "calls_per_run": CALLS,
           "multi_calls": HAVE_MULTI, "bit_identical_to_full_slice": identical,
           "us_per_call": {n: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in times.items()},
           "stages": stages, "plans": plans}
    line = json.dumps(res)
    print(line)
    if os.environ.get("LAB_WRITE"):
        with open(os.environ["LAB_WRITE"], "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""An opened stream at C3 (512^3 f32, default algorithm, abs 1e-4): a screenful of tiles through the multi-box calls against a request of a
handle. One JSON line (LAB_WRITE=<file> appends it there: profiles/r15_stream.txt holds the lines of the measurement in
section 15). Protocol and screens are tools/tiles_lab.py's, so the lines compare with profiles/r14_tiles.txt.

Screens: 4 x 4 tiles of 64^3 at level 0 and at level 1, 2 x 2 tiles of 128^3 at level 0 — one plane of tiles, centred in the slowest
dimension. Variants per screen: the container multi call (sz3hip_decompress_tiles_to_device), the context multi call
(sz3hip_decompress_device_tiles), and — where the package has them — the handle's request with the chain off and at 2048, 8192 and 32768
points. Beside them: open itself (open + close of the container's handle) against one full decompress_to_device of the container, a single
centred 64^3 tile through the handle against sz3hip_decompress_device_tile, and the full device decode. A run is CALLS calls between two
device synchronisations; the variants alternate, seven runs each; the figure is the median (us per call) with the runs' min and max. The
stage split comes in runs of its own: sz3hip_get_stage_times for the context's call, a pair of events around one request for the handle (a
request IS the reconstruction). Every box is compared with the full decode's slice.
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package is the A side of an A/B; a package without the
handle runs the existing calls alone. Run it under a time limit of its own (timeout -k 10 500 python tools/stream_lab.py); LAB_SIZE=<n>
takes n^3; LAB_TAG=<name> goes into the line as "build"."""
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
HAVE_STREAM = hasattr(sz3_amd, "open_stream")
CHAINS = (0, 2048, 8192, 32768)


def screens():
    out = {}
    for name, k, e, m in (("L0_4x4_64", 0, S // 8, 4), ("L1_4x4_64", 1, S // 8, 4), ("L0_2x2_128", 0, S // 4, 2)):
        G = ((S - 1) >> k) + 1
        z = (G - e) // 2 + 1
        o = (G - m * e) // 2
        out[name] = (k, [((z, o + i * e, o + j * e), (e, e, e)) for i in range(m) for j in range(m)])
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
    whole = torch.empty_like(d_in)
    st = dc.open_stream(pl.data_ptr(), size, s) if HAVE_STREAM else None

    variants = {"full": lambda: dc.decompress(pl.data_ptr(), size, full.data_ptr(), s),
                "blob_decompress_to_device": lambda: sz3_amd.decompress(blob, np.float32, out=whole)}
    checks, info = [], {}
    G = S
    c = (G - S // 8) // 2 + 1
    tile = (0, (c, c, c), (S // 8,) * 3)
    t_ctx = torch.empty(tile[2], dtype=torch.float32, device=dev)
    variants["ctx_tile_L0_centre_64"] = lambda: dc.decompress_tile(pl.data_ptr(), size, tile[0], tile[1], tile[2], t_ctx.data_ptr(), s)
    checks.append(("ctx_tile_L0_centre_64", 0, [(tile[1], tile[2])], [t_ctx]))
    if HAVE_STREAM:
        def opened():
            h = sz3_amd.open_stream(blob, np.float32, device=dev)
            h.close()
        variants["blob_open_close"] = opened
        t_st = torch.empty(tile[2], dtype=torch.float32, device=dev)

        def stream_tile():
            sz3_amd.set_chain_points(0)
            st.tile(tile[0], tile[1], tile[2], out=t_st)
        variants["stream_tile_L0_centre_64"] = stream_tile
        checks.append(("stream_tile_L0_centre_64", 0, [(tile[1], tile[2])], [t_st]))
    for n, (k, bx) in screens().items():
        mouts = [torch.empty(ext, dtype=torch.float32, device=dev) for _, ext in bx]
        ptrs = [o.data_ptr() for o in mouts]
        variants["ctx_%s_multi" % n] = (lambda k=k, bx=bx, ptrs=ptrs: dc.decompress_tiles(pl.data_ptr(), size, k, bx, ptrs, s))
        checks.append(("ctx_%s_multi" % n, k, bx, mouts))
        bouts = [torch.empty(ext, dtype=torch.float32, device=dev) for _, ext in bx]
        variants["blob_%s_multi" % n] = (lambda k=k, bx=bx, bouts=bouts: sz3_amd.decompress_tiles(blob, np.float32, k, bx, out=bouts))
        checks.append(("blob_%s_multi" % n, k, bx, bouts))
        if HAVE_STREAM:
            for pts in CHAINS:
                souts = [torch.empty(ext, dtype=torch.float32, device=dev) for _, ext in bx]

                def req(k=k, bx=bx, souts=souts, pts=pts):
                    sz3_amd.set_chain_points(pts)
                    st.tiles(k, bx, out=souts)
                variants["stream_%s_chain%d" % (n, pts)] = req
                checks.append(("stream_%s_chain%d" % (n, pts), k, bx, souts))

    for f in variants.values():  # warm-up: code objects, lazy buffers
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    identical = True
    for n, k, bx, outs in checks:
        for o in outs:
            o.fill_(77.0)
        variants[n]()
        torch.cuda.synchronize()
        if n.startswith("stream_") and "_chain" in n:
            stt = st.stats()
            info[n] = {q: stt[q] for q in ("launches_last_request", "chain_levels_last_request", "n_levels_last_request")}
        cv = full[tuple(slice(None, None, 1 << k) for _ in range(3))]
        for (lo, ext), o in zip(bx, outs):
            identical = identical and bool(torch.equal(o, cv[tuple(slice(l, l + e) for l, e in zip(lo, ext))]))
    identical = identical and bool(torch.equal(whole, full))
    times = {n: [] for n in variants}
    for _ in range(RUNS):
        for n, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / CALLS * 1e6)
    # the stage split, in runs of its own: one call at a time
    stages = {}
    dc.set_profiling(True)
    for n, f in variants.items():
        if n.startswith("ctx_") and n.endswith("_multi"):
            h, r = [], []
            for _ in range(RUNS):
                f()
                torch.cuda.synchronize()
                t = dc.stage_times()
                h.append(1e3 * t.get("huffman_decode", 0.0))
                r.append(1e3 * t.get("reconstruct", 0.0))
            stages[n] = {"huffman_decode_us": round(float(np.median(h)), 1), "reconstruct_us": round(float(np.median(r)), 1)}
        elif n.startswith("stream_"):
            d = []
            for _ in range(RUNS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                d.append(1e3 * e0.elapsed_time(e1))
            stages[n] = {"device_us": round(float(np.median(d)), 1)}
    dc.set_profiling(False)
    res = {"build": os.environ.get("LAB_TAG", "this"), "case": "C3", "shape": [S, S, S], "dtype": "float32", "abs_eb": 1e-4, "ratio": round(a.nbytes / size, 3), "runs": RUNS,
           "calls_per_run": CALLS, "stream_calls": HAVE_STREAM, "bit_identical_to_full_slice": identical,
           "us_per_call": {n: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in times.items()},
           "stages": stages, "requests": info, "stream_stats": st.stats() if st else None}
    if st:
        st.close()
    line = json.dumps(res)
    print(line)
    if os.environ.get("LAB_WRITE"):
        with open(os.environ["LAB_WRITE"], "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

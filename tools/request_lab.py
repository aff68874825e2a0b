#!/usr/bin/env python3
"""A level-of-detail frame at C3 (512^3 f32, default algorithm, abs 1e-4) through an opened stream: one 128^3 tile at
level 0 in the centre, four 64^3 tiles at level 1 around it, the whole grid at level 3 — all of it into ONE atlas tensor.
  (a) request        one sz3hip_stream_request: six boxes of three levels, written through the atlas's strided views
  (b) tiles_copies   what a viewer issues without it: three sz3hip_stream_tiles calls (one per level, contiguous outputs) and the six device
                     copies into the atlas
  (b') tiles_alone   the three calls without the copies
One JSON line (LAB_WRITE=<file> appends it there: profiles/r16_request.txt holds the lines of the measurement in section 16). Protocol:
tools/stream_lab.py's — a run is CALLS calls between two device synchronisations, the variants alternate, seven runs each, the figure is the
median (us per call) with the runs' min and max; the chain is off and at 2048 points (a mixed request never takes it, the three tiles calls may).
Every box of every variant is compared with the full decode's slice.
LAB_PKG=<dir> imports <dir>/sz3_amd instead of this tree's: the parent commit's package has no request and runs (b) alone — the baseline's
figures, confirmed in the same session. Run it under a time limit of its own (timeout -k 10 300 python tools/request_lab.py); LAB_SIZE=<n>
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
HAVE_REQUEST = hasattr(sz3_amd.Stream, "request")


def frame():
    """(level, lo, shape) of the six boxes and each box's corner in the atlas"""
    e0, e1 = S // 4, S // 8
    c0 = (S - e0) // 2 + 1  # (odd corners: no box starts on a coarse lattice line)
    G1 = ((S - 1) >> 1) + 1
    c1 = (G1 - 2 * e1) // 2 + 1
    G3 = ((S - 1) >> 3) + 1
    items = [(0, (c0, c0, c0), (e0, e0, e0))]
    items += [(1, (c1, c1 + i * e1, c1 + j * e1), (e1, e1, e1)) for i in range(2) for j in range(2)]
    items.append((3, (0, 0, 0), (G3, G3, G3)))
    # the atlas: e0 planes of e0 x (e0 + 2 e1 + G3): the fine tile, the four level-1 tiles as a 2 x 2 block, the overview
    corners = [(0, 0, 0)] + [(0, i * e1, e0 + j * e1) for i in range(2) for j in range(2)] + [(0, 0, e0 + 2 * e1)]
    return items, corners, (e0, e0, e0 + 2 * e1 + G3)


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
    items, corners, adims = frame()
    levels = sorted({it[0] for it in items})

    def atlas_views():
        atlas = torch.full(adims, 77.0, dtype=torch.float32, device=dev)
        return atlas, [atlas[tuple(slice(c, c + e) for c, e in zip(cn, it[2]))] for it, cn in zip(items, corners)]

    atlases, variants, info = {}, {}, {}
    for pts in (0, 2048):
        atlas_b, views_b = atlas_views()
        tiles_out = {k: [torch.empty(it[2], dtype=torch.float32, device=dev) for it in items if it[0] == k] for k in levels}
        boxes = {k: [it[1:] for it in items if it[0] == k] for k in levels}
        where = {k: [v for it, v in zip(items, views_b) if it[0] == k] for k in levels}

        def tiles_alone(pts=pts, tiles_out=tiles_out, boxes=boxes):
            sz3_amd.set_chain_points(pts)
            for k in levels:
                st.tiles(k, boxes[k], out=tiles_out[k])

        def tiles_copies(pts=pts, tiles_out=tiles_out, boxes=boxes, where=where):
            tiles_alone(pts, tiles_out, boxes)
            for k in levels:
                for v, t in zip(where[k], tiles_out[k]):
                    v.copy_(t)
        variants["tiles_alone_chain%d" % pts] = tiles_alone
        variants["tiles_copies_chain%d" % pts] = tiles_copies
        atlases["tiles_copies_chain%d" % pts] = (atlas_b, views_b)
        if HAVE_REQUEST:
            atlas_a, views_a = atlas_views()

            def request(pts=pts, views_a=views_a):
                sz3_amd.set_chain_points(pts)
                st.request([it + (v,) for it, v in zip(items, views_a)])
            variants["request_chain%d" % pts] = request
            atlases["request_chain%d" % pts] = (atlas_a, views_a)

    for f in variants.values():  # warm-up: code objects, the handle's scratch and table
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    identical = True
    for n, (atlas, views) in atlases.items():
        atlas.fill_(77.0)
        l0 = sz3_amd.lib().sz3hip_debug_region_launches()
        variants[n]()
        torch.cuda.synchronize()
        stt = st.stats()
        info[n] = {"region_launches": int(sz3_amd.lib().sz3hip_debug_region_launches() - l0)}
        if n.startswith("request"):
            info[n].update({q: stt[q] for q in ("launches_last_request", "chain_levels_last_request", "n_levels_last_request")})
        for (k, lo, ext), v in zip(items, views):
            cv = full[tuple(slice(None, None, 1 << k) for _ in range(3))]
            identical = identical and bool(torch.equal(v, cv[tuple(slice(l, l + e) for l, e in zip(lo, ext))]))
        written = sum(int(np.prod(it[2])) for it in items)
        identical = identical and int((atlas != 77.0).sum()) <= written and int((atlas == 77.0).sum()) >= atlas.numel() - written
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
           "frame": [{"level": k, "lo": list(lo), "shape": list(ext)} for k, lo, ext in items], "atlas": list(adims), "runs": RUNS, "calls_per_run": CALLS,
           "request_call": HAVE_REQUEST, "bit_identical_to_full_slice": identical,
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

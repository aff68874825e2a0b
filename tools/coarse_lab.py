#!/usr/bin/env python3
"""Coarse decode against the full decode at C3 (512^3 f32, default algorithm, abs 1e-4), through the device context. One JSON line.

Variants: the full decode, the full decode followed by the strided gather of the level-1 points (what a consumer without the coarse call
has to run), and the coarse decode at levels 1, 2, 3. A run is CALLS calls between two device synchronisations; the variants alternate,
seven runs each, and the figure is the median (us per call) with the runs' min and max beside it. The stage split (Huffman stage,
reconstruction) comes from sz3hip_get_stage_times in runs of its own.  --full-only: the full decode alone (SZ3HIP_LIB=<another build>
python tools/coarse_lab.py --full-only times that build's decoder, e.g. the parent commit's)."""
import ctypes as C
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
FULL_ONLY = "--full-only" in sys.argv


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
    L = sz3_amd.lib()

    def run_full():
        dc.decompress(pl.data_ptr(), size, full.data_ptr(), s)

    variants = {"full": run_full}
    outs = {}
    if not FULL_ONLY:
        dims = (C.c_uint64 * 3)(*sz3_amd.coarse_dims(conf, 1))
        strides = (C.c_int64 * 3)(2 * S * S, 2 * S, 2)
        gathered = torch.empty(sz3_amd.coarse_dims(conf, 1), dtype=torch.float32, device=dev)
        L.sz3hip_debug_gather.restype = C.c_int
        L.sz3hip_debug_gather.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]

        def run_full_gather():
            dc.decompress(pl.data_ptr(), size, full.data_ptr(), s)
            sz3_amd._check(L.sz3hip_debug_gather(0, full.data_ptr(), 3, dims, strides, gathered.data_ptr(), s))

        variants["full_plus_gather_l1"] = run_full_gather
        for k in (1, 2, 3):
            outs[k] = torch.empty(sz3_amd.coarse_dims(conf, k), dtype=torch.float32, device=dev)
            variants["coarse_l%d" % k] = (lambda k=k: dc.decompress_coarse(pl.data_ptr(), size, k, outs[k].data_ptr(), s))

    for f in variants.values():  # warm-up: code objects, the context's lazy buffers
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    identical = None
    if not FULL_ONLY:
        identical = all(bool(torch.equal(outs[k], full[::2 ** k, ::2 ** k, ::2 ** k])) for k in outs) and bool(torch.equal(gathered, full[::2, ::2, ::2]))
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
        if n == "full_plus_gather_l1":
            continue
        h, r = [], []
        for _ in range(RUNS):
            f()
            torch.cuda.synchronize()
            t = dc.stage_times()
            h.append(1e3 * t.get("huffman_decode", 0.0))
            r.append(1e3 * t.get("reconstruct", 0.0))
        stages[n] = {"huffman_decode_us": round(float(np.median(h)), 1), "reconstruct_us": round(float(np.median(r)), 1)}
    dc.set_profiling(False)
    res = {"case": "C3", "shape": [S, S, S], "dtype": "float32", "abs_eb": 1e-4, "ratio": round(a.nbytes / size, 3),
           "lib": os.path.basename(os.environ.get("SZ3HIP_LIB", "libsz3hip.so")), "runs": RUNS, "calls_per_run": CALLS,
           "bit_identical_to_full_subsampled": identical,
           "us_per_call": {n: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in times.items()},
           "stages": stages}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

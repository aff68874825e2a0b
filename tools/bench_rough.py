"""The benchmark's step (stage1 -> stage2 -> finish on one context, Lorenzo, abs 1e-3, 512^3 f32) on a ROUGH field — tests/packb_fields.py's
"all" field, whose chunks all take k_pack_b's slow tiers — for A/B runs of two builds (SZ3HIP_LIB=path/to/libsz3hip.so).
--sigma: the grain of the noise; at 0.03 the probe chooses two-byte codes (k_pack's), at 0.02 one-byte codes (k_pack_b's slow tiers).
python tools/bench_rough.py [--steps K] [--warmup W] [--size S] [--sigma G]   -> one JSON line"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import sz3_amd
from packb_fields import device_field


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sigma", type=float, default=0.03)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = (args.size,) * 3
    t = device_field(torch, dev, shape, "all", args.sigma)
    n = t.numel()
    conf = sz3_amd.Config(*shape)
    conf.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
    conf.lorenzo, conf.lorenzo2, conf.regression = 1, 0, 0
    conf.errorBoundMode = sz3_amd.EB_ABS
    conf.absErrorBound = 1e-3
    dc = sz3_amd.DeviceCompressor(n, np.float32)
    cap = dc.payload_bound(n)
    pl = torch.empty(cap, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        dc.stage1(conf, t.data_ptr(), stream)
        dc.stage2(pl.data_ptr(), cap, stream)
        return dc.finish(stream)

    for _ in range(args.warmup):
        size = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        size = step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    print(json.dumps({"field": "rough-all", "sigma": args.sigma, "shape": list(shape), "ms_per_step": 1e3 * el / args.steps, "ratio": 4.0 * n / size,
                      "narrow_codes": dc.stats()["narrow_codes"], "lib": sz3_amd.LIB_PATH}), flush=True)


if __name__ == "__main__":
    main()

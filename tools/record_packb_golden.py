"""Records tests/golden/packb_units.json: sha256 and size of the sampled-book payloads of tests/test_gpu_packb_units.py's fields, as
the library in the tree writes them. Run it with the build of the commit BEFORE a change to the packer; the test then holds the
changed packer to those bytes.   python tools/record_packb_golden.py [OUT.json]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import sz3_amd
import szh_ref
from packb_fields import device_field

SHAPES = [(64, 256, 256), (192, 512, 512)]
EB = 1e-3


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "packb_units.json")
    dev = torch.device("cuda:0")
    rec = {}
    for shape in SHAPES:
        t = device_field(torch, dev, shape)
        n = t.numel()
        conf = sz3_amd.Config(*shape)
        conf.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
        conf.regression = 0
        conf.errorBoundMode = sz3_amd.EB_ABS
        conf.absErrorBound = EB
        dc = sz3_amd.DeviceCompressor(n, np.float32)
        cap = dc.payload_bound(n, worst_case=True)
        pl = torch.empty(cap, dtype=torch.uint8, device=dev)
        blobs = []
        for _ in range(3):
            size = dc.compress(conf, t.data_ptr(), pl.data_ptr(), cap, 0)
            blobs.append(pl[:size].cpu().numpy().tobytes())
        assert blobs[0] == blobs[1] == blobs[2], "the three calls of a fresh context disagree"
        h, _, _ = szh_ref.parse(np.frombuffer(blobs[0], dtype=np.uint8))
        assert dc.stats()["narrow_codes"] and h["esc_sym"] != 0, "not the sampled book's path: choose another field"
        rec["x".join(map(str, shape))] = {"size": len(blobs[0]), "sha256": hashlib.sha256(blobs[0]).hexdigest()}
        print(shape, rec["x".join(map(str, shape))], flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

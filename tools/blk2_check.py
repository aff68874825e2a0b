"""8192^2 f32 at 0.15 (VERDICT round 3, item 4's 2-D figure) through the 2-D block decoders (debug flags 0 / Dbg.BLKDEC_PER_FRONT): bit for bit the
same, and the decompress time of each (device-resident, events)"""
import sys, os, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch
import sz3_amd
from fields import field2d  # noqa

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
eb = float(sys.argv[2]) if len(sys.argv) > 2 else 0.15
a = field2d((n, n), np.float32)
conf = sz3_amd.Config(n, n)
conf.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
conf.errorBoundMode = sz3_amd.EB_ABS
conf.absErrorBound = eb
conf.lorenzo, conf.lorenzo2, conf.regression = 1, 0, 1
blob, _ = sz3_amd.compress(a, conf)
outs = {}
PER_FRONT = int(sz3_amd.Dbg.BLKDEC_PER_FRONT)
for flag in (0, PER_FRONT, 0, PER_FRONT):
    sz3_amd.lib().sz3hip_debug_flags(flag)
    out = np.empty_like(a)
    for _ in range(3):
        sz3_amd.decompress(blob, np.float32, a.shape, out=out)
    t0 = time.perf_counter()
    for _ in range(5):
        sz3_amd.decompress(blob, np.float32, a.shape, out=out)
    dt = (time.perf_counter() - t0) / 5
    outs.setdefault(flag, []).append(out.copy())
    print("flag %d: host-side decompress %.2f ms per call (includes the copies)" % (flag, dt * 1e3))
sz3_amd.lib().sz3hip_debug_flags(0)
same = all(np.array_equal(outs[0][0], o) for v in outs.values() for o in v)
err = float(np.max(np.abs(outs[0][0].astype(np.float64) - a.astype(np.float64))))
print("n", n, "ratio %.2f" % (a.nbytes / len(blob)), "identical", same, "max err", err)
sys.exit(0 if same and err <= eb else 1)

"""GPU tests (-m gpu) of the sampled stage 2 in three launches: k_pack_b scans the offset groups' word counts itself, in LDS, where
its table holds them (at most 4096 groups), instead of reading the offsets a k_scan_groups launch left in memory.
Every case compresses the same device-built field (tests/packb_fields.py) on two fresh contexts, three calls each — the first call
of a context waits for the probe, the one-launch stage 1 and with it this form run from the second on: once as the library chooses
and once with Dbg2.PACK_SCAN_LAUNCH, which forces the scan's own launch. The payloads and their sizes must agree byte for byte,
the launch counts must be the expected ones, and one payload must decode within the bound."""
import numpy as np
import pytest

import sz3_amd
import szh_ref
from packb_fields import device_field, spike

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EB = 1e-3
SCAN_LAUNCH = sz3_amd.Dbg2.PACK_SCAN_LAUNCH


def _conf(shape):
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
    c.regression = 0
    c.errorBoundMode = sz3_amd.EB_ABS
    c.absErrorBound = EB
    return c


def _three_calls(t, flags2, decode):
    """three calls of a fresh context; returns the payloads, the encoder's launch count of every call, the stats and (decode) the
    largest error of the last payload's reconstruction"""
    n = t.numel()
    conf = _conf(tuple(t.shape))
    dc = sz3_amd.DeviceCompressor(n, np.float32)
    cap = dc.payload_bound(n, worst_case=True)
    pl = torch.empty(cap, dtype=torch.uint8, device=t.device)
    outs, launches = [], []
    with sz3_amd.debug_flags2(flags2):
        for _ in range(3):
            size = dc.compress(conf, t.data_ptr(), pl.data_ptr(), cap, 0)
            launches.append(sz3_amd.last_encode_launches())
            outs.append(pl[:size].cpu().numpy().tobytes())
    err = None
    if decode:
        dec = torch.empty_like(t)
        dc.decompress(pl.data_ptr(), size, dec.data_ptr(), 0)
        torch.cuda.synchronize()
        err = float((dec.double() - t.double()).abs().max())
    return outs, launches, dc.stats(), err


CASES = [
    # name, shape, rough, sigma, spikes, the packer scans the offsets itself
    ("whole-groups", (64, 256, 256), None, 0.0, 0, True),         # 2^22 elements, the smallest array the sampled form takes: 128 groups
    ("partial-last-group", (64, 257, 256), None, 0.0, 0, True),   # 4112 chunks = 128.5 groups
    ("ragged-last-chunk", (65, 257, 256), None, 0.0, 0, True),    # 16 705 rows of 256: not a multiple of 1024 elements
    ("mixed-tiers", (64, 256, 256), "chunks5", 0.03, 0, True),    # fast and slow chunks in every order inside a unit
    ("listed-deltas", (64, 256, 512), None, 0.0, 40, True),       # byte 255, the escape (tests/test_gpu_packb_units.py's "spiky-narrow": the field of that size keeps one-byte codes)
    ("capacity", (512, 512, 512), None, 0.0, 0, True),            # exactly 4096 groups: the table is full
    ("over-capacity", (513, 512, 512), None, 0.0, 0, False),      # 4104 groups: the scan's own launch
]


@pytest.mark.parametrize("name,shape,rough,sigma,spikes,in_launch", CASES, ids=[c[0] for c in CASES])
def test_scan_in_the_packers_launch_writes_the_same_bytes(name, shape, rough, sigma, spikes, in_launch):
    dev = torch.device("cuda:0")
    t = device_field(torch, dev, shape, rough, sigma)
    if spikes:
        spike(torch, t, spikes)
    new, l_new, st, err = _three_calls(t, 0, True)
    old, l_old, _, _ = _three_calls(t, SCAN_LAUNCH, False)
    print("%s: narrow_codes %d, payload %d bytes, launches %s / %s, max error %.3g" % (name, st["narrow_codes"], len(new[2]), l_new, l_old, err))
    assert st["narrow_codes"], "two-byte codes: not the sampled book's path"
    h, _, _ = szh_ref.parse(np.frombuffer(new[2], dtype=np.uint8))
    assert h["esc_sym"] != 0, "the call did not code with a sampled book"  # (the header's escape symbol: sampled books only)
    assert err <= EB, err
    for k in range(3):
        assert len(new[k]) == len(old[k]), (k, len(new[k]), len(old[k]))
        assert new[k] == old[k], "call %d: the two forms of the offset scan disagree (%s)" % (k, name)
    # the segment pass, the scan and the packer — or the segment pass and the packer
    assert l_old[1:] == [3, 3], l_old
    assert l_new[1:] == ([2, 2] if in_launch else [3, 3]), l_new

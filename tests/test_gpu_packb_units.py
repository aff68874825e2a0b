"""GPU tests (-m gpu) of k_pack_b's unit loop (round 9: the next unit's loads issued unconditionally a unit ahead, two register sets
that swap roles, one stage and one 16-byte-per-lane copy-out per unit of four chunks, issued behind the next unit's wait).
tests/test_gpu_packb.py's arrays give every wave at most one unit, so the rotation of the register sets never runs there: the
arrays here give every wave at least three (n >= 3 * 16 * 253 * 4096 elements), are built on the device (tests/packb_fields.py)
and are a pure function of their indices.
 1. Against k_pack on the same context state (Dbg.CB_NO_SAMPLED with and without Dbg.PACK_OLD): same book, same chunk table, so
    the payloads agree byte for byte.
 2. The sampled book's path — the benchmark's, whose books k_pack cannot pack — against the bytes of the commit before the change
    (tests/golden/packb_units.json, written by tools/record_packb_golden.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

import sz3_amd
import szh_ref
from packb_fields import device_field, spike

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OLD_PACKER = sz3_amd.Dbg.PACK_OLD
NO_SAMPLE = sz3_amd.Dbg.CB_NO_SAMPLED
EB = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packb_units.json")


def _conf(shape, eb):
    c = sz3_amd.Config(*shape)
    c.cmprAlgo = sz3_amd.ALGO_LORENZO_REG
    c.regression = 0
    c.errorBoundMode = sz3_amd.EB_ABS
    c.absErrorBound = eb
    return c


def _three_calls(t, flags, spec=None):
    """three calls of a fresh context (the first waits for the probe: the one-launch form — and k_pack_b — from the second on);
    returns the payloads, the context's stats and whether the last payload decodes within the bound"""
    n = t.numel()
    conf = _conf(tuple(t.shape), EB)
    dc = sz3_amd.DeviceCompressor(n, np.float32)
    if spec is not None:
        dc.set_speculation(spec)
    cap = dc.payload_bound(n, worst_case=True)
    pl = torch.empty(cap, dtype=torch.uint8, device=t.device)
    outs = []
    with sz3_amd.debug_flags(flags):
        for _ in range(3):
            size = dc.compress(conf, t.data_ptr(), pl.data_ptr(), cap, 0)
            outs.append(pl[:size].cpu().numpy().tobytes())
    dec = torch.empty_like(t)
    dc.decompress(pl.data_ptr(), size, dec.data_ptr(), 0)
    torch.cuda.synchronize()
    err = float((dec.double() - t.double()).abs().max())
    return outs, dc.stats(), err


CASES = [
    # name, shape, rough, sigma, spikes, one-byte codes expected
    ("rounds-even", (192, 512, 512), None, 0.0, 0, True),        # 12 288 units: three full rounds of the launch's waves and a partial fourth
    ("rounds-ragged", (193, 509, 516), None, 0.0, 0, True),      # 49 502 whole chunks: a last unit of two chunks, a ragged last chunk of 244 symbols
    ("mixed-units", (192, 512, 512), "rows5", 0.03, 0, True),    # every fifth row of 512 rough
    ("mixed-chunks", (192, 512, 512), "chunks5", 0.03, 0, True),  # fast and slow chunks in every order inside a unit: the flush in front of a slow chunk, a fast chunk behind one, a slow first and last chunk
    # sigma = 0.03 everywhere puts 0.3 % of the deltas outside one byte, and 4000 spikes 0.4 %: the probe (at most 1 / 4096) then chooses
    # two-byte codes and both sides of the comparison are k_pack's. The two cases stay as they were set; the two behind them are the
    # same fields at the largest grain / number of spikes that keeps one-byte codes, and it is those that run this packer's slow tiers.
    ("rough-all", (64, 256, 512), "all", 0.03, 0, False),
    ("spiky", (64, 256, 512), None, 0.0, 4000, False),
    ("rough-all-narrow", (64, 256, 512), "all", 0.02, 0, True),  # 2 % of the bytes outside the pair table's window: the slow tiers only
    ("spiky-narrow", (64, 256, 512), None, 0.0, 40, True),       # byte 255: listed deltas
    ("rough-rounds", (192, 512, 512), "all", 0.02, 0, True),     # the slow tiers through three rounds of the rotation
]


@pytest.mark.parametrize("name,shape,rough,sigma,spikes,narrow", CASES, ids=[c[0] for c in CASES])
def test_unit_loop_writes_the_old_packers_bytes(name, shape, rough, sigma, spikes, narrow):
    dev = torch.device("cuda:0")
    t = device_field(torch, dev, shape, rough, sigma)
    if spikes:
        spike(torch, t, spikes)
    new, st, err = _three_calls(t, NO_SAMPLE, False)
    old, _, err_old = _three_calls(t, NO_SAMPLE | OLD_PACKER, False)
    print("%s: narrow_codes %d, payload %d bytes, max error %.3g / %.3g" % (name, st["narrow_codes"], len(new[2]), err, err_old))
    if narrow:
        assert st["narrow_codes"], "the field took two-byte codes: not this packer's case"
    assert err <= EB and err_old <= EB, (err, err_old)
    for k in range(3):
        assert new[k] == old[k], "call %d: k_pack_b and k_pack disagree (%s)" % (k, name)
    assert new[0] == new[1] == new[2]


def test_the_cases_give_every_wave_three_units():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for name, shape in [(c[0], c[1]) for c in CASES if c[1][0] >= 192]:
        n = shape[0] * shape[1] * shape[2]
        assert n // 4096 >= 3 * 16 * (cus - 3), (name, n, cus)


GOLDEN_SHAPES = [(64, 256, 256), (192, 512, 512)]


@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=["x".join(map(str, s)) for s in GOLDEN_SHAPES])
def test_sampled_book_payload_is_the_parents(shape):
    with open(GOLDEN) as f:
        want = json.load(f)["x".join(map(str, shape))]
    dev = torch.device("cuda:0")
    t = device_field(torch, dev, shape)
    outs, st, err = _three_calls(t, 0)
    assert err <= EB, err
    assert st["narrow_codes"], "two-byte codes: not the sampled book's path"
    for k, blob in enumerate(outs):
        h, _, _ = szh_ref.parse(np.frombuffer(blob, dtype=np.uint8))
        assert h["esc_sym"] != 0, "call %d did not code with a sampled book" % k  # (the header's escape symbol: sampled books only)
        assert len(blob) == want["size"], (k, len(blob), want["size"])
        assert hashlib.sha256(blob).hexdigest() == want["sha256"], "call %d: not the bytes of the commit before the change" % k

"""bench.py without a device: its inputs are tests/fields.py's arrays bit for bit, its options, and what --dump-outputs writes"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fields import field3d, field_c4a  # noqa: E402


@pytest.mark.parametrize("shape", [(13, 17, 29), (33, 47, 50), (7, 100, 101), (64, 64, 64)])
def test_fast_field_is_fields_field3d_bit_for_bit(shape):
    assert bench.field3d_fast(shape).tobytes() == field3d(shape).tobytes()
    assert bench.field3d_fast(shape, seed=20261928).tobytes() == field3d(shape, seed=20261928).tobytes()
    assert (bench.field3d_fast(shape, np.float64, seed=20260929, sigma=2e-6).tobytes()
            == field3d(shape, np.float64, seed=20260929, sigma=2e-6).tobytes())
    assert (bench.field3d_fast(shape, np.float64, sigma=2e-3, seed=20260928, scale=3.3e-5).tobytes()
            == field_c4a(shape, seed=20260928).tobytes())


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()


class _Payload:
    def __init__(self, n, seed):
        torch = pytest.importorskip("torch")
        self.d_payload = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, n + 100, dtype=np.uint8))


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in ("payload", "payload_index", "payload_size")}


def test_dump_outputs_small_payload_is_whole(tmp_path):
    w = _Payload(5000, 1)
    bench.dump_outputs(w, 5000, str(tmp_path))
    o = _load(str(tmp_path))
    assert o["payload"].dtype == np.float32 and o["payload_index"].dtype == np.float64 and o["payload_size"].tolist() == [5000.0]
    assert np.array_equal(o["payload"], w.d_payload.numpy()[:5000].astype(np.float32))
    assert np.array_equal(o["payload_index"], np.arange(5000))


def test_dump_outputs_long_payload_is_a_fixed_sample_under_64_mb(tmp_path):
    n = bench.DUMP_MAX_POSITIONS + 123457
    w = _Payload(n, 2)
    bench.dump_outputs(w, n, str(tmp_path / "a"))
    bench.dump_outputs(w, n, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    for k in a:
        assert np.array_equal(a[k], b[k])
    idx = a["payload_index"].astype(np.int64)
    assert len(idx) <= bench.DUMP_MAX_POSITIONS and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(idx[:bench.DUMP_HEAD], np.arange(bench.DUMP_HEAD))
    assert np.array_equal(a["payload"], w.d_payload.numpy()[idx].astype(np.float32))
    total = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20

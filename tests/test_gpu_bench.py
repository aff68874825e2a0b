"""GPU test (-m gpu) of bench.py's plain run: the headline line and nothing of --full, --steps as the number of timed steps, and
--dump-outputs writing the same payload for the same arguments run after run"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "ratio", "n_gpus", "steps", "warmup", "config")


def _bench(args, env_extra=None, timeout=600):
    env = dict(os.environ, **(env_extra or {}))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_payload(tmp_path):
    outs = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        line = _bench(["--gpus", "1", "--steps", "5", "--warmup", "2", "--size", "128", "--dump-outputs", d])
        assert all(key in line for key in HEADLINE), line
        assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "GB/s" and line["higher_is_better"]
        assert line["ratio"] > 2 and line["dtype"] == "f32"
        assert not any(key in line for key in ("roofline", "cpu_baseline", "extra_configs", "stage_ms", "decompress_device", "cold", "host_e2e"))
        o = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
        assert sorted(o) == ["payload", "payload_index", "payload_size"]
        assert o["payload_size"].tolist() == [float(line["payload_bytes_rank0"])]
        assert o["payload"].dtype == np.float32 and len(o["payload"]) == line["payload_bytes_rank0"]  # (a 128^3 payload is written whole)
        assert o["payload"][:4].tolist() == [float(b) for b in b"SZH1"]  # (sz3hip_format.h: the payload's magic)
        outs.append(o)
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_plain_run_as_two_ranks_on_the_one_gpu():
    d = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--size", "128"], {"SZ3_BENCH_ONE_GPU": "1"}, timeout=900)
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["config"]["parallelism"] == "slab2" and "gloo" in d["config"]["exchange"]
    assert d["value"] > 0 and d["ratio"] > 2 and "roofline" not in d and "extra_configs" not in d

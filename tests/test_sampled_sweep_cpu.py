"""tests/checks/sampled_sweep.py without a device (DRY=1): for exactly the seeds the GPU test runs, every drawn case passes the premises the
numpy model sets before anything is launched — one-byte codes, the class of the listed deltas, whether the book is sampled — and the draws of
those seeds together cover what the sweep is there for (the floors below). A floor that is missed means other seeds, not a lower floor."""
import json
import os
import subprocess
import sys
from collections import Counter

import pytest

from sweep_seeds import SAMPLED_SWEEP_N, SAMPLED_SWEEP_SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("smooth", "c2", "rough", "constant", "listed-few", "listed-many", "nonfinite", "far-value")
ENCODER = ("K1_NO_Q16", "K1_NO_SAMP_IN_LAUNCH", "K1_Q16_PLAIN_STORES", "K1_NO_XCD_ORDER", "K1_NO_DEFER_FOLD", "CTX_NO_MEMORY", "PACK_SCAN_LAUNCH", "no-speculation")
DECODER = ("DEC_NO_FUSED_X", "DEC_NO_HALF", "DEC_CARRY_PASS")
RUN = SAMPLED_SWEEP_N + 2  # (the two fixed cases of every seed)


def dry(seed):
    env = dict(os.environ, SEED=str(seed), N=str(SAMPLED_SWEEP_N), DRY="1")
    for k in ("CASES", "VERBOSE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "sampled_sweep.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "cases %d (SEED %d, DRY: draws and premises only) failures 0" % (RUN, seed) in r.stdout, r.stdout[-3000:]
    tally = [ln for ln in r.stdout.splitlines() if ln.startswith("TALLY ")]
    assert len(tally) == 1
    return json.loads(tally[0][6:])


@pytest.fixture(scope="module")
def tallies():
    return {seed: dry(seed) for seed in SAMPLED_SWEEP_SEEDS}


def test_every_draw_meets_its_premises(tallies):
    assert len(tallies) == len(SAMPLED_SWEEP_SEEDS) == 4
    for t in tallies.values():
        assert sum(t["kind"].values()) == RUN  # (a case whose premise fails is not tallied)
        assert t["kind"]["steps-2048"] == t["kind"]["steps-2049"] == 1
        assert t["listed"].get("few", 0) >= 1 and t["listed"].get("many", 0) >= 1


def test_the_floors(tallies):
    agg = {}
    for t in tallies.values():
        for k, v in t.items():
            if isinstance(v, dict):
                agg.setdefault(k, Counter()).update(v)
            elif k != "excess":
                agg[k] = agg.get(k, 0) + v
    # the shapes, over the cases that take the sampled book
    assert all(agg["y_mod_4"][str(r)] >= 1 for r in range(4)), dict(agg["y_mod_4"])
    assert all(agg["z_mod_16"][str(r)] >= 1 for r in (0, 1, 15)), dict(agg["z_mod_16"])
    assert agg["z_below_16"] >= 1 and agg["ragged_chunk"] >= 1 and agg["ragged_nseg"] >= 1
    assert all(agg["rank"][str(r)] >= 1 for r in (1, 2, 3)), dict(agg["rank"])
    assert all(agg["dtype_rank"]["%s/%d" % (d, r)] >= 1 for d in ("float32", "float64") for r in (1, 2, 3)), dict(agg["dtype_rank"])
    # the data, the settings, the neighbours
    assert all(agg["kind"][k] >= 2 for k in KINDS), dict(agg["kind"])
    assert all(agg["listed"][c] >= 2 for c in ("none", "few", "many")), dict(agg["listed"])
    assert all(agg["encoder"][s] >= 2 for s in ENCODER), dict(agg["encoder"])
    assert all(agg["decoder"][s] >= 2 for s in DECODER), dict(agg["decoder"])
    assert sum(v for k, v in agg["neighbour"].items() if k != "None") >= 3, dict(agg["neighbour"])
    assert agg["licensed"] >= 2 and agg["voids"] >= 1, "the 16-bit form of stage 1: licensed %d, voided %d" % (agg["licensed"], agg["voids"])

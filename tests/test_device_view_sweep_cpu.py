"""tests/checks/device_view_sweep.py without a device (DRY=1): for exactly the seeds the GPU test runs, every drawn view lies inside its
allocation, every drawn output passes view_model.dev_view_rule and names no element twice, every pieces draw is one the library cuts — and the
draws of those seeds together cover what the sweep is there for (the floors below, counted from the draws by the form functions of
tests/view_model.py). A floor that is missed means other seeds or other weights of the draw, not a lower floor."""
import json
import os
import subprocess
import sys
from collections import Counter

import pytest

import view_model as M
from sweep_seeds import DEVICE_VIEW_SWEEP_N, DEVICE_VIEW_SWEEP_SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dry(seed, n=DEVICE_VIEW_SWEEP_N):
    env = dict(os.environ, SEED=str(seed), N=str(n), DRY="1")
    for k in ("CASES", "VERBOSE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "device_view_sweep.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "cases %d (SEED %d, DRY: draws only) failures 0" % (n, seed) in r.stdout, r.stdout[-3000:]
    tally = [ln for ln in r.stdout.splitlines() if ln.startswith("TALLY ")]
    assert len(tally) == 1
    return json.loads(tally[0][6:])


def aggregate(tallies):
    agg = {}
    for t in tallies:
        for k, v in t.items():
            if isinstance(v, dict):
                agg.setdefault(k, Counter()).update(v)
            else:
                agg[k] = agg.get(k, 0) + v
    return agg


def missed_floors(agg):
    """-> the floors the aggregated tallies miss, as text"""
    miss = []

    def floor(what, have, need):
        if have < need:
            miss.append("%s: %d < %d" % (what, have, need))

    for dt in M.DTYPES:
        floor("dtype %s as input" % dt, agg["dtype_in"].get(dt, 0), 2)
        floor("dtype %s as output" % dt, agg["dtype_out"].get(dt, 0), 2)
    for rank in "1234":
        floor("rank " + rank, agg["rank"].get(rank, 0), 3)
    for side in ("gather", "scatter"):
        for form in ("16", "8", M.ELEMENT):
            floor("%s in %s units" % (side, form), agg[side + "_form"].get(form, 0), 3)
        floor("%s that converts (widen / narrow)" % side, agg[side + "_convert"], 6)
        floor("%s with rows_per_wave > 1" % side, agg[side + "_packed"], 3)
        floor("%s with rows_per_wave == 1" % side, agg[side + "_one_row"], 3)
        floor("%s with row_passes > 1" % side, agg[side + "_passes"], 3)
    floor("permuted output", agg["permuted_out"], 3)
    floor("stepped output", agg["stepped_out"], 3)
    floor("stride-0 input", agg["zero_in"], 2)
    floor("slabs over a strided input", agg["slabs_strided_in"], 3)
    floor("pieces over a strided input", agg["pieces_strided_in"], 2)
    floor("stock format", agg["stock"], 4)
    floor("coarse into a strided output", agg["coarse_strided_out"], 3)
    floor("integer data reaching the clamp", agg["clamp"], 3)
    return miss


@pytest.fixture(scope="module")
def tallies():
    return {seed: dry(seed) for seed in DEVICE_VIEW_SWEEP_SEEDS}


def test_every_draw_meets_its_premises(tallies):
    assert len(tallies) == len(DEVICE_VIEW_SWEEP_SEEDS) == 2
    for t in tallies.values():
        assert sum(t["dtype_in"].values()) == sum(t["rank"].values()) == DEVICE_VIEW_SWEEP_N


def test_the_floors(tallies):
    assert missed_floors(aggregate(tallies.values())) == []

"""tests/checks/partial_sweep.py without a device (DRY=1): for exactly the seeds the GPU test runs, every drawn request passes the pure host
plan functions (region, tile, tiles, request, reduce, select, map, sample, project) — a refused draw is a bug in the draw; the one exception,
which the sweep itself counts as such, is a case whose anchor stride is no power of two: every plan must answer SZ3HIP_EUNSUPPORTED — and the
draws of those seeds together cover what the sweep is there for (the floors below). A floor that is missed means other seeds, not a lower
floor."""
import json
import math
import os
import subprocess
import sys
from collections import Counter

import pytest

from sweep_seeds import PARTIAL_SWEEP_N, PARTIAL_SWEEP_SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINKS = ("reduce", "select", "map", "sample", "project")
ROUTES = ("chain", "merged", "by_level")


def dry(seed):
    env = dict(os.environ, SEED=str(seed), N=str(PARTIAL_SWEEP_N), DRY="1")
    for k in ("CASES", "VERBOSE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "partial_sweep.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "cases %d (SEED %d, DRY: plans only) failures 0" % (PARTIAL_SWEEP_N, seed) in r.stdout, r.stdout[-3000:]
    tally = [ln for ln in r.stdout.splitlines() if ln.startswith("TALLY ")]
    assert len(tally) == 1
    return json.loads(tally[0][6:])


@pytest.fixture(scope="module")
def tallies():
    return {seed: dry(seed) for seed in PARTIAL_SWEEP_SEEDS}


def test_every_draw_passes_the_plans(tallies):
    assert len(tallies) == len(PARTIAL_SWEEP_SEEDS) >= 4
    assert all(sum(t["rank"].values()) == PARTIAL_SWEEP_N for t in tallies.values())


def test_the_floors(tallies):
    agg = {}
    for t in tallies.values():
        for k, v in t.items():
            if isinstance(v, dict):
                agg.setdefault(k, Counter()).update(v)
            else:
                agg[k] = agg.get(k, 0) + v
    d = agg["direction"]
    for N in (2, 3):
        assert all(d["%dD:%d" % (N, i)] >= 1 for i in range(math.factorial(N))), "every direction id of rank %d: %s" % (N, dict(d))
    assert sum(1 for k in d if k.startswith("4D:")) >= 8, "eight distinct 4-D ids: %s" % dict(d)
    assert all(agg["anchor"][a] >= 1 for a in ("None", "0", "2", "4", "8", "16", "32", "64")), dict(agg["anchor"])
    assert agg["anchor"]["12"] + agg["anchor"]["24"] >= 1 and agg["odd"] >= 1, "a stride that is no power of two"
    assert all(agg["rank"][str(r)] >= 4 for r in (1, 2, 3, 4)), dict(agg["rank"])
    assert all(agg["sink"][s] >= 6 for s in SINKS), dict(agg["sink"])
    assert all(agg["sink_route_drawn"]["%s/%s" % (s, r)] >= 1 for s in SINKS for r in ROUTES), dict(agg["sink_route_drawn"])
    assert agg["all_anchor"] >= 4 and agg["one_point"] >= 2
    assert 3 * agg["oracle2plus"] >= agg["rank2plus"] > 0, "a third of the cases of rank >= 2 drawn as oracle: %d of %d" % (agg["oracle2plus"], agg["rank2plus"])
    assert all(agg["kind"][k] >= 1 for k in ("own", "payload", "oracle"))

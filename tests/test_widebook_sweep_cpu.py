"""The seeds of tests/checks/widebook_sweep.py that the suite runs on the device (tests/sweep_seeds.py), held without a GPU to the model's
premises — every drawn array codes to its prescribed stream, its histogram is the wide book's, a book that keeps every rule exists — and to
floors of what the committed seeds must cover together."""
import json
import os
import subprocess
import sys

import pytest

from sweep_seeds import WIDEBOOK_SWEEP_N, WIDEBOOK_SWEEP_SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOORS = ("one_class_below_4097", "both_tiers_rejected", "tier1", "tier2", "floor_engaged", "floor_not_engaged", "n_rare_pow2", "mk_beyond_lds",
          "limit_16_wide", "limit_binds")
_TALLIES = {}


def _dry(seed):
    if seed not in _TALLIES:
        env = dict(os.environ, SEED=str(seed), N=str(WIDEBOOK_SWEEP_N), DRY="1")
        env.pop("CASES", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "widebook_sweep.py")], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "cases %d (SEED %d, DRY: draws and premises only) failures 0" % (WIDEBOOK_SWEEP_N, seed) in r.stdout
        _TALLIES[seed] = json.loads([l for l in r.stdout.splitlines() if l.startswith("TALLY ")][0][6:])
    return _TALLIES[seed]


@pytest.mark.parametrize("seed", WIDEBOOK_SWEEP_SEEDS)
def test_draws_pass_the_models_premises(seed):
    t = _dry(seed)
    assert sum(t["kind"].values()) == WIDEBOOK_SWEEP_N


def test_committed_seeds_cover_the_regimes():
    """each regime at least twice over the committed seeds together; both dtypes; (a seed that misses is replaced, never the floor)"""
    assert len(WIDEBOOK_SWEEP_SEEDS) == 4 and WIDEBOOK_SWEEP_N == 6
    total = {k: sum(_dry(s)[k] for s in WIDEBOOK_SWEEP_SEEDS) for k in FLOORS}
    for k in FLOORS:
        assert total[k] >= 2, (k, total)
    for d in ("f32", "f64"):
        assert sum(_dry(s)["dtype"].get(d, 0) for s in WIDEBOOK_SWEEP_SEEDS) >= 2, d

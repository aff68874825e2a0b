"""The opened stream's calls against a pinned table of refusals (tests/golden/stream_errors.json, made by tests/golden/make_stream_errors.py
from a build of the commit before the calls' shared code was folded): for every case — a call and one or two faults in its arguments — the
return code and the whole sz3hip_last_error text are what the table holds. What the table is there for is the PRECEDENCE of two faults
and the _device calls' own orders (gradient and composite check their options before any pointer; the others the pointer first). No case
reaches a device."""
import json
import os
import sys

import pytest

import sz3_amd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_stream_errors as gen  # noqa: E402

with open(os.path.join(HERE, "golden", "stream_errors.json")) as f:
    TABLE = json.load(f)
CALLS = sorted({row["id"].split("[")[0] for row in TABLE})


def test_table_holds_every_case_once():
    """the table and the generator's list are the same cases in the same order: none left out, none that the generator no longer makes"""
    assert [row["id"] for row in TABLE] == gen.cases()
    assert len({row["id"] for row in TABLE}) == len(TABLE)
    assert len(CALLS) == 8 + 9 + 7


def test_table_covers_what_it_is_for():
    ids = {row["id"] for row in TABLE}
    for kind in gen.KINDS:
        assert "sz3hip_%s_plan_for[dtype_12+null_reqs]" % kind in ids
        assert "sz3hip_stream_%s[null_handle]" % kind in ids
    for kind in gen.KINDS[1:]:
        assert "sz3hip_%s_plan_for[reserved+opts]" % kind in ids and "sz3hip_%s_plan_for[opts+off_grid]" % kind in ids
        assert "sz3hip_%s_device[null_output+opts]" % kind in ids and "sz3hip_%s_device[opts+N_5]" % kind in ids
    for kind in gen.TILE_KINDS + ("select", "sample"):
        assert "sz3hip_%s_plan_for[off_grid+overlap]" % kind in ids
    for kind in ("project", "gradient", "composite"):
        assert "sz3hip_%s_plan_for[axis+misaligned]" % kind in ids
    assert "sz3hip_gradient_plan_for[interior_ext_2+overlap]" in ids and "sz3hip_stream_tiles[null_handle]" in ids
    assert all(row["rc"] != 0 and row["error"] for row in TABLE)


@pytest.mark.parametrize("call", CALLS)
def test_replay(call):
    """every case of the call, code and text for equality"""
    rows = [row for row in TABLE if row["id"].split("[")[0] == call]
    assert rows
    got = [dict(zip(("rc", "error"), gen.run(sz3_amd, row["id"])), id=row["id"]) for row in rows]
    wrong = [(g, row) for g, row in zip(got, rows) if g != row]
    assert not wrong, "\n".join("%s: got (%d, %r), the table holds (%d, %r)" % (g["id"], g["rc"], g["error"], r["rc"], r["error"]) for g, r in wrong)


def test_regenerated_table_is_byte_identical():
    with open(os.path.join(HERE, "golden", "stream_errors.json")) as f:
        assert gen.dumps(gen.table(sz3_amd)) == f.read()

"""-m gpu: the tools of the tick budget.  tools/roundtrip --compact --multi S --budget BYTES: a server core diffs S cameras per
tick, thins the records that exceed BYTES (mi355_cwire_budget_cwire_batch with mi355_cwire_budget_entries(N, BYTES) entries) and
sends them; a client core applies them.  The tool itself checks that every record written fits BYTES, that each client's frame
equals the sender's state after every tick, and that with the input held still every client's frame comes within the threshold of
the camera's.  tools/bench_multi.py --legs budget prints its line."""
import json
import os
import subprocess
import sys

import pytest

from cudavideostream_amd import cwire_budget_entries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


def test_roundtrip_multi_budget():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = [RT, "--width", "64", "--height", "48", "--compact", "--multi", "3", "--budget", "600"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])           # the verification line
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["width"] == 64 and r["height"] == 48 and r["ticks"] == 24
    assert r["budget_bytes"] == 600 and r["budget_entries"] == cwire_budget_entries(3 * 64 * 48, 600)
    assert r["records_within_budget"] is True and r["largest_record_bytes"] <= 600
    assert r["states_equal_every_tick"] is True
    assert r["max_abs_error_when_still"] <= 20 and r["still_ticks"] >= 1
    assert r["thinned_records"] > 0 and r["largest_threshold"] > 20, "the budget never bit: nothing was tested"


def test_roundtrip_budget_needs_multi():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run([RT, "--compact", "--budget", "600"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--budget" in out.stderr


def test_bench_multi_budget_prints_one_line():
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "budget", "--size", "64x48", "--streams", "2,3",
            "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_budget" and r["size"] == "64x48" and [leg["streams"] for leg in r["budget"]] == [2, 3]
    for leg in r["budget"]:
        assert 0 < leg["kept_entries_per_stream"] <= leg["entries_per_stream"] / 2
        assert leg["threshold_min"] > 20
        for name in ("budget", "second_diff"):
            assert leg[name + "_us_per_stream"]["median"] > 0

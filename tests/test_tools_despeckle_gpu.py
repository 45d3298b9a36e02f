"""-m gpu: the tools of the despeckle call.  tools/roundtrip --compact --multi S --despeckle NEED: a server core diffs S cameras
per tick, drops the isolated changes (mi355_cwire_despeckle_cwire_batch) and sends the rest; a host client per camera applies it.
The tool itself checks every tick that each client's frame equals the sender's state, that records and states equal
mi355_cwire_despeckle_host on a host copy, and that every sent entry has NEED changed pixels around it by a plain count; with the
input held still it checks that the states stand still.  tools/bench_multi.py --legs despeckle prints its line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


def test_roundtrip_multi_despeckle():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = [RT, "--width", "160", "--height", "120", "--compact", "--multi", "3", "--despeckle", "3"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])           # the verification line
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["despeckle"] == 3 and r["width"] == 160 and r["height"] == 120
    assert r["ticks"] == 24 and r["still_ticks"] >= 1
    assert r["states_equal_every_tick"] is True and r["equals_host_form"] is True and r["sent_entries_have_neighbours"] is True
    assert r["states_stand_still"] is True
    assert 0 < r["entries_out"] < r["entries_in"], "nothing was dropped, or nothing was sent: nothing was tested"
    assert 0 < r["bytes_out"] < r["bytes_in"]


def test_roundtrip_despeckle_needs_multi_alone():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    for args in (["--compact", "--despeckle", "3"], ["--compact", "--multi", "2", "--despeckle", "9"],
                 ["--compact", "--multi", "2", "--despeckle", "3", "--budget", "600"],
                 ["--compact", "--multi", "2", "--despeckle", "3", "--burst", "2"]):
        out = subprocess.run([RT] + args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--despeckle" in out.stderr, args


def test_bench_multi_despeckle_prints_one_line():
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "despeckle", "--size", "64x48", "--streams", "2",
            "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_despeckle" and r["size"] == "64x48" and r["rounds"] == 1
    assert [(leg["input"], leg["streams"]) for leg in r["despeckle"]] == [("webcam", 2), ("local", 2)]
    for leg in r["despeckle"]:
        assert leg["need"] == 3 and 0 <= leg["entries_out"] <= leg["entries_in"] and 0 < leg["bytes_out"] <= leg["bytes_in"]
        assert leg["entries_in"] > 0 and leg["budget_entries_out"] <= leg["entries_in"] // 2 + leg["streams"]
        for name in ("despeckle", "budget"):
            assert leg[name + "_us_per_stream"]["median"] > 0
        assert isinstance(leg["despeckle_no_slower_than_budget"], bool)
    web = r["despeckle"][0]
    assert web["equals_host_form"] is True and web["entries_out"] < web["entries_in"]
    assert "verdict" in r

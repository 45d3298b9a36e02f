"""-m gpu: the tools of the burst coalescer.  tools/roundtrip --multi S --burst K --coalesce: a server core makes K ticks of S
cameras in one call, a relay that holds no frame makes one record per camera of them (mi355_cwire_coalesce_cwire_batch) and
forwards those, a client core applies them with one mi355_apply_multi_cwire_batch; every camera's state is compared with a
host client that applied all K original records, and with the server.  tools/bench_multi.py --legs coalesce prints its line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.parametrize("w,h", [(64, 48), (640, 360)])
def test_roundtrip_multi_burst_coalesce(w, h):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = [RT, "--width", str(w), "--height", str(h), "--compact", "--multi", "3", "--burst", "4", "--coalesce"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])           # the verification line
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["burst"] == 4 and r["coalesce"] is True and r["ticks"] == 24
    assert r["width"] == w and r["height"] == h and r["relay_calls"] == 6 and r["max_abs_error"] <= 20
    assert 0 < r["coalesced_entries"] <= r["changed_bytes"]     # (equal when no byte changes twice within a burst)
    assert 0 < r["relay_forwarded_bytes"] < r["relay_received_bytes"]


def test_roundtrip_coalesce_needs_a_burst():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run([RT, "--compact", "--multi", "3", "--coalesce"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--coalesce" in out.stderr


def test_bench_multi_coalesce_prints_one_line_with_both_routes():
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "coalesce", "--size", "64x48", "--streams", "2",
            "--frames", "2", "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_coalesce" and r["size"] == "64x48" and len(r["coalesce"]) == 2
    assert [leg["input"] for leg in r["coalesce"]] == ["webcam", "local"]
    for leg in r["coalesce"]:
        assert leg["streams"] == 2 and leg["frames"] == 2
        assert 0 < leg["output_bytes_per_stream"] <= leg["input_bytes_per_stream"]
        for name in ("coalesce", "state_route"):
            assert leg[name + "_us_per_input_record"]["median"] > 0

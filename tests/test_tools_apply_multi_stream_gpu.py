"""-m gpu: the tools of the receiving end of a burst.  tools/roundtrip --multi S --burst K --burst-client: a server core makes K
ticks of S cameras in one call, every camera's slice crosses a pipe and is uploaded as it came, a client core applies the
burst with one mi355_apply_multi_stream_cwire_batch into output frames; states and frames are compared with the server and
with host clients.  tools/bench_multi.py --legs burst_client prints its line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


def test_roundtrip_multi_burst_client():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = [RT, "--width", "64", "--height", "48", "--frames", "8", "--compact", "--multi", "3", "--burst", "4", "--burst-client"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["burst"] == 4 and r["burst_client"] is True and r["ticks"] == 8
    assert r["sender_calls"] == r["receiver_calls"] == 2 and r["max_abs_error"] <= 20
    assert 0 < r["changed_bytes"] and r["wire_bytes"] < r["reference_wire_bytes"]


def test_bench_multi_burst_client_prints_one_line_with_the_four_legs():
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "burst_client", "--size", "64x48", "--streams", "2",
            "--frames", "2", "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_stream_client" and r["size"] == "64x48" and len(r["burst_client"]) == 2
    assert [leg["input"] for leg in r["burst_client"]] == ["webcam", "local"]
    for leg in r["burst_client"]:
        assert leg["streams"] == 2 and leg["frames"] == 2 and leg["changed_bytes_per_record"] > 0
        assert 0 < leg["touched_tiles_per_record"] <= leg["tiles_per_state"]
        for name in ("burst_apply", "burst_apply_frames", "multi_ticks", "cores_client"):
            assert leg[name + "_us_per_record"]["median"] > 0

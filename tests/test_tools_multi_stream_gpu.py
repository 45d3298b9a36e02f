"""-m gpu: the tools of the many-streams, many-frames form.  tools/roundtrip --multi S --burst K: a server core makes K ticks of
S cameras in one mi355_diff_multi_stream_cwire_batch, every camera's slice crosses a pipe, a client core applies the ticks
with mi355_apply_multi_cwire_batch, the states are compared at both ends.  tools/bench_multi.py --legs burst prints its line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.parametrize("S,w,h,T,K", [(3, 64, 48, 24, 5), (3, 97, 13, 7, 3)])
def test_roundtrip_multi_burst(S, w, h, T, K):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    assert (w, h) != (97, 13) or (3 * w * h) % 16 != 0
    args = [RT, "--width", str(w), "--height", str(h), "--frames", str(T), "--compact", "--multi", str(S), "--burst", str(K)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["multi"] == S and r["burst"] == K and r["ticks"] == T and r["max_abs_error"] <= 20
    assert r["sender_calls"] == (T + K - 1) // K
    assert 0 < r["changed_bytes"] and r["wire_bytes"] < r["reference_wire_bytes"]


def test_bench_multi_burst_prints_one_line_with_the_three_legs():
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "burst", "--size", "160x140", "--streams", "2",
            "--frames", "3", "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_stream" and r["size"] == "160x140" and len(r["burst"]) == 1
    leg = r["burst"][0]
    assert leg["streams"] == 2 and leg["frames"] == 3 and leg["changed_bytes_per_frame"] > 0
    for name in ("burst_cwire", "multi_ticks", "cores_stream"):
        assert leg[name + "_us_per_frame"]["median"] > 0

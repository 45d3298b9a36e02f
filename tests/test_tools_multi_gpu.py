"""-m gpu: tools/roundtrip --multi S closes the many-cameras loop over the C-ABI alone: mi355_diff_multi_cwire_batch on a
server core, the records through a pipe, mi355_apply_multi_cwire_batch on a client core, the states compared every tick."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.parametrize("S,w,h,T", [(3, 97, 13, 6), (4, 1920, 1080, 4)])
def test_roundtrip_multi(S, w, h, T):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = [RT, "--multi", str(S), "--width", str(w), "--height", str(h), "--frames", str(T), "--compact"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["multi"] == S and r["ticks"] == T and r["max_abs_error"] <= 20
    assert 0 < r["changed_bytes"] and r["wire_bytes"] < r["reference_wire_bytes"]

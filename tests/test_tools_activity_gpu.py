"""-m gpu: the tools of the motion grids.  tools/roundtrip --compact --multi S --activity CELL: after every tick (with --burst K
--burst-client: every burst) the receiver runs mi355_cwire_activity_batch on the records it is about to apply and checks grids
and summaries against a plain C++ count over records it decodes itself; it exits non-zero on a mismatch and prints every
camera's box and active cells of the last tick."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.parametrize("burst", [(), ("--burst", "4", "--burst-client")], ids=["ticks", "burst-client"])
def test_roundtrip_multi_activity(burst):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = [RT, "--width", "64", "--height", "48", "--compact", "--multi", "3", "--activity", "16", *burst]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["ticks"] == 24 and r["max_abs_error"] <= 20
    a = r["activity"]
    assert a["cell"] == 16 and a["grid"] == [4, 3] and a["checked_calls"] == (6 if burst else 24) and len(a["cameras"]) == 3
    for cam in a["cameras"]:   # the moving block: 17 x 13 pixels from row 16 on
        x0, y0, x1, y1 = cam["box"]
        assert cam["entries"] > 0 and 0 <= x0 <= x1 < 64 and y0 == 16 and y1 == 28 and 1 <= cam["active_cells"] <= 12

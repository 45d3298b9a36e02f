"""-m gpu: the tools of the record check.  tools/roundtrip --compact --multi S --check: before it applies a tick (with --burst K
--burst-client: a burst) the receiver runs mi355_cwire_check_batch on the records it received and requires every verdict clean,
equal to mi355_cwire_check_host's, and word 3 equal to 1 + the last byte the apply then changes; a damaged copy of the first
non-empty record must come back with MI355_CWIRE_BAD_CODES.  It exits non-zero when any of this fails."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.parametrize("burst", [(), ("--burst", "8", "--burst-client")], ids=["ticks", "burst-client"])
def test_roundtrip_multi_check(burst):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = [RT, "--width", "160", "--height", "140", "--compact", "--multi", "4", "--check", *burst]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["multi"] == 4 and r["ticks"] == 24 and r["max_abs_error"] <= 20
    assert r["check"] == {"records": 4 * 24, "damaged_copy": "bad_codes"}


def test_roundtrip_check_needs_the_multi_receiver():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run([RT, "--compact", "--check"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--check needs" in out.stderr

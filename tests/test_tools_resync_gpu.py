"""-m gpu: the tool of the resynchronisation calls.  tools/roundtrip --compact --multi S --resync K: at tick K the receiver drops
one camera's record; after tick K + 1 it digests its states (mi355_state_digest_batch), the sender answers with a tile mask and
refresh records (mi355_refresh_cwire_batch), the receiver clears (mi355_state_clear_tiles_batch) and applies them.  The tool
requires the dropped camera's frames to differ from the sender's between the loss and the refresh, and every frame to equal the
sender's from then on; it exits non-zero when any of this fails.  With --burst B the sender is a burst ahead when it answers."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.parametrize("burst", [(), ("--burst", "4")], ids=["ticks", "burst"])
def test_roundtrip_multi_resync(burst):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = [RT, "--width", "96", "--height", "64", "--frames", "10", "--compact", "--multi", "3", "--resync", "4", *burst]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["ticks"] == 10 and r["resync"] == 4
    assert r["dropped_camera"] == 4 % 3 and r["dropped_entries"] > 0
    assert r["tiles"] == 5 and 1 <= r["tiles_selected"] <= 3 * 5
    # the loss at tick 4; the digests after tick 5; plain ticks: refreshed behind tick 5, bursts of 4: behind tick 7
    assert r["wrong_ticks"] == (4 if burst else 2) and r["ticks_equal_after_refresh"] == (2 if burst else 4)
    assert r["refresh_bytes"] < r["key_frame_bytes"]


def test_roundtrip_resync_needs_the_multi_receiver():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run([RT, "--compact", "--resync", "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--resync K needs" in out.stderr

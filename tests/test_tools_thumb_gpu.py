"""-m gpu: the tool of the thumbnail records.  tools/roundtrip --compact --multi S --thumb K: behind every tick -- every burst with
--burst T -- the sender makes the touched-tile mask of its own records (mi355_cwire_touched_tiles_batch) and ONE thumbnail record
per camera (mi355_thumb_cwire_batch, threshold 0); each goes through a pipe of its own to a host-only viewer
(mi355_cwire_apply_host on S frames of tw x th pixels) that joined late with key records.  After every tick or burst the tool
compares the viewer with a plain C++ box average of the sender's downloaded states and exits non-zero when they differ.  With
--thumb-drop TICK the viewer loses one camera's record, its picture is checked to be wrong, the key-record procedure repairs it.
100x60 at K = 2: thumbnails of 50x30, two thumbnail tiles, the second partial."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")
# extra arguments -> (comparisons besides the one behind the join, calls, repairs)
MODES = {"ticks": ((), 24, 25, 0), "burst": (("--burst", "4"), 6, 7, 0), "drop": (("--thumb-drop", "3"), 24, 26, 1)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_roundtrip_multi_thumb(mode):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    extra, compared, calls, repaired = MODES[mode]
    args = [RT, "--width", "100", "--height", "60", "--compact", "--multi", "3", "--thumb", "2", *extra]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["ticks"] == 24
    t = r["thumb"]
    assert t["scale"] == 2 and t["size"] == [50, 30]
    assert (t["viewers_equal"], t["calls"], t["repaired"]) == (compared + 1, calls, repaired)
    assert t["wire_bytes"] >= 8 * 3 * calls and r["wire_bytes"] > 0


def test_roundtrip_thumb_needs_the_multi_sender():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    for args in (["--compact", "--thumb", "2"], ["--compact", "--multi", "3", "--thumb", "17"],
                 ["--compact", "--multi", "3", "--thumb", "2", "--wall", "2"], ["--compact", "--multi", "3", "--thumb-drop", "3"]):
        out = subprocess.run([RT, *args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--thumb K needs" in out.stderr
    out = subprocess.run([RT, "--compact", "--multi", "3", "--thumb", "2", "--thumb-drop", "24"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--thumb-drop TICK needs" in out.stderr

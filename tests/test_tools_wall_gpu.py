"""-m gpu: the tool of the wall calls.  tools/roundtrip --compact --multi S --wall K: the receiver keeps a wall of ceil(sqrt(S))
columns of thumbnails at scale K, composed fully once (mi355_wall_compose_batch); after every tick's apply -- every burst's with
--burst B --burst-client -- it makes the touched-tile mask of the records (mi355_cwire_touched_tiles_batch) and runs the masked
compose, and with --resync R the refresh's own mask goes through the same masked compose.  After every tick or burst the tool
compares the wall, pitch gaps and the pattern between the thumbnails included, with a plain C++ box average of the receiver's
states and exits non-zero when they differ.  97x65 at K = 4: thumbnails of 25x17 with ragged blocks at both edges."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")
MODES = {"ticks": ((), 10), "burst": (("--burst", "8", "--burst-client"), 2), "resync": (("--resync", "3"), 11)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_roundtrip_multi_wall(mode):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    extra, walls = MODES[mode]
    args = [RT, "--width", "97", "--height", "65", "--frames", "10", "--compact", "--multi", "4", "--wall", "4", *extra]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["multi"] == 4 and r["ticks"] == 10
    wall = r["wall"]
    assert wall["scale"] == 4 and wall["thumb"] == [25, 17] and wall["size"] == [2 * 26 + 1, 2 * 18 + 1]
    # one comparison per tick (10), per burst (8 + 2), or per tick and one more behind the refresh
    assert wall["walls_equal"] == walls and wall["composes"] == walls + 1


def test_roundtrip_wall_needs_the_multi_receiver():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    for args in (["--compact", "--wall", "4"], ["--compact", "--multi", "4", "--wall", "17"],
                 ["--compact", "--multi", "4", "--burst", "8", "--wall", "4"]):
        out = subprocess.run([RT, *args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--wall K needs" in out.stderr

"""-m gpu: the tools of the mosaic call.  tools/roundtrip --compact --multi S --mosaic CxR [--burst K]: a server core makes the
records of S cameras, a relay that holds no frame makes ONE record of a canvas of C x R cells per tick -- of a burst, of the
coalesced burst -- (mi355_cwire_mosaic_cwire_batch) and forwards it, a viewer that holds one C*W x R*H host state applies it; after
every tick or burst its canvas is compared with the tiling of the server's states and of full-size host clients.
tools/bench_multi.py --legs mosaic prints one line."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")
BASE = [RT, "--width", "64", "--height", "48", "--compact", "--multi", "4"]


@pytest.mark.parametrize("burst", [0, 4])
def test_roundtrip_multi_mosaic(burst):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = BASE + ["--mosaic", "2x2"] + (["--burst", str(burst)] if burst else [])
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])           # the verification line
    assert r["roundtrip"] == "ok" and r["multi"] == 4 and r["burst"] == burst and r["mosaic"] == [2, 2] and r["ticks"] == 24
    assert r["width"] == 64 and r["height"] == 48 and r["canvas"] == [128, 96] and r["relay_calls"] == (6 if burst else 24)
    assert r["canvases_equal_every_step"] is True
    assert 0 < r["canvas_entries"] <= r["changed_bytes"]
    assert 0 < r["relay_forwarded_bytes"] <= r["relay_received_bytes"]


def test_roundtrip_mosaic_with_an_empty_cell():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run([RT, "--width", "33", "--height", "7", "--compact", "--multi", "3", "--mosaic", "2x2"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["canvas"] == [66, 14] and r["canvases_equal_every_step"] is True


@pytest.mark.parametrize("grid", ["1x2", "0x4", "2", "2x2x2", "-2x-2"])
def test_roundtrip_mosaic_grid_must_hold_the_cameras(grid):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + ["--mosaic", grid], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--mosaic" in out.stderr


def test_roundtrip_mosaic_needs_many_cameras():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run([RT, "--compact", "--mosaic", "2x2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--mosaic" in out.stderr


def test_bench_multi_mosaic_prints_one_line():
    import sys
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "mosaic", "--size", "64x48", "--streams", "4",
            "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_mosaic" and r["size"] == "64x48" and len(r["mosaic"]) == 4
    assert [(leg["frames"], leg["input"]) for leg in r["mosaic"]] == [(1, "webcam"), (1, "local"), (16, "webcam"), (16, "local")]
    for leg in r["mosaic"]:
        assert leg["streams"] == 4 and leg["grid"] == [2, 2] and leg["canvas"] == [128, 96]
        # (the local input's block is back where it began after 16 frames of a 64-pixel row: that burst sums to nothing)
        assert leg["route_record_equals_mosaic"] is True and (leg["canvas_entries"] > 0 or leg["frames"] == 16)
        for name in ("mosaic", "state_route"):
            assert leg[name + "_us_per_record"]["median"] > 0

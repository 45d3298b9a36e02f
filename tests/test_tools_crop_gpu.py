"""-m gpu: the tool of the crop call.  tools/roundtrip --compact --multi S --crop X,Y,W,H [--burst K]: a server core makes the
records of S cameras, a relay that holds no frame cuts every camera's records -- of a burst, the coalesced burst -- to the
rectangle (mi355_cwire_crop_cwire_batch) and forwards those, a client core of W x H pixels, seeded from the cropped base frames,
applies them with one mi355_apply_multi_cwire_batch; after every tick or burst its states are compared with the crop of the
server's states and of full-size host clients."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")
BASE = [RT, "--width", "64", "--height", "48", "--compact", "--multi", "3"]


@pytest.mark.parametrize("burst", [0, 4])
def test_roundtrip_multi_crop(burst):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = BASE + ["--crop", "8,4,40,30"] + (["--burst", str(burst)] if burst else [])
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])           # the verification line
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["burst"] == burst and r["crop"] == [8, 4, 40, 30] and r["ticks"] == 24
    assert r["width"] == 64 and r["height"] == 48 and r["relay_calls"] == (6 if burst else 24)
    assert r["cropped_states_equal_every_step"] is True
    assert 0 < r["cropped_entries"] < r["changed_bytes"]
    assert 0 < r["relay_forwarded_bytes"] < r["relay_received_bytes"]


@pytest.mark.parametrize("rect", ["30,4,40,30", "8,20,40,30", "8,4,0,30", "-1,4,40,30", "8,4,40"])
def test_roundtrip_crop_rectangle_must_lie_inside_the_frame(rect):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + ["--crop", rect], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--crop" in out.stderr


def test_roundtrip_crop_needs_many_cameras():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run([RT, "--compact", "--crop", "1,1,2,2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--crop" in out.stderr


def test_bench_multi_crop_prints_one_line_with_all_three_legs():
    import sys
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "crop", "--size", "64x48", "--streams", "2",
            "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_crop" and r["size"] == "64x48" and len(r["crop"]) == 2
    assert [leg["input"] for leg in r["crop"]] == ["webcam", "local"]
    for leg in r["crop"]:
        assert leg["streams"] == 2 and leg["frames"] == 1 and leg["rectangle"] == [16, 12, 32, 24]
        assert 0 < leg["quarter_entries_per_stream"] <= leg["input_entries_per_stream"]
        for name in ("coalesce", "crop_quarter", "crop_full"):
            assert leg[name + "_us_per_stream"]["median"] > 0

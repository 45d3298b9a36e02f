"""-m gpu: the tool of the split call.  tools/roundtrip --compact --multi S [--burst K --coalesce] --datagram BYTES: a server core
makes the records of S cameras, a relay that holds no frame cuts every camera's record of a tick -- with --burst K --coalesce the
coalesced record of the burst -- into pieces of at most BYTES bytes (mi355_cwire_split_cwire_batch), every piece travels as one
datagram, and a client core applies each camera's pieces in a shuffled order, padded with empty records to a common count, with
mi355_apply_multi_stream_cwire_batch; after every tick or burst its states are compared with the server's and with host clients
that applied the original records."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")
BASE = [RT, "--width", "160", "--height", "120", "--compact", "--multi", "3"]


@pytest.mark.parametrize("burst", [0, 4])
def test_roundtrip_multi_datagram(burst):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    args = BASE + (["--burst", str(burst), "--coalesce"] if burst else []) + ["--datagram", "1400"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])           # the verification line
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["burst"] == burst and r["coalesce"] is bool(burst)
    assert r["datagram"] == 1400 and r["ticks"] == 24 and r["width"] == 160 and r["height"] == 120
    steps = 6 if burst else 24
    assert r["relay_calls"] == steps
    # a camera's block is 41 x 31 pixels, 3813 bytes: the first records alone need several datagrams each
    assert r["pieces"] > 3 * steps and 0 < r["largest_piece"] <= 1400
    assert r["pieces_per_tick"] == pytest.approx(r["pieces"] / steps, abs=0.01)
    assert r["piece_bytes_per_tick"] == pytest.approx(r["piece_bytes"] / steps, abs=0.1)
    assert r["piece_bytes"] >= r["pieces"] * 8


def test_roundtrip_datagram_at_the_least_size():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + ["--frames", "4", "--datagram", "64"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["largest_piece"] <= 64
    assert r["pieces"] > 3 * 2 * 64   # the first tick: 3813 entries a camera, more than 128 pieces: three calls of the receiver


@pytest.mark.parametrize("size", ["60", "1402", "65540", "-4"])
def test_roundtrip_datagram_size_must_be_in_range(size):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + ["--datagram", size], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--datagram" in out.stderr


def test_bench_multi_split_prints_one_line_with_all_three_legs():
    import sys
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "split", "--size", "160x120", "--streams", "2",
            "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_split" and r["size"] == "160x120" and len(r["split"]) == 2 and "coalesce" in r["verdict"]
    assert [leg["input"] for leg in r["split"]] == ["webcam", "local"]
    for leg in r["split"]:
        assert leg["streams"] == 2 and leg["frames"] == 1
        assert leg["pieces_per_stream_1400"] >= leg["pieces_per_stream_8972"] >= 1
        for name in ("coalesce", "split_1400", "split_8972"):
            assert leg[name + "_us_per_record"]["median"] > 0


def test_roundtrip_datagram_needs_many_cameras_and_a_coalesced_burst():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    for args in ([RT, "--compact", "--datagram", "1400"], BASE + ["--burst", "4", "--datagram", "1400"]):
        out = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--datagram" in out.stderr

"""-m gpu: the tool of the parity calls.  tools/roundtrip --compact --multi S [--burst K --coalesce] --datagram BYTES --fec G[,K]:
the relay of the datagram mode calls mi355_cwire_fec_batch behind its split call, every parity block is one more datagram, the
tool's seeded generator loses up to K datagrams of every group -- one piece; a piece and P; a piece and Q; two pieces; parity
only, class by class -- and the receiver rebuilds the lost pieces with one mi355_cwire_fec_repair_batch per tick, checks them
(mi355_cwire_check_batch) and applies them with the survivors in a shuffled order; after every tick its states are compared
with the server's and with host clients that applied the original records.  The tool's default geometry (320 x 180)."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")
BASE = [RT, "--compact", "--multi", "3"]
PLAIN_KEYS = ["roundtrip", "format", "multi", "burst", "coalesce", "datagram", "relay_calls", "width", "height", "ticks", "changed_bytes",
              "relay_received_bytes", "pieces", "piece_bytes", "pieces_per_tick", "piece_bytes_per_tick", "largest_piece", "raw_bytes",
              "max_abs_error"]


def run(args):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])           # the verification line


@pytest.mark.parametrize("fec,burst", [("8,2", 0), ("4,1", 0), ("8,2", 4)])
def test_roundtrip_datagram_with_parity(fec, burst):
    G, K = (int(v) for v in fec.split(","))
    r = run((["--burst", str(burst), "--coalesce"] if burst else []) + ["--datagram", "1400", "--fec", fec])
    assert r["roundtrip"] == "ok" and r["multi"] == 3 and r["datagram"] == 1400 and r["fec"] == [G, K]
    assert r["width"] == 320 and r["height"] == 180 and r["ticks"] == 24
    assert r["pieces_rebuilt"] == r["pieces_lost"] > 0
    groups = r["parity_datagrams"] // K
    assert r["parity_datagrams"] == groups * K and -(-r["pieces"] // G) <= groups <= r["pieces"]
    assert 8 * r["parity_datagrams"] <= r["parity_bytes"] <= 1400 * r["parity_datagrams"]
    assert r["pieces_lost"] <= K * groups


def test_the_default_parity_count_is_one():
    r = run(["--frames", "6", "--datagram", "1400", "--fec", "4"])
    assert r["fec"] == [4, 1] and r["pieces_rebuilt"] == r["pieces_lost"] > 0


def test_the_plain_datagram_line_is_unchanged():
    r = run(["--datagram", "1400"])
    assert list(r) == PLAIN_KEYS and r["roundtrip"] == "ok"


@pytest.mark.parametrize("args", [["--fec", "8,2"], ["--datagram", "1400", "--fec", "0"], ["--datagram", "1400", "--fec", "256"],
                                  ["--datagram", "1400", "--fec", "8,3"], ["--datagram", "1400", "--fec", "8,2,1"]])
def test_fec_needs_a_datagram_size_and_a_valid_shape(args):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--fec" in out.stderr

"""-m gpu: the tools of the run-coded records.  tools/roundtrip --compact --multi S --runs: behind whatever relay steps were asked
for, the records cross the stream socket as mi355_cwire_runs_encode_batch wrote them (forms table, then bytes) and the receiver
decodes them with mi355_cwire_runs_decode_batch before it does what it did without the flag; the tool compares the decoded bytes
with the sender's and prints a line with the compact bytes, the link bytes and the records packed.  The link bytes are checked
against tests/runs_spec.py on the tool's own seeded frames, rebuilt here.  tools/bench_multi.py --legs runs prints one line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cwire_spec as spec
import runs_spec as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "tools", "roundtrip")
W, H, S, T = 64, 48, 2, 6
BASE = [RT, "--width", str(W), "--height", str(H), "--frames", str(T), "--compact", "--multi", str(S)]


def tool_frames(K):
    """The frames tools/roundtrip draws (Cameras::fill, make_frame, its seeded generator), in its order: bursts of K ticks,
    stream-major inside a burst -> (bases [S][n], frames [T][S][n])."""
    n = 3 * W * H
    i = np.arange(n, dtype=np.int64)
    bases = np.stack([(40 + (i * 7 + s * 31) % 150).astype(np.uint8) for s in range(S)])
    state = 12345
    frames = np.empty((T, S, n), np.uint8)
    bw, bh, y0 = W // 4 + 1, H // 4 + 1, H // 3
    for t0 in range(0, T, K):
        for s in range(S):
            for k in range(min(K, T - t0)):
                noise = np.empty(n, np.uint8)
                for j in range(n):
                    state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
                    noise[j] = (state >> 24) % 9
                f = (bases[s] + noise).reshape(H, W, 3)
                x0 = ((t0 + k + 5 * s) * 3) % (W - bw + 1)
                f[y0:min(y0 + bh, H), x0:x0 + bw] = np.array([200, 210, 220], np.uint8)
                frames[t0 + k, s] = f.reshape(-1)
    return bases, frames


def link_sums(K):
    """(records, compact bytes, link bytes, records packed) of what crosses the link: a tick's S records, or with K > 1 the S
    coalesced records of every burst of K ticks."""
    bases, frames = tool_frames(K)
    states = bases.copy()
    nrec = compact = link = packed = 0
    for t0 in range(0, T, K):
        before = states.copy()
        for t in range(t0, min(t0 + K, T)):
            df = frames[t].astype(np.int16) - states.astype(np.int16)
            hit = np.abs(df) > 20
            states[hit] = frames[t][hit]
        recs = []
        for s in range(S):
            xs = np.flatnonzero(states[s] != before[s])   # (one tick: its entries; a burst: the sums that do not cancel)
            recs.append(np.frombuffer(spec.encode_frame(xs, (states[s][xs] - before[s][xs]).astype(np.uint8)), np.uint8))
        buf = np.concatenate(recs)
        forms, pos, _ = rs.encode(buf, S, rs.WHERE_SMALLER)
        nrec, compact, link, packed = nrec + S, compact + buf.size, link + int(pos[-1]), packed + int(forms[:, 0].sum())
    return nrec, compact, link, packed


@pytest.mark.parametrize("extra,K", [([], 1), (["--burst", "2", "--coalesce"], 2)])
def test_roundtrip_runs(extra, K):
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + extra + ["--runs"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1]["roundtrip"] == "ok" and lines[-1]["multi"] == S
    r = [ln for ln in lines if ln.get("runs") is True]
    assert len(r) == 1
    nrec, compact, link, packed = link_sums(K)
    assert (r[0]["records"], r[0]["compact_bytes"], r[0]["link_bytes"], r[0]["records_packed"]) == (nrec, compact, link, packed)
    assert r[0]["forms_table_bytes"] == 16 * nrec and 0 < packed and link < compact


@pytest.mark.parametrize("extra", [["--burst", "2"], ["--burst", "2", "--burst-client"], ["--mosaic", "2x1"], ["--resync", "2"],
                                   ["--resync", "2", "--burst", "2"]])
def test_roundtrip_runs_composes_with_the_other_modes(extra):
    """The link behind a burst, a burst client, a mosaic relay (records of the canvas) and a resync (ticks and the refresh records):
    the mode's own checks pass and the link never carries more than the compact records."""
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + extra + ["--runs"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1]["roundtrip"] == "ok"
    r = [ln for ln in lines if ln.get("runs") is True]
    assert len(r) == 1 and r[0]["records"] > 0 and 0 < r[0]["link_bytes"] <= r[0]["compact_bytes"] and r[0]["records_packed"] > 0


def test_roundtrip_runs_is_refused_with_datagram():
    assert os.path.exists(RT), "tools/roundtrip is not built"
    out = subprocess.run(BASE + ["--datagram", "1400", "--runs"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--runs" in out.stderr


def test_bench_multi_runs_prints_one_line():
    args = [sys.executable, os.path.join(ROOT, "tools", "bench_multi.py"), "--legs", "runs", "--size", "64x48", "--streams", "2", "--rounds", "1"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["bench"] == "multi_runs" and r["size"] == "64x48" and len(r["runs"]) == 3 and "coalesce" in r["verdict"]
    assert [leg["input"] for leg in r["runs"]] == ["webcam", "local", "keyframe"]
    for leg in r["runs"]:
        assert leg["streams"] == 2 and leg["frames"] == 1 and leg["records"] == 2 and 0 <= leg["records_packed"] <= 2
        assert 0 < leg["bytes_out_per_stream"] <= leg["bytes_in_per_stream"]
        for name in ("coalesce", "encode", "decode"):
            assert leg[name + "_us_per_record"]["median"] > 0
        for name in ("encode", "decode"):
            assert isinstance(leg[name + "_no_slower_than_coalesce"], bool) and leg[name + "_over_coalesce"] > 0
    key = r["runs"][2]
    assert key["records_packed"] == 2 and key["bytes_out_over_in"] < 0.6

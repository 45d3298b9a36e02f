"""bench.py's plain run and --dump-outputs: the line carries the headline keys and none of --full's, --steps sets the
timed steps, and the files hold what the last timed step handed its caller -- the same, byte for byte, as the oracle's
stream after warm-up + timed passes over the batch from the base frame (the preheat in front of them does not count)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cudavideostream_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_step(po, tmp_path):
    W, H, B, K, WU = 160, 90, 6, 3, 2
    out_dir = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(WU),
           "--width", str(W), "--height", str(H), "--batch", str(B), "--preheat-s", "0.2", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in r.stdout.decode(errors="replace").splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == K and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "frames/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8" and line["preheat"]["steps"] > 0
    for key in ("cold_start_window", "steady_state", "pair_mode", "regimes", "board", "host_path", "parity"):
        assert key not in line, key
    assert line["cpu_baseline"] is None

    d = {n[:-4]: np.load(os.path.join(out_dir, n)) for n in os.listdir(out_dir)}
    assert set(d) == {"offsets", "xs_sum", "diff_sum", "pos", "xs", "diff", "state_pos", "state"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    base, frames = synth.webcam_stream(B, W, H, seed=21)
    state = base
    for _ in range(WU + K):
        eo, exs, edf, state = po.diff_stream(frames, state)
    assert np.array_equal(d["offsets"], eo.astype(np.float64))
    p = int(eo[-1])
    assert p > 0 and np.array_equal(d["pos"], np.arange(p))      # fewer entries than the sample: all of them
    assert np.array_equal(d["xs"], exs.astype(np.float64)) and np.array_equal(d["diff"], edf.astype(np.float32))
    for t in range(B):
        a, b = int(eo[t]), int(eo[t + 1])
        assert d["xs_sum"][t] == exs[a:b].astype(np.int64).sum() and d["diff_sum"][t] == edf[a:b].astype(np.int64).sum()
    assert np.array_equal(d["state_pos"], np.arange(state.size)) and np.array_equal(d["state"], state.astype(np.float32))

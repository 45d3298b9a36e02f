"""-m gpu: tools/diffbench --consecutive runs mi355_diff_consecutive_batch and mi355_diff_pairs_batch on the same views of
one buffer of B + 1 frames, prints the time per pair of both and says whether offsets and entries are equal."""
import json
import os
import subprocess

import pytest

from cudavideostream_amd import synth
from gpu_util import oracle_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "diffbench")


def test_consecutive_mode_reports_equal_outputs(po):
    w, h, B = 160, 140, 9
    r = subprocess.run([EXE, "--consecutive", "--width", str(w), "--height", str(h), "--batch", str(B), "--steps", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["mode"] == "consecutive" and line["outputs"] == "equal"
    assert line["consecutive_us_per_pair"] > 0 and line["pairs_us_per_pair"] > 0
    # the tool's frames are synth.py's (test_tools_gpu.py): frame t - 1 of the stream is frame t's predecessor, the base frame 0's
    base, frames = synth.webcam_stream(B, w, h, seed=21)
    off, _, _ = oracle_pairs(po, frames, [base, *frames[:-1]])
    assert abs(line["changed_bytes_per_frame"] * B - int(off[-1])) < 0.5 * B

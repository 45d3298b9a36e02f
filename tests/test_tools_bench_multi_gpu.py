"""-m gpu: every --legs value of tools/bench_multi.py prints what it printed before the tool's legs were put on one input
function, one record maker, one timing loop and one report.  The inputs are hash-seeded, so every field of a line that does not
depend on a clock is a pure function of the arguments: tests/golden/bench_multi_lines.json holds the lines of the tool as it was
before that change, one run with --rounds 1 per case below, and each case's lines must equal them key for key and in key order
once the clock-dependent fields (CLOCK, by name) are replaced by their shape.  Of those the test checks presence and type, and
a positive median of every statistics object.

Sizes: the seven legs that a tests/test_tools_*_gpu.py already runs keep that test's arguments; the others run at 64x48 with two
streams (and two steps where the leg takes them), at which every leg's own assertions hold -- but for the refresh leg, which
runs at 320x216: its 1 % receiver changes a byte in the 51st tile of every state (byte 50 * 4096 + 1234), and 207360 bytes are
the first state of a usual aspect that has that byte; below 51 tiles the leg ends where it builds that receiver."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bench_multi.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bench_multi_lines.json")

SMALL = ["--size", "64x48", "--streams", "2"]
CASES = {
    "default": SMALL + ["--steps", "2"],
    "multi_pairs_write_probe": ["--legs", "multi,pairs,write_probe"] + SMALL + ["--steps", "2"],
    "client": ["--legs", "client"] + SMALL + ["--steps", "2"],
    "burst": ["--legs", "burst", "--size", "160x140", "--streams", "2", "--frames", "3"],
    "burst_client": ["--legs", "burst_client"] + SMALL + ["--frames", "2"],
    "coalesce": ["--legs", "coalesce"] + SMALL + ["--frames", "2"],
    "crop": ["--legs", "crop"] + SMALL,
    "split": ["--legs", "split", "--size", "160x120", "--streams", "2"],
    "fec": ["--legs", "fec"] + SMALL,
    "mosaic": ["--legs", "mosaic", "--size", "64x48", "--streams", "4"],
    "budget": ["--legs", "budget", "--size", "64x48", "--streams", "2,3"],
    "activity": ["--legs", "activity"] + SMALL,
    "check": ["--legs", "check"] + SMALL,
    "refresh": ["--legs", "refresh", "--size", "320x216", "--streams", "2"],
    "wall": ["--legs", "wall"] + SMALL,
    "thumb": ["--legs", "thumb"] + SMALL,
}

KINDS, SCALES = ("webcam", "local"), (2, 4, 8)
# ---- the clock-dependent fields, by name (each is computed from time.perf_counter() differences and from nothing else
# that varies; `hbm_write_gbps` is the library's own timed probe)
STATS = (
    [n + "_us_per_frame" for n in ("multi", "multi_cwire", "pairs", "cores_loop", "burst_cwire", "multi_ticks", "cores_stream")]
    + [n + "_us_per_stream" for n in ("multi_client", "cores_client", "decode_arrays", "budget", "second_diff", "coalesce", "crop_quarter",
                                      "crop_full", "digest", "digest_skewed", "refresh_1pct", "refresh_10pct", "refresh_all", "clear_10pct",
                                      "diff", "full_skewed_k4")]
    + [f"{n}_k{k}_us_per_stream" for n in ("full", "masked_webcam", "masked_local") for k in SCALES]
    + [f"{n}_{kind}_k{k}_us_per_stream" for n in ("touched_plus_call", "call", "call_nullmask", "route") for kind in KINDS for k in SCALES]
    + [n + "_us_per_record" for n in ("burst_apply", "burst_apply_frames", "multi_ticks", "cores_client", "activity", "check", "coalesce",
                                      "split_1400", "split_8972", "split", "fec_k1", "fec_k2", "mosaic", "state_route")]
    + ["coalesce_us_per_input_record", "state_route_us_per_input_record", "repair_one_us_per_job", "repair_two_us_per_job"])
RATIOS = ["cores_loop_over_multi", "multi_over_pairs", "cores_client_over_multi_client", "decode_arrays_over_multi_client",
          "multi_ticks_over_burst", "cores_stream_over_burst", "multi_ticks_over_burst_apply", "cores_client_over_burst_apply",
          "activity_over_burst_apply", "check_over_burst_apply", "digest_over_diff", "full_k8_over_digest", "state_route_over_coalesce",
          "crop_quarter_over_coalesce", "crop_full_over_coalesce", "split_1400_over_coalesce", "split_8972_over_coalesce",
          "fec_k1_over_split", "fec_k2_over_split", "mosaic_over_route", "second_diff_over_budget",
          "full_minus_coalesce_us_per_call", "hbm_write_gbps"]
RATIO_TABLES = ["masked_local_over_full", "touched_plus_call_over_route", "call_local_over_nullmask"]     # {point: ratio}
FLAGS = ["no_slower_than_burst_apply", "digest_no_slower_than_diff", "masked_local_cheaper_than_full", "full_k8_no_slower_than_digest",
         "touched_plus_call_no_slower_than_route", "call_local_cheaper_than_nullmask", "quarter_no_slower_than_coalesce",
         "split_1400_no_slower_than_coalesce", "split_8972_no_slower_than_coalesce", "fec_k2_no_slower_than_split",
         "mosaic_no_slower_than_route"]
CLOCK = set(STATS) | set(RATIOS) | set(RATIO_TABLES) | set(FLAGS) | {"verdict"}


def number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def shape_of(key, v):
    """Checks a clock-dependent field's type and returns what stands for it in the comparison: its kind and its own keys."""
    if key in STATS:
        assert isinstance(v, dict) and all(number(x) for x in v.values()), (key, v)
        assert v["median"] > 0 and v["min"] <= v["median"] <= v["max"], (key, v)
        return {"statistics": list(v)}                  # median, min, max, and spread where the leg prints it
    if key in RATIO_TABLES:
        assert isinstance(v, dict) and all(number(x) for x in v.values()), (key, v)
        return {"ratios": list(v)}
    if key in FLAGS:
        assert isinstance(v, bool), (key, v)
        return "flag"
    if key == "verdict":
        assert isinstance(v, str) and v, v
        return "text"
    assert number(v), (key, v)
    return "number"


def masked(obj):
    if isinstance(obj, dict):
        return {k: shape_of(k, v) if k in CLOCK else masked(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [masked(v) for v in obj]
    return obj


@pytest.fixture(scope="module")
def parent_lines():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_bench_multi_prints_the_lines_it_printed_before(case, parent_lines):
    out = subprocess.run([sys.executable, TOOL] + CASES[case] + ["--rounds", "1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.strip()]
    want = parent_lines[case]
    assert len(lines) == len(want) == 1                 # one line per run; the default legs print one per S, and S is one value here
    for got, ref in zip(lines, want):
        # json.dumps keeps the order of the keys, so equal texts are equal key for key and in key order
        assert json.dumps(masked(got), indent=1) == json.dumps(masked(ref), indent=1)

#!/usr/bin/env python3
"""Secondary benchmark: pairs of consecutive frames of ONE buffer of T + 1 frames, the two ways the library diffs them
(include/mi355diff.h).  Not the headline metric (bench.py).

  consecutive  mi355_diff_consecutive_batch(first_prev = buffer, frames = buffer + N): every frame is read once, the
               previous frame of a tile stays in the wave's registers;
  pairs        mi355_diff_pairs_batch(cur = buffer + N, prev = buffer): both operands of every pair come from memory.

Configurations: 1080p with T = 128 and 4K with T = 64, S1 webcam-like input resident in HBM, threshold 20.  Both legs run in
ONE process on one core's own stream, alternating within every round, behind a preheat; a leg's window is `calls` calls and
one synchronisation (wall clock, what a caller sees), a fraction of a second long.  Round 0 warms both legs up and is
dropped; the object carries median, minimum and maximum of the other rounds in microseconds per pair.  `pairs` runs code this
entry point did not touch: it is the figure of the library without the new call, taken on the same board in the same minute.
Before the rounds the two calls' offsets and entries are compared (they must be equal, bit for bit).

  python tools/bench_consecutive.py > profiles/pair_consecutive.json

Bytes fetched (optional, a run of its own with nothing else collected -- counters and tracing do not go together, and
the counter interposer does not get on with PyTorch's kernels, so it runs the C++ harness):
  MI355_PIPELINE=0 rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- \\
      tools/diffbench --consecutive --width 3840 --height 2160 --batch 64 --steps 1 --warmup 0
  python tools/bench_consecutive.py --into profiles/pair_consecutive.json --fetch-csv DIR/.../*_counter_collection.csv
adds (to the earlier output, printed again; nothing is measured), per form of the pack kernel, FETCH_SIZE of one batch of 64 4K pairs (KiB as the tool reports them, and bytes with the
gfx950 correction of profiles/summarize.py: a wide coalesced read request of 128 bytes is tallied as 64)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("1080p", 1920, 1080, 128), ("4k", 3840, 2160, 64)]


def stats(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}


def run(name, W, H, T, rounds, window_s, preheat_s):
    import torch
    from cudavideostream_amd import CUDACore, lib, synth
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    base, frames = synth.webcam_stream(T, W, H, device=dev)
    buf = torch.cat([base.reshape(1, n), frames.reshape(T, n)])   # frame t's predecessor is row t
    del base, frames
    cap = T * n // 8                                   # S1 changes ~2 % of the bytes
    outs = [(torch.zeros(T + 1, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
             torch.empty(cap, dtype=torch.uint8, device=dev)) for _ in range(2)]
    core = CUDACore(W, H, max_batch=T)
    core.prepare(lib.PREPARE_BATCHES)
    torch.cuda.synchronize()

    def consecutive(o):
        core.diff_consecutive_batch(buf[0], buf[1:], T, o[0], o[1], o[2], cap)

    def pairs(o):
        core.diff_pairs_batch(buf[1:], buf[:T], T, o[0], o[1], o[2], cap)

    legs = {"consecutive": consecutive, "pairs": pairs}
    # the same answer, bit for bit
    consecutive(outs[0])
    pairs(outs[1])
    core.synchronize()
    total = int(outs[0][0].cpu()[-1])
    assert 0 < total <= cap, (total, cap)
    (off0, xs0, df0), (off1, xs1, df1) = outs
    equal = torch.equal(off0, off1) and torch.equal(xs0[:total], xs1[:total]) and torch.equal(df0[:total], df1[:total])
    assert equal, "mi355_diff_consecutive_batch and mi355_diff_pairs_batch disagree"

    def window(leg, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            leg(outs[0])
        core.synchronize()
        return time.perf_counter() - t0

    # preheat (clocks and caches settle), and the number of calls that fills a window
    t_end = time.perf_counter() + preheat_s
    per_call = []
    while time.perf_counter() < t_end:
        per_call = [window(leg, 8) / 8 for leg in legs.values()]
    calls = max(8, int(window_s / max(per_call)))
    times = {k: [] for k in legs}
    for r in range(rounds + 1):                        # round 0 warms both legs up and is dropped
        for k, leg in legs.items():
            dt = window(leg, calls)
            if r:
                times[k].append(dt * 1e6 / (calls * T))
    core.close()
    out = {"size": f"{W}x{H}", "pairs_per_call": T, "calls_per_window": calls, "rounds": rounds,
           "changed_bytes_per_frame": round(total / T, 1), "outputs_equal": bool(equal)}
    for k in legs:
        out[k + "_us_per_pair"] = stats(times[k])
    med = {k: statistics.median(v) for k, v in times.items()}
    out["pairs_over_consecutive"] = round(med["pairs"] / med["consecutive"], 3)
    # algorithmic bytes of a pair over the time: 2N read (the model's) + 5 bytes per entry, of 8 TB/s
    alg = 2 * n + 5 * total / T
    for k in legs:
        out[k + "_frac_of_8TBps"] = round(alg / (med[k] * 1e-6) / 8e12, 4)
    return out


def fetched(path):
    """FETCH_SIZE per form of the pack kernel from a rocprofv3 counter CSV: the sum over the launches of ONE batch (the last
    call of each form; a batch may be packed by two launches)."""
    rows = [r for r in csv.DictReader(open(path)) if r.get("Counter_Name") == "FETCH_SIZE" and "k_diff_pack" in r.get("Kernel_Name", "")]
    out = {}
    for r in rows:
        form = "pairs" if "k_diff_pack<true" in r["Kernel_Name"].replace(" ", "") else "consecutive"
        out.setdefault(form, []).append(float(r["Counter_Value"]))
    res = {}
    for form, v in out.items():
        res[form] = {"launches": len(v), "fetch_size_KiB_all_launches": round(sum(v), 1),
                     "read_bytes_all_launches_corrected": int(2 * sum(v) * 1024)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--preheat-s", type=float, default=1.0)
    ap.add_argument("--fetch-csv", default=None)
    ap.add_argument("--into", default=None, help="an earlier output of this script: only add --fetch-csv's figures to it")
    a = ap.parse_args()
    if a.into:
        result = json.load(open(a.into))
        result["fetch_64_pairs_4k"] = fetched(a.fetch_csv)
        print(json.dumps(result, indent=1))
        return
    assert a.rounds >= 5, "median of at least five rounds"
    import torch
    assert torch.cuda.is_available(), "tools/bench_consecutive.py measures on the GPU only"
    result = {"benchmark": "consecutive pairs of one buffer: mi355_diff_consecutive_batch against mi355_diff_pairs_batch",
              "unit": "microseconds per pair, wall clock around a window of calls and one synchronise",
              "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, W, H, T in CONFIGS:
        result["configs"][name] = run(name, W, H, T, a.rounds, a.window_s, a.preheat_s)
    if a.fetch_csv:
        result["fetch_64_pairs_4k"] = fetched(a.fetch_csv)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

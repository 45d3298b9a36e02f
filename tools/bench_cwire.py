#!/usr/bin/env python3
"""Secondary benchmark: the compact wire format's encoder and decoder (include/mi355diff.h, "compact wire format") on
batches of S1 webcam frames resident in HBM: 1080p with B = 256 and 4K with B = 64.

Prints one JSON line per size: microseconds per frame of diff_stream_batch alone, of the encoder alone, of the two
back to back, of diff_stream_cwire_batch (`direct`: the same records in one call, without the xs / diff arrays) and of
the decoder; compact and reference-wire bytes per frame; and the encoder's achieved GB/s on its
algorithmic bytes (per frame: read 4P + 5P, write 8 + 2 pad4(P) + 4e, P = changed bytes).
The GPU client: apply_cwire_batch (records straight onto a client core's state, one call) with the shown frames written
out (`frames`) and state only (`state`), next to decode + apply_batch in the same two modes, measured in the same run;
for the `frames` mode also the achieved write rate on N bytes per frame.  Not the headline metric (bench.py).

`bench_cwire.py host`: the per-frame host path instead.  1080p webcam-like frames in pinned host memory, a pipe of depth 4:
frames/s and bytes returned per frame of exec_submit_compact (mi355_pipe_submit_cwire) against exec_submit
(mi355_pipe_submit) on the same frames, from the same state, in the same run on the same board; median of five rounds with
their spread, written to profiles/host_cwire.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudavideostream_amd import CUDACore, cwire_bytes_max, lib, synth  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / reps   # us per call


def run(W, H, B, reps):
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    base, frames = synth.webcam_stream(B, W, H, device=dev)
    cap = B * n // 8                               # S1 changes ~2 % of the bytes
    d_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    d_xs = torch.empty(cap, dtype=torch.int32, device=dev)
    d_df = torch.empty(cap, dtype=torch.uint8, device=dev)
    cwcap = cwire_bytes_max(n, B)
    d_pos = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    o_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    o_xs = torch.empty(cap, dtype=torch.int32, device=dev)
    o_df = torch.empty(cap, dtype=torch.uint8, device=dev)
    base_h = base.cpu().numpy()
    with CUDACore(W, H, sample_mat_data=base_h, max_batch=B) as core, CUDACore(W, H, max_batch=1) as client, \
            CUDACore(W, H, sample_mat_data=base_h, max_batch=B) as gclient:
        core.use_torch_stream()
        client.use_torch_stream()
        gclient.use_torch_stream()

        def diff():
            core.diff_stream_batch(frames, B, d_off, d_xs, d_df, cap)

        def encode():
            core.cwire_encode_batch(d_off, d_xs, d_df, cap, B, d_pos, d_cw, cwcap)

        def both():
            diff()
            encode()

        q_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        q_pos = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        q_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)

        def direct():
            core.diff_stream_cwire_batch(frames, B, q_off, q_pos, q_cw, cwcap)

        # the same batch over and over (the state carries over: its first frame is then diffed against its last one)
        us_diff = timed(diff, reps)
        core.set_state(base_h)
        diff()
        torch.cuda.synchronize()
        us_enc = timed(encode, reps)
        us_both = timed(both, reps)
        us_direct = timed(direct, reps)
        core.set_state(base_h)
        diff()
        encode()
        torch.cuda.synchronize()
        core.set_state(base_h)
        direct()
        torch.cuda.synchronize()
        assert torch.equal(q_off, d_off) and torch.equal(q_pos, d_pos)   # the one-call form writes the same records
        assert torch.equal(q_cw[:int(q_pos[-1])], d_cw[:int(d_pos[-1])])
        off = d_off.cpu().numpy().view(np.uint32).astype(np.int64)
        pos = d_pos.cpu().numpy().view(np.uint64).astype(np.int64)
        assert int(off[-1]) <= cap and int(pos[-1]) <= cwcap
        # the headers, as a client reads them from the socket
        buf = d_cw[:int(pos[-1])].cpu().numpy()
        hdr = np.stack([buf[p:p + 8].view("<u4") for p in pos[:-1]])
        counts, escapes = hdr[:, 0].copy(), hdr[:, 1].copy()
        assert np.array_equal(counts.astype(np.int64), np.diff(off))

        def decode():
            client.cwire_decode_batch(d_cw, counts, escapes, B, o_off, o_xs, o_df, cap)

        us_dec = timed(decode, reps)
        torch.cuda.synchronize()
        assert torch.equal(o_off, d_off)

        # the GPU client: one call against decode + apply_batch, both modes
        shown = torch.empty(B * n, dtype=torch.uint8, device=dev)
        shown2 = torch.empty(B * n, dtype=torch.uint8, device=dev)

        def apply_frames():
            gclient.apply_cwire_batch(d_cw, counts, escapes, B, shown, n)

        def apply_state():
            gclient.apply_cwire_batch(d_cw, counts, escapes, B)

        def two_frames():
            client.cwire_decode_batch(d_cw, counts, escapes, B, o_off, o_xs, o_df, cap)
            client.apply_batch(o_off, o_xs, o_df, B, shown2, n)

        def two_state():
            client.cwire_decode_batch(d_cw, counts, escapes, B, o_off, o_xs, o_df, cap)
            client.apply_batch(o_off, o_xs, o_df, B)

        us_af = timed(apply_frames, reps)
        us_as = timed(apply_state, reps)
        us_tf = timed(two_frames, reps)
        us_ts = timed(two_state, reps)
        gclient.set_state(base_h)
        client.set_state(base_h)
        apply_frames()
        two_frames()
        torch.cuda.synchronize()
        assert torch.equal(shown, shown2)   # the one call shows the same frames
        assert np.array_equal(gclient.get_state(), client.get_state())
        del shown, shown2
        P = int(off[-1]) / B
        e = float(escapes.sum()) / B
        pad4 = float(np.sum((np.diff(off) + 3) // 4 * 4)) / B
        alg = 9 * P + 8 + 2 * pad4 + 4 * e
        print(json.dumps({"size": f"{W}x{H}", "batch": B, "changed_bytes_per_frame": round(P, 1),
                          "escapes_per_frame": round(e, 1),
                          "cwire_bytes_per_frame": round(int(pos[-1]) / B, 1),
                          "reference_wire_bytes_per_frame": round(4 + 5 * P, 1),
                          "ratio": round((4 + 5 * P) / (int(pos[-1]) / B), 3),
                          "diff_stream_us_per_frame": round(us_diff / B, 3),
                          "encode_us_per_frame": round(us_enc / B, 3),
                          "diff_plus_encode_us_per_frame": round(us_both / B, 3),
                          "direct_us_per_frame": round(us_direct / B, 3),
                          "direct_over_diff": round(us_direct / us_diff, 3),
                          "direct_over_diff_plus_encode": round(us_direct / us_both, 3),
                          "encode_share_of_diff": round(us_enc / us_diff, 3),
                          "decode_us_per_frame": round(us_dec / B, 3),
                          "encode_algorithmic_bytes_per_frame": int(alg),
                          "encode_achieved_gbps": round(alg * B / (us_enc * 1e-6) / 1e9, 1),
                          "apply_cwire_frames_us_per_frame": round(us_af / B, 3),
                          "apply_cwire_state_us_per_frame": round(us_as / B, 3),
                          "decode_apply_frames_us_per_frame": round(us_tf / B, 3),
                          "decode_apply_state_us_per_frame": round(us_ts / B, 3),
                          "apply_cwire_frames_speedup": round(us_tf / us_af, 2),
                          "apply_cwire_state_speedup": round(us_ts / us_as, 2),
                          "apply_cwire_state_over_direct": round(us_as / us_direct, 3),
                          "apply_cwire_frames_write_tbps": round(n * B / (us_af * 1e-6) / 1e12, 2)}), flush=True)


def run_host(W, H, nbuf, frames_per_round, rounds, out):
    """Both forms of the pipelined per-frame path over the same cycle of nbuf pinned frames (played forth and back, so that
    every step is a webcam-like one), depth 4.  The plain form writes the differences over the head of frame_data: those
    bytes are put back after each wait (a server's next capture does that).  That is work of this harness, not of the entry
    point, and the compact form needs none: its time is taken out of the plain form's figure, and reported by itself."""
    depth = 4
    n = 3 * W * H
    base, frames = synth.webcam_stream(nbuf, W, H, device=torch.device("cuda", 0))
    base, frames = base.cpu().numpy(), frames.cpu().numpy()
    order = list(range(nbuf)) + list(range(nbuf - 2, 0, -1))
    sets = [CUDACore.alloc_arrays(H, W) for _ in range(nbuf)]
    for i in range(nbuf):
        sets[i][0].array[:n] = frames[i]
    xs_ring = [sets[i][3] for i in range(depth)]
    recs = [CUDACore.alloc_record(H, W) for _ in range(depth)]
    cap = recs[0].array.nbytes
    res = {"plain": [], "compact": []}
    info = {}
    with CUDACore(W, H, sample_mat_data=base) as core:
        core.prepare(lib.PREPARE_EXEC | lib.PREPARE_EXEC_CWIRE)
        core.pipe_open(depth)

        def one_round(compact, count):
            core.pipe_close()
            core.set_state(base)
            core.pipe_open(depth)
            tickets, entries, nbytes, restore = [], 0, 0, 0.0
            t0 = time.perf_counter()
            for k in range(count + depth):
                if k >= depth:
                    j = k - depth
                    if compact:
                        pos, _, b = core.exec_wait_compact(tickets[j])
                        nbytes += b
                    else:
                        pos = core.exec_wait(tickets[j])
                        nbytes += 4 + 5 * pos
                        f = order[j % len(order)]
                        r0 = time.perf_counter()
                        sets[f][0].array[:pos] = frames[f][:pos]
                        restore += time.perf_counter() - r0
                    entries += pos
                if k < count:
                    f = order[k % len(order)]
                    if compact:
                        tickets.append(core.exec_submit_compact(sets[f][0].array, None, "", recs[k % depth].array, cap))
                    else:
                        tickets.append(core.exec_submit(sets[f][0].array, None, "", xs_ring[k % depth].array))
            dt = time.perf_counter() - t0
            return count / (dt - restore), nbytes / count, entries, restore / count * 1e6

        for compact in (False, True):   # warm-up, and the two forms see the same entries
            info["entries_compact" if compact else "entries_plain"] = one_round(compact, 2 * len(order))[2]
        assert info["entries_compact"] == info["entries_plain"], info
        restore_us = []
        for _ in range(rounds):
            for compact in (False, True):
                fps, bpf, entries, rus = one_round(compact, frames_per_round)
                res["compact" if compact else "plain"].append((fps, bpf, entries))
                if not compact:
                    restore_us.append(rus)
        core.pipe_close()
    for s in sets:
        for a in s:
            a.free()
    for r in recs:
        r.free()

    def summary(rows):
        fps = [r[0] for r in rows]
        return {"frames_per_s_median": round(statistics.median(fps), 1), "frames_per_s_min": round(min(fps), 1),
                "frames_per_s_max": round(max(fps), 1), "frames_per_s_rounds": [round(v, 1) for v in fps],
                "bytes_returned_per_frame": round(rows[0][1], 1), "entries_per_frame": round(rows[0][2] / frames_per_round, 1)}

    plain, compact = summary(res["plain"]), summary(res["compact"])
    assert res["plain"][0][2] == res["compact"][0][2]
    spread = max(plain["frames_per_s_max"] - plain["frames_per_s_min"], compact["frames_per_s_max"] - compact["frames_per_s_min"])
    result = {"leg": "host", "size": f"{W}x{H}", "depth": depth, "frames_per_round": frames_per_round, "rounds": rounds,
              "device": torch.cuda.get_device_name(0), "pipe_submit": plain, "pipe_submit_cwire": compact,
              "plain_restore_us_per_frame": round(statistics.median(restore_us), 2),
              "bytes_ratio_compact_over_plain": round(compact["bytes_returned_per_frame"] / plain["bytes_returned_per_frame"], 3),
              "speed_ratio_compact_over_plain": round(compact["frames_per_s_median"] / plain["frames_per_s_median"], 3),
              "rounds_spread_frames_per_s": round(spread, 1),
              "compact_no_slower_than_plain_within_spread":
                  bool(compact["frames_per_s_median"] >= plain["frames_per_s_median"] - spread)}
    line = json.dumps(result)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", nargs="?", default="device", choices=["device", "host"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080x256,3840x2160x64", help="WxHxB,...")
    ap.add_argument("--rounds", type=int, default=5, help="host: rounds per form")
    ap.add_argument("--frames", type=int, default=600, help="host: frames per round")
    ap.add_argument("--buffers", type=int, default=12, help="host: distinct pinned frames in the cycle")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_cwire.json"), help="host: where the result goes ('' = nowhere)")
    a = ap.parse_args()
    if a.leg == "host":
        run_host(1920, 1080, a.buffers, a.frames, a.rounds, a.out)
        return
    for s in a.sizes.split(","):
        W, H, B = (int(v) for v in s.split("x"))
        run(W, H, B, a.reps)


if __name__ == "__main__":
    main()

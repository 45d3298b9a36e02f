#!/usr/bin/env python3
"""Secondary benchmark: the compact wire format's encoder and decoder (include/mi355diff.h, "compact wire format") on
batches of S1 webcam frames resident in HBM: 1080p with B = 256 and 4K with B = 64.

Prints one JSON line per size: microseconds per frame of diff_stream_batch alone, of the encoder alone, of the two
back to back, of diff_stream_cwire_batch (`direct`: the same records in one call, without the xs / diff arrays) and of
the decoder; compact and reference-wire bytes per frame; and the encoder's achieved GB/s on its
algorithmic bytes (per frame: read 4P + 5P, write 8 + 2 pad4(P) + 4e, P = changed bytes).
The GPU client: apply_cwire_batch (records straight onto a client core's state, one call) with the shown frames written
out (`frames`) and state only (`state`), next to decode + apply_batch in the same two modes, measured in the same run;
for the `frames` mode also the achieved write rate on N bytes per frame.  Not the headline metric (bench.py)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudavideostream_amd import CUDACore, cwire_bytes_max, synth  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080x256,3840x2160x64", help="WxHxB,...")
    a = ap.parse_args()
    for s in a.sizes.split(","):
        W, H, B = (int(v) for v in s.split("x"))
        run(W, H, B, a.reps)


if __name__ == "__main__":
    main()

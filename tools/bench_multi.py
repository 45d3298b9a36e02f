#!/usr/bin/env python3
"""Secondary benchmark: one frame of each of S camera streams per tick (mi355_diff_multi_*, include/mi355diff.h), 1080p,
S = 8, 64, 256, S1 webcam-like input resident in HBM.  Not the headline metric (bench.py).

Three legs, each in microseconds per frame (wall clock around `ticks` ticks on the cores' own streams, then a
synchronisation -- what a server sees), alternating within every round; the line carries median, minimum and maximum of
the rounds:
  multi       the arrays call and the compact call: one call per tick, the S states in the caller's memory;
  cores_loop  S cores, each diff_stream_batch(nframes = 1) per tick -- the only way before these entry points;
  pairs       mi355_diff_pairs_batch on the same operands: the same kernel without the write-back, a floor for the pack.
`cores_loop` and `pairs` use old entry points only: against a library without the new symbols (MI355DIFF_LIB names
another build) the script runs them alone, which is how their numbers on the parent commit are taken.

What `pairs` is and is not: it diffs frames 1 .. S against a constant copy of the initial states every tick (nothing is
fed back, so walking the frames would let the differences grow), i.e. one webcam step per stream like every tick of
`multi`, but the SAME 2 S N bytes each time.  At S = 8 those 100 MB stay in the 256 MB last-level cache, while `multi`
walks through (S + K) N bytes of frames: there `multi_over_pairs` compares a streaming run with a cache-resident floor.
At S = 64 and 256 neither fits and the ratio is the write-back's cost.
Where the time goes (a run of its own; tracing slows the host, so no timing is taken from it):
  rocprofv3 --kernel-trace --stats --output-format csv -d trace -- python tools/bench_multi.py --legs multi,pairs --streams 64 --rounds 1
and compare k_diff_pack<true, true, false, true, true> (multi) with k_diff_pack<true, true, false, true, false> (pairs) in
*_kernel_stats.csv; counters (--pmc) go in yet another run.

The client leg (--legs client, a run of its own: `--legs client --streams 4,16,64` is how profiles/multi_client.json was
taken) measures the receiving end of such ticks, in microseconds per stream and tick, ONE JSON line for all S:
  multi_client   mi355_apply_multi_cwire_batch: one call per tick onto the S states in the caller's memory;
  cores_client   S client cores, each apply_cwire_batch(nframes = 1) on its own record -- the only way before;
  decode_arrays  cwire_decode_batch + mi355_apply_multi_batch: two calls per tick through the (offsets, xs, diff) arrays;
and the bytes of the states the compact form moves per stream and tick: touched 4096-byte tiles x 2 x 4096, counted from
the decoded indices.  The records are K ticks of a server core (diff_multi_cwire_batch on the same input), applied round
and round: adding a record to a state is the same work whatever the state holds.

The burst leg (--legs burst, a run of its own: `--legs burst --streams 4,16 --frames 4,16,64` is how
profiles/multi_stream.json was taken) measures T frames of each of S streams, in microseconds per frame, ONE JSON line for
all (S, T), the three ways a sender can make the S * T compact records:
  burst_cwire    mi355_diff_multi_stream_cwire_batch: one call, the S states in the caller's memory;
  multi_ticks    T calls of mi355_diff_multi_cwire_batch on the same frames arranged tick-major ([T][S][N]), on the same states;
  cores_stream   S cores, each mi355_diff_stream_cwire_batch(T) on its own state (a workspace sized for T per camera).
Its input is ONE webcam stream of S * T + 1 frames cut into S pieces: stream s starts from frame s * T as its state and
takes the T frames behind it.  A timed window runs the pieces forwards, then backwards (frames T - 1 .. 0 of each piece),
and so on, so that every step of every window is the step between two neighbouring webcam frames.  A core takes
max_batch * N < 2^32 bytes per call (682 frames of 1080p): where S * T is more, burst_cwire makes the fewest calls that fit,
each with as many whole streams as it can hold (`calls_per_burst` in the line).

The burst-client leg (--legs burst_client, a run of its own: `--legs burst_client --streams 4,16 --frames 4,16,64` is how
profiles/multi_stream_client.json was taken) measures the receiving end of such bursts, in microseconds per record, ONE JSON
line for all (S, T) and both inputs, the ways a receiver can apply the S * T compact records of a burst:
  burst_apply         mi355_apply_multi_stream_cwire_batch without output frames: one call, straight from the stream-major records;
  burst_apply_frames  the same with every frame in between written out;
  multi_ticks         T calls of mi355_apply_multi_cwire_batch on records re-staged tick-major BEFOREHAND (the staging is not
                      timed, which flatters this baseline);
  cores_client        S client cores, each mi355_apply_cwire_batch(T) on its camera's slice.
Inputs: `webcam`, the burst leg's (every tile of every state is touched every tick), and `local`, a static background with
the moving block of tools/roundtrip's make_frame without the noise (few tiles are touched).  The records are one burst of a
server core, applied round and round: adding a record to a state is the same work whatever the state holds.  The line also
carries the touched 4096-byte tiles per record and per stream and call, counted from the decoded indices.

The budget leg (--legs budget, a run of its own: `--legs budget --streams 4,16,64 > profiles/multi_budget.json`) measures the
sender's rate control, in microseconds per stream, ONE JSON line for all S:
  budget       mi355_cwire_budget_cwire_batch on the records of one tick, every stream's budget at half of its count;
  second_diff  a second mi355_diff_multi_cwire_batch over the same S frames from the states before the tick: the cheapest
               re-diff a caller has without the call -- and it still lacks the threshold choice.
Every pass of a timed window works on its own copy of the S states (restored outside the window).

The crop leg (--legs crop, a run of its own: `--legs crop --streams 4,16,64 > profiles/multi_crop.json`) measures the crop call on
the records of one tick (T = 1), in microseconds per stream, ONE JSON line for all S, on the webcam-like and the local input:
  coalesce       mi355_cwire_coalesce_cwire_batch on the same records: the nearest route a relay has without the crop call;
  crop_quarter   mi355_cwire_crop_cwire_batch with the rectangle (W/4, H/4, W/2, H/2) for every stream;
  crop_full      the same call with the full frame: the coalescer's work plus the rectangle table's launch.
The expectations to test: `crop_quarter` no slower than `coalesce` by more than the rounds' spread
(`quarter_no_slower_than_coalesce`), and `crop_full` within the spread plus the one table launch (`full_minus_coalesce_us_per_call`).

The split leg (--legs split, a run of its own: `--legs split --streams 4,16,64 > profiles/multi_split.json`) measures the call that
cuts records into datagram-sized pieces on the records of one tick (T = 1), in microseconds per input record, ONE JSON line for all
S, on the webcam-like and the local input:
  coalesce       mi355_cwire_coalesce_cwire_batch with T = 1 on the same records (it gives them back): the family's nearest call;
  split_1400     mi355_cwire_split_cwire_batch at max_bytes = 1400 (a UDP datagram inside an Ethernet frame);
  split_8972     the same at max_bytes = 8972 (a jumbo frame).
The expectation to test: either no slower than `coalesce` by more than the rounds' spread (`split_M_no_slower_than_coalesce`).

The fec leg (--legs fec, a run of its own: `--legs fec --streams 4,16,64 > profiles/multi_fec.json`) measures the parity call behind
the split call on the split leg's inputs (max_bytes = 1400, groups of 8), us per input record, and the repair call, us per job:
  split          mi355_cwire_split_cwire_batch at max_bytes = 1400 on the records of one tick;
  fec_k1, fec_k2 mi355_cwire_fec_batch with one and two parity blocks per group on the pieces it left;
  repair_one, repair_two  mi355_cwire_fec_repair_batch, one job per stream, one and two lost pieces (reported, not judged).
The expectation to test: fec_k2 no slower than `split` by more than the rounds' spread (`fec_k2_no_slower_than_split`).

The mosaic leg (--legs mosaic, a run of its own: `--legs mosaic --streams 4,16 > profiles/multi_mosaic.json`) measures the call that
places S cameras side by side on one canvas (a C x C grid of whole frames, C = ceil(sqrt(S)): 2x2 into 3840x2160 and 4x4 into
7680x4320 at 1080p), in microseconds per input record, ONE JSON line: T = 1 and T = 16, on the webcam-like and the local input:
  mosaic         mi355_cwire_mosaic_cwire_batch on the S*T records: ONE canvas record, no state;
  state_route    the route a caller has without the call: mi355_apply_multi_stream_cwire_batch onto relay-held states,
                 mi355_wall_compose_batch at k = 1 into a canvas, then (behind a synchronize: another core)
                 mi355_diff_stream_cwire_batch(nframes = 1) on a threshold-0 core of the canvas' geometry.
The expectation to test: `mosaic` no slower than `state_route` by more than the rounds' spread (`mosaic_no_slower_than_route`).

The activity leg (--legs activity, a run of its own: `--legs activity --streams 4,16,64 > profiles/multi_activity.json`) measures
the motion grids, in microseconds per record, ONE JSON line: S = 4, 16, 64 (--streams) with T = 1 and S = 16 with T = 16, on both
inputs of the burst-client leg:
  activity     mi355_cwire_activity_batch, 16x16 cells, the grids cleared by every call;
  burst_apply  mi355_apply_multi_stream_cwire_batch without output frames on the same records: the same directory kernels and
               the same entry walk, plus the state tiles it moves.
The expectation to test: `activity` no slower than `burst_apply` at any point by more than the rounds' spread (`verdict`).

The check leg (--legs check, a run of its own: `--legs check --streams 4,16,64 > profiles/multi_check.json`) measures the record
check, in microseconds per record, ONE JSON line, at the points and on the inputs of the activity leg:
  check        mi355_cwire_check_batch: a verdict per record, no state;
  burst_apply  mi355_apply_multi_stream_cwire_batch without output frames on the same records.
The expectation to test: `check` no slower than `burst_apply` at any point by more than the rounds' spread (`verdict`): the check
reads the records about twice and moves no state tile.

The refresh leg (--legs refresh, a run of its own: `--legs refresh --streams 4,16,64 > profiles/multi_refresh.json`) measures the
calls that resynchronise a receiver, in microseconds per stream, ONE JSON line for all S, on webcam-like states:
  digest        mi355_state_digest_batch: two words per 4096-byte tile of every state;
  digest_skewed the same on a copy of the states one byte behind an aligned address, stride N: every tile takes the unaligned
                tile load (reported, not judged);
  refresh_1pct, refresh_10pct, refresh_all
                mi355_refresh_cwire_batch with the peer's digests differing in 1 % and in 10 % of the tiles (one byte changed
                in each, evenly spread) and with no peer digests (every tile: a key frame);
  clear_10pct   mi355_state_clear_tiles_batch with the 10 % mask;
  diff          mi355_diff_multi_cwire_batch on the same streams: the call the sender pays every tick anyway; it reads 2N per
                stream where the digest reads N.
The expectation to test: `digest` no slower than `diff` at any S by more than the rounds' spread (`verdict`).  The other figures
are reported, not judged.

The wall leg (--legs wall, a run of its own: `--legs wall --streams 4,16,64 > profiles/multi_wall.json`) measures the calls of a
wall that shows its cameras, in microseconds per stream, ONE JSON line for all S, at the scales k = 2, 4 and 8, the wall a grid
of ceil(sqrt(S)) columns:
  digest             mi355_state_digest_batch on the same 16-byte aligned states: like the full compose it reads N per stream once;
  full_k2, full_k4, full_k8
                     mi355_wall_compose_batch without a mask: every thumbnail from the states;
  full_skewed_k4     the same on a copy of the states one byte behind an aligned address, stride N: every row takes the byte
                     loads (reported, not judged);
  masked_webcam_k*, masked_local_k*
                     mi355_cwire_touched_tiles_batch plus the masked compose on the records of ONE tick: a webcam-like tick
                     (noise everywhere: nearly every tile is touched) and a block moving over a still background.
The expectations to test: `masked_local` cheaper than `full` at every k and S by more than the rounds' spread, and `full_k8` no
slower than `digest` by more than the spread (`verdict`).  The other figures are reported, not judged.

The thumb leg (--legs thumb, a run of its own: `--legs thumb --streams 4,16,64 > profiles/multi_thumb.json`) measures the call that
serves a low-resolution viewer, mi355_thumb_cwire_batch at threshold 0, in microseconds per stream, ONE JSON line for all S, at the
scales k = 2, 4 and 8, on ONE tick of the webcam-like and of the local (moving block) input.  Every pass alternates between the
states before and after that tick, so the held thumbnails are always one tick behind:
  touched_plus_call_*  mi355_cwire_touched_tiles_batch of the tick's records plus the call with that mask;
  call_*               the call alone, the mask given;
  call_nullmask_*      the call without a mask;
  route_*              what a caller had before: touched tiles, the masked mi355_wall_compose_batch into a scratch wall, a
                       synchronize (another core), mi355_diff_multi_cwire_batch on a threshold-0 core of the thumbnail's geometry.
                       Its records, frame positions and states are asserted equal to the call's at every point before anything
                       is timed.
The expectations to test: `touched_plus_call` no slower than `route` at any point by more than the rounds' spread, and `call_local`
cheaper than `call_nullmask_local` (`verdict`).

Input of the other legs: ONE webcam stream of S + K + 1 frames; stream s shows frame s + j at step j, so every tick of every stream is the
step between two consecutive webcam frames, and a tick's S frames are one contiguous region.  j walks 1 .. K and back."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudavideostream_amd import lib, synth  # noqa: E402

MULTI = ("mi355_diff_multi_batch", "mi355_diff_multi_wire_batch", "mi355_diff_multi_cwire_batch")


def load_library():
    """True if the library has the many-streams entry points; a build without them is bound without them."""
    probe = ctypes.CDLL(lib.LIB_PATH)
    have = all(hasattr(probe, n) for n in MULTI)
    if not have:
        for n in MULTI:
            lib.SYMBOLS.pop(n, None)
    lib.load()
    return have


def walk(K, ticks):
    """Steps 1, 2, .. K, K - 1, .. 2, 1, 2, ..: consecutive ticks are consecutive frames, for ever."""
    j, d, out = 1, 1, []
    for _ in range(ticks):
        out.append(j)
        if K > 1:
            if j + d > K or j + d < 1:
                d = -d
            j += d
    return out


def stats(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}


def run(W, H, S, K, rounds, legs, have_multi):
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    ticks = max(16, min(2048, 16384 // S))             # ~16 k frames per timed window: tens of milliseconds
    steps = walk(K, ticks)
    _, frames = synth.webcam_stream(S + K + 1, W, H, device=dev)
    frames = frames.reshape(S + K + 1, n)
    states0 = frames[:S].clone()
    states = states0.clone()
    cap = S * n // 8                                   # S1 changes ~2 % of the bytes
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_xs = torch.empty(cap, dtype=torch.int32, device=dev)
    d_df = torch.empty(cap, dtype=torch.uint8, device=dev)
    cwcap = cwire_bytes_max(n, S)
    d_pos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    result = {"size": f"{W}x{H}", "streams": S, "ticks": ticks, "rounds": rounds, "has_multi": have_multi}
    times = {}
    core = CUDACore(W, H, max_batch=S)
    core.prepare(lib.PREPARE_BATCHES)
    cores, outs = [], []
    if "cores_loop" in legs:
        one = n // 8
        for s in range(S):
            c = CUDACore(W, H, max_batch=1)
            c.prepare(lib.PREPARE_BATCHES)
            cores.append(c)
            outs.append((torch.zeros(2, dtype=torch.int32, device=dev), torch.empty(one, dtype=torch.int32, device=dev),
                         torch.empty(one, dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()

    host0 = states0.cpu().numpy() if cores else None

    def reset(name):
        states.copy_(states0)
        if name == "cores_loop":
            for s, c in enumerate(cores):
                c.set_state(host0[s])
        torch.cuda.synchronize()

    def leg_multi():
        for j in steps:
            core.diff_multi_batch(frames[j:j + S], states, S, d_off, d_xs, d_df, cap)
        core.synchronize()

    def leg_multi_cwire():
        for j in steps:
            core.diff_multi_cwire_batch(frames[j:j + S], states, S, d_off, d_pos, d_cw, cwcap)
        core.synchronize()

    def leg_pairs():
        for _ in steps:
            core.diff_pairs_batch(frames[1:1 + S], states0, S, d_off, d_xs, d_df, cap)
        core.synchronize()

    def leg_cores():
        one = n // 8
        for j in steps:
            for s, c in enumerate(cores):
                c.diff_stream_batch(frames[j + s], 1, outs[s][0], outs[s][1], outs[s][2], one)
        for c in cores:
            c.synchronize()

    table = {"multi": leg_multi, "multi_cwire": leg_multi_cwire, "pairs": leg_pairs, "cores_loop": leg_cores}
    active = [k for k in table if ("multi" if k.startswith("multi") else k) in legs and (have_multi or not k.startswith("multi"))]
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name in active:
            reset(name)
            t0 = time.perf_counter()
            table[name]()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (ticks * S))
    if "multi" in active:
        reset("multi")
        core.diff_multi_batch(frames[1:1 + S], states, S, d_off, d_xs, d_df, cap)
        core.synchronize()
        total = int(d_off.cpu()[-1])
        assert 0 < total <= cap
        result["changed_bytes_per_frame"] = round(total / S, 1)
    for name in active:
        result[name + "_us_per_frame"] = stats(times[name])
    if "multi" in times and "cores_loop" in times:
        result["cores_loop_over_multi"] = round(statistics.median(times["cores_loop"]) / statistics.median(times["multi"]), 2)
    if "multi" in times and "pairs" in times:
        result["multi_over_pairs"] = round(statistics.median(times["multi"]) / statistics.median(times["pairs"]), 3)
    if "write_probe" in legs:                          # the board's streaming-write rate (wide stores), for the write-back's bound
        result["hbm_write_gbps"] = round(core.probe_hbm_write(1024, narrow=False), 1)
    print(json.dumps(result), flush=True)
    for c in cores:
        c.close()
    core.close()


def run_client(W, H, S, K, rounds):
    """The client leg for one S -> its dictionary."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    ticks = max(16, min(512, 4096 // S))
    _, frames = synth.webcam_stream(S + K + 1, W, H, device=dev)
    frames = frames.reshape(S + K + 1, n)
    states0 = frames[:S].clone()
    states = states0.clone()
    cwcap = cwire_bytes_max(n, S)
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    recs = []                                          # per recorded tick: (records, counts, escapes, positions)
    with CUDACore(W, H, max_batch=S) as server:
        for j in range(1, K + 1):
            server.diff_multi_cwire_batch(frames[j:j + S], states, S, d_off, d_pos, d_cw, cwcap)
            server.synchronize()
            pos = d_pos.cpu().numpy().astype(np.int64)
            counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
            pad = (counts.astype(np.int64) + 3) & ~3
            escapes = ((np.diff(pos) - 8 - 2 * pad) // 4).astype(np.uint32)
            recs.append((d_cw[:int(pos[S])].clone(), counts, escapes, pos))
    cap = max(int(r[1].sum()) for r in recs) + 16
    d_xs = torch.empty(cap, dtype=torch.int32, device=dev)
    d_df = torch.empty(cap, dtype=torch.uint8, device=dev)
    client = CUDACore(W, H, max_batch=S)
    cores = [CUDACore(W, H, max_batch=1) for _ in range(S)]
    own = [[r[0][int(r[3][s]):int(r[3][s + 1])] for s in range(S)] for r in recs]   # camera s's record of tick k
    hdr = [[(r[1][s:s + 1], r[2][s:s + 1]) for s in range(S)] for r in recs]
    host0 = states0.cpu().numpy()
    # touched tiles, from the decoded indices
    touched = []
    for r in recs:
        client.cwire_decode_batch(r[0], r[1], r[2], S, d_off, d_xs, d_df, cap)
        client.synchronize()
        tot = int(r[1].sum())
        seg = torch.repeat_interleave(torch.arange(S, device=dev), torch.from_numpy(r[1].astype(np.int64)).to(dev))
        key = seg * ((n + 4095) // 4096) + d_xs[:tot].to(torch.int64) // 4096
        touched.append(int(torch.unique(key).numel()))
    torch.cuda.synchronize()

    def leg_multi_client():
        for t in range(ticks):
            r = recs[t % K]
            client.apply_multi_cwire_batch(r[0], r[1], r[2], S, states)
        client.synchronize()

    def leg_cores_client():
        for t in range(ticks):
            k = t % K
            for s, c in enumerate(cores):
                c.apply_cwire_batch(own[k][s], hdr[k][s][0], hdr[k][s][1], 1)
        for c in cores:
            c.synchronize()

    def leg_decode_arrays():
        for t in range(ticks):
            r = recs[t % K]
            client.cwire_decode_batch(r[0], r[1], r[2], S, d_off, d_xs, d_df, cap)
            client.apply_multi_batch(d_off, d_xs, d_df, S, states)
        client.synchronize()

    table = {"multi_client": leg_multi_client, "cores_client": leg_cores_client, "decode_arrays": leg_decode_arrays}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            states.copy_(states0)
            if name == "cores_client":
                for s, c in enumerate(cores):
                    c.set_state(host0[s])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (ticks * S))
    out = {"streams": S, "ticks": ticks, "changed_bytes_per_stream": round(sum(int(r[1].sum()) for r in recs) / (K * S), 1),
           "record_bytes_per_stream": round(sum(int(r[3][S]) for r in recs) / (K * S), 1),
           "touched_tiles_per_stream": round(sum(touched) / (K * S), 1), "tiles_per_state": (n + 4095) // 4096,
           "state_bytes_moved_per_stream": round(sum(touched) * 2 * 4096 / (K * S), 1), "state_bytes_2N": 2 * n}
    for name in table:
        out[name + "_us_per_stream"] = stats(times[name])
    med = {k: statistics.median(v) for k, v in times.items()}
    out["cores_client_over_multi_client"] = round(med["cores_client"] / med["multi_client"], 2)
    out["decode_arrays_over_multi_client"] = round(med["decode_arrays"] / med["multi_client"], 2)
    for c in cores:
        c.close()
    client.close()
    return out


def run_burst(W, H, S, T, rounds):
    """The burst leg for one (S, T) -> its dictionary."""
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    passes = 2 * max(1, 1024 // B)                     # forwards and backwards in turn: ~2 k frames per timed window
    _, web = synth.webcam_stream(B + 1, W, H, device=dev)
    web = web.reshape(B + 1, n)
    states0 = web[0:B:T].clone()                                        # [S][n]: frame s * T
    fwd = web[1:].reshape(S, T, n)                                      # stream-major, a view
    bwd = web[:B].reshape(S, T, n).flip(1).contiguous()                 # frames T - 1 .. 0 of each piece
    sets = [(fwd, fwd.transpose(0, 1).contiguous()), (bwd, bwd.transpose(0, 1).contiguous())]   # (stream-major, tick-major)
    states = states0.clone()
    cwcap = min(cwire_bytes_max(n, B), max(B * n // 4, 1 << 16))        # the input changes ~2 % of the bytes
    d_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    per_call = min(S, max(1, ((1 << 32) - 1) // n // T))             # whole streams per call: max_batch * N < 2^32
    chunks = [(s0, min(per_call, S - s0)) for s0 in range(0, S, per_call)]
    burst = CUDACore(W, H, max_batch=per_call * T)
    ticks = CUDACore(W, H, max_batch=S)
    cores = [CUDACore(W, H, max_batch=T) for _ in range(S)]
    one = cwcap // S
    outs = [(torch.zeros(T + 1, dtype=torch.int32, device=dev), torch.zeros(T + 1, dtype=torch.int64, device=dev),
             torch.empty(one, dtype=torch.uint8, device=dev)) for _ in range(S)]
    for c in [burst, ticks] + cores:
        c.prepare(lib.PREPARE_BATCHES)
    host0 = states0.cpu().numpy()
    torch.cuda.synchronize()

    def leg_burst():
        for p in range(passes):
            for s0, ns in chunks:
                burst.diff_multi_stream_cwire_batch(sets[p & 1][0][s0], states[s0], ns, T, d_off, d_pos, d_cw, cwcap)
        burst.synchronize()

    def leg_ticks():
        for p in range(passes):
            tm = sets[p & 1][1]
            for t in range(T):
                ticks.diff_multi_cwire_batch(tm[t], states, S, d_off, d_pos, d_cw, cwcap)
        ticks.synchronize()

    def leg_cores():
        for p in range(passes):
            sm = sets[p & 1][0]
            for s, c in enumerate(cores):
                c.diff_stream_cwire_batch(sm[s], T, outs[s][0], outs[s][1], outs[s][2], one)
        for c in cores:
            c.synchronize()

    table = {"burst_cwire": leg_burst, "multi_ticks": leg_ticks, "cores_stream": leg_cores}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            states.copy_(states0)
            if name == "cores_stream":
                for s, c in enumerate(cores):
                    c.set_state(host0[s])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * B))
    states.copy_(states0)
    torch.cuda.synchronize()
    total = nbytes = 0
    for s0, ns in chunks:
        burst.diff_multi_stream_cwire_batch(fwd[s0], states[s0], ns, T, d_off, d_pos, d_cw, cwcap)
        burst.synchronize()
        total, nbytes = total + int(d_off.cpu()[ns * T]), nbytes + int(d_pos.cpu()[ns * T])
        assert int(d_pos.cpu()[ns * T]) <= cwcap                                               # nothing was dropped
    assert 0 < total and all(int(o[1].cpu()[-1]) <= one for o in outs)
    out = {"streams": S, "frames": T, "passes": passes, "calls_per_burst": len(chunks), "changed_bytes_per_frame": round(total / B, 1),
           "record_bytes_per_frame": round(nbytes / B, 1)}
    for name in table:
        out[name + "_us_per_frame"] = stats(times[name])
    med = {k: statistics.median(v) for k, v in times.items()}
    out["multi_ticks_over_burst"] = round(med["multi_ticks"] / med["burst_cwire"], 3)
    out["cores_stream_over_burst"] = round(med["cores_stream"] / med["burst_cwire"], 3)
    for c in [burst, ticks] + cores:
        c.close()
    return out


def local_streams(S, T, W, H, dev):
    """The local input: a static background with a block that moves 3 pixels per frame, as tools/roundtrip's make_frame
    draws it, without the noise -> (states0 [S][n], frames [S][T][n])."""
    n = 3 * W * H
    i = torch.arange(n, device=dev, dtype=torch.int64)
    bw, bh, y0 = W // 4 + 1, H // 4 + 1, H // 3
    colour = torch.tensor([200, 210, 220], dtype=torch.uint8, device=dev)
    frames = torch.empty(S, T + 1, n, dtype=torch.uint8, device=dev)
    for s in range(S):
        base = (40 + (i * 7 + s * 31) % 150).to(torch.uint8)
        for t in range(T + 1):
            f = frames[s, t]
            f.copy_(base)
            x0 = ((t + 5 * s) * 3) % (W - bw + 1)
            f.view(H, W, 3)[y0:y0 + bh, x0:x0 + bw] = colour
    return frames[:, 0].contiguous(), frames[:, 1:].contiguous()


def run_burst_client(W, H, S, T, rounds, kind):
    """The burst-client leg for one (S, T) and one input -> its dictionary."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    ntiles = (n + 4095) // 4096
    passes = 2 * max(1, 1024 // B)                     # ~2 k records per timed window
    if kind == "webcam":                                # run_burst's input: one stream cut into S pieces
        _, web = synth.webcam_stream(B + 1, W, H, device=dev)
        web = web.reshape(B + 1, n)
        states0, fwd = web[0:B:T].clone(), web[1:].reshape(S, T, n)
    else:
        states0, fwd = local_streams(S, T, W, H, dev)
    per_call = min(S, max(1, ((1 << 32) - 1) // n // T))             # whole streams per call: max_batch * N < 2^32
    chunks = [(s0, min(per_call, S - s0)) for s0 in range(0, S, per_call)]
    # ---- the records, as a sender's mi355_diff_multi_stream_cwire_batch makes them: per chunk (records, counts, escapes, positions)
    recs = []
    srv_states = states0.clone()
    with CUDACore(W, H, max_batch=per_call * T) as server:
        for s0, ns in chunks:
            nb = ns * T
            cwcap = cwire_bytes_max(n, nb)
            d_off = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
            d_pos = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
            d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            server.diff_multi_stream_cwire_batch(fwd[s0], srv_states[s0], ns, T, d_off, d_pos, d_cw, cwcap)
            server.synchronize()
            pos = d_pos.cpu().numpy().astype(np.int64)
            counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
            pad = (counts.astype(np.int64) + 3) & ~3
            escapes = ((np.diff(pos) - 8 - 2 * pad) // 4).astype(np.uint32)
            recs.append((d_cw[:int(pos[nb])].clone(), counts, escapes, pos))
            del d_cw
    # re-staged tick-major for baseline (3): tick t = record (s, t) of every s back to back
    flat = [(recs[c][0], recs[c][3], j * T, recs[c][1], recs[c][2]) for c, (s0, ns) in enumerate(chunks) for j in range(ns)]
    staged = []
    for t in range(T):
        parts = [r[int(p[b0 + t]):int(p[b0 + t + 1])] for r, p, b0, _, _ in flat]
        staged.append((torch.cat(parts), np.array([c[b0 + t] for _, _, b0, c, _ in flat], np.uint32),
                       np.array([e[b0 + t] for _, _, b0, _, e in flat], np.uint32)))
    # camera s's slice for baseline (4)
    own = [(r[int(p[b0]):int(p[b0 + T])], c[b0:b0 + T], e[b0:b0 + T]) for r, p, b0, c, e in flat]
    states = states0.clone()
    d_out = torch.empty(B, n, dtype=torch.uint8, device=dev)
    client = CUDACore(W, H, max_batch=per_call * T)
    ticks = CUDACore(W, H, max_batch=S)
    cores = [CUDACore(W, H, max_batch=T) for _ in range(S)]
    host0 = states0.cpu().numpy()
    # touched tiles, from the decoded indices: per record, and per stream and call (what the new call loads and stores)
    entries = sum(int(r[1].sum()) for r in recs)
    tiles_rec = tiles_call = 0
    for (s0, ns), r in zip(chunks, recs):
        tot, nb = int(r[1].sum()), ns * T
        d_off = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
        d_xs = torch.empty(tot + 16, dtype=torch.int32, device=dev)
        d_df = torch.empty(tot + 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        client.cwire_decode_batch(r[0], r[1], r[2], nb, d_off, d_xs, d_df, tot + 16)
        client.synchronize()
        b = torch.repeat_interleave(torch.arange(nb, device=dev), torch.from_numpy(r[1].astype(np.int64)).to(dev))
        tile = d_xs[:tot].to(torch.int64) // 4096
        tiles_rec += int(torch.unique(b * ntiles + tile).numel())
        tiles_call += int(torch.unique((b // T) * ntiles + tile).numel())
        del d_xs, d_df, b, tile
    torch.cuda.synchronize()

    def leg_burst(out):
        for _ in range(passes):
            for (s0, ns), r in zip(chunks, recs):
                client.apply_multi_stream_cwire_batch(r[0], r[1], r[2], ns, T, states[s0], d_frames_out=out[s0 * T] if out is not None else None)
        client.synchronize()

    def leg_ticks():
        for _ in range(passes):
            for r, c, e in staged:
                ticks.apply_multi_cwire_batch(r, c, e, S, states)
        ticks.synchronize()

    def leg_cores():
        for _ in range(passes):
            for s, c in enumerate(cores):
                c.apply_cwire_batch(own[s][0], own[s][1], own[s][2], T)
        for c in cores:
            c.synchronize()

    table = {"burst_apply": lambda: leg_burst(None), "burst_apply_frames": lambda: leg_burst(d_out), "multi_ticks": leg_ticks,
             "cores_client": leg_cores}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            states.copy_(states0)
            if name == "cores_client":
                for s, c in enumerate(cores):
                    c.set_state(host0[s])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * B))
    # one burst from the base states is what the sender's states became, by every way
    states.copy_(states0)
    torch.cuda.synchronize()
    for (s0, ns), r in zip(chunks, recs):
        client.apply_multi_stream_cwire_batch(r[0], r[1], r[2], ns, T, states[s0], d_frames_out=d_out[s0 * T])
    client.synchronize()
    assert torch.equal(states, srv_states) and torch.equal(d_out[T - 1::T], srv_states)
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "calls_per_burst": len(chunks),
           "changed_bytes_per_record": round(entries / B, 1), "record_bytes_per_record": round(sum(int(r[3][-1]) for r in recs) / B, 1),
           "tiles_per_state": ntiles, "touched_tiles_per_record": round(tiles_rec / B, 1),
           "touched_tiles_per_stream_and_call": round(tiles_call / S, 1)}
    for name in table:
        out[name + "_us_per_record"] = stats(times[name])
    med = {k: statistics.median(v) for k, v in times.items()}
    out["multi_ticks_over_burst_apply"] = round(med["multi_ticks"] / med["burst_apply"], 3)
    out["cores_client_over_burst_apply"] = round(med["cores_client"] / med["burst_apply"], 3)
    for c in [client, ticks] + cores:
        c.close()
    return out


def run_activity(W, H, S, T, rounds, kind, cell=16):
    """The activity leg for one (S, T) and one input -> its dictionary."""
    import numpy as np
    from cudavideostream_amd import CUDACore, activity_cells, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    passes = 2 * max(1, 1024 // B)                     # ~2 k records per timed window
    if kind == "webcam":                                # run_burst's input: one stream cut into S pieces
        _, web = synth.webcam_stream(B + 1, W, H, device=dev)
        web = web.reshape(B + 1, n)
        states0, fwd = web[0:B:T].clone(), web[1:].reshape(S, T, n)
    else:
        states0, fwd = local_streams(S, T, W, H, dev)
    # ---- the records, as a sender's mi355_diff_multi_stream_cwire_batch makes them
    cwcap = cwire_bytes_max(n, B)
    d_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    srv_states = states0.clone()
    with CUDACore(W, H, max_batch=B) as server:
        torch.cuda.synchronize()
        server.diff_multi_stream_cwire_batch(fwd, srv_states, S, T, d_off, d_pos, d_cw, cwcap)
        server.synchronize()
    pos = d_pos.cpu().numpy().astype(np.int64)
    off = d_off.cpu().numpy().view(np.uint32).astype(np.int64)
    counts = np.diff(off).astype(np.uint32)
    escapes = ((np.diff(pos) - 8 - 2 * ((counts.astype(np.int64) + 3) & ~3)) // 4).astype(np.uint32)
    recs = d_cw[:int(pos[B])].clone()
    del d_cw, fwd
    ncells = activity_cells(W, H, cell, cell)[0]
    d_cells = torch.empty(S * ncells, dtype=torch.int32, device=dev)
    d_sum = torch.empty(S * 8, dtype=torch.int32, device=dev)
    states = states0.clone()
    core = CUDACore(W, H, max_batch=B)
    torch.cuda.synchronize()

    def leg_activity():
        for _ in range(passes):
            core.cwire_activity_batch(recs, counts, escapes, S, T, cell, cell, d_cells, d_sum)
        core.synchronize()

    def leg_apply():
        for _ in range(passes):
            core.apply_multi_stream_cwire_batch(recs, counts, escapes, S, T, states)
        core.synchronize()

    table = {"activity": leg_activity, "burst_apply": leg_apply}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms both legs up and is dropped
        for name, leg in table.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * B))
    # every counted entry is in the grids, and every stream's count is its records'
    summ = d_sum.cpu().numpy().view(np.uint32).reshape(S, 8)
    per_stream = counts.astype(np.int64).reshape(S, T).sum(axis=1)
    assert (summ[:, 0] == per_stream).all()
    assert (d_cells.cpu().numpy().view(np.uint32).astype(np.int64).reshape(S, ncells).sum(axis=1) == per_stream).all()
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "cell": cell, "cells_per_stream": ncells,
           "changed_bytes_per_record": round(int(counts.sum()) / B, 1), "active_cells_per_stream": round(float(summ[:, 5].mean()), 1)}
    for name in table:
        out[name + "_us_per_record"] = stats(times[name])
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(max(v) - min(v) for v in times.values())
    out["activity_over_burst_apply"] = round(med["activity"] / med["burst_apply"], 3)
    out["no_slower_than_burst_apply"] = bool(med["activity"] <= med["burst_apply"] + spread)
    core.close()
    return out


def run_check(W, H, S, T, rounds, kind):
    """The check leg for one (S, T) and one input -> its dictionary."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, cwire_check_host
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    passes = 2 * max(1, 1024 // B)                     # ~2 k records per timed window
    if kind == "webcam":                                # run_burst's input: one stream cut into S pieces
        _, web = synth.webcam_stream(B + 1, W, H, device=dev)
        web = web.reshape(B + 1, n)
        states0, fwd = web[0:B:T].clone(), web[1:].reshape(S, T, n)
    else:
        states0, fwd = local_streams(S, T, W, H, dev)
    # ---- the records, as a sender's mi355_diff_multi_stream_cwire_batch makes them
    cwcap = cwire_bytes_max(n, B)
    d_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    srv_states = states0.clone()
    with CUDACore(W, H, max_batch=B) as server:
        torch.cuda.synchronize()
        server.diff_multi_stream_cwire_batch(fwd, srv_states, S, T, d_off, d_pos, d_cw, cwcap)
        server.synchronize()
    pos = d_pos.cpu().numpy().astype(np.int64)
    off = d_off.cpu().numpy().view(np.uint32).astype(np.int64)
    counts = np.diff(off).astype(np.uint32)
    escapes = ((np.diff(pos) - 8 - 2 * ((counts.astype(np.int64) + 3) & ~3)) // 4).astype(np.uint32)
    recs = d_cw[:int(pos[B])].clone()
    del d_cw, fwd
    d_verdicts = torch.empty(B * 4, dtype=torch.int32, device=dev)
    states = states0.clone()
    core = CUDACore(W, H, max_batch=B)
    torch.cuda.synchronize()

    def leg_check():
        for _ in range(passes):
            core.cwire_check_batch(recs, counts, escapes, B, d_verdicts)
        core.synchronize()

    def leg_apply():
        for _ in range(passes):
            core.apply_multi_stream_cwire_batch(recs, counts, escapes, S, T, states)
        core.synchronize()

    table = {"check": leg_check, "burst_apply": leg_apply}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms both legs up and is dropped
        for name, leg in table.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * B))
    # a sender's records are clean, and the device's verdicts are the host's
    got = d_verdicts.cpu().numpy().view(np.uint32).reshape(B, 4)
    assert not got[:, 0].any() and (got[:, 1] == escapes).all() and (got[:, 2] == counts).all()
    assert np.array_equal(got, cwire_check_host(recs.cpu().numpy(), counts, escapes, n))
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "changed_bytes_per_record": round(int(counts.sum()) / B, 1),
           "record_bytes_per_record": round(int(pos[B]) / B, 1)}
    for name in table:
        out[name + "_us_per_record"] = stats(times[name])
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(max(v) - min(v) for v in times.values())
    out["check_over_burst_apply"] = round(med["check"] / med["burst_apply"], 3)
    out["no_slower_than_burst_apply"] = bool(med["check"] <= med["burst_apply"] + spread)
    core.close()
    return out


def run_refresh(W, H, S, rounds):
    """The refresh leg for one S -> its dictionary.  All legs on one core's own stream, alternating within every round; the diff
    leg has its own copy of the states per pass, restored outside the window (it is the only leg that writes states it reads)."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, state_tiles
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    tiles = state_tiles(n)
    mask_words = (tiles + 31) // 32
    passes = max(2, min(16, 128 // S))
    _, web = synth.webcam_stream(S + 1, W, H, device=dev)
    web = web.reshape(S + 1, n)
    sender, frames = web[:S].clone(), web[1:].clone()   # stream s: webcam frame s, and the tick s -> s + 1 for the diff leg
    cwcap = cwire_bytes_max(n, S)
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    d_mask = torch.zeros(S * mask_words, dtype=torch.int32, device=dev)
    d_dig = torch.zeros(S * tiles * 2, dtype=torch.int32, device=dev)
    core = CUDACore(W, H, max_batch=S)
    torch.cuda.synchronize()
    peers, masks, selected = {}, {}, {}
    for name, every in (("1pct", 100), ("10pct", 10)):   # the receiver: the sender's states with a byte changed in every k-th tile
        recv = sender.clone()
        hit = torch.arange(every // 2, tiles, every, device=dev) * 4096 + 1234
        hit = hit[hit < n]
        recv[:, hit] ^= 0x5A
        peers[name] = torch.zeros_like(d_dig)
        torch.cuda.synchronize()
        core.state_digest_batch(recv, S, peers[name])
        core.refresh_cwire_batch(sender, S, peers[name], d_mask, d_off, d_pos, d_cw, cwcap)
        core.synchronize()
        masks[name] = d_mask.clone()
        selected[name] = int(sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in d_mask.cpu().numpy()))
        assert selected[name] == S * int(hit.numel()), "the refresh did not select exactly the changed tiles"
        del recv
    work = torch.empty(passes, S, n, dtype=torch.uint8, device=dev)
    scratch = sender.clone()                             # the clear leg's states
    skew_buf = torch.empty(S * n + 16, dtype=torch.uint8, device=dev)
    skewed = skew_buf[1:1 + S * n]                       # 1080p: N is a multiple of 16, so every stream is one byte off
    skewed.copy_(sender.reshape(-1))
    assert skewed.data_ptr() % 16 == 1
    rec_bytes = {}

    def leg_digest():
        for _ in range(passes):
            core.state_digest_batch(sender, S, d_dig)
        core.synchronize()

    def leg_digest_skewed():
        for _ in range(passes):
            core.state_digest_batch(skewed, S, d_dig)
        core.synchronize()

    def leg_refresh(peer):
        def leg():
            for _ in range(passes):
                core.refresh_cwire_batch(sender, S, peer, d_mask, d_off, d_pos, d_cw, cwcap)
            core.synchronize()
        return leg

    def leg_clear():
        for _ in range(passes):
            core.state_clear_tiles_batch(scratch, S, masks["10pct"])
        core.synchronize()

    def leg_diff():
        for p in range(passes):
            core.diff_multi_cwire_batch(frames, work[p], S, d_off, d_pos, d_cw, cwcap)
        core.synchronize()

    table = {"digest": leg_digest, "digest_skewed": leg_digest_skewed, "refresh_1pct": leg_refresh(peers["1pct"]), "refresh_10pct": leg_refresh(peers["10pct"]),
             "refresh_all": leg_refresh(None), "clear_10pct": leg_clear, "diff": leg_diff}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            if name == "diff":
                work.copy_(sender.unsqueeze(0).expand(passes, S, n))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * S))
            if name.startswith("refresh"):
                rec_bytes[name] = int(d_pos[S].item())
    out = {"streams": S, "passes": passes, "tiles": tiles, "state_bytes": n}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + "_us_per_stream"] = st
    for name in ("1pct", "10pct"):
        out["refresh_" + name + "_tiles_per_stream"] = selected[name] // S
    for name, b in rec_bytes.items():
        out[name + "_bytes_per_stream"] = round(b / S, 1)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(max(times[k]) - min(times[k]) for k in ("digest", "diff"))
    out["digest_over_diff"] = round(med["digest"] / med["diff"], 3)
    out["digest_no_slower_than_diff"] = bool(med["digest"] <= med["diff"] + spread)
    core.close()
    return out


def run_wall(W, H, S, rounds, scales=(2, 4, 8)):
    """The wall leg for one S -> its dictionary.  All legs on one core's own stream, alternating within every round."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, state_tiles, wall_thumb_size
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    tiles = state_tiles(n)
    mask_words = (tiles + 31) // 32
    passes = max(2, min(16, 128 // S))
    cols = int(np.ceil(np.sqrt(S)))
    cwcap = cwire_bytes_max(n, S)
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    d_mask = torch.zeros(S * mask_words, dtype=torch.int32, device=dev)
    d_dig = torch.zeros(S * tiles * 2, dtype=torch.int32, device=dev)
    core = CUDACore(W, H, max_batch=S)
    # ---- one tick of every input: the states after it and its records
    ticks = {}
    for kind in ("webcam", "local"):
        if kind == "webcam":
            _, web = synth.webcam_stream(S + 1, W, H, device=dev)
            web = web.reshape(S + 1, n)
            before, frames = web[:S].clone(), web[1:].clone()
        else:
            before, fwd = local_streams(S, 1, W, H, dev)
            frames = fwd[:, 0].contiguous()
        states = before.clone()
        torch.cuda.synchronize()
        core.diff_multi_cwire_batch(frames, states, S, d_off, d_pos, d_cw, cwcap)
        core.synchronize()
        pos = d_pos.cpu().numpy().astype(np.int64)
        counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
        escapes = ((np.diff(pos) - 8 - 2 * ((counts.astype(np.int64) + 3) & ~3)) // 4).astype(np.uint32)
        core.cwire_touched_tiles_batch(d_cw, counts, escapes, S, 1, d_mask)
        core.synchronize()
        touched = int(sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in d_mask.cpu().numpy()))
        ticks[kind] = (states, d_cw[:int(pos[S])].clone(), counts, escapes, touched)
        del before, frames
    aligned = ticks["webcam"][0]
    assert aligned.data_ptr() % 16 == 0
    skew_buf = torch.empty(S * n + 16, dtype=torch.uint8, device=dev)
    skewed = skew_buf[1:1 + S * n]                       # 1080p: N is a multiple of 16, so every stream is one byte off
    skewed.copy_(aligned.reshape(-1))
    walls = {}
    for k in scales:
        _, tw, th = wall_thumb_size(W, H, k)
        place = np.array([((s % cols) * tw, (s // cols) * th, k) for s in range(S)], np.int32)
        wall_w, wall_h = cols * tw, ((S + cols - 1) // cols) * th
        walls[k] = (place, torch.zeros(wall_h * wall_w * 3, dtype=torch.uint8, device=dev), wall_w, wall_h)
    torch.cuda.synchronize()

    def leg_digest():
        for _ in range(passes):
            core.state_digest_batch(aligned, S, d_dig)
        core.synchronize()

    def leg_full(k, states):
        place, d_wall, wall_w, wall_h = walls[k]

        def leg():
            for _ in range(passes):
                core.wall_compose_batch(states, S, place, d_wall, wall_w, wall_h)
            core.synchronize()
        return leg

    def leg_masked(k, kind):
        place, d_wall, wall_w, wall_h = walls[k]
        states, recs, counts, escapes, _ = ticks[kind]

        def leg():
            for _ in range(passes):
                core.cwire_touched_tiles_batch(recs, counts, escapes, S, 1, d_mask)
                core.wall_compose_batch(states, S, place, d_wall, wall_w, wall_h, d_tile_mask=d_mask)
            core.synchronize()
        return leg

    table = {"digest": leg_digest, "full_skewed_k4": leg_full(4, skewed)}
    for k in scales:
        table[f"full_k{k}"] = leg_full(k, aligned)
        table[f"masked_webcam_k{k}"] = leg_masked(k, "webcam")
        table[f"masked_local_k{k}"] = leg_masked(k, "local")
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * S))
    out = {"streams": S, "passes": passes, "tiles": tiles, "state_bytes": n, "columns": cols,
           "touched_tiles_per_stream": {kind: round(ticks[kind][4] / S, 1) for kind in ticks}}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + "_us_per_stream"] = st
    med = {k: statistics.median(v) for k, v in times.items()}

    def spread(*names):
        return max(max(times[k]) - min(times[k]) for k in names)

    out["masked_local_over_full"] = {f"k{k}": round(med[f"masked_local_k{k}"] / med[f"full_k{k}"], 3) for k in scales}
    out["masked_local_cheaper_than_full"] = bool(all(
        med[f"masked_local_k{k}"] + spread(f"masked_local_k{k}", f"full_k{k}") < med[f"full_k{k}"] for k in scales))
    out["full_k8_over_digest"] = round(med["full_k8"] / med["digest"], 3)
    out["full_k8_no_slower_than_digest"] = bool(med["full_k8"] <= med["digest"] + spread("full_k8", "digest"))
    core.close()
    return out


def run_thumb(W, H, S, rounds, scales=(2, 4, 8)):
    """The thumb leg for one S -> its dictionary.  Every leg alternates between the states before and after ONE tick (A, B, A, ..)
    with the tick's tile mask, so every pass finds the held thumbnails one tick behind and does a tick's work; the route's
    thumbnail-core states follow in the same way.  All legs alternate within every round."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, state_tiles, wall_thumb_size
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    mask_words = (state_tiles(n) + 31) // 32
    passes = 2 * max(1, min(8, 64 // S))
    cwcap = cwire_bytes_max(n, S)
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    d_mask = torch.zeros(S * mask_words, dtype=torch.int32, device=dev)
    core = CUDACore(W, H, max_batch=S)
    ticks = {}
    for kind in ("webcam", "local"):
        if kind == "webcam":
            _, web = synth.webcam_stream(S + 1, W, H, device=dev)
            web = web.reshape(S + 1, n)
            before, frames = web[:S].clone(), web[1:].clone()
        else:
            before, fwd = local_streams(S, 1, W, H, dev)
            frames = fwd[:, 0].contiguous()
        after = before.clone()
        torch.cuda.synchronize()
        core.diff_multi_cwire_batch(frames, after, S, d_off, d_pos, d_cw, cwcap)
        core.synchronize()
        pos = d_pos.cpu().numpy().astype(np.int64)
        counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
        escapes = ((np.diff(pos) - 8 - 2 * ((counts.astype(np.int64) + 3) & ~3)) // 4).astype(np.uint32)
        d_kind_mask = torch.zeros_like(d_mask)
        core.cwire_touched_tiles_batch(d_cw, counts, escapes, S, 1, d_kind_mask)
        core.synchronize()
        touched = int(sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in d_kind_mask.cpu().numpy()))
        ticks[kind] = ((before, after), d_cw[:int(pos[S])].clone(), counts, escapes, d_kind_mask, touched)
        del frames
    geo = {}
    for k in scales:
        _, tw, th = wall_thumb_size(W, H, k)
        nt = 3 * tw * th
        cap = cwire_bytes_max(nt, S)
        geo[k] = dict(tw=tw, th=th, nt=nt, cap=cap, small=CUDACore(tw, th, threshold=0, max_batch=S),
                      place=np.array([(0, s * th, k) for s in range(S)], np.int32),
                      wall=torch.zeros(S * nt, dtype=torch.uint8, device=dev),
                      out=[(torch.zeros(S + 1, dtype=torch.int32, device=dev), torch.zeros(S + 1, dtype=torch.int64, device=dev),
                            torch.empty(cap, dtype=torch.uint8, device=dev)) for _ in range(2)])

    def thumbs_of(states, k):
        """The thumbnails of the states, by the call itself from zeroed held thumbnails (a key record)."""
        g = geo[k]
        d = torch.zeros(S * g["nt"], dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        core.thumb_cwire_batch(states, S, k, 0, d, *g["out"][0], g["cap"])
        core.synchronize()
        return d

    def call(k, states, held, mask, out):
        core.thumb_cwire_batch(states, S, k, 0, held, *out, geo[k]["cap"], d_tile_mask=mask)

    def route(k, states, held, mask, out):
        g = geo[k]
        core.wall_compose_batch(states, S, g["place"], g["wall"], g["tw"], S * g["th"], d_tile_mask=mask)
        core.synchronize()                                  # (another core, another stream)
        g["small"].diff_multi_cwire_batch(g["wall"], held, S, *out, g["cap"])

    table, checked = {}, 0
    for kind in ("webcam", "local"):
        (A, B), recs, counts, escapes, kmask, _ = ticks[kind]
        for k in scales:
            g = geo[k]
            held = {name: thumbs_of(A, k) for name in ("touched", "masked", "null", "route")}
            g["wall"].copy_(held["route"])                  # the scratch wall begins as the full composition, as a caller's would
            # ---- the records of the tick A -> B: the call's equal the route's, byte for byte (and both leave the thumbnails of B)
            torch.cuda.synchronize()
            call(k, B, held["masked"], kmask, g["out"][0])
            route(k, B, held["route"], kmask, g["out"][1])
            core.synchronize()
            g["small"].synchronize()
            (o0, p0, c0), (o1, p1, c1) = g["out"]
            end = int(p0[S].item())
            assert torch.equal(o0, o1) and torch.equal(p0, p1) and torch.equal(c0[:end], c1[:end]), (kind, k)
            assert torch.equal(held["masked"], held["route"]) and end > 8 * S, (kind, k)
            checked += 1
            for name in ("touched", "null"):                # every leg begins at B, like the two above
                call(k, B, held[name], None, g["out"][0])
            core.synchronize()

            def legs(kind=kind, k=k, held=held, recs=recs, counts=counts, escapes=escapes, kmask=kmask, pair=(A, B)):
                out = geo[k]["out"][0]

                def touched_plus_call():
                    for i in range(passes):
                        core.cwire_touched_tiles_batch(recs, counts, escapes, S, 1, d_mask)
                        call(k, pair[i % 2], held["touched"], d_mask, out)
                    core.synchronize()

                def call_masked():
                    for i in range(passes):
                        call(k, pair[i % 2], held["masked"], kmask, out)
                    core.synchronize()

                def call_null():
                    for i in range(passes):
                        call(k, pair[i % 2], held["null"], None, out)
                    core.synchronize()

                def the_route():
                    for i in range(passes):
                        core.cwire_touched_tiles_batch(recs, counts, escapes, S, 1, d_mask)
                        route(k, pair[i % 2], held["route"], d_mask, geo[k]["out"][1])
                        geo[k]["small"].synchronize()
                return {f"touched_plus_call_{kind}_k{k}": touched_plus_call, f"call_{kind}_k{k}": call_masked,
                        f"call_nullmask_{kind}_k{k}": call_null, f"route_{kind}_k{k}": the_route}
            table.update(legs())
    times = {}
    for r in range(rounds + 1):                            # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * S))
    out = {"streams": S, "passes": passes, "tiles": state_tiles(n), "state_bytes": n, "records_equal_to_the_route": checked,
           "touched_tiles_per_stream": {kind: round(ticks[kind][5] / S, 1) for kind in ticks}}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + "_us_per_stream"] = st
    med = {k: statistics.median(v) for k, v in times.items()}

    def spread(*names):
        return max(max(times[k]) - min(times[k]) for k in names)

    points = [(kind, k) for kind in ticks for k in scales]
    out["touched_plus_call_over_route"] = {f"{kind}_k{k}": round(med[f"touched_plus_call_{kind}_k{k}"] / med[f"route_{kind}_k{k}"], 3)
                                           for kind, k in points}
    out["touched_plus_call_no_slower_than_route"] = bool(all(
        med[f"touched_plus_call_{kind}_k{k}"] <= med[f"route_{kind}_k{k}"] + spread(f"touched_plus_call_{kind}_k{k}", f"route_{kind}_k{k}")
        for kind, k in points))
    out["call_local_over_nullmask"] = {f"k{k}": round(med[f"call_local_k{k}"] / med[f"call_nullmask_local_k{k}"], 3) for k in scales}
    out["call_local_cheaper_than_nullmask"] = bool(all(
        med[f"call_local_k{k}"] + spread(f"call_local_k{k}", f"call_nullmask_local_k{k}") < med[f"call_nullmask_local_k{k}"]
        for k in scales))
    for g in geo.values():
        g["small"].close()
    core.close()
    return out


def run_coalesce(W, H, S, T, rounds, kind):
    """The coalesce leg for one (S, T) and one input -> its dictionary.  coalesce: mi355_cwire_coalesce_cwire_batch on the
    burst's records, nothing else.  state_route: what a relay did before -- mi355_apply_multi_stream_cwire_batch onto states it
    holds, then mi355_diff_multi_cwire_batch of a threshold-0 core between the new states and the saved ones (which the call
    advances), both on one core, no synchronisation in between."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    passes = 2 * max(1, 1024 // B)                     # ~2 k records per timed window
    if kind == "webcam":                                # run_burst's input: one stream cut into S pieces
        _, web = synth.webcam_stream(B + 1, W, H, device=dev)
        web = web.reshape(B + 1, n)
        states0, fwd = web[0:B:T].clone(), web[1:].reshape(S, T, n)
    else:
        states0, fwd = local_streams(S, T, W, H, dev)
    per_call = min(S, max(1, ((1 << 32) - 1) // n // T))             # whole streams per call: max_batch * N < 2^32
    chunks = [(s0, min(per_call, S - s0)) for s0 in range(0, S, per_call)]
    recs = []                                           # per chunk: (records, counts, escapes, bytes)
    srv_states = states0.clone()
    with CUDACore(W, H, max_batch=per_call * T) as server:
        for s0, ns in chunks:
            nb = ns * T
            cwcap = cwire_bytes_max(n, nb)
            d_off = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
            d_pos = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
            d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            server.diff_multi_stream_cwire_batch(fwd[s0], srv_states[s0], ns, T, d_off, d_pos, d_cw, cwcap)
            server.synchronize()
            pos = d_pos.cpu().numpy().astype(np.int64)
            counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
            pad = (counts.astype(np.int64) + 3) & ~3
            escapes = ((np.diff(pos) - 8 - 2 * pad) // 4).astype(np.uint32)
            recs.append((d_cw[:int(pos[nb])].clone(), counts, escapes, int(pos[nb])))
            del d_cw
    ocap = cwire_bytes_max(n, per_call)
    d_ooff = torch.zeros(per_call + 1, dtype=torch.int32, device=dev)
    d_opos = torch.zeros(per_call + 1, dtype=torch.int64, device=dev)
    d_out = torch.empty(ocap, dtype=torch.uint8, device=dev)
    d_roff, d_rpos, d_rout = torch.zeros_like(d_ooff), torch.zeros_like(d_opos), torch.empty_like(d_out)
    states, saved = states0.clone(), states0.clone()
    relay = CUDACore(W, H, max_batch=per_call * T)
    route = CUDACore(W, H, max_batch=per_call * T, threshold=0)
    torch.cuda.synchronize()

    def leg_coalesce():
        for _ in range(passes):
            for (s0, ns), r in zip(chunks, recs):
                relay.cwire_coalesce_cwire_batch(r[0], r[1], r[2], ns, T, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()

    def leg_route():
        for _ in range(passes):
            for (s0, ns), r in zip(chunks, recs):
                route.apply_multi_stream_cwire_batch(r[0], r[1], r[2], ns, T, states[s0])
                route.diff_multi_cwire_batch(states[s0], saved[s0], ns, d_roff, d_rpos, d_rout, ocap)
        route.synchronize()

    table = {"coalesce": leg_coalesce, "state_route": leg_route}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            states.copy_(states0)
            saved.copy_(states0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * B))
    # one burst from the base states: both ways make the same records, and they lead to the sender's states
    states.copy_(states0)
    saved.copy_(states0)
    out_bytes = out_entries = 0
    torch.cuda.synchronize()
    for (s0, ns), r in zip(chunks, recs):
        relay.cwire_coalesce_cwire_batch(r[0], r[1], r[2], ns, T, d_ooff, d_opos, d_out, ocap)
        route.apply_multi_stream_cwire_batch(r[0], r[1], r[2], ns, T, states[s0])
        route.diff_multi_cwire_batch(states[s0], saved[s0], ns, d_roff, d_rpos, d_rout, ocap)
        relay.synchronize()
        route.synchronize()
        nbytes = int(d_opos[ns].item())
        assert torch.equal(d_opos[:ns + 1], d_rpos[:ns + 1]) and torch.equal(d_out[:nbytes], d_rout[:nbytes])
        out_bytes += nbytes
        out_entries += int(d_ooff[ns].item())
    assert torch.equal(states, srv_states) and torch.equal(saved, srv_states)
    in_bytes = sum(r[3] for r in recs)
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "calls_per_burst": len(chunks),
           "input_entries_per_stream": round(sum(int(r[1].sum()) for r in recs) / S, 1), "output_entries_per_stream": round(out_entries / S, 1),
           "input_bytes_per_stream": round(in_bytes / S, 1), "output_bytes_per_stream": round(out_bytes / S, 1),
           "output_over_input_bytes": round(out_bytes / in_bytes, 4)}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + "_us_per_input_record"] = st
    med = {k: statistics.median(v) for k, v in times.items()}
    out["state_route_over_coalesce"] = round(med["state_route"] / med["coalesce"], 3)
    relay.close()
    route.close()
    return out


def run_crop(W, H, S, rounds, kind):
    """The crop leg for one S and one input, T = 1 -> its dictionary.  coalesce: mi355_cwire_coalesce_cwire_batch on the records of
    one tick, the nearest route without the crop call.  crop_quarter / crop_full: mi355_cwire_crop_cwire_batch on the same records
    with the rectangle (W/4, H/4, W/2, H/2) for every stream, and with the full frame.  All on one core's own stream, alternating
    within every round."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n, T = 3 * W * H, 1
    passes = 2 * max(1, 1024 // S)                     # ~2 k records per timed window
    if kind == "webcam":                                # run_burst's input: one stream cut into S pieces
        _, web = synth.webcam_stream(S + 1, W, H, device=dev)
        web = web.reshape(S + 1, n)
        states0, fwd = web[0:S].clone(), web[1:].reshape(S, T, n)
    else:
        states0, fwd = local_streams(S, T, W, H, dev)
    per_call = min(S, max(1, ((1 << 32) - 1) // n))                  # streams per call: max_batch * N < 2^32
    chunks = [(s0, min(per_call, S - s0)) for s0 in range(0, S, per_call)]
    recs = []                                           # per chunk: (records, counts, escapes, bytes)
    srv_states = states0.clone()
    with CUDACore(W, H, max_batch=per_call) as server:
        for s0, ns in chunks:
            cwcap = cwire_bytes_max(n, ns)
            d_off = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
            d_pos = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
            d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            server.diff_multi_stream_cwire_batch(fwd[s0], srv_states[s0], ns, T, d_off, d_pos, d_cw, cwcap)
            server.synchronize()
            pos = d_pos.cpu().numpy().astype(np.int64)
            counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
            pad = (counts.astype(np.int64) + 3) & ~3
            escapes = ((np.diff(pos) - 8 - 2 * pad) // 4).astype(np.uint32)
            recs.append((d_cw[:int(pos[ns])].clone(), counts, escapes, int(pos[ns])))
            del d_cw
    ocap = cwire_bytes_max(n, per_call)
    d_ooff = torch.zeros(per_call + 1, dtype=torch.int32, device=dev)
    d_opos = torch.zeros(per_call + 1, dtype=torch.int64, device=dev)
    d_out = torch.empty(ocap, dtype=torch.uint8, device=dev)
    d_coff, d_cpos, d_cout = torch.zeros_like(d_ooff), torch.zeros_like(d_opos), torch.empty_like(d_out)
    quarter = np.tile(np.array([W // 4, H // 4, W // 2, H // 2], np.int32), (per_call, 1))
    full = np.tile(np.array([0, 0, W, H], np.int32), (per_call, 1))
    relay = CUDACore(W, H, max_batch=per_call)
    torch.cuda.synchronize()

    def leg_coalesce():
        for _ in range(passes):
            for (s0, ns), r in zip(chunks, recs):
                relay.cwire_coalesce_cwire_batch(r[0], r[1], r[2], ns, T, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()

    def leg_crop(rects):
        def leg():
            for _ in range(passes):
                for (s0, ns), r in zip(chunks, recs):
                    relay.cwire_crop_cwire_batch(r[0], r[1], r[2], ns, T, rects, d_ooff, d_opos, d_out, ocap)
            relay.synchronize()
        return leg

    table = {"coalesce": leg_coalesce, "crop_quarter": leg_crop(quarter), "crop_full": leg_crop(full)}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * S))
    # the full-frame crop of one record per stream is the coalescer's output (and the input); the quarter holds fewer entries
    in_entries = quarter_entries = quarter_bytes = 0
    for (s0, ns), r in zip(chunks, recs):
        relay.cwire_coalesce_cwire_batch(r[0], r[1], r[2], ns, T, d_coff, d_cpos, d_cout, ocap)
        relay.cwire_crop_cwire_batch(r[0], r[1], r[2], ns, T, full, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()
        nbytes = int(d_cpos[ns].item())
        assert nbytes == r[3] and torch.equal(d_opos[:ns + 1], d_cpos[:ns + 1]) and torch.equal(d_out[:nbytes], d_cout[:nbytes])
        assert torch.equal(d_out[:nbytes], r[0])
        in_entries += int(d_coff[ns].item())
        relay.cwire_crop_cwire_batch(r[0], r[1], r[2], ns, T, quarter, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()
        quarter_entries += int(d_ooff[ns].item())
        quarter_bytes += int(d_opos[ns].item())
    assert quarter_entries <= in_entries
    in_bytes = sum(r[3] for r in recs)
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "calls_per_tick": len(chunks),
           "rectangle": [int(v) for v in quarter[0]],
           "input_entries_per_stream": round(in_entries / S, 1), "quarter_entries_per_stream": round(quarter_entries / S, 1),
           "input_bytes_per_stream": round(in_bytes / S, 1), "quarter_bytes_per_stream": round(quarter_bytes / S, 1)}
    med, spread = {}, {}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + "_us_per_stream"] = st
        med[name], spread[name] = st["median"], st["max"] - st["min"]
    out["crop_quarter_over_coalesce"] = round(med["crop_quarter"] / med["coalesce"], 3)
    out["crop_full_over_coalesce"] = round(med["crop_full"] / med["coalesce"], 3)
    # the expectation: the quarter no slower than the coalescer by more than the rounds' spread (of either leg)
    out["quarter_no_slower_than_coalesce"] = bool(med["crop_quarter"] <= med["coalesce"] + max(spread["crop_quarter"], spread["coalesce"]))
    out["full_minus_coalesce_us_per_call"] = round((med["crop_full"] - med["coalesce"]) * S / len(chunks), 3)
    relay.close()
    return out


def run_split(W, H, S, rounds, kind, limits=(1400, 8972)):
    """The split leg for one S and one input, T = 1 -> its dictionary.  coalesce: mi355_cwire_coalesce_cwire_batch on the records of
    one tick (with T = 1 it gives the input back): the nearest call of the family that reads every record once and writes it once.
    split_M: mi355_cwire_split_cwire_batch on the same records at max_bytes = M.  All on one core's own stream, alternating within
    every round.  Before anything is timed the pieces are compared with mi355_cwire_split_host."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, cwire_split_bytes_max, cwire_split_host, cwire_split_pieces_max
    dev = torch.device("cuda", 0)
    n, T = 3 * W * H, 1
    passes = 2 * max(1, 1024 // S)                     # ~2 k records per timed window
    if kind == "webcam":                                # run_burst's input: one stream cut into S pieces
        _, web = synth.webcam_stream(S + 1, W, H, device=dev)
        web = web.reshape(S + 1, n)
        states0, fwd = web[0:S].clone(), web[1:].reshape(S, T, n)
    else:
        states0, fwd = local_streams(S, T, W, H, dev)
    per_call = min(S, max(1, ((1 << 32) - 1) // n))                  # streams per call: max_batch * N < 2^32
    chunks = [(s0, min(per_call, S - s0)) for s0 in range(0, S, per_call)]
    recs = []                                           # per chunk: (records, counts, escapes, bytes)
    srv_states = states0.clone()
    with CUDACore(W, H, max_batch=per_call) as server:
        for s0, ns in chunks:
            cwcap = cwire_bytes_max(n, ns)
            d_off = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
            d_pos = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
            d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            server.diff_multi_stream_cwire_batch(fwd[s0], srv_states[s0], ns, T, d_off, d_pos, d_cw, cwcap)
            server.synchronize()
            pos = d_pos.cpu().numpy().astype(np.int64)
            counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
            pad = (counts.astype(np.int64) + 3) & ~3
            escapes = ((np.diff(pos) - 8 - 2 * pad) // 4).astype(np.uint32)
            recs.append((d_cw[:int(pos[ns])].clone(), counts, escapes, int(pos[ns])))
            del d_cw
    ocap = cwire_bytes_max(n, per_call)
    d_ooff = torch.zeros(per_call + 1, dtype=torch.int32, device=dev)
    d_opos = torch.zeros(per_call + 1, dtype=torch.int64, device=dev)
    d_out = torch.empty(ocap, dtype=torch.uint8, device=dev)
    low = min(limits)
    pcap = max(sum(cwire_split_pieces_max(c, e, low) for c, e in zip(r[1], r[2])) for r in recs)
    bcap = max(sum(cwire_split_bytes_max(c, e, low) for c, e in zip(r[1], r[2])) for r in recs)
    d_first = torch.zeros(per_call + 1, dtype=torch.int32, device=dev)
    d_ppos = torch.zeros(pcap + 1, dtype=torch.int64, device=dev)
    d_pieces = torch.empty(bcap, dtype=torch.uint8, device=dev)
    relay = CUDACore(W, H, max_batch=per_call)
    torch.cuda.synchronize()

    def leg_coalesce():
        for _ in range(passes):
            for (s0, ns), r in zip(chunks, recs):
                relay.cwire_coalesce_cwire_batch(r[0], r[1], r[2], ns, T, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()

    def leg_split(M):
        def leg():
            for _ in range(passes):
                for (s0, ns), r in zip(chunks, recs):
                    relay.cwire_split_cwire_batch(r[0], r[1], r[2], ns, M, d_first, d_ppos, pcap, d_pieces, bcap)
            relay.synchronize()
        return leg

    # the pieces are the host form's, at every limit
    in_entries = sum(int(r[1].sum()) for r in recs)
    in_bytes = sum(r[3] for r in recs)
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "calls_per_tick": len(chunks),
           "input_entries_per_stream": round(in_entries / S, 1), "input_bytes_per_stream": round(in_bytes / S, 1)}
    for M in limits:
        pieces = nbytes = 0
        for (s0, ns), r in zip(chunks, recs):
            relay.cwire_split_cwire_batch(r[0], r[1], r[2], ns, M, d_first, d_ppos, pcap, d_pieces, bcap)
            relay.synchronize()
            wf, wp, wo = cwire_split_host(r[0].cpu().numpy(), r[1], r[2], n, M, piece_capacity=pcap, capacity_bytes=bcap)
            total = int(wf[-1])
            assert np.array_equal(d_first[:ns + 1].cpu().numpy().view(np.uint32), wf)
            assert np.array_equal(d_ppos[:total + 1].cpu().numpy().view(np.uint64), wp[:total + 1])
            assert np.array_equal(d_pieces[:int(wp[total])].cpu().numpy(), wo[:int(wp[total])])
            pieces += total
            nbytes += int(wp[total])
        out[f"pieces_per_stream_{M}"] = round(pieces / S, 1)
        out[f"piece_bytes_per_stream_{M}"] = round(nbytes / S, 1)
    table = {"coalesce": leg_coalesce}
    table.update({f"split_{M}": leg_split(M) for M in limits})
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * S))
    med, spread = {}, {}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + "_us_per_record"] = st
        med[name], spread[name] = st["median"], st["max"] - st["min"]
    for M in limits:
        out[f"split_{M}_over_coalesce"] = round(med[f"split_{M}"] / med["coalesce"], 3)
        # the expectation: no slower than the coalescer by more than the rounds' spread (of either leg)
        out[f"split_{M}_no_slower_than_coalesce"] = bool(med[f"split_{M}"] <= med["coalesce"] + max(spread[f"split_{M}"], spread["coalesce"]))
    relay.close()
    return out


def run_fec(W, H, S, rounds, kind, M=1400, G=8):
    """The fec leg for one S and one input, T = 1 -> its dictionary.  split: mi355_cwire_split_cwire_batch at max_bytes = M on the
    records of one tick; fec_k1 / fec_k2: mi355_cwire_fec_batch with K = 1 / 2 parity blocks per group of G on the pieces that call
    left; repair_one / repair_two: mi355_cwire_fec_repair_batch with one job per stream, the first piece (the first two) of its
    first group lost.  All on one core's own stream, alternating within every round.  Before anything is timed the parity is
    compared with mi355_cwire_fec_host and the rebuilt pieces with the pieces."""
    import numpy as np
    from cudavideostream_amd import (CUDACore, cwire_bytes_max, cwire_fec_groups_max, cwire_fec_host, cwire_split_bytes_max, cwire_split_host,
                                     cwire_split_pieces_max, lib)
    dev = torch.device("cuda", 0)
    n, T = 3 * W * H, 1
    passes = 2 * max(1, 1024 // S)                     # ~2 k records per timed window
    if kind == "webcam":                                # run_split's input
        _, web = synth.webcam_stream(S + 1, W, H, device=dev)
        web = web.reshape(S + 1, n)
        states0, fwd = web[0:S].clone(), web[1:].reshape(S, T, n)
    else:
        states0, fwd = local_streams(S, T, W, H, dev)
    assert S * n < (1 << 32), "one call per tick: max_batch * N < 2^32"
    cwcap = cwire_bytes_max(n, S)
    with CUDACore(W, H, max_batch=S) as server:
        d_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        d_pos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        server.diff_multi_stream_cwire_batch(fwd, states0.clone(), S, T, d_off, d_pos, d_cw, cwcap)
        server.synchronize()
        pos = d_pos.cpu().numpy().astype(np.int64)
        counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
        escapes = ((np.diff(pos) - 8 - 2 * ((counts.astype(np.int64) + 3) & ~3)) // 4).astype(np.uint32)
        recs = d_cw[:int(pos[S])].clone()
        del d_cw
    pcap = sum(cwire_split_pieces_max(c, e, M) for c, e in zip(counts, escapes))
    bcap = sum(cwire_split_bytes_max(c, e, M) for c, e in zip(counts, escapes))
    gcap = cwire_fec_groups_max(pcap, S, G)
    d_first = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_ppos = torch.zeros(pcap + 1, dtype=torch.int64, device=dev)
    d_all = torch.zeros(bcap + 2 * gcap * M, dtype=torch.uint8, device=dev)   # the pieces, then the parity blocks: the repair's d_rx
    d_pieces, d_par = d_all[:bcap], d_all[bcap:]
    d_ffirst = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_flen = torch.zeros(gcap, dtype=torch.int32, device=dev)
    d_rep = torch.zeros(2 * S * M, dtype=torch.uint8, device=dev)
    d_vd = torch.zeros(2 * S, dtype=torch.int32, device=dev)
    relay = CUDACore(W, H, max_batch=S)
    torch.cuda.synchronize()

    def split():
        relay.cwire_split_cwire_batch(recs, counts, escapes, S, M, d_first, d_ppos, pcap, d_pieces, bcap)

    def fec(K):
        relay.cwire_fec_batch(d_pieces, bcap, d_first, d_ppos, pcap, S, G, K, M, d_ffirst, d_flen, gcap, d_par, gcap * K * M)

    # the pieces and the parity are the host forms', at both K
    wf, wp, wo = cwire_split_host(recs.cpu().numpy(), counts, escapes, n, M, piece_capacity=pcap, capacity_bytes=bcap)
    total = int(wf[-1])
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "max_bytes": M, "group": G,
           "input_entries_per_stream": round(int(counts.sum()) / S, 1), "input_bytes_per_stream": round(int(pos[S]) / S, 1),
           "pieces_per_stream": round(total / S, 1), "piece_bytes_per_stream": round(int(wp[total]) / S, 1)}
    for K in (1, 2):
        split()
        fec(K)                                          # behind the split call, no synchronisation in between
        relay.synchronize()
        hf, hl, ho = cwire_fec_host(wo, bcap, wf, wp, pcap, G, K, M, group_capacity=gcap, capacity_bytes=gcap * K * M)
        ng = int(hf[-1])
        assert np.array_equal(d_pieces[:int(wp[total])].cpu().numpy(), wo[:int(wp[total])])
        assert np.array_equal(d_ffirst.cpu().numpy().view(np.uint32), hf) and np.array_equal(d_flen[:ng].cpu().numpy().view(np.uint32), hl[:ng])
        got = d_par[:ng * K * M].cpu().numpy().reshape(ng * K, M)
        want = ho[:ng * K * M].reshape(ng * K, M)
        for g in range(ng):
            L = int(hl[g])
            assert L > 0 and np.array_equal(got[g * K:(g + 1) * K, :L], want[g * K:(g + 1) * K, :L]), (K, g)
        out[f"groups_per_stream_k{K}"] = round(ng / S, 1)
        out[f"parity_bytes_per_stream_k{K}"] = round(K * int(hl[:ng].astype(np.int64).sum()) / S, 1)
    # (K = 2 is what d_par holds now)  one repair job per stream with a piece: its first group, the first piece or two lost
    A = lib.FEC_ABSENT
    jobs = {}
    for lose in (1, 2):
        job_first, slot_off, slot_len, par_off, fec_len, lost = [0], [], [], [], [], []
        for s in range(S):
            c = int(wf[s + 1]) - int(wf[s])
            if c == 0:
                continue
            m, p0, g = min(G, c), int(wf[s]), int(hf[s])
            gone = list(range(min(lose, m)))
            for i in range(m):
                slot_off.append(A if i in gone else int(wp[p0 + i]))
                slot_len.append(int(wp[p0 + i + 1]) - int(wp[p0 + i]))
            par_off.append([bcap + 2 * g * M, bcap + (2 * g + 1) * M if len(gone) == 2 else A])
            fec_len.append(int(hl[g]))
            job_first.append(len(slot_off))
            lost.append([p0 + i for i in gone])
        jobs[lose] = (len(fec_len), np.array(job_first, np.uint32), np.array(slot_off, np.uint64), np.array(slot_len, np.uint32),
                      np.array(par_off, np.uint64), np.array(fec_len, np.uint32), lost)

    def repair(lose):
        nj, jf, so, sl, po, fl, _ = jobs[lose]
        relay.cwire_fec_repair_batch(d_all, d_all.numel(), nj, jf, so, sl, po, fl, d_rep, M, d_vd)

    for lose in (1, 2):
        repair(lose)
        relay.synchronize()
        rep, vd = d_rep.cpu().numpy().reshape(2 * S, M), d_vd.cpu().numpy()
        for j, ps in enumerate(jobs[lose][6]):
            for k, p in enumerate(ps):
                a, b = int(wp[p]), int(wp[p + 1])
                assert vd[2 * j + k] == 0 and np.array_equal(rep[2 * j + k, :b - a], wo[a:b]), (lose, j, k)
        out[f"repair_jobs_{lose}"] = jobs[lose][0]

    def timed(call):
        def leg():
            for _ in range(passes):
                call()
            relay.synchronize()
        return leg

    table = {"split": timed(split), "fec_k1": timed(lambda: fec(1)), "fec_k2": timed(lambda: fec(2)),
             "repair_one": timed(lambda: repair(1)), "repair_two": timed(lambda: repair(2))}
    split()
    relay.synchronize()
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                per = jobs[1][0] if name.startswith("repair") else S
                times.setdefault(name, []).append(dt * 1e6 / (passes * max(per, 1)))
    med, spread = {}, {}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + ("_us_per_job" if name.startswith("repair") else "_us_per_record")] = st
        med[name], spread[name] = st["median"], st["max"] - st["min"]
    for K in (1, 2):
        out[f"fec_k{K}_over_split"] = round(med[f"fec_k{K}"] / med["split"], 3)
    # the expectation: at K = 2 no slower than the split call that feeds it by more than the rounds' spread (of either leg)
    out["fec_k2_no_slower_than_split"] = bool(med["fec_k2"] <= med["split"] + max(spread["fec_k2"], spread["split"]))
    relay.close()
    return out


def run_mosaic(W, H, S, T, rounds, kind):
    """The mosaic leg for one (S, T) and one input -> its dictionary.  mosaic: mi355_cwire_mosaic_cwire_batch on the burst's
    records, whole frames in a C x R grid.  state_route: mi355_apply_multi_stream_cwire_batch onto states the relay holds,
    mi355_wall_compose_batch at k = 1 into a canvas, a synchronize, mi355_diff_stream_cwire_batch(nframes = 1) on a threshold-0
    core of the canvas' geometry.  Alternating within every round."""
    import math
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    C = math.isqrt(S - 1) + 1
    R = (S + C - 1) // C
    cw, ch = C * W, R * H
    nc = 3 * cw * ch
    assert B * n < (1 << 32) and nc < (1 << 31), "the leg runs in one call: max_batch * N < 2^32 and a canvas below 2^31 bytes"
    passes = 2 * max(1, 256 // B)
    if kind == "webcam":                                # run_burst's input: one stream cut into S pieces
        _, web = synth.webcam_stream(B + 1, W, H, device=dev)
        web = web.reshape(B + 1, n)
        states0, fwd = web[0:B:T].clone(), web[1:].reshape(S, T, n)
    else:
        states0, fwd = local_streams(S, T, W, H, dev)
    cwcap = cwire_bytes_max(n, B)
    d_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    srv_states = states0.clone()
    with CUDACore(W, H, max_batch=B) as server:
        torch.cuda.synchronize()
        server.diff_multi_stream_cwire_batch(fwd, srv_states, S, T, d_off, d_pos, d_cw, cwcap)
        server.synchronize()
    pos = d_pos.cpu().numpy().astype(np.int64)
    counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
    pad = (counts.astype(np.int64) + 3) & ~3
    escapes = ((np.diff(pos) - 8 - 2 * pad) // 4).astype(np.uint32)
    recs, in_bytes = d_cw[:int(pos[B])].clone(), int(pos[B])
    del d_cw, fwd, srv_states
    ocap = cwire_bytes_max(nc, 1)
    d_ooff = torch.zeros(2, dtype=torch.int32, device=dev)
    d_opos = torch.zeros(2, dtype=torch.int64, device=dev)
    d_out = torch.empty(ocap, dtype=torch.uint8, device=dev)
    d_roff, d_rpos, d_rout = torch.zeros_like(d_ooff), torch.zeros_like(d_opos), torch.empty_like(d_out)
    place = np.array([[0, 0, W, H, (s % C) * W, (s // C) * H] for s in range(S)], np.int32)
    wall_place = np.array([[(s % C) * W, (s // C) * H, 1] for s in range(S)], np.int32)
    states = states0.clone()
    d_canvas = torch.zeros(nc, dtype=torch.uint8, device=dev)
    relay = CUDACore(W, H, max_batch=max(B, C * R))    # one fact word per canvas tile where max_batch frames keep theirs
    route = CUDACore(W, H, max_batch=B)
    canvas = CUDACore(cw, ch, max_batch=1, threshold=0)
    torch.cuda.synchronize()

    def route_pass():
        route.apply_multi_stream_cwire_batch(recs, counts, escapes, S, T, states)
        route.wall_compose_batch(states, S, wall_place, d_canvas, cw, ch)
        route.synchronize()
        canvas.diff_stream_cwire_batch(d_canvas, 1, d_roff, d_rpos, d_rout, ocap)

    # the route's record of the first burst, from a canvas core primed with the tiling of the base states, is the call's record
    route.wall_compose_batch(states, S, wall_place, d_canvas, cw, ch)
    route.synchronize()
    canvas.diff_stream_cwire_batch(d_canvas, 1, d_roff, d_rpos, d_rout, ocap)
    canvas.synchronize()
    route_pass()
    canvas.synchronize()
    relay.cwire_mosaic_cwire_batch(recs, counts, escapes, S, T, place, cw, ch, d_ooff, d_opos, d_out, ocap)
    relay.synchronize()
    out_entries, out_bytes = int(d_ooff[1].item()), int(d_opos[1].item())
    equal = bool(int(d_rpos[1].item()) == out_bytes and torch.equal(d_rout[:out_bytes], d_out[:out_bytes]))

    def leg_mosaic():
        for _ in range(passes):
            relay.cwire_mosaic_cwire_batch(recs, counts, escapes, S, T, place, cw, ch, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()

    def leg_route():
        for _ in range(passes):
            route_pass()
        canvas.synchronize()

    table = {"mosaic": leg_mosaic, "state_route": leg_route}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, leg in table.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * B))
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "grid": [C, R], "canvas": [cw, ch],
           "input_entries_per_record": round(float(counts.sum()) / B, 1), "input_bytes_per_record": round(in_bytes / B, 1),
           "canvas_entries": out_entries, "canvas_record_bytes": out_bytes, "route_record_equals_mosaic": equal}
    med, spread = {}, {}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + "_us_per_record"] = st
        med[name], spread[name] = st["median"], st["max"] - st["min"]
    out["mosaic_over_route"] = round(med["mosaic"] / med["state_route"], 3)
    out["mosaic_no_slower_than_route"] = bool(med["mosaic"] <= med["state_route"] + max(spread["mosaic"], spread["state_route"]))
    for c in (relay, route, canvas):
        c.close()
    return out


def run_budget(W, H, S, rounds):
    """The budget leg for one S -> its dictionary.  budget: mi355_cwire_budget_cwire_batch on the records of one tick with every
    stream's budget at half of its count, on the states as the tick left them.  second_diff: mi355_diff_multi_cwire_batch over the
    same S frames from the states before the tick -- the cheapest re-diff a caller has without the call (and one that still lacks
    the threshold choice).  Both on a core's own stream; every pass of a timed window has its own copy of the states, restored
    outside the window, so no pass sees what another one wrote."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    passes = max(2, min(16, 128 // S))
    _, web = synth.webcam_stream(S + 1, W, H, device=dev)
    web = web.reshape(S + 1, n)
    pre, frames = web[:S].clone(), web[1:].clone()      # stream s: webcam frame s -> s + 1
    cwcap = cwire_bytes_max(n, S)
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_cw = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    d_thr = torch.zeros(S, dtype=torch.int32, device=dev)
    d_ooff, d_opos, d_out = torch.zeros_like(d_off), torch.zeros_like(d_pos), torch.empty_like(d_cw)
    d_roff, d_rpos, d_rcw = torch.zeros_like(d_off), torch.zeros_like(d_pos), torch.empty_like(d_cw)
    post = pre.clone()
    core = CUDACore(W, H, max_batch=S)
    torch.cuda.synchronize()
    core.diff_multi_cwire_batch(frames, post, S, d_off, d_pos, d_cw, cwcap)
    core.synchronize()
    pos = d_pos.cpu().numpy().astype(np.int64)
    counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
    escapes = ((np.diff(pos) - 8 - 2 * ((counts.astype(np.int64) + 3) & ~3)) // 4).astype(np.uint32)
    budgets = (counts // 2).astype(np.uint32)
    work = torch.empty(passes, S, n, dtype=torch.uint8, device=dev)

    def leg_budget():
        for p in range(passes):
            core.cwire_budget_cwire_batch(d_cw, counts, escapes, work[p], S, budgets, d_thr, d_ooff, d_opos, d_out, cwcap)
        core.synchronize()

    def leg_diff():
        for p in range(passes):
            core.diff_multi_cwire_batch(frames, work[p], S, d_roff, d_rpos, d_rcw, cwcap)
        core.synchronize()

    table = {"budget": (leg_budget, post), "second_diff": (leg_diff, pre)}
    times = {}
    for r in range(rounds + 1):                        # round 0 warms every leg up and is dropped
        for name, (leg, start) in table.items():
            work.copy_(start.unsqueeze(0).expand(passes, S, n))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times.setdefault(name, []).append(dt * 1e6 / (passes * S))
    kept = np.diff(d_ooff.cpu().numpy().view(np.uint32).astype(np.int64))
    thr = d_thr.cpu().numpy().view(np.uint32)
    assert (kept <= budgets).all() and (thr >= 20).all() and torch.equal(d_rpos, d_pos)
    out = {"streams": S, "passes": passes, "entries_per_stream": round(float(counts.mean()), 1),
           "kept_entries_per_stream": round(float(kept.mean()), 1), "record_bytes_per_stream": round(int(pos[S]) / S, 1),
           "kept_bytes_per_stream": round(int(d_opos[S].item()) / S, 1), "threshold_min": int(thr.min()), "threshold_max": int(thr.max())}
    for name in table:
        st = stats(times[name])
        st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + "_us_per_stream"] = st
    out["second_diff_over_budget"] = round(statistics.median(times["second_diff"]) / statistics.median(times["budget"]), 3)
    core.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--streams", default="8,64,256")
    ap.add_argument("--steps", type=int, default=8, help="K: webcam frames a stream walks through")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="multi,cores_loop,pairs",
                    help="of multi, cores_loop, pairs, write_probe; or client alone; or burst alone; or burst_client alone; or coalesce alone; or crop alone; or split alone; or fec alone; or mosaic alone; or budget alone; or activity alone; or check alone; or refresh alone; or wall alone; or thumb alone")
    ap.add_argument("--frames", default="4,16,64", help="burst, burst_client and coalesce legs: T, frames per stream and call")
    a = ap.parse_args()
    have = load_library()
    W, H = (int(v) for v in a.size.split("x"))
    if a.legs == "client":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            per.append(run_client(W, H, S, a.steps, a.rounds))
            torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_client", "size": f"{W}x{H}", "input": "synth.webcam_stream", "rounds": a.rounds,
                          "steps": a.steps, "client": per}), flush=True)
        return
    if a.legs == "burst":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            for T in (int(v) for v in a.frames.split(",")):
                per.append(run_burst(W, H, S, T, a.rounds))
                torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_stream", "size": f"{W}x{H}", "input": "synth.webcam_stream", "rounds": a.rounds,
                          "burst": per}), flush=True)
        return
    if a.legs == "burst_client":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            for T in (int(v) for v in a.frames.split(",")):
                for kind in ("webcam", "local"):
                    per.append(run_burst_client(W, H, S, T, a.rounds, kind))
                    torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_stream_client", "size": f"{W}x{H}", "rounds": a.rounds, "burst_client": per}), flush=True)
        return
    if a.legs == "coalesce":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            for T in (int(v) for v in a.frames.split(",")):
                for kind in ("webcam", "local"):
                    per.append(run_coalesce(W, H, S, T, a.rounds, kind))
                    print(f"coalesce S={S} T={T} {kind}: done", file=sys.stderr, flush=True)
                    torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_coalesce", "size": f"{W}x{H}", "rounds": a.rounds, "coalesce": per}), flush=True)
        return
    if a.legs == "crop":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            for kind in ("webcam", "local"):
                per.append(run_crop(W, H, S, a.rounds, kind))
                print(f"crop S={S} {kind}: done", file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_crop", "size": f"{W}x{H}", "rounds": a.rounds, "crop": per}), flush=True)
        return
    if a.legs == "split":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            for kind in ("webcam", "local"):
                per.append(run_split(W, H, S, a.rounds, kind))
                print(f"split S={S} {kind}: done", file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
        ok = all(p[k] for p in per for k in p if k.endswith("_no_slower_than_coalesce"))
        print(json.dumps({"bench": "multi_split", "size": f"{W}x{H}", "rounds": a.rounds, "split": per,
                          "verdict": "no slower than coalesce at every point" if ok else "slower than coalesce at some point"}),
              flush=True)
        return
    if a.legs == "fec":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            for kind in ("webcam", "local"):
                per.append(run_fec(W, H, S, a.rounds, kind))
                print(f"fec S={S} {kind}: done", file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
        ok = all(p["fec_k2_no_slower_than_split"] for p in per)
        print(json.dumps({"bench": "multi_fec", "size": f"{W}x{H}", "rounds": a.rounds, "fec": per,
                          "verdict": "parity at K = 2 no slower than split at every point" if ok else "parity at K = 2 slower than split at some point"}),
              flush=True)
        return
    if a.legs == "mosaic":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            for T in (1, 16):
                for kind in ("webcam", "local"):
                    per.append(run_mosaic(W, H, S, T, a.rounds, kind))
                    print(f"mosaic S={S} T={T} {kind}: done", file=sys.stderr, flush=True)
                    torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_mosaic", "size": f"{W}x{H}", "rounds": a.rounds, "mosaic": per}), flush=True)
        return
    if a.legs == "budget":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            per.append(run_budget(W, H, S, a.rounds))
            print(f"budget S={S}: done", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_budget", "size": f"{W}x{H}", "input": "synth.webcam_stream", "rounds": a.rounds,
                          "budget": per}), flush=True)
        return
    if a.legs == "activity":
        points = [(S, 1) for S in (int(v) for v in a.streams.split(","))] + [(16, 16)]
        per = []
        for S, T in points:
            for kind in ("webcam", "local"):
                per.append(run_activity(W, H, S, T, a.rounds, kind))
                print(f"activity S={S} T={T} {kind}: done", file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_activity", "size": f"{W}x{H}", "rounds": a.rounds, "activity": per,
                          "verdict": "no slower than burst_apply at every point" if all(p["no_slower_than_burst_apply"] for p in per)
                          else "slower than burst_apply at some point"}), flush=True)
        return
    if a.legs == "check":
        points = [(S, 1) for S in (int(v) for v in a.streams.split(","))] + [(16, 16)]
        per = []
        for S, T in points:
            for kind in ("webcam", "local"):
                per.append(run_check(W, H, S, T, a.rounds, kind))
                print(f"check S={S} T={T} {kind}: done", file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_check", "size": f"{W}x{H}", "rounds": a.rounds, "check": per,
                          "verdict": "no slower than burst_apply at every point" if all(p["no_slower_than_burst_apply"] for p in per)
                          else "slower than burst_apply at some point"}), flush=True)
        return
    if a.legs == "refresh":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            per.append(run_refresh(W, H, S, a.rounds))
            print(f"refresh S={S}: done", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        print(json.dumps({"bench": "multi_refresh", "size": f"{W}x{H}", "rounds": a.rounds, "refresh": per,
                          "verdict": "digest no slower than diff at every S" if all(p["digest_no_slower_than_diff"] for p in per)
                          else "digest slower than diff at some S"}), flush=True)
        return
    if a.legs == "wall":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            per.append(run_wall(W, H, S, a.rounds))
            print(f"wall S={S}: done", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        ok_mask, ok_full = all(p["masked_local_cheaper_than_full"] for p in per), all(p["full_k8_no_slower_than_digest"] for p in per)
        print(json.dumps({"bench": "multi_wall", "size": f"{W}x{H}", "rounds": a.rounds, "wall": per,
                          "verdict": ("masked update on the moving block cheaper than the full compose at every k and S"
                                      if ok_mask else "masked update on the moving block not cheaper than the full compose at some k or S")
                          + "; " + ("full compose at k = 8 no slower than digest at every S" if ok_full
                                    else "full compose at k = 8 slower than digest at some S")}), flush=True)
        return
    if a.legs == "thumb":
        per = []
        for S in (int(v) for v in a.streams.split(",")):
            per.append(run_thumb(W, H, S, a.rounds))
            print(f"thumb S={S}: done", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        ok_route, ok_mask = all(p["touched_plus_call_no_slower_than_route"] for p in per), all(p["call_local_cheaper_than_nullmask"] for p in per)
        print(json.dumps({"bench": "multi_thumb", "size": f"{W}x{H}", "rounds": a.rounds, "thumb": per,
                          "verdict": ("touched tiles plus the call no slower than the wall-and-diff route at every point"
                                      if ok_route else "touched tiles plus the call slower than the wall-and-diff route at some point")
                          + "; " + ("the call with the moving block's mask cheaper than without a mask at every k and S" if ok_mask
                                    else "the call with the moving block's mask not cheaper than without a mask at some k or S")}), flush=True)
        return
    for S in (int(v) for v in a.streams.split(",")):
        run(W, H, S, a.steps, a.rounds, set(a.legs.split(",")), have)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

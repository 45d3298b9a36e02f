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

The despeckle leg (--legs despeckle, a run of its own: `--legs despeckle --streams 4,16,64 > profiles/multi_despeckle.json`)
measures the sender's second lever on the records of one tick, in microseconds per stream, ONE JSON line for all S, on the
webcam-like and the local input:
  despeckle    mi355_cwire_despeckle_cwire_batch at need = 3 for every stream;
  budget       mi355_cwire_budget_cwire_batch on the same records, every stream's budget at half of its count: the nearest
               sibling (the same directory, three tile passes, a state tile read).
The line carries entries and bytes in and out of both calls; on the webcam-like input the despeckle call's are compared with
mi355_cwire_despeckle_host's.  The expectation to test: `despeckle` no slower than `budget` by more than the rounds' spread
(judged strictly; `bitmap_pass_bytes_per_stream`, N/24, is the one cost the call has that follows N).

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

The runs leg (--legs runs, a run of its own: `--legs runs --streams 4,16,64 > profiles/multi_runs.json`) measures the link-edge
transcoder on the records of one tick (T = 1), us per record, on the webcam-like input, the local input and `keyframe`
(mi355_refresh_cwire_batch of every tile of the webcam-like states: what a late joiner is sent):
  coalesce       mi355_cwire_coalesce_cwire_batch with T = 1 on the same records: the split leg's comparator;
  encode         mi355_cwire_runs_encode_batch under MI355_RUNS_WHERE_SMALLER;
  decode         mi355_cwire_runs_decode_batch on what it wrote.
It also reports bytes in, bytes out and records packed per input; both outputs are compared with the host forms before anything is
timed.  The expectation to test: each no slower than `coalesce` by more than the rounds' spread
(`encode_no_slower_than_coalesce`, `decode_no_slower_than_coalesce`).

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
import itertools
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
KINDS = ("webcam", "local")


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


# ---- the inputs and the sender's records: what every leg is fed
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


def burst_input(kind, S, T, W, H, dev):
    """The burst-shaped input -> (states0 [S][n], frames [S][T][n]).  `webcam`: ONE webcam stream of S * T + 1 frames cut into S
    pieces, stream s starts from frame s * T as its state and takes the T frames behind it (a view of the stream); `local`:
    local_streams.  With T = 1 it is one tick of S streams."""
    if kind != "webcam":
        return local_streams(S, T, W, H, dev)
    n, B = 3 * W * H, S * T
    _, web = synth.webcam_stream(B + 1, W, H, device=dev)
    web = web.reshape(B + 1, n)
    return web[0:B:T].clone(), web[1:].reshape(S, T, n)


def burst_chunks(S, T, n):
    """A core takes max_batch * N < 2^32 bytes per call: the whole streams one call holds, and the fewest calls that cover S
    streams of T frames as (first stream, streams)."""
    per_call = min(S, max(1, ((1 << 32) - 1) // n // T))
    return per_call, [(s0, min(per_call, S - s0)) for s0 in range(0, S, per_call)]


def sender_records(W, H, fwd, states):
    """The records of the burst fwd [S][T][n] from states [S][n], as a sender's mi355_diff_multi_stream_cwire_batch makes them on
    a throw-away server core, one call per chunk of burst_chunks -> per chunk (records, counts, escapes, positions): the record
    bytes cut to their end, the two header words of every record and the chunk's uint64[streams * T + 1] record positions.
    `states` is advanced to the server's states after the burst."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    S, T, n = fwd.shape
    per_call, chunks = burst_chunks(S, T, n)
    recs = []
    with CUDACore(W, H, max_batch=per_call * T) as server:
        for s0, ns in chunks:
            nb = ns * T
            cwcap = cwire_bytes_max(n, nb)
            d_off = torch.zeros(nb + 1, dtype=torch.int32, device=fwd.device)
            d_pos = torch.zeros(nb + 1, dtype=torch.int64, device=fwd.device)
            d_cw = torch.empty(cwcap, dtype=torch.uint8, device=fwd.device)
            torch.cuda.synchronize()
            server.diff_multi_stream_cwire_batch(fwd[s0], states[s0], ns, T, d_off, d_pos, d_cw, cwcap)
            server.synchronize()
            pos = d_pos.cpu().numpy().astype(np.int64)
            counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
            pad = (counts.astype(np.int64) + 3) & ~3     # a record: 8 header bytes, 2 * pad4(count) and 4 per escape
            escapes = ((np.diff(pos) - 8 - 2 * pad) // 4).astype(np.uint32)
            recs.append((d_cw[:int(pos[nb])].clone(), counts, escapes, pos))
            del d_cw
    torch.cuda.synchronize()
    return recs


def one_call(recs):
    """The records of a leg that runs in one call."""
    assert len(recs) == 1, "the leg runs in one call: max_batch * N < 2^32"
    return recs[0]


def mask_bits(d_mask):
    """Tiles selected in a tile mask of 32-bit words."""
    return int(sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in d_mask.cpu().numpy()))


# ---- the method: how every leg is timed, reported and judged
def time_legs(table, rounds, per, before=None, after=None):
    """Times the legs of `table` (name -> closure that ends in its cores' own synchronize()) -> name -> microseconds per unit of
    every round but the first, which warms every leg up and is dropped.  The legs alternate within every round, in the table's
    order.  `before(name)`, a leg's restore of its states or work copies, runs outside the timed window, which is
    time.perf_counter() around leg() alone, behind a device-wide synchronize; `after(name)` runs behind it.  `per` is the units
    of one window, a number or a function of the name."""
    times = {name: [] for name in table}
    for r in range(rounds + 1):
        for name, leg in table.items():
            if before:
                before(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if r:
                times[name].append(dt * 1e6 / (per(name) if callable(per) else per))
            if after:
                after(name)
    return times


def restorer(states, states0, cores, host0, cores_leg):
    """before(name) of the legs that advance caller-held states, and, in the leg `cores_leg`, the states of one core each."""
    def before(name):
        states.copy_(states0)
        if name == cores_leg:
            for s, c in enumerate(cores):
                c.set_state(host0[s])
    return before


def stats(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}


def report(out, times, unit, spread=False, as_printed=False):
    """out[name + unit] = the statistics of the leg's rounds, with the relative spread where the leg prints it -> name ->
    (median, max - min), the figures a leg is judged by: of the rounds themselves, or, where the leg judges by what it prints,
    of the rounded statistics."""
    fig = {}
    for name, us in times.items():
        st = stats(us)
        if spread:
            st["spread"] = round((st["max"] - st["min"]) / st["median"], 4)
        out[name + unit] = st
        fig[name] = (st["median"], st["max"] - st["min"]) if as_printed else (statistics.median(us), max(us) - min(us))
    return fig


def ratio(fig, a, b, digits=3):
    return round(fig[a][0] / fig[b][0], digits)


def versus(fig, a, b):
    """(a over b, a no slower than b by more than the rounds' spread: the larger of the two legs' max - min)."""
    return ratio(fig, a, b), bool(fig[a][0] <= fig[b][0] + max(fig[a][1], fig[b][1]))


def cheaper(fig, a, b):
    """a cheaper than b by more than the rounds' spread."""
    return bool(fig[a][0] + max(fig[a][1], fig[b][1]) < fig[b][0])


# ---- the legs
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
    reset = restorer(states, states0, cores, states0.cpu().numpy() if cores else None, "cores_loop")

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
    table = {k: leg for k, leg in table.items()
             if ("multi" if k.startswith("multi") else k) in legs and (have_multi or not k.startswith("multi"))}
    times = time_legs(table, rounds, ticks * S, before=reset)
    if "multi" in table:
        reset("multi")
        torch.cuda.synchronize()
        core.diff_multi_batch(frames[1:1 + S], states, S, d_off, d_xs, d_df, cap)
        core.synchronize()
        total = int(d_off.cpu()[-1])
        assert 0 < total <= cap
        result["changed_bytes_per_frame"] = round(total / S, 1)
    fig = report(result, times, "_us_per_frame")
    if "multi" in times and "cores_loop" in times:
        result["cores_loop_over_multi"] = ratio(fig, "cores_loop", "multi", 2)
    if "multi" in times and "pairs" in times:
        result["multi_over_pairs"] = ratio(fig, "multi", "pairs")
    if "write_probe" in legs:                          # the board's streaming-write rate (wide stores), for the write-back's bound
        result["hbm_write_gbps"] = round(core.probe_hbm_write(1024, narrow=False), 1)
    print(json.dumps(result), flush=True)
    for c in cores:
        c.close()
    core.close()


def run_client(W, H, rounds, S, K):
    """The client leg for one S -> its dictionary."""
    import numpy as np
    from cudavideostream_amd import CUDACore
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    ticks = max(16, min(512, 4096 // S))
    _, frames = synth.webcam_stream(S + K + 1, W, H, device=dev)
    frames = frames.reshape(S + K + 1, n)
    states0 = frames[:S].clone()
    states = states0.clone()
    recs = []                                          # per recorded tick: (records, counts, escapes, positions)
    for j in range(1, K + 1):
        recs.append(one_call(sender_records(W, H, frames[j:j + S].unsqueeze(1), states)))
    cap = max(int(r[1].sum()) for r in recs) + 16
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_xs = torch.empty(cap, dtype=torch.int32, device=dev)
    d_df = torch.empty(cap, dtype=torch.uint8, device=dev)
    client = CUDACore(W, H, max_batch=S)
    cores = [CUDACore(W, H, max_batch=1) for _ in range(S)]
    own = [[r[0][int(r[3][s]):int(r[3][s + 1])] for s in range(S)] for r in recs]   # camera s's record of tick k
    hdr = [[(r[1][s:s + 1], r[2][s:s + 1]) for s in range(S)] for r in recs]
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
    times = time_legs(table, rounds, ticks * S, before=restorer(states, states0, cores, states0.cpu().numpy(), "cores_client"))
    out = {"streams": S, "ticks": ticks, "changed_bytes_per_stream": round(sum(int(r[1].sum()) for r in recs) / (K * S), 1),
           "record_bytes_per_stream": round(sum(int(r[3][S]) for r in recs) / (K * S), 1),
           "touched_tiles_per_stream": round(sum(touched) / (K * S), 1), "tiles_per_state": (n + 4095) // 4096,
           "state_bytes_moved_per_stream": round(sum(touched) * 2 * 4096 / (K * S), 1), "state_bytes_2N": 2 * n}
    fig = report(out, times, "_us_per_stream")
    out["cores_client_over_multi_client"] = ratio(fig, "cores_client", "multi_client", 2)
    out["decode_arrays_over_multi_client"] = ratio(fig, "decode_arrays", "multi_client", 2)
    for c in cores:
        c.close()
    client.close()
    return out


def run_burst(W, H, rounds, S, T):
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
    per_call, chunks = burst_chunks(S, T, n)
    burst = CUDACore(W, H, max_batch=per_call * T)
    ticks = CUDACore(W, H, max_batch=S)
    cores = [CUDACore(W, H, max_batch=T) for _ in range(S)]
    one = cwcap // S
    outs = [(torch.zeros(T + 1, dtype=torch.int32, device=dev), torch.zeros(T + 1, dtype=torch.int64, device=dev),
             torch.empty(one, dtype=torch.uint8, device=dev)) for _ in range(S)]
    for c in [burst, ticks] + cores:
        c.prepare(lib.PREPARE_BATCHES)
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
    times = time_legs(table, rounds, passes * B, before=restorer(states, states0, cores, states0.cpu().numpy(), "cores_stream"))
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
    fig = report(out, times, "_us_per_frame")
    out["multi_ticks_over_burst"] = ratio(fig, "multi_ticks", "burst_cwire")
    out["cores_stream_over_burst"] = ratio(fig, "cores_stream", "burst_cwire")
    for c in [burst, ticks] + cores:
        c.close()
    return out


def run_burst_client(W, H, rounds, S, T, kind):
    """The burst-client leg for one (S, T) and one input -> its dictionary."""
    import numpy as np
    from cudavideostream_amd import CUDACore
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    ntiles = (n + 4095) // 4096
    passes = 2 * max(1, 1024 // B)                     # ~2 k records per timed window
    states0, fwd = burst_input(kind, S, T, W, H, dev)
    per_call, chunks = burst_chunks(S, T, n)
    srv_states = states0.clone()
    recs = sender_records(W, H, fwd, srv_states)       # per chunk (records, counts, escapes, positions)
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
    times = time_legs(table, rounds, passes * B, before=restorer(states, states0, cores, states0.cpu().numpy(), "cores_client"))
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
    fig = report(out, times, "_us_per_record")
    out["multi_ticks_over_burst_apply"] = ratio(fig, "multi_ticks", "burst_apply")
    out["cores_client_over_burst_apply"] = ratio(fig, "cores_client", "burst_apply")
    for c in [client, ticks] + cores:
        c.close()
    return out


def run_activity(W, H, rounds, S, T, kind, cell=16):
    """The activity leg for one (S, T) and one input -> its dictionary."""
    import numpy as np
    from cudavideostream_amd import CUDACore, activity_cells
    dev = torch.device("cuda", 0)
    B = S * T
    passes = 2 * max(1, 1024 // B)                     # ~2 k records per timed window
    states0, fwd = burst_input(kind, S, T, W, H, dev)
    recs, counts, escapes, _ = one_call(sender_records(W, H, fwd, states0.clone()))
    del fwd
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

    times = time_legs({"activity": leg_activity, "burst_apply": leg_apply}, rounds, passes * B)
    # every counted entry is in the grids, and every stream's count is its records'
    summ = d_sum.cpu().numpy().view(np.uint32).reshape(S, 8)
    per_stream = counts.astype(np.int64).reshape(S, T).sum(axis=1)
    assert (summ[:, 0] == per_stream).all()
    assert (d_cells.cpu().numpy().view(np.uint32).astype(np.int64).reshape(S, ncells).sum(axis=1) == per_stream).all()
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "cell": cell, "cells_per_stream": ncells,
           "changed_bytes_per_record": round(int(counts.sum()) / B, 1), "active_cells_per_stream": round(float(summ[:, 5].mean()), 1)}
    fig = report(out, times, "_us_per_record")
    out["activity_over_burst_apply"], out["no_slower_than_burst_apply"] = versus(fig, "activity", "burst_apply")
    core.close()
    return out


def run_check(W, H, rounds, S, T, kind):
    """The check leg for one (S, T) and one input -> its dictionary."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_check_host
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    passes = 2 * max(1, 1024 // B)                     # ~2 k records per timed window
    states0, fwd = burst_input(kind, S, T, W, H, dev)
    recs, counts, escapes, pos = one_call(sender_records(W, H, fwd, states0.clone()))
    del fwd
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

    times = time_legs({"check": leg_check, "burst_apply": leg_apply}, rounds, passes * B)
    # a sender's records are clean, and the device's verdicts are the host's
    got = d_verdicts.cpu().numpy().view(np.uint32).reshape(B, 4)
    assert not got[:, 0].any() and (got[:, 1] == escapes).all() and (got[:, 2] == counts).all()
    assert np.array_equal(got, cwire_check_host(recs.cpu().numpy(), counts, escapes, n))
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "changed_bytes_per_record": round(int(counts.sum()) / B, 1),
           "record_bytes_per_record": round(int(pos[B]) / B, 1)}
    fig = report(out, times, "_us_per_record")
    out["check_over_burst_apply"], out["no_slower_than_burst_apply"] = versus(fig, "check", "burst_apply")
    core.close()
    return out


def run_refresh(W, H, rounds, S):
    """The refresh leg for one S -> its dictionary.  All legs on one core's own stream, alternating within every round; the diff
    leg has its own copy of the states per pass, restored outside the window (it is the only leg that writes states it reads)."""
    from cudavideostream_amd import CUDACore, cwire_bytes_max, state_tiles
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    tiles = state_tiles(n)
    mask_words = (tiles + 31) // 32
    passes = max(2, min(16, 128 // S))
    sender, fwd = burst_input("webcam", S, 1, W, H, dev)   # stream s: webcam frame s, and the tick s -> s + 1 for the diff leg
    frames = fwd[:, 0].clone()
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
        selected[name] = mask_bits(d_mask)
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

    def before(name):
        if name == "diff":
            work.copy_(sender.unsqueeze(0).expand(passes, S, n))

    def after(name):
        if name.startswith("refresh"):
            rec_bytes[name] = int(d_pos[S].item())

    table = {"digest": leg_digest, "digest_skewed": leg_digest_skewed, "refresh_1pct": leg_refresh(peers["1pct"]), "refresh_10pct": leg_refresh(peers["10pct"]),
             "refresh_all": leg_refresh(None), "clear_10pct": leg_clear, "diff": leg_diff}
    times = time_legs(table, rounds, passes * S, before=before, after=after)
    out = {"streams": S, "passes": passes, "tiles": tiles, "state_bytes": n}
    fig = report(out, times, "_us_per_stream", spread=True)
    for name in ("1pct", "10pct"):
        out["refresh_" + name + "_tiles_per_stream"] = selected[name] // S
    for name, b in rec_bytes.items():
        out[name + "_bytes_per_stream"] = round(b / S, 1)
    out["digest_over_diff"], out["digest_no_slower_than_diff"] = versus(fig, "digest", "diff")
    core.close()
    return out


def one_tick(W, H, S, core, d_mask, dev):
    """One tick of every input for the wall and thumb legs -> kind -> (states before, states after, records, counts, escapes,
    the tick's tile mask from mi355_cwire_touched_tiles_batch on `core`, tiles in it)."""
    ticks = {}
    for kind in KINDS:
        before, fwd = burst_input(kind, S, 1, W, H, dev)
        after = before.clone()
        recs, counts, escapes, _ = one_call(sender_records(W, H, fwd, after))
        d_kind_mask = torch.zeros_like(d_mask)
        core.cwire_touched_tiles_batch(recs, counts, escapes, S, 1, d_kind_mask)
        core.synchronize()
        ticks[kind] = (before, after, recs, counts, escapes, d_kind_mask, mask_bits(d_kind_mask))
    return ticks


def run_wall(W, H, rounds, S, scales=(2, 4, 8)):
    """The wall leg for one S -> its dictionary.  All legs on one core's own stream, alternating within every round."""
    import numpy as np
    from cudavideostream_amd import CUDACore, state_tiles, wall_thumb_size
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    tiles = state_tiles(n)
    mask_words = (tiles + 31) // 32
    passes = max(2, min(16, 128 // S))
    cols = int(np.ceil(np.sqrt(S)))
    d_mask = torch.zeros(S * mask_words, dtype=torch.int32, device=dev)
    d_dig = torch.zeros(S * tiles * 2, dtype=torch.int32, device=dev)
    core = CUDACore(W, H, max_batch=S)
    ticks = one_tick(W, H, S, core, d_mask, dev)        # the legs show the states after the tick
    aligned = ticks["webcam"][1]
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
        _, states, recs, counts, escapes, _, _ = ticks[kind]

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
    times = time_legs(table, rounds, passes * S)
    out = {"streams": S, "passes": passes, "tiles": tiles, "state_bytes": n, "columns": cols,
           "touched_tiles_per_stream": {kind: round(ticks[kind][6] / S, 1) for kind in ticks}}
    fig = report(out, times, "_us_per_stream", spread=True)
    out["masked_local_over_full"] = {f"k{k}": ratio(fig, f"masked_local_k{k}", f"full_k{k}") for k in scales}
    out["masked_local_cheaper_than_full"] = all(cheaper(fig, f"masked_local_k{k}", f"full_k{k}") for k in scales)
    out["full_k8_over_digest"], out["full_k8_no_slower_than_digest"] = versus(fig, "full_k8", "digest")
    core.close()
    return out


def run_thumb(W, H, rounds, S, scales=(2, 4, 8)):
    """The thumb leg for one S -> its dictionary.  Every leg alternates between the states before and after ONE tick (A, B, A, ..)
    with the tick's tile mask, so every pass finds the held thumbnails one tick behind and does a tick's work; the route's
    thumbnail-core states follow in the same way.  All legs alternate within every round."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, state_tiles, wall_thumb_size
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    mask_words = (state_tiles(n) + 31) // 32
    passes = 2 * max(1, min(8, 64 // S))
    d_mask = torch.zeros(S * mask_words, dtype=torch.int32, device=dev)
    core = CUDACore(W, H, max_batch=S)
    ticks = one_tick(W, H, S, core, d_mask, dev)
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
    for kind in KINDS:
        A, B, recs, counts, escapes, kmask, _ = ticks[kind]
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
    times = time_legs(table, rounds, passes * S)
    out = {"streams": S, "passes": passes, "tiles": state_tiles(n), "state_bytes": n, "records_equal_to_the_route": checked,
           "touched_tiles_per_stream": {kind: round(ticks[kind][6] / S, 1) for kind in ticks}}
    fig = report(out, times, "_us_per_stream", spread=True)
    points = [(kind, k) for kind in ticks for k in scales]
    out["touched_plus_call_over_route"] = {f"{kind}_k{k}": ratio(fig, f"touched_plus_call_{kind}_k{k}", f"route_{kind}_k{k}")
                                           for kind, k in points}
    out["touched_plus_call_no_slower_than_route"] = all(versus(fig, f"touched_plus_call_{kind}_k{k}", f"route_{kind}_k{k}")[1]
                                                        for kind, k in points)
    out["call_local_over_nullmask"] = {f"k{k}": ratio(fig, f"call_local_k{k}", f"call_nullmask_local_k{k}") for k in scales}
    out["call_local_cheaper_than_nullmask"] = all(cheaper(fig, f"call_local_k{k}", f"call_nullmask_local_k{k}") for k in scales)
    for g in geo.values():
        g["small"].close()
    core.close()
    return out


def run_coalesce(W, H, rounds, S, T, kind):
    """The coalesce leg for one (S, T) and one input -> its dictionary.  coalesce: mi355_cwire_coalesce_cwire_batch on the
    burst's records, nothing else.  state_route: what a relay did before -- mi355_apply_multi_stream_cwire_batch onto states it
    holds, then mi355_diff_multi_cwire_batch of a threshold-0 core between the new states and the saved ones (which the call
    advances), both on one core, no synchronisation in between."""
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n, B = 3 * W * H, S * T
    passes = 2 * max(1, 1024 // B)                     # ~2 k records per timed window
    states0, fwd = burst_input(kind, S, T, W, H, dev)
    per_call, chunks = burst_chunks(S, T, n)
    srv_states = states0.clone()
    recs = sender_records(W, H, fwd, srv_states)       # per chunk (records, counts, escapes, positions)
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

    def before(name=None):
        states.copy_(states0)
        saved.copy_(states0)

    times = time_legs({"coalesce": leg_coalesce, "state_route": leg_route}, rounds, passes * B, before=before)
    # one burst from the base states: both ways make the same records, and they lead to the sender's states
    before()
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
    in_bytes = sum(int(r[3][-1]) for r in recs)
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "calls_per_burst": len(chunks),
           "input_entries_per_stream": round(sum(int(r[1].sum()) for r in recs) / S, 1), "output_entries_per_stream": round(out_entries / S, 1),
           "input_bytes_per_stream": round(in_bytes / S, 1), "output_bytes_per_stream": round(out_bytes / S, 1),
           "output_over_input_bytes": round(out_bytes / in_bytes, 4)}
    fig = report(out, times, "_us_per_input_record", spread=True)
    out["state_route_over_coalesce"] = ratio(fig, "state_route", "coalesce")
    relay.close()
    route.close()
    return out


def run_crop(W, H, rounds, S, kind):
    """The crop leg for one S and one input, T = 1 -> its dictionary.  coalesce: mi355_cwire_coalesce_cwire_batch on the records of
    one tick, the nearest route without the crop call.  crop_quarter / crop_full: mi355_cwire_crop_cwire_batch on the same records
    with the rectangle (W/4, H/4, W/2, H/2) for every stream, and with the full frame.  All on one core's own stream, alternating
    within every round."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    dev = torch.device("cuda", 0)
    n, T = 3 * W * H, 1
    passes = 2 * max(1, 1024 // S)                     # ~2 k records per timed window
    states0, fwd = burst_input(kind, S, T, W, H, dev)
    per_call, chunks = burst_chunks(S, T, n)
    recs = sender_records(W, H, fwd, states0.clone())   # per chunk (records, counts, escapes, positions)
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

    times = time_legs({"coalesce": leg_coalesce, "crop_quarter": leg_crop(quarter), "crop_full": leg_crop(full)}, rounds, passes * S)
    # the full-frame crop of one record per stream is the coalescer's output (and the input); the quarter holds fewer entries
    in_entries = quarter_entries = quarter_bytes = 0
    for (s0, ns), r in zip(chunks, recs):
        relay.cwire_coalesce_cwire_batch(r[0], r[1], r[2], ns, T, d_coff, d_cpos, d_cout, ocap)
        relay.cwire_crop_cwire_batch(r[0], r[1], r[2], ns, T, full, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()
        nbytes = int(d_cpos[ns].item())
        assert nbytes == int(r[3][-1]) and torch.equal(d_opos[:ns + 1], d_cpos[:ns + 1]) and torch.equal(d_out[:nbytes], d_cout[:nbytes])
        assert torch.equal(d_out[:nbytes], r[0])
        in_entries += int(d_coff[ns].item())
        relay.cwire_crop_cwire_batch(r[0], r[1], r[2], ns, T, quarter, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()
        quarter_entries += int(d_ooff[ns].item())
        quarter_bytes += int(d_opos[ns].item())
    assert quarter_entries <= in_entries
    in_bytes = sum(int(r[3][-1]) for r in recs)
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "calls_per_tick": len(chunks),
           "rectangle": [int(v) for v in quarter[0]],
           "input_entries_per_stream": round(in_entries / S, 1), "quarter_entries_per_stream": round(quarter_entries / S, 1),
           "input_bytes_per_stream": round(in_bytes / S, 1), "quarter_bytes_per_stream": round(quarter_bytes / S, 1)}
    fig = report(out, times, "_us_per_stream", spread=True, as_printed=True)
    # the expectation: the quarter no slower than the coalescer by more than the rounds' spread (of either leg)
    out["crop_quarter_over_coalesce"], quarter_ok = versus(fig, "crop_quarter", "coalesce")
    out["crop_full_over_coalesce"] = ratio(fig, "crop_full", "coalesce")
    out["quarter_no_slower_than_coalesce"] = quarter_ok
    out["full_minus_coalesce_us_per_call"] = round((fig["crop_full"][0] - fig["coalesce"][0]) * S / len(chunks), 3)
    relay.close()
    return out


def run_split(W, H, rounds, S, kind, limits=(1400, 8972)):
    """The split leg for one S and one input, T = 1 -> its dictionary.  coalesce: mi355_cwire_coalesce_cwire_batch on the records of
    one tick (with T = 1 it gives the input back): the nearest call of the family that reads every record once and writes it once.
    split_M: mi355_cwire_split_cwire_batch on the same records at max_bytes = M.  All on one core's own stream, alternating within
    every round.  Before anything is timed the pieces are compared with mi355_cwire_split_host."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, cwire_split_bytes_max, cwire_split_host, cwire_split_pieces_max
    dev = torch.device("cuda", 0)
    n, T = 3 * W * H, 1
    passes = 2 * max(1, 1024 // S)                     # ~2 k records per timed window
    states0, fwd = burst_input(kind, S, T, W, H, dev)
    per_call, chunks = burst_chunks(S, T, n)
    recs = sender_records(W, H, fwd, states0.clone())   # per chunk (records, counts, escapes, positions)
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
    in_bytes = sum(int(r[3][-1]) for r in recs)
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
    times = time_legs(table, rounds, passes * S)
    fig = report(out, times, "_us_per_record", spread=True, as_printed=True)
    for M in limits:
        # the expectation: no slower than the coalescer by more than the rounds' spread (of either leg)
        out[f"split_{M}_over_coalesce"], out[f"split_{M}_no_slower_than_coalesce"] = versus(fig, f"split_{M}", "coalesce")
    relay.close()
    return out


def key_frame_records(W, H, states):
    """The key frames of states [S][n], as a sender's mi355_refresh_cwire_batch without digests makes them (every tile) -> one
    chunk (records, counts, escapes, positions) as sender_records gives them."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max
    S, n = states.shape
    cap = cwire_bytes_max(n, S)
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=states.device)
    d_pos = torch.zeros(S + 1, dtype=torch.int64, device=states.device)
    d_cw = torch.empty(cap, dtype=torch.uint8, device=states.device)
    with CUDACore(W, H, max_batch=S) as server:
        d_mask = torch.zeros(S * ((n + 4095) // 4096 + 31) // 32 + S, dtype=torch.int32, device=states.device)
        torch.cuda.synchronize()
        server.refresh_cwire_batch(states, S, None, d_mask, d_off, d_pos, d_cw, cap)
        server.synchronize()
    pos = d_pos.cpu().numpy().astype(np.int64)
    counts = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)).astype(np.uint32)
    escapes = ((np.diff(pos) - 8 - 2 * ((counts.astype(np.int64) + 3) & ~3)) // 4).astype(np.uint32)
    return [(d_cw[:int(pos[S])].clone(), counts, escapes, pos)]


def run_runs(W, H, rounds, S, kind):
    """The runs leg for one S and one input, T = 1 -> its dictionary.  coalesce: mi355_cwire_coalesce_cwire_batch on the records of
    one tick (with T = 1 it gives the input back), the comparator of the split leg.  encode: mi355_cwire_runs_encode_batch under
    MI355_RUNS_WHERE_SMALLER on the same records; decode: mi355_cwire_runs_decode_batch on what it wrote.  Inputs: the webcam-like
    tick, the local tick, and `keyframe`, mi355_refresh_cwire_batch of every tile of the webcam-like states.  All on one core's own
    stream, alternating within every round.  Before anything is timed both outputs are compared with the host forms."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, cwire_runs_bytes_max, cwire_runs_decode_host, cwire_runs_encode_host
    dev = torch.device("cuda", 0)
    n, T = 3 * W * H, 1
    passes = 2 * max(1, 1024 // S)                     # ~2 k records per timed window
    states0, fwd = burst_input("webcam" if kind == "keyframe" else kind, S, T, W, H, dev)
    per_call, chunks = burst_chunks(S, T, n)
    assert len(chunks) == 1, "the leg runs in one call: max_batch * N < 2^32"
    recs = key_frame_records(W, H, states0) if kind == "keyframe" else sender_records(W, H, fwd, states0.clone())
    d_cw, counts, escapes, pos = one_call(recs)
    ocap = cwire_bytes_max(n, S)
    d_ooff = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_opos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_out = torch.empty(ocap, dtype=torch.uint8, device=dev)
    lcap = cwire_runs_bytes_max(n, S, lib.RUNS_WHERE_SMALLER)
    d_forms = torch.zeros(4 * S, dtype=torch.int32, device=dev)
    d_lpos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_link = torch.empty(lcap, dtype=torch.uint8, device=dev)
    d_fpos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_back = torch.empty(ocap, dtype=torch.uint8, device=dev)
    relay = CUDACore(W, H, max_batch=S)
    torch.cuda.synchronize()
    # both outputs are the host forms', and the decode is the input
    relay.cwire_runs_encode_batch(d_cw, counts, escapes, S, lib.RUNS_WHERE_SMALLER, d_forms, d_lpos, d_link, lcap)
    relay.synchronize()
    host = d_cw.cpu().numpy()
    wf, wp, wo = cwire_runs_encode_host(host, counts, escapes, n, lib.RUNS_WHERE_SMALLER, capacity_bytes=lcap)
    forms = d_forms.cpu().numpy().view(np.uint32).reshape(S, 4).copy()
    link_bytes = int(wp[-1])
    assert np.array_equal(forms, wf) and np.array_equal(d_lpos.cpu().numpy().view(np.uint64), wp)
    assert np.array_equal(d_link[:link_bytes].cpu().numpy(), wo[:link_bytes])
    relay.cwire_runs_decode_batch(d_link, forms, S, d_fpos, d_back, ocap)
    relay.synchronize()
    fp, back = cwire_runs_decode_host(wo[:link_bytes], wf, n)
    assert np.array_equal(d_fpos.cpu().numpy().view(np.uint64), fp) and int(fp[-1]) == host.size
    assert np.array_equal(d_back[:host.size].cpu().numpy(), host) and np.array_equal(back, host)

    def leg_coalesce():
        for _ in range(passes):
            relay.cwire_coalesce_cwire_batch(d_cw, counts, escapes, S, T, d_ooff, d_opos, d_out, ocap)
        relay.synchronize()

    def leg_encode():
        for _ in range(passes):
            relay.cwire_runs_encode_batch(d_cw, counts, escapes, S, lib.RUNS_WHERE_SMALLER, d_forms, d_lpos, d_link, lcap)
        relay.synchronize()

    def leg_decode():
        for _ in range(passes):
            relay.cwire_runs_decode_batch(d_link, forms, S, d_fpos, d_back, ocap)
        relay.synchronize()

    out = {"input": kind, "streams": S, "frames": T, "passes": passes,
           "input_entries_per_stream": round(int(counts.sum()) / S, 1), "runs_per_stream": round(int(wf[:, 3].sum()) / S, 1),
           "bytes_in_per_stream": round(host.size / S, 1), "bytes_out_per_stream": round(link_bytes / S, 1),
           "bytes_out_over_in": round(link_bytes / host.size, 4), "records_packed": int(wf[:, 0].sum()), "records": S}
    times = time_legs({"coalesce": leg_coalesce, "encode": leg_encode, "decode": leg_decode}, rounds, passes * S)
    fig = report(out, times, "_us_per_record", spread=True, as_printed=True)
    # the expectation: neither call slower than the coalescer by more than the rounds' spread (of either leg)
    for name in ("encode", "decode"):
        out[f"{name}_over_coalesce"], out[f"{name}_no_slower_than_coalesce"] = versus(fig, name, "coalesce")
    relay.close()
    return out


def run_fec(W, H, rounds, S, kind, M=1400, G=8):
    """The fec leg for one S and one input, T = 1 -> its dictionary.  split: mi355_cwire_split_cwire_batch at max_bytes = M on the
    records of one tick; fec_k1 / fec_k2: mi355_cwire_fec_batch with K = 1 / 2 parity blocks per group of G on the pieces that call
    left; repair_one / repair_two: mi355_cwire_fec_repair_batch with one job per stream, the first piece (the first two) of its
    first group lost.  All on one core's own stream, alternating within every round.  Before anything is timed the parity is
    compared with mi355_cwire_fec_host and the rebuilt pieces with the pieces."""
    import numpy as np
    from cudavideostream_amd import (CUDACore, cwire_fec_groups_max, cwire_fec_host, cwire_split_bytes_max, cwire_split_host,
                                     cwire_split_pieces_max, lib)
    dev = torch.device("cuda", 0)
    n, T = 3 * W * H, 1
    passes = 2 * max(1, 1024 // S)                     # ~2 k records per timed window
    states0, fwd = burst_input(kind, S, T, W, H, dev)   # run_split's input
    recs, counts, escapes, pos = one_call(sender_records(W, H, fwd, states0.clone()))
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
    times = time_legs(table, rounds, lambda name: passes * max(jobs[1][0] if name.startswith("repair") else S, 1))
    fig = report(out, {k: v for k, v in times.items() if not k.startswith("repair")}, "_us_per_record", spread=True, as_printed=True)
    report(out, {k: v for k, v in times.items() if k.startswith("repair")}, "_us_per_job", spread=True)
    out["fec_k1_over_split"] = ratio(fig, "fec_k1", "split")
    # the expectation: at K = 2 no slower than the split call that feeds it by more than the rounds' spread (of either leg)
    out["fec_k2_over_split"], out["fec_k2_no_slower_than_split"] = versus(fig, "fec_k2", "split")
    relay.close()
    return out


def run_mosaic(W, H, rounds, S, T, kind):
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
    states0, fwd = burst_input(kind, S, T, W, H, dev)
    recs, counts, escapes, pos = one_call(sender_records(W, H, fwd, states0.clone()))
    in_bytes = int(pos[B])
    del fwd
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

    times = time_legs({"mosaic": leg_mosaic, "state_route": leg_route}, rounds, passes * B)
    out = {"input": kind, "streams": S, "frames": T, "passes": passes, "grid": [C, R], "canvas": [cw, ch],
           "input_entries_per_record": round(float(counts.sum()) / B, 1), "input_bytes_per_record": round(in_bytes / B, 1),
           "canvas_entries": out_entries, "canvas_record_bytes": out_bytes, "route_record_equals_mosaic": equal}
    fig = report(out, times, "_us_per_record", spread=True, as_printed=True)
    out["mosaic_over_route"], out["mosaic_no_slower_than_route"] = versus(fig, "mosaic", "state_route")
    for c in (relay, route, canvas):
        c.close()
    return out


def run_budget(W, H, rounds, S):
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
    pre, fwd = burst_input("webcam", S, 1, W, H, dev)   # stream s: webcam frame s -> s + 1
    frames = fwd[:, 0].clone()
    post = pre.clone()
    recs, counts, escapes, pos = one_call(sender_records(W, H, fwd, post))
    cwcap = cwire_bytes_max(n, S)
    d_thr = torch.zeros(S, dtype=torch.int32, device=dev)
    d_ooff = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_opos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_out = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    d_roff, d_rpos, d_rcw = torch.zeros_like(d_ooff), torch.zeros_like(d_opos), torch.empty_like(d_out)
    core = CUDACore(W, H, max_batch=S)
    budgets = (counts // 2).astype(np.uint32)
    work = torch.empty(passes, S, n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def leg_budget():
        for p in range(passes):
            core.cwire_budget_cwire_batch(recs, counts, escapes, work[p], S, budgets, d_thr, d_ooff, d_opos, d_out, cwcap)
        core.synchronize()

    def leg_diff():
        for p in range(passes):
            core.diff_multi_cwire_batch(frames, work[p], S, d_roff, d_rpos, d_rcw, cwcap)
        core.synchronize()

    start = {"budget": post, "second_diff": pre}
    times = time_legs({"budget": leg_budget, "second_diff": leg_diff}, rounds, passes * S,
                      before=lambda name: work.copy_(start[name].unsqueeze(0).expand(passes, S, n)))
    kept = np.diff(d_ooff.cpu().numpy().view(np.uint32).astype(np.int64))
    thr = d_thr.cpu().numpy().view(np.uint32)
    assert (kept <= budgets).all() and (thr >= 20).all() and np.array_equal(d_rpos.cpu().numpy(), pos)
    out = {"streams": S, "passes": passes, "entries_per_stream": round(float(counts.mean()), 1),
           "kept_entries_per_stream": round(float(kept.mean()), 1), "record_bytes_per_stream": round(int(pos[S]) / S, 1),
           "kept_bytes_per_stream": round(int(d_opos[S].item()) / S, 1), "threshold_min": int(thr.min()), "threshold_max": int(thr.max())}
    fig = report(out, times, "_us_per_stream", spread=True)
    out["second_diff_over_budget"] = ratio(fig, "second_diff", "budget")
    core.close()
    return out


def run_despeckle(W, H, rounds, S, kind):
    """The despeckle leg for one S and one input -> its dictionary.  despeckle: mi355_cwire_despeckle_cwire_batch at need = 3 on
    the records of one tick, on the states as the tick left them.  budget: mi355_cwire_budget_cwire_batch on the same records with
    every stream's budget at half of its count -- the nearest sibling: the same directory, three tile passes, a state tile read.
    Both on one core's own stream, alternating within every round; every pass of a timed window has its own copy of the states,
    restored outside the window.  On the webcam-like input the entries and bytes out are compared with the host form's."""
    import numpy as np
    from cudavideostream_amd import CUDACore, cwire_bytes_max, cwire_despeckle_host, lib as _lib
    dev = torch.device("cuda", 0)
    n = 3 * W * H
    passes = max(2, min(16, 128 // S))
    pre, fwd = burst_input(kind, S, 1, W, H, dev)
    post = pre.clone()
    recs, counts, escapes, pos = one_call(sender_records(W, H, fwd, post))
    del fwd
    cwcap = cwire_bytes_max(n, S)
    d_drop = torch.zeros(S, dtype=torch.int32, device=dev)
    d_ooff = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    d_opos = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_out = torch.empty(cwcap, dtype=torch.uint8, device=dev)
    d_thr, d_boff, d_bpos, d_bout = torch.zeros_like(d_drop), torch.zeros_like(d_ooff), torch.zeros_like(d_opos), torch.empty_like(d_out)
    core = CUDACore(W, H, max_batch=S)
    core.prepare(_lib.PREPARE_DESPECKLE)
    need = np.full(S, 3, np.uint32)
    budgets = (counts // 2).astype(np.uint32)
    work = torch.empty(passes, S, n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def leg_despeckle():
        for p in range(passes):
            core.cwire_despeckle_cwire_batch(recs, counts, escapes, work[p], S, need, d_drop, d_ooff, d_opos, d_out, cwcap)
        core.synchronize()

    def leg_budget():
        for p in range(passes):
            core.cwire_budget_cwire_batch(recs, counts, escapes, work[p], S, budgets, d_thr, d_boff, d_bpos, d_bout, cwcap)
        core.synchronize()

    times = time_legs({"despeckle": leg_despeckle, "budget": leg_budget}, rounds, passes * S,
                      before=lambda name: work.copy_(post.unsqueeze(0).expand(passes, S, n)))
    work[0].copy_(post)                    # once more outside the windows: the states the figures below are read from
    torch.cuda.synchronize()
    core.cwire_despeckle_cwire_batch(recs, counts, escapes, work[0], S, need, d_drop, d_ooff, d_opos, d_out, cwcap)
    core.synchronize()
    kept = np.diff(d_ooff.cpu().numpy().view(np.uint32).astype(np.int64))
    dropped = d_drop.cpu().numpy().view(np.uint32).astype(np.int64)
    out_bytes = int(d_opos[S].item())
    assert np.array_equal(kept + dropped, counts.astype(np.int64))
    out = {"input": kind, "streams": S, "passes": passes, "need": 3, "entries_in": int(counts.sum()), "entries_out": int(kept.sum()),
           "bytes_in": int(pos[S]), "bytes_out": out_bytes, "budget_entries_out": int(np.diff(d_boff.cpu().numpy().view(np.uint32).astype(np.int64)).sum()),
           "budget_bytes_out": int(d_bpos[S].item()), "bitmap_pass_bytes_per_stream": n // 24}
    if kind == "webcam":   # the host form on the same records: entries, bytes and the records themselves
        states = post.cpu().numpy()
        h_drop, h_off, h_pos, h_out = cwire_despeckle_host(W, H, recs.cpu().numpy()[:int(pos[S])], counts, escapes, states, need)
        out["equals_host_form"] = bool(np.array_equal(np.diff(h_off.astype(np.int64)), kept) and int(h_pos[S]) == out_bytes and
                                       np.array_equal(h_out[:out_bytes], d_out[:out_bytes].cpu().numpy()) and
                                       np.array_equal(states, work[0].cpu().numpy()))
        assert out["equals_host_form"], "the call's records differ from mi355_cwire_despeckle_host's"
    fig = report(out, times, "_us_per_stream", spread=True)
    # the expectation, judged without the allowance for the N/24 bitmap pass (bitmap_pass_bytes_per_stream says how large it is)
    out["despeckle_over_budget"], out["despeckle_no_slower_than_budget"] = versus(fig, "despeckle", "budget")
    core.close()
    return out


# ---- the command line: one entry per --legs value that runs alone
def ints(text):
    return [int(v) for v in text.split(",")]


def grid(**axes):
    """Every combination of the axes' values, the first axis outermost -> the runners' keyword arguments."""
    return [dict(zip(axes, p)) for p in itertools.product(*axes.values())]


def activity_points(a):
    """S of --streams with T = 1, and S = 16 with T = 16, on both inputs."""
    return [dict(S=S, T=T, kind=kind) for S, T in [(S, 1) for S in ints(a.streams)] + [(16, 16)] for kind in KINDS]


# run: the leg's runner, called with (W, H, rounds, **point); points: the points it runs at, from the arguments; bench: the name in
# its JSON line, whose list of the points' dictionaries stands under the leg's own name; input, steps: further fields of that line;
# quiet: no progress line on stderr; verdict: per part (the suffix of the points' booleans, the text if all hold, the text if not)
LEGS = {
    "client": dict(run=run_client, points=lambda a: grid(S=ints(a.streams), K=[a.steps]), bench="multi_client", input=True, steps=True,
                   quiet=True),
    "burst": dict(run=run_burst, points=lambda a: grid(S=ints(a.streams), T=ints(a.frames)), bench="multi_stream", input=True, quiet=True),
    "burst_client": dict(run=run_burst_client, points=lambda a: grid(S=ints(a.streams), T=ints(a.frames), kind=KINDS),
                         bench="multi_stream_client", quiet=True),
    "coalesce": dict(run=run_coalesce, points=lambda a: grid(S=ints(a.streams), T=ints(a.frames), kind=KINDS), bench="multi_coalesce"),
    "crop": dict(run=run_crop, points=lambda a: grid(S=ints(a.streams), kind=KINDS), bench="multi_crop"),
    "split": dict(run=run_split, points=lambda a: grid(S=ints(a.streams), kind=KINDS), bench="multi_split",
                  verdict=[("_no_slower_than_coalesce", "no slower than coalesce at every point", "slower than coalesce at some point")]),
    "fec": dict(run=run_fec, points=lambda a: grid(S=ints(a.streams), kind=KINDS), bench="multi_fec",
                verdict=[("fec_k2_no_slower_than_split", "parity at K = 2 no slower than split at every point",
                          "parity at K = 2 slower than split at some point")]),
    "runs": dict(run=run_runs, points=lambda a: grid(S=ints(a.streams), kind=KINDS + ("keyframe",)), bench="multi_runs",
                 verdict=[("encode_no_slower_than_coalesce", "encode no slower than coalesce at every point", "encode slower than coalesce at some point"),
                          ("decode_no_slower_than_coalesce", "decode no slower than coalesce at every point", "decode slower than coalesce at some point")]),
    "mosaic": dict(run=run_mosaic, points=lambda a: grid(S=ints(a.streams), T=(1, 16), kind=KINDS), bench="multi_mosaic"),
    "budget": dict(run=run_budget, points=lambda a: grid(S=ints(a.streams)), bench="multi_budget", input=True),
    "despeckle": dict(run=run_despeckle, points=lambda a: grid(S=ints(a.streams), kind=KINDS), bench="multi_despeckle",
                      verdict=[("despeckle_no_slower_than_budget", "despeckle no slower than budget at every point",
                                "despeckle slower than budget at some point")]),
    "activity": dict(run=run_activity, points=activity_points, bench="multi_activity",
                     verdict=[("no_slower_than_burst_apply", "no slower than burst_apply at every point", "slower than burst_apply at some point")]),
    "check": dict(run=run_check, points=activity_points, bench="multi_check",
                  verdict=[("no_slower_than_burst_apply", "no slower than burst_apply at every point", "slower than burst_apply at some point")]),
    "refresh": dict(run=run_refresh, points=lambda a: grid(S=ints(a.streams)), bench="multi_refresh",
                    verdict=[("digest_no_slower_than_diff", "digest no slower than diff at every S", "digest slower than diff at some S")]),
    "wall": dict(run=run_wall, points=lambda a: grid(S=ints(a.streams)), bench="multi_wall",
                 verdict=[("masked_local_cheaper_than_full", "masked update on the moving block cheaper than the full compose at every k and S",
                           "masked update on the moving block not cheaper than the full compose at some k or S"),
                          ("full_k8_no_slower_than_digest", "full compose at k = 8 no slower than digest at every S",
                           "full compose at k = 8 slower than digest at some S")]),
    "thumb": dict(run=run_thumb, points=lambda a: grid(S=ints(a.streams)), bench="multi_thumb",
                  verdict=[("touched_plus_call_no_slower_than_route", "touched tiles plus the call no slower than the wall-and-diff route at every point",
                            "touched tiles plus the call slower than the wall-and-diff route at some point"),
                           ("call_local_cheaper_than_nullmask", "the call with the moving block's mask cheaper than without a mask at every k and S",
                            "the call with the moving block's mask not cheaper than without a mask at some k or S")]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--streams", default="8,64,256")
    ap.add_argument("--steps", type=int, default=8, help="K: webcam frames a stream walks through")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="multi,cores_loop,pairs",
                    help="of multi, cores_loop, pairs, write_probe" + "".join(f"; or {name} alone" for name in LEGS))
    ap.add_argument("--frames", default="4,16,64", help="burst, burst_client and coalesce legs: T, frames per stream and call")
    a = ap.parse_args()
    have = load_library()
    W, H = (int(v) for v in a.size.split("x"))
    if a.legs not in LEGS:
        for S in ints(a.streams):
            run(W, H, S, a.steps, a.rounds, set(a.legs.split(",")), have)
            torch.cuda.empty_cache()
        return
    leg = LEGS[a.legs]
    per = []
    for point in leg["points"](a):
        per.append(leg["run"](W, H, a.rounds, **point))
        if not leg.get("quiet"):
            where = " ".join(str(v) if k == "kind" else f"{k}={v}" for k, v in point.items())
            print(f"{a.legs} {where}: done", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    line = {"bench": leg["bench"], "size": f"{W}x{H}"}
    if leg.get("input"):
        line["input"] = "synth.webcam_stream"
    line["rounds"] = a.rounds
    if leg.get("steps"):
        line["steps"] = a.steps
    line[a.legs] = per
    if "verdict" in leg:
        line["verdict"] = "; ".join(ok if all(v for p in per for k, v in p.items() if k.endswith(flag)) else bad
                                    for flag, ok, bad in leg["verdict"])
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

"""-m gpu: mi355_diff_stream_cwire_batch, the frame stream straight into the compact wire format (include/mi355diff.h),
against the numpy statement of the format (tests/cwire_spec.py) on the oracle's stream, and against the two-call path
(diff_stream_batch + cwire_encode_batch), byte for byte."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib, synth
from oracle import pyoracle as po
from gpu_util import DEV, CUDACore, to_dev

pytestmark = pytest.mark.gpu

GUARD = 0x5C
ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))


def direct(core, d_frames, T, capacity=None):
    """One direct call into guarded buffers -> (offsets uint32[T+1], frame_pos uint64[T+1], bytes of the whole buffer)."""
    cap = cwire_bytes_max(core.total, T) if capacity is None else capacity
    d_off = torch.full((T + 1,), -5, dtype=torch.int32, device=DEV)
    d_pos = torch.full((T + 1,), -3, dtype=torch.int64, device=DEV)
    d_cw = torch.full((cap + 256,), GUARD, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()   # (the new entry point is not in gpu_util's synced list)
    core.diff_stream_cwire_batch(d_frames, T, d_off, d_pos, d_cw, cap)
    core.synchronize()
    return d_off.cpu().numpy().view(np.uint32), d_pos.cpu().numpy().view(np.uint64), d_cw.cpu().numpy()


def two_call(core, d_frames, T):
    """The reference path of the library: diff_stream_batch, then cwire_encode_batch -> (offsets, frame_pos, bytes)."""
    n = core.total
    d_off = torch.zeros(T + 1, dtype=torch.int32, device=DEV)
    d_xs = torch.empty(max(T * n, 1), dtype=torch.int32, device=DEV)
    d_df = torch.empty(max(T * n, 1), dtype=torch.uint8, device=DEV)
    cap = cwire_bytes_max(n, T)
    d_pos = torch.zeros(T + 1, dtype=torch.int64, device=DEV)
    d_cw = torch.empty(max(cap, 1), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    core.diff_stream_batch(d_frames, T, d_off, d_xs, d_df, T * n)
    core.cwire_encode_batch(d_off, d_xs, d_df, T * n, T, d_pos, d_cw, cap)
    core.synchronize()
    pos = d_pos.cpu().numpy().view(np.uint64)
    return d_off.cpu().numpy().view(np.uint32), pos, d_cw[:int(pos[-1])].cpu().numpy()


def check_full(off, pos, got, want_off, want, wpos):
    assert np.array_equal(off, want_off)
    assert np.array_equal(pos, wpos)
    assert np.array_equal(got[:want.size], want)
    assert (got[want.size:] == GUARD).all()


def check_oracle(core, frames, state, thr=20, T=None):
    """Direct call on frames (numpy) vs the oracle continuing from `state`; returns the oracle's state after them."""
    T = frames.shape[0] if T is None else T
    eo, exs, edf, est = po.diff_stream(frames, state, thr)
    want, wpos = spec.encode(eo, exs, edf)
    off, pos, got = direct(core, to_dev(frames), T)
    check_full(off, pos, got, eo, want, wpos)
    return est, want


def cumulative_flips(base, positions):
    """Frame t = frame t - 1 with the bytes at positions[t] flipped by 0x80: every flip is one entry of frame t."""
    frames, cur = [], base.copy()
    for p in positions:
        cur = cur.copy()
        cur[np.asarray(p, np.int64)] ^= 0x80
        frames.append(cur)
    return np.stack(frames)


@pytest.mark.parametrize("thr", [0, 20, 255])
@pytest.mark.parametrize("w,h,T", [(1, 1, 4), (33, 7, 9), (211, 3, 17), (64, 48, 6), (1920, 1080, 8), (3840, 2160, 3)])
def test_direct_equals_spec_and_two_call_path(w, h, T, thr):
    base, frames = synth.webcam_stream(T, w, h, seed=5)
    frames = frames.copy()
    frames[T // 2] = frames[T // 2 - 1] if T > 1 else frames[0]   # a frame with nothing to send
    d_frames = to_dev(frames)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T, threshold=thr) as core, \
            CUDACore(w, h, sample_mat_data=base, max_batch=T, threshold=thr) as ref:
        off, pos, got = direct(core, d_frames, T)
        r_off, r_pos, r_buf = two_call(ref, d_frames, T)
        check_full(off, pos, got, r_off, r_buf, r_pos)
        assert np.array_equal(core.get_state(), ref.get_state())
        if w * h < 10 ** 6:
            eo, exs, edf, est = po.diff_stream(frames, base, thr)
            want, wpos = spec.encode(eo, exs, edf)
            check_full(off, pos, got, eo, want, wpos)
            assert np.array_equal(core.get_state(), est)


def _regime(name, n, T):
    base = synth.refrand_frame(n, 100)
    if name == "S0":
        return base, np.stack([synth.refrand_frame(n, 1 + t) for t in range(T)])
    if name == "S2":
        return base, np.stack([base] * T)
    if name == "S3":   # every byte of every frame changes: every tile full
        return base, np.stack([base ^ np.uint8(0x80 * ((t + 1) & 1)) for t in range(T)])
    if name == "S4":   # isolated bytes far apart: escapes
        frames = np.stack([base] * T)
        for t in range(T):
            frames[t, np.arange(t, n, 997 + 131 * t)] ^= 0x80
        return base, frames
    # S1 with an all-changed frame and a still frame in the middle
    b, fr = synth.webcam_stream(T, n // 3 // 180, 180, seed=8)
    fr = fr.copy()
    fr[1] = fr[0] ^ np.uint8(0x80)
    fr[2] = fr[1]
    return b, fr


@pytest.mark.parametrize("regime", ["S0", "S1", "S2", "S3", "S4"])
def test_direct_regimes(regime):
    w, h, T = 320, 180, 5
    n = 3 * w * h
    base, frames = _regime(regime, n, T)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        est, want = check_oracle(core, frames, base)
        assert np.array_equal(core.get_state(), est)
        counts, escapes = spec.headers(want, T)
        if regime == "S2":
            assert counts.sum() == 0 and want.size == 8 * T
        if regime == "S3":
            assert (counts == n).all()
        if regime == "S4":
            assert escapes.min() > 0


def test_direct_gap_boundaries():
    """Single changed bytes with gaps of exactly 254, 255 and 256 inside a tile, across tiles (1 KiB) and across items
    (16 tiles), first indices of 254, 255 and 256, and a lane with several bytes before and after a long gap."""
    w, h = 128, 128                      # 48 KiB: three items of 16 tiles
    n = 3 * w * h
    base = (np.arange(n) % 97).astype(np.uint8)
    positions = [[254], [255], [256], [0, 100]]
    for g in (254, 255, 256):
        positions.append([10, 10 + g + 1, 10 + 2 * (g + 1)])                 # inside tile 0
        positions.append([1024 - 100, 1024 - 100 + g + 1])                    # across tiles 0 / 1
        positions.append([16384 - 60, 16384 - 60 + g + 1, 32768 + 5])         # across items 0 / 1, then 1 / 2
        positions.append([300, 301, 305, 305 + g + 1, 305 + g + 2])           # multi-byte lanes either side
        positions.append([16384 + 3, 16384 + 3 + g + 1, n - 1])
    positions.append([])                                                      # nothing changes
    positions.append([n - 1])
    frames = cumulative_flips(base, positions)
    T = frames.shape[0]
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        est, want = check_oracle(core, frames, base)
        assert np.array_equal(core.get_state(), est)
        counts, escapes = spec.headers(want, T)
        assert list(counts[:3]) == [1, 1, 1] and list(escapes[:3]) == [0, 1, 1]


def test_direct_capacity_skips_whole_frames_and_keeps_the_state():
    w, h, T = 64, 48, 6
    base, frames = synth.webcam_stream(2 * T, w, h, seed=9)
    eo, exs, edf, est = po.diff_stream(frames[:T], base)
    want, wpos = spec.encode(eo, exs, edf)
    big = int(np.argmax(np.diff(wpos.astype(np.int64))))
    caps = [0, 7, 8, 9, int(wpos[3]) - 1, int(wpos[3]), int(wpos[3]) + 1, int(wpos[big + 1]) - 1, int(wpos[T]) - 1]
    for cap in caps:
        with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
            off, pos, got = direct(core, to_dev(frames[:T]), T, capacity=cap)
            assert np.array_equal(off, eo) and np.array_equal(pos, wpos), cap   # exact regardless
            fit = int(wpos[np.searchsorted(wpos, cap, side="right") - 1])        # frames are written as a prefix
            assert np.array_equal(got[:fit], want[:fit]), cap
            assert (got[fit:] == GUARD).all(), cap
            assert np.array_equal(core.get_state(), est), cap
            check_oracle(core, frames[T:], est)                                 # the next batch goes on from the state


def test_direct_consecutive_batches_pipelined():
    """Own-stream batches back to back with no synchronisation in between: sparse, a dense batch after sparse ones, sparse
    again.  640x360 has 675 tiles: every pipelined pack is split."""
    w, h, T, K = 640, 360, 6, 5
    n = 3 * w * h
    base, fr = synth.webcam_stream(K * T, w, h, seed=41)
    batches = [fr[k * T:(k + 1) * T].copy() for k in range(K)]
    batches[2] = np.stack([synth.refrand_frame(n, 300 + t) for t in range(T)])   # dense after sparse
    cap = cwire_bytes_max(n, T)
    d_in = [to_dev(b) for b in batches]
    outs = [(torch.full((T + 1,), -5, dtype=torch.int32, device=DEV), torch.full((T + 1,), -3, dtype=torch.int64, device=DEV),
             torch.full((cap + 64,), GUARD, dtype=torch.uint8, device=DEV)) for _ in range(K)]
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        torch.cuda.synchronize()
        for k in range(K):
            core.diff_stream_cwire_batch(d_in[k], T, outs[k][0], outs[k][1], outs[k][2], cap)
        core.synchronize()
        state = base.copy()
        for k in range(K):
            eo, exs, edf, state = po.diff_stream(batches[k], state)
            want, wpos = spec.encode(eo, exs, edf)
            check_full(outs[k][0].cpu().numpy().view(np.uint32), outs[k][1].cpu().numpy().view(np.uint64),
                       outs[k][2].cpu().numpy(), eo, want, wpos)
        assert np.array_equal(core.get_state(), state)


def test_direct_split_pack_at_1080p():
    """1080p, pipelined and split, three batches, each checked against the oracle."""
    w, h, T, K = 1920, 1080, 4, 3
    n = 3 * w * h
    base, fr = synth.webcam_stream(K * T, w, h, seed=17)
    cap = cwire_bytes_max(n, T)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        state = base.copy()
        for k in range(K):
            d_in = to_dev(fr[k * T:(k + 1) * T])
            d_off = torch.zeros(T + 1, dtype=torch.int32, device=DEV)
            d_pos = torch.zeros(T + 1, dtype=torch.int64, device=DEV)
            d_cw = torch.full((cap,), GUARD, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize()
            core.diff_stream_cwire_batch(d_in, T, d_off, d_pos, d_cw, cap)
            core.synchronize()
            eo, exs, edf, state = po.diff_stream(fr[k * T:(k + 1) * T], state)
            want, wpos = spec.encode(eo, exs, edf)
            assert np.array_equal(d_pos.cpu().numpy().view(np.uint64), wpos), k
            assert np.array_equal(d_cw[:want.size].cpu().numpy(), want), k
        assert np.array_equal(core.get_state(), state)


def test_direct_after_filter_and_interleaved_with_diff_stream_batch():
    """A frame filter, then the direct call (sequential schedule); then diff_stream_batch and the direct call alternating
    on the same core and stream of frames -- each result against the oracle."""
    w, h, T = 320, 180, 4
    n = 3 * w * h
    base, fr = synth.webcam_stream(5 * T, w, h, seed=12)
    d_fr = to_dev(fr)
    vis = torch.empty((T, n), dtype=torch.uint8, device=DEV)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        core.filter_batch(lib.OP_GRAY_WEIGHTED_BINARIZE, d_fr[:T], vis, T)
        state, _ = check_oracle(core, fr[:T], base)
        for k in range(1, 5):
            chunk = fr[k * T:(k + 1) * T]
            if k % 2:
                eo, exs, edf, state = po.diff_stream(chunk, state)
                d_off = torch.zeros(T + 1, dtype=torch.int32, device=DEV)
                d_xs = torch.empty(T * n, dtype=torch.int32, device=DEV)
                d_df = torch.empty(T * n, dtype=torch.uint8, device=DEV)
                core.diff_stream_batch(d_fr[k * T:(k + 1) * T], T, d_off, d_xs, d_df, T * n)
                core.synchronize()
                tot = int(eo[-1])
                assert np.array_equal(d_off.cpu().numpy().view(np.uint32), eo)
                assert np.array_equal(d_xs[:tot].cpu().numpy(), exs) and np.array_equal(d_df[:tot].cpu().numpy(), edf)
            else:
                state, _ = check_oracle(core, chunk, state)
        assert np.array_equal(core.get_state(), state)


def test_direct_records_rebuild_every_frame_on_the_host():
    w, h, T = 160, 90, 8
    base, fr = synth.webcam_stream(T, w, h, seed=29)
    eo, exs, edf, _ = po.diff_stream(fr, base)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        off, pos, got = direct(core, to_dev(fr), T)
    buf = got[:int(pos[-1])]
    client, want = base.copy(), base.copy()
    for t in range(T):
        used = cwire_apply_host(client, buf[int(pos[t]):], 1)
        assert used == int(pos[t + 1] - pos[t])
        a, b = int(eo[t]), int(eo[t + 1])
        want[exs[a:b]] += edf[a:b]
        assert np.array_equal(client, want), t


RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.skipif(not os.path.exists(RT), reason="tools/roundtrip not built")
@pytest.mark.parametrize("w,h,T,B", [(320, 180, 24, 8), (97, 13, 10, 4), (1920, 1080, 6, 3)])
def test_roundtrip_compact_direct(w, h, T, B):
    out = subprocess.run([RT, "--width", str(w), "--height", str(h), "--frames", str(T), "--batch", str(B), "--compact",
                          "--direct"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["format"] == "compact" and r["direct"] is True and r["max_abs_error"] <= 20


def test_direct_refuses_bad_arguments_and_writes_nothing():
    w, h, T = 64, 48, 4
    base, fr = synth.webcam_stream(T, w, h, seed=2)
    n = 3 * w * h
    cap = cwire_bytes_max(n, T)
    d_fr = to_dev(fr)
    d_off = torch.full((T + 2,), -5, dtype=torch.int32, device=DEV)
    d_pos = torch.full((T + 2,), -3, dtype=torch.int64, device=DEV)
    d_cw = torch.full((cap + 16,), GUARD, dtype=torch.uint8, device=DEV)
    off_p, pos_p, cw_p = d_off.data_ptr(), d_pos.data_ptr(), d_cw.data_ptr()
    bad = [
        (d_fr, T, None, pos_p, cw_p, cap),          # null d_offsets
        (d_fr, T, off_p, None, cw_p, cap),          # null d_frame_pos
        (d_fr, T, off_p, pos_p, None, cap),         # null d_cwire with room
        (None, T, off_p, pos_p, cw_p, cap),         # null frames
        (d_fr, T, off_p, pos_p, cw_p + 1, cap),     # misaligned records
        (d_fr, T, off_p, pos_p, cw_p + 2, cap),
        (d_fr, T, off_p + 2, pos_p, cw_p, cap),     # misaligned offsets
        (d_fr, T, off_p, pos_p + 4, cw_p, cap),     # frame_pos 4- but not 8-aligned
        (d_fr, T + 1, off_p, pos_p, cw_p, cap),     # nframes > max_batch
        (d_fr, -1, off_p, pos_p, cw_p, cap),        # negative nframes
    ]
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        torch.cuda.synchronize()
        for args in bad:
            with pytest.raises(lib.Mi355Error) as e:
                core.diff_stream_cwire_batch(*args)
            assert e.value.code == lib.ERR_INVALID, args[1:]
        core.synchronize()
        assert (d_off.cpu().numpy() == -5).all()
        assert (d_pos.cpu().numpy() == -3).all()
        assert (d_cw.cpu().numpy() == GUARD).all()
        assert np.array_equal(core.get_state(), base)

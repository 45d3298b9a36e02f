"""-m gpu: the compact wire format's encoder and decoder on the device (include/mi355diff.h, "compact wire format") against
the numpy statement of the format (tests/cwire_spec.py), byte for byte, on the streams every entry point produces."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_bytes_max, synth
from oracle import pyoracle as po
from gpu_util import DEV, CUDACore, run_stream, to_dev

pytestmark = pytest.mark.gpu

GUARD = 0x5C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def encode(core, d_off, d_xs, d_df, ecap, T, capacity=None, frame_bytes=None):
    """GPU encode into a guarded buffer -> (frame_pos uint64[T+1], bytes of the whole buffer)."""
    n = core.total if frame_bytes is None else frame_bytes
    cap = cwire_bytes_max(n, T) if capacity is None else capacity
    d_pos = torch.full((T + 1,), -3, dtype=torch.int64, device=DEV)
    d_cw = torch.full((cap + 256,), GUARD, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()   # (the new entry points are not in gpu_util's synced list)
    core.cwire_encode_batch(d_off, d_xs, d_df, ecap, T, d_pos, d_cw, cap)
    core.synchronize()
    return d_pos.cpu().numpy().view(np.uint64), d_cw.cpu().numpy()


def check_encode(core, off, xs, df, d_bufs=None):
    T = off.size - 1
    if d_bufs is None:
        d_off, d_xs, d_df = to_dev(off.view(np.int32)), to_dev(np.append(xs, np.int32(0))), to_dev(np.append(df, np.uint8(0)))
        ecap = xs.size
    else:
        d_off, (d_xs, d_df) = to_dev(off.view(np.int32)), d_bufs
        ecap = d_xs.numel()
    want, wpos = spec.encode(off, xs, df)
    pos, got = encode(core, d_off, d_xs, d_df, ecap, T)
    assert np.array_equal(pos, wpos)
    assert np.array_equal(got[:want.size], want)
    assert (got[want.size:] == GUARD).all()
    return want


@pytest.mark.parametrize("w,h,T", [(1, 1, 4), (33, 7, 9), (211, 3, 17), (64, 48, 6), (1920, 1080, 8), (3840, 2160, 3)])
def test_encode_stream_equals_spec(w, h, T):
    base, frames = synth.webcam_stream(T, w, h, seed=5)
    frames = frames.copy()
    frames[T // 2] = frames[T // 2 - 1] if T > 1 else frames[0]   # a frame with nothing to send
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        off, xs, df, bufs = run_stream(core, frames)
        check_encode(core, off, xs, df, bufs)


@pytest.mark.parametrize("w,h,T", [(33, 7, 5), (64, 48, 4), (1920, 1080, 4)])
def test_encode_pairs_equals_spec(w, h, T):
    _, frames = synth.webcam_stream(T + 1, w, h, seed=11)
    with CUDACore(w, h, max_batch=T) as core:
        d_frames = to_dev(frames)
        off, xs, df, bufs = run_stream(core, d_frames[1:], pair_prev=d_frames[:-1])
        check_encode(core, off, xs, df, bufs)


@pytest.mark.parametrize("regime", ["S0", "S2", "S3", "S4"])
def test_encode_regimes_equal_spec(regime):
    """S0 noise (~85 % of the bytes change), S2 static (nothing), S3 flip (every byte, gaps 0), S4 an edge strip of isolated
    bytes far apart (escapes)."""
    w, h, T = 320, 180, 4
    n = 3 * w * h
    base = synth.refrand_frame(n, 100)
    if regime == "S0":
        frames = np.stack([synth.refrand_frame(n, 1 + t) for t in range(T)])
    elif regime == "S2":
        frames = np.stack([base] * T)
    elif regime == "S3":
        frames = np.stack([base ^ np.uint8(0x80 * ((t + 1) & 1)) for t in range(T)])
    else:
        frames = np.stack([base] * T)
        for t in range(T):
            frames[t, (np.arange(t, n, 997 + 131 * t))] ^= 0x80
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        off, xs, df, bufs = run_stream(core, frames)
        if regime == "S2":
            assert int(off[-1]) == 0
        if regime == "S3":
            assert int(off[-1]) == T * n
        want = check_encode(core, off, xs, df, bufs)
        if regime == "S4":
            assert spec.headers(want, T)[1].min() > 0


@pytest.mark.parametrize("w,h,T,parts", [(64, 50, 4, 3), (1920, 1080, 3, 8)])
def test_encode_merged_bands_equals_spec(w, h, T, parts):
    base, frames = synth.webcam_stream(T, w, h, seed=23)
    n = 3 * w * h
    rows = [h * p // parts for p in range(parts + 1)]
    d_frames = to_dev(frames)
    p_off, p_xs, p_df = [], [], []
    for p in range(parts):
        b0, b1 = 3 * w * rows[p], 3 * w * rows[p + 1]
        with CUDACore(w, rows[p + 1] - rows[p], sample_mat_data=base[b0:b1], max_batch=T) as band:
            o, x, d, _ = run_stream(band, d_frames[:, b0:b1].contiguous())
            p_off.append(o); p_xs.append(x); p_df.append(d)
    part_base = np.concatenate([[0], np.cumsum([x.size for x in p_xs])])[:-1]
    total = sum(x.size for x in p_xs)
    with CUDACore(w, h, max_batch=T) as core:
        d_off = torch.zeros(T + 1, dtype=torch.int32, device=DEV)
        d_xs = torch.zeros(total + 1, dtype=torch.int32, device=DEV)
        d_df = torch.zeros(total + 1, dtype=torch.uint8, device=DEV)
        core.merge_parts(to_dev(np.stack(p_off).view(np.int32)), part_base, [3 * w * r for r in rows[:-1]],
                         to_dev(np.concatenate(p_xs + [[0]]).astype(np.int32)), to_dev(np.concatenate(p_df + [[0]]).astype(np.uint8)),
                         T, d_off, d_xs, d_df, total)
        # no synchronize: the encoder is ordered behind the merge on the core's stream
        cap = cwire_bytes_max(n, T)
        d_pos = torch.zeros(T + 1, dtype=torch.int64, device=DEV)
        d_cw = torch.full((cap + 64,), GUARD, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        core.cwire_encode_batch(d_off, d_xs, d_df, total, T, d_pos, d_cw, cap)
        core.synchronize()
        off = d_off.cpu().numpy().view(np.uint32)
        want, wpos = spec.encode(off, d_xs[:total].cpu().numpy(), d_df[:total].cpu().numpy())
        got = d_cw.cpu().numpy()
        assert np.array_equal(d_pos.cpu().numpy().view(np.uint64), wpos)
        assert np.array_equal(got[:want.size], want) and (got[want.size:] == GUARD).all()


def test_encode_capacity_skips_whole_frames():
    w, h, T = 64, 48, 6
    base, frames = synth.webcam_stream(T, w, h, seed=9)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        off, xs, df, bufs = run_stream(core, frames)
        want, wpos = spec.encode(off, xs, df)
        d_off = to_dev(off.view(np.int32))
        cap = int(wpos[3]) + 12                     # frames 0..2 fit, frame 3 does not (nor 4, 5)
        pos, got = encode(core, d_off, bufs[0], bufs[1], bufs[0].numel(), T, capacity=cap)
        assert np.array_equal(pos, wpos)            # exact regardless
        assert np.array_equal(got[:int(wpos[3])], want[:int(wpos[3])])
        assert (got[int(wpos[3]):] == GUARD).all()
        # a frame in the middle that does not fit while a smaller later one would: skipped, and only it
        big = int(np.argmax(np.diff(wpos.astype(np.int64))))
        cap = int(wpos[big + 1]) - 4
        pos, got = encode(core, d_off, bufs[0], bufs[1], bufs[0].numel(), T, capacity=cap)
        assert np.array_equal(got[:int(wpos[big])], want[:int(wpos[big])])
        assert (got[int(wpos[big]):] == GUARD).all()


def test_encode_overflowed_diff_batch_writes_nothing():
    w, h, T = 64, 48, 5
    base, frames = synth.webcam_stream(T, w, h, seed=3)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        off, xs, df, _ = run_stream(core, frames)
        small = int(off[-1]) - 1
        d_off = to_dev(off.view(np.int32))
        pos, got = encode(core, d_off, to_dev(xs[:small]), to_dev(df[:small]), small, T)
        assert int(pos[T]) == 2 ** 64 - 1
        assert (pos[:T].view(np.int64) == -3).all()
        assert (got == GUARD).all()


@pytest.mark.parametrize("w,h,T", [(33, 7, 9), (64, 48, 6), (1920, 1080, 6), (3840, 2160, 2)])
def test_decode_equals_original_and_reconstructs(w, h, T):
    base, frames = synth.webcam_stream(T, w, h, seed=31)
    off, xs, df, st = po.diff_stream(frames, base) if w * h < 10 ** 6 else (None,) * 4
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as server, CUDACore(w, h, sample_mat_data=base, max_batch=T) as client:
        if off is None:
            off, xs, df, _ = run_stream(server, frames)
            st = server.get_state()
        buf, pos = spec.encode(off, xs, df)
        counts, escapes = spec.headers(buf, T)
        cap = xs.size
        d_off = torch.full((T + 1,), -1, dtype=torch.int32, device=DEV)
        d_xs = torch.full((cap + 8,), -7, dtype=torch.int32, device=DEV)
        d_df = torch.full((cap + 8,), GUARD, dtype=torch.uint8, device=DEV)
        d_cw = to_dev(buf)
        torch.cuda.synchronize()
        client.cwire_decode_batch(d_cw, counts, escapes, T, d_off, d_xs, d_df, cap)
        client.apply_batch(d_off, d_xs, d_df, T)
        client.synchronize()
        assert np.array_equal(d_off.cpu().numpy().view(np.uint32), off)
        g_xs, g_df = d_xs.cpu().numpy(), d_df.cpu().numpy()
        assert np.array_equal(g_xs[:cap], xs) and (g_xs[cap:] == -7).all()
        assert np.array_equal(g_df[:cap], df) and (g_df[cap:] == GUARD).all()
        assert np.array_equal(client.get_state(), st)


def test_decode_capacity_and_bad_escape_rank():
    rng = np.random.default_rng(4)
    N = 3 * 40 * 30
    x0 = np.sort(rng.choice(N, 300, replace=False)).astype(np.int32)
    x1 = np.array([0, 400, 401, 1000], np.int32)
    off = np.array([0, x0.size, x0.size + x1.size], np.uint32)
    xs = np.concatenate([x0, x1]); df = rng.integers(1, 256, xs.size).astype(np.uint8)
    buf, pos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(buf, 2)
    with CUDACore(40, 30, max_batch=2) as core:
        cap = x0.size + 2                               # frame 1 loses its last two entries
        d_off = torch.full((3,), -1, dtype=torch.int32, device=DEV)
        d_xs = torch.full((cap + 8,), -7, dtype=torch.int32, device=DEV)
        d_df = torch.full((cap + 8,), GUARD, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        core.cwire_decode_batch(to_dev(buf), counts, escapes, 2, d_off, d_xs, d_df, cap)
        core.synchronize()
        assert np.array_equal(d_off.cpu().numpy().view(np.uint32), off)   # exact
        g = d_xs.cpu().numpy()
        assert np.array_equal(g[:cap], xs[:cap]) and (g[cap:] == -7).all()
        # frame 1 with header e = 1 though it holds 2 escape codes: the second decodes to 0xFFFFFFFF
        e_bad = escapes.copy(); e_bad[1] = escapes[1] - 1
        b2 = bytearray(buf.tobytes())
        at = int(pos[1])
        b2[at + 4:at + 8] = np.uint32(e_bad[1]).tobytes()
        rec = spec.frame_bytes(x1.size, e_bad[1])
        b2 = bytes(b2[:at]) + bytes(b2[at:at + 8 + 4]) + bytes(b2[at + 12:at + 12 + 4 * int(e_bad[1])]) + bytes(b2[at + 12 + 4 * int(escapes[1]):])
        assert len(b2) == at + rec
        d_xs = torch.full((xs.size + 8,), -7, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        core.cwire_decode_batch(to_dev(np.frombuffer(b2, np.uint8)), counts, e_bad, 2, d_off, d_xs, d_df, xs.size)
        core.synchronize()
        g = d_xs.cpu().numpy().view(np.uint32)
        codes = np.frombuffer(b2, np.uint8)[at + 8:at + 12]
        ranks = np.cumsum(codes == 255) - 1
        bad = (codes == 255) & (ranks >= int(e_bad[1]))
        assert bad.sum() == 1
        assert g[x0.size + int(np.argmax(bad))] == 0xFFFFFFFF
        assert (g[xs.size:].view(np.int32) == -7).all()


@pytest.mark.parametrize("dense", [False, True])
def test_encode_right_behind_a_pipelined_batch(dense):
    """The encoder joins a pipelined own-stream batch (whose index and expansion run on a side stream) before it reads it:
    no synchronize between the batch and the encode."""
    w, h, T, K = 640, 360, 8, 4
    n = 3 * w * h
    if dense:
        base = synth.refrand_frame(n, 100)
        batches = [np.stack([synth.refrand_frame(n, 1 + k * T + t) for t in range(T)]) for k in range(K)]
    else:
        base, fr = synth.webcam_stream(K * T, w, h, seed=41)
        batches = [fr[k * T:(k + 1) * T] for k in range(K)]
    cap = T * n
    cwcap = cwire_bytes_max(n, T)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        outs = []
        d_in = [to_dev(b) for b in batches]
        torch.cuda.synchronize()
        for k in range(K):
            d_off = torch.zeros(T + 1, dtype=torch.int32, device=DEV)
            d_xs = torch.empty(cap, dtype=torch.int32, device=DEV)
            d_df = torch.empty(cap, dtype=torch.uint8, device=DEV)
            d_pos = torch.zeros(T + 1, dtype=torch.int64, device=DEV)
            d_cw = torch.empty(cwcap, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize()
            core.diff_stream_batch(d_in[k], T, d_off, d_xs, d_df, cap)
            core.cwire_encode_batch(d_off, d_xs, d_df, cap, T, d_pos, d_cw, cwcap)
            outs.append((d_pos, d_cw))
        core.synchronize()
    state = base.copy()
    for k in range(K):
        off, xs, df, state = po.diff_stream(batches[k], state)
        want, wpos = spec.encode(off, xs, df)
        d_pos, d_cw = outs[k]
        assert np.array_equal(d_pos.cpu().numpy().view(np.uint64), wpos), k
        assert np.array_equal(d_cw[:want.size].cpu().numpy(), want), k


RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.skipif(not os.path.exists(RT), reason="tools/roundtrip not built")
@pytest.mark.parametrize("w,h,T,B", [(320, 180, 24, 8), (97, 13, 10, 4), (1920, 1080, 6, 3)])
def test_roundtrip_compact(w, h, T, B):
    out = subprocess.run([RT, "--width", str(w), "--height", str(h), "--frames", str(T), "--batch", str(B), "--compact"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["format"] == "compact" and r["max_abs_error"] <= 20
    assert r["wire_bytes"] < 4 * T + 5 * r["changed_bytes"]

"""-m gpu: mi355_apply_cwire_batch, compact records applied straight to a client core's state in one call
(include/mi355diff.h), against the host client (mi355_cwire_apply_host) and against decode + apply_batch, in both modes."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib, synth
from gpu_util import DEV, CUDACore, to_dev

pytestmark = pytest.mark.gpu

GUARD = 0x5C
PAD = 256            # guard bytes before and after every device buffer
TILE = 4096          # bytes of the state per workgroup of the apply kernel (csrc/internal.h, kCwaTile)
CHUNK = 4096         # codes per workgroup of the directory kernels (kCwaChunk)
ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))


def guarded(data, size=None):
    """A device buffer of PAD guard bytes, the data (or `size` guard bytes), PAD guard bytes -> (buffer, view)."""
    size = data.size if data is not None else size
    buf = torch.full((size + 2 * PAD,), GUARD, dtype=torch.uint8, device=DEV)
    if data is not None and data.size:
        buf[PAD:PAD + size] = to_dev(data)
    return buf, buf[PAD:PAD + size]


def host_frames(state, recs, T):
    """The host client, frame by frame -> (frames[T, N], final state)."""
    st = state.copy()
    out, at = [], 0
    for _ in range(T):
        at += cwire_apply_host(st, recs[at:], 1)
        out.append(st.copy())
    return (np.stack(out) if out else np.zeros((0, st.size), np.uint8)), st


def gpu_apply(core, recs, counts, escapes, T, outputs=True, stride=None, shift=0):
    """One call on a guarded copy of the records -> (frames[T, N] or None, state); guard bytes checked."""
    n = core.total
    stride = n if stride is None else stride
    cw, d_cw = guarded(recs)
    frames = None
    if outputs:
        ob, d_out = guarded(None, T * stride + shift)
        d_out = d_out[shift:]
    else:
        d_out = None
    torch.cuda.synchronize()   # (the new entry point is not in gpu_util's synced list)
    core.apply_cwire_batch(d_cw, counts, escapes, T, d_out, stride)
    core.synchronize()
    c = cw.cpu().numpy()
    assert (c[:PAD] == GUARD).all() and (c[PAD + recs.size:] == GUARD).all()
    assert np.array_equal(c[PAD:PAD + recs.size], recs)
    if outputs:
        o = ob.cpu().numpy()
        assert (o[:PAD + shift] == GUARD).all() and (o[PAD + shift + T * stride:] == GUARD).all()
        body = o[PAD + shift:PAD + shift + T * stride].reshape(T, stride) if T else np.zeros((0, stride), np.uint8)
        assert (body[:, n:] == GUARD).all()   # the stride gap
        frames = body[:, :n].copy()
    return frames, core.get_state()


def two_call(core, recs, counts, escapes, T, outputs=True):
    """decode + apply_batch on `core` -> (frames or None, state)."""
    n = core.total
    total = int(counts.astype(np.int64).sum())
    d_cw = to_dev(recs) if recs.size else torch.zeros(4, dtype=torch.uint8, device=DEV)
    d_off = torch.zeros(T + 1, dtype=torch.int32, device=DEV)
    d_xs = torch.zeros(max(total, 1), dtype=torch.int32, device=DEV)
    d_df = torch.zeros(max(total, 1), dtype=torch.uint8, device=DEV)
    d_out = torch.zeros(max(T * n, 1), dtype=torch.uint8, device=DEV) if outputs else None
    torch.cuda.synchronize()
    core.cwire_decode_batch(d_cw, counts, escapes, T, d_off, d_xs, d_df, total)
    core.apply_batch(d_off, d_xs, d_df, T, d_out, n)
    core.synchronize()
    frames = d_out[:T * n].cpu().numpy().reshape(T, n) if outputs else None
    return frames, core.get_state()


def check_all(w, h, state, recs, T, max_batch=None, stride=None, shift=0):
    """The new call in both modes against the host client and decode + apply_batch."""
    counts, escapes = spec.headers(recs, T)
    want_frames, want_state = host_frames(state, recs, T)
    mb = max(T, 1) if max_batch is None else max_batch
    for outputs in (True, False):
        with CUDACore(w, h, sample_mat_data=state, max_batch=mb) as a, \
                CUDACore(w, h, sample_mat_data=state, max_batch=max(T, 1)) as b:
            got, st = gpu_apply(a, recs, counts, escapes, T, outputs, stride, shift)
            ref, rst = two_call(b, recs, counts, escapes, T, outputs)
            assert np.array_equal(st, want_state)
            assert np.array_equal(rst, want_state)
            if outputs:
                assert np.array_equal(got, want_frames)
                assert np.array_equal(ref, want_frames)


def server_records(w, h, base, frames, T):
    """mi355_diff_stream_cwire_batch on a server core -> the records (numpy) and the server's final state."""
    n = 3 * w * h
    cap = cwire_bytes_max(n, T)
    d_off = torch.zeros(T + 1, dtype=torch.int32, device=DEV)
    d_pos = torch.zeros(T + 1, dtype=torch.int64, device=DEV)
    d_cw = torch.zeros(max(cap, 4), dtype=torch.uint8, device=DEV)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as srv:
        d_fr = to_dev(frames)
        torch.cuda.synchronize()
        srv.diff_stream_cwire_batch(d_fr, T, d_off, d_pos, d_cw, cap)
        srv.synchronize()
        pos = d_pos.cpu().numpy().view(np.uint64)
        return d_cw[:int(pos[-1])].cpu().numpy(), srv.get_state()


def encoder_records(offsets, xs, diff):
    """mi355_cwire_encode_batch on (offsets, xs, diff) -> the records (numpy), checked against the numpy statement."""
    T = offsets.size - 1
    want, wpos = spec.encode(offsets, xs, diff)
    total = int(offsets[-1])
    cap = max(int(wpos[-1]), 4)
    d_pos = torch.zeros(T + 1, dtype=torch.int64, device=DEV)
    d_cw = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    with CUDACore(1, 1, max_batch=1) as enc:
        d_off = to_dev(offsets.astype(np.uint32).view(np.int32))
        d_xs = to_dev(np.asarray(xs, np.int32)) if total else torch.zeros(1, dtype=torch.int32, device=DEV)
        d_df = to_dev(np.asarray(diff, np.uint8)) if total else torch.zeros(1, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        enc.cwire_encode_batch(d_off, d_xs, d_df, total, T, d_pos, d_cw, cap)
        enc.synchronize()
        got = d_cw[:int(wpos[-1])].cpu().numpy()
    assert np.array_equal(got, want)
    return got


def stream_of(frames_xs, rng):
    """Per-frame index lists -> (offsets, xs, diff) with random non-zero diffs."""
    offs = np.zeros(len(frames_xs) + 1, np.int64)
    for t, x in enumerate(frames_xs):
        offs[t + 1] = offs[t] + len(x)
    xs = np.concatenate([np.asarray(x, np.int64) for x in frames_xs]) if offs[-1] else np.zeros(0, np.int64)
    diff = rng.integers(1, 256, xs.size).astype(np.uint8)
    return offs, xs, diff


@pytest.mark.parametrize("w,h,T", [(1, 1, 4), (33, 7, 9), (211, 3, 17), (64, 48, 6), (1920, 1080, 6), (3840, 2160, 3)])
def test_equals_host_and_two_call_path(w, h, T):
    base, frames = synth.webcam_stream(T, w, h, seed=11)
    frames = frames.copy()
    frames[T // 2] = frames[T // 2 - 1]   # a frame with nothing changed
    recs, srv_state = server_records(w, h, base, frames, T)
    counts, _ = spec.headers(recs, T)
    assert counts[T // 2] == 0
    check_all(w, h, base, recs, T)
    _, st = host_frames(base, recs, T)
    assert np.array_equal(st, srv_state)


def _regime_frames(name, n):
    if name == "S0":      # every byte changes
        return [np.arange(n)] * 2
    if name == "last":    # a single change at byte N-1: g0 is an escape
        return [[n - 1], [n - 1], []]
    if name == "gaps":    # gaps of exactly 254, 255 and 256 ending / starting at tile and chunk boundaries
        out = []
        for gap in (254, 255, 256):
            xs = set()
            for b in range(TILE, n, TILE):
                for x in (b - 1 - gap - 1, b - 1, b + gap, b + 2 * gap + 1):
                    if 0 <= x < n:
                        xs.add(x)
            out.append(sorted(xs))
        # a dense run long enough to cross a chunk of codes, then gaps across it
        dense = list(range(0, CHUNK + 7)) + [CHUNK + 7 + 254, CHUNK + 7 + 254 + 256, CHUNK + 7 + 254 + 256 + 256]
        out.append([x for x in dense if x < n])
        return out
    if name == "edges":   # the first and last byte of every tile
        xs = sorted({x for b in range(0, n, TILE) for x in (b, min(b + TILE, n) - 1)})
        return [xs, xs[::2], xs[1::2]]
    if name == "sparse":  # gaps that jump many tiles
        return [[3, 5 * TILE + 17, n - 2], [n // 2], [0, n - 1], list(range(7, n, 9 * TILE + 1))]
    raise AssertionError(name)


@pytest.mark.parametrize("regime", ["S0", "last", "gaps", "edges", "sparse"])
@pytest.mark.parametrize("w,h", [(128, 90), (1920, 1080)])
def test_regimes(regime, w, h):
    n = 3 * w * h
    rng = np.random.default_rng(len(regime) * 7 + w)
    offs, xs, diff = stream_of(_regime_frames(regime, n), rng)
    recs = encoder_records(offs, xs, diff)
    counts, escapes = spec.headers(recs, offs.size - 1)
    if regime == "last":
        assert escapes[0] == 1
    check_all(w, h, synth.refrand_frame(n, 3), recs, offs.size - 1)


@pytest.mark.parametrize("stride_extra,shift", [(13, 5), (1, 3), (16, 0)])
def test_outputs_strided_with_guards(stride_extra, shift):
    w, h, T = 97, 45, 7
    base, frames = synth.webcam_stream(T, w, h, seed=4)
    recs, _ = server_records(w, h, base, frames, T)
    check_all(w, h, base, recs, T, stride=3 * w * h + stride_extra, shift=shift)


@pytest.mark.parametrize("max_batch", [1, 4])
def test_slices_longer_than_max_batch(max_batch):
    w, h, T = 64, 48, 9
    base, frames = synth.webcam_stream(T, w, h, seed=6)
    recs, _ = server_records(w, h, base, frames, T)
    check_all(w, h, base, recs, T, max_batch=max_batch)


def test_round_trip_server_to_client_every_frame():
    """Server core, one frame per batch (its state after every frame) -> records -> client core, one call."""
    w, h, T = 320, 180, 12
    n = 3 * w * h
    base, frames = synth.webcam_stream(T, w, h, seed=9)
    cap = cwire_bytes_max(n, 1)
    states, parts = [], []
    with CUDACore(w, h, sample_mat_data=base, max_batch=1) as srv:
        d_off = torch.zeros(2, dtype=torch.int32, device=DEV)
        d_pos = torch.zeros(2, dtype=torch.int64, device=DEV)
        d_cw = torch.zeros(cap, dtype=torch.uint8, device=DEV)
        for t in range(T):
            d_fr = to_dev(frames[t:t + 1])
            torch.cuda.synchronize()
            srv.diff_stream_cwire_batch(d_fr, 1, d_off, d_pos, d_cw, cap)
            srv.synchronize()
            parts.append(d_cw[:int(d_pos.cpu().numpy().view(np.uint64)[1])].cpu().numpy())
            states.append(srv.get_state())
    recs = np.concatenate(parts)
    counts, escapes = spec.headers(recs, T)
    with CUDACore(w, h, sample_mat_data=base, max_batch=5) as cli:
        got, st = gpu_apply(cli, recs, counts, escapes, T)
    for t in range(T):
        assert np.array_equal(got[t], states[t]), t
    assert np.array_equal(st, states[-1])


@pytest.mark.parametrize("seed", range(6))
def test_malformed_content_stays_in_bounds(seed):
    """Consistent headers, random code / escape / diff bytes: no byte outside the state and the outputs changes; where the
    host client accepts the records, the results are equal."""
    rng = np.random.default_rng(seed)
    w, h, T = 64, 48, 5
    n = 3 * w * h
    counts = rng.integers(0, n + 1, T).astype(np.uint32)
    counts[0] = n
    escapes = np.array([rng.integers(0, c + 1) if seed % 2 else min(int(c), int(rng.integers(0, 40)))
                        for c in counts], np.uint32)
    parts = []
    for c, e in zip(counts, escapes):
        p = spec.pad4(int(c))
        code = rng.integers(0, 256, p, dtype=np.uint8)
        if seed % 3 == 0:
            code = np.where(code > 250, 255, code % 3).astype(np.uint8)   # mostly small gaps, some escapes
        esc = rng.integers(0, 2 ** 32, int(e), dtype=np.uint64).astype(np.uint32)
        if seed % 3 == 1:
            esc %= 600
        body = np.concatenate([np.array([c, e], "<u4").view(np.uint8), code, esc.view(np.uint8),
                               rng.integers(0, 256, p, dtype=np.uint8)])
        parts.append(body)
    recs = np.concatenate(parts)
    base = synth.refrand_frame(n, seed)
    with CUDACore(w, h, sample_mat_data=base, max_batch=2) as core:
        got, st = gpu_apply(core, recs, counts, escapes, T, stride=n + 7, shift=3)
    try:
        want_frames, want_state = host_frames(base, recs, T)
    except lib.Mi355Error:
        return
    assert np.array_equal(got, want_frames) and np.array_equal(st, want_state)


def test_malformed_escape_values_host_accepts():
    """Records whose escapes hold values below 255 (not canonical, but the host client accepts them) and a frame whose
    decoded indices stay below N: equal to the host client."""
    w, h, T = 40, 30, 3
    n = 3 * w * h
    rng = np.random.default_rng(1)
    parts = []
    for _ in range(T):
        code = np.full(40, 255, np.uint8)
        code[::3] = 7
        e = int((code == 255).sum())
        esc = rng.integers(0, 60, e).astype(np.uint32)
        parts.append(np.concatenate([np.array([40, e], "<u4").view(np.uint8), code, esc.view(np.uint8),
                                     rng.integers(0, 256, 40, dtype=np.uint8)]))
    recs = np.concatenate(parts)
    check_all(w, h, synth.refrand_frame(n, 2), recs, T)


def test_refuses_bad_arguments_and_writes_nothing():
    w, h, T = 33, 7, 3
    n = 3 * w * h
    base, frames = synth.webcam_stream(T, w, h, seed=3)
    recs, _ = server_records(w, h, base, frames, T)
    counts, escapes = spec.headers(recs, T)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        cw, d_cw = guarded(recs)
        ob, d_out = guarded(None, T * n + 8)
        torch.cuda.synchronize()
        bad_e = escapes.copy()
        bad_e[1] = counts[1] + 1
        big = counts.copy()
        big[2] = n + 1
        cases = [
            dict(nframes=-1),
            dict(d_cwire=None),
            dict(counts=None),
            dict(escapes=None),
            dict(escapes=bad_e),
            dict(counts=big, escapes=np.minimum(escapes, big)),
            dict(d_cwire=cw[PAD + 1:PAD + 1 + recs.size]),
            dict(stride=n - 1),
        ]
        L = lib.load()
        for case in cases:
            c = case.get("counts", counts)
            e = case.get("escapes", escapes)
            c_ptr = None if c is None else np.ascontiguousarray(c, np.uint32)
            e_ptr = None if e is None else np.ascontiguousarray(e, np.uint32)
            dc = case.get("d_cwire", d_cw)
            rc = L.mi355_apply_cwire_batch(core._h, None if dc is None else dc.data_ptr(),
                                           None if c_ptr is None else c_ptr.ctypes.data,
                                           None if e_ptr is None else e_ptr.ctypes.data,
                                           case.get("nframes", T), d_out.data_ptr(), case.get("stride", n))
            assert rc == lib.ERR_INVALID, case
        core.synchronize()
        assert np.array_equal(core.get_state(), base)
        assert (ob.cpu().numpy() == GUARD).all()
        # nframes = 0 and null pointers: nothing to do, accepted
        assert L.mi355_apply_cwire_batch(core._h, None, None, None, 0, None, 0) == lib.OK


RT = os.path.join(ROOT, "tools", "roundtrip")


@pytest.mark.skipif(not os.path.exists(RT), reason="tools/roundtrip not built")
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("w,h,T,B", [(1920, 1080, 6, 3), (97, 13, 10, 4)])
def test_roundtrip_gpu_client(direct, w, h, T, B):
    args = [RT, "--width", str(w), "--height", str(h), "--frames", str(T), "--batch", str(B), "--compact", "--gpu-client"]
    if direct:
        args.append("--direct")
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["roundtrip"] == "ok" and r["gpu_client"] is True and r["direct"] is direct and r["max_abs_error"] <= 20

"""-m gpu: mi355_diff_multi_batch / _wire_batch / _cwire_batch -- one frame of each of S streams per call, the states in the
caller's memory (include/mi355diff.h, "many streams, one frame each").  Everything is compared bit for bit: with the oracle
stream by stream, with S separate cores fed diff_stream_batch(nframes = 1), and the three output forms with each other."""
import ctypes as C

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib, synth
from oracle import pyoracle as po
from gpu_util import DEV, CUDACore, to_dev

pytestmark = pytest.mark.gpu

GUARD = 0x5C


class Region:
    """S frames of n bytes, `stride` apart, inside a guarded device buffer that starts `skew` bytes behind an aligned
    address.  Every byte outside the S frames holds GUARD and must still hold it afterwards."""

    def __init__(self, S, n, stride=None, skew=0):
        self.S, self.n, self.stride, self.skew = S, n, n if stride is None else stride, skew
        self.buf = torch.full((skew + max(S, 1) * self.stride + 64,), GUARD, dtype=torch.uint8, device=DEV)
        self.t = self.buf[skew:]
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == skew % 16

    def put(self, rows):
        for s, row in enumerate(rows):
            self.t[s * self.stride:s * self.stride + self.n] = to_dev(row)
        return self

    def get(self):
        """(rows as numpy [S, n]); asserts the guard bytes."""
        h = self.buf.cpu().numpy()
        keep = np.zeros(h.size, bool)
        for s in range(self.S):
            keep[self.skew + s * self.stride:self.skew + s * self.stride + self.n] = True
        assert (h[~keep] == GUARD).all(), "bytes outside the frames were written"
        return np.stack([h[self.skew + s * self.stride:self.skew + s * self.stride + self.n] for s in range(self.S)]) \
            if self.S else np.empty((0, self.n), np.uint8)

    def clone(self):
        r = Region(self.S, self.n, self.stride, self.skew)
        r.buf.copy_(self.buf)
        return r


def oracle_tick(frames, states, thr=20):
    """Every stream on its own through the oracle -> (offsets, xs, diff, new states)."""
    offs, xs, df, out = [0], [], [], []
    for s in range(len(frames)):
        eo, x, d, st = po.diff_stream(frames[s][None], states[s], thr)
        assert eo[0] == 0
        offs.append(offs[-1] + int(eo[1])); xs.append(x); df.append(d); out.append(st)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.empty(0, dt)
    return np.array(offs, np.uint32), cat(xs, np.int32), cat(df, np.uint8), out


def arrays_out(S, cap):
    return (torch.full((S + 2,), -5, dtype=torch.int32, device=DEV), torch.full((max(cap, 0) + 64,), -7, dtype=torch.int32, device=DEV),
            torch.full((max(cap, 0) + 64,), GUARD, dtype=torch.uint8, device=DEV))


def read_arrays(out, S, cap):
    """(offsets, xs, diff) cut to min(total, cap); asserts that nothing was written behind them."""
    off = out[0].cpu().numpy().view(np.uint32)
    assert off[S + 1] == np.uint32(-5 & 0xFFFFFFFF)
    tot = min(int(off[S]), cap)
    xs, df = out[1].cpu().numpy(), out[2].cpu().numpy()
    assert (xs[tot:] == -7).all() and (df[tot:] == GUARD).all(), "entries written past the total / the capacity"
    return off[:S + 1], xs[:tot], df[:tot]


def multi(core, fr, st, S=None, cap=None, sync=True):
    """One arrays-form tick on Regions -> (offsets, xs, diff)."""
    S = fr.S if S is None else S
    cap = S * fr.n if cap is None else cap
    out = arrays_out(S, cap)
    torch.cuda.synchronize()   # (the new entry points are not in gpu_util's synced list)
    core.diff_multi_batch(fr.t, st.t, S, out[0], out[1], out[2], cap, stride=fr.stride)
    if not sync:
        return out
    core.synchronize()
    return read_arrays(out, S, cap)


def check_tick(got, want, st, what=""):
    off, xs, df = got
    eo, exs, edf, est = want
    assert np.array_equal(off, eo), what
    assert np.array_equal(xs, exs) and np.array_equal(df, edf), what
    assert np.array_equal(st.get(), np.stack(est)), what


def streams(S, K, w, h, seed0=1):
    """S different streams of K frames: (bases [S][n], frames [K][S][n])."""
    per = [synth.webcam_stream(K, w, h, seed=seed0 + 7 * s) for s in range(S)]
    return [b for b, _ in per], [[per[s][1][k] for s in range(S)] for k in range(K)]


@pytest.mark.parametrize("w,h,S", [(64, 48, 5), (33, 7, 3), (1920, 1080, 8), (3840, 2160, 2)])
def test_ticks_equal_the_oracle_stream_by_stream(w, h, S):
    K, n = 4, 3 * w * h
    assert (w, h) != (33, 7) or n % 16 != 0
    if (w, h) == (3840, 2160):
        # frames and states 2 S N, outputs of a tick 5 S N (twice: the allocator may still hold the tick before), the core's
        # two log sets and buffers about (8 + 3 S) N
        need = (2 * S + 10 * S + 8 + 3 * S) * n
        free = torch.cuda.mem_get_info()[0]
        if free < need:
            pytest.skip(f"the 4K case with S = 2 needs about {need >> 20} MiB of device memory, {free >> 20} MiB are free")
    bases, ticks = streams(S, K, w, h)
    st, fr = Region(S, n).put(bases), Region(S, n)
    with CUDACore(w, h, max_batch=S) as core:
        states = bases
        for k in range(K):
            fr.put(ticks[k])
            want = oracle_tick(ticks[k], states)
            check_tick(multi(core, fr, st), want, st, k)
            states = want[3]
            assert np.array_equal(fr.get(), np.stack(ticks[k]))   # the frames are only read


def test_same_as_one_core_per_stream():
    w, h, S, K = 320, 180, 4, 4
    n = 3 * w * h
    bases, ticks = streams(S, K, w, h, seed0=3)
    st, fr = Region(S, n).put(bases), Region(S, n)
    cores = [CUDACore(w, h, sample_mat_data=bases[s], max_batch=1) for s in range(S)]
    try:
        with CUDACore(w, h, max_batch=S) as core:
            for k in range(K):
                off, xs, df = multi(core, fr.put(ticks[k]), st)
                for s in range(S):
                    o1 = torch.zeros(2, dtype=torch.int32, device=DEV)
                    x1 = torch.empty(n, dtype=torch.int32, device=DEV)
                    d1 = torch.empty(n, dtype=torch.uint8, device=DEV)
                    cores[s].diff_stream_batch(to_dev(ticks[k][s][None]), 1, o1, x1, d1, n)
                    cores[s].synchronize()
                    cnt = int(o1.cpu().numpy().view(np.uint32)[1])
                    a, b = int(off[s]), int(off[s + 1])
                    assert b - a == cnt, (k, s)
                    assert np.array_equal(xs[a:b], x1[:cnt].cpu().numpy()) and np.array_equal(df[a:b], d1[:cnt].cpu().numpy()), (k, s)
                now = st.get()
                for s in range(S):
                    assert np.array_equal(now[s], cores[s].get_state()), (k, s)
    finally:
        for c in cores:
            c.close()


def wire_tick(core, fr, st, S, cap):
    d_off = torch.full((S + 1,), -5, dtype=torch.int32, device=DEV)
    d_wire = torch.full((cap + 64,), GUARD, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    core.diff_multi_wire_batch(fr.t, st.t, S, d_off, d_wire, cap, stride=fr.stride)
    core.synchronize()
    return d_off.cpu().numpy().view(np.uint32), d_wire.cpu().numpy()


def cwire_tick(core, fr, st, S, cap):
    d_off = torch.full((S + 1,), -5, dtype=torch.int32, device=DEV)
    d_pos = torch.full((S + 1,), -3, dtype=torch.int64, device=DEV)
    d_cw = torch.full((cap + 64,), GUARD, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    core.diff_multi_cwire_batch(fr.t, st.t, S, d_off, d_pos, d_cw, cap, stride=fr.stride)
    core.synchronize()
    return d_off.cpu().numpy().view(np.uint32), d_pos.cpu().numpy().view(np.uint64), d_cw.cpu().numpy()


@pytest.mark.parametrize("w,h", [(320, 180), (97, 13)])
def test_the_three_forms_agree(w, h):
    S, n = 5, 3 * w * h
    bases, ticks = streams(S, 2, w, h, seed0=11)
    ticks[1][2] = ticks[0][2]                       # a stream with nothing to send
    st0, fr = Region(S, n).put(bases), Region(S, n)
    with CUDACore(w, h, max_batch=S) as core:
        multi(core, fr.put(ticks[0]), st0)
        fr.put(ticks[1])
        old = st0.get()
        st_a, st_w, st_c = st0, st0.clone(), st0.clone()
        off, xs, df = multi(core, fr, st_a)
        assert off[3] == off[2]
        new = st_a.get()
        # the reference's socket bytes
        want_wire = po.wire_pack(off, xs, df)
        w_off, wire = wire_tick(core, fr, st_w, S, core.wire_bytes(S, int(off[S])))
        assert np.array_equal(w_off, off)
        assert np.array_equal(wire[:want_wire.size], want_wire) and (wire[want_wire.size:] == GUARD).all()
        assert np.array_equal(st_w.get(), new)
        # compact records: the numpy statement of the format, and the library's own encoder on the arrays
        want_cw, wpos = spec.encode(off, xs, df)
        cap = cwire_bytes_max(n, S)
        c_off, c_pos, cw = cwire_tick(core, fr, st_c, S, cap)
        assert np.array_equal(c_off, off) and np.array_equal(c_pos, wpos)
        assert np.array_equal(cw[:want_cw.size], want_cw) and (cw[want_cw.size:] == GUARD).all()
        assert np.array_equal(st_c.get(), new)
        d_pos = torch.zeros(S + 1, dtype=torch.int64, device=DEV)
        d_cw = torch.full((cap,), GUARD, dtype=torch.uint8, device=DEV)
        tot = max(int(off[S]), 1)
        torch.cuda.synchronize()
        core.cwire_encode_batch(to_dev(off.view(np.int32)), to_dev(np.resize(xs, tot)), to_dev(np.resize(df, tot)), int(off[S]), S, d_pos, d_cw, cap)
        core.synchronize()
        assert np.array_equal(d_pos.cpu().numpy().view(np.uint64), wpos)
        assert np.array_equal(d_cw[:want_cw.size].cpu().numpy(), want_cw)
        # a client of stream s applies record s to the state it holds
        for s in range(S):
            client = old[s].copy()
            used = cwire_apply_host(client, want_cw[int(wpos[s]):], 1)
            assert used == int(wpos[s + 1] - wpos[s]) and np.array_equal(client, new[s]), s


def test_regimes_side_by_side():
    """Stream 0 does not change, every byte of stream 1 changes, stream 2 changes at byte 0 and byte N - 1 only, stream 3 is
    dense noise beside the quiet ones, stream 4 is webcam-like."""
    w, h, S = 320, 180, 5
    n = 3 * w * h
    base = [synth.refrand_frame(n, 100 + s) for s in range(S)]
    frames = [base[0].copy(), base[1] ^ np.uint8(0x80), base[2].copy(), synth.refrand_frame(n, 7), None]
    frames[2][0] ^= 0x80
    frames[2][n - 1] ^= 0x80
    base[4], f4 = synth.webcam_stream(1, w, h, seed=5)
    frames[4] = f4[0]
    st, fr = Region(S, n, stride=n + 32).put(base), Region(S, n, stride=n + 32).put(frames)
    with CUDACore(w, h, max_batch=S) as core:
        want = oracle_tick(frames, base)
        got = multi(core, fr, st)
        check_tick(got, want, st)
        off = got[0]
        assert off[1] == 0 and off[2] - off[1] == n and off[3] - off[2] == 2
        assert list(got[1][int(off[2]):int(off[3])]) == [0, n - 1]
        assert np.array_equal(st.get()[0], base[0])
        # the same again: nothing is left to send in the streams that took their frame completely
        again = multi(core, fr, st)
        assert again[0][2] == 0 and again[0][3] == again[0][2]


@pytest.mark.parametrize("thr", [0, 20, 127, 128, 255])
@pytest.mark.parametrize("w,h", [(64, 48), (97, 13)])
def test_thresholds(w, h, thr):
    S, n = 3, 3 * w * h
    base = [synth.refrand_frame(n, 40 + s) for s in range(S)]
    st, fr = Region(S, n).put(base), Region(S, n)
    with CUDACore(w, h, max_batch=S, threshold=thr) as core:
        states = base
        for k in range(2):
            frames = [synth.refrand_frame(n, 60 + 10 * k + s) for s in range(S)]
            frames[1][::3] = (states[1][::3].astype(np.int32) + thr).astype(np.uint8)        # |df| == thr: not flagged
            frames[1][1::3] = (states[1][1::3].astype(np.int32) - thr - 1).astype(np.uint8)  # |df| == thr + 1 (mod 256)
            want = oracle_tick(frames, states, thr)
            check_tick(multi(core, fr.put(frames), st), want, st, (thr, k))
            states = want[3]


@pytest.mark.parametrize("w,h,pad,skew_f,skew_s", [(64, 48, 48, 0, 0), (64, 48, 37, 0, 0), (64, 48, 16, 3, 5), (211, 3, 5, 1, 9),
                                                   (640, 360, 64, 0, 0), (640, 360, 16, 16, 7)])
def test_strides_gaps_and_unaligned_pointers(w, h, pad, skew_f, skew_s):
    S, n = 4, 3 * w * h
    bases, ticks = streams(S, 2, w, h, seed0=21)
    st, fr = Region(S, n, n + pad, skew_s).put(bases), Region(S, n, n + pad, skew_f)
    with CUDACore(w, h, max_batch=S + 1) as core:
        states = bases
        for k in range(2):
            want = oracle_tick(ticks[k], states)
            check_tick(multi(core, fr.put(ticks[k]), st), want, st, k)   # (Region.get asserts the gap bytes)
            fr.get()
            states = want[3]


def test_capacity_smaller_than_the_total():
    w, h, S = 160, 90, 4
    n = 3 * w * h
    bases, ticks = streams(S, 2, w, h, seed0=31)
    with CUDACore(w, h, max_batch=S) as core:
        fr = Region(S, n).put(ticks[0])
        eo, exs, edf, est = oracle_tick(ticks[0], bases)
        total = int(eo[S])
        assert total > 8
        for cap in (0, 1, int(eo[2]) - 1, int(eo[2]), total - 1):
            st = Region(S, n).put(bases)
            off, xs, df = multi(core, fr, st, cap=cap)       # (read_arrays: nothing behind min(total, cap))
            assert np.array_equal(off, eo), cap
            assert np.array_equal(xs, exs[:cap]) and np.array_equal(df, edf[:cap]), cap
            assert np.array_equal(st.get(), np.stack(est)), cap            # the states advance completely
            want2 = oracle_tick(ticks[1], est)
            check_tick(multi(core, Region(S, n).put(ticks[1]), st), want2, st, cap)
        # wire: a stream that does not fit is dropped whole
        wire = po.wire_pack(eo, exs, edf)
        ends = [4 * (s + 1) + 5 * int(eo[s + 1]) for s in range(S)]
        for cap in (ends[1], ends[2] - 1, ends[3] - 1):
            st = Region(S, n).put(bases)
            w_off, got = wire_tick(core, fr, st, S, cap)
            fit = max([e for e in ends if e <= cap] + [0])
            assert np.array_equal(w_off, eo), cap
            assert np.array_equal(got[:fit], wire[:fit]) and (got[cap:] == GUARD).all(), cap
            assert np.array_equal(st.get(), np.stack(est)), cap
        # compact: whole records are skipped, header included
        want_cw, wpos = spec.encode(eo, exs, edf)
        for cap in (0, 7, int(wpos[2]) - 1, int(wpos[2]), int(wpos[S]) - 1):
            st = Region(S, n).put(bases)
            c_off, c_pos, got = cwire_tick(core, fr, st, S, cap)
            assert np.array_equal(c_off, eo) and np.array_equal(c_pos, wpos), cap
            fit = int(wpos[np.searchsorted(wpos, cap, side="right") - 1])
            assert np.array_equal(got[:fit], want_cw[:fit]) and (got[fit:] == GUARD).all(), cap
            assert np.array_equal(st.get(), np.stack(est)), cap


def download(core, d_tensor, nbytes):
    out = np.empty(nbytes, np.uint8)
    lib.check(core._lib.mi355_download(core._h, out.ctypes.data, C.c_void_p(d_tensor.data_ptr()), nbytes))
    return out


@pytest.mark.parametrize("mode", ["own", "sequential", "callers"])
@pytest.mark.parametrize("w,h", [(64, 48), (640, 360), (1920, 1080)])
def test_ticks_back_to_back_without_synchronisation(w, h, mode):
    """Three ticks on the same states with nothing in between (640x360 and 1080p: every pipelined pack is split over two
    streams), then the download of one state straight behind the last tick."""
    S, K = 3, 3
    n = 3 * w * h
    bases, ticks = streams(S, K, w, h, seed0=41)
    st = Region(S, n).put(bases)
    frs = [Region(S, n).put(ticks[k]) for k in range(K)]
    outs = [arrays_out(S, S * n) for _ in range(K)]
    with CUDACore(w, h, max_batch=S) as core:
        if mode == "sequential":
            core.set_option(lib.OPT_PIPELINE, 0)
        if mode == "callers":
            core.use_torch_stream()
        torch.cuda.synchronize()
        for k in range(K):
            core.diff_multi_batch(frs[k].t, st.t, S, outs[k][0], outs[k][1], outs[k][2], S * n)
        last = download(core, st.t[n:], n)          # state of stream 1, no synchronisation in front
        core.synchronize()
        torch.cuda.synchronize()
        states = bases
        for k in range(K):
            want = oracle_tick(ticks[k], states)
            off, xs, df = read_arrays(outs[k], S, S * n)
            assert np.array_equal(off, want[0]) and np.array_equal(xs, want[1]) and np.array_equal(df, want[2]), k
            states = want[3]
        assert np.array_equal(st.get(), np.stack(states))
        assert np.array_equal(last, states[1])


def test_a_tick_then_other_readers_of_the_states():
    """A split tick, then -- with no synchronisation -- mi355_diff_pairs_batch that reads the states at another tile
    position (one stream further), and a tick on states that overlap the first ones.  A race test: with the wait for the
    tick's parts missing (core.hip, run_batch) it may still pass; it is a smoke check of that schedule, not a proof."""
    w, h, S = 640, 360, 3
    n = 3 * w * h
    bases, ticks = streams(S + 1, 2, w, h, seed0=51)
    st = Region(S + 1, n).put(bases)
    fr0, fr1 = Region(S, n).put(ticks[0][:S]), Region(S, n).put(ticks[1][:S])
    out0, outp, out1 = arrays_out(S, S * n), arrays_out(S, S * n), arrays_out(S, S * n)
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        core.diff_multi_batch(fr0.t, st.t, S, out0[0], out0[1], out0[2], S * n)
        core.diff_pairs_batch(fr1.t, st.t[n:], S, outp[0], outp[1], outp[2], S * n)      # prev = states 1 .. S
        core.diff_multi_batch(fr1.t, st.t[n:], S, out1[0], out1[1], out1[2], S * n)      # states 1 .. S
        core.synchronize()
    w0 = oracle_tick(ticks[0][:S], bases[:S])
    mid = list(w0[3]) + [bases[S]]
    check = read_arrays(out0, S, S * n)
    assert np.array_equal(check[0], w0[0]) and np.array_equal(check[1], w0[1])
    wp = oracle_tick(ticks[1][:S], mid[1:])          # what the pairs see: no feedback, same entries as the tick below
    gp, g1 = read_arrays(outp, S, S * n), read_arrays(out1, S, S * n)
    for got in (gp, g1):
        assert np.array_equal(got[0], wp[0]) and np.array_equal(got[1], wp[1]) and np.array_equal(got[2], wp[2])
    assert np.array_equal(st.get(), np.stack([mid[0]] + list(wp[3])))


def test_the_cores_own_state_is_not_involved():
    w, h, S = 320, 180, 3
    n = 3 * w * h
    bases, ticks = streams(S, 2, w, h, seed0=61)
    own_base, own_frames = synth.webcam_stream(2, w, h, seed=99)
    st, fr = Region(S, n).put(bases), Region(S, n)
    with CUDACore(w, h, sample_mat_data=own_base, max_batch=S) as core:
        w0 = oracle_tick(ticks[0], bases)
        check_tick(multi(core, fr.put(ticks[0]), st), w0, st)
        assert np.array_equal(core.get_state(), own_base)
        for tick in (wire_tick, cwire_tick):                      # the other two forms, on copies of the states
            other = Region(S, n).put(bases)
            tick(core, fr, other, S, cwire_bytes_max(n, S))
            assert np.array_equal(other.get(), np.stack(w0[3]))
            assert np.array_equal(core.get_state(), own_base)
        # a batch of the core's own stream between two ticks disturbs neither
        o = torch.zeros(3, dtype=torch.int32, device=DEV)
        x = torch.empty(2 * n, dtype=torch.int32, device=DEV)
        d = torch.empty(2 * n, dtype=torch.uint8, device=DEV)
        core.diff_stream_batch(to_dev(own_frames), 2, o, x, d, 2 * n)
        w1 = oracle_tick(ticks[1], w0[3])
        check_tick(multi(core, fr.put(ticks[1]), st), w1, st)
        eo, exs, edf, est = po.diff_stream(own_frames, own_base)
        assert np.array_equal(o.cpu().numpy().view(np.uint32), eo)
        assert np.array_equal(x[:int(eo[-1])].cpu().numpy(), exs) and np.array_equal(d[:int(eo[-1])].cpu().numpy(), edf)
        assert np.array_equal(core.get_state(), est)


def test_no_streams():
    w, h = 64, 48
    n = 3 * w * h
    st, fr = Region(2, n), Region(2, n)
    with CUDACore(w, h, max_batch=2) as core:
        off, xs, df = multi(core, fr, st, S=0, cap=16)
        assert list(off) == [0] and xs.size == 0
        w_off, wire = wire_tick(core, fr, st, 0, 16)
        assert w_off[0] == 0 and (wire == GUARD).all()
        c_off, c_pos, cw = cwire_tick(core, fr, st, 0, 16)
        assert c_off[0] == 0 and c_pos[0] == 0 and (cw == GUARD).all()
        core.diff_multi_batch(None, None, 0, torch.zeros(1, dtype=torch.int32, device=DEV), None, None, 0)
        core.synchronize()
    st.get(), fr.get()


def test_refusals_write_nothing():
    w, h, S = 64, 48, 3
    n = 3 * w * h
    bases, ticks = streams(S, 1, w, h)
    both = Region(2 * S, n).put(list(ticks[0]) + list(bases))      # frames, then states, in ONE buffer
    f, s = both.t, both.t[S * n:]
    cap = S * n
    out = arrays_out(S, cap)
    d_pos = torch.full((S + 2,), -3, dtype=torch.int64, device=DEV)
    d_bytes = torch.full((cwire_bytes_max(n, S) + 64,), GUARD, dtype=torch.uint8, device=DEV)
    o, x, d, p, b = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), d_pos.data_ptr(), d_bytes.data_ptr()
    with CUDACore(w, h, sample_mat_data=bases[0], max_batch=S) as core:
        arrays = [
            (None, s, S, o, x, d, cap), (f, None, S, o, x, d, cap),                          # null frames / states
            (f, s, S + 1, o, x, d, cap), (f, s, -1, o, x, d, cap),                           # nstreams outside [0, max_batch]
            (f, s, S, None, x, d, cap), (f, s, S, o, None, d, cap), (f, s, S, o, x, None, cap),   # the single-stream form's
        ]
        overlaps = [f, f[n - 1:], f[(S - 1) * n + n - 1:], f[n:]]                            # states inside / across the frames
        torch.cuda.synchronize()
        for args in arrays:
            with pytest.raises(lib.Mi355Error) as e:
                core.diff_multi_batch(*args)
            assert e.value.code == lib.ERR_INVALID and str(e.value).split(":", 1)[1].strip(), args[2:]
        for call in (lambda: core.diff_multi_batch(f, s, S, o, x, d, cap, stride=n - 1),        # stride < N, every form
                     lambda: core.diff_multi_wire_batch(f, s, S, o, b, cap, stride=n - 1),
                     lambda: core.diff_multi_cwire_batch(f, s, S, o, p, b, cap, stride=n - 1)):
            with pytest.raises(lib.Mi355Error) as e:
                call()
            assert e.value.code == lib.ERR_INVALID and "stride" in str(e.value)
        for ov in overlaps:
            for call in (lambda: core.diff_multi_batch(f, ov, S, o, x, d, cap),
                         lambda: core.diff_multi_batch(ov, f, S, o, x, d, cap),
                         lambda: core.diff_multi_wire_batch(f, ov, S, o, b, cap),
                         lambda: core.diff_multi_cwire_batch(f, ov, S, o, p, b, cap)):
                with pytest.raises(lib.Mi355Error) as e:
                    call()
                assert e.value.code == lib.ERR_INVALID and "overlap" in str(e.value)
        for args in [(f, s, S, o, None, cap), (f, s, S, None, b, cap), (None, s, S, o, b, cap)]:
            with pytest.raises(lib.Mi355Error) as e:
                core.diff_multi_wire_batch(*args)
            assert e.value.code == lib.ERR_INVALID
        for args in [(f, s, S, None, p, b, cap), (f, s, S, o, None, b, cap), (f, s, S, o, p, None, cap), (f, None, S, o, p, b, cap),
                     (f, s, S, o, p, b + 1, cap), (f, s, S, o + 2, p, b, cap), (f, s, S, o, p + 4, b, cap), (f, s, S + 1, o, p, b, cap)]:
            with pytest.raises(lib.Mi355Error) as e:
                core.diff_multi_cwire_batch(*args)
            assert e.value.code == lib.ERR_INVALID, args[2:]
        core.synchronize()
        assert np.array_equal(core.get_state(), bases[0])
    assert (out[0].cpu().numpy() == -5).all() and (out[1].cpu().numpy() == -7).all() and (out[2].cpu().numpy() == GUARD).all()
    assert (d_pos.cpu().numpy() == -3).all() and (d_bytes.cpu().numpy() == GUARD).all()
    assert np.array_equal(both.get(), np.stack(list(ticks[0]) + list(bases)))

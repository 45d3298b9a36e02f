"""-m gpu: mi355_diff_multi_stream_batch / _wire_batch / _cwire_batch -- T frames of each of S streams per call, the states in
the caller's memory, batch index b = s*T + t (include/mi355diff.h, "many streams, many frames each").  Everything is compared
bit for bit: with the oracle stream by stream, with the stream form on S cores, with the multi form, and the three output
forms with each other.  Frames and states live in guarded regions (gpu_util.Region): every byte outside them is checked."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, cwire_frame_bytes, lib, synth
from oracle import pyoracle as po
from gpu_util import DEV, GUARD, CUDACore, Guarded, Region, to_dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def sequences(S, T, w, h, seed0=1, calls=1):
    """S different webcam-like streams of calls*T frames: (bases [S][n], frames [calls][S][T][n]); read-only."""
    per = []
    for s in range(S):                                  # (made on the device: the same bytes, much sooner at 1080p)
        base, frames = synth.webcam_stream(calls * T, w, h, seed=seed0 + 7 * s, device=DEV)
        per.append((base.cpu().numpy(), frames.cpu().numpy()))
        per[-1][0].setflags(write=False)
        per[-1][1].setflags(write=False)
    return [b for b, _ in per], [[[per[s][1][c * T + t] for t in range(T)] for s in range(S)] for c in range(calls)]


def oracle_call(frames, states, thr=20):
    """Every stream on its own through the oracle, concatenated in stream order ->
    (offsets [S*T + 1], xs, diff, new states [S][n])."""
    offs, xs, df, out = [np.zeros(1, np.int64)], [], [], []
    for s in range(len(frames)):
        eo, x, d, st = po.diff_stream(np.stack(frames[s]), states[s], thr)
        offs.append(offs[-1][-1] + eo[1:].astype(np.int64)); xs.append(x); df.append(d); out.append(st)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.empty(0, dt)
    return np.concatenate(offs).astype(np.uint32), cat(xs, np.int32), cat(df, np.uint8), out


@functools.lru_cache(maxsize=None)
def oracle_run(S, T, w, h, seed0=1, calls=1, thr=20):
    """`calls` calls in a row on the same states -> [(offsets, xs, diff, states)] per call; computed once per shape."""
    bases, frames = sequences(S, T, w, h, seed0, calls)
    out, states = [], bases
    for c in range(calls):
        out.append(oracle_call(frames[c], states, thr))
        states = out[-1][3]
    return out


def rows(frames):
    """[S][T][n] -> the S*T rows of the frames' region, stream-major."""
    return [f for per_stream in frames for f in per_stream]


class Arrays:
    def __init__(self, B, cap):
        self.B, self.cap = B, cap
        self.off, self.xs, self.df = Guarded(B + 1, torch.int32), Guarded(cap, torch.int32), Guarded(cap, torch.uint8)

    def read(self):
        """(offsets, xs, diff) cut to min(total, cap); asserts that nothing was written behind them."""
        off = self.off.get().view(np.uint32)
        tot = min(int(off[self.B]), self.cap)
        return off, self.xs.get(tot)[:tot], self.df.get(tot)[:tot]


def call_arrays(core, fr, st, S, T, cap=None, sync=True):
    cap = S * T * fr.n if cap is None else cap
    out = Arrays(S * T, cap)
    torch.cuda.synchronize()
    core.diff_multi_stream_batch(fr.ptr, st.ptr, S, T, out.off.ptr, out.xs.ptr, out.df.ptr, cap, stride=fr.stride)
    if not sync:
        return out
    core.synchronize()
    return out.read()


def call_wire(core, fr, st, S, T, cap):
    off, wire = Guarded(S * T + 1, torch.int32), Guarded(cap)
    torch.cuda.synchronize()
    core.diff_multi_stream_wire_batch(fr.ptr, st.ptr, S, T, off.ptr, wire.ptr, cap, stride=fr.stride)
    core.synchronize()
    return off.get().view(np.uint32), wire.get()


def call_cwire(core, fr, st, S, T, cap):
    off, pos, cw = Guarded(S * T + 1, torch.int32), Guarded(S * T + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.diff_multi_stream_cwire_batch(fr.ptr, st.ptr, S, T, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
    core.synchronize()
    return off.get().view(np.uint32), pos.get().view(np.uint64), cw.get()


def check_call(got, want, st, what=""):
    off, xs, df = got
    eo, exs, edf, est = want
    assert np.array_equal(off, eo), what
    assert np.array_equal(xs, exs) and np.array_equal(df, edf), what
    assert np.array_equal(st.get(), np.stack(est)), what


# 1. the oracle, over the shapes where the exchange can go wrong: an exchange at every frame, inside the first and the second
# register group (4 frames each) and on a group boundary; a ragged tile; the pipelined split (64 tiles and more); 1080p
SHAPES = [(64, 48, S, T) for S, T in [(1, 7), (3, 1), (3, 2), (2, 3), (3, 4), (2, 5), (2, 8), (2, 9)]] + \
         [(33, 7, 3, 5), (160, 140, 2, 6), (1920, 1080, 3, 5)]


@pytest.mark.parametrize("w,h,S,T", SHAPES)
def test_two_calls_equal_the_oracle_stream_by_stream(w, h, S, T):
    n = 3 * w * h
    assert (w, h) != (33, 7) or n % 16 != 0
    bases, frames = sequences(S, T, w, h, 1, 2)
    want = oracle_run(S, T, w, h, 1, 2)
    assert int(want[0][0][-1]) > 0 and int(want[1][0][-1]) > 0
    st = Region(S, n).put(bases)
    with CUDACore(w, h, max_batch=S * T) as core:
        for c in range(2):
            fr = Region(S * T, n).put(rows(frames[c]))
            check_call(call_arrays(core, fr, st, S, T), want[c], st, c)
            assert np.array_equal(fr.get(), np.stack(rows(frames[c])))   # the frames are only read


# 2. both forms of the compare
@pytest.mark.parametrize("thr", [0, 20, 127, 128, 255])
def test_thresholds(thr):
    w, h, S, T = 64, 48, 2, 5
    n = 3 * w * h
    bases, frames = sequences(S, T, w, h, 5)
    want = oracle_run(S, T, w, h, 5, 1, thr)[0]
    st, fr = Region(S, n).put(bases), Region(S * T, n).put(rows(frames[0]))
    with CUDACore(w, h, max_batch=S * T, threshold=thr) as core:
        check_call(call_arrays(core, fr, st, S, T), want, st, thr)


# 3. the byte path: a stride that is no multiple of 16, pointers 3 bytes behind an aligned address
@pytest.mark.parametrize("skew_f,skew_s", [(3, 0), (0, 3), (3, 3)])
def test_byte_path_strides_and_unaligned_pointers(skew_f, skew_s):
    w, h, S, T = 64, 48, 2, 5
    n = 3 * w * h
    bases, frames = sequences(S, T, w, h, 1, 2)
    want = oracle_run(S, T, w, h, 1, 2)
    st = Region(S, n, n + 5, skew_s).put(bases)
    with CUDACore(w, h, max_batch=S * T) as core:
        for c in range(2):
            fr = Region(S * T, n, n + 5, skew_f).put(rows(frames[c]))
            check_call(call_arrays(core, fr, st, S, T), want[c], st, c)   # (Region.get asserts the gaps of the stride)
            assert np.array_equal(fr.get(), np.stack(rows(frames[c])))


# 4. the three forms agree
@pytest.mark.parametrize("w,h", [(160, 140), (33, 7)])
def test_the_three_forms_agree(w, h):
    S, T, n = 3, 5, 3 * w * h
    B = S * T
    bases, frames = sequences(S, T, w, h, 11)
    fr = Region(B, n).put(rows(frames[0]))
    st_a, st_w, st_c = (Region(S, n).put(bases) for _ in range(3))
    with CUDACore(w, h, max_batch=B) as core:
        off, xs, df = call_arrays(core, fr, st_a, S, T)
        new = st_a.get()
        assert np.array_equal(off, oracle_run(S, T, w, h, 11)[0][0])
        # the sender's bytes: u32 n | i32 xs | u8 diff per batch index
        want_wire = po.wire_pack(off, xs, df)
        w_off, wire = call_wire(core, fr, st_w, S, T, core.wire_bytes(B, int(off[B])))
        assert np.array_equal(w_off, off) and np.array_equal(wire, want_wire)
        for b in range(B):
            at = 4 * b + 5 * int(off[b])
            assert int(wire[at:at + 4].view("<u4")[0]) == int(off[b + 1]) - int(off[b]), b
        assert np.array_equal(st_w.get(), new)
        # compact records: the library's own encoder on the arrays form, byte for byte
        cap = cwire_bytes_max(n, B)
        e_pos, e_cw = Guarded(B + 1, torch.int64), Guarded(cap)
        tot = max(int(off[B]), 1)
        torch.cuda.synchronize()
        core.cwire_encode_batch(to_dev(off.view(np.int32)), to_dev(np.resize(xs, tot)), to_dev(np.resize(df, tot)), int(off[B]), B,
                                e_pos.ptr, e_cw.ptr, cap)
        core.synchronize()
        want_pos, want_cw = e_pos.get().view(np.uint64), e_cw.get()
        c_off, c_pos, cw = call_cwire(core, fr, st_c, S, T, cap)
        assert np.array_equal(c_off, off) and np.array_equal(c_pos, want_pos)
        used = int(want_pos[B])
        assert np.array_equal(cw[:used], want_cw[:used]) and (cw[used:] == GUARD).all()
        assert np.array_equal(st_c.get(), new)
        counts, escapes = spec.headers(cw, B)
        sizes = [cwire_frame_bytes(int(c), int(e)) for c, e in zip(counts, escapes)]
        assert np.array_equal(c_pos, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
        assert np.array_equal(counts, np.diff(off.astype(np.int64)))
        # a client of stream s applies that stream's slice -- T records back to back -- to the base it holds
        for s in range(S):
            client = bases[s].copy()
            a, b = int(c_pos[s * T]), int(c_pos[(s + 1) * T])
            assert cwire_apply_host(client, cw[a:b], T) == b - a and np.array_equal(client, new[s]), s


# 5. equal to what exists
def stream_core_run(core, frames_s, n):
    T = len(frames_s)
    out = Arrays(T, T * n)
    core.diff_stream_batch(to_dev(np.stack(frames_s)), T, out.off.ptr, out.xs.ptr, out.df.ptr, T * n)
    core.synchronize()
    return out.read()


def test_same_as_the_stream_form_on_one_core_per_stream():
    w, h, S, T = 160, 140, 3, 6
    n = 3 * w * h
    bases, frames = sequences(S, T, w, h, 3)
    st, fr = Region(S, n).put(bases), Region(S * T, n).put(rows(frames[0]))
    with CUDACore(w, h, max_batch=S * T) as core:
        off, xs, df = call_arrays(core, fr, st, S, T)
    now = st.get()
    for s in range(S):
        with CUDACore(w, h, sample_mat_data=bases[s], max_batch=T) as one:
            o1, x1, d1 = stream_core_run(one, frames[0][s], n)
            a, b = int(off[s * T]), int(off[(s + 1) * T])
            assert np.array_equal(off[s * T:(s + 1) * T + 1].astype(np.int64) - a, o1[:T + 1].astype(np.int64)), s
            assert np.array_equal(xs[a:b], x1) and np.array_equal(df[a:b], d1), s
            assert np.array_equal(now[s], one.get_state()), s


def test_one_stream_is_the_stream_form_on_a_caller_held_state():
    w, h, T = 160, 140, 7
    n = 3 * w * h
    bases, frames = sequences(1, T, w, h, 9)
    own = synth.refrand_frame(n, 77)
    st, fr = Region(1, n).put(bases), Region(T, n).put(rows(frames[0]))
    with CUDACore(w, h, sample_mat_data=own, max_batch=T) as core:
        got = call_arrays(core, fr, st, 1, T)
        assert np.array_equal(core.get_state(), own)          # the core's own state is not involved
        with CUDACore(w, h, sample_mat_data=bases[0], max_batch=T) as one:
            o1, x1, d1 = stream_core_run(one, frames[0][0], n)
            assert np.array_equal(got[0], o1) and np.array_equal(got[1], x1) and np.array_equal(got[2], d1)
            assert np.array_equal(st.get()[0], one.get_state())


def multi_tick(core, fr, st, S, n):
    out = Arrays(S, S * n)
    torch.cuda.synchronize()
    core.diff_multi_batch(fr.ptr, st.ptr, S, out.off.ptr, out.xs.ptr, out.df.ptr, S * n, stride=fr.stride)
    core.synchronize()
    return out.read()


def test_one_frame_per_stream_is_the_multi_form():
    w, h, S = 160, 140, 4
    n = 3 * w * h
    bases, frames = sequences(S, 1, w, h, 13)
    fr = Region(S, n).put(rows(frames[0]))
    st, st_m = Region(S, n).put(bases), Region(S, n).put(bases)
    with CUDACore(w, h, max_batch=S) as core:
        got = call_arrays(core, fr, st, S, 1)
        want = multi_tick(core, fr, st_m, S, n)
        assert all(np.array_equal(g, x) for g, x in zip(got, want))
        assert np.array_equal(st.get(), st_m.get())


def test_same_as_tick_major_calls_of_the_multi_form():
    w, h, S, T = 160, 140, 3, 5
    n = 3 * w * h
    bases, frames = sequences(S, T, w, h, 17)
    fr = Region(S * T, n).put(rows(frames[0]))
    st, st_m = Region(S, n).put(bases), Region(S, n).put(bases)
    with CUDACore(w, h, max_batch=S * T) as core:
        off, xs, df = call_arrays(core, fr, st, S, T)
        ticks = [multi_tick(core, Region(S, n).put([frames[0][s][t] for s in range(S)]), st_m, S, n) for t in range(T)]
    assert np.array_equal(st.get(), st_m.get())
    for s in range(S):
        for t in range(T):
            a, b = int(off[s * T + t]), int(off[s * T + t + 1])
            o, x, d = ticks[t]
            assert np.array_equal(xs[a:b], x[int(o[s]):int(o[s + 1])]) and np.array_equal(df[a:b], d[int(o[s]):int(o[s + 1])]), (s, t)


# 6. capacity
def test_capacity_smaller_than_the_total():
    w, h, S, T = 64, 48, 3, 3
    n, B = 3 * w * h, 9
    bases, frames = sequences(S, T, w, h, 31, 2)
    (eo, exs, edf, est), want2 = oracle_run(S, T, w, h, 31, 2)
    total = int(eo[B])
    assert total > 8 and eo[T + 2] > eo[T + 1] > eo[T]
    fr, fr2 = Region(B, n).put(rows(frames[0])), Region(B, n).put(rows(frames[1]))
    with CUDACore(w, h, max_batch=B) as core:
        for cap in (0, 1, int(eo[T + 1]) - 1, total - 1):
            st = Region(S, n).put(bases)
            off, xs, df = call_arrays(core, fr, st, S, T, cap=cap)     # (Arrays.read: nothing behind min(total, cap))
            assert np.array_equal(off, eo), cap
            assert np.array_equal(xs, exs[:cap]) and np.array_equal(df, edf[:cap]), cap
            assert np.array_equal(st.get(), np.stack(est)), cap      # the states advance completely
            check_call(call_arrays(core, fr2, st, S, T), want2, st, cap)
        # wire: a frame that does not fit is dropped whole; the cut falls inside stream 1
        wire = po.wire_pack(eo, exs, edf)
        ends = [4 * (b + 1) + 5 * int(eo[b + 1]) for b in range(B)]
        for cap in (ends[T], ends[T + 1] - 1, ends[2 * T - 1] - 1):
            st = Region(S, n).put(bases)
            w_off, got = call_wire(core, fr, st, S, T, cap)
            fit = max([e for e in ends if e <= cap] + [0])
            assert ends[T - 1] <= fit < ends[2 * T - 1]
            assert np.array_equal(w_off, eo), cap
            assert np.array_equal(got[:fit], wire[:fit]), cap
            assert np.array_equal(st.get(), np.stack(est)), cap
        # compact: whole records are skipped, header included
        want_cw, wpos = spec.encode(eo, exs, edf)
        for cap in (int(wpos[T + 1]) - 1, int(wpos[T + 1]), int(wpos[2 * T]) - 1):
            st = Region(S, n).put(bases)
            c_off, c_pos, got = call_cwire(core, fr, st, S, T, cap)
            assert np.array_equal(c_off, eo) and np.array_equal(c_pos, wpos), cap
            fit = int(wpos[np.searchsorted(wpos, cap, side="right") - 1])
            assert np.array_equal(got[:fit], want_cw[:fit]) and (got[fit:] == GUARD).all(), cap
            assert np.array_equal(st.get(), np.stack(est)), cap


# 7. refusals
def test_refusals_write_nothing_and_the_bounds_are_accepted():
    w, h, S, T = 64, 48, 2, 3
    n, B = 3 * w * h, 6
    bases, frames = sequences(S, T, w, h, 1)
    both = Region(B + S, n).put(rows(frames[0]) + list(bases))      # frames, then states, in ONE buffer
    f, s = both.ptr, both.ptr + B * n
    cap = B * n
    out = Arrays(B, cap)
    pos, by = Guarded(B + 1, torch.int64), Guarded(cwire_bytes_max(n, B))
    o, x, d, p, b = out.off.ptr, out.xs.ptr, out.df.ptr, pos.ptr, by.ptr
    with CUDACore(w, h, sample_mat_data=bases[0], max_batch=B) as core:
        forms = [lambda F, St, s_, t_, stride=None: core.diff_multi_stream_batch(F, St, s_, t_, o, x, d, cap, stride=stride),
                 lambda F, St, s_, t_, stride=None: core.diff_multi_stream_wire_batch(F, St, s_, t_, o, b, cap, stride=stride),
                 lambda F, St, s_, t_, stride=None: core.diff_multi_stream_cwire_batch(F, St, s_, t_, o, p, b, cap, stride=stride)]
        bad = [(f, s, B + 1, 1, None), (f, s, 1, B + 1, None), (f, s, S + 1, T, None), (f, s, 65536, 65536, None),   # S*T > max_batch
               (f, s, -1, T, None), (f, s, S, -1, None), (f, s, -1, -1, None),                                       # negative
               (f, s, S, T, n - 1),                                                                                  # stride < N
               (f, f, S, T, None), (f, f + n - 1, S, T, None), (f, f + (B - 1) * n + n - 1, S, T, None),             # states in / across the frames
               (f + (S - 1) * n + n - 1, f, S, T, None),                                                             # frames that begin in the last state
               (None, s, S, T, None), (f, None, S, T, None)]                                                         # null with S*T > 0
        torch.cuda.synchronize()
        for form in forms:
            for args in bad:
                with pytest.raises(lib.Mi355Error) as e:
                    form(*args)
                assert e.value.code == lib.ERR_INVALID and str(e.value).split(":", 1)[1].strip(), args[2:]
        singles = [lambda: core.diff_multi_stream_batch(f, s, S, T, None, x, d, cap), lambda: core.diff_multi_stream_batch(f, s, S, T, o, None, d, cap),
                   lambda: core.diff_multi_stream_batch(f, s, S, T, o, x, None, cap), lambda: core.diff_multi_stream_wire_batch(f, s, S, T, o, None, cap),
                   lambda: core.diff_multi_stream_wire_batch(f, s, S, T, None, b, cap), lambda: core.diff_multi_stream_cwire_batch(f, s, S, T, None, p, b, cap),
                   lambda: core.diff_multi_stream_cwire_batch(f, s, S, T, o, None, b, cap), lambda: core.diff_multi_stream_cwire_batch(f, s, S, T, o, p, None, cap),
                   lambda: core.diff_multi_stream_cwire_batch(f, s, S, T, o, p, b + 1, cap), lambda: core.diff_multi_stream_cwire_batch(f, s, S, T, o + 2, p, b, cap),
                   lambda: core.diff_multi_stream_cwire_batch(f, s, S, T, o, p + 4, b, cap)]
        for call in singles:                                         # what the single-stream form of the same output refuses
            with pytest.raises(lib.Mi355Error) as e:
                call()
            assert e.value.code == lib.ERR_INVALID
        core.synchronize()
        assert np.array_equal(core.get_state(), bases[0])
        assert (out.off.get() == -7).all() and (out.xs.get() == -7).all() and (out.df.get() == GUARD).all()
        assert (pos.get() == -3).all() and (by.get() == GUARD).all()
        assert np.array_equal(both.get(), np.stack(rows(frames[0]) + list(bases)))
        # S*T == 0: offsets[0] (and frame_pos[0]) and nothing else, whatever the other arguments
        for s_, t_ in [(0, T), (S, 0), (0, 0)]:
            e_off, e_pos, e_by = Guarded(1, torch.int32), Guarded(1, torch.int64), Guarded(64)
            core.diff_multi_stream_batch(None, None, s_, t_, e_off.ptr, x, d, cap)
            core.synchronize()
            assert list(e_off.get()) == [0]
            e_off = Guarded(1, torch.int32)
            core.diff_multi_stream_wire_batch(f, s, s_, t_, e_off.ptr, e_by.ptr, 64)
            core.synchronize()
            assert list(e_off.get()) == [0] and (e_by.get() == GUARD).all()
            e_off = Guarded(1, torch.int32)
            core.diff_multi_stream_cwire_batch(f, s, s_, t_, e_off.ptr, e_pos.ptr, e_by.ptr, 64)
            core.synchronize()
            assert list(e_off.get()) == [0] and list(e_pos.get()) == [0] and (e_by.get() == GUARD).all()
        assert (out.xs.get() == -7).all() and (out.df.get() == GUARD).all()
        assert np.array_equal(both.get(), np.stack(rows(frames[0]) + list(bases)))
        # S*T == max_batch is accepted, in both factorings that are no single stream
        want = oracle_run(S, T, w, h, 1)[0]
        st = Region(S, n).put(bases)
        check_call(call_arrays(core, Region(B, n).put(rows(frames[0])), st, S, T), want, st)
        assert np.array_equal(core.get_state(), bases[0])


# 8. ordering without synchronisation (160x140: 66 tiles, every pipelined pack is split over two streams)
def download(core, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    lib.check(core._lib.mi355_download(core._h, out.ctypes.data, C.c_void_p(ptr), nbytes))
    return out


@pytest.mark.parametrize("mode", ["own", "sequential", "callers"])
def test_calls_back_to_back_without_synchronisation(mode):
    """Three calls on the same states with nothing in between, then the download of one state straight behind the last."""
    w, h, S, T, K = 160, 140, 2, 6, 3
    n, B = 3 * w * h, 12
    bases, frames = sequences(S, T, w, h, 41, K)
    want = oracle_run(S, T, w, h, 41, K)
    st = Region(S, n).put(bases)
    frs = [Region(B, n).put(rows(frames[k])) for k in range(K)]
    outs = [Arrays(B, B * n) for _ in range(K)]
    with CUDACore(w, h, max_batch=B) as core:
        if mode == "sequential":
            core.set_option(lib.OPT_PIPELINE, 0)
        if mode == "callers":
            core.use_torch_stream()
        torch.cuda.synchronize()
        for k in range(K):
            core.diff_multi_stream_batch(frs[k].ptr, st.ptr, S, T, outs[k].off.ptr, outs[k].xs.ptr, outs[k].df.ptr, B * n)
        last = download(core, st.ptr + n, n)          # state of stream 1, no synchronisation in front
        core.synchronize()
        torch.cuda.synchronize()
        for k in range(K):
            off, xs, df = outs[k].read()
            assert np.array_equal(off, want[k][0]) and np.array_equal(xs, want[k][1]) and np.array_equal(df, want[k][2]), k
        assert np.array_equal(st.get(), np.stack(want[K - 1][3]))
        assert np.array_equal(last, want[K - 1][3][1])


@pytest.mark.parametrize("mode", ["own", "sequential", "callers"])
def test_alternating_with_the_multi_form_without_synchronisation(mode):
    """A call, then mi355_diff_multi_batch on the same states, then a call again: the states pass from one form to the other
    with no synchronisation."""
    w, h, S, T = 160, 140, 2, 6
    n, B = 3 * w * h, 12
    bases, frames = sequences(S, T, w, h, 41, 3)
    tick = [frames[1][s][0] for s in range(S)]                     # the middle call takes one frame of each stream
    w0 = oracle_call(frames[0], bases)
    w1 = oracle_call([[f] for f in tick], w0[3])
    w2 = oracle_call(frames[2], w1[3])
    st = Region(S, n).put(bases)
    fr0, fr1, fr2 = Region(B, n).put(rows(frames[0])), Region(S, n).put(tick), Region(B, n).put(rows(frames[2]))
    out0, out1, out2 = Arrays(B, B * n), Arrays(S, S * n), Arrays(B, B * n)
    with CUDACore(w, h, max_batch=B) as core:
        if mode == "sequential":
            core.set_option(lib.OPT_PIPELINE, 0)
        if mode == "callers":
            core.use_torch_stream()
        torch.cuda.synchronize()
        core.diff_multi_stream_batch(fr0.ptr, st.ptr, S, T, out0.off.ptr, out0.xs.ptr, out0.df.ptr, B * n)
        core.diff_multi_batch(fr1.ptr, st.ptr, S, out1.off.ptr, out1.xs.ptr, out1.df.ptr, S * n)
        core.diff_multi_stream_batch(fr2.ptr, st.ptr, S, T, out2.off.ptr, out2.xs.ptr, out2.df.ptr, B * n)
        core.synchronize()
        torch.cuda.synchronize()
        for out, want in ((out0, w0), (out1, w1), (out2, w2)):
            off, xs, df = out.read()
            assert np.array_equal(off, want[0]) and np.array_equal(xs, want[1]) and np.array_equal(df, want[2])
        assert np.array_equal(st.get(), np.stack(w2[3]))

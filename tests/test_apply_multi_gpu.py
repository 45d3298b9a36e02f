"""-m gpu: mi355_apply_multi_batch / _wire_batch / _cwire_batch -- one segment or record of each of S streams applied to S
states in the caller's memory, in one call (include/mi355diff.h, "many streams, one frame each").  Everything is compared
bit for bit: with the server's states and the oracle tick by tick, with the host client and S one-stream client cores
record by record, and the three input forms with each other.  The states live in guarded regions: no byte outside the N
bytes of each state may change."""
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


def streams(S, K, w, h, seed0=1):
    """S different streams of K frames: (bases [S][n], frames [K][S][n])."""
    per = [synth.webcam_stream(K, w, h, seed=seed0 + 7 * s) for s in range(S)]
    return [b for b, _ in per], [[per[s][1][k] for s in range(S)] for k in range(K)]


def oracle_tick(frames, states, thr=20):
    """Every stream on its own through the oracle -> (offsets, xs, diff, new states)."""
    offs, xs, df, out = [0], [], [], []
    for s in range(len(frames)):
        eo, x, d, st = po.diff_stream(frames[s][None], states[s], thr)
        offs.append(offs[-1] + int(eo[1])); xs.append(x); df.append(d); out.append(st)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.empty(0, dt)
    return np.array(offs, np.uint32), cat(xs, np.int32), cat(df, np.uint8), out


def packed(segments):
    """[(xs, diff)] per stream -> (offsets uint32[S + 1], xs int32, diff uint8)."""
    off = np.cumsum([0] + [len(x) for x, _ in segments]).astype(np.uint32)
    xs = np.concatenate([np.asarray(x, np.int64) for x, _ in segments] + [np.empty(0, np.int64)]).astype(np.int32)
    df = np.concatenate([np.asarray(d, np.uint8) for _, d in segments] + [np.empty(0, np.uint8)]).astype(np.uint8)
    return off, xs, df


def numpy_apply(states, off, xs, df):
    """client/opencv.cpp:64-66 per stream, in numpy."""
    out = []
    for s, st in enumerate(states):
        st = st.copy()
        a, b = int(off[s]), int(off[s + 1])
        st[xs[a:b]] += df[a:b]          # indices of a segment are distinct; uint8 wraps
        out.append(st)
    return np.stack(out) if out else np.empty((0, 0), np.uint8)


def host_apply(states, recs, pos):
    """mi355_cwire_apply_host per stream on its own record."""
    out = []
    for s, st in enumerate(states):
        st = np.ascontiguousarray(st).copy()
        used = cwire_apply_host(st, recs[int(pos[s]):int(pos[s + 1])], 1)
        assert used == int(pos[s + 1] - pos[s])
        out.append(st)
    return np.stack(out)


def padded(a, dtype):
    """A device copy with guard room behind it (and never empty)."""
    return to_dev(np.concatenate([np.asarray(a, dtype), np.zeros(16, dtype)]))


def apply_arrays(core, st, off, xs, df, S=None):
    S = st.S if S is None else S
    d = (padded(off.view(np.int32), np.int32), padded(xs, np.int32), padded(df, np.uint8))
    torch.cuda.synchronize()   # (the new entry points are not in gpu_util's synced list)
    core.apply_multi_batch(d[0], d[1], d[2], S, st.t, stride=st.stride)
    core.synchronize()
    return st.get()


def apply_wire(core, st, off, xs, df, S=None):
    S = st.S if S is None else S
    d_wire = padded(po.wire_pack(off[:S + 1], xs, df), np.uint8)
    torch.cuda.synchronize()
    core.apply_multi_wire_batch(d_wire, np.diff(off.astype(np.int64))[:S], S, st.t, stride=st.stride)
    core.synchronize()
    return st.get()


def apply_compact(core, st, recs, counts, escapes, S=None):
    S = st.S if S is None else S
    d_cw = padded(recs, np.uint8)
    torch.cuda.synchronize()
    core.apply_multi_cwire_batch(d_cw, counts, escapes, S, st.t, stride=st.stride)
    core.synchronize()
    return st.get()


def all_three(core, st0, off, xs, df):
    """The tick through the three forms on clones of st0 -> the (identical) states."""
    recs, pos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, st0.S)
    a = apply_arrays(core, st0.clone(), off, xs, df)
    w = apply_wire(core, st0.clone(), off, xs, df)
    c = apply_compact(core, st0.clone(), recs, counts, escapes)
    assert np.array_equal(a, w), "arrays and wire forms differ"
    assert np.array_equal(a, c), "arrays and compact forms differ"
    return c, recs, pos


def server_tick(core, fr, st, S):
    """diff_multi_cwire_batch -> (records, counts, escapes, frame_pos)."""
    cap = cwire_bytes_max(fr.n, S)
    d_off = torch.zeros(S + 1, dtype=torch.int32, device=DEV)
    d_pos = torch.zeros(S + 1, dtype=torch.int64, device=DEV)
    d_cw = torch.full((cap + 64,), GUARD, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    core.diff_multi_cwire_batch(fr.t, st.t, S, d_off, d_pos, d_cw, cap, stride=fr.stride)
    core.synchronize()
    pos = d_pos.cpu().numpy().view(np.uint64)
    recs = d_cw[:int(pos[S])].cpu().numpy()
    counts, escapes = spec.headers(recs, S)
    return recs, counts, escapes, pos


@pytest.mark.parametrize("w,h,S,K", [(33, 7, 3, 4), (33, 7, 5, 4), (64, 48, 3, 4), (64, 48, 5, 4), (1920, 1080, 3, 2)])
def test_round_trip_server_client_oracle(w, h, S, K):
    """A server core diffs K ticks of S cameras into compact records, a client core applies them to states of its own that
    start from the base frames: after every tick client == server == oracle, stream by stream."""
    n = 3 * w * h
    bases, ticks = streams(S, K, w, h)
    srv, cli, fr = Region(S, n).put(bases), Region(S, n).put(bases), Region(S, n)
    with CUDACore(w, h, max_batch=S) as server, CUDACore(w, h, max_batch=S) as client:
        states = bases
        for k in range(K):
            recs, counts, escapes, _ = server_tick(server, fr.put(ticks[k]), srv, S)
            got = apply_compact(client, cli, recs, counts, escapes)
            states = oracle_tick(ticks[k], states)[3]
            assert np.array_equal(got, srv.get()), k
            assert np.array_equal(got, np.stack(states)), k


def download(core, d_tensor, nbytes):
    out = np.empty(nbytes, np.uint8)
    lib.check(core._lib.mi355_download(core._h, out.ctypes.data, C.c_void_p(d_tensor.data_ptr()), nbytes))
    return out


@pytest.mark.parametrize("w,h", [(64, 48), (640, 360)])
def test_loop_back_on_one_core_without_synchronisation(w, h):
    """diff_multi_cwire_batch, then apply_multi_cwire_batch of its records on the SAME core with nothing in between (the
    headers are known beforehand, from the oracle), then the download of one client state straight behind."""
    S, K = 3, 2
    n = 3 * w * h
    bases, ticks = streams(S, K, w, h, seed0=41)
    srv, cli = Region(S, n).put(bases), Region(S, n).put(bases)
    frs = [Region(S, n).put(ticks[k]) for k in range(K)]
    cap = cwire_bytes_max(n, S)
    states, hdrs = bases, []
    for k in range(K):
        off, xs, df, states = oracle_tick(ticks[k], states)
        recs, _ = spec.encode(off, xs, df)
        hdrs.append(spec.headers(recs, S))
    outs = [(torch.zeros(S + 1, dtype=torch.int32, device=DEV), torch.zeros(S + 1, dtype=torch.int64, device=DEV),
             torch.full((cap + 64,), GUARD, dtype=torch.uint8, device=DEV)) for _ in range(K)]
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        for k in range(K):
            core.diff_multi_cwire_batch(frs[k].t, srv.t, S, outs[k][0], outs[k][1], outs[k][2], cap)
            core.apply_multi_cwire_batch(outs[k][2], hdrs[k][0], hdrs[k][1], S, cli.t)
        last = download(core, cli.t[n:], n)          # state of stream 1, no synchronisation in front
        core.synchronize()
    want = np.stack(states)
    assert np.array_equal(srv.get(), want) and np.array_equal(cli.get(), want)
    assert np.array_equal(last, want[1])


@pytest.mark.parametrize("w,h", [(33, 7), (64, 48)])
def test_the_three_forms_agree_with_host_and_one_stream_cores(w, h):
    S, n = 4, 3 * w * h
    bases, ticks = streams(S, 1, w, h, seed0=11)
    off, xs, df, est = oracle_tick(ticks[0], bases)
    assert off[S] > 0
    st0 = Region(S, n).put(bases)
    with CUDACore(w, h, max_batch=S) as core:
        got, recs, pos = all_three(core, st0, off, xs, df)
    assert np.array_equal(got, np.stack(est))
    assert np.array_equal(got, host_apply(bases, recs, pos))
    counts, escapes = spec.headers(recs, S)
    for s in range(S):   # a one-stream client core that holds states[s]
        with CUDACore(w, h, sample_mat_data=bases[s], max_batch=1) as one:
            d_rec = padded(recs[int(pos[s]):int(pos[s + 1])], np.uint8)
            torch.cuda.synchronize()
            one.apply_cwire_batch(d_rec, counts[s:s + 1], escapes[s:s + 1], 1)
            one.synchronize()
            assert np.array_equal(one.get_state(), got[s]), s


def test_crafted_records():
    """64x48 (2.25 tiles): entries at {0, N - 1}; an escaped gap across a tile edge (4000 -> 4400); every byte changed (three
    chunks of codes); streams without entries between streams with some; nstreams == max_batch."""
    w, h = 64, 48
    n = 3 * w * h
    rng = np.random.default_rng(5)
    every = (np.arange(n), rng.integers(1, 256, n))
    segments = [([0, n - 1], [200, 77]), ([], []), ([4000, 4400], [1, 255]), ([], []), every, ([], []),
                ([4095, 4096, 8191, 8192], [9, 8, 7, 6])]
    S = len(segments)
    off, xs, df = packed(segments)
    base = [synth.refrand_frame(n, 70 + s) for s in range(S)]
    st0 = Region(S, n).put(base)
    with CUDACore(w, h, max_batch=S) as core:
        got, recs, pos = all_three(core, st0, off, xs, df)
        counts, escapes = spec.headers(recs, S)
        assert list(escapes) == [1, 0, 2, 0, 0, 0, 2] and counts[4] == n
        assert np.array_equal(got, numpy_apply(base, off, xs, df))
        assert np.array_equal(got, host_apply(base, recs, pos))
        # fewer streams than the region holds: the states behind them stay as they were
        part = apply_compact(core, st0.clone(), recs, counts, escapes, S=3)
        assert np.array_equal(part[:3], got[:3]) and np.array_equal(part[3:], np.stack(base[3:]))
        # no streams: every byte stays, with and without pointers
        for call in (lambda r: apply_arrays(core, r, off, xs, df, S=0), lambda r: apply_wire(core, r, off, xs, df, S=0),
                     lambda r: apply_compact(core, r, recs, counts, escapes, S=0)):
            assert np.array_equal(call(st0.clone()), np.stack(base))
        core.apply_multi_batch(None, None, None, 0, None)
        core.apply_multi_wire_batch(None, np.empty(0, np.uint32), 0, None)
        core.apply_multi_cwire_batch(None, np.empty(0, np.uint32), np.empty(0, np.uint32), 0, None)
        core.synchronize()


def test_more_streams_than_one_table_launch():
    """130 streams at 33x7: the headers of the compact and wire forms travel 128 per launch."""
    w, h, S = 33, 7, 130
    n = 3 * w * h
    rng = np.random.default_rng(9)
    segments = []
    for s in range(S):
        cnt = 0 if s % 7 == 3 else int(rng.integers(1, 40))
        x = np.sort(rng.choice(n, cnt, replace=False))
        segments.append((x, rng.integers(1, 256, cnt)))
    segments[127] = ([0, n - 1], [1, 2])
    segments[128] = ([0, 300, n - 1], [3, 4, 5])
    off, xs, df = packed(segments)
    base = [synth.refrand_frame(n, 200 + s) for s in range(S)]
    with CUDACore(w, h, max_batch=S) as core:
        got, _, _ = all_three(core, Region(S, n).put(base), off, xs, df)
    assert np.array_equal(got, numpy_apply(base, off, xs, df))


@pytest.mark.parametrize("pad,skew", [(0, 0), (0, 1), (0, 5), (13, 0), (13, 5)])
def test_neighbouring_states(pad, skew):
    """33x7: N = 693 is no multiple of 4, so with stride == N the last byte of state s and the first byte of state s + 1
    share a dword.  Both change in the same call; both come out right and nothing else moves."""
    w, h, S = 33, 7, 4
    n = 3 * w * h
    assert n % 4 and n % 16
    segments = [([0, n - 1], [10 + s, 250 - s]) for s in range(S)]
    segments[2] = ([0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1], [1, 2, 3, 4, 5, 6, 7, 8])
    off, xs, df = packed(segments)
    base = [synth.refrand_frame(n, 90 + s) for s in range(S)]
    st0 = Region(S, n, n + pad, skew).put(base)
    with CUDACore(w, h, max_batch=S) as core:
        got, _, _ = all_three(core, st0, off, xs, df)     # (Region.get asserts the guard and gap bytes)
    assert np.array_equal(got, numpy_apply(base, off, xs, df))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_malformed_content_stays_in_bounds(seed):
    """Stream 0's record: consistent headers over random code / escape / diff bytes.  No byte outside the states changes,
    the call succeeds, and the well-formed streams beside it come out as the host client makes them."""
    rng = np.random.default_rng(seed)
    w, h, S = 64, 48, 4
    n = 3 * w * h
    c0 = n if seed == 0 else int(rng.integers(1, n + 1))
    e0 = int(rng.integers(0, c0 + 1)) if seed % 2 else min(c0, int(rng.integers(0, 40)))
    p = spec.pad4(c0)
    code = rng.integers(0, 256, p, dtype=np.uint8)
    if seed % 3 == 0:
        code = np.where(code > 250, 255, code % 3).astype(np.uint8)   # mostly small gaps, some escapes
    esc = rng.integers(0, 2 ** 32, e0, dtype=np.uint64).astype(np.uint32)
    if seed % 3 == 1:
        esc %= 600
    bad = np.concatenate([np.array([c0, e0], "<u4").view(np.uint8), code, esc.view(np.uint8), rng.integers(0, 256, p, dtype=np.uint8)])
    segments = []
    for s in range(1, S):
        cnt = int(rng.integers(1, 3000))
        segments.append((np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)))
    off, xs, df = packed(segments)
    good, gpos = spec.encode(off, xs, df)
    gc, ge = spec.headers(good, S - 1)
    recs = np.concatenate([bad, good])
    counts, escapes = np.concatenate([[c0], gc]).astype(np.uint32), np.concatenate([[e0], ge]).astype(np.uint32)
    base = [synth.refrand_frame(n, 30 + seed + s) for s in range(S)]
    st = Region(S, n, n + 7, 3).put(base)
    with CUDACore(w, h, max_batch=S) as core:
        got = apply_compact(core, st, recs, counts, escapes)   # raises unless MI355_OK; Region.get asserts the guards
    assert np.array_equal(got[1:], host_apply(base[1:], good, gpos))


def test_refusals_write_nothing():
    w, h, S = 64, 48, 3
    n = 3 * w * h
    rng = np.random.default_rng(3)
    segments = [(np.sort(rng.choice(n, 50, replace=False)), rng.integers(1, 256, 50)) for _ in range(S)]
    off, xs, df = packed(segments)
    recs, pos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, S)
    wire = po.wire_pack(off, xs, df)
    base = [synth.refrand_frame(n, 50 + s) for s in range(S)]
    # the states behind a "frame" 0 of ONE guarded buffer, whose last bytes are the records: an input right up against them
    assert max(recs.size, wire.size) < n
    front = np.zeros(n, np.uint8)
    front[n - recs.size:] = recs
    both = Region(S + 1, n).put([front] + base)
    own = synth.refrand_frame(n, 49)
    d_off, d_xs, d_df = padded(off.view(np.int32), np.int32), padded(xs, np.int32), padded(df, np.uint8)
    d_cw, d_wire = padded(recs, np.uint8), padded(wire, np.uint8)
    s = both.t[n:]
    o, x, d, cw, wr, sp = (t.data_ptr() for t in (d_off, d_xs, d_df, d_cw, d_wire, s))
    z = np.zeros(S, np.uint32)
    big, esc_gt = counts.copy(), escapes.copy()
    big[1] = n + 1
    esc_gt[2] = counts[2] + 1
    with CUDACore(w, h, sample_mat_data=own, max_batch=S) as core:
        L, H = core._lib, core._h
        u32 = lambda a: a.ctypes.data
        A, W, CW = L.mi355_apply_multi_batch, L.mi355_apply_multi_wire_batch, L.mi355_apply_multi_cwire_batch
        # records inside the states' region: at its first byte, across its last state, and ending one byte into it
        inside = [sp, sp + (S - 1) * n + n - 4, sp - int(pos[S]) + 4]
        cases = [
            (A, (None, o, x, d, S, sp, n)), (W, (None, wr, u32(counts), S, sp, n)), (CW, (None, cw, u32(counts), u32(escapes), S, sp, n)),
            (A, (H, o, x, d, S + 1, sp, n)), (A, (H, o, x, d, -1, sp, n)),
            (W, (H, wr, u32(counts), S + 1, sp, n)), (W, (H, wr, u32(counts), -1, sp, n)),
            (CW, (H, cw, u32(counts), u32(escapes), S + 1, sp, n)), (CW, (H, cw, u32(counts), u32(escapes), -1, sp, n)),
            (A, (H, None, x, d, S, sp, n)), (A, (H, o, None, d, S, sp, n)), (A, (H, o, x, None, S, sp, n)),
            (W, (H, None, u32(counts), S, sp, n)), (W, (H, wr, None, S, sp, n)),
            (CW, (H, None, u32(counts), u32(escapes), S, sp, n)), (CW, (H, cw, None, u32(escapes), S, sp, n)),
            (CW, (H, cw, u32(counts), None, S, sp, n)),
            (A, (H, o, x, d, S, None, n)), (W, (H, wr, u32(counts), S, None, n)), (CW, (H, cw, u32(counts), u32(escapes), S, None, n)),
            (A, (H, o, x, d, S, sp, n - 1)), (W, (H, wr, u32(counts), S, sp, n - 1)),
            (CW, (H, cw, u32(counts), u32(escapes), S, sp, n - 1)),
            (CW, (H, cw, u32(counts), u32(esc_gt), S, sp, n)),                      # more escapes than entries
            (CW, (H, cw, u32(big), u32(z), S, sp, n)), (W, (H, wr, u32(big), S, sp, n)),   # more entries than bytes
            (CW, (H, cw + 1, u32(counts), u32(escapes), S, sp, n)), (CW, (H, cw + 2, u32(counts), u32(escapes), S, sp, n)),
            (A, (H, o + 2, x, d, S, sp, n)), (A, (H, o, x + 1, d, S, sp, n)),
        ]
        cases += [(CW, (H, at, u32(counts), u32(escapes), S, sp, n)) for at in inside]
        cases += [(W, (H, at, u32(counts), S, sp, n)) for at in (sp, sp + (S - 1) * n + n - 1, sp - int(wire.size) + 1)]
        torch.cuda.synchronize()
        for i, (fn, args) in enumerate(cases):
            assert fn(*args) == lib.ERR_INVALID, i
            assert L.mi355_last_error(), i
        core.synchronize()
        assert np.array_equal(core.get_state(), own)
        assert np.array_equal(both.get(), np.stack([front] + base))
        # records that END where the states begin do not overlap them: taken
        assert recs.size % 4 == 0 and CW(H, sp - recs.size, u32(counts), u32(escapes), S, sp, n) == lib.OK
        core.synchronize()
    assert np.array_equal(both.get(), np.concatenate([front[None], numpy_apply(base, off, xs, df)]))

"""-m gpu: mi355_apply_multi_stream_batch / _wire_batch / _cwire_batch -- T segments or records of each of S streams applied
to S states in the caller's memory in one call, batch index b = s*T + t, with every frame in between on request
(include/mi355diff.h, "The receiving end of a burst").  Everything is compared bit for bit: with the server's states and the
oracle, with the host client and one-stream client cores, with T ticks of mi355_apply_multi_cwire_batch, and the three
input forms with each other.  Inputs, states and output frames live in guarded buffers (gpu_util): no byte outside the N
bytes of each state and of each output frame may change."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib, synth
from oracle import pyoracle as po
from gpu_util import DEV, CUDACore, Guarded, Region

pytestmark = pytest.mark.gpu


# ---- references ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sequences(S, T, w, h, seed0=1, calls=1):
    """S different webcam-like streams of calls*T frames: (bases [S][n], frames [calls][S][T][n]); read-only."""
    per = []
    for s in range(S):
        base, frames = synth.webcam_stream(calls * T, w, h, seed=seed0 + 7 * s, device=DEV)
        per.append((base.cpu().numpy(), frames.cpu().numpy()))
        per[-1][0].setflags(write=False)
        per[-1][1].setflags(write=False)
    return [b for b, _ in per], [[[per[s][1][c * T + t] for t in range(T)] for s in range(S)] for c in range(calls)]


@functools.lru_cache(maxsize=None)
def oracle_run(S, T, w, h, seed0=1, calls=1, thr=20):
    """`calls` bursts in a row, every stream on its own through the oracle, frame by frame ->
    [(offsets [S*T + 1], xs, diff, frames after every record [S*T][n], states [S][n])] per call; computed once per shape."""
    bases, frames = sequences(S, T, w, h, seed0, calls)
    out, states = [], bases
    for c in range(calls):
        cnt, xs, df, after, new = [], [], [], [], []
        for s in range(S):
            st = states[s]
            for t in range(T):
                eo, x, d, st = po.diff_stream(frames[c][s][t][None], st, thr)
                cnt.append(int(eo[1])); xs.append(x); df.append(d); after.append(st)
            new.append(st)
        out.append((np.cumsum([0] + cnt).astype(np.uint32), np.concatenate(xs).astype(np.int32),
                    np.concatenate(df).astype(np.uint8), np.stack(after), new))
        states = new
    return out


def packed(segments):
    """[(xs, diff)] per batch index -> (offsets uint32[B + 1], xs int32, diff uint8)."""
    off = np.cumsum([0] + [len(x) for x, _ in segments]).astype(np.uint32)
    xs = np.concatenate([np.asarray(x, np.int64) for x, _ in segments] + [np.empty(0, np.int64)]).astype(np.int32)
    df = np.concatenate([np.asarray(d, np.uint8) for _, d in segments] + [np.empty(0, np.uint8)]).astype(np.uint8)
    return off, xs, df


def numpy_client(states, off, xs, df, S, T):
    """client/opencv.cpp:64-66 in numpy -> (frames after every record [S*T][n], states [S][n])."""
    after, out = [], []
    for s in range(S):
        st = np.array(states[s], np.uint8)
        for t in range(T):
            a, b = int(off[s * T + t]), int(off[s * T + t + 1])
            st[xs[a:b]] += df[a:b]          # indices of a segment are distinct; uint8 wraps
            after.append(st.copy())
        out.append(st)
    return np.stack(after), np.stack(out)


def random_segments(rng, n, B, most=40, empty_every=7):
    segs = []
    for b in range(B):
        cnt = 0 if b % empty_every == 3 else int(rng.integers(1, most))
        segs.append((np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)))
    return segs


# ---- the three forms ------------------------------------------------------------------------------------------------------
def run_form(form, core, st, out, off, xs, df, S, T, recs=None, hdr=None):
    """One call of `form` ("arrays", "wire", "compact") on the regions st (states) and out (frames, or None) -> (states,
    frames or None).  The inputs sit in guarded buffers; every guard is asserted."""
    B = S * T
    ins = []
    if form == "arrays":
        ins = [Guarded(B + 1, torch.int32, data=off.view(np.int32)), Guarded(xs.size, torch.int32, data=xs),
               Guarded(df.size, torch.uint8, data=df)]
        call = lambda: core.apply_multi_stream_batch(ins[0].ptr, ins[1].ptr, ins[2].ptr, S, T, st.ptr, st.stride,
                                                     out.ptr if out else None, out.stride if out else 0)
    elif form == "wire":
        wire = po.wire_pack(off, xs, df)
        ins = [Guarded(wire.size, torch.uint8, data=wire)]
        call = lambda: core.apply_multi_stream_wire_batch(ins[0].ptr, np.diff(off.astype(np.int64)), S, T, st.ptr, st.stride,
                                                          out.ptr if out else None, out.stride if out else 0)
    else:
        if recs is None:
            recs, _ = spec.encode(off, xs, df)
        counts, escapes = spec.headers(recs, B) if hdr is None else hdr
        ins = [Guarded(recs.size, torch.uint8, data=recs)]
        call = lambda: core.apply_multi_stream_cwire_batch(ins[0].ptr, counts, escapes, S, T, st.ptr, st.stride,
                                                           out.ptr if out else None, out.stride if out else 0)
    torch.cuda.synchronize()   # (the new entry points are not in gpu_util's synced list)
    call()
    core.synchronize()
    for g in ins:
        g.get()                # the inputs' guards
    return st.get(), (out.get() if out else None)


def all_forms(core, st0, off, xs, df, S, T, out_stride=None, out_skew=0):
    """The burst through the three forms, with and without output frames, on clones of st0 -> the (identical) states and
    frames."""
    first = None
    for form in ("compact", "wire", "arrays"):
        for with_out in (True, False):
            out = Region(S * T, st0.n, out_stride, out_skew) if with_out else None
            got = run_form(form, core, st0.clone(), out, off, xs, df, S, T)
            if first is None:
                first = got
            assert np.array_equal(got[0], first[0]), (form, with_out, "states")
            if with_out:
                assert np.array_equal(got[1], first[1]), (form, "frames")
    return first


# ---- 1. server -> client -> oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,S,T,calls", [(33, 7, 3, 4, 1), (64, 48, 3, 4, 2), (64, 48, 5, 3, 1), (640, 360, 2, 3, 1)])
def test_round_trip_server_client_oracle(w, h, S, T, calls):
    """A server core diffs bursts of T frames of S cameras into compact records, a client core applies each burst in one
    call to states of its own: client == server == oracle stream by stream, and every output frame is the oracle's state
    after that frame."""
    n, B = 3 * w * h, S * T
    assert (w, h) != (33, 7) or n % 2 == 1
    bases, frames = sequences(S, T, w, h, 1, calls)
    want = oracle_run(S, T, w, h, 1, calls)
    srv, cli = Region(S, n).put(bases), Region(S, n).put(bases)
    cap = cwire_bytes_max(n, B)
    with CUDACore(w, h, max_batch=B) as server, CUDACore(w, h, max_batch=B) as client:
        for c in range(calls):
            fr = Region(B, n).put([f for per in frames[c] for f in per])
            off, pos, cw = Guarded(B + 1, torch.int32), Guarded(B + 1, torch.int64), Guarded(cap)
            torch.cuda.synchronize()
            server.diff_multi_stream_cwire_batch(fr.ptr, srv.ptr, S, T, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
            server.synchronize()
            recs = cw.get()[:int(pos.get().view(np.uint64)[B])]
            out = Region(B, n)
            got, shown = run_form("compact", client, cli, out, None, None, None, S, T, recs=recs)
            assert int(want[c][0][B]) > 0
            assert np.array_equal(got, srv.get()), c
            assert np.array_equal(got, np.stack(want[c][4])), c
            assert np.array_equal(shown, want[c][3]), c


# ---- 2. the three forms, the host client, one-stream cores, T ticks of the multi form ---------------------------------------
@pytest.mark.parametrize("w,h", [(33, 7), (64, 48)])
def test_the_three_forms_agree_with_host_one_stream_cores_and_ticks(w, h):
    S, T, n = 3, 4, 3 * w * h
    B = S * T
    bases, _ = sequences(S, T, w, h, 11)
    off, xs, df, after, est = oracle_run(S, T, w, h, 11)[0]
    assert off[B] > 0
    recs, pos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, B)
    with CUDACore(w, h, max_batch=B) as core:
        got, shown = all_forms(core, Region(S, n).put(bases), off, xs, df, S, T)
        assert np.array_equal(got, np.stack(est)) and np.array_equal(shown, after)
        # T ticks of apply_multi_cwire_batch on re-staged records
        tick = Region(S, n).put(bases)
        for t in range(T):
            idx = [s * T + t for s in range(S)]
            stage = np.concatenate([recs[int(pos[b]):int(pos[b + 1])] for b in idx])
            g = Guarded(stage.size, torch.uint8, data=stage)
            torch.cuda.synchronize()
            core.apply_multi_cwire_batch(g.ptr, counts[idx], escapes[idx], S, tick.ptr, stride=tick.stride)
            core.synchronize()
            assert np.array_equal(tick.get(), shown[t::T]), t
    for s in range(S):
        sl = recs[int(pos[s * T]):int(pos[(s + 1) * T])]
        host = np.array(bases[s], np.uint8)
        assert cwire_apply_host(host, sl, T) == sl.size           # the host client on the stream's slice
        assert np.array_equal(host, got[s]), s
        with CUDACore(w, h, sample_mat_data=bases[s], max_batch=T) as one:   # a one-stream client core that holds states[s]
            g, out = Guarded(sl.size, torch.uint8, data=sl), Region(T, n)
            torch.cuda.synchronize()
            one.apply_cwire_batch(g.ptr, counts[s * T:(s + 1) * T], escapes[s * T:(s + 1) * T], T, out.ptr, out.stride)
            one.synchronize()
            assert np.array_equal(one.get_state(), got[s]), s
            assert np.array_equal(out.get(), shown[s * T:(s + 1) * T]), s


# ---- 3. crafted records -----------------------------------------------------------------------------------------------------
def test_crafted_records():
    """64x48 (2.25 tiles of 4096 bytes), T = 4.  Stream 0: a dense record (n = N: three chunks of codes, every tile) between
    sparse ones; stream 1: n = 0 records in the middle; stream 2: only n = 0 records; stream 3: an escaped gap across a tile
    edge, and three records in a row on the same bytes whose sum wraps past 255; stream 4: only the last, partial tile."""
    w, h, S, T = 64, 48, 5, 4
    n = 3 * w * h
    rng = np.random.default_rng(5)
    none = ([], [])
    segments = [
        ([0, n - 1], [200, 77]), (np.arange(n), rng.integers(1, 256, n)), ([5, 4095, 4096], [1, 2, 3]), ([0, n - 1], [100, 200]),
        ([7, 4100, 9000], [9, 9, 9]), none, none, ([7, 4100, 9000], [250, 250, 250]),
        none, none, none, none,
        ([4000, 4400], [1, 255]), ([100, 4000, 8191, 8192], [200, 200, 7, 6]), ([100, 4000], [100, 57]), ([100, 4400], [250, 1]),
        ([8192, n - 1], [3, 4]), ([8200], [5]), none, ([8192, 8193, n - 2, n - 1], [254, 1, 2, 255]),
    ]
    assert len(segments) == S * T
    off, xs, df = packed(segments)
    base = [synth.refrand_frame(n, 70 + s) for s in range(S)]
    after, want = numpy_client(base, off, xs, df, S, T)
    assert want[3][100] == (int(base[3][100]) + 550) % 256 and int(base[3][100]) + 550 > 255
    counts, escapes = spec.headers(spec.encode(off, xs, df)[0], S * T)
    assert counts[1] == n and escapes[12] == 2 and not counts[8:12].any()
    with CUDACore(w, h, max_batch=S * T) as core:
        got, shown = all_forms(core, Region(S, n).put(base), off, xs, df, S, T)
    assert np.array_equal(got, want) and np.array_equal(shown, after)
    assert np.array_equal(got[2], base[2]) and all(np.array_equal(shown[2 * T + t], base[2]) for t in range(T))
    assert np.array_equal(got[4][:8192], base[4][:8192])


# ---- 4. seams ---------------------------------------------------------------------------------------------------------------
def test_more_records_than_one_table_launch():
    """S*T = 150 = max_batch at 33x7: the records' headers travel 128 per k_cwa_table launch."""
    w, h, S, T = 33, 7, 5, 30
    n = 3 * w * h
    off, xs, df = packed(random_segments(np.random.default_rng(9), n, S * T))
    base = [synth.refrand_frame(n, 200 + s) for s in range(S)]
    after, want = numpy_client(base, off, xs, df, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        got, shown = all_forms(core, Region(S, n).put(base), off, xs, df, S, T)
    assert np.array_equal(got, want) and np.array_equal(shown, after)


def test_more_streams_than_one_wire_launch():
    """130 streams of 2 records at 33x7: the wire form's segments travel 128 per launch and t."""
    w, h, S, T = 33, 7, 130, 2
    n = 3 * w * h
    off, xs, df = packed(random_segments(np.random.default_rng(10), n, S * T))
    base = [synth.refrand_frame(n, 400 + s) for s in range(S)]
    after, want = numpy_client(base, off, xs, df, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        got, shown = all_forms(core, Region(S, n).put(base), off, xs, df, S, T)
    assert np.array_equal(got, want) and np.array_equal(shown, after)


def test_more_records_per_stream_than_one_ballot_pass():
    """T = 70 at 64x48: a wave looks at 64 records of its stream per pass.  Stream 1 has no entry before record 66 (its tiles
    are first loaded in the second pass), stream 0 only touches its last tile from record 64 on."""
    w, h, S, T = 64, 48, 2, 70
    n = 3 * w * h
    rng = np.random.default_rng(12)
    seg0 = [(np.sort(rng.choice(8192 if t < 64 else n, 30, replace=False)), rng.integers(1, 256, 30)) for t in range(T)]
    seg1 = [([], []) if t < 66 else (np.sort(rng.choice(n, 50, replace=False)), rng.integers(1, 256, 50)) for t in range(T)]
    off, xs, df = packed(seg0 + seg1)
    base = [synth.refrand_frame(n, 300 + s) for s in range(S)]
    after, want = numpy_client(base, off, xs, df, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        got, shown = all_forms(core, Region(S, n).put(base), off, xs, df, S, T)
    assert np.array_equal(got, want) and np.array_equal(shown, after)


def test_one_frame_is_the_multi_form_and_one_stream_is_the_client():
    w, h, n = 64, 48, 3 * 64 * 48
    rng = np.random.default_rng(13)
    with CUDACore(w, h, max_batch=4) as core:
        # nframes == 1: apply_multi_*
        S = 4
        off, xs, df = packed(random_segments(rng, n, S, most=3000))
        recs, _ = spec.encode(off, xs, df)
        counts, escapes = spec.headers(recs, S)
        base = [synth.refrand_frame(n, 500 + s) for s in range(S)]
        got, shown = all_forms(core, Region(S, n).put(base), off, xs, df, S, 1)
        assert np.array_equal(got, shown)
        ref = {}
        for form in ("arrays", "wire", "compact"):
            st = Region(S, n).put(base)
            ins = {"arrays": [off.view(np.int32), xs, df], "wire": [po.wire_pack(off, xs, df)], "compact": [recs]}[form]
            g = [Guarded(a.size, torch.int32 if a.dtype == np.int32 else torch.uint8, data=a) for a in ins]
            torch.cuda.synchronize()
            if form == "arrays":
                core.apply_multi_batch(g[0].ptr, g[1].ptr, g[2].ptr, S, st.ptr, stride=st.stride)
            elif form == "wire":
                core.apply_multi_wire_batch(g[0].ptr, np.diff(off.astype(np.int64)), S, st.ptr, stride=st.stride)
            else:
                core.apply_multi_cwire_batch(g[0].ptr, counts, escapes, S, st.ptr, stride=st.stride)
            core.synchronize()
            ref[form] = st.get()
            assert np.array_equal(ref[form], got), form
        # nstreams == 1: the one-stream client on a caller-held state
        T = 4
        off, xs, df = packed(random_segments(rng, n, T, most=3000))
        recs, _ = spec.encode(off, xs, df)
        counts, escapes = spec.headers(recs, T)
        got, shown = all_forms(core, Region(1, n).put(base[:1]), off, xs, df, 1, T)
    with CUDACore(w, h, sample_mat_data=base[0], max_batch=T) as one:
        g, out = Guarded(recs.size, torch.uint8, data=recs), Region(T, n)
        torch.cuda.synchronize()
        one.apply_cwire_batch(g.ptr, counts, escapes, T, out.ptr, out.stride)
        one.synchronize()
        assert np.array_equal(one.get_state(), got[0]) and np.array_equal(out.get(), shown)


# ---- 5. neighbouring states and frames ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("opad,oskew", [(0, 0), (0, 5), (13, 5)])
@pytest.mark.parametrize("pad,skew", [(0, 0), (0, 1), (0, 5), (13, 0), (13, 5)])
def test_neighbouring_states_and_frames(pad, skew, opad, oskew):
    """33x7: N = 693 is odd, so with stride == N the last byte of state (or frame) s and the first byte of s + 1 share a dword
    and a 16-byte word.  Both change in the same call; both come out right and nothing else moves."""
    w, h, S, T = 33, 7, 3, 3
    n = 3 * w * h
    assert n % 4 and n % 16
    segments = [([0, n - 1], [10 + b, 250 - b]) for b in range(S * T)]
    segments[4] = ([0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1], [1, 2, 3, 4, 5, 6, 7, 8])
    off, xs, df = packed(segments)
    base = [synth.refrand_frame(n, 90 + s) for s in range(S)]
    after, want = numpy_client(base, off, xs, df, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        got, shown = all_forms(core, Region(S, n, n + pad, skew).put(base), off, xs, df, S, T, n + opad, oskew)
    assert np.array_equal(got, want) and np.array_equal(shown, after)   # (Region.get asserted the guard and gap bytes)


# ---- 6. loop-back on one core ---------------------------------------------------------------------------------------------------
def download(core, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    lib.check(core._lib.mi355_download(core._h, out.ctypes.data, C.c_void_p(ptr), nbytes))
    return out


@pytest.mark.parametrize("w,h", [(64, 48), (640, 360)])
def test_loop_back_on_one_core_without_synchronisation(w, h):
    """diff_multi_stream_cwire_batch, then apply_multi_stream_cwire_batch of its records on the SAME core with nothing in
    between (the headers are known beforehand, from the oracle), then the download of one output frame straight behind."""
    S, T, K = 2, 3, 2
    n, B = 3 * w * h, S * T
    bases, frames = sequences(S, T, w, h, 41, K)
    want = oracle_run(S, T, w, h, 41, K)
    hdrs = [spec.headers(spec.encode(*want[k][:3])[0], B) for k in range(K)]
    srv, cli = Region(S, n).put(bases), Region(S, n).put(bases)
    frs = [Region(B, n).put([f for per in frames[k] for f in per]) for k in range(K)]
    cap = cwire_bytes_max(n, B)
    outs = [(Guarded(B + 1, torch.int32), Guarded(B + 1, torch.int64), Guarded(cap), Region(B, n)) for _ in range(K)]
    with CUDACore(w, h, max_batch=B) as core:
        torch.cuda.synchronize()
        for k in range(K):
            o = outs[k]
            core.diff_multi_stream_cwire_batch(frs[k].ptr, srv.ptr, S, T, o[0].ptr, o[1].ptr, o[2].ptr, cap, stride=n)
            core.apply_multi_stream_cwire_batch(o[2].ptr, hdrs[k][0], hdrs[k][1], S, T, cli.ptr, n, o[3].ptr, n)
        last = download(core, outs[K - 1][3].ptr + (B - 2) * n, n)   # the frame before the last, no synchronisation in front
        core.synchronize()
    final = np.stack(want[K - 1][4])
    assert np.array_equal(srv.get(), final) and np.array_equal(cli.get(), final)
    assert np.array_equal(last, want[K - 1][3][B - 2])
    for k in range(K):
        assert np.array_equal(outs[k][3].get(), want[k][3]), k


# ---- 7. malformed content ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_malformed_content_stays_in_bounds(seed):
    """Stream 1's records: consistent headers over random code / escape / diff bytes.  No byte outside the states and the
    output frames changes, the input's guards included; the call succeeds; the well-formed streams beside it come out as
    the numpy client makes them."""
    rng = np.random.default_rng(seed)
    w, h, S, T = 64, 48, 3, 3
    n, B = 3 * w * h, S * T
    good = random_segments(rng, n, B, most=3000)
    off, xs, df = packed(good)
    wrecs, wpos = spec.encode(off, xs, df)
    counts, escapes = (a.copy() for a in spec.headers(wrecs, B))
    parts = []
    for b in range(B):
        if b // T != 1:
            parts.append(wrecs[int(wpos[b]):int(wpos[b + 1])])
            continue
        c0 = n if (seed == 0 and b % T == 0) else int(rng.integers(1, n + 1))
        e0 = int(rng.integers(0, c0 + 1)) if b % 2 else min(c0, int(rng.integers(0, 40)))
        p = spec.pad4(c0)
        code = rng.integers(0, 256, p, dtype=np.uint8)
        if b % 3 == 0:
            code = np.where(code > 250, 255, code % 3).astype(np.uint8)   # mostly small gaps, some escapes
        esc = rng.integers(0, 2 ** 32, e0, dtype=np.uint64).astype(np.uint32)
        if b % 3 == 1:
            esc %= 600
        parts.append(np.concatenate([np.array([c0, e0], "<u4").view(np.uint8), code, esc.view(np.uint8),
                                     rng.integers(0, 256, p, dtype=np.uint8)]))
        counts[b], escapes[b] = c0, e0
    recs = np.concatenate(parts)
    base = [synth.refrand_frame(n, 30 + seed + s) for s in range(S)]
    after, want = numpy_client(base, off, xs, df, S, T)
    with CUDACore(w, h, max_batch=B) as core:
        for with_out in (True, False):
            st, out = Region(S, n, n + 7, 3).put(base), (Region(B, n, n + 5, 1) if with_out else None)
            got, shown = run_form("compact", core, st, out, None, None, None, S, T, recs=recs, hdr=(counts, escapes))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
            if with_out:
                assert np.array_equal(shown[:T], after[:T]) and np.array_equal(shown[2 * T:], after[2 * T:])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, S, T = 64, 48, 2, 2
    n, B = 3 * w * h, S * T
    rng = np.random.default_rng(3)
    off, xs, df = packed([(np.sort(rng.choice(n, 50, replace=False)), rng.integers(1, 256, 50)) for _ in range(B)])
    recs, pos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, B)
    wire = po.wire_pack(off, xs, df)
    base = [synth.refrand_frame(n, 50 + s) for s in range(S)]
    # ONE guarded buffer: row 0 ends with the records, rows 1 .. S are the states, the B rows behind them the output frames
    assert max(recs.size, wire.size) < n and recs.size % 4 == 0
    front = np.zeros(n, np.uint8)
    front[n - recs.size:] = recs
    rows = [front] + base + [synth.refrand_frame(n, 60 + b) for b in range(B)]
    both = Region(1 + S + B, n).put(rows)
    own = synth.refrand_frame(n, 49)
    g = [Guarded(a.size, torch.int32 if a.dtype == np.int32 else torch.uint8, data=a)
         for a in (off.view(np.int32), xs, df, recs, wire)]
    o, x, d, cw, wr = (q.ptr for q in g)
    sp = both.ptr + n             # the states
    fp = sp + S * n               # the output frames, right behind them
    u32 = lambda a: a.ctypes.data
    big, esc_gt = counts.copy(), escapes.copy()
    big[1] = n + 1
    esc_gt[2] = counts[2] + 1
    z = np.zeros(B, np.uint32)
    c_, e_ = u32(counts), u32(escapes)
    with CUDACore(w, h, sample_mat_data=own, max_batch=B) as core:
        L, H = core._lib, core._h
        A, W, CW = L.mi355_apply_multi_stream_batch, L.mi355_apply_multi_stream_wire_batch, L.mi355_apply_multi_stream_cwire_batch
        tail = (sp, n, fp, n)
        cases = [
            (A, (None, o, x, d, S, T) + tail), (W, (None, wr, c_, S, T) + tail), (CW, (None, cw, c_, e_, S, T) + tail),
            (A, (H, o, x, d, -1, T) + tail), (A, (H, o, x, d, S, -1) + tail), (W, (H, wr, c_, -1, T) + tail),
            (W, (H, wr, c_, S, -1) + tail), (CW, (H, cw, c_, e_, -1, T) + tail), (CW, (H, cw, c_, e_, S, -1) + tail),
            # S*T = max_batch + 1, and a product that only fits 64 bits
            (A, (H, o, x, d, 1, B + 1) + tail), (W, (H, wr, c_, B + 1, 1) + tail), (CW, (H, cw, c_, e_, 1, B + 1) + tail),
            (CW, (H, cw, c_, e_, 1 << 16, 1 << 16) + tail), (A, (H, o, x, d, 1 << 16, 1 << 16) + tail),
            (W, (H, wr, c_, 1 << 16, 1 << 16) + tail),
            (A, (H, None, x, d, S, T) + tail), (A, (H, o, None, d, S, T) + tail), (A, (H, o, x, None, S, T) + tail),
            (W, (H, None, c_, S, T) + tail), (W, (H, wr, None, S, T) + tail),
            (CW, (H, None, c_, e_, S, T) + tail), (CW, (H, cw, None, e_, S, T) + tail), (CW, (H, cw, c_, None, S, T) + tail),
            (A, (H, o, x, d, S, T, None, n, fp, n)), (W, (H, wr, c_, S, T, None, n, fp, n)), (CW, (H, cw, c_, e_, S, T, None, n, fp, n)),
            (A, (H, o, x, d, S, T, sp, n - 1, fp, n)), (W, (H, wr, c_, S, T, sp, n - 1, fp, n)),
            (CW, (H, cw, c_, e_, S, T, sp, n - 1, fp, n)),
            (A, (H, o, x, d, S, T, sp, n, fp, n - 1)), (W, (H, wr, c_, S, T, sp, n, fp, n - 1)),      # out_stride < N
            (CW, (H, cw, c_, e_, S, T, sp, n, fp, n - 1)),
            (CW, (H, cw, c_, u32(esc_gt), S, T) + tail),                                               # more escapes than entries
            (CW, (H, cw, u32(big), u32(z), S, T) + tail), (W, (H, wr, u32(big), S, T) + tail),         # more entries than bytes
            (CW, (H, cw + 1, c_, e_, S, T) + tail), (CW, (H, cw + 2, c_, e_, S, T) + tail),            # misaligned d_cwire
            (A, (H, o + 2, x, d, S, T) + tail), (A, (H, o, x + 1, d, S, T) + tail),
        ]
        # the states against the output frames: one byte into them from either side, and inside
        for bad_fp in (sp + S * n - 1, sp - (B - 1) * n - n + 1, sp):
            cases += [(A, (H, o, x, d, S, T, sp, n, bad_fp, n)), (W, (H, wr, c_, S, T, sp, n, bad_fp, n)),
                      (CW, (H, cw, c_, e_, S, T, sp, n, bad_fp, n))]
        # the input against the states: at their first byte, across the last state, ending one word / byte into them
        cases += [(CW, (H, at, c_, e_, S, T) + tail) for at in (sp, sp + (S - 1) * n + n - 4, sp - recs.size + 4)]
        cases += [(W, (H, at, c_, S, T) + tail) for at in (sp, sp + (S - 1) * n + n - 1, sp - wire.size + 1)]
        # the input against the output frames, with the frames in rows 1 .. B and the states behind them: at the frames' first
        # byte, across their end, and ending one word / byte into them (the input then begins in row 0, far from the states)
        alt = (sp + B * n, n, sp, n)
        cases += [(CW, (H, at, c_, e_, S, T) + alt) for at in (sp, sp + B * n - 4, sp - recs.size + 4)]
        cases += [(W, (H, at, c_, S, T) + alt) for at in (sp, sp + B * n - 1, sp - wire.size + 1)]
        torch.cuda.synchronize()
        for i, (fn, args) in enumerate(cases):
            assert fn(*args) == lib.ERR_INVALID, i
            assert L.mi355_last_error(), i
        core.synchronize()
        assert np.array_equal(core.get_state(), own)
        assert np.array_equal(both.get(), np.stack(rows))
        # S*T == 0 in both ways: OK, with and without pointers, and nothing is written
        for S0, T0 in ((0, T), (S, 0), (0, 0)):
            assert A(H, o, x, d, S0, T0, sp, n, fp, n) == lib.OK and A(H, None, None, None, S0, T0, None, 0, None, 0) == lib.OK
            assert W(H, wr, c_, S0, T0, sp, n, fp, n) == lib.OK and W(H, None, None, S0, T0, None, 0, None, 0) == lib.OK
            assert CW(H, cw, c_, e_, S0, T0, sp, n, fp, n) == lib.OK and CW(H, None, None, None, S0, T0, None, 0, None, 0) == lib.OK
        core.synchronize()
        assert np.array_equal(both.get(), np.stack(rows))
        # records that END where the states begin overlap nothing: taken
        assert CW(H, sp - recs.size, c_, e_, S, T, sp, n, fp, n) == lib.OK
        core.synchronize()
    for q in g:
        q.get()
    after, want = numpy_client(base, off, xs, df, S, T)
    assert np.array_equal(both.get(), np.concatenate([front[None], want, after]))

"""-m gpu: the compact wire format, the GPU client, the merge and the many-streams forms at frame and stream counts past
the fixed counts at which their kernels and host loops start another round: the 64 lanes of a wave and the 1024 threads of
cwire_scan_frame_pos (csrc/cwire_common.h), the 8192 slots of the encoder (cwire_blocks_per_frame below 256, the scan's LDS
at its largest), the 64 frames of a decode launch, the 128 headers of a table launch of the GPU clients, max_batch slices,
the 64 parts of a merge.  Frames are tiny, so that thousands of them cost seconds.

Everything is compared np.array_equal with the oracle (oracle/pyoracle.py), the numpy statement of the format
(tests/cwire_spec.py), the host client (mi355_cwire_apply_host) and `state[xs] += diff`; every output lies in a guarded
buffer (gpu_util.Guarded, gpu_util.Region).  Before the GPU is touched each case asserts, from the reference alone, that its
input reaches the seam it is there for (check_input)."""
import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib
from oracle import pyoracle as po
from gpu_util import CUDACore, Guarded, Region, to_dev

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64


# ---- inputs -------------------------------------------------------------------------------------------------------------
def mutate(rng, img, kind):
    """A copy of img with bytes flipped by 0x80 (128 > every threshold used here, so each flip is one entry and the state
    takes the frame whole): kind 0 none, 1 one byte, 2 every byte, 3 about n / 200 + 1 bytes at random places (n >= 512:
    gaps of 255 and more, hence escapes), 4 a run of adjacent bytes across a multiple of 256 (the second or a later one
    where there is one: the run's first gap is then escaped)."""
    out, n = img.copy(), img.size
    if kind == 1:
        out[rng.integers(0, n)] ^= 0x80
    elif kind == 2:
        out ^= 0x80
    elif kind == 3:
        out[rng.choice(n, n // 200 + 1, replace=False)] ^= 0x80
    elif kind == 4:
        edges = np.arange(256, n - 4, 256)
        edge = int(rng.choice(edges[1:] if edges.size > 1 else edges)) if edges.size else n // 2
        out[max(edge - 3, 0):min(edge + 5, n)] ^= 0x80
    return out


def stream_frames(T, n, seed, kinds=(0, 1, 2, 3, 4)):
    """(base, frames[T, n]): frame t is frame t - 1 (the state) changed as kinds[t % len(kinds)] says."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, n, dtype=np.uint8)
    frames, cur = np.empty((T, n), np.uint8), base
    for t in range(T):
        cur = mutate(rng, cur, kinds[t % len(kinds)])
        frames[t] = cur
    return base, frames


def tick_frames(S, n, seed):
    """(states[S, n], frames[S, n]): stream s's frame is its state changed as kind s % 5 says."""
    rng = np.random.default_rng(seed)
    states = rng.integers(0, 256, (S, n), dtype=np.uint8)
    return states, np.stack([mutate(rng, states[s], s % 5) for s in range(S)])


def reference(base, frames):
    """Oracle stream of the frames, its compact records and their headers: (off, xs, df, state, recs, pos, counts, escapes)."""
    off, xs, df, st = po.diff_stream(frames, base)
    recs, pos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, frames.shape[0])
    return off, xs, df, st, recs, pos, counts, escapes


def oracle_tick(frames, states):
    """Every stream on its own through the oracle -> (offsets, xs, diff, new states[S, n])."""
    offs, xs, df, out = [0], [], [], []
    for s in range(len(frames)):
        c, x, d, st = po.diff_pack(frames[s], states[s])
        offs.append(offs[-1] + c); xs.append(x); df.append(d); out.append(st)
    return np.array(offs, np.uint32), np.concatenate(xs).astype(np.int32), np.concatenate(df).astype(np.uint8), np.stack(out)


def check_input(n, counts, escapes, pos, seam):
    """The input does what it is for: an empty record, a full one, and -- frames of 512 bytes and more -- escapes, one of them
    at or behind record `seam`, the first record of the second round / launch of the seam under test; the records from
    there on have bytes, so that a total which lost the first round's cannot be right."""
    T = counts.size
    assert (counts == 0).any() and (counts == n).any()
    assert 0 <= seam < T and int(pos[T]) != int(pos[seam]) and (seam == 0 or int(pos[seam]) != 0)
    if n >= 512:
        assert escapes.sum() > 0 and escapes[seam:].any()
    else:
        assert escapes.sum() == 0


def scan_seam(T):
    """First record of the second round of cwire_scan_frame_pos<1024>, else of its second wave, else 0."""
    return 1024 if T > 1024 else 64 if T > 64 else 0


# ---- 1. mi355_cwire_encode_batch against the numpy statement ------------------------------------------------------------
def gpu_stream(core, frames, off, xs, df):
    """diff_stream_batch into guarded arrays, checked against the oracle's -> the device arrays (Guarded) and their room."""
    T, n = frames.shape
    cap = T * n
    g_off, g_xs, g_df = Guarded(T + 1, I32), Guarded(cap, I32), Guarded(cap)
    core.diff_stream_batch(to_dev(frames), T, g_off.ptr, g_xs.ptr, g_df.ptr, cap)
    core.synchronize()
    tot = int(off[-1])
    assert np.array_equal(g_off.get().view(np.uint32), off)
    assert np.array_equal(g_xs.get(written=tot)[:tot], xs) and np.array_equal(g_df.get(written=tot)[:tot], df)
    return g_off, g_xs, g_df, cap


def gpu_encode(core, g_off, g_xs, g_df, ecap, T, cap):
    g_pos, g_cw = Guarded(T + 1, I64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_encode_batch(g_off.ptr, g_xs.ptr, g_df.ptr, ecap, T, g_pos.ptr, g_cw.ptr, cap)
    core.synchronize()
    return g_pos, g_cw


# blocks per frame of the count / emit kernels (8192 / T, at most 256): 256, 248, 128, 126, 63, 8, 7; 1, 1 (the scan's
# dynamic LDS: 4097 and 8192 words); 63 with a dozen code dwords and several escapes per frame
@pytest.mark.parametrize("w,h,T", [(33, 7, 32), (33, 7, 33), (33, 7, 64), (33, 7, 65), (33, 7, 129), (33, 7, 1024), (33, 7, 1025),
                                   (5, 1, 4097), (5, 1, 8192), (64, 48, 130)])
def test_encode_equals_spec(w, h, T):
    n = 3 * w * h
    base, frames = stream_frames(T, n, seed=T)
    off, xs, df, st, want, wpos, counts, escapes = reference(base, frames)
    check_input(n, counts, escapes, wpos, scan_seam(T))
    if (w, h) == (64, 48):
        assert (escapes >= 3).any()
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        g_off, g_xs, g_df, ecap = gpu_stream(core, frames, off, xs, df)
        assert np.array_equal(core.get_state(), st)
        g_pos, g_cw = gpu_encode(core, g_off, g_xs, g_df, ecap, T, cwire_bytes_max(n, T))
        assert np.array_equal(g_pos.get().view(np.uint64), wpos)
        assert np.array_equal(g_cw.get(written=want.size)[:want.size], want)
        if T == 1025:
            # one byte short of the whole: the last record -- the second round's only one -- is skipped, and only it
            cap = int(wpos[T]) - 1
            g_pos, g_cw = gpu_encode(core, g_off, g_xs, g_df, ecap, T, cap)
            fit = int(wpos[T - 1])
            assert np.array_equal(g_pos.get().view(np.uint64), wpos)
            assert np.array_equal(g_cw.get(written=fit)[:fit], want[:fit])


def test_encode_refuses_more_frames_than_slots():
    T = 8193
    g_off, g_pos, g_cw = Guarded(T + 1, I32, data=np.zeros(T + 1, np.int32)), Guarded(T + 1, I64), Guarded(8 * T)
    g_xs, g_df = Guarded(4, I32), Guarded(4)
    with CUDACore(5, 1, max_batch=1) as core:
        torch.cuda.synchronize()
        with pytest.raises(lib.Mi355Error) as e:
            core.cwire_encode_batch(g_off.ptr, g_xs.ptr, g_df.ptr, 4, T, g_pos.ptr, g_cw.ptr, 8 * T)
        assert e.value.code == lib.ERR_INVALID
        core.synchronize()
    g_pos.get(written=0), g_cw.get(written=0)


# ---- 2. the direct forms ------------------------------------------------------------------------------------------------
def direct_out(T, cap):
    return Guarded(T + 1, I32), Guarded(T + 1, I64), Guarded(cap)


def check_direct(out, off, wpos, want):
    g_off, g_pos, g_cw = out
    assert np.array_equal(g_off.get().view(np.uint32), off)
    assert np.array_equal(g_pos.get().view(np.uint64), wpos)
    assert np.array_equal(g_cw.get(written=want.size)[:want.size], want)


@pytest.mark.parametrize("w,h,T", [(33, 7, 65), (33, 7, 1024), (33, 7, 1025), (5, 1, 2050)])
def test_direct_equals_spec(w, h, T):
    n = 3 * w * h
    base, frames = stream_frames(T, n, seed=100 + T)
    off, xs, df, st, want, wpos, counts, escapes = reference(base, frames)
    check_input(n, counts, escapes, wpos, scan_seam(T))
    cap = cwire_bytes_max(n, T)
    out = direct_out(T, cap)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        d_frames = to_dev(frames)
        torch.cuda.synchronize()
        core.diff_stream_cwire_batch(d_frames, T, out[0].ptr, out[1].ptr, out[2].ptr, cap)
        core.synchronize()
        check_direct(out, off, wpos, want)
        assert np.array_equal(core.get_state(), st)


def test_direct_two_long_batches_back_to_back():
    """Two batches of 1025 frames on the core's own stream with nothing in between."""
    w, h, T = 33, 7, 1025
    n = 3 * w * h
    base, frames = stream_frames(2 * T, n, seed=7)
    refs, state = [], base
    for k in range(2):
        r = reference(state, frames[k * T:(k + 1) * T])
        check_input(n, r[6], r[7], r[5], 1024)
        refs.append(r)
        state = r[3]
    cap = cwire_bytes_max(n, T)
    outs = [direct_out(T, cap) for _ in range(2)]
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as core:
        d_frames = to_dev(frames)
        torch.cuda.synchronize()
        for k in range(2):
            core.diff_stream_cwire_batch(d_frames[k * T:(k + 1) * T], T, outs[k][0].ptr, outs[k][1].ptr, outs[k][2].ptr, cap)
        core.synchronize()
        for k in range(2):
            check_direct(outs[k], refs[k][0], refs[k][5], refs[k][4])
        assert np.array_equal(core.get_state(), state)


@pytest.mark.parametrize("pad", [0, 13])
@pytest.mark.parametrize("S", [65, 129, 1025])
def test_multi_forms_equal_spec_and_oracle(S, pad):
    """One tick of S streams at 33x7 (N = 693 is no multiple of 4: with stride N neighbouring states share dwords) through
    the arrays, the sender's-wire and the compact form, each on its own copy of the states."""
    w, h = 33, 7
    n = 3 * w * h
    states, frames = tick_frames(S, n, seed=S)
    off, xs, df, est = oracle_tick(frames, states)
    want, wpos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(want, S)
    check_input(n, counts, escapes, wpos, scan_seam(S))
    wire = po.wire_pack(off, xs, df)
    tot, cap = int(off[S]), cwire_bytes_max(n, S)
    fr = Region(S, n, n + pad, skew=3).put(frames)
    st_a, st_w, st_c = (Region(S, n, n + pad, skew=5).put(states) for _ in range(3))
    a_off, a_xs, a_df = Guarded(S + 1, I32), Guarded(S * n, I32), Guarded(S * n)
    w_off, w_wire = Guarded(S + 1, I32), Guarded(wire.size)
    c_out = direct_out(S, cap)
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        core.diff_multi_batch(fr.ptr, st_a.ptr, S, a_off.ptr, a_xs.ptr, a_df.ptr, S * n, stride=n + pad)
        core.diff_multi_wire_batch(fr.ptr, st_w.ptr, S, w_off.ptr, w_wire.ptr, wire.size, stride=n + pad)
        core.diff_multi_cwire_batch(fr.ptr, st_c.ptr, S, c_out[0].ptr, c_out[1].ptr, c_out[2].ptr, cap, stride=n + pad)
        core.synchronize()
    assert np.array_equal(a_off.get().view(np.uint32), off)
    assert np.array_equal(a_xs.get(written=tot)[:tot], xs) and np.array_equal(a_df.get(written=tot)[:tot], df)
    assert np.array_equal(w_off.get().view(np.uint32), off)
    assert np.array_equal(w_wire.get(), wire)
    check_direct(c_out, off, wpos, want)
    for st in (st_a, st_w, st_c):
        assert np.array_equal(st.get(), est)
    assert np.array_equal(fr.get(), frames)   # the frames are only read


# ---- 3. mi355_cwire_decode_batch: 64 frames per launch ---------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 65, 128, 129, 200])
def test_decode_equals_spec(T):
    w, h = 33, 7
    n = 3 * w * h
    base, frames = stream_frames(T, n, seed=200 + T)
    off, xs, df, st, recs, pos, counts, escapes = reference(base, frames)
    check_input(n, counts, escapes, pos, 64 * ((T - 1) // 64))   # (the last launch)
    s_off, s_xs, s_df = spec.decode(recs, T)
    assert np.array_equal(s_off, off) and np.array_equal(s_xs, xs) and np.array_equal(s_df, df)
    tot = int(off[T])
    caps = [tot]
    if T == 129:
        assert counts[128] >= 2
        caps.append(int(off[128]) + 1)   # cuts inside the first frame of the third launch
    with CUDACore(w, h, max_batch=1) as core:
        d_cw = Guarded(recs.size, data=recs)
        for cap in caps:
            g_off, g_xs, g_df = Guarded(T + 1, I32), Guarded(tot, I32), Guarded(tot)
            torch.cuda.synchronize()
            core.cwire_decode_batch(d_cw.ptr, counts, escapes, T, g_off.ptr, g_xs.ptr, g_df.ptr, cap)
            core.synchronize()
            assert np.array_equal(g_off.get().view(np.uint32), s_off), cap   # exact regardless
            assert np.array_equal(g_xs.get(written=cap)[:cap], s_xs[:cap]), cap
            assert np.array_equal(g_df.get(written=cap)[:cap], s_df[:cap]), cap
        assert np.array_equal(d_cw.get(), recs)


# ---- 4. mi355_apply_cwire_batch: max_batch slices, 128 headers per table launch --------------------------------------------
def host_frames(state, recs, T):
    """The host client, frame by frame -> (frames[T, N], final state)."""
    st, out, at = state.copy(), [], 0
    for _ in range(T):
        at += cwire_apply_host(st, recs[at:], 1)
        out.append(st.copy())
    assert at == recs.size
    return np.stack(out), st


@pytest.mark.parametrize("outputs", [False, True])
@pytest.mark.parametrize("w,h,max_batch,T", [(33, 7, 128, 128), (33, 7, 129, 129), (33, 7, 130, 300), (33, 7, 256, 257),
                                             (64, 48, 129, 129)])
def test_gpu_client_equals_host_client(w, h, max_batch, T, outputs):
    n = 3 * w * h
    base, frames = stream_frames(T, n, seed=320 + T)
    off, xs, df, st, recs, pos, counts, escapes = reference(base, frames)
    # the second table launch of a slice where there is one (a slice's records 128 and up), else the second slice
    seam = 128 if max_batch > 128 else 0
    check_input(n, counts, escapes, pos, seam)
    if T > max_batch:
        assert escapes[max_batch:].any()
    want_frames, want_state = host_frames(base, recs, T)
    assert np.array_equal(want_state, st)
    d_cw = Guarded(recs.size, data=recs)
    out = Region(T, n, n + 13, skew=5) if outputs else None
    with CUDACore(w, h, sample_mat_data=base, max_batch=max_batch) as core:
        torch.cuda.synchronize()
        core.apply_cwire_batch(d_cw.ptr, counts, escapes, T, out.ptr if outputs else None, n + 13)
        core.synchronize()
        got_state = core.get_state()
    assert np.array_equal(d_cw.get(), recs)
    if outputs:
        got = out.get()
        for t in range(T):
            assert np.array_equal(got[t], want_frames[t]), t
    assert np.array_equal(got_state, want_state)


# ---- 5. mi355_apply_batch / mi355_apply_wire_batch over 300 frames -----------------------------------------------------------
@pytest.mark.parametrize("outputs", [False, True])
@pytest.mark.parametrize("form", ["arrays", "wire"])
def test_clients_of_the_other_forms_over_300_frames(form, outputs):
    w, h, T = 33, 7, 300
    n = 3 * w * h
    base, frames = stream_frames(T, n, seed=5)
    off, xs, df, st = po.diff_stream(frames, base)
    want, state = [], base.copy()
    for t in range(T):
        a, b = int(off[t]), int(off[t + 1])
        state[xs[a:b]] += df[a:b]
        want.append(state.copy())
    assert np.array_equal(state, st)
    out = Region(T, n, n + 13, skew=5) if outputs else None
    with CUDACore(w, h, sample_mat_data=base, max_batch=1) as core:
        if form == "arrays":
            d_in = (Guarded(T + 1, I32, data=off.view(np.int32)), Guarded(xs.size, I32, data=xs), Guarded(df.size, data=df))
            core.apply_batch(d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, T, out.ptr if outputs else None, n + 13)
        else:
            wire = po.wire_pack(off, xs, df)
            d_in = Guarded(wire.size, data=wire)
            core.apply_wire_batch(d_in.ptr, np.diff(off.astype(np.int64)).astype(np.uint32), T, out.ptr if outputs else None, n + 13)
        core.synchronize()
        got_state = core.get_state()
    if outputs:
        got = out.get()
        for t in range(T):
            assert np.array_equal(got[t], want[t]), t
    assert np.array_equal(got_state, st)


# ---- 6. mi355_merge_parts at its 64 parts ------------------------------------------------------------------------------------
def band_streams(base, frames, w, parts):
    """The oracle's stream of every one-row band -> (part_off[parts, T + 1], part_base, bias, xs_all, diff_all)."""
    p_off, p_xs, p_df = [], [], []
    for p in range(parts):
        b0, b1 = 3 * w * p, 3 * w * (p + 1)
        o, x, d, _ = po.diff_stream(frames[:, b0:b1], base[b0:b1])
        p_off.append(o); p_xs.append(x); p_df.append(d)
    part_base = np.concatenate([[0], np.cumsum([x.size for x in p_xs])])[:-1]
    return (np.stack(p_off), part_base, [3 * w * p for p in range(parts)], np.concatenate(p_xs).astype(np.int32),
            np.concatenate(p_df).astype(np.uint8))


def test_merge_of_64_row_bands_and_refusal_of_65():
    w, h, T = 5, 64, 3
    n = 3 * w * h
    base, frames = stream_frames(T, n, seed=6, kinds=(3, 2, 4))
    off, xs, df, _ = po.diff_stream(frames, base)
    p_off, part_base, bias, xs_all, df_all = band_streams(base, frames, w, h)
    assert (np.diff(p_off.astype(np.int64), axis=1)[:, 0] == 0).any() and (p_off[:, T] > 0).all()
    tot = int(off[T])
    assert xs_all.size == tot
    d_poff = Guarded(p_off.size, I32, data=p_off.view(np.int32).reshape(-1))
    d_xs_all, d_df_all = Guarded(tot, I32, data=xs_all), Guarded(tot, data=df_all)
    with CUDACore(w, h, max_batch=1) as core:
        g_off, g_xs, g_df = Guarded(T + 1, I32), Guarded(tot, I32), Guarded(tot)
        torch.cuda.synchronize()
        core.merge_parts(d_poff.ptr, part_base, bias, d_xs_all.ptr, d_df_all.ptr, T, g_off.ptr, g_xs.ptr, g_df.ptr, tot)
        core.synchronize()
        assert np.array_equal(g_off.get().view(np.uint32), off)
        assert np.array_equal(g_xs.get(), xs) and np.array_equal(g_df.get(), df)
        # a 65th part: refused, nothing written
        g_off, g_xs, g_df = Guarded(T + 1, I32), Guarded(tot, I32), Guarded(tot)
        d_poff65 = Guarded(p_off.size + T + 1, I32, data=np.concatenate([p_off.view(np.int32).reshape(-1), np.zeros(T + 1, np.int32)]))
        torch.cuda.synchronize()
        with pytest.raises(lib.Mi355Error) as e:
            core.merge_parts(d_poff65.ptr, np.append(part_base, tot), bias + [n], d_xs_all.ptr, d_df_all.ptr, T, g_off.ptr, g_xs.ptr,
                             g_df.ptr, tot)
        assert e.value.code == lib.ERR_INVALID
        core.synchronize()
        g_off.get(written=0), g_xs.get(written=0), g_df.get(written=0)


# ---- 7. server -> records -> client over 1025 frames -------------------------------------------------------------------------
def test_long_round_trip_server_to_gpu_client():
    w, h, T = 33, 7, 1025
    n = 3 * w * h
    base, frames = stream_frames(T, n, seed=9)
    off, xs, df, st, want, wpos, counts, escapes = reference(base, frames)
    check_input(n, counts, escapes, wpos, 1024)
    cap = cwire_bytes_max(n, T)
    out = direct_out(T, cap)
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as server, CUDACore(w, h, sample_mat_data=base, max_batch=130) as client:
        d_frames = to_dev(frames)
        torch.cuda.synchronize()
        server.diff_stream_cwire_batch(d_frames, T, out[0].ptr, out[1].ptr, out[2].ptr, cap)
        server.synchronize()
        check_direct(out, off, wpos, want)
        client.apply_cwire_batch(out[2].ptr, counts, escapes, T)   # eight slices, each of two table launches but the last
        client.synchronize()
        assert np.array_equal(client.get_state(), server.get_state())
        assert np.array_equal(client.get_state(), st)
    check_direct(out, off, wpos, want)   # the client only read the records

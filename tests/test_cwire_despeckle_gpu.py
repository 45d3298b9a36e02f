"""-m gpu: mi355_cwire_despeckle_cwire_batch -- the records of one tick of S cameras without the entries of isolated pixels, the
caller's states reverted where an entry is dropped (include/mi355diff.h, "A tick without its speckle").  The reference of every
comparison is the host form mi355_cwire_despeckle_host, which tests/test_cwire_despeckle_spec.py holds against the numpy
statement of the semantics (tests/despeckle_spec.py); the inputs are that module's, through mi355_diff_multi_cwire_batch.  Inputs,
outputs and states live in guarded buffers (gpu_util) that start as a non-zero pattern."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
import despeckle_spec as ds
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, cwire_despeckle_host, lib
from gpu_util import DEV, CUDACore, FarRegion, Guarded, Region
from test_cwire_check_host import m_code_to_255, put_esc

pytestmark = pytest.mark.gpu

MAXB = 5


def diff_tick(core, w, h, pre, frames, stride=None):
    """One tick of mi355_diff_multi_cwire_batch -> (records, frame_pos, states after)."""
    S, n = len(pre), 3 * w * h
    cap = cwire_bytes_max(n, S)
    st, fr = Region(S, n, stride).put(pre), Region(S, n, stride).put(frames)
    off, pos, cw = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.diff_multi_cwire_batch(fr.ptr, st.ptr, S, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
    core.synchronize()
    p = pos.get().view(np.uint64)
    return cw.get()[:int(p[S])].copy(), p.copy(), off.get().view(np.uint32).copy(), st.get()


@functools.lru_cache(maxsize=None)
def gpu_tick(w, h, density, S):
    """ds.tick's streams through mi355_diff_multi_cwire_batch on a fresh core: the records and states are the oracle's."""
    pre, frames, recs, counts, escapes, post = ds.tick(w, h, density, S)
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        got, pos, off, st = diff_tick(core, w, h, pre, frames)
    assert np.array_equal(got, recs) and np.array_equal(st, post), "the tick differs from the oracle's"
    return pre, frames, recs, counts, escapes, post


def host(w, h, recs, counts, escapes, post, need, capacity=None):
    """The host form on copies -> (dropped, offsets, frame_pos, out, states [S, n])."""
    states = np.ascontiguousarray(post).copy()
    d, off, pos, out = cwire_despeckle_host(w, h, recs, counts, escapes, states, need, capacity_bytes=capacity)
    return d, off, pos, out, states.reshape(len(need), -1)


def run(core, w, h, recs, counts, escapes, post, need, stride=None, skew=0, cap=None):
    """-> (dropped, offsets, frame_pos, the whole output buffer, states [S, n]); every guard and the stride gaps asserted."""
    S, n = len(need), 3 * w * h
    cap = cwire_bytes_max(n, S) if cap is None else cap
    st = Region(S, n, stride, skew).put(list(post))
    src = Guarded(recs.size, torch.uint8, data=recs)
    drp, off, pos, out = Guarded(S, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_despeckle_cwire_batch(src.ptr, counts, escapes, st.ptr, S, need, drp.ptr, off.ptr, pos.ptr, out.ptr, cap, stride=st.stride)
    core.synchronize()
    assert np.array_equal(src.get(), recs), "the input records were written"
    return drp.get().view(np.uint32), off.get().view(np.uint32), pos.get().view(np.uint64), out.get(), st.get()


def check(core, w, h, recs, counts, escapes, post, need, **layout):
    want = host(w, h, recs, counts, escapes, post, need)
    got = run(core, w, h, recs, counts, escapes, post, need, **layout)
    what = (w, h, list(need), layout)
    end = int(want[2][-1])
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[3][:end], want[3][:end]), what
    assert (got[3][end:] == 0x5C).all(), (what, "written behind the last record")
    assert np.array_equal(got[4], want[4]), what
    return want


def head(recs, counts, escapes, post, S):
    """The first S streams of a tick."""
    end = int(sum(spec.frame_bytes(n, e) for n, e in zip(counts[:S], escapes[:S])))
    return recs[:end], counts[:S], escapes[:S], post[:S]


# ---- 1. every shape, need and layout against the host form ------------------------------------------------------------------
def layouts(w, h):
    n = 3 * w * h
    if (w, h) == (37, 11):                     # N = 1221: stride == N (odd), a 16-byte aligned and an unaligned stride > N
        return [dict(), dict(stride=1232), dict(stride=1225, skew=3)]
    if (w, h) == (33, 9):
        return [dict(), dict(stride=n + 1, skew=1)]
    return [dict()]


@pytest.mark.parametrize("shape", ds.SHAPES, ids=lambda s: "%dx%d" % s)
def test_equals_the_host_form(shape):
    w, h = shape
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        for density in ds.DENSITIES:
            pre, frames, recs, counts, escapes, post = gpu_tick(w, h, density, 2)
            for need in range(9):
                for layout in layouts(w, h):
                    want = check(core, w, h, recs, counts, escapes, post, [need, need], **layout)
                kept, gone = int(want[1][1]), int(want[0][0])
                if need == 0:
                    assert gone == 0 and np.array_equal(want[3][:recs.size], recs)
                elif density == ds.density_for(need) and min(w, h) > 2:
                    assert kept > 0 and gone > 0, (shape, density, need)
                elif ds.degenerate(w, h, need):
                    assert kept == 0 and np.array_equal(want[4], pre)


@pytest.mark.parametrize("shape", [(37, 11), (64, 48), (1400, 3), (2, 40)], ids=lambda s: "%dx%d" % s)
def test_mixed_need_across_five_streams(shape):
    w, h = shape
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        for density, needs in ((0.7, ([3, 0, 8, 5, 4], [0, 0, 4, 0, 6])), (0.3, ([1, 2, 0, 5, 3],))):
            pre, frames, recs, counts, escapes, post = gpu_tick(w, h, density, 5)
            for need in needs:
                for S in (5, 3):
                    check(core, w, h, *head(recs, counts, escapes, post, S), need[:S])


# ---- 2. guarantee 1: a diff on blanked frames -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 11), (64, 48), (160, 120), (1400, 3), (2, 40)], ids=lambda s: "%dx%d" % s)
def test_equals_a_diff_on_blanked_frames(shape):
    w, h = shape
    S, need = 3, [3, 5, 1]
    pre, frames, recs, counts, escapes, post = gpu_tick(w, h, 0.7, 5)
    pre, frames = pre[:S], frames[:S]
    recs, counts, escapes, post = head(recs, counts, escapes, post, S)
    blank = ds.blanked(pre, frames, recs, need, w, h)
    assert (blank != frames).any()
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        drp, off, pos, out, states = run(core, w, h, recs, counts, escapes, post, need)
        wrecs, wpos, woff, wstates = diff_tick(core, w, h, pre, blank)
    assert np.array_equal(off, woff) and np.array_equal(pos, wpos)
    assert np.array_equal(out[:wrecs.size], wrecs) and np.array_equal(states, wstates)
    assert np.array_equal(drp, counts - np.diff(woff))


# ---- 3. guarantee 2: untouched streams --------------------------------------------------------------------------------------
def test_untouched_streams_come_back_byte_for_byte():
    """need 0, and a full frame at need 3 (a corner has three neighbours): records and states as they were, the gap intact."""
    w, h, S = 37, 11, 3
    n = 3 * w * h
    pre0, fr0 = ds.frames_for(w, h, 0.3, 0)
    rng = np.random.default_rng(5)
    pre1 = rng.integers(0, 256, n, dtype=np.uint8)
    fr1 = (pre1.astype(np.int64) + np.where(pre1 < 128, 50, -50)).astype(np.uint8)       # every byte changes by 50
    pre, frames = np.stack([pre0, pre1, pre0]), np.stack([fr0, fr1, fr0])
    recs, counts, escapes, post = ds.tick_of(pre, frames)
    assert counts[1] == n
    need = [0, 3, 3]
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        for layout in (dict(), dict(stride=n + 11, skew=5)):
            want = check(core, w, h, recs, counts, escapes, post, need, **layout)      # (Region.get asserts the gap's guard bytes)
            for s in (0, 1):
                a, b = int(want[2][s]), int(want[2][s + 1])
                assert want[0][s] == 0 and np.array_equal(want[3][a:b], recs[a:b]) and np.array_equal(want[4][s], post[s])
            assert want[0][2] > 0


# ---- 4. guarantee 5: no stale scratch ---------------------------------------------------------------------------------------
def test_consecutive_calls_are_independent():
    """A dense call, a sparse call with fewer streams, the dense one again, then a call that filters other streams than the one
    before: each equals the host form."""
    w, h = 64, 48
    dense = gpu_tick(w, h, 0.7, 5)[2:]
    sparse = head(*gpu_tick(w, h, 0.05, 2)[2:], 2)
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        check(core, w, h, *dense, [3, 3, 8, 1, 5])
        check(core, w, h, *sparse, [1, 2])
        check(core, w, h, *dense, [3, 3, 8, 1, 5])
        check(core, w, h, *sparse, [0, 1])
        check(core, w, h, *dense, [0, 4, 0, 2, 0])
        check(core, w, h, *dense, [5, 0, 6, 0, 1])


# ---- 5. chained behind the diff, nothing waited for in between --------------------------------------------------------------
def test_two_ticks_without_a_synchronisation():
    """diff, despeckle, diff, despeckle on ONE core with a single synchronisation at the end (the headers the host needs are
    those of the same ticks made beforehand by the oracle and the host form).  The states equal the reference's after both
    ticks, and a host client that applies the sent records holds the sender's state."""
    w, h, S = 64, 48, 3
    n = 3 * w * h
    need = [3, 2, 4]
    base, f1 = (np.stack(z) for z in zip(*[ds.frames_for(w, h, 0.3, s) for s in range(S)]))

    def tick(pre, frames):
        recs, counts, escapes, post = ds.tick_of(pre, frames)
        d, off, pos, out, states = host(w, h, recs, counts, escapes, post, need)
        assert d.all() and off[S] > 0
        return (recs, counts, escapes), d, out[:int(pos[S])], states

    in1, d1, out1, state1 = tick(base, f1)
    f2 = np.stack([ds.frames_for(w, h, 0.3, 10 + s, pre=state1[s])[1] for s in range(S)])     # the next frames move on from the states
    in2, d2, out2, state2 = tick(state1, f2)
    cap = cwire_bytes_max(n, S)
    st, fr1, fr2 = Region(S, n).put(base), Region(S, n).put(f1), Region(S, n).put(f2)
    bufs = [(Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap), Guarded(S, torch.int32),
             Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)) for _ in range(2)]
    ticks = []
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        core.prepare(lib.PREPARE_DESPECKLE)
        torch.cuda.synchronize()                             # (every buffer is filled before the first call is enqueued)
        for fr, (recs, counts, escapes), (off, pos, cw, drp, ooff, opos, out) in ((fr1, in1, bufs[0]), (fr2, in2, bufs[1])):
            core.diff_multi_cwire_batch(fr.ptr, st.ptr, S, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
            core.cwire_despeckle_cwire_batch(cw.ptr, counts, escapes, st.ptr, S, need, drp.ptr, ooff.ptr, opos.ptr, out.ptr, cap,
                                             stride=st.stride)
            ticks.append((cw, recs, drp, opos, out))
        core.synchronize()
    assert np.array_equal(st.get(), state2)
    client = base.copy()
    for (cw, recs, drp, opos, out), wd, wout in zip(ticks, (d1, d2), (out1, out2)):
        assert np.array_equal(cw.get()[:recs.size], recs), "the tick's records are those the headers were read from"
        assert np.array_equal(drp.get().view(np.uint32), wd)
        made, p = out.get(), opos.get().view(np.uint64)
        assert np.array_equal(made[:int(p[S])], wout)
        for s in range(S):
            sl = made[int(p[s]):int(p[s + 1])]
            assert cwire_apply_host(client[s], sl, 1) == sl.size
    assert np.array_equal(client, state2), "the host client holds the sender's state"


# ---- 5b. states more than 4 GiB apart ---------------------------------------------------------------------------------------
def test_states_far_apart():
    """The states' spacing is 64-bit arithmetic: two states 4 GiB and 4099 bytes apart (unaligned), every byte between them
    a guard byte that must survive (gpu_util.FarRegion asserts it on the device)."""
    w, h, S = 64, 48, 2
    n = 3 * w * h
    stride = (1 << 32) + 4099
    recs, counts, escapes, post = head(*gpu_tick(w, h, 0.7, 2)[2:], S)
    need = [3, 5]
    wd, woff, wpos, wout, wst = host(w, h, recs, counts, escapes, post, need)
    assert wd.all()
    cap = cwire_bytes_max(n, S)
    st = FarRegion(S, n, stride, skew=3).put(post)
    src = Guarded(recs.size, torch.uint8, data=recs)
    drp, off, pos, out = Guarded(S, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        torch.cuda.synchronize()
        core.cwire_despeckle_cwire_batch(src.ptr, counts, escapes, st.ptr, S, need, drp.ptr, off.ptr, pos.ptr, out.ptr, cap, stride=stride)
        core.synchronize()
    assert np.array_equal(st.get(), wst)
    st.free()
    assert np.array_equal(drp.get().view(np.uint32), wd) and np.array_equal(pos.get().view(np.uint64), wpos)
    assert np.array_equal(out.get()[:int(wpos[S])], wout[:int(wpos[S])])


# ---- 6. capacity ------------------------------------------------------------------------------------------------------------
def test_capacity():
    """Exactly the needed bytes pass; with fewer the records that end past the capacity are skipped whole, the earlier ones are
    written, frame_pos stays exact and the states are still reverted."""
    w, h, S = 64, 48, 3
    recs, counts, escapes, post = head(*gpu_tick(w, h, 0.7, 5)[2:], S)
    need = [3, 5, 2]
    wd, woff, wpos, wrecs, wstates = host(w, h, recs, counts, escapes, post, need)
    full = int(wpos[S])
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        for cap in (full, full - 1, int(wpos[2]) - 4, int(wpos[1]), 0):
            drp, off, pos, out, states = run(core, w, h, recs, counts, escapes, post, need, cap=cap)
            assert out.size == cap
            assert np.array_equal(drp, wd) and np.array_equal(off, woff) and np.array_equal(pos, wpos), cap
            assert np.array_equal(states, wstates), (cap, "the states are reverted whatever fits")
            for s in range(S):
                a, b = int(wpos[s]), int(wpos[s + 1])
                if b <= cap:
                    assert np.array_equal(out[a:b], wrecs[a:b]), (cap, s)
                else:
                    assert (out[min(a, cap):cap] == 0x5C).all(), (cap, s, "a record that does not fit is skipped whole")


# ---- 7. the prepare bit -----------------------------------------------------------------------------------------------------
def test_with_and_without_the_prepare_bit():
    w, h, T = 64, 48, 7
    n = 3 * w * h
    recs, counts, escapes, post = gpu_tick(w, h, 0.7, 5)[2:]
    need = [3, 3, 8, 1, 5]
    scratch = 2 * T * 4 * ((w * h + 31) // 32)
    got = []
    for prepare in (True, False):
        with CUDACore(w, h, max_batch=T, threshold=ds.THR) as core:
            before = core.workspace_bytes
            if prepare:
                core.prepare(lib.PREPARE_ALL)
                before = core.workspace_bytes          # (PREPARE_ALL does not contain the bit)
                core.prepare(lib.PREPARE_DESPECKLE)
                assert core.workspace_bytes == before + scratch
                core.prepare(lib.PREPARE_DESPECKLE)
                assert core.workspace_bytes == before + scratch, "the prepare is idempotent"
            got.append(check(core, w, h, recs, counts, escapes, post, need))
            assert core.workspace_bytes == before + scratch, "the scratch is made once and counted"
            check(core, w, h, recs, counts, escapes, post, need)
            assert core.workspace_bytes == before + scratch
            L = lib.load()
            assert L.mi355_prepare(core._h, 1 << 9) == lib.ERR_INVALID and L.mi355_prepare(core._h, 64 | 1 << 9) == lib.ERR_INVALID
    for a, b in zip(*got):
        assert np.array_equal(a, b)


# ---- 8. malformed content under consistent headers --------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["escape ranked past e", "index past N"])
def test_malformed_stream_leaves_the_others_exact(how):
    w, h, S = 160, 120, 3
    n = 3 * w * h
    recs, counts, escapes, post = head(*gpu_tick(w, h, 0.05, 3)[2:], S)
    need = [2, 2, 2]
    a, b = (int(sum(spec.frame_bytes(c, e) for c, e in zip(counts[:k], escapes[:k]))) for k in (1, 2))
    n1, e1 = int(counts[1]), int(escapes[1])
    assert e1 >= 1, "the sparse stream has escapes"
    bad = recs[a:b].copy()
    if how == "escape ranked past e":
        bad = m_code_to_255(bad, n1, e1, n, np.random.default_rng(3))      # one more 255 code than escape words
    else:
        put_esc(bad, n1, 0, n + 12345)                                      # the running index leaves the frame at once
    damaged = recs.copy()
    damaged[a:b] = bad
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        drp, off, fp, out, states = run(core, w, h, damaged, counts, escapes, post, need)     # (guards and gaps asserted inside)
    for s in (0, 2):                                         # each of the others equals the host form on it alone
        lo, hi = (0, a) if s == 0 else (b, recs.size)
        wd, woff, wpos, wout, wst = host(w, h, recs[lo:hi], counts[s:s + 1], escapes[s:s + 1], post[s:s + 1], need[s:s + 1])
        assert drp[s] == wd[0] and off[s + 1] - off[s] == woff[1] and fp[s + 1] - fp[s] == wpos[1], (how, s)
        assert np.array_equal(out[int(fp[s]):int(fp[s + 1])], wout[:int(wpos[1])]), (how, s)
        assert np.array_equal(states[s], wst[0]), (how, s)
    assert int(fp[S]) <= out.size and (out[int(fp[S]):] == 0x5C).all()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, S = 64, 48, 2
    n = 3 * w * h
    recs, counts, escapes, post = head(*gpu_tick(w, h, 0.7, 2)[2:], S)
    counts, escapes = counts.copy(), escapes.copy()
    cap = cwire_bytes_max(n, S)
    need = np.array([3, 2], np.uint32)
    # one buffer that holds the input in front and room behind it, for the overlap cases; one that holds the states likewise
    big = Guarded(recs.size + cap + 64, torch.uint8)
    big.t[:recs.size].copy_(torch.from_numpy(recs.copy()).to(DEV))
    src = Guarded(recs.size, torch.uint8, data=recs)
    st = Region(S + 2, n).put(list(post))                    # two spare frames behind the S states (they hold the guard value)
    drp, off, pos, out = Guarded(S, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    L = lib.load()
    inside = big.ptr + recs.size - 8
    inside -= inside % 8
    last = st.ptr + (S - 1) * st.stride + n - 8              # inside the last state, 8-aligned
    last -= last % 8
    with CUDACore(w, h, max_batch=MAXB, threshold=ds.THR) as core:
        torch.cuda.synchronize()

        def call(core_=core._h, src_=src.ptr, c_=counts.ctypes.data, e_=escapes.ctypes.data, st_=st.ptr, stride_=st.stride, S_=S,
                 n_=need.ctypes.data, drp_=drp.ptr, off_=off.ptr, pos_=pos.ptr, out_=out.ptr, cap_=cap):
            return L.mi355_cwire_despeckle_cwire_batch(core_, src_, c_, e_, st_, stride_, S_, n_, drp_, off_, pos_, out_, cap_)

        more_e = (escapes + counts + 1).astype(np.uint32)
        more_n = np.full(S, n + 1, np.uint32)
        zero_e = np.zeros(S, np.uint32)
        nine = np.array([3, 9], np.uint32)
        cases = [
            call(core_=None), call(S_=-1), call(S_=MAXB + 1),
            call(src_=None), call(c_=None), call(e_=None), call(st_=None), call(n_=None), call(drp_=None), call(off_=None),
            call(pos_=None), call(out_=None),
            call(e_=more_e.ctypes.data), call(c_=more_n.ctypes.data, e_=zero_e.ctypes.data), call(n_=nine.ctypes.data),
            call(stride_=n - 1),
            call(src_=src.ptr + 2), call(out_=out.ptr + 2), call(off_=off.ptr + 2), call(drp_=drp.ptr + 2), call(pos_=pos.ptr + 4),
            # the input span [big, big + recs.size) against every output region and the states
            call(src_=big.ptr, out_=big.ptr + recs.size - 4), call(src_=big.ptr, out_=big.ptr - 4, cap_=8),
            call(src_=big.ptr, off_=big.ptr + recs.size - 4), call(src_=big.ptr, drp_=big.ptr + recs.size - 4),
            call(src_=big.ptr, pos_=inside), call(src_=big.ptr, st_=big.ptr + recs.size - 1),
            call(src_=st.ptr + (S - 1) * st.stride + n - 4),
            # an output region against the states' region
            call(out_=last), call(out_=st.ptr - 4, cap_=8), call(off_=last), call(drp_=last), call(pos_=last),
        ]
        assert all(rc == lib.ERR_INVALID for rc in cases), cases
        core.synchronize()
        assert core.workspace_bytes > 0
        for g in (drp, off, pos, out):
            g.get(written=0)
        assert np.array_equal(src.get(), recs)
        h_big = big.get()
        assert np.array_equal(h_big[:recs.size], recs) and (h_big[recs.size:] == 0x5C).all()
        rows = st.get()
        assert np.array_equal(rows[:S], post) and (rows[S:] == 0x5C).all()
        # nstreams == 0: offsets[0] = 0 and frame_pos[0] = 0 and nothing else
        assert call(S_=0) == lib.OK
        core.synchronize()
        assert off.get(written=1)[0] == 0 and pos.get(written=1)[0] == 0
        for g in (drp, out):
            g.get(written=0)
        assert np.array_equal(st.get()[:S], post)
        # ... and the calls above left the core in order: the tick is despeckled
        assert call() == lib.OK
        core.synchronize()
        wd, woff, wpos, wout, wst = host(w, h, recs, counts, escapes, post, need)
        assert np.array_equal(drp.get().view(np.uint32), wd) and np.array_equal(pos.get().view(np.uint64), wpos)
        assert np.array_equal(out.get()[:int(wpos[S])], wout[:int(wpos[S])]) and np.array_equal(st.get()[:S], wst)

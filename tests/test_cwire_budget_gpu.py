"""-m gpu: mi355_cwire_budget_cwire_batch -- the records of one tick of S cameras thinned to an entry budget each, the caller's
states reverted where an entry is dropped (include/mi355diff.h, "A tick held to a budget").  The reference of every comparison is
numpy plus the library's existing entry point: the input records are decoded with cwire_spec, the magnitudes come from the
pre-tick states and the frames, T_s from a numpy histogram, and the expected records, offsets, frame positions and states are
those of mi355_diff_multi_cwire_batch on a fresh core created with threshold T_s, cross-checked against cwire_spec.encode of the
filtered entries.  Inputs, outputs and states live in guarded buffers (gpu_util) that start as a non-zero pattern."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib, synth
from gpu_util import DEV, CUDACore, Guarded, Region

pytestmark = pytest.mark.gpu

NOLIMIT = 0xFFFFFFFF
MAXB = 5


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def isolated_pair(n, s):
    """Entries more than 4096 bytes apart, one per tile at most, every magnitude different (one of them through the wrap:
    250 -> 10 is a = 240 with the diff byte 16)."""
    pre = np.full(n, 100, np.uint8)
    cur = pre.copy()
    xs = 100 + 37 * s + 4200 * np.arange(n // 4200)
    for k, x in enumerate(xs):
        cur[x] = 100 + (21 + 9 * k) * (1 if k % 2 else -1) if 21 + 9 * k <= 100 else 100 + 21 + 9 * k
    pre[xs[-1]], cur[xs[-1]] = 250, 10
    return pre, cur


CASES = {   # name: (w, h, core threshold)
    "webcam-15x1": (15, 1, 20), "webcam-37x11": (37, 11, 20), "webcam-64x48": (64, 48, 20),
    "refrand-15x1": (15, 1, 20), "refrand-37x11": (37, 11, 20), "refrand-64x48": (64, 48, 20),
    "refrand-64x48-thr0": (64, 48, 0), "refrand-64x48-thr200": (64, 48, 200),
    "edge-256x256": (256, 256, 20), "isolated-256x64": (256, 64, 20),
}


def pair(case, s):
    """(pre-tick state, frame) of stream s."""
    w, h, _ = CASES[case]
    n = 3 * w * h
    kind = case.split("-")[0]
    if kind == "webcam":
        base, fr = synth.webcam_stream(1, w, h, seed=1 + 7 * s)
        return base, fr[0]
    if kind == "refrand":
        return synth.refrand_frame(n, 11 + 2 * s), synth.refrand_frame(n, 12 + 2 * s)
    if kind == "edge":
        cur, prev = synth.edge_strip(3)          # every (prev, cur) byte pair, three times: 196608 = 3 * 256 * 256 bytes
        assert cur.size == n
        return [(prev, cur), (cur, prev), (np.roll(prev, 1), cur), (prev, np.roll(cur, 5)), (np.roll(prev, 77), cur)][s]
    return isolated_pair(n, s)


def diff_tick(w, h, thr, pre, frames):
    """One tick of mi355_diff_multi_cwire_batch on a fresh core of threshold thr -> (records, frame_pos, offsets, states after)."""
    S, n = len(pre), 3 * w * h
    cap = cwire_bytes_max(n, S)
    st, fr = Region(S, n).put(pre), Region(S, n).put(frames)
    off, pos, cw = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    with CUDACore(w, h, max_batch=max(S, 1), threshold=int(thr)) as core:
        torch.cuda.synchronize()
        core.diff_multi_cwire_batch(fr.ptr, st.ptr, S, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
        core.synchronize()
    p = pos.get().view(np.uint64)
    return cw.get()[:int(p[S])].copy(), p.copy(), off.get().view(np.uint32).copy(), st.get()


@functools.lru_cache(maxsize=None)
def tick(case):
    """The tick of MAXB streams at the core's threshold, made once per case and read-only: (pre [S][n], frames [S][n], records,
    frame_pos, counts, escapes, states after [S][n], per stream (xs, diff, a))."""
    w, h, thr = CASES[case]
    pre, frames = (np.stack(z) for z in zip(*[pair(case, s) for s in range(MAXB)]))
    recs, pos, _, post = diff_tick(w, h, thr, pre, frames)
    counts, escapes = spec.headers(recs, MAXB)
    off, xs, df = spec.decode(recs, MAXB)
    ent = []
    for s in range(MAXB):
        x, d = xs[int(off[s]):int(off[s + 1])], df[int(off[s]):int(off[s + 1])]
        a = np.abs(frames[s][x].astype(np.int64) - pre[s][x].astype(np.int64))      # from the pre-tick state and the frame
        assert (a > thr).all()
        ent.append((x, d, a))
    out = (pre, frames, recs, pos, counts, escapes, post, ent)
    for z in (pre, frames, recs, pos, counts, escapes, post):
        z.setflags(write=False)
    return out


def threshold_for(a, thr0, budget):
    """The least T in [thr0, 255] with at most `budget` magnitudes above it, from a numpy histogram."""
    hist = np.bincount(a, minlength=256)
    above = hist[::-1].cumsum()[::-1]                       # above[T] = entries with a >= T
    for T in range(thr0, 256):
        if (int(above[T + 1]) if T < 255 else 0) <= budget:
            return T
    raise AssertionError("T = 255 keeps nothing")


@functools.lru_cache(maxsize=None)
def reference_stream(case, s, T):
    """Stream s of the case diffed by a fresh core of threshold T -> (record bytes, entries, state after); cross-checked against
    cwire_spec.encode of the entries with a > T and against the state rule."""
    w, h, thr0 = CASES[case]
    pre, frames, recs, pos, counts, escapes, post, ent = tick(case)
    if T == thr0:
        rec, n, state = recs[int(pos[s]):int(pos[s + 1])], int(counts[s]), post[s]
    else:
        rec, _, off, st = diff_tick(w, h, T, pre[s:s + 1], frames[s:s + 1])
        n, state = int(off[1]), st[0]
    x, d, a = ent[s]
    keep = a > T
    want, _ = spec.encode(np.array([0, int(keep.sum())], np.uint32), x[keep], d[keep])
    assert n == int(keep.sum()) and np.array_equal(rec, want)
    rule = post[s].copy()
    rule[x[~keep]] = pre[s][x[~keep]]                       # cur - diff = prev at the dropped entries
    assert np.array_equal(state, rule)
    return rec, n, state


PATTERNS = ("nolimit", "n", "n-1", "half", "eighth", "zero", "mixed")


def budgets_for(case, S, pattern):
    ns = [len(tick(case)[7][s][0]) for s in range(S)]
    one = {"nolimit": lambda n: NOLIMIT, "n": lambda n: n, "n-1": lambda n: max(n - 1, 0), "half": lambda n: n // 2,
           "eighth": lambda n: n // 8, "zero": lambda n: 0}
    if pattern == "mixed":
        order = ("nolimit", "half", "n-1", "zero", "eighth")
        return np.array([one[order[s % 5]](ns[s]) for s in range(S)], np.uint32)
    return np.array([one[pattern](n) for n in ns], np.uint32)


def expected(case, S, budgets):
    """-> (thresholds uint32[S], offsets uint32[S + 1], frame_pos uint64[S + 1], records, states [S][n]) from the reference."""
    thr0 = CASES[case][2]
    ent = tick(case)[7]
    thr, recs, ns, states = [], [], [], []
    for s in range(S):
        a = ent[s][2]
        T = threshold_for(a, thr0, int(budgets[s]))
        if int(budgets[s]) < len(a):
            assert T > thr0, (case, s, "a budget below the count must raise the threshold")
        else:
            assert T == thr0
        rec, n, state = reference_stream(case, s, T)
        assert n <= int(budgets[s])
        thr.append(T); recs.append(rec); ns.append(n); states.append(state)
    pos = np.cumsum([0] + [r.size for r in recs]).astype(np.uint64)
    off = np.cumsum([0] + ns).astype(np.uint32)
    return np.array(thr, np.uint32), off, pos, np.concatenate(recs), np.stack(states)


# ---- the call under test --------------------------------------------------------------------------------------------------
def run(core, case, S, budgets, stride=None, skew=0, cap=None, recs=None, post=None):
    """-> (thresholds, offsets, frame_pos, the whole output buffer, states [S][n]); every guard and the stride gaps asserted."""
    w, h, _ = CASES[case]
    n = 3 * w * h
    t = tick(case)
    recs = t[2][:int(t[3][S])] if recs is None else recs
    post = t[6][:S] if post is None else post
    cap = cwire_bytes_max(n, S) if cap is None else cap
    st = Region(S, n, stride, skew).put(list(post))
    src = Guarded(recs.size, torch.uint8, data=recs)
    thr, off, pos, out = Guarded(S, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_budget_cwire_batch(src.ptr, t[4][:S], t[5][:S], st.ptr, S, budgets, thr.ptr, off.ptr, pos.ptr, out.ptr, cap,
                                  stride=st.stride)
    core.synchronize()
    assert np.array_equal(src.get(), recs), "the input records were written"
    return thr.get().view(np.uint32), off.get().view(np.uint32), pos.get().view(np.uint64), out.get(), st.get()


def check(core, case, S, budgets, **layout):
    want = expected(case, S, budgets)
    thr, off, pos, out, states = run(core, case, S, budgets, **layout)
    what = (case, S, list(budgets), layout)
    assert np.array_equal(thr, want[0]), what
    assert np.array_equal(off, want[1]) and np.array_equal(pos, want[2]), what
    assert np.array_equal(out[:want[3].size], want[3]), what
    assert (out[want[3].size:] == 0x5C).all(), (what, "written behind the last record")
    assert np.array_equal(states, want[4]), what
    return want


# ---- 1. every input, shape, stream count and budget -----------------------------------------------------------------------
def layouts(case):
    if case.endswith("37x11"):                 # N = 1221: stride == N (odd), a 16-byte aligned and an unaligned stride > N
        return [dict(), dict(stride=1232), dict(stride=1225, skew=3)]
    return [dict()]


@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("case", sorted(CASES))
def test_budget_against_a_core_of_the_chosen_threshold(case, S):
    w, h, thr0 = CASES[case]
    ent = tick(case)[7]
    if case == "refrand-64x48":
        assert all(len(ent[s][0]) > 4096 for s in range(S)), "two directory chunks per record"
    if case.startswith("isolated"):
        assert all((np.diff(ent[s][0]) > 4096).all() and len(ent[s][0]) >= 8 for s in range(S))
    if case.startswith("edge"):                # the magnitude is not a function of the diff byte: df and df +- 256 share it
        x, d, a = ent[0]
        assert any(len(set(a[d == v])) > 1 for v in (16, 100, 240))
    with CUDACore(w, h, max_batch=MAXB, threshold=thr0) as core:
        for pattern in PATTERNS:
            budgets = budgets_for(case, S, pattern)
            for layout in layouts(case):
                want = check(core, case, S, budgets, **layout)
            if pattern in ("nolimit", "n"):    # a stream within its budget comes back byte for byte, its state as it was
                t = tick(case)
                assert np.array_equal(want[3], t[2][:int(t[3][S])]) and np.array_equal(want[4], t[6][:S])
            if pattern == "zero":              # empty 8-byte records, the pre-tick states
                assert int(want[2][S]) == 8 * S and np.array_equal(want[4], tick(case)[0][:S])
            if pattern == "mixed":
                assert (want[0] == thr0).any(), "one stream of a mixed call keeps the core's threshold"


# ---- 2. capacity ----------------------------------------------------------------------------------------------------------
def test_capacity():
    """Exactly the needed bytes pass; with one byte fewer the last record is skipped whole, the earlier ones are written,
    frame_pos stays exact and the states are still thinned."""
    case, S = "refrand-64x48", 3
    w, h, thr0 = CASES[case]
    budgets = budgets_for(case, S, "half")
    wthr, woff, wpos, wrecs, wstates = expected(case, S, budgets)
    need = int(wpos[S])
    with CUDACore(w, h, max_batch=MAXB, threshold=thr0) as core:
        for cap in (need, need - 1, int(wpos[1]), 0):
            thr, off, pos, out, states = run(core, case, S, budgets, cap=cap)
            assert out.size == cap
            assert np.array_equal(thr, wthr) and np.array_equal(off, woff) and np.array_equal(pos, wpos), cap
            assert np.array_equal(states, wstates), (cap, "the states are thinned whatever fits")
            for s in range(S):
                a, b = int(wpos[s]), int(wpos[s + 1])
                if b <= cap:
                    assert np.array_equal(out[a:b], wrecs[a:b]), (cap, s)
                else:
                    assert (out[min(a, cap):cap] == 0x5C).all(), (cap, s, "a record that does not fit is skipped whole")


# ---- 3. two ticks in a row, nothing waited for in between -----------------------------------------------------------------
def test_two_ticks_without_a_synchronisation():
    """diff, budget, diff, budget on ONE core with a single synchronisation at the end (the headers the host needs are those of
    the same ticks made beforehand by the reference).  The states equal the reference's after both ticks, and a host client
    that applies the thinned records holds the sender's state."""
    w, h, thr0, S = 64, 48, 20, 3
    n = 3 * w * h
    base, f1, f2 = [], [], []
    for s in range(S):
        b, fr = synth.webcam_stream(2, w, h, seed=3 + 5 * s)
        base.append(b); f1.append(fr[0]); f2.append(fr[1])
    base, f1, f2 = np.stack(base), np.stack(f1), np.stack(f2)

    def thin(pre, frames):
        """-> (the tick's records at thr0 with their headers, budgets at half, and per stream the reference's thresholds,
        records and states)"""
        recs, pos, _, _ = diff_tick(w, h, thr0, pre, frames)
        counts, escapes = spec.headers(recs, S)
        off, xs, _ = spec.decode(recs, S)
        budgets = (counts // 2).astype(np.uint32)
        thr, out, states = [], [], []
        for s in range(S):
            x = xs[int(off[s]):int(off[s + 1])]
            a = np.abs(frames[s][x].astype(np.int64) - pre[s][x].astype(np.int64))
            T = threshold_for(a, thr0, int(budgets[s]))
            assert T > thr0
            r, _, _, st = diff_tick(w, h, T, pre[s:s + 1], frames[s:s + 1])
            thr.append(T); out.append(r); states.append(st[0])
        return (recs, counts, escapes), budgets, np.array(thr, np.uint32), out, np.stack(states)

    in1, b1, thr1, out1, state1 = thin(base, f1)
    in2, b2, thr2, out2, state2 = thin(state1, f2)
    cap = cwire_bytes_max(n, S)
    st, fr1, fr2 = Region(S, n).put(base), Region(S, n).put(f1), Region(S, n).put(f2)
    ticks = []
    bufs = [(Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap), Guarded(S, torch.int32),
             Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)) for _ in range(2)]
    with CUDACore(w, h, max_batch=MAXB, threshold=thr0) as core:
        torch.cuda.synchronize()                             # (every buffer is filled before the first call is enqueued)
        for fr, (recs, counts, escapes), budgets, (off, pos, cw, thr, ooff, opos, out) in ((fr1, in1, b1, bufs[0]),
                                                                                           (fr2, in2, b2, bufs[1])):
            core.diff_multi_cwire_batch(fr.ptr, st.ptr, S, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
            core.cwire_budget_cwire_batch(cw.ptr, counts, escapes, st.ptr, S, budgets, thr.ptr, ooff.ptr, opos.ptr, out.ptr, cap,
                                          stride=st.stride)
            ticks.append((cw, recs, thr, opos, out))
        core.synchronize()
    assert np.array_equal(st.get(), state2)
    client = base.copy()
    for (cw, recs, thr, opos, out), wthr, wout in zip(ticks, (thr1, thr2), (out1, out2)):
        assert np.array_equal(cw.get()[:recs.size], recs), "the tick's records are those the headers were read from"
        assert np.array_equal(thr.get().view(np.uint32), wthr)
        made, p = out.get(), opos.get().view(np.uint64)
        assert np.array_equal(made[:int(p[S])], np.concatenate(wout))
        for s in range(S):
            sl = made[int(p[s]):int(p[s + 1])]
            assert cwire_apply_host(client[s], sl, 1) == sl.size
    assert np.array_equal(client, state2), "the host client holds the sender's state"


# ---- 4. malformed content under consistent headers ------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["escape ranked past e", "index past N"])
def test_malformed_stream_leaves_the_others_exact(how):
    case, S = "refrand-64x48", 3
    w, h, thr0 = CASES[case]
    n = 3 * w * h
    t = tick(case)
    recs, pos, counts = t[2][:int(t[3][S])].copy(), t[3], t[4]
    code = int(pos[1]) + 8                                   # stream 1's codes
    if how == "escape ranked past e":
        recs[code:code + int(counts[1]):3] = 255             # thousands of escape codes, e of them have a word
    else:
        recs[code:code + int(counts[1])] = 254               # the running index leaves the frame after 37 entries
    budgets = budgets_for(case, S, "half")
    wthr, woff, wpos, wrecs, wstates = expected(case, S, budgets)
    with CUDACore(w, h, max_batch=MAXB, threshold=thr0) as core:
        thr, off, fp, out, states = run(core, case, S, budgets, recs=recs)     # (guards and gaps asserted inside)
    for s in (0, 2):
        assert thr[s] == wthr[s] and off[s + 1] - off[s] == woff[s + 1] - woff[s], (how, s)
        assert fp[s + 1] - fp[s] == wpos[s + 1] - wpos[s], (how, s)
        assert np.array_equal(out[int(fp[s]):int(fp[s + 1])], wrecs[int(wpos[s]):int(wpos[s + 1])]), (how, s)
        assert np.array_equal(states[s], wstates[s]), (how, s)
    assert thr0 <= thr[1] <= 255 and int(fp[S]) <= out.size and (out[int(fp[S]):] == 0x5C).all()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    case, S = "webcam-64x48", 2
    w, h, thr0 = CASES[case]
    n = 3 * w * h
    t = tick(case)
    recs, counts, escapes, post = t[2][:int(t[3][S])], t[4][:S].copy(), t[5][:S].copy(), t[6][:S]
    cap = cwire_bytes_max(n, S)
    budgets = (counts // 2).astype(np.uint32)
    # one buffer that holds the input in front and room behind it, for the overlap cases; one that holds the states likewise
    big = Guarded(recs.size + cap + 64, torch.uint8)
    big.t[:recs.size].copy_(torch.from_numpy(recs).to(DEV))
    src = Guarded(recs.size, torch.uint8, data=recs)
    st = Region(S + 2, n).put(list(post))                    # two spare frames behind the S states (they hold the guard value)
    thr, off, pos, out = Guarded(S, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    L = lib.load()
    inside = big.ptr + recs.size - 8
    inside -= inside % 8
    last = st.ptr + (S - 1) * st.stride + n - 8              # inside the last state, 8-aligned
    last -= last % 8
    with CUDACore(w, h, max_batch=MAXB, threshold=thr0) as core:
        torch.cuda.synchronize()

        def call(core_=core._h, src_=src.ptr, c_=counts.ctypes.data, e_=escapes.ctypes.data, st_=st.ptr, stride_=st.stride, S_=S,
                 b_=budgets.ctypes.data, thr_=thr.ptr, off_=off.ptr, pos_=pos.ptr, out_=out.ptr, cap_=cap):
            return L.mi355_cwire_budget_cwire_batch(core_, src_, c_, e_, st_, stride_, S_, b_, thr_, off_, pos_, out_, cap_)

        more_e = (escapes + counts + 1).astype(np.uint32)
        more_n = np.full(S, n + 1, np.uint32)
        zero_e = np.zeros(S, np.uint32)
        cases = [
            call(core_=None), call(S_=-1), call(S_=MAXB + 1),
            call(src_=None), call(c_=None), call(e_=None), call(st_=None), call(b_=None), call(thr_=None), call(off_=None),
            call(pos_=None), call(out_=None),
            call(e_=more_e.ctypes.data), call(c_=more_n.ctypes.data, e_=zero_e.ctypes.data),
            call(stride_=n - 1),
            call(src_=src.ptr + 2), call(out_=out.ptr + 2), call(off_=off.ptr + 2), call(thr_=thr.ptr + 2), call(pos_=pos.ptr + 4),
            # the input span [big, big + recs.size) against every output region and the states
            call(src_=big.ptr, out_=big.ptr + recs.size - 4), call(src_=big.ptr, out_=big.ptr - 4, cap_=8),
            call(src_=big.ptr, off_=big.ptr + recs.size - 4), call(src_=big.ptr, thr_=big.ptr + recs.size - 4),
            call(src_=big.ptr, pos_=inside), call(src_=big.ptr, st_=big.ptr + recs.size - 1),
            call(src_=st.ptr + (S - 1) * st.stride + n - 4),
            # an output region against the states' region
            call(out_=last), call(out_=st.ptr - 4, cap_=8), call(off_=last), call(thr_=last), call(pos_=last),
        ]
        assert all(rc == lib.ERR_INVALID for rc in cases), cases
        core.synchronize()
        for g in (thr, off, pos, out):
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
        for g in (thr, out):
            g.get(written=0)
        assert np.array_equal(st.get()[:S], post)
        # ... and the calls above left the core in order: the tick is thinned
        assert call() == lib.OK
        core.synchronize()
        want = expected(case, S, budgets)
        assert np.array_equal(thr.get().view(np.uint32), want[0]) and np.array_equal(pos.get().view(np.uint64), want[2])
        assert np.array_equal(out.get()[:want[3].size], want[3]) and np.array_equal(st.get()[:S], want[4])

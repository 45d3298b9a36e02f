"""-m gpu tests of the compact form of the per-frame host entry points (mi355_exec_cwire, mi355_pipe_submit_cwire /
mi355_pipe_wait_cwire): each frame gets what exec_core gives it, and its changes arrive in host memory as ONE canonical
compact record.  The expected record is encoded here, in numpy, from the format description of include/mi355diff.h and the
oracle's entries -- never by the library's own encoder."""
import ctypes as C

import numpy as np
import pytest

from cudavideostream_amd import core as corelib
from cudavideostream_amd import lib, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from gpu_util import DEV, CUDACore  # noqa: E402
from test_filters_gpu import oracle_exec  # noqa: E402

from cudavideostream_amd.core import PinnedArray  # noqa: E402

SENT = 0xC7      # what a record buffer holds before a call
SLACK = 64       # bytes of every record buffer behind the capacity that is passed


def np_record(xs, df):
    """u32 n | u32 e | u8 code[pad4(n)] | u32 esc[e] | u8 diff[pad4(n)], little-endian, pads zero (include/mi355diff.h):
    g_0 = xs[0], g_k = xs[k] - xs[k-1] - 1; code = min(g, 255); esc = the g of the codes 255, in order."""
    xs = np.asarray(xs, np.int64)
    n = xs.size
    g = np.empty(n, np.int64)
    if n:
        g[0] = xs[0]
        g[1:] = xs[1:] - xs[:-1] - 1
    assert (g >= 0).all()
    esc = g[g >= 255].astype("<u4")
    pad = np.zeros((-n) % 4, np.uint8)
    return np.concatenate([np.array([n, esc.size], "<u4").view(np.uint8), np.minimum(g, 255).astype(np.uint8), pad,
                           esc.view(np.uint8), np.asarray(df, np.uint8), pad])


class Rec:
    """A record buffer: cap = cwire_bytes_max(N, 1) bytes that are handed to the library, SLACK more behind them, the first
    `skew` bytes behind a 16-byte aligned address; pinned or pageable."""

    def __init__(self, n, skew=0, pinned=True):
        self.cap = corelib.cwire_bytes_max(n, 1)
        total = skew + self.cap + SLACK
        if pinned:
            self.block = PinnedArray(total + 16)
            whole = self.block.array
        else:
            self.block = None
            whole = np.empty(total + 16, np.uint8)
        lead = (-whole.ctypes.data) % 16 + skew
        self.view = whole[lead:lead + self.cap + SLACK]
        assert self.view.ctypes.data % 16 == skew % 16
        self.fill()

    def fill(self):
        self.view[:] = SENT

    def check(self, got, c, xs, df, old=None):
        """got = (n, e, bytes) of the call; the record is the numpy one and nothing at or past its end was written (old: what
        the buffer held there before the call, the sentinel by default)."""
        want = np_record(xs, df)
        n, e, b = got
        assert (n, b) == (c, want.size), (got, c, want.size)
        assert e == int(want[4:8].view("<u4")[0])
        assert b == corelib.cwire_frame_bytes(n, e)
        assert np.array_equal(self.view[:b], want)
        rest = self.view[b:]
        assert np.array_equal(rest, np.full(rest.size, SENT, np.uint8) if old is None else old[b:])
        return want

    def free(self):
        if self.block is not None:
            self.view = None
            self.block.free()


def pinned_frame(n):
    return PinnedArray(n + 32)


# ---- 1. parity with exec_core ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("vis", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("noise_filter,depth", [(False, 3), (True, 2)])
def test_compact_matches_exec_core_semantics(po, vis, noise_filter, depth):
    w, h, T = 96, 54, 7
    base, frames = synth.webcam_stream(T, w, h, seed=60 + vis)
    k = po.gaussian_kernel(3, 1.5)
    n = 3 * w * h
    want, state = [], base
    for t in range(T):
        c, xs, df, state, show = oracle_exec(po, frames[t], state, vis, k, noise_filter, w, h)
        want.append((c, xs, df, show))
    recs = [Rec(n) for _ in range(depth)]
    fbuf = [pinned_frame(n) for _ in range(depth)]
    sbuf = [pinned_frame(n) for _ in range(depth)]
    client = {}

    def check(t, got, form):
        c, xs, df, show = want[t]
        record = recs[t % depth].check(got, c, xs, df)
        assert np.array_equal(fbuf[t % depth].array[:n], frames[t]), "frame_data was written"
        if show is not None:
            assert np.array_equal(sbuf[t % depth].array[:n], show)
        client.setdefault(form, []).append(record.copy())

    # the blocking form
    with CUDACore(w, h, k=k, sample_mat_data=base, visualizer=vis, noise_filter=noise_filter) as core:
        for t in range(T):
            recs[t % depth].fill()
            fbuf[t % depth].array[:n] = frames[t]
            got = core.exec_core_compact(fbuf[t % depth].array, sbuf[t % depth].array, "", recs[t % depth].view, recs[t % depth].cap)
            check(t, got, "exec")
        assert np.array_equal(core.get_state(), state)
    # the pipe, several frames in flight
    with CUDACore(w, h, k=k, sample_mat_data=base, visualizer=vis, noise_filter=noise_filter) as core:
        core.pipe_open(depth)
        tickets = {}
        for t in range(T):
            if t >= depth:
                check(t - depth, core.exec_wait_compact(tickets.pop(t - depth)), "pipe")   # the slot's buffers are about to be reused
            recs[t % depth].fill()
            fbuf[t % depth].array[:n] = frames[t]
            tickets[t] = core.exec_submit_compact(fbuf[t % depth].array, sbuf[t % depth].array, "", recs[t % depth].view,
                                                  recs[t % depth].cap)
        for t in sorted(tickets):
            check(t, core.exec_wait_compact(tickets[t]), "pipe")
        assert np.array_equal(core.get_state(), state)
        core.pipe_close()
    # a host client that applies the records to the base frame ends at the same state
    for form in ("exec", "pipe"):
        st = np.ascontiguousarray(base).copy()
        stream = np.concatenate(client[form])
        assert corelib.cwire_apply_host(st, stream, T) == stream.size
        assert np.array_equal(st, state)
    for a in recs + fbuf + sbuf:
        a.free()


# ---- 2. record shapes at their edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(5, 3), (64, 48), (96, 54)])   # N = 45: no multiple of 4; 96x54: N no multiple of 1024
@pytest.mark.parametrize("form", ["exec_pinned", "exec_pageable", "pipe1"])
@pytest.mark.parametrize("skew", [0, 4])                         # h_record 16-byte aligned, and 4- but not 16-byte aligned
def test_record_shapes_at_their_edges(po, w, h, form, skew):
    n = 3 * w * h
    rng = np.random.default_rng(1000 * w + skew)
    base = rng.integers(0, 256, n, dtype=np.uint8)
    pinned = form != "exec_pageable"
    rec = Rec(n, skew, pinned)
    fblock = pinned_frame(n) if pinned else None
    frame = fblock.array[:n] if pinned else np.empty(n, np.uint8)
    with CUDACore(w, h, sample_mat_data=base) as core:
        if form == "pipe1":
            core.pipe_open(1)

        def run(cur):
            frame[:] = cur
            if form == "pipe1":
                got = core.exec_wait_compact(core.exec_submit_compact(frame, None, "", rec.view, rec.cap))
            else:
                got = core.exec_core_compact(frame, None, "", rec.view, rec.cap)
            assert np.array_equal(frame, cur), "frame_data was written"
            return got

        state = base
        # every byte changes by 128, far more than the threshold: n = N, e = 0, the capacity bound met exactly
        cur = state + np.uint8(128)
        c, xs, df, state = po.diff_pack(cur, state)
        assert c == n
        got = run(cur)
        rec.check(got, c, xs, df)
        assert got == (n, 0, rec.cap)
        # an identical frame, into the SAME buffer without refilling it: 8 bytes, and the large record's bytes past them stay
        old = rec.view.copy()
        cur = state.copy()
        c, xs, df, state = po.diff_pack(cur, state)
        got = run(cur)
        rec.check(got, c, xs, df, old=old)
        assert got == (0, 0, 8)
        # a few changed bytes at least 256 apart, the first at an index of at least 255: escapes
        if n >= 1024:
            where = np.arange(255 + skew, n, 256 + 41)[:9]
            cur = state.copy()
            cur[where] += np.uint8(100)
            c, xs, df, state = po.diff_pack(cur, state)
            assert c == where.size
            rec.fill()
            got = run(cur)
            rec.check(got, c, xs, df)
            assert got[1] == where.size > 0
        # a webcam-like amount of scattered change: escapes and one-byte gaps mixed, n no multiple of 4
        cur = state.copy()
        count = max(n // 50, 3)
        where = np.sort(rng.choice(n, count - (count - 3) % 4, replace=False))
        assert where.size % 4 == 3
        cur[where] += np.uint8(60)
        c, xs, df, state = po.diff_pack(cur, state)
        rec.fill()
        rec.check(run(cur), c, xs, df)
        assert np.array_equal(core.get_state(), state)
        if form == "pipe1":
            core.pipe_close()
    rec.free()
    if fblock is not None:
        frame = None
        fblock.free()


# ---- 3. several frames in flight at 1080p, plain and compact submits alternating -----------------------------------------
def test_plain_and_compact_alternate_in_flight_1080p(po):
    w, h, T, depth = 1920, 1080, 12, 4
    base, frames = synth.webcam_stream(T, w, h, device=DEV)
    base, frames = base.cpu().numpy(), frames.cpu().numpy()
    n = 3 * w * h
    sets = [CUDACore.alloc_arrays(h, w) for _ in range(depth)]
    recs = [Rec(n) for _ in range(depth)]
    off, xs, df, st = po.diff_stream(frames, base)
    with CUDACore(w, h, sample_mat_data=base) as core:
        core.pipe_open(depth)
        tickets = []

        def finish(t):
            a, b = off[t], off[t + 1]
            if t % 2:   # compact
                recs[t % depth].check(core.exec_wait_compact(tickets[t]), int(b - a), xs[a:b], df[a:b])
                assert np.array_equal(sets[t % depth][0].array[:n], frames[t]), "frame_data was written"
            else:       # plain, as test_pipe_gpu.check_frame
                h_frame, _, _, h_xs = sets[t % depth]
                pos = core.exec_wait(tickets[t])
                assert pos == b - a
                assert np.array_equal(h_xs.array[:pos], xs[a:b])
                assert np.array_equal(h_frame.array[:pos], df[a:b])

        for t in range(T):
            if t >= depth:
                finish(t - depth)
            h_frame, _, _, h_xs = sets[t % depth]
            h_frame.array[:n] = frames[t]
            if t % 2:
                recs[t % depth].fill()
                tickets.append(core.exec_submit_compact(h_frame.array, None, "", recs[t % depth].view, recs[t % depth].cap))
            else:
                tickets.append(core.exec_submit(h_frame.array, None, "", h_xs.array))
        assert tickets == list(range(T))
        for t in range(T - depth, T):
            finish(t)
        assert np.array_equal(core.get_state(), st)
    for s in sets:
        for a in s:
            a.free()
    for r in recs:
        r.free()


# ---- 4. rules ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(po):
    w, h = 64, 48
    n = 3 * w * h
    base, frames = synth.webcam_stream(1, w, h, seed=5)
    k = po.gaussian_kernel(3, 1.5)
    rec, frame, show = Rec(n), pinned_frame(n), pinned_frame(n)
    frame.array[:n] = frames[0]
    pos, esc, nbytes, ticket = C.c_uint32(7), C.c_uint32(7), C.c_size_t(7), C.c_int64(-5)
    f, s, r = frame.array.ctypes.data, show.array.ctypes.data, rec.view.ctypes.data

    def refused(core, code, call):
        rec.fill()
        show.array[:] = SENT
        before = core.get_state()
        assert call() == code, lib.load().mi355_last_error()
        assert (rec.view == SENT).all() and (show.array == SENT).all()
        assert np.array_equal(core.get_state(), before)
        assert (pos.value, esc.value, nbytes.value, ticket.value) == (7, 7, 7, -5)

    L = lib.load()
    out = (C.byref(pos), C.byref(esc), C.byref(nbytes))
    with CUDACore(w, h, sample_mat_data=base, visualizer=lib.VIS_GRAY) as core:
        H = core._h
        for form in ("exec", "pipe"):
            if form == "pipe":
                core.pipe_open(2)
                call = lambda fd, sh, hr, cap: L.mi355_pipe_submit_cwire(H, fd, sh, None, hr, cap, C.byref(ticket))  # noqa: E731
            else:
                call = lambda fd, sh, hr, cap: L.mi355_exec_cwire(H, fd, sh, None, hr, cap, *out)  # noqa: E731
            refused(core, lib.ERR_INVALID, lambda: call(None, s, r, rec.cap))          # what check_exec_args refuses
            refused(core, lib.ERR_INVALID, lambda: call(f, None, r, rec.cap))          # ... a visualiser without show_ready
            refused(core, lib.ERR_INVALID, lambda: call(f, s, None, rec.cap))          # null h_record
            refused(core, lib.ERR_INVALID, lambda: call(f, s, r + 2, rec.cap))         # not 4-byte aligned
            refused(core, lib.ERR_INVALID, lambda: call(f, s, r, rec.cap - 1))         # below the worst case
            refused(core, lib.ERR_INVALID, lambda: call(f, s, r, 0))
        # (the pipe is open)
        refused(core, lib.ERR_INVALID, lambda: L.mi355_pipe_submit_cwire(H, f, s, None, r, rec.cap, None))
        refused(core, lib.ERR_STATE, lambda: L.mi355_exec_cwire(H, f, s, None, r, rec.cap, *out))
        pageable = np.full(n + 32, 3, np.uint8)
        pageable_rec = np.full(rec.cap, SENT, np.uint8)
        refused(core, lib.ERR_INVALID, lambda: L.mi355_pipe_submit_cwire(H, pageable.ctypes.data, s, None, r, rec.cap, C.byref(ticket)))
        refused(core, lib.ERR_INVALID, lambda: L.mi355_pipe_submit_cwire(H, f, pageable.ctypes.data, None, r, rec.cap, C.byref(ticket)))
        refused(core, lib.ERR_INVALID, lambda: L.mi355_pipe_submit_cwire(H, f, s, None, pageable_rec.ctypes.data, rec.cap, C.byref(ticket)))
        assert (pageable_rec == SENT).all() and (pageable == 3).all()
        refused(core, lib.ERR_INVALID, lambda: L.mi355_pipe_wait_cwire(H, 0, *out))   # unknown ticket: nothing was submitted
        for i in range(3):
            bad = list(out)
            bad[i] = None
            refused(core, lib.ERR_INVALID, lambda: L.mi355_pipe_wait_cwire(H, 0, *bad))
        core.pipe_close()
        # no pipe open
        refused(core, lib.ERR_STATE, lambda: L.mi355_pipe_submit_cwire(H, f, s, None, r, rec.cap, C.byref(ticket)))
        refused(core, lib.ERR_STATE, lambda: L.mi355_pipe_wait_cwire(H, 0, *out))
        for i in range(3):
            bad = list(out)
            bad[i] = None
            refused(core, lib.ERR_INVALID, lambda: L.mi355_exec_cwire(H, f, s, None, r, rec.cap, *bad))
        refused(core, lib.ERR_INVALID, lambda: L.mi355_exec_cwire(None, f, s, None, r, rec.cap, *out))
    with CUDACore(w, h, sample_mat_data=base, noise_filter=True) as core:   # the noise filter without its kernel
        refused(core, lib.ERR_STATE, lambda: L.mi355_exec_cwire(core._h, f, None, None, r, rec.cap, *out))
    # ... and the same call goes through once nothing is wrong with it
    with CUDACore(w, h, k=k, sample_mat_data=base, noise_filter=True) as core:
        c, xs, df, _, _ = oracle_exec(po, frames[0], base, 0, k, True, w, h)
        rec.fill()
        rec.check(core.exec_core_compact(frame.array, None, "", rec.view, rec.cap), c, xs, df)
    for a in (rec, frame, show):
        a.free()


def test_ticket_rules_and_ring_overrun(po):
    w, h, T, depth = 64, 48, 5, 2
    base, frames = synth.webcam_stream(T + 2, w, h, seed=71)
    n = 3 * w * h
    off, xs, df, st = po.diff_stream(frames, base)
    recs = [Rec(n) for _ in range(T)]                  # one buffer set per frame: nothing is overwritten
    fbuf = [pinned_frame(n) for _ in range(T)]
    h_xs = PinnedArray(4 * n + 32, np.int32)
    with CUDACore(w, h, sample_mat_data=base) as core:
        core.pipe_open(depth)
        tickets = []
        for t in range(T):                             # never waits: the ring (depth 2) is overrun on purpose
            fbuf[t].array[:n] = frames[t]
            tickets.append(core.exec_submit_compact(fbuf[t].array, None, "", recs[t].view, recs[t].cap))
        assert tickets == list(range(T))
        with pytest.raises(lib.Mi355Error, match="already waited for or overwritten"):
            core.exec_wait_compact(tickets[0])
        with pytest.raises(lib.Mi355Error, match="unknown ticket"):
            core.exec_wait_compact(T)
        got = {T - 1: core.exec_wait_compact(tickets[T - 1])}
        with pytest.raises(lib.Mi355Error, match="already waited"):
            core.exec_wait_compact(tickets[T - 1])
        # exec_wait on a compact ticket is valid and returns n
        assert core.exec_wait(tickets[T - 2]) == off[T - 1] - off[T - 2]
        # frames whose tickets were overrun were still processed, in order, each into its own buffer
        for t in range(T):
            want = np_record(xs[off[t]:off[t + 1]], df[off[t]:off[t + 1]])
            assert np.array_equal(recs[t].view[:want.size], want)
            assert (recs[t].view[want.size:] == SENT).all()
            assert np.array_equal(fbuf[t].array[:n], frames[t])
        recs[T - 1].check(got[T - 1], int(off[T] - off[T - 1]), xs[off[T - 1]:off[T]], df[off[T - 1]:off[T]])
        # a plain ticket: exec_wait_compact is refused, and the ticket is then waited with exec_wait
        t = T
        fbuf[0].array[:n] = frames[t]
        plain = core.exec_submit(fbuf[0].array, None, "", h_xs.array)
        with pytest.raises(lib.Mi355Error, match="mi355_pipe_wait") as ei:
            core.exec_wait_compact(plain)
        assert ei.value.code == lib.ERR_STATE
        pos = core.exec_wait(plain)
        assert pos == off[t + 1] - off[t]
        assert np.array_equal(h_xs.array[:pos], xs[off[t]:off[t + 1]])
        assert np.array_equal(fbuf[0].array[:pos], df[off[t]:off[t + 1]])
        # ... and a compact one behind it
        t = T + 1
        fbuf[1].array[:n] = frames[t]
        recs[1].fill()
        recs[1].check(core.exec_wait_compact(core.exec_submit_compact(fbuf[1].array, None, "", recs[1].view, recs[1].cap)),
                      int(off[t + 1] - off[t]), xs[off[t]:off[t + 1]], df[off[t]:off[t + 1]])
        assert np.array_equal(core.get_state(), st)
        core.pipe_close()
    for a in recs + fbuf + [h_xs]:
        a.free()


def test_exec_core_and_exec_core_compact_alternate(po):
    w, h, T = 96, 54, 6
    base, frames = synth.webcam_stream(T, w, h, seed=9)
    n = 3 * w * h
    off, xs, df, st = po.diff_stream(frames, base)
    rec = Rec(n)
    h_frame, n_frame, o_frame, h_xs = CUDACore.alloc_arrays(h, w)
    with CUDACore(w, h, sample_mat_data=base) as core:
        for t in range(T):
            a, b = off[t], off[t + 1]
            h_frame.array[:n] = frames[t]
            if t % 2 == 0:
                rec.fill()
                rec.check(core.exec_core_compact(h_frame.array, None, "", rec.view, rec.cap), int(b - a), xs[a:b], df[a:b])
                assert np.array_equal(h_frame.array[:n], frames[t])
            else:
                pos = core.exec_core(h_frame.array, None, "", h_xs.array)
                assert pos == b - a
                assert np.array_equal(h_xs.array[:pos], xs[a:b]) and np.array_equal(h_frame.array[:pos], df[a:b])
        assert np.array_equal(core.get_state(), st)
    for a in (rec, h_frame, n_frame, o_frame, h_xs):
        a.free()


def test_prepare_exec_cwire(po):
    w, h = 96, 54
    n = 3 * w * h
    base, frames = synth.webcam_stream(1, w, h, seed=3)
    rec, frame = Rec(n), pinned_frame(n)
    frame.array[:n] = frames[0]
    c, xs, df, st = po.diff_pack(frames[0], base)
    assert lib.PREPARE_EXEC_CWIRE == 32 and lib.PREPARE_ALL == 31
    grow = (corelib.cwire_bytes_max(n, 1) + 15) // 16 * 16 + 16   # the record buffer, rounded up to 16, and its two positions
    with CUDACore(w, h, sample_mat_data=base) as core:
        core.prepare(lib.PREPARE_ALL)
        ws0 = core.workspace_bytes
        core.prepare(lib.PREPARE_EXEC_CWIRE)
        ws1 = core.workspace_bytes
        assert ws1 - ws0 == grow
        core.prepare(lib.PREPARE_EXEC_CWIRE)
        core.prepare(lib.PREPARE_ALL | lib.PREPARE_EXEC_CWIRE)
        assert core.workspace_bytes == ws1
        assert np.array_equal(core.get_state(), base)          # the warm pass ran on an empty frame
        rec.check(core.exec_core_compact(frame.array, None, "", rec.view, rec.cap), c, xs, df)
        assert core.workspace_bytes == ws1
        assert np.array_equal(core.get_state(), st)
        with pytest.raises(lib.Mi355Error) as ei:
            core.prepare(1 << 9)
        assert ei.value.code == lib.ERR_INVALID
    # without the call: the first compact call makes the same, once; pipe_open makes nothing for it
    with CUDACore(w, h, sample_mat_data=base) as core:
        ws0 = core.workspace_bytes
        core.pipe_open(2)
        ws_open = core.workspace_bytes
        rec.fill()
        rec.check(core.exec_wait_compact(core.exec_submit_compact(frame.array, None, "", rec.view, rec.cap)), c, xs, df)
        assert core.workspace_bytes - ws_open == grow
        core.pipe_close()
        assert core.workspace_bytes - ws0 == grow
    # alloc_record: pinned, the capacity the calls ask for
    buf = CUDACore.alloc_record(h, w)
    assert buf.array.nbytes == corelib.cwire_bytes_max(n, 1) and buf.ptr % 16 == 0
    with CUDACore(w, h, sample_mat_data=base) as core:
        got = core.exec_core_compact(frame.array, None, "", buf.array)
        assert np.array_equal(buf.array[:got[2]], np_record(xs, df))
    for a in (rec, frame, buf):
        a.free()

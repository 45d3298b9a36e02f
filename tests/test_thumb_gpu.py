"""-m gpu: mi355_thumb_cwire_batch (include/mi355diff.h, "Thumbnail records").  The reference of every comparison is numpy:
thumb_spec on top of wall_spec (the block average, the required pixels) and cwire_spec (the records), never the code under test.
States, held thumbnails, masks and outputs live in guarded buffers (gpu_util) that start as a non-zero pattern, so every byte
outside the N' bytes of each held thumbnail, the outputs' written part and the stride gaps is checked.

Shapes (thumb_spec.SHAPES; test_thumb_spec.py checks that each produces its condition): 37x11 at k = 1, 2, 3, 4, 16 (one source
tile, ragged right and bottom blocks, thumbnail rows of 30 bytes, a thumbnail one pixel high), 64x48 at k = 16 (the 16-bit column
sums at their top, the rounding tie), 100x60 at k = 2 and 3 (five source tiles, pixel 1365 astride tiles 0 and 1, two thumbnail
tiles with the second partial; one source tile selected, each in turn), 2800x6 at k = 2 (a thumbnail row of 4200 bytes: a tile
inside one row, a row meeting two tiles).  Layouts, S = 3: everything aligned; states at stride N + 5 one byte behind an aligned
address with thumbnails at stride N' + 3 one byte behind one."""
import numpy as np
import pytest
import torch

import cwire_spec as spec
import thumb_spec as ts
import wall_spec as ws
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib
from gpu_util import DEV, GUARD, CUDACore, Guarded, Region

pytestmark = pytest.mark.gpu

S = 3
LAYOUTS = [("aligned", 0, None, 0, None), ("skewed", 1, 5, 1, 3)]   # (name, states' skew, stride - N, thumbs' skew, stride - N')


def aligned(n):
    return (n + 15) // 16 * 16


def regions(layout, n, nt, states, thumbs):
    _, sk, ex, tsk, tex = layout
    return (Region(S, n, aligned(n) if ex is None else n + ex, sk).put(states),
            Region(S, nt, aligned(nt) if tex is None else nt + tex, tsk).put(thumbs))


def mask_buffer(sel):
    """bool[S, tiles] -> a guarded device copy of uint32[S, mask_words], the bits at or past `tiles` set (they are ignored)."""
    rows = ws.mask_of(sel)
    t = sel.shape[1]
    if t % 32:
        rows[:, -1] |= np.uint32((0xFFFFFFFF << (t % 32)) & 0xFFFFFFFF)
    return Guarded(rows.size, torch.int32, data=rows.view(np.int32).ravel())


class Out:
    """The three outputs of one call in guarded buffers."""

    def __init__(self, nstreams, cap):
        self.S, self.cap = nstreams, cap
        self.off, self.pos, self.out = Guarded(nstreams + 1, torch.int32), Guarded(nstreams + 1, torch.int64), Guarded(cap)
        assert self.out.ptr % 4 == 0 and self.pos.ptr % 8 == 0

    def results(self):
        """(offsets uint32, frame_pos uint64, out uint8[cap]); the guards asserted."""
        return (self.off.get().view(np.uint32).copy(), self.pos.get().view(np.uint64).copy(), self.out.get().copy())


def thumb_call(core, k, thr, st, th, mask, o, nstreams=S):
    core.thumb_cwire_batch(st.ptr, nstreams, k, thr, th.ptr, o.off.ptr, o.pos.ptr, o.out.ptr, o.cap,
                           d_tile_mask=None if mask is None else mask.ptr, stride=st.stride, thumb_stride=th.stride)


def run(core, w, h, k, thr, st, th, sel, cap=None):
    """One synchronised call -> (offsets, frame_pos, out, held thumbnails after); every guard asserted."""
    nt = ts.thumb_bytes(w, h, k)
    o = Out(S, cwire_bytes_max(nt, S) if cap is None else cap)
    mask = None if sel is None else mask_buffer(sel)
    torch.cuda.synchronize()
    thumb_call(core, k, thr, st, th, mask, o)
    core.synchronize()
    if mask is not None:
        mask.get()
    return o.results() + (th.get(),)


def assert_equals_spec(got, want, what=""):
    off, pos, out, after = got
    woff, wpos, wrecs, wafter = want
    assert np.array_equal(off, woff) and np.array_equal(pos, wpos), what
    for s, rec in enumerate(wrecs):
        a, b = int(wpos[s]), int(wpos[s + 1])
        if rec is None:
            assert (out[a:min(b, out.size)] == GUARD).all(), f"{what}: a byte of skipped record {s} was written"
        else:
            assert out[a:b].tobytes() == rec, f"{what}: record {s}"
    assert (out[int(wpos[-1]):] == GUARD).all(), what
    assert np.array_equal(after, wafter), what


def tick(rng, prev, sel):
    """The states after a tick that changes bytes inside the selected tiles only (about one in eight of them)."""
    hit = np.repeat(sel, ws.TILE, axis=1)[:, :prev.shape[1]] & (rng.random(prev.shape) < 0.125)
    out = prev.copy()
    out[hit] += rng.integers(1, 256, int(hit.sum()), dtype=np.uint8)
    return out


def selections(rng, n):
    t = ws.tiles(n)
    sels = [None, rng.random((S, t)) < 0.4, np.zeros((S, t), bool)]
    if n == 18000:
        sels += [np.repeat(row[None, :], S, axis=0) for row in ts.one_tile_masks(n)]
    return sels


# ---- 1. law 3: parity with the numpy statement under the invariant --------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize("w,h,k", ts.SHAPES)
def test_parity_under_the_invariant(w, h, k, layout):
    """The held thumbnails are within the threshold of the thumbnails before the tick, the tick changes bytes of the selected
    tiles only: the output is unique and the host form's."""
    rng = np.random.default_rng(31 * w + k)
    n, nt = 3 * w * h, ts.thumb_bytes(w, h, k)
    prev = ts.random_states(rng, S, w, h)
    before = np.stack([ws.thumbnail(prev[s], w, h, k).reshape(-1) for s in range(S)])
    with CUDACore(w, h, max_batch=S) as core:
        for thr in (0, 20):
            held = np.clip(before.astype(int) + rng.integers(-thr, thr + 1, before.shape), 0, 255).astype(np.uint8)
            for sel in selections(rng, n):
                states = prev if sel is None else tick(rng, prev, sel)
                # (a NULL mask requires every pixel: no invariant to keep, any held thumbnail will do)
                h0 = rng.integers(0, 256, before.shape, dtype=np.uint8) if sel is None else held
                st, th = regions(layout, n, nt, states, h0)
                got = run(core, w, h, k, thr, st, th, sel)
                assert_equals_spec(got, ts.batch(states, h0, w, h, k, thr, sel), f"threshold {thr}")
                assert np.array_equal(st.get(), states)


def test_crafted_states_at_the_top_of_the_sums():
    """64x48, k = 16: every byte 255 (column sums 16 * 255, block sums 256 * 255) and the rounding tie (every block sums to a / 2)."""
    w, h, k = 64, 48, 16
    n, nt = 3 * w * h, ts.thumb_bytes(w, h, k)
    states = np.stack([np.full(n, 255, np.uint8), ts.tie_state(w, h, k), np.full(n, 1, np.uint8)])
    held = np.zeros((S, nt), np.uint8)
    with CUDACore(w, h, max_batch=S) as core:
        for layout in LAYOUTS:
            st, th = regions(layout, n, nt, states, held)
            got = run(core, w, h, k, 0, st, th, None)
            assert_equals_spec(got, ts.batch(states, held, w, h, k, 0))
            assert (got[3][0] == 255).all() and (got[3][1] == 1).all() and (got[3][2] == 1).all()


@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_record_mechanics(layout):
    """100x60, k = 2: an escape behind a gap >= 255 with pad bytes, a first entry at j >= 255, a difference that wraps, the
    8-byte record (thumb_spec.mechanics_ticks)."""
    w, h, k = 100, 60, 2
    n, nt = 3 * w * h, ts.thumb_bytes(w, h, k)
    ticks = ts.mechanics_ticks(np.random.default_rng(3))
    with CUDACore(w, h, max_batch=S) as core:
        for group in (ticks[:3], ticks[1:]):
            a, b = np.stack([t[1] for t in group]), np.stack([t[2] for t in group])
            held = np.stack([ws.thumbnail(x, w, h, k).reshape(-1) for x in a])
            sel = np.stack([ts.touched_sel(x, y) for x, y in zip(a, b)])
            st, th = regions(layout, n, nt, b, held)
            got = run(core, w, h, k, 0, st, th, sel)
            assert_equals_spec(got, ts.batch(b, held, w, h, k, 0, sel))
            assert np.array_equal(got[3], np.stack([ws.thumbnail(x, w, h, k).reshape(-1) for x in b]))


# ---- 2. laws 1 and 2 without the invariant --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize("w,h,k", ts.SHAPES)
def test_laws_1_and_2_with_random_held_thumbnails(w, h, k, layout):
    """Held thumbnails that have nothing to do with the states, a mask of a few tiles; the processed set is taken as whatever
    changed or is required, and the record must be the numpy statement's for that set."""
    rng = np.random.default_rng(17 * w + k)
    n, nt = 3 * w * h, ts.thumb_bytes(w, h, k)
    states, held = ts.random_states(rng, S, w, h), rng.integers(0, 256, (S, nt), dtype=np.uint8)
    sel = rng.random((S, ws.tiles(n))) < 0.4
    sel[0, 0] = True
    with CUDACore(w, h, max_batch=S) as core:
        for thr in (0, 20):
            st, th = regions(layout, n, nt, states, held)
            off, pos, out, after = run(core, w, h, k, thr, st, th, sel)
            processed = np.stack([ts.required_bytes(sel[s], w, h, k) for s in range(S)]) | (after != held)
            assert_equals_spec((off, pos, out, after), ts.batch(states, held, w, h, k, thr, sel, processed))
            for s in range(S):
                rec = out[int(pos[s]):int(pos[s + 1])].tobytes()
                assert np.array_equal(ts.apply(held[s], rec), after[s])                        # law 1
                ts.check_law2(states[s], held[s], after[s], w, h, k, thr, sel[s])               # law 2


# ---- 3. law 3's route: the wall into a second core of the thumbnail's geometry ---------------------------------------------
@pytest.mark.parametrize("w,h,k", [(37, 11, 4), (100, 60, 2), (100, 60, 3), (2800, 6, 2)])
def test_equals_the_wall_and_a_diff_on_a_thumbnail_core(w, h, k):
    rng = np.random.default_rng(5 * w + k)
    n, nt = 3 * w * h, ts.thumb_bytes(w, h, k)
    tw, thh = ws.thumb_size(w, h, k)
    states, held = ts.random_states(rng, S, w, h), rng.integers(0, 256, (S, nt), dtype=np.uint8)
    places = np.array([[0, s * thh, k] for s in range(S)], np.int32)
    for thr in (0, 20):
        st, th = regions(("packed", 0, None, 0, 0), n, nt, states, held)
        route_states = Region(S, nt).put(held)
        wall = Region(S, nt)
        o = Out(S, cwire_bytes_max(nt, S))
        with CUDACore(w, h, max_batch=S) as core, CUDACore(tw, thh, threshold=thr, max_batch=S) as small:
            got = run(core, w, h, k, thr, st, th, None)
            core.wall_compose_batch(st.ptr, S, places, wall.ptr, tw, S * thh, stride=st.stride)
            core.synchronize()
            small.diff_multi_cwire_batch(wall.ptr, route_states.ptr, S, o.off.ptr, o.pos.ptr, o.out.ptr, o.cap, stride=nt)
            small.synchronize()
        roff, rpos, rout = o.results()
        assert np.array_equal(got[0], roff) and np.array_equal(got[1], rpos)
        end = int(rpos[-1])
        assert np.array_equal(got[2][:end], rout[:end]) and np.array_equal(got[3], route_states.get())


# ---- 4. law 4: the chain, one synchronise at the end -----------------------------------------------------------------------
TICKS = 6


def chain_inputs(rng, w, h):
    """states[t]: uint8[S, N] after tick t (states[0]: the start), a moving change of a few hundred bytes per stream and tick;
    stream 2 stands still on odd ticks."""
    n = 3 * w * h
    states = [ts.random_states(rng, S, w, h)]
    for t in range(1, TICKS + 1):
        nxt = states[-1].copy()
        for s in range(S):
            if s == 2 and t % 2:
                continue
            xs = (rng.integers(0, n) + np.arange(0, 3 * rng.integers(1, 200))) % n
            nxt[s, xs] += rng.integers(1, 256, xs.size, dtype=np.uint8)
        states.append(nxt)
    return states


def records_between(a, b):
    """The compact record that takes state a to state b (threshold 0), with its header."""
    xs = np.flatnonzero(a != b)
    rec = spec.encode_frame(xs.astype(np.int32), (b[xs] - a[xs]).astype(np.uint8))
    return rec, xs.size, int(np.frombuffer(rec[4:8], "<u4")[0])


def check_chain(outs, k, w, h, first, final_states, thumbs_after):
    """The viewers apply every record of the chain to the thumbnails they began with: they, the held thumbnails and the
    thumbnails of the final states are one."""
    want = np.stack([ws.thumbnail(final_states[s], w, h, k).reshape(-1) for s in range(S)])
    assert np.array_equal(thumbs_after, want)
    viewers = first.copy()
    for o in outs:
        off, pos, out = o.results()
        for s in range(S):
            v = viewers[s].copy()
            assert cwire_apply_host(v, out[int(pos[s]):int(pos[s + 1])], 1) == int(pos[s + 1] - pos[s])
            viewers[s] = v
    assert np.array_equal(viewers, want)


@pytest.mark.parametrize("w,h,k", [(100, 60, 2), (100, 60, 3), (2800, 6, 2)])
def test_chain_on_a_sender(w, h, k):
    """diff_multi_cwire_batch (threshold 0), touched tiles of its records, this call: six ticks enqueued back to back.  The
    headers the touched-tiles call needs come from numpy -- nothing is read back inside the chain."""
    rng = np.random.default_rng(w + k)
    n, nt, mw = 3 * w * h, ts.thumb_bytes(w, h, k), ws.mask_words(3 * w * h)
    states = chain_inputs(rng, w, h)
    first = np.stack([ws.thumbnail(states[0][s], w, h, k).reshape(-1) for s in range(S)])
    st, th = regions(LAYOUTS[0], n, nt, states[0], first)
    frames = [Region(S, n, st.stride).put(states[t]) for t in range(1, TICKS + 1)]
    tick_out = [Out(S, cwire_bytes_max(n, S)) for _ in range(TICKS)]
    outs = [Out(S, cwire_bytes_max(nt, S)) for _ in range(TICKS)]
    mask = Guarded(S * mw, torch.int32)
    with CUDACore(w, h, threshold=0, max_batch=S) as core:
        torch.cuda.synchronize()
        for t in range(TICKS):
            hdr = [records_between(states[t][s], states[t + 1][s]) for s in range(S)]
            core.diff_multi_cwire_batch(frames[t].ptr, st.ptr, S, tick_out[t].off.ptr, tick_out[t].pos.ptr, tick_out[t].out.ptr,
                                        tick_out[t].cap, stride=st.stride)
            core.cwire_touched_tiles_batch(tick_out[t].out.ptr, [x[1] for x in hdr], [x[2] for x in hdr], S, 1, mask.ptr)
            thumb_call(core, k, 0, st, th, mask, outs[t])
        core.synchronize()
    assert np.array_equal(st.get(), states[-1])
    check_chain(outs, k, w, h, first, states[-1], th.get())


@pytest.mark.parametrize("w,h,k", [(100, 60, 2), (37, 11, 4), (2800, 6, 2)])
def test_chain_on_a_relay(w, h, k):
    """apply_multi_stream_cwire_batch of bursts of T = 2 records, touched tiles of the burst ORed onto the mask, this call behind
    every second burst with the mask of both (then the mask starts again)."""
    rng = np.random.default_rng(w + 7 * k)
    T = 2
    n, nt, mw = 3 * w * h, ts.thumb_bytes(w, h, k), ws.mask_words(3 * w * h)
    states = chain_inputs(rng, w, h)
    first = np.stack([ws.thumbnail(states[0][s], w, h, k).reshape(-1) for s in range(S)])
    st, th = regions(LAYOUTS[1], n, nt, states[0], first)
    bursts = []
    for b in range(TICKS // T):
        recs = [records_between(states[T * b + t][s], states[T * b + t + 1][s]) for s in range(S) for t in range(T)]
        buf = np.frombuffer(b"".join(r[0] for r in recs), np.uint8).copy()
        bursts.append((Guarded(buf.size, data=buf), [r[1] for r in recs], [r[2] for r in recs]))
    outs = [Out(S, cwire_bytes_max(nt, S)) for _ in range(2)]
    mask = Guarded(S * mw, torch.int32)
    with CUDACore(w, h, max_batch=S * T) as core:
        torch.cuda.synchronize()
        for b, (d_recs, counts, escapes) in enumerate(bursts):
            core.apply_multi_stream_cwire_batch(d_recs.ptr, counts, escapes, S, T, st.ptr, stride=st.stride)
            core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, T, mask.ptr, accumulate=b == 1)
            if b != 0:
                thumb_call(core, k, 0, st, th, mask, outs[b - 1])
        core.synchronize()
    assert np.array_equal(st.get(), states[-1])
    check_chain(outs, k, w, h, first, states[-1], th.get())


# ---- 5. laws 5 and 6 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,k", ts.SHAPES)
def test_key_record(w, h, k):
    rng = np.random.default_rng(3 * w + k)
    n, nt = 3 * w * h, ts.thumb_bytes(w, h, k)
    states = ts.random_states(rng, S, w, h)
    states[rng.random(states.shape) < 0.6] = 0
    with CUDACore(w, h, max_batch=S) as core:
        st, th = regions(LAYOUTS[1], n, nt, states, np.zeros((S, nt), np.uint8))
        off, pos, out, after = run(core, w, h, k, 0, st, th, None)
    for s in range(S):
        t = ws.thumbnail(states[s], w, h, k).reshape(-1)
        xs = np.flatnonzero(t)
        assert out[int(pos[s]):int(pos[s + 1])].tobytes() == spec.encode_frame(xs.astype(np.int32), t[xs])
        assert np.array_equal(after[s], t)


@pytest.mark.parametrize("w,h", [(37, 11), (100, 60)])
def test_scale_one_equals_the_refresh_call(w, h):
    rng = np.random.default_rng(w)
    n = 3 * w * h
    states = ts.random_states(rng, S, w, h)
    states[rng.random(states.shape) < 0.7] = 0
    st, th = regions(LAYOUTS[0], n, n, states, np.zeros((S, n), np.uint8))
    ref, rmask = Out(S, cwire_bytes_max(n, S)), Guarded(S * ws.mask_words(n), torch.int32)
    with CUDACore(w, h, max_batch=S) as core:
        off, pos, out, after = run(core, w, h, 1, 0, st, th, None)
        core.refresh_cwire_batch(st.ptr, S, None, rmask.ptr, ref.off.ptr, ref.pos.ptr, ref.out.ptr, ref.cap, stride=st.stride)
        core.synchronize()
    roff, rpos, rout = ref.results()
    assert np.array_equal(off, roff) and np.array_equal(pos, rpos) and np.array_equal(out, rout)
    assert np.array_equal(after, states)


# ---- 6. capacity ----------------------------------------------------------------------------------------------------------
def test_a_record_that_does_not_fit_leaves_its_thumbnail_alone():
    """Frame positions are running sums, as the refresh call's: once record s ends past the capacity so does every later one.
    Room for stream 0 alone, for streams 0 and 1, for none: the records that fit are written and their thumbnails move, the
    others' records are absent and their thumbnails untouched, offsets and frame positions exact; a repeat with the same mask
    and full capacity then delivers the rest."""
    w, h, k = 100, 60, 2
    rng = np.random.default_rng(1)
    n, nt = 3 * w * h, ts.thumb_bytes(w, h, k)
    states, held = ts.random_states(rng, S, w, h), rng.integers(0, 256, (S, nt), dtype=np.uint8)
    sel = np.ones((S, ws.tiles(n)), bool)
    _, full_pos, _, _ = ts.batch(states, held, w, h, k, 0, sel)
    with CUDACore(w, h, max_batch=S) as core:
        for layout in LAYOUTS:
            for cap in (int(full_pos[1]), int(full_pos[2]) - 4, int(full_pos[2]), int(full_pos[3]) - 4, int(full_pos[1]) - 4, 0):
                st, th = regions(layout, n, nt, states, held)
                want = ts.batch(states, held, w, h, k, 0, sel, capacity=cap)
                got = run(core, w, h, k, 0, st, th, sel, cap=cap)
                assert_equals_spec(got, want, f"capacity {cap}")
                again = run(core, w, h, k, 0, st, th, sel)                                   # the same mask, room for all
                assert_equals_spec(again, ts.batch(states, want[3], w, h, k, 0, sel), f"after capacity {cap}")
                for s in range(S):
                    assert (int(again[0][s + 1]) - int(again[0][s]) == 0) == (want[2][s] is not None)


# ---- 7. refusals and the empty batch --------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, k = 64, 48, 2
    n, nt = 3 * w * h, ts.thumb_bytes(w, h, k)
    mw = ws.mask_words(n)
    L = lib.load()
    arena = torch.full((8 * 16384,), 0xA5, dtype=torch.uint8, device=DEV)
    at = (lambda slot: arena.data_ptr() + slot * 16384)
    cap = cwire_bytes_max(nt, S)
    assert S * aligned(n) <= 2 * 16384 and cap <= 16384 and arena.data_ptr() % 256 == 0
    with CUDACore(w, h, max_batch=S) as core:
        good = dict(core=core._h, states=at(0), stride=n, S=S, k=k, thr=0, mask=at(2), thumbs=at(3), tstride=nt, off=at(4), pos=at(5),
                    out=at(6), cap=cap)
        thumbs_end = at(3) + (S - 1) * nt + nt
        bad = [(dict(core=None), "null core"), (dict(S=-1), "nstreams"), (dict(S=S + 1), "nstreams"), (dict(k=0), "k outside"),
               (dict(k=17), "k outside"), (dict(thr=-1), "threshold"), (dict(thr=256), "threshold"),
               (dict(states=None), "null"), (dict(thumbs=None), "null"), (dict(off=None), "null"), (dict(pos=None), "null"),
               (dict(out=None), "null"), (dict(stride=n - 1), "state_spacing_bytes"), (dict(tstride=nt - 1), "thumb_spacing_bytes"),
               (dict(mask=at(2) + 2), "4-byte"), (dict(off=at(4) + 2), "4-byte"), (dict(out=at(6) + 1), "4-byte"),
               (dict(pos=at(5) + 4), "8-byte"),
               # any two regions overlapping, the last byte of one on the first of the other
               (dict(thumbs=at(0) + (S - 1) * n + n - 1), "overlap"), (dict(mask=at(0) + (S - 1) * n + n - 4), "overlap"),
               (dict(off=at(0)), "overlap"), (dict(pos=at(0) + 8), "overlap"), (dict(out=at(0) + 16), "overlap"),
               (dict(mask=(thumbs_end - 1) & ~3), "overlap"), (dict(off=(thumbs_end - 1) & ~3), "overlap"),
               (dict(pos=at(3)), "overlap"), (dict(out=at(3) + 4), "overlap"),
               (dict(off=at(2) + 4 * S * mw - 4), "overlap"), (dict(pos=at(2)), "overlap"), (dict(out=at(2)), "overlap"),
               (dict(pos=at(4) + 8), "overlap"), (dict(out=at(4) + 4 * S), "overlap"), (dict(out=at(5) + 8 * S), "overlap")]
        torch.cuda.synchronize()
        for change, text in bad:
            a = dict(good, **change)
            rc = L.mi355_thumb_cwire_batch(a["core"], a["states"], a["stride"], a["S"], a["k"], a["thr"], a["mask"], a["thumbs"],
                                           a["tstride"], a["off"], a["pos"], a["out"], a["cap"])
            assert rc == lib.ERR_INVALID, change
            assert text in L.mi355_last_error().decode(), (change, L.mi355_last_error())
        core.synchronize()
        assert bool((arena == 0xA5).all()), "a refused call wrote something"
        a = good   # ... and the valid call is taken
        assert L.mi355_thumb_cwire_batch(a["core"], a["states"], a["stride"], S, k, 0, None, a["thumbs"], a["tstride"], a["off"],
                                         a["pos"], a["out"], a["cap"]) == lib.OK
        core.synchronize()


def test_an_empty_batch_writes_the_two_heads():
    w, h, k = 37, 11, 2
    off, pos, out = Guarded(2, torch.int32), Guarded(2, torch.int64), Guarded(64)
    L = lib.load()
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        assert L.mi355_thumb_cwire_batch(core._h, None, 0, 0, k, 0, None, None, 0, off.ptr, pos.ptr, out.ptr, 64) == lib.OK
        core.synchronize()
    assert off.get(written=1)[0] == 0 and pos.get(written=1)[0] == 0
    out.get(written=0)

"""-m gpu: mi355_wall_compose_batch and mi355_cwire_touched_tiles_batch (include/mi355diff.h, "A wall of many cameras").  The
reference of every comparison is numpy: wall_spec (the block average, the required pixels, the touched tiles) and cwire_spec (the
records), never the code under test.  States, records, masks and the wall live in guarded buffers (gpu_util) that start as a
non-zero pattern; the wall is a Region of wall_h rows of 3*wall_w bytes, one byte behind an aligned address, pitch 3*wall_w + 5.

Shapes, the smallest at which each seam exists: 7x5 (one ragged tile, every k above 5 gives one pixel), 33x7 (N = 693, odd: a
row pitch of 99 bytes, so nearly every row takes the byte loads), 64x48 (N = 9216: byte 4096 falls inside pixel 1365; rows of 192
bytes take the 16-byte loads), 256x171 (N = 131328: 33 tiles, the mask's second word holds one bit), 1500x2 (two column chunks
per thumbnail row at k = 1, 2 and 3), 33x7 with S = 1025 (more placements than one launch carries)."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
import wall_spec as ws
from cudavideostream_amd import cwire_bytes_max, lib
from gpu_util import GUARD, CUDACore, Guarded, Region

pytestmark = pytest.mark.gpu

SHAPES = [(7, 5), (33, 7), (64, 48), (256, 171), (1500, 2)]
# (skew of the base, stride - N): every stream 16-byte aligned where N allows; stride == N on a skewed base; an odd stride
LAYOUTS = [(0, None), (5, 0), (0, 3)]
KS = [1, 2, 3, 5, 16]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_states(w, h, S, seed=0):
    st = np.random.default_rng(1000 * w + h + S + seed).integers(0, 256, (S, 3 * w * h), dtype=np.uint8)
    st.setflags(write=False)
    return st


def aligned_stride(n, extra):
    return (n + 15) // 16 * 16 if extra is None else n + extra


def row_layout(w, h, ks):
    """The streams' thumbnails left to right, three pixels apart, each one row lower than the one before; a hidden stream
    (k == 0) keeps the place it would have.  -> (int32[S, 3], wall_w, wall_h)."""
    x, places, bottom = 2, [], 1
    for i, k in enumerate(ks):
        places.append((x, 1 + i, k))
        if k:
            tw, th = ws.thumb_size(w, h, k)
            x += tw + 3
            bottom = max(bottom, 1 + i + th)
    return np.array(places, np.int32), x + 1, bottom + 2


class Wall:
    """A guarded wall: every byte starts as the pattern, or as `init` (uint8[wall_h, wall_w, 3]) inside the wall's pixels."""

    def __init__(self, wall_w, wall_h, init=None):
        self.w, self.h = wall_w, wall_h
        self.reg = Region(wall_h, 3 * wall_w, 3 * wall_w + 5, 1)
        if init is not None:
            self.reg.put(np.ascontiguousarray(init).reshape(wall_h, 3 * wall_w))
        self.ptr, self.pitch = self.reg.ptr, self.reg.stride

    def get(self):
        """uint8[wall_h, wall_w, 3]; the pitch gaps and the guards around the wall asserted."""
        return self.reg.get().reshape(self.h, self.w, 3)


def pattern(wall_w, wall_h):
    return np.full((wall_h, wall_w, 3), GUARD, np.uint8)


def compose(core, states, S, places, wall, mask=None):
    core.wall_compose_batch(states.ptr, S, places, wall.ptr, wall.w, wall.h, wall_pitch=wall.pitch,
                            d_tile_mask=None if mask is None else mask.ptr, stride=states.stride)


def mask_buffer(rows):
    """uint32[S, mask_words] -> a guarded device copy."""
    rows = np.ascontiguousarray(rows, np.uint32)
    return Guarded(rows.size, torch.int32, data=rows.view(np.int32).ravel())


def make_records(n, S, T, entries, seed=3):
    """entries(s, t) -> ascending indices of record b = s*T + t.  -> (records uint8, counts, escapes, delta uint8[S, n]: the sum of
    the streams' differences mod 256, xs per record)."""
    rng = np.random.default_rng(seed)
    off, xs_all, df_all, lists = [0], [], [], []
    delta = np.zeros((S, n), np.uint8)
    for s in range(S):
        for t in range(T):
            xs = np.asarray(entries(s, t), np.int64)
            assert (np.diff(xs) > 0).all() and (xs.size == 0 or (0 <= xs[0] and xs[-1] < n))
            df = rng.integers(1, 256, xs.size, dtype=np.uint8)
            delta[s, xs] += df
            xs_all.append(xs.astype(np.int32)); df_all.append(df); lists.append(xs)
            off.append(off[-1] + xs.size)
    cat = (lambda a, dt: np.concatenate(a + [np.empty(0, dt)]).astype(dt))
    recs, _ = spec.encode(np.array(off, np.uint32), cat(xs_all, np.int32), cat(df_all, np.uint8))
    counts, escapes = spec.headers(recs, S * T)
    return recs, counts, escapes, delta, lists


# ---- 1. the full compose --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skew,extra", LAYOUTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_full_compose_equals_numpy(w, h, skew, extra):
    """Three streams with different k, one of them hidden, for every k of KS: the rectangles hold the numpy thumbnails; the pitch
    gap, the wall outside the rectangles and the hidden stream's would-be area still hold the pattern."""
    S, n = 3, 3 * w * h
    src = random_states(w, h, S)
    states = Region(S, n, aligned_stride(n, extra), skew).put(src)
    with CUDACore(w, h, max_batch=S) as core:
        for i, k in enumerate(KS):
            places, wall_w, wall_h = row_layout(w, h, [k, 0, KS[(i + 2) % len(KS)]])
            wall = Wall(wall_w, wall_h)
            torch.cuda.synchronize()
            compose(core, states, S, places, wall)
            core.synchronize()
            want = ws.compose(pattern(wall_w, wall_h), src, w, h, places)
            assert np.array_equal(wall.get(), want), f"k = {k}"
    assert np.array_equal(states.get(), src)             # guards and stride gaps intact, the states only read


def test_rounding_on_crafted_states():
    """7x5: k = 2 has blocks of 4, 2 and 1 pixels, k = 3 blocks of 9, 3, 6 and 2.  Stream 0: block sums exactly at a half and
    next to it; stream 1: every byte 255; stream 2: every byte 1 (a mean of 1 whatever the area)."""
    w, h, S = 7, 5, 3
    n = 3 * w * h
    img = np.zeros((S, h, w, 3), np.uint8)
    img[0, 0, 0, 0] = 1                                  # k = 2, area 4: sum 1 -> 0
    img[0, 0, 2, 0] = 2                                  #                sum 2 -> 1 (exactly a half rounds up)
    img[0, 1, 4, 0] = 3                                  #                sum 3 -> 1
    img[0, 0, 6, 1] = 1                                  # k = 2, right edge, area 2: sum 1 -> 1; k = 3, area 3: sum 1 -> 0
    img[0, 4, 0, 1] = 1                                  # k = 2, bottom edge, area 2: sum 1 -> 1; k = 3, area 6: sum 1 -> 0
    img[0, 4, 6, 2] = 77                                 # k = 2, the corner, area 1: itself; k = 3, area 2: 77 -> 39
    img[0, 3, 3, 2] = 3                                  # k = 3, bottom band, area 6: sum 3 -> 1 (a half)
    img[0, 2, 6, 2] = 2                                  # k = 3, right edge, area 3: sum 2 -> 1
    img[1], img[2] = 255, 1
    src = img.reshape(S, n)
    states = Region(S, n, n, 3).put(src)
    with CUDACore(w, h, max_batch=S) as core:
        for k in (2, 3):
            places, wall_w, wall_h = row_layout(w, h, [k] * S)
            wall = Wall(wall_w, wall_h)
            torch.cuda.synchronize()
            compose(core, states, S, places, wall)
            core.synchronize()
            got = wall.get()
            assert np.array_equal(got, ws.compose(pattern(wall_w, wall_h), src, w, h, places))
            x0, y0 = int(places[0][0]), int(places[0][1])
            t0 = got[y0:, x0:]
            if k == 2:
                assert [t0[0, 0, 0], t0[0, 1, 0], t0[0, 2, 0], t0[0, 3, 1], t0[2, 0, 1], t0[2, 3, 2]] == [0, 1, 1, 1, 1, 77]
            else:
                assert [t0[0, 2, 1], t0[1, 0, 1], t0[1, 2, 2], t0[1, 1, 2], t0[0, 2, 2]] == [0, 0, 39, 1, 1]
            for s, v in ((1, 255), (2, 1)):
                x, y, tw, th = ws.rect(w, h, places[s])
                assert (got[y:y + th, x:x + tw] == v).all()


# ---- 2. touched tiles -----------------------------------------------------------------------------------------------------
def touched_entries(n, T):
    """Stream 0: byte 4095, byte 4096 and the last byte in separate records (T == 1: in the one), empty records between them; stream 1: random
    entries, every third record empty; stream 2: empty records only."""
    rng = np.random.default_rng(n + T)

    def entries(s, t):
        if s == 0:
            marks = [[min(4095, n - 1)], [min(4096, n - 1)], [n - 1]]
            if T == 1:
                return np.unique(marks)
            return marks[t // 2 % 3] if t % 2 == 0 else []
        if s == 1:
            return [] if t % 3 == 2 else np.unique(rng.integers(0, n, 1 + t % 7))
        return []
    return entries


@pytest.mark.parametrize("T", [1, 65])
@pytest.mark.parametrize("w,h", [(33, 7), (64, 48), (256, 171)])
def test_touched_tiles_equal_unique_of_the_entries(w, h, T):
    """Overwriting a pattern mask, then ORing onto a start mask; the row behind the last stream keeps its pattern."""
    S, n = 3, 3 * w * h
    t, mw = ws.tiles(n), ws.mask_words(n)
    recs, counts, escapes, _, lists = make_records(n, S, T, touched_entries(n, T))
    want = np.stack([ws.touched(n, lists[s * T:(s + 1) * T]) for s in range(S)])
    assert want[0].any() and want[1].any() and not want[2].any()
    if n == 131328:
        assert want[0, 32] and ws.mask_of(want)[0, 1] == 1           # the second mask word holds one bit
    d_recs = Guarded(recs.size, data=recs)
    mask = Guarded((S + 1) * mw, torch.int32)                        # (the pattern: -7, nearly every bit set)
    start = np.zeros((S + 1, mw), np.uint32)
    start[:, 0] = 0b100                                              # tile 2 where it exists: a bit past `tiles` otherwise
    acc = mask_buffer(start)
    with CUDACore(w, h, max_batch=S * T) as core:
        torch.cuda.synchronize()
        core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, T, mask.ptr)
        core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, T, acc.ptr, accumulate=True)
        core.synchronize()
    got = mask.get(written=S * mw).view(np.uint32)[:S * mw].reshape(S, mw)
    assert np.array_equal(got, ws.mask_of(want))
    got_acc = acc.get().view(np.uint32).reshape(S + 1, mw)
    assert np.array_equal(got_acc[:S], ws.mask_of(want) | start[:S])
    assert np.array_equal(got_acc[S], start[S])
    assert np.array_equal(d_recs.get(), recs)
    assert t == want.shape[1]


def test_touched_tiles_or_onto_a_refresh_mask():
    """The mask of mi355_refresh_cwire_batch (one damaged tile) and a tick's touched tiles are one object."""
    w, h, S = 64, 48, 2
    n = 3 * w * h
    mw = ws.mask_words(n)
    sender = random_states(w, h, S)
    recv = sender.copy()
    recv[0, 4096 + 9] ^= 0x21                                        # stream 0, tile 1
    recs, counts, escapes, _, lists = make_records(n, S, 1, lambda s, t: [5, 8200] if s == 0 else [4100])
    snd, rcv, d_recs = Region(S, n).put(sender), Region(S, n).put(recv), Guarded(recs.size, data=recs)
    cap = cwire_bytes_max(n, S)
    dig, mask = Guarded(2 * S * ws.tiles(n), torch.int32), Guarded(S * mw, torch.int32)
    off, pos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        core.state_digest_batch(rcv.ptr, S, dig.ptr)
        core.refresh_cwire_batch(snd.ptr, S, dig.ptr, mask.ptr, off.ptr, pos.ptr, out.ptr, cap)
        core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, 1, mask.ptr, accumulate=True)
        core.synchronize()
    assert np.array_equal(mask.get().view(np.uint32).reshape(S, mw), np.array([[0b111], [0b010]], np.uint32))


# ---- 3. the tying property ------------------------------------------------------------------------------------------------
def test_apply_touched_and_masked_compose_keep_the_wall_current():
    """The wall starts as the numpy composition of the old states; apply, touched tiles and the masked compose, with no
    synchronisation between the three, make it the numpy composition of the new states -- and what the synchronised run gives.
    Then the same over a resync: refresh, clear, apply and the masked compose with the refresh's own mask.  Stream 3 is a still
    camera; 256x171 at k = 2, 3, 1, 5 (33 tiles)."""
    w, h, S, T = 256, 171, 4, 3
    n = 3 * w * h
    ks = [2, 3, 1, 5]
    places, wall_w, wall_h = row_layout(w, h, ks)
    old = random_states(w, h, S, seed=9)
    rng = np.random.default_rng(11)

    def entries(s, t):
        if s == 3:
            return []
        if s == 0:                                                   # a block of 12 rows moving down, 40 pixels wide
            rows = np.arange(20 + 30 * t, 32 + 30 * t)
            return np.sort((3 * (rows[:, None] * w + 100) + np.arange(120)[None, :]).ravel())
        return np.unique(np.concatenate([rng.integers(0, n, 300), [4095, 4096, n - 1]]))

    recs, counts, escapes, delta, _ = make_records(n, S, T, entries)
    new = old + delta
    want_old = ws.compose(pattern(wall_w, wall_h), old, w, h, places)
    want_new = ws.compose(pattern(wall_w, wall_h), new, w, h, places)
    assert not np.array_equal(want_old, want_new)
    mw = ws.mask_words(n)
    # the resync: the receiver's states differ from the sender's (`new`) in a few tiles
    damaged = new.copy()
    for s, tile in [(0, 0), (0, 32), (1, 7), (3, 31)]:
        damaged[s, tile * ws.TILE + 5] ^= 0x3C
    want_damaged = ws.compose(pattern(wall_w, wall_h), damaged, w, h, places)
    cap = cwire_bytes_max(n, S)
    results = []
    r_counts = r_escapes = None
    with CUDACore(w, h, max_batch=S * T) as core:
        for sync in (True, False):
            step = core.synchronize if sync else (lambda: None)
            states, d_recs, mask = Region(S, n).put(old), Guarded(recs.size, data=recs), Guarded(S * mw, torch.int32)
            wall = Wall(wall_w, wall_h, want_old)
            snd, rcv, wall2 = Region(S, n).put(new), Region(S, n).put(damaged), Wall(wall_w, wall_h, want_damaged)
            dig, rmask = Guarded(2 * S * ws.tiles(n), torch.int32), Guarded(S * mw, torch.int32)
            off, pos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
            torch.cuda.synchronize()
            core.apply_multi_stream_cwire_batch(d_recs.ptr, counts, escapes, S, T, states.ptr)
            step()
            core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, T, mask.ptr)
            step()
            compose(core, states, S, places, wall, mask)
            step()
            core.state_digest_batch(rcv.ptr, S, dig.ptr)
            step()
            core.refresh_cwire_batch(snd.ptr, S, dig.ptr, rmask.ptr, off.ptr, pos.ptr, out.ptr, cap)
            step()
            if sync:                                                 # the headers of the refresh records, for both runs
                r_counts, r_escapes = spec.headers(out.get()[:int(pos.get().view(np.uint64)[S])], S)
            core.state_clear_tiles_batch(rcv.ptr, S, rmask.ptr)
            step()
            core.apply_multi_cwire_batch(out.ptr, r_counts, r_escapes, S, rcv.ptr)
            step()
            compose(core, rcv, S, places, wall2, rmask)
            core.synchronize()
            results.append((states.get(), wall.get(), mask.get(), rcv.get(), wall2.get(), rmask.get()))
            assert np.array_equal(d_recs.get(), recs) and np.array_equal(snd.get(), new)
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    got_states, got_wall, got_mask, got_rcv, got_wall2, got_rmask = results[1]
    assert np.array_equal(got_states, new)
    assert np.array_equal(got_wall, want_new)
    assert not got_mask.view(np.uint32).reshape(S, mw)[3].any()      # the still camera: no tile, nothing repainted
    assert np.array_equal(got_rcv, new)
    assert np.array_equal(got_wall2, want_new)
    assert np.array_equal(got_rmask.view(np.uint32).reshape(S, mw),
                          np.array([[1, 1], [1 << 7, 0], [0, 0], [1 << 31, 0]], np.uint32))


# ---- 4. the masked compose on a pattern wall ------------------------------------------------------------------------------
@pytest.mark.parametrize("sel_tiles", [(0,), (1,), (0, 2)], ids=str)
def test_masked_compose_writes_the_required_pixels(sel_tiles):
    """64x48, stream 0 with the tiles of `sel_tiles`, stream 1 with an empty mask row but for bits past `tiles`: every required
    pixel of stream 0 is correct (with only tile 0 that includes the block of pixel 1365, whose bytes 4095 .. 4097 straddle the
    edge), every other pixel of its rectangle is the pattern or correct, stream 1 and everything else is pattern."""
    w, h, S = 64, 48, 2
    n = 3 * w * h
    src = random_states(w, h, S)
    src = np.where(src == GUARD, np.uint8(GUARD + 1), src)
    states = Region(S, n, n + 3, 5).put(src)
    sel = np.zeros(ws.tiles(n), bool)
    sel[list(sel_tiles)] = True
    rows = np.array([[sum(1 << t for t in sel_tiles)], [0xFFFFFFF8]], np.uint32)
    assert not ws.selected_of(rows[1], n).any() and np.array_equal(ws.selected_of(rows[0], n), sel)
    mask = mask_buffer(rows)
    with CUDACore(w, h, max_batch=S) as core:
        for k in (1, 2, 3, 5, 16):
            places, wall_w, wall_h = row_layout(w, h, [k, k])
            wall = Wall(wall_w, wall_h)
            torch.cuda.synchronize()
            compose(core, states, S, places, wall, mask)
            core.synchronize()
            got = wall.get()
            full = ws.compose(pattern(wall_w, wall_h), src, w, h, places)
            x, y, tw, th = ws.rect(w, h, places[0])
            req = ws.required(sel, w, h, k)
            assert req.shape == (th, tw) and req.any()
            if sel_tiles == (0,):
                assert req[(1365 // w) // k, (1365 % w) // k]
            inside = np.zeros((wall_h, wall_w), bool)
            inside[y:y + th, x:x + tw] = True
            needed = np.zeros((wall_h, wall_w), bool)
            needed[y:y + th, x:x + tw] = req
            assert np.array_equal(got[needed], full[needed]), f"k = {k}: a required pixel is wrong"
            ok = (got == full) | (got == GUARD)
            assert ok[inside].all(), f"k = {k}: a pixel of the rectangle is neither the pattern nor its value"
            assert (got[~inside] == GUARD).all(), f"k = {k}: written outside stream 0's rectangle"
    assert np.array_equal(mask.get().view(np.uint32).reshape(S, 1), rows)
    assert np.array_equal(states.get(), src)


# ---- 5. many streams ------------------------------------------------------------------------------------------------------
def test_many_streams():
    """S = 1025 at 33x7, k = 3, on a grid of 33 columns: nine launches' worth of placements.  Full, then masked on a pattern wall
    with four streams selected: only their rectangles are written."""
    w, h, S, k = 33, 7, 1025, 3
    n = 3 * w * h
    tw, th = ws.thumb_size(w, h, k)
    cols = 33
    places = np.array([((s % cols) * tw, (s // cols) * th, k) for s in range(S)], np.int32)
    wall_w, wall_h = cols * tw, ((S + cols - 1) // cols) * th
    src = random_states(w, h, S)
    states = Region(S, n, n, 1).put(src)
    chosen = [0, 127, 128, 1024]
    rows = np.zeros((S, 1), np.uint32)
    rows[chosen] = 1
    mask = mask_buffer(rows)
    wall, wall_m = Wall(wall_w, wall_h), Wall(wall_w, wall_h)
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        compose(core, states, S, places, wall)
        compose(core, states, S, places, wall_m, mask)
        core.synchronize()
    full = ws.compose(pattern(wall_w, wall_h), src, w, h, places)
    assert np.array_equal(wall.get(), full)
    hidden = places.copy()
    hidden[[s for s in range(S) if s not in chosen], 2] = 0
    assert np.array_equal(wall_m.get(), ws.compose(pattern(wall_w, wall_h), src, w, h, hidden))
    assert np.array_equal(states.get(), src)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, S, T = 64, 48, 2, 2
    n = 3 * w * h
    mw = ws.mask_words(n)
    src = random_states(w, h, S)
    states = Region(S, n, n + 16).put(src)
    span = (S - 1) * states.stride + n
    good, wall_w, wall_h = row_layout(w, h, [2, 3])
    wall = Wall(wall_w, wall_h)
    mask = Guarded(S * mw, torch.int32)
    recs, counts, escapes, _, _ = make_records(n, S, T, lambda s, t: [7 * s + t, 5000])
    d_recs = Guarded(recs.size, data=recs)
    keep = []                                                        # the host arrays of the calls below

    def place(rows):
        keep.append(np.ascontiguousarray(rows, np.int32))
        return keep[-1].ctypes.data

    def hdr(values):
        keep.append(np.ascontiguousarray(values, np.uint32))
        return keep[-1].ctypes.data

    def moved(s, dx=0, dy=0, k=None):
        rows = good.copy()
        rows[s, 0] += dx
        rows[s, 1] += dy
        if k is not None:
            rows[s, 2] = k
        return place(rows)

    tw0, th0 = ws.thumb_size(w, h, 2)
    with CUDACore(w, h, max_batch=S * T) as core:
        torch.cuda.synchronize()
        L, H = core._lib, core._h

        def comp(st=states.ptr, stride=states.stride, k=S, p=place(good), m=mask.ptr, wl=wall.ptr, ww=wall_w, wh=wall_h,
                 pitch=wall.pitch):
            return L.mi355_wall_compose_batch(H, st, stride, k, p, m, wl, ww, wh, pitch)

        def touched(cw=d_recs.ptr, c=hdr(counts), e=hdr(escapes), k=S, t=T, acc=0, m=mask.ptr):
            return L.mi355_cwire_touched_tiles_batch(H, cw, c, e, k, t, acc, m)

        big = counts.copy()
        big[1] = n + 1
        esc = escapes.copy()
        esc[2] = counts[2] + 1
        refused = [
            comp(k=-1), comp(k=S * T + 1), comp(st=None), comp(p=None), comp(wl=None), comp(stride=n - 1),
            comp(ww=0), comp(wh=0), comp(ww=-1), comp(pitch=3 * wall_w - 1),
            comp(p=moved(0, k=17)), comp(p=moved(1, k=-1)),
            comp(p=moved(0, dx=-3)), comp(p=moved(0, dy=-2)), comp(p=moved(1, dx=wall_w)), comp(p=moved(1, dy=wall_h)),
            comp(ww=int(good[1][0]) + 1), comp(wh=th0),              # a rectangle one pixel too far right, too far down
            comp(m=mask.ptr + 2),
            comp(wl=states.ptr + 8), comp(wl=states.ptr + span - 1), comp(wl=states.ptr - ((wall_h - 1) * wall.pitch + 3 * wall_w) + 1),
            comp(m=states.ptr), comp(m=states.ptr + span - 4),
            comp(m=wall.ptr + 3), comp(wl=mask.ptr),
            touched(k=-1), touched(t=-1), touched(k=S + 1, t=T), touched(cw=None), touched(c=None), touched(e=None), touched(m=None),
            touched(c=hdr(big)), touched(e=hdr(esc)), touched(cw=d_recs.ptr + 2), touched(m=mask.ptr + 2),
            touched(m=d_recs.ptr), touched(m=d_recs.ptr + recs.size - 4),
        ]
        assert refused == [lib.ERR_INVALID] * len(refused)
        assert comp(k=0) == lib.OK and comp(k=0, st=None, p=None, wl=None) == lib.OK     # nothing to do
        assert touched(k=0) == lib.OK and touched(t=0) == lib.OK and touched(k=0, cw=None, c=None, e=None, m=None) == lib.OK
        core.synchronize()
        assert (wall.get() == GUARD).all()
        mask.get(written=0)
        assert np.array_equal(states.get(), src) and np.array_equal(d_recs.get(), recs)
        # a hidden stream's place is not looked at, and nothing of it is written
        assert comp(k=1, stride=n, p=moved(0, dx=1000, k=0)) == lib.OK
        assert comp(p=moved(1, dx=1000, k=0), m=None) == lib.OK
        core.synchronize()
    got = wall.get()
    hidden = good.copy()
    hidden[1, 2] = 0
    assert np.array_equal(got, ws.compose(pattern(wall_w, wall_h), src, w, h, hidden))
    assert (tw0, th0) == (32, 24)

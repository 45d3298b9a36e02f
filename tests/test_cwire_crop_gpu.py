"""-m gpu: mi355_cwire_crop_batch / _cwire_batch -- the T compact records of each of S streams summed and cut to one rectangle
per stream, written with the byte indices of the rectangle's own frame or, MI355_CROP_KEEP_INDEX, of the full frame
(include/mi355diff.h, "A camera cropped").  The reference of every comparison is numpy (crop_spec).  Inputs and outputs live
in guarded buffers (gpu_util) that start as a non-zero pattern.  The shapes are the smallest that reach each seam of the tile
kernels: 33x7 (one partial tile, N no multiple of 4), 21x70 (a row is 63 bytes: a lane's 64 bytes straddle rows, the tile
edge at byte 4096 falls in mid-row), 64x48 (three tiles), 100x31 (a rectangle whose rows are 255 bytes: gaps of 254, 255,
256), 1400x3 (a row is wider than a tile), 640x360 (169 tiles, bursts of a server core)."""
import functools

import numpy as np
import pytest
import torch

import crop_spec
import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, cwire_check_host, lib
from gpu_util import DEV, CUDACore, Guarded, Region
from test_cwire_coalesce_gpu import burst, packed
from test_cwire_coalesce_gpu import run_compact as coalesce_compact

pytestmark = pytest.mark.gpu

KEEP = lib.CROP_KEEP_INDEX


# ---- the two forms --------------------------------------------------------------------------------------------------------
def run_compact(core, recs, hdr, S, T, rects, flags=0, cap=None):
    """-> (offsets uint32[S + 1], frame_pos uint64[S + 1], the whole output buffer of cap bytes); guards asserted."""
    cap = cwire_bytes_max(core.total, S) if cap is None else cap
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, pos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_crop_cwire_batch(src.ptr, hdr[0], hdr[1], S, T, rects, off.ptr, pos.ptr, out.ptr, cap, flags=flags)
    core.synchronize()
    assert np.array_equal(src.get(), recs)
    return off.get().view(np.uint32), pos.get().view(np.uint64), out.get()


def run_arrays(core, recs, hdr, S, T, rects, flags=0, cap=None, skew=0):
    """-> (offsets uint32[S + 1], xs, diff: the whole buffers of cap entries); guards asserted."""
    cap = S * core.total if cap is None else cap
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, xs, df = Guarded(S + 1, torch.int32), Guarded(cap, torch.int32), Guarded(cap, torch.uint8, skew=skew)
    torch.cuda.synchronize()
    core.cwire_crop_batch(src.ptr, hdr[0], hdr[1], S, T, rects, off.ptr, xs.ptr, df.ptr, cap, flags=flags)
    core.synchronize()
    assert np.array_equal(src.get(), recs)
    return off.get().view(np.uint32), xs.get(), df.get()


def check_both_forms(core, recs, hdr, S, T, w, h, rects, flags=0):
    """Both forms against the numpy reference, byte for byte; nothing behind the result is written.  -> the reference."""
    want = crop_spec.reference(recs, S, T, w, h, rects, keep_index=bool(flags & KEEP))
    what = (rects, flags)
    off, pos, out = run_compact(core, recs, hdr, S, T, rects, flags)
    assert np.array_equal(off, want[0]) and np.array_equal(pos, want[4]), what
    assert np.array_equal(out[:want[3].size], want[3]), what
    assert (out[want[3].size:] == 0x5C).all(), (what, "written behind the last record")
    aoff, axs, adf = run_arrays(core, recs, hdr, S, T, rects, flags, skew=1)
    tot = int(want[0][S])
    assert np.array_equal(aoff, want[0]) and np.array_equal(axs[:tot], want[1]) and np.array_equal(adf[:tot], want[2]), what
    assert (axs[tot:] == -7).all() and (adf[tot:] == 0x5C).all(), (what, "written behind the last entry")
    return want


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_records(w, h, S, T, seed=0):
    """Random records, about a fifth of the bytes each; a stream's later records repeat every second index of the one before
    with the negated difference, so that sums cancel.  -> (records, counts, escapes), read-only."""
    n = 3 * w * h
    rng = np.random.default_rng(1000 * w + h + seed)
    segs = []
    for b in range(S * T):
        cnt = int(rng.integers(n // 8, n // 4))
        x, d = np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)
        if b % T:
            px, pd = segs[-1]
            cx, cd = px[::2], (256 - np.asarray(pd[::2])) % 256
            fresh = ~np.isin(x, cx)
            x, d = np.concatenate([x[fresh], cx]), np.concatenate([d[fresh], cd])
            order = np.argsort(x)
            x, d = x[order], d[order]
        segs.append((x, d))
    recs, _ = spec.encode(*packed(segs))
    counts, escapes = spec.headers(recs, S * T)
    for a in (recs, counts, escapes):
        a.setflags(write=False)
    return recs, counts, escapes


def rectangle_sets(w, h, skip):
    """[(what, [3 rectangles])]: the same rectangle for three streams, and three different ones in one call.  skip: rows that
    leave whole tiles of the frame out (the frame's last rows where it has a single tile)."""
    one = lambda r: [r, r, r]
    return [
        ("the full frame", one((0, 0, w, h))),
        ("one pixel", one((w // 2, h // 2, 1, 1))),
        ("one column", one((w - 1, 0, 1, h))),
        ("one row", one((0, h // 2, w, 1))),
        ("the bottom-right corner", one((w - max(w // 3, 1), h - max(h // 3, 1), max(w // 3, 1), max(h // 3, 1)))),
        ("rows that skip whole tiles", one((1, skip[0], w - 1, skip[1]))),
        ("no column", one((w // 2, 1, 0, 2))),
        ("no row", one((0, h, w, 0))),
        ("three different rectangles", [(w // 3, h // 3, max(w // 3, 1), max(h // 3, 1)), (0, 0, 0, 0), (0, 1, w, h - 1)]),
    ]


# ---- 1. every rectangle at every small shape ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,skip", [(33, 7, (5, 2)), (21, 70, (66, 4)), (64, 48, (22, 20)), (1400, 3, (2, 1))])
def test_rectangles(w, h, skip):
    """33x7: N = 693; 21x70: tile 0 ends in mid-row, rows 66 .. 69 lie in tile 1 alone; 64x48: rows 22 .. 41 are bytes 4224 ..
    8063, inside tile 1; 1400x3: a row is 4200 bytes, row 2 begins at 8400 and leaves tiles 0 and 1 out, and every rectangle
    narrower than the frame leaves tiles inside its rows but outside its columns."""
    S, T = 3, 2
    n = 3 * w * h
    recs, counts, escapes = random_records(w, h, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        for what, rects in rectangle_sets(w, h, skip):
            for flags in (0, KEEP):
                want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, rects, flags)
                if what in ("no column", "no row"):
                    assert list(want[4]) == [0, 8, 16, 24], what
                elif what not in ("one pixel", "three different rectangles"):
                    assert int(want[0][S]) > 0, what
        # the full frame is the coalescer, with or without KEEP_INDEX
        coff, cpos, cout = coalesce_compact(core, recs, (counts, escapes), S, T, n)
        for flags in (0, KEEP):
            off, pos, out = run_compact(core, recs, (counts, escapes), S, T, [(0, 0, w, h)] * S, flags)
            assert np.array_equal(off, coff) and np.array_equal(pos, cpos) and np.array_equal(out, cout)
        # ... and with one record per stream, the input
        off, pos, out = run_compact(core, recs, (counts, escapes), S * T, 1, [(0, 0, w, h)] * (S * T), cap=cwire_bytes_max(n, S * T))
        assert int(pos[S * T]) == recs.size and np.array_equal(out[:recs.size], recs)


# ---- 2. gaps of 254, 255 and 256 in the rectangle's frame -----------------------------------------------------------------
def test_mapped_gaps_of_254_255_256():
    """100x31, rectangle (5, 2, 85, 20): a row of the frame is 300 bytes, a row of the rectangle 255.  Stream d (d = 0, 1, 2)
    holds entries one row apart at column bytes c and c + d, inside input tile 0 (rows 3 and 4) and across the tile edge at
    byte 4096 (rows 13 and 14; the edge is row 13, column byte 196): input gaps of 299 + d, all escaped, become 254 + d -- the
    first no longer an escape, the others still.  A second record per stream puts an entry outside the rectangle between each
    pair."""
    w, h, rect, c = 100, 31, (5, 2, 85, 20), 100
    n, S = 3 * w * h, 3
    T, segs = 2, []
    for d in range(S):
        x = [3 * 300 + c, 4 * 300 + c + d, 13 * 300 + c, 14 * 300 + c + d]
        assert x[2] < 4096 <= x[3] and list(spec.gaps(x)) == [1000, 299 + d, 2699 - d, 299 + d]
        outside = [4 * 300 + 5, 13 * 300 + 280, 14 * 300 + 2]          # column bytes 5, 280 and 2: not in [15, 270)
        segs += [(x, [1 + d] * 4), (outside, [9, 9, 9])]
    recs, _ = spec.encode(*packed(segs))
    counts, escapes = spec.headers(recs, S * T)
    assert list(escapes[::2]) == [4, 4, 4]
    want = crop_spec.reference(recs, S, T, w, h, [rect] * S)
    for d in range(S):
        kept = want[1][int(want[0][d]):int(want[0][d + 1])]
        assert list(spec.gaps(kept)) == [255 + c - 15, 254 + d, 9 * 255 - d - 1, 254 + d]
    assert list(spec.headers(want[3], S)[1]) == [2, 4, 4]
    with CUDACore(w, h, max_batch=S * T) as core:
        for flags in (0, KEEP):
            check_both_forms(core, recs, (counts, escapes), S, T, w, h, [rect] * S, flags)
        check_both_forms(core, recs, (counts, escapes), S, T, w, h, [rect, (0, 0, w, h), (5, 4, 85, 11)])


# ---- 3. bursts of a server core -------------------------------------------------------------------------------------------
def test_server_bursts():
    """640x360, S = 2, T = 3: 169 tiles, the last one ragged; a row is 1920 bytes."""
    w, h, S, T = 640, 360, 2, 3
    _, recs, counts, escapes, _, _ = burst(w, h, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        for rects in ([(0, 0, w, h)] * 2, [(160, 90, 320, 180), (639, 0, 1, 360)], [(3, 100, 630, 10), (0, 0, 0, 0)]):
            for flags in (0, KEEP):
                want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, rects, flags)
                assert int(want[0][1]) > 0


# ---- 4. the law, on the GPU route -----------------------------------------------------------------------------------------
def test_law_through_the_gpu_client():
    """The cropped records applied (mi355_apply_multi_cwire_batch of a core of the rectangle's size) to the crops of the base
    states give the crops of the sender's states after the burst; the KEEP_INDEX records applied to the full base states
    change exactly the rectangles, in the same way.  The host client agrees."""
    w, h, S, T = 64, 48, 3, 4
    n = 3 * w * h
    bases, recs, counts, escapes, after, _ = burst(w, h, S, T)
    rw, rh = 23, 17
    rects = [(0, 0, rw, rh), (20, 15, rw, rh), (w - rw, h - rh, rw, rh)]
    m = 3 * rw * rh
    with CUDACore(w, h, max_batch=S * T) as core, CUDACore(rw, rh, max_batch=S) as small:
        off, pos, out = run_compact(core, recs, (counts, escapes), S, T, rects)
        made = out[:int(pos[S])]
        oc, oe = spec.headers(made, S)
        assert int(off[S]) > 0
        src = Guarded(made.size, torch.uint8, data=made)
        st = Region(S, m).put([crop_spec.crop_state(bases[s], w, h, rects[s]) for s in range(S)])
        torch.cuda.synchronize()
        small.apply_multi_cwire_batch(src.ptr, oc, oe, S, st.ptr, stride=st.stride)
        small.synchronize()
        got = st.get()
        for s in range(S):
            assert np.array_equal(got[s], crop_spec.crop_state(after[s], w, h, rects[s])), s
            host = crop_spec.crop_state(bases[s], w, h, rects[s])
            sl = made[int(pos[s]):int(pos[s + 1])]
            assert cwire_apply_host(host, sl, 1) == sl.size and np.array_equal(host, got[s]), s
        off, pos, out = run_compact(core, recs, (counts, escapes), S, T, rects, KEEP)
        made = out[:int(pos[S])]
        oc, oe = spec.headers(made, S)
        src = Guarded(made.size, torch.uint8, data=made)
        st = Region(S, n).put(bases)
        torch.cuda.synchronize()
        core.apply_multi_cwire_batch(src.ptr, oc, oe, S, st.ptr, stride=st.stride)
        core.synchronize()
        got = st.get()
        for s in range(S):
            x0, y0, _, _ = rects[s]
            expect = np.array(bases[s]).reshape(h, 3 * w)
            expect[y0:y0 + rh, 3 * x0:3 * (x0 + rw)] = after[s].reshape(h, 3 * w)[y0:y0 + rh, 3 * x0:3 * (x0 + rw)]
            assert np.array_equal(got[s], expect.reshape(-1)), s


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------
def test_capacity():
    """Compact form: with one byte too few for the middle record it is skipped whole (and so is the one behind it: positions
    ascend), the one in front is written, nothing is written past capacity_bytes, frame_pos stays exact.  The sum of the
    per-rectangle maxima suffices, exactly, for records that change every byte.  Arrays form: entries past `capacity` are
    dropped, the offsets stay exact."""
    w, h, S, T = 64, 48, 3, 2
    n = 3 * w * h
    recs, counts, escapes = random_records(w, h, S, T)
    rects = [(0, 0, 40, 30), (8, 4, 40, 30), (24, 18, 40, 30)]
    woff, wxs, wdf, wrecs, wpos = crop_spec.reference(recs, S, T, w, h, rects)
    with CUDACore(w, h, max_batch=S * T) as core:
        for cap in (int(wpos[2]) - 1, int(wpos[2]), int(wpos[3]) - 1, 8, 0):
            off, pos, out = run_compact(core, recs, (counts, escapes), S, T, rects, cap=cap)
            assert np.array_equal(off, woff) and np.array_equal(pos, wpos), cap
            assert out.size == cap
            for s in range(S):
                a, b = int(wpos[s]), int(wpos[s + 1])
                if b <= cap:
                    assert np.array_equal(out[a:b], wrecs[a:b]), (cap, s)
                else:
                    assert (out[a:cap] == 0x5C).all(), (cap, s, "a record that does not fit is skipped whole")
        mid = int(woff[1]) + (int(woff[2]) - int(woff[1])) // 2
        for cap in (mid, int(woff[S]) - 1, 3, 0):
            off, xs, df = run_arrays(core, recs, (counts, escapes), S, T, rects, cap=cap, skew=3)
            assert np.array_equal(off, woff), cap
            assert np.array_equal(xs, wxs[:cap]) and np.array_equal(df, wdf[:cap]), cap
        # every byte of every stream changed: record s holds 3*w_s*h_s entries and no escape
        every = np.arange(n)
        dense, _ = spec.encode(*packed([(every, 1 + every % 255)] * S))
        rects = [(0, 0, w, h), (1, 1, 21, 7), (63, 47, 1, 1)]
        cap = sum(cwire_bytes_max(3 * r[2] * r[3], 1) for r in rects)
        want = crop_spec.reference(dense, S, 1, w, h, rects)
        assert want[3].size == cap
        off, pos, out = run_compact(core, dense, spec.headers(dense, S), S, 1, rects, cap=cap)
        assert np.array_equal(pos, want[4]) and np.array_equal(out, want[3])


# ---- 6. malformed content -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5, 6])
def test_malformed_content_under_consistent_headers(seed):
    """The damaged records of test_cwire_coalesce_gpu: random bytes where well-formed records of the same headers stood.  The
    guards around the input span and all outputs stay intact; every output record is well-formed and canonical for its
    rectangle's frame (mi355_cwire_check_host against N'_s; against N with KEEP_INDEX), and offsets and frame_pos agree."""
    w, h, S, T = 64, 48, 3, 4
    n, B = 3 * w * h, S * T
    rng = np.random.default_rng(seed)
    segs = []
    for b in range(B):
        cnt = [n, 0, 700, 64, 3000, 1][b % 6]
        segs.append((np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)))
    good, _ = spec.encode(*packed(segs))
    counts, escapes = spec.headers(good, B)
    assert int(escapes.sum()) > 0
    bad = rng.integers(0, 256, good.size, dtype=np.uint8)
    if seed == 6:                                       # many escape codes, escapes that run far past N and wrap
        bad[rng.random(good.size) < 0.3] = 255
    rects = [(0, 0, w, h), (7, 5, 50, 40), (63, 0, 1, 48)]
    with CUDACore(w, h, max_batch=B) as core:
        for flags in (0, KEEP):
            off, pos, out = run_compact(core, bad, (counts, escapes), S, T, rects, flags)
            c2, e2 = spec.headers(out, S)
            assert np.array_equal(np.diff(off.astype(np.int64)), c2)
            assert np.array_equal(pos, np.cumsum([0] + [spec.frame_bytes(a, b) for a, b in zip(c2, e2)]).astype(np.uint64))
            assert (out[int(pos[S]):] == 0x5C).all()
            assert int(off[S]) > 0
            for s in range(S):
                frame = n if flags else 3 * rects[s][2] * rects[s][3]
                v = cwire_check_host(out[int(pos[s]):int(pos[s + 1])], c2[s:s + 1], e2[s:s + 1], frame)
                assert v[0][0] == 0, (flags, s, v)
            doff, dxs, ddf = spec.decode(out, S)
            aoff, axs, adf = run_arrays(core, bad, (counts, escapes), S, T, rects, flags)
            tot = int(doff[S])
            assert np.array_equal(aoff, doff) and np.array_equal(axs[:tot], dxs) and np.array_equal(adf[:tot], ddf)
            assert (ddf != 0).all()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, S, T = 64, 48, 2, 2
    n, B = 3 * w * h, S * T
    rng = np.random.default_rng(3)
    recs, _ = spec.encode(*packed([(np.sort(rng.choice(n, 50, replace=False)), rng.integers(1, 256, 50)) for _ in range(B)]))
    counts, escapes = spec.headers(recs, B)
    cap = cwire_bytes_max(n, S)
    # one buffer that holds the input in front and room behind it, for the overlap cases
    big = Guarded(recs.size + cap + 64, torch.uint8)
    big.t[:recs.size].copy_(torch.from_numpy(recs).to(DEV))
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, pos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    xs, df = Guarded(S * n, torch.int32), Guarded(S * n, torch.uint8)
    L = lib.load()
    c, e = counts.ctypes.data, escapes.ctypes.data
    good = np.array([[8, 4, 40, 30], [0, 0, w, h]], np.int32)
    r = good.ctypes.data
    inside = big.ptr + recs.size - 8
    inside -= inside % 8
    with CUDACore(w, h, max_batch=B) as core:
        H = core._h
        torch.cuda.synchronize()

        def compact(core_=H, src_=src.ptr, c_=c, e_=e, S_=S, T_=T, r_=r, f_=0, off_=off.ptr, pos_=pos.ptr, out_=out.ptr, cap_=cap):
            return L.mi355_cwire_crop_cwire_batch(core_, src_, c_, e_, S_, T_, r_, f_, off_, pos_, out_, cap_)

        def arrays(core_=H, src_=src.ptr, c_=c, e_=e, S_=S, T_=T, r_=r, f_=0, off_=off.ptr, xs_=xs.ptr, df_=df.ptr, cap_=S * n):
            return L.mi355_cwire_crop_batch(core_, src_, c_, e_, S_, T_, r_, f_, off_, xs_, df_, cap_)

        more_e = (escapes + counts + 1).astype(np.uint32)
        more_n = np.full(B, n + 1, np.uint32)
        zero_e = np.zeros(B, np.uint32)
        big_i = 2 ** 31 - 1
        bad_rects = [np.array([[8, 4, 40, 30], rect], np.int32) for rect in (
            [-1, 0, 4, 4], [0, -1, 4, 4], [0, 0, -1, 4], [0, 0, 4, -1],            # a negative member
            [w - 3, 0, 4, 4], [0, h - 3, 4, 4], [w, 0, 1, 1], [0, 0, w + 1, h],    # past the right or the bottom edge
            [1, 0, big_i, 1], [0, 1, 1, big_i], [big_i, 0, big_i, 1])]            # sums that wrap in 32 bits
        cases = [
            # whatever the coalescer refuses
            compact(core_=None), arrays(core_=None),
            compact(S_=-1), compact(T_=-1), arrays(S_=-1), arrays(T_=-1),
            compact(S_=B + 1, T_=1), compact(S_=S, T_=T + 1), arrays(S_=1, T_=B + 1),
            compact(src_=None), compact(c_=None), compact(e_=None), compact(off_=None), compact(pos_=None), compact(out_=None),
            arrays(src_=None), arrays(c_=None), arrays(e_=None), arrays(off_=None), arrays(xs_=None), arrays(df_=None),
            compact(e_=more_e.ctypes.data), arrays(e_=more_e.ctypes.data),
            compact(c_=more_n.ctypes.data, e_=zero_e.ctypes.data), arrays(c_=more_n.ctypes.data, e_=zero_e.ctypes.data),
            compact(src_=src.ptr + 2), compact(out_=out.ptr + 2), compact(off_=off.ptr + 2), compact(pos_=pos.ptr + 4),
            arrays(src_=src.ptr + 1), arrays(off_=off.ptr + 1), arrays(xs_=xs.ptr + 2),
            compact(src_=big.ptr, out_=big.ptr + recs.size - 4), compact(src_=big.ptr, out_=big.ptr - 4, cap_=8),
            compact(src_=big.ptr, off_=big.ptr + recs.size - 4), compact(src_=big.ptr, pos_=inside),
            arrays(src_=big.ptr, xs_=big.ptr + recs.size - 4), arrays(src_=big.ptr, df_=big.ptr + recs.size - 1),
            arrays(src_=big.ptr, off_=big.ptr - 4 * S), arrays(src_=big.ptr, df_=big.ptr - 3, cap_=4),
            # the call's own
            compact(r_=None), arrays(r_=None),
            compact(f_=2), arrays(f_=2), compact(f_=KEEP | 4), arrays(f_=0x80000000),
        ]
        cases += [compact(r_=b.ctypes.data) for b in bad_rects] + [arrays(r_=b.ctypes.data, f_=KEEP) for b in bad_rects]
        assert all(rc == lib.ERR_INVALID for rc in cases), cases
        core.synchronize()
        for g in (off, pos, out, xs, df):
            g.get(written=0)
        assert np.array_equal(src.get(), recs)
        h_big = big.get()
        assert np.array_equal(h_big[:recs.size], recs) and (h_big[recs.size:] == 0x5C).all()
        # nstreams * nframes == 0: offsets[0] = 0 (and frame_pos[0] = 0) and nothing else, with or without rectangles
        assert compact(S_=0, r_=None) == lib.OK and arrays(T_=0) == lib.OK
        core.synchronize()
        assert off.get(written=1)[0] == 0 and pos.get(written=1)[0] == 0
        for g in (out, xs, df):
            g.get(written=0)
        # ... and the calls above left the core in order: the burst is cropped
        assert compact() == lib.OK
        core.synchronize()
        want = crop_spec.reference(recs, S, T, w, h, good)
        assert np.array_equal(out.get()[:want[3].size], want[3])

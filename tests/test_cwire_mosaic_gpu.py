"""-m gpu: mi355_cwire_mosaic_batch / _cwire_batch -- the T compact records of each of S cameras summed and placed side by side
into ONE record of a canvas frame (include/mi355diff.h, "Many cameras on one canvas").  The reference of every comparison is
numpy (mosaic_spec).  Inputs and outputs live in guarded buffers (gpu_util) that start as a non-zero pattern.  The shapes are the
smallest that reach each seam of the canvas tile kernels: 2 x 2 grids of 33x7, 21x70, 64x48 and 1400x3 cameras in canvases of
(2w + 1) x (2h + 1) pixels, whose rows are 201, 129, 387 and 8403 bytes (a lane's 64 bytes straddle rows, a tile edge falls in
mid-row, a row is wider than a tile) and whose byte count is odd; a 10 x 80 canvas with rows of 30 bytes; 65 and 129 streams (one
past a ballot round, one past a table launch of 128); 65 records per stream; a 1280x720 canvas of 675 tiles."""
import functools

import numpy as np
import pytest
import torch

import crop_spec
import cwire_spec as spec
import mosaic_spec
from cudavideostream_amd import cwire_bytes_max, cwire_check_host, lib
from gpu_util import DEV, CUDACore, Guarded, Region
from test_cwire_coalesce_gpu import burst, packed
from test_cwire_coalesce_gpu import run_compact as coalesce_compact
from test_cwire_crop_gpu import random_records
from test_cwire_crop_gpu import run_compact as crop_compact

pytestmark = pytest.mark.gpu


# ---- the two forms --------------------------------------------------------------------------------------------------------
def run_compact(core, recs, hdr, S, T, place, cw, ch, cap=None):
    """-> (offsets uint32[2], frame_pos uint64[2], the whole output buffer of cap bytes); guards asserted."""
    cap = cwire_bytes_max(3 * cw * ch, 1) if cap is None else cap
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, pos, out = Guarded(2, torch.int32), Guarded(2, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_mosaic_cwire_batch(src.ptr, hdr[0], hdr[1], S, T, place, cw, ch, off.ptr, pos.ptr, out.ptr, cap)
    core.synchronize()
    assert np.array_equal(src.get(), recs)
    return off.get().view(np.uint32), pos.get().view(np.uint64), out.get()


def run_arrays(core, recs, hdr, S, T, place, cw, ch, cap=None, skew=0):
    """-> (offsets uint32[2], xs, diff: the whole buffers of cap entries); guards asserted."""
    cap = 3 * cw * ch if cap is None else cap
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, xs, df = Guarded(2, torch.int32), Guarded(cap, torch.int32), Guarded(cap, torch.uint8, skew=skew)
    torch.cuda.synchronize()
    core.cwire_mosaic_batch(src.ptr, hdr[0], hdr[1], S, T, place, cw, ch, off.ptr, xs.ptr, df.ptr, cap)
    core.synchronize()
    assert np.array_equal(src.get(), recs)
    return off.get().view(np.uint32), xs.get(), df.get()


def check_both_forms(core, recs, hdr, S, T, w, h, place, cw, ch):
    """Both forms against the numpy reference, byte for byte; nothing behind the result is written.  -> the reference."""
    want = mosaic_spec.reference(recs, S, T, w, h, place, cw, ch)
    what = (place, cw, ch)
    off, pos, out = run_compact(core, recs, hdr, S, T, place, cw, ch)
    assert np.array_equal(off, want[0]) and np.array_equal(pos, want[4]), what
    assert np.array_equal(out[:want[3].size], want[3]), what
    assert (out[want[3].size:] == 0x5C).all(), (what, "written behind the record")
    aoff, axs, adf = run_arrays(core, recs, hdr, S, T, place, cw, ch, skew=1)
    tot = int(want[0][1])
    assert np.array_equal(aoff, want[0]) and np.array_equal(axs[:tot], want[1]) and np.array_equal(adf[:tot], want[2]), what
    assert (axs[tot:] == -7).all() and (adf[tot:] == 0x5C).all(), (what, "written behind the last entry")
    return want


def stream_slice(recs, counts, escapes, s, T):
    """The bytes of stream s's T records."""
    pos = np.cumsum([0] + [spec.frame_bytes(a, b) for a, b in zip(counts, escapes)])
    return recs[int(pos[s * T]):int(pos[(s + 1) * T])]


def grid_2x2(w, h):
    """Four whole cameras in a (2w + 1) x (2h + 1) canvas: column w and row h of the canvas stay uncovered, the fourth camera
    ends in the canvas' last row and column."""
    return [(0, 0, w, h, 0, 0), (0, 0, w, h, w + 1, 0), (0, 0, w, h, 0, h + 1), (0, 0, w, h, w + 1, h + 1)], 2 * w + 1, 2 * h + 1


# ---- 1. 2 x 2 grids at every small shape ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(33, 7), (21, 70), (64, 48), (1400, 3)])
def test_grid_2x2(w, h):
    S, T = 4, 2
    recs, counts, escapes = random_records(w, h, S, T)
    place, cw, ch = grid_2x2(w, h)
    assert (3 * cw * ch) % 2 == 1 and 3 * cw in (201, 129, 387, 8403)
    with CUDACore(w, h, max_batch=S * T) as core:
        want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, place, cw, ch)
        assert int(want[0][1]) > 0
        # the cameras moved: the margin at the right and at the bottom, and the first two swapped
        moved = [(0, 0, w, h, w, 0), (0, 0, w, h, 0, 0), (0, 0, w, h, 0, h), (0, 0, w, h, w, h)]
        check_both_forms(core, recs, (counts, escapes), S, T, w, h, moved, cw, ch)
        # law (d): bands stacked vertically are the bands' coalesced records with index bias s*N
        n = 3 * w * h
        bands = check_both_forms(core, recs, (counts, escapes), S, T, w, h, [(0, 0, w, h, 0, s * h) for s in range(S)], w, S * h)
        coff, cpos, cout = coalesce_compact(core, recs, (counts, escapes), S, T, n)
        doff, dxs, ddf = spec.decode(cout, S)
        bias = np.repeat(np.arange(S) * n, np.diff(doff.astype(np.int64)))
        assert np.array_equal(bands[1], (dxs + bias).astype(np.int32)) and np.array_equal(bands[2], ddf)


# ---- 2. a canvas of short rows ---------------------------------------------------------------------------------------------
def test_narrow_canvas():
    """Source 16x40, the rectangle (3, 0, 5, 40) of two cameras into a 10 x 80 canvas: rows of 30 bytes, 2400 bytes in all, so
    the one tile spans every row and the walk over a camera crosses 40 source rows of which it keeps 15 bytes each."""
    w, h, S, T = 16, 40, 2, 2
    recs, counts, escapes = random_records(w, h, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        for place in ([(3, 0, 5, 40, 0, 0), (3, 0, 5, 40, 5, 40)], [(3, 0, 5, 40, 5, 0), (3, 0, 5, 40, 0, 40)],
                      [(3, 0, 5, 40, 0, 20), (3, 0, 5, 40, 5, 20)]):
            want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, place, 10, 80)
            assert int(want[0][1]) > 0


# ---- 3. gaps of 254, 255 and 256 on the canvas -----------------------------------------------------------------------------
@pytest.mark.parametrize("d", [255, 256, 257])
def test_canvas_gaps(d):
    """Source 100x31 (rows of 300 bytes), three cameras' rectangles of 20 x 31 pixels stacked in a 20 x 100 canvas (rows of 60
    bytes, 6000 bytes, the tile edge at byte 4096 = row 68, column byte 16) at rows 0, 33 and 66: an empty band of two rows
    between the first two.  Pairs of entries whose canvas indices differ by exactly d: inside canvas tile 0 (camera 0), across
    the empty band (camera 0's row 29 and camera 1's row 0) and across the tile edge (camera 2)."""
    w, h, S, T = 100, 31, 3, 1
    sx = [0, 7, 11]
    place = [(sx[0], 0, 20, 31, 0, 0), (sx[1], 0, 20, 31, 0, 33), (sx[2], 0, 20, 31, 0, 66)]
    cw, ch = 20, 100

    def source(s, y):        # the source byte of canvas byte y of camera s
        R, q = divmod(y, 60)
        return (R - place[s][5]) * 300 + 3 * sx[s] + q

    pairs = {0: [100, 100 + d, 1750], 1: [1750 + d], 2: [3996, 3996 + d]}
    assert 3996 < 4096 <= 3996 + d and 1750 // 60 == 29 and (1750 + d) // 60 == 33
    segs = [([source(s, y) for y in pairs[s]], [1 + s + k for k in range(len(pairs[s]))]) for s in range(S)]
    # ... and an entry of every camera outside its rectangle, in between
    segs[0] = (sorted(segs[0][0] + [2 * 300 + 200]), [5, 6, 7, 8])
    recs, _ = spec.encode(*packed(segs))
    counts, escapes = spec.headers(recs, S * T)
    want = mosaic_spec.reference(recs, S, T, w, h, place, cw, ch)
    assert list(want[1]) == [100, 100 + d, 1750, 1750 + d, 3996, 3996 + d]
    assert list(spec.gaps(want[1]))[1::2] == [d - 1] * 3
    assert int(spec.headers(want[3], 1)[1][0]) == (5 if d >= 256 else 2)
    with CUDACore(w, h, max_batch=S * T) as core:
        check_both_forms(core, recs, (counts, escapes), S, T, w, h, place, cw, ch)


# ---- 4. source rectangles that are not the frame ---------------------------------------------------------------------------
def test_rectangles_of_different_sizes():
    """64x48 cameras, 100 x 70 canvas: different sizes per stream, w == 0, h == 0, and a camera that ends in the canvas' last
    row and column."""
    w, h, S, T = 64, 48, 5, 2
    recs, counts, escapes = random_records(w, h, S, T)
    place = [(5, 3, 30, 20, 0, 0), (10, 8, 50, 40, 40, 25), (4, 4, 0, 10, 50, 0), (4, 4, 10, 0, 0, 60), (0, 20, 64, 5, 36, 65)]
    with CUDACore(w, h, max_batch=S * T) as core:
        want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, place, 100, 70)
        assert int(want[1][-1]) >= 3 * 100 * 69 + 3 * 36       # an entry in the last row
        # nothing but empty placements: the 8-byte record
        none = check_both_forms(core, recs, (counts, escapes), S, T, w, h, [(4, 4, 0, 10, 50, 0), (4, 4, 10, 0, 0, 60)] * 2 + [(0, 0, 0, 0, 0, 0)],
                                100, 70)
        assert list(none[4]) == [0, 8]


# ---- 5. many streams, many records -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T", [(65, 1), (129, 1), (2, 65)])
def test_many_streams_and_records(S, T):
    """Source 16x8.  S = 65: one past a ballot round of 64 streams; S = 129: one past a table launch of 128; 4x4 rectangles,
    16 to a canvas row.  S = 2, T = 65: the records of a stream in two ballot rounds, whole cameras side by side."""
    w, h = 16, 8
    recs, counts, escapes = random_records(w, h, S, T)
    if T == 1:
        place = [(s % 13, s % 5, 4, 4, 4 * (s % 16), 4 * (s // 16)) for s in range(S)]
        cw, ch = 64, 4 * ((S + 15) // 16)
    else:
        place, cw, ch = [(0, 0, w, h, 0, 0), (0, 0, w, h, 17, 1)], 33, 9
    with CUDACore(w, h, max_batch=S * T) as core:
        want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, place, cw, ch)
        assert int(want[0][1]) > 0
        last = place[S - 1]
        assert mosaic_spec.canvas_sums(crop_spec.sums(recs, S, T, 3 * w * h), w, h, place, cw, ch).reshape(ch, 3 * cw)[
            last[5]:last[5] + last[3], 3 * last[4]:3 * (last[4] + last[2])].any(), "the last stream lands somewhere"


# ---- 6. overlapping destinations -------------------------------------------------------------------------------------------
def test_overlapping_destinations_add():
    w, h = 33, 7
    n = 3 * w * h
    recs, counts, escapes = random_records(w, h, 3, 2)
    rng = np.random.default_rng(9)
    x = np.sort(rng.choice(n, 300, replace=False))
    d = rng.integers(1, 256, 300).astype(np.uint8)
    neg, _ = spec.encode(*packed([(x, d), (x, (256 - d.astype(np.int64)).astype(np.uint8))]))
    with CUDACore(w, h, max_batch=6) as core:
        place = [(0, 0, w, h, 0, 0), (0, 0, w, h, 10, 3), (3, 1, 20, 5, 5, 2)]
        want = check_both_forms(core, recs, (counts, escapes), 3, 2, w, h, place, 50, 12)
        assert int(want[0][1]) > 0
        # a second stream that negates the first, on the same destination: n = 0
        none = check_both_forms(core, neg, spec.headers(neg, 2), 2, 1, w, h, [(0, 0, w, h, 4, 2)] * 2, 40, 10)
        assert list(none[4]) == [0, 8] and list(none[0]) == [0, 0]


# ---- 7. the laws through a second core of the canvas' geometry ---------------------------------------------------------------
def test_laws_b_and_c_on_the_gpu():
    w, h, S, T = 64, 48, 4, 2
    n = 3 * w * h
    recs, counts, escapes = random_records(w, h, S, T)
    cw, ch = 2 * w + 1, 2 * h + 1
    place = [(0, 0, w, h, 0, 0), (16, 0, 32, h, w + 1, 0), (0, 16, w, 16, 0, h + 1), (w - 1, h - 1, 1, 1, 2 * w, 2 * h)]
    with CUDACore(w, h, max_batch=S * T) as core, CUDACore(cw, ch, max_batch=1) as canvas:
        off, pos, out = run_compact(core, recs, (counts, escapes), S, T, place, cw, ch)
        made = out[:int(pos[1])]
        hdr = spec.headers(made, 1)
        # (b) the crop of the output to a destination = the crop of the camera's input to its source
        for s in range(S):
            sx, sy, rw, rh, dx, dy = place[s]
            _, bpos, back = crop_compact(canvas, made, hdr, 1, 1, [(dx, dy, rw, rh)])
            sl = stream_slice(recs, counts, escapes, s, T)
            _, spos, direct = crop_compact(core, sl, (counts[s * T:(s + 1) * T], escapes[s * T:(s + 1) * T]), 1, T, [(sx, sy, rw, rh)])
            assert np.array_equal(bpos, spos) and np.array_equal(back[:int(bpos[1])], direct[:int(spos[1])]), s
        # (c) one full frame on a canvas of its size: the coalescer; one rectangle at the origin of its own canvas: the crop
        sl = stream_slice(recs, counts, escapes, 1, T)
        h1 = (counts[T:2 * T], escapes[T:2 * T])
        coff, cpos, cout = coalesce_compact(core, sl, h1, 1, T, n)
        off, pos, out = run_compact(core, sl, h1, 1, T, [(0, 0, w, h, 0, 0)], w, h, cap=cwire_bytes_max(n, 1))
        assert np.array_equal(off, coff) and np.array_equal(pos, cpos) and np.array_equal(out, cout)
        rect = (9, 5, 40, 30)
        coff, cpos, cout = crop_compact(core, sl, h1, 1, T, [rect], cap=cwire_bytes_max(3 * 40 * 30, 1))
        off, pos, out = run_compact(core, sl, h1, 1, T, [rect + (0, 0)], 40, 30)
        assert np.array_equal(off, coff) and np.array_equal(pos, cpos) and np.array_equal(out, cout)


# ---- 8. capacity ----------------------------------------------------------------------------------------------------------
def test_capacity():
    """Compact form: with capacity_bytes 4 short of the record nothing is written, offsets and frame_pos are exact; with
    exactly its size the record is there.  Arrays form: entries past `capacity` are dropped, the offsets stay exact."""
    w, h, S, T = 64, 48, 4, 2
    recs, counts, escapes = random_records(w, h, S, T)
    place, cw, ch = grid_2x2(w, h)
    woff, wxs, wdf, wrec, wpos = mosaic_spec.reference(recs, S, T, w, h, place, cw, ch)
    with CUDACore(w, h, max_batch=S * T) as core:
        for cap in (wrec.size - 4, wrec.size, 8, 4, 0):
            off, pos, out = run_compact(core, recs, (counts, escapes), S, T, place, cw, ch, cap=cap)
            assert np.array_equal(off, woff) and np.array_equal(pos, wpos), cap
            assert out.size == cap
            if cap >= wrec.size:
                assert np.array_equal(out, wrec)
            else:
                assert (out == 0x5C).all(), (cap, "a record that does not fit is not written at all")
        tot = int(woff[1])
        for cap in (tot - 1, tot // 2, 4097, 3, 0):
            off, xs, df = run_arrays(core, recs, (counts, escapes), S, T, place, cw, ch, cap=cap, skew=3)
            assert np.array_equal(off, woff), cap
            assert np.array_equal(xs, wxs[:cap]) and np.array_equal(df, wdf[:cap]), cap
        # every byte of every camera changed, the canvas covered whole: mi355_cwire_bytes_max(Nc, 1) is needed, exactly
        every = np.arange(3 * w * h)
        dense, _ = spec.encode(*packed([(every, 1 + every % 255)] * S))
        tight = [(0, 0, w, h, 0, 0), (0, 0, w, h, w, 0), (0, 0, w, h, 0, h), (0, 0, w, h, w, h)]
        want = mosaic_spec.reference(dense, S, 1, w, h, tight, 2 * w, 2 * h)
        assert want[3].size == cwire_bytes_max(3 * 4 * w * h, 1)
        off, pos, out = run_compact(core, dense, spec.headers(dense, S), S, 1, tight, 2 * w, 2 * h)
        assert np.array_equal(pos, want[4]) and np.array_equal(out, want[3])


# ---- 9. the scratch bound --------------------------------------------------------------------------------------------------
def test_scratch_bound():
    """Source 33x7 (one tile) on a core of max_batch 2: the facts of two canvas tiles fit.  A BGR24 canvas has a multiple of 3
    bytes, so the largest canvas of two tiles is 65 x 42 = 8190 bytes (accepted and correct) and the smallest of three is
    2731 x 1 = 8193 bytes (refused, every output untouched); so is 66 x 42."""
    w, h, S, T = 33, 7, 2, 1
    recs, counts, escapes = random_records(w, h, S, T)
    place = [(0, 0, w, h, 0, 0), (0, 0, w, h, 32, 35)]
    L = lib.load()
    with CUDACore(w, h, max_batch=2) as core:
        want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, place, 65, 42)
        assert int(want[0][1]) > 0 and int(want[1][-1]) >= 4096
        src = Guarded(recs.size, torch.uint8, data=recs)
        cap = cwire_bytes_max(8193 * 2, 1)
        off, pos, out = Guarded(2, torch.int32), Guarded(2, torch.int64), Guarded(cap)
        xs, df = Guarded(8193, torch.int32), Guarded(8193, torch.uint8)
        torch.cuda.synchronize()
        row = np.array([[0, 0, w, 1, 0, 0], [0, 0, w, 1, 40, 0]], np.int32)
        both = np.array(place, np.int32)
        for pl, cw, ch in ((row, 2731, 1), (both, 66, 42), (both, 65, 43)):
            args = (core._h, src.ptr, counts.ctypes.data, escapes.ctypes.data, S, T, pl.ctypes.data, cw, ch)
            assert L.mi355_cwire_mosaic_cwire_batch(*args, off.ptr, pos.ptr, out.ptr, cap) == lib.ERR_INVALID
            assert L.mi355_cwire_mosaic_batch(*args, off.ptr, xs.ptr, df.ptr, 8193) == lib.ERR_INVALID
        core.synchronize()
        for g in (off, pos, out, xs, df):
            g.get(written=0)


# ---- 10. malformed content -------------------------------------------------------------------------------------------------
def test_malformed_record_of_one_camera():
    """Camera 1's second record is damaged under its header: more 255 codes than it has escapes (an escape ranked past e), and
    an escape value that decodes far past N.  The guards stay intact, the output is one canonical record of the canvas, and the
    crops of the output to the OTHER cameras' destinations are what those cameras' records give."""
    w, h, S, T = 64, 48, 4, 2
    n = 3 * w * h
    rng = np.random.default_rng(11)
    segs = [(np.sort(rng.choice(n, 1500, replace=False)), rng.integers(1, 256, 1500)) for _ in range(S * T)]
    b = 1 * T + 1
    x = np.sort(np.concatenate([300 + rng.choice(1700, 250, replace=False), 3000 + rng.choice(2000, 250, replace=False),
                                6000 + rng.choice(3000, 200, replace=False)]))
    segs[b] = (x, rng.integers(1, 256, x.size))
    recs, _ = spec.encode(*packed(segs))
    counts, escapes = spec.headers(recs, S * T)
    place, cw, ch = grid_2x2(w, h)
    pos = np.cumsum([0] + [spec.frame_bytes(a, b_) for a, b_ in zip(counts, escapes)])
    bad = recs.copy()
    nb, eb, at = int(counts[b]), int(escapes[b]), int(pos[b])
    assert nb == 700 and eb == 3
    code = bad[at + 8:at + 8 + nb]
    code[100:140] = 255                                              # 40 escape codes more than the header's e
    esc = bad[at + 8 + spec.pad4(nb):at + 8 + spec.pad4(nb) + 4 * eb].view("<u4")
    esc[0] = 0xFFFFFF00                                              # decodes past N (and the running index wraps)
    esc[1] = 5 * n                                                   # decodes past N
    with CUDACore(w, h, max_batch=S * T) as core:
        off, fp, out = run_compact(core, bad, (counts, escapes), S, T, place, cw, ch)
        made = out[:int(fp[1])]
        assert (out[int(fp[1]):] == 0x5C).all()
        c2, e2 = spec.headers(made, 1)
        assert int(off[0]) == 0 and int(off[1]) == int(c2[0]) and int(fp[1]) == spec.frame_bytes(c2[0], e2[0])
        v = cwire_check_host(made, c2, e2, 3 * cw * ch)
        assert v[0][0] == 0, v
        aoff, axs, adf = run_arrays(core, bad, (counts, escapes), S, T, place, cw, ch)
        doff, dxs, ddf = spec.decode(made, 1)
        tot = int(doff[1])
        assert np.array_equal(aoff, doff) and np.array_equal(axs[:tot], dxs) and np.array_equal(adf[:tot], ddf)
        for s in (0, 2, 3):
            sx, sy, rw, rh, dx, dy = place[s]
            back = crop_spec.reference(made, 1, 1, cw, ch, [(dx, dy, rw, rh)])
            direct = crop_spec.reference(stream_slice(recs, counts, escapes, s, T), 1, T, w, h, [(sx, sy, rw, rh)])
            assert np.array_equal(back[3], direct[3]), s


# ---- 11. ordering on one core ----------------------------------------------------------------------------------------------
def test_behind_the_diff_on_one_core():
    """mi355_diff_multi_stream_cwire_batch, then the mosaic of what it writes, with no synchronisation between: the headers are
    known from a rehearsal of the same frames and states (test_cwire_coalesce_gpu.burst)."""
    w, h, S, T = 64, 48, 4, 2
    n, B = 3 * w * h, S * T
    bases, recs, counts, escapes, after, frames = burst(w, h, S, T)
    place, cw, ch = grid_2x2(w, h)
    want = mosaic_spec.reference(recs, S, T, w, h, place, cw, ch)
    assert int(want[0][1]) > 0
    cap_in, cap = cwire_bytes_max(n, B), cwire_bytes_max(3 * cw * ch, 1)
    srv, fr = Region(S, n).put(bases), Region(B, n).put(frames)
    doff, dpos, cwb = Guarded(B + 1, torch.int32), Guarded(B + 1, torch.int64), Guarded(cap_in)
    off, pos, out = Guarded(2, torch.int32), Guarded(2, torch.int64), Guarded(cap)
    with CUDACore(w, h, max_batch=B, threshold=20) as core:
        torch.cuda.synchronize()
        core.diff_multi_stream_cwire_batch(fr.ptr, srv.ptr, S, T, doff.ptr, dpos.ptr, cwb.ptr, cap_in, stride=fr.stride)
        core.cwire_mosaic_cwire_batch(cwb.ptr, counts, escapes, S, T, place, cw, ch, off.ptr, pos.ptr, out.ptr, cap)
        core.synchronize()
    assert np.array_equal(cwb.get()[:recs.size], recs)
    assert np.array_equal(off.get().view(np.uint32), want[0]) and np.array_equal(pos.get().view(np.uint64), want[4])
    assert np.array_equal(out.get()[:want[3].size], want[3])
    assert np.array_equal(srv.get(), after)


# ---- 12. a canvas of many tiles --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cancelling_records(w, h, S, T):
    """Records of n/40 entries; a stream's later records repeat half of the one before with the negated difference."""
    n = 3 * w * h
    rng = np.random.default_rng(77)
    segs = []
    for b in range(S * T):
        x = np.unique(rng.integers(0, n, n // 40))
        d = rng.integers(1, 256, x.size)
        if b % T:
            px, pd = segs[-1]
            cx, cd = px[::2], (256 - np.asarray(pd[::2])) % 256
            fresh = ~np.isin(x, cx)
            x, d = np.concatenate([x[fresh], cx]), np.concatenate([d[fresh], cd])
            order = np.argsort(x)
            x, d = x[order], d[order]
        segs.append((x, d))
    recs, _ = spec.encode(*packed(segs))
    return (recs,) + spec.headers(recs, S * T)


def test_medium_canvas():
    """Four 640x360 cameras in a 1280x720 canvas: 675 canvas tiles over 4 x 169 source tiles, a canvas row is 3840 bytes (a
    tile edge wanders through the rows), T = 4 with records that cancel."""
    w, h, S, T = 640, 360, 4, 4
    recs, counts, escapes = cancelling_records(w, h, S, T)
    place = [(0, 0, w, h, 0, 0), (0, 0, w, h, w, 0), (0, 0, w, h, 0, h), (0, 0, w, h, w, h)]
    with CUDACore(w, h, max_batch=S * T) as core:
        want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, place, 2 * w, 2 * h)
        assert 0 < int(want[0][1]) < int(counts.sum())


# ---- 13. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, S, T = 64, 48, 2, 2
    n, B = 3 * w * h, S * T
    cw, ch = 2 * w + 1, h + 2
    nc = 3 * cw * ch
    rng = np.random.default_rng(3)
    recs, _ = spec.encode(*packed([(np.sort(rng.choice(n, 50, replace=False)), rng.integers(1, 256, 50)) for _ in range(B)]))
    counts, escapes = spec.headers(recs, B)
    cap = cwire_bytes_max(nc, 1)
    # one buffer that holds the input in front and room behind it, for the overlap cases
    big = Guarded(recs.size + cap + 64, torch.uint8)
    big.t[:recs.size].copy_(torch.from_numpy(recs).to(DEV))
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, pos, out = Guarded(2, torch.int32), Guarded(2, torch.int64), Guarded(cap)
    xs, df = Guarded(nc, torch.int32), Guarded(nc, torch.uint8)
    L = lib.load()
    c, e = counts.ctypes.data, escapes.ctypes.data
    good = np.array([[8, 4, 40, 30, 0, 0], [0, 0, w, h, w + 1, 2]], np.int32)
    p = good.ctypes.data
    inside = big.ptr + recs.size - 8
    inside -= inside % 8
    with CUDACore(w, h, max_batch=B) as core:
        H = core._h
        torch.cuda.synchronize()

        def compact(core_=H, src_=src.ptr, c_=c, e_=e, S_=S, T_=T, p_=p, cw_=cw, ch_=ch, off_=off.ptr, pos_=pos.ptr, out_=out.ptr,
                    cap_=cap):
            return L.mi355_cwire_mosaic_cwire_batch(core_, src_, c_, e_, S_, T_, p_, cw_, ch_, off_, pos_, out_, cap_)

        def arrays(core_=H, src_=src.ptr, c_=c, e_=e, S_=S, T_=T, p_=p, cw_=cw, ch_=ch, off_=off.ptr, xs_=xs.ptr, df_=df.ptr,
                   cap_=nc):
            return L.mi355_cwire_mosaic_batch(core_, src_, c_, e_, S_, T_, p_, cw_, ch_, off_, xs_, df_, cap_)

        more_e = (escapes + counts + 1).astype(np.uint32)
        more_n = np.full(B, n + 1, np.uint32)
        zero_e = np.zeros(B, np.uint32)
        big_i = 2 ** 31 - 1
        bad_places = [np.array([[8, 4, 40, 30, 0, 0], pl], np.int32) for pl in (
            [-1, 0, 4, 4, 0, 0], [0, -1, 4, 4, 0, 0], [0, 0, -1, 4, 0, 0], [0, 0, 4, -1, 0, 0], [0, 0, 4, 4, -1, 0],
            [0, 0, 4, 4, 0, -1],                                                              # a negative member
            [w - 3, 0, 4, 4, 0, 0], [0, h - 3, 4, 4, 0, 0], [w, 0, 1, 1, 0, 0], [0, 0, w + 1, h, 0, 0],   # source past the frame
            [0, 0, 4, 4, cw - 3, 0], [0, 0, 4, 4, 0, ch - 3], [0, 0, 1, 1, cw, 0], [0, 0, 1, 1, 0, ch],   # destination past the canvas
            [1, 0, big_i, 1, 0, 0], [0, 1, 1, big_i, 0, 0], [big_i, 0, big_i, 1, 0, 0],      # sums that wrap in 32 bits
            [0, 0, 1, 1, big_i, 0], [0, 0, 2, 2, big_i, big_i], [0, 0, 1, 2, 0, big_i])]
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
            arrays(src_=big.ptr, off_=big.ptr - 4), arrays(src_=big.ptr, df_=big.ptr - 3, cap_=4),
            # the call's own
            compact(p_=None), arrays(p_=None),
            compact(cw_=0), compact(ch_=0), arrays(cw_=-1), arrays(ch_=-5),
            compact(cw_=26755, ch_=26755), arrays(cw_=26755, ch_=26755),          # 3 * 26755^2 = 2^31 + 6427
            compact(cw_=big_i, ch_=big_i), arrays(cw_=big_i, ch_=1),
            compact(cw_=cw, ch_=4 * ch), arrays(cw_=4096, ch_=5),                   # more tiles than max_batch frames hold (12)
        ]
        cases += [compact(p_=b.ctypes.data) for b in bad_places] + [arrays(p_=b.ctypes.data) for b in bad_places]
        assert all(rc == lib.ERR_INVALID for rc in cases), cases
        core.synchronize()
        for g in (off, pos, out, xs, df):
            g.get(written=0)
        assert np.array_equal(src.get(), recs)
        h_big = big.get()
        assert np.array_equal(h_big[:recs.size], recs) and (h_big[recs.size:] == 0x5C).all()
        # nstreams * nframes == 0: offsets[0] = 0 (and frame_pos[0] = 0) and nothing else, with or without placements
        assert compact(S_=0, p_=None) == lib.OK and arrays(T_=0) == lib.OK
        core.synchronize()
        assert off.get(written=1)[0] == 0 and pos.get(written=1)[0] == 0
        for g in (out, xs, df):
            g.get(written=0)
        # ... and the calls above left the core in order: the burst is placed
        assert compact() == lib.OK
        core.synchronize()
        want = mosaic_spec.reference(recs, S, T, w, h, good, cw, ch)
        assert np.array_equal(out.get()[:want[3].size], want[3])

"""-m gpu: mi355_activity_batch / mi355_cwire_activity_batch -- per stream, a grid of counts of the entries of its records per
cell and eight summary words (include/mi355diff.h, "Where a camera moves").  All results are integers and every comparison is
exact.  The oracle is numpy on the entries: cells from np.bincount, box, active cells, peak and peak index (the lowest among
equals) from numpy; the compact records are built with cwire_spec.encode or by the library's own diff call and decoded with
cwire_spec.decode.  Inputs and outputs live in guarded buffers (gpu_util) that start as a non-zero pattern; the guards are
checked after every call."""
import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import activity_cells, lib, synth
from gpu_util import CUDACore, Guarded, Region

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
EMPTY = np.array([0, MAX, MAX, 0, 0, 0, 0, 0], np.uint32)
BIG = 5000   # a cell larger than every frame here


# ---- inputs and oracle ------------------------------------------------------------------------------------------------------
def packed(segments):
    """[xs per record] -> (offsets uint32[B + 1], xs int32, diff uint8: all 1, the grids do not look at it)."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in segments])]).astype(np.uint32)
    xs = np.concatenate([np.asarray(x, np.int64) for x in segments] + [np.empty(0, np.int64)]).astype(np.int32)
    return off, xs, np.ones(xs.size, np.uint8)


def random_segments(rng, n, B, most=None):
    """B records: empty ones, single entries, sparse and dense ones, ascending distinct indices."""
    most = n if most is None else min(most, n)
    out = []
    for b in range(B):
        k = (0, 1, most // 7, most, most // 2, 2)[b % 6] if b else most // 3
        out.append(np.sort(rng.choice(n, min(max(k, 0), n), replace=False)))
    return out


def oracle(w, h, cw, ch, min_count, S, T, off, xs, onto=None):
    """(cells [S][cells], summary [S][8]) of the entries, added onto `onto` = (cells, summary) when given."""
    ncells, gw, _ = activity_cells(w, h, cw, ch)
    n = 3 * w * h
    cells = np.zeros((S, ncells), np.uint32) if onto is None else onto[0].copy()
    summ = np.tile(EMPTY, (S, 1)) if onto is None else onto[1].copy()
    for s in range(S):
        x = xs[int(off[s * T]):int(off[(s + 1) * T])].view(np.uint32).astype(np.int64)
        x = x[x < n]
        p = x // 3
        px, py = p % w, p // w
        cells[s] += np.bincount((py // ch) * gw + px // cw, minlength=ncells).astype(np.uint32)
        if x.size:
            summ[s, 0] += np.uint32(x.size)
            summ[s, 1], summ[s, 2] = min(summ[s, 1], px.min()), min(summ[s, 2], py.min())
            summ[s, 3], summ[s, 4] = max(summ[s, 3], px.max()), max(summ[s, 4], py.max())
        peak = int(cells[s].max()) if ncells else 0
        summ[s, 5], summ[s, 6] = int((cells[s] >= min_count).sum()), peak
        summ[s, 7] = int(np.argmax(cells[s])) if peak else 0      # (argmax: the first of equals)
    return cells, summ


class Outputs:
    """Guarded d_cells / d_summary for `rows` streams; they hold the pattern, or `start` = (cells, summary)."""

    def __init__(self, rows, ncells, start=None):
        self.rows, self.ncells = rows, ncells
        self.cells = Guarded(rows * ncells, torch.int32, data=None if start is None else start[0].reshape(-1).view(np.int32))
        self.summ = Guarded(rows * 8, torch.int32, data=None if start is None else start[1].reshape(-1).view(np.int32))

    def get(self, S=None):
        """(cells [S][ncells], summary [S][8]); the rows behind the first S must still hold the pattern."""
        S = self.rows if S is None else S
        c = self.cells.get(written=S * self.ncells).view(np.uint32)[:S * self.ncells].reshape(S, self.ncells).copy()
        m = self.summ.get(written=S * 8).view(np.uint32)[:S * 8].reshape(S, 8).copy()
        return c, m

    def untouched(self):
        self.cells.get(written=0)
        self.summ.get(written=0)


def run_arrays(core, geom, S, T, off, xs, out, accumulate=False):
    cw, ch, mc = geom
    g = [Guarded(off.size, torch.int32, data=off.view(np.int32)), Guarded(xs.size, torch.int32, data=xs)]
    torch.cuda.synchronize()
    core.activity_batch(g[0].ptr, g[1].ptr, S, T, cw, ch, out.cells.ptr, out.summ.ptr, min_count=mc, accumulate=accumulate)
    core.synchronize()
    assert np.array_equal(g[0].get().view(np.uint32), off) and np.array_equal(g[1].get(), xs)


def run_compact(core, geom, S, T, recs, hdr, out, accumulate=False):
    cw, ch, mc = geom
    g = Guarded(recs.size, data=recs)
    torch.cuda.synchronize()
    core.cwire_activity_batch(g.ptr, hdr[0], hdr[1], S, T, cw, ch, out.cells.ptr, out.summ.ptr, min_count=mc, accumulate=accumulate)
    core.synchronize()
    assert np.array_equal(g.get(), recs)


def both_forms(core, w, h, geom, S, T, segments, spare=2):
    """Both forms on the same entries, over buffers that hold the pattern and have `spare` streams' worth of room behind the
    S that are written: identical outputs, equal to the oracle; returns them."""
    off, xs, df = packed(segments)
    recs, _ = spec.encode(off, xs, df)
    hdr = spec.headers(recs, S * T)
    ncells = activity_cells(w, h, geom[0], geom[1])[0]
    want = oracle(w, h, geom[0], geom[1], geom[2], S, T, off, xs)
    got = []
    for form in ("arrays", "compact"):
        out = Outputs(S + spare, ncells)
        if form == "arrays":
            run_arrays(core, geom, S, T, off, xs, out)
        else:
            run_compact(core, geom, S, T, recs, hdr, out)
        got.append(out.get(S))
        assert np.array_equal(got[-1][1], want[1]), (form, got[-1][1], want[1])
        assert np.array_equal(got[-1][0], want[0]), form
    assert all(np.array_equal(a, b) for a, b in zip(*got))
    return want


# ---- 1. geometries x cells --------------------------------------------------------------------------------------------------
GEOMETRIES = [(15, 1), (37, 11), (50, 37), (1400, 3)]
CELLS = [(1, 1), (16, 16), (7, 5), (BIG, BIG)]


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "cell%dx%d" % c)
@pytest.mark.parametrize("wh", GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_geometries_and_cells(wh, cell):
    """15x1: one partial tile, N no multiple of 4; 37x11: odd width, several rows in a tile; 50x37: the tile boundary at byte
    4096 inside pixel 1365, the second tile partial; 1400x3: a row longer than a tile.  S = 3 streams of T = 2 records."""
    w, h = wh
    n, S, T = 3 * w * h, 3, 2
    segments = random_segments(np.random.default_rng(w + h + cell[0]), n, S * T)
    if n > 4096:   # both sides of the boundary, in both records of stream 0: pixel 1365 is bytes 4095 (tile 0), 4096, 4097 (tile 1)
        segments[0] = np.union1d(segments[0], [4094, 4095, 4096, 4097])
        segments[1] = np.array([4095, 4096, n - 1])
    with CUDACore(w, h, max_batch=S * T + 1) as core:
        for min_count in (1, 3):
            cells, summ = both_forms(core, w, h, cell + (min_count,), S, T, segments)
        assert summ[0, 0] == len(segments[0]) + len(segments[1]) and cells.sum() == sum(len(x) for x in segments)
        if cell == (BIG, BIG):
            assert cells.shape == (S, 1) and (summ[:, 7] == 0).all()


def test_dense_record_and_single_entries():
    """64x48 with every byte changed: n = 9216, three directory chunks, no escapes, every cell 3 * its pixels; beside it a
    stream with one entry and a stream with the frame's last byte only."""
    w, h = 64, 48
    n = 3 * w * h
    segments = [np.arange(n), [5000], [n - 1]]
    with CUDACore(w, h, max_batch=4) as core:
        cells, summ = both_forms(core, w, h, (16, 16, 1), 3, 1, segments)
        assert (cells[0] == 3 * 256).all() and list(summ[0]) == [n, 0, 0, 63, 47, 12, 768, 0]
        assert list(summ[2]) == [1, 63, 47, 63, 47, 1, 1, 11]
        both_forms(core, w, h, (7, 5, 3), 3, 1, segments)


def test_isolated_entries_with_escapes():
    """256x64 (12 tiles) with entries more than 4200 bytes apart: every gap is escaped, there are tiles nothing lands in and
    one entry per touched tile; stream 1 starts in the last tile."""
    w, h = 256, 64
    n = 3 * w * h
    segments = [100 + 4200 * np.arange(n // 4200), 37 + 8300 * np.arange(n // 8300), [n - 2], []]
    off, xs, df = packed(segments)
    _, escapes = spec.headers(spec.encode(off, xs, df)[0], 4)
    assert escapes[0] == len(segments[0]) - 1 > 5
    with CUDACore(w, h, max_batch=4) as core:
        for cell in ((16, 16), (1, 1), (7, 5)):
            _, summ = both_forms(core, w, h, cell + (1,), 2, 2, segments)
        assert summ[0, 0] == len(segments[0]) + len(segments[1]) and summ[1, 0] == 1


# ---- 2. streams and frames --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T,room", [(1, 1, 1), (3, 1, 1), (1, 3, 1), (3, 3, 0), (130, 1, 3), (130, 3, 0)])
def test_streams_and_frames(S, T, room):
    """15x1.  130 streams are past the 128 records of a table launch; room == 0: nstreams*nframes == max_batch."""
    w, h = 15, 1
    segments = random_segments(np.random.default_rng(S * 7 + T), 3 * w * h, S * T)
    with CUDACore(w, h, max_batch=S * T + room) as core:
        both_forms(core, w, h, (4, 1, 2), S, T, segments)
        both_forms(core, w, h, (1, 1, 1), S, T, segments)


def test_more_records_per_stream_than_one_ballot_pass():
    """T = 70 at 50x37: a wave looks at 64 records of its stream per pass; stream 1 has no entry before record 66."""
    w, h, S, T = 50, 37, 2, 70
    n = 3 * w * h
    rng = np.random.default_rng(70)
    segments = [np.sort(rng.choice(n, int(rng.integers(0, 40)), replace=False)) for _ in range(S * T)]
    for t in range(66):
        segments[T + t] = []
    with CUDACore(w, h, max_batch=S * T) as core:
        both_forms(core, w, h, (16, 16, 3), S, T, segments)


def test_empty_records():
    """Records with n = 0 among others, and a call in which every record is empty: empty summaries, zero grids."""
    w, h, S, T = 37, 11, 3, 2
    n = 3 * w * h
    with CUDACore(w, h, max_batch=S * T) as core:
        cells, summ = both_forms(core, w, h, (7, 5, 1), S, T, [[], [3, 4, 5], [], [], [n - 1], []])
        assert np.array_equal(summ[1], EMPTY) and not cells[1].any() and summ[0, 0] == 3 and summ[2, 0] == 1
        cells, summ = both_forms(core, w, h, (7, 5, 1), S, T, [[]] * (S * T))
        assert np.array_equal(summ, np.tile(EMPTY, (S, 1))) and not cells.any()


def test_indices_past_the_frame_contribute_nothing():
    """Arrays form: d_xs is read as uint32, so N, N + 1, a negative index and 2^31 - 1 are all past the frame."""
    w, h, S = 37, 11, 2
    n = 3 * w * h
    off = np.array([0, 6, 9], np.uint32)
    xs = np.array([0, 7, n, n + 1, -1, 2 ** 31 - 1, -5, n - 1, n], np.int32)
    want = oracle(w, h, 16, 16, 1, S, 1, off, xs)
    assert list(want[1][:, 0]) == [2, 1]
    with CUDACore(w, h, max_batch=S) as core:
        out = Outputs(S + 1, 3)
        run_arrays(core, (16, 16, 1), S, 1, off, xs, out)
        got = out.get(S)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 3. straight behind the diff, no synchronisation ------------------------------------------------------------------------
def test_behind_diff_multi_batch_without_synchronisation():
    """Webcam-like input, 64x48, S = 3: mi355_diff_multi_batch, then mi355_activity_batch on its offsets and indices on the
    same core with nothing in between; the compact form on the same entries gives identical outputs."""
    w, h, S = 64, 48, 3
    n = 3 * w * h
    streams = [synth.webcam_stream(1, w, h, seed=1 + 7 * s) for s in range(S)]
    pre, frames = np.stack([b for b, _ in streams]), np.stack([f[0] for _, f in streams])
    st, fr = Region(S, n).put(pre), Region(S, n).put(frames)
    off, xs, df = Guarded(S + 1, torch.int32), Guarded(S * n, torch.int32), Guarded(S * n)
    ncells = activity_cells(w, h, 16, 16)[0]
    out = Outputs(S + 1, ncells)
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        core.diff_multi_batch(fr.ptr, st.ptr, S, off.ptr, xs.ptr, df.ptr, S * n, stride=fr.stride)
        core.activity_batch(off.ptr, xs.ptr, S, 1, 16, 16, out.cells.ptr, out.summ.ptr, min_count=3)
        core.synchronize()
        o = off.get().view(np.uint32).copy()
        x, d = xs.get()[:int(o[S])].copy(), df.get()[:int(o[S])].copy()
        assert (np.diff(o.astype(np.int64)) > 0).all()
        want = oracle(w, h, 16, 16, 3, S, 1, o, x)
        got = out.get(S)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
        recs, _ = spec.encode(o, x, d)
        out2 = Outputs(S + 1, ncells)
        run_compact(core, (16, 16, 3), S, 1, recs, spec.headers(recs, S), out2)
        got2 = out2.get(S)
    assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[1], got[1])


# ---- 4. the peak's tie rule -------------------------------------------------------------------------------------------------
def test_a_tie_for_the_peak_picks_the_lowest_cell():
    """50x37, 16x16 cells (4 x 3): cells 9 and 2 both count 4, cell 0 counts 3 -- in two records, the later cell first; with
    min_count 4 only the two are active.  Stream 1: the tie is between the first and the last cell."""
    w, h = 50, 37

    def byte(px, py, c=0):
        return 3 * (py * w + px) + c

    a = sorted([byte(20, 35), byte(20, 35, 1), byte(21, 36), byte(31, 32, 2)])            # cell 2 * 4 + 1 = 9: 4 entries
    b = sorted([byte(33, 0), byte(40, 15), byte(47, 3, 1), byte(47, 3, 2),                # cell 2: 4 entries
                byte(0, 0), byte(15, 15, 2), byte(7, 7, 1)])                              # cell 0: 3 entries
    c = sorted([byte(0, 0), byte(1, 1), byte(49, 36), byte(48, 36, 2)])                   # cells 0 and 11: 2 each
    with CUDACore(w, h, max_batch=4) as core:
        cells, summ = both_forms(core, w, h, (16, 16, 4), 2, 2, [a, b, c, []])
    assert cells[0, 9] == cells[0, 2] == 4 and cells[0, 0] == 3
    assert list(summ[0]) == [11, 0, 0, 47, 36, 2, 4, 2]
    assert list(summ[1]) == [4, 0, 0, 49, 36, 0, 2, 0]


# ---- 5. accumulate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", [(37, 11), (50, 37)], ids=lambda g: "%dx%d" % g)
def test_a_burst_equals_its_ticks_accumulated(wh):
    """T = 3 in one call == three accumulating single-tick calls on the same records, begun on the empty values == the oracle;
    a fourth accumulating call of the whole burst doubles the counts and keeps the box."""
    w, h = wh
    n, S, T = 3 * w * h, 3, 3
    geom = (7, 5, 3)
    ncells = activity_cells(w, h, 7, 5)[0]
    segments = random_segments(np.random.default_rng(w), n, S * T, most=600)
    off, xs, df = packed(segments)
    want = oracle(w, h, 7, 5, 3, S, T, off, xs)
    empty = (np.zeros((S + 1, ncells), np.uint32), np.tile(EMPTY, (S + 1, 1)))
    with CUDACore(w, h, max_batch=S * T) as core:
        burst = both_forms(core, w, h, geom, S, T, segments)
        assert np.array_equal(burst[0], want[0]) and np.array_equal(burst[1], want[1])
        for form in ("arrays", "compact"):
            out = Outputs(S + 1, ncells, start=empty)
            for t in range(T):
                o, x, d = packed([segments[s * T + t] for s in range(S)])
                if form == "arrays":
                    run_arrays(core, geom, S, 1, o, x, out, accumulate=True)
                else:
                    recs, _ = spec.encode(o, x, d)
                    run_compact(core, geom, S, 1, recs, spec.headers(recs, S), out, accumulate=True)
            got = out.cells.get().view(np.uint32).reshape(S + 1, ncells), out.summ.get().view(np.uint32).reshape(S + 1, 8)
            assert np.array_equal(got[0][:S], want[0]) and np.array_equal(got[1][:S], want[1]), form
            assert not got[0][S].any() and np.array_equal(got[1][S], EMPTY)            # the stream behind: as it was
            twice = oracle(w, h, 7, 5, 3, S, T, off, xs, onto=want)
            if form == "arrays":
                run_arrays(core, geom, S, T, off, xs, out, accumulate=True)
            else:
                recs, _ = spec.encode(off, xs, df)
                run_compact(core, geom, S, T, recs, spec.headers(recs, S * T), out, accumulate=True)
            got = out.get(S + 1)
            assert np.array_equal(got[0][:S], twice[0]) and np.array_equal(got[1][:S], twice[1]), form
            assert np.array_equal(twice[0], 2 * want[0]) and np.array_equal(twice[1][:, 1:5], want[1][:, 1:5])


def test_counts_wrap_around():
    """accumulate onto counts near 2^32: counts and word 0 add with uint32 wrap-around, words 5 to 7 follow the grid."""
    w, h, S = 15, 1, 1
    start = (np.array([[MAX, 5, 0, MAX - 1]], np.uint32), np.array([[MAX - 2, 3, 0, 9, 0, 0, 0, 0]], np.uint32))
    off, xs, df = packed([[0, 1, 2, 3, 40, 41, 44]])                   # pixels 0 (3), 1 (1), 13 (2), 14 (1): cells 0 and 3
    want = oracle(w, h, 4, 1, 2, S, 1, off, xs, onto=start)
    assert list(want[0][0]) == [3, 5, 0, 1] and list(want[1][0]) == [4, 0, 0, 14, 0, 2, 5, 1]
    recs, _ = spec.encode(off, xs, df)
    with CUDACore(w, h, max_batch=1) as core:
        for form in ("arrays", "compact"):
            out = Outputs(S, 4, start=start)
            if form == "arrays":
                run_arrays(core, (4, 1, 2), S, 1, off, xs, out, accumulate=True)
            else:
                run_compact(core, (4, 1, 2), S, 1, recs, spec.headers(recs, 1), out, accumulate=True)
            got = out.get()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), form


# ---- 6. malformed content ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", [(37, 11), (50, 37)], ids=lambda g: "%dx%d" % g)
def test_malformed_content_stays_in_bounds(wh):
    """Stream 1 of 3 is a hand-made record under a consistent header {n = 8, e = 1}: three well-formed entries, then an escaped
    gap that runs the index past N, then an escape code ranked past e among small gaps.  The other two streams are exact,
    nothing outside the outputs changes, and stream 1 counts at most its well-formed prefix."""
    w, h = wh
    n, S = 3 * w * h, 3
    good = [np.array([1, 2, n - 1]), np.array([0]), np.arange(0, n, 7)]
    off, xs, df = packed(good)
    wrecs, wpos = spec.encode(off, xs, df)
    counts, escapes = (a.copy() for a in spec.headers(wrecs, S))
    code = np.array([10, 20, 30, 255, 5, 255, 7, 9], np.uint8)          # entries 10, 31, 62 | + n + 1 | ... | rank 1 >= e | ...
    bad = np.concatenate([np.array([8, 1], "<u4").view(np.uint8), code, np.array([n], "<u4").view(np.uint8), np.full(8, 9, np.uint8)])
    assert bad.size == spec.frame_bytes(8, 1)
    recs = np.concatenate([wrecs[:int(wpos[1])], bad, wrecs[int(wpos[2]):]])
    counts[1], escapes[1] = 8, 1
    want = oracle(w, h, 7, 5, 1, S, 1, off, xs)
    ncells = activity_cells(w, h, 7, 5)[0]
    with CUDACore(w, h, max_batch=S) as core:
        out = Outputs(S + 1, ncells)
        run_compact(core, (7, 5, 1), S, 1, recs, (counts, escapes), out)
        cells, summ = out.get(S)
    for s in (0, 2):
        assert np.array_equal(cells[s], want[0][s]) and np.array_equal(summ[s], want[1][s])
    assert summ[1, 0] <= 3


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, S, T = 37, 11, 2, 2
    n, B = 3 * w * h, S * T
    ncells = activity_cells(w, h, 16, 16)[0]
    segments = random_segments(np.random.default_rng(3), n, B, most=200)
    off, xs, df = packed(segments)
    recs, _ = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, B)
    g = [Guarded(off.size, torch.int32, data=off.view(np.int32)), Guarded(xs.size, torch.int32, data=xs), Guarded(recs.size, data=recs)]
    o, x, cw = (q.ptr for q in g)
    # ONE guarded buffer of the pattern: [records | cells | summary], for the overlap cases
    assert recs.size % 4 == 0
    row = Guarded(recs.size + 4 * S * ncells + 32 * S)
    rp = row.ptr
    cp, sp = rp + recs.size, rp + recs.size + 4 * S * ncells
    out = Outputs(S, ncells)
    oc, os_ = out.cells.ptr, out.summ.ptr
    u32 = lambda a: a.ctypes.data
    big, esc_gt = counts.copy(), escapes.copy()
    big[1] = n + 1
    esc_gt[2] = counts[2] + 1
    z = np.zeros(B, np.uint32)
    c_, e_ = u32(counts), u32(escapes)
    with CUDACore(w, h, max_batch=B) as core:
        L, H = core._lib, core._h
        A, CW = L.mi355_activity_batch, L.mi355_cwire_activity_batch
        geo, tail = (16, 16, 1, 0), (oc, os_)
        cases = [
            (A, (None, o, x, S, T) + geo + tail), (CW, (None, cw, c_, e_, S, T) + geo + tail),
            (A, (H, o, x, -1, T) + geo + tail), (A, (H, o, x, S, -1) + geo + tail),
            (CW, (H, cw, c_, e_, -1, T) + geo + tail), (CW, (H, cw, c_, e_, S, -1) + geo + tail),
            # S*T = max_batch + 1, and a product that only fits 64 bits
            (A, (H, o, x, 1, B + 1) + geo + tail), (CW, (H, cw, c_, e_, B + 1, 1) + geo + tail),
            (A, (H, o, x, 1 << 16, 1 << 16) + geo + tail), (CW, (H, cw, c_, e_, 1 << 16, 1 << 16) + geo + tail),
            (A, (H, o, x, S, T, 0, 16, 1, 0) + tail), (A, (H, o, x, S, T, 16, 0, 1, 0) + tail), (A, (H, o, x, S, T, -1, 16, 1, 0) + tail),
            (A, (H, o, x, S, T, 16, 16, 0, 0) + tail),
            (CW, (H, cw, c_, e_, S, T, 0, 16, 1, 0) + tail), (CW, (H, cw, c_, e_, S, T, 16, -2, 1, 0) + tail),
            (CW, (H, cw, c_, e_, S, T, 16, 16, 0, 0) + tail),
            (A, (H, None, x, S, T) + geo + tail), (A, (H, o, None, S, T) + geo + tail), (A, (H, o, x, S, T) + geo + (None, os_)),
            (A, (H, o, x, S, T) + geo + (oc, None)),
            (CW, (H, None, c_, e_, S, T) + geo + tail), (CW, (H, cw, None, e_, S, T) + geo + tail),
            (CW, (H, cw, c_, None, S, T) + geo + tail), (CW, (H, cw, c_, e_, S, T) + geo + (None, os_)),
            (CW, (H, cw, c_, e_, S, T) + geo + (oc, None)),
            (CW, (H, cw, c_, u32(esc_gt), S, T) + geo + tail),                                   # more escapes than entries
            (CW, (H, cw, u32(big), u32(z), S, T) + geo + tail),                                  # more entries than frame bytes
            (CW, (H, cw + 1, c_, e_, S, T) + geo + tail), (CW, (H, cw + 2, c_, e_, S, T) + geo + tail),
            (CW, (H, cw, c_, e_, S, T) + geo + (oc + 2, os_)), (CW, (H, cw, c_, e_, S, T) + geo + (oc, os_ + 1)),
            (A, (H, o + 2, x, S, T) + geo + tail), (A, (H, o, x + 1, S, T) + geo + tail),
            (A, (H, o, x, S, T) + geo + (oc + 1, os_)), (A, (H, o, x, S, T) + geo + (oc, os_ + 2)),
        ]
        # the input span against either output region: at its first word, across its end, ending one word into it
        for at in (cp, cp + 4 * S * ncells - 4, cp - recs.size + 4):
            cases.append((CW, (H, at, c_, e_, S, T) + geo + (cp, os_)))
        for at in (sp, sp + 32 * S - 4, sp - recs.size + 4):
            cases.append((CW, (H, at, c_, e_, S, T) + geo + (oc, sp)))
        torch.cuda.synchronize()
        for i, (fn, args) in enumerate(cases):
            assert fn(*args) == lib.ERR_INVALID, i
            assert L.mi355_last_error(), i
        core.synchronize()
        out.untouched()
        row.get(written=0)
        # S*T == 0 in both ways: OK, with and without pointers, and nothing is written
        for S0, T0 in ((0, T), (S, 0), (0, 0)):
            assert A(H, o, x, S0, T0, 16, 16, 1, 0, oc, os_) == lib.OK and A(H, None, None, S0, T0, 16, 16, 1, 0, None, None) == lib.OK
            assert CW(H, cw, c_, e_, S0, T0, 16, 16, 1, 0, oc, os_) == lib.OK
            assert CW(H, None, None, None, S0, T0, 16, 16, 1, 0, None, None) == lib.OK
        core.synchronize()
        out.untouched()
        # records that END where the grids begin overlap nothing: taken
        torch.cuda.synchronize()
        row.t[:recs.size].copy_(torch.from_numpy(recs))
        torch.cuda.synchronize()
        assert CW(H, rp, c_, e_, S, T, 16, 16, 1, 0, cp, sp) == lib.OK
        core.synchronize()
    for q in g:
        q.get()
    want = oracle(w, h, 16, 16, 1, S, T, off, xs)
    body = row.get()
    assert np.array_equal(body[:recs.size], recs)
    assert np.array_equal(body[recs.size:recs.size + 4 * S * ncells].view(np.uint32).reshape(S, ncells), want[0])
    assert np.array_equal(body[recs.size + 4 * S * ncells:].view(np.uint32).reshape(S, 8), want[1])

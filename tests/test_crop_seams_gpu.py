"""-m gpu: mi355_cwire_crop_batch / _cwire_batch past the fixed counts at which their kernels and the host loop start another
round (csrc/stream_ops.hip), and the crop call next to the other calls that share its scratch:
    k_crop_facts    128 rectangles per launch (kCropStreams), h.first the launch's first stream: 127, 128, 129 and 257 streams of
                    one and of three tiles, a rectangle per stream that differs from its neighbours' and from the one 128 before
    k_cwc_place     1024 streams per round: 1024, 1025 and 2049 streams of 15x1 with a rectangle per stream, and capacities that
                    end inside the second round
    k_cwc_scan      256 tiles per round, fed facts in MAPPED indices and all-zero facts outside the rectangle's rows: 1024x342
                    (257 tiles) and 1024x683 (513 tiles); mapped gaps of 254, 255, 256 across each round seam, rectangles whose
                    rows miss whole rounds, a column of one pixel, dense tiles cut in mid-row
    crop_tile       three and more rows in a lane's 64 bytes (rows of 3, 6, 15 and 30 bytes), tiles inside the rectangle's rows
    CropMap         and outside its columns (rows of 9000 and 8193 bytes)
    c->cwb_hist     the crop call's six words per stream live in the budget call's rows, its facts in the directory's chunk
    c->cwa_chunk    table: every ordered pair of {crop compact, crop arrays, coalesce, budget, check, activity, touched tiles,
                    refresh} queued on one core with nothing in between

The reference is crop_spec.reference (numpy) and, for the other calls of the last part, the numpy statements the suite already
has; every comparison is np.array_equal.  Every buffer the GPU sees is guarded (gpu_util.Guarded / Region) and starts as a
non-zero pattern.  The inputs are made once, read-only, by the builders below; each builder asserts from the reference alone that
its input reaches the seam it is named for, and test_crop_seams_host.py runs every builder without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import crop_spec
import cwire_spec as spec
import resync_spec as rs
import wall_spec as ws
from cudavideostream_amd import CWIRE_BAD_CODES, activity_cells, cwire_bytes_max, lib
from gpu_util import CUDACore, Guarded, Region
from test_activity_gpu import Outputs, oracle
from test_cwire_check_host import batch_of, ref_verdict
from test_cwire_coalesce_gpu import packed
from test_cwire_coalesce_gpu import reference as coalesce_reference
from test_cwire_crop_gpu import check_both_forms, random_records, rectangle_sets, run_arrays, run_compact
from test_cwire_round_seams_gpu import expected as budget_expected
from test_cwire_round_seams_gpu import numpy_tick
from test_resync_gpu import Refresh, check_refresh, damaged

pytestmark = pytest.mark.gpu

KEEP = lib.CROP_KEEP_INDEX
FLAGS = (0, KEEP)
K = 4096                      # bytes of a tile
ROUND = 256 * K               # bytes of a round of k_cwc_scan
PLACE = 1024                  # streams of a round of k_cwc_place
LAUNCH = 128                  # streams of a k_crop_facts launch


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def kept_of(want, s):
    """The indices stream s keeps, from a crop_spec.reference result."""
    return want[1][int(want[0][s]):int(want[0][s + 1])].astype(np.int64)


def same_segment(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 1. more streams than one k_crop_facts launch ---------------------------------------------------------------------------
LAUNCH_FRAMES = [(40, 30), (64, 48)]                                  # 3600 bytes, one tile; 9216 bytes, three tiles
LAUNCH_COUNTS = [(127, 1), (128, 1), (129, 1), (129, 3), (257, 2)]    # (S, T)
NAMED = (0, 127, 128, 129, 256)


def launch_rects(w, h, S):
    """One rectangle per stream, a function of s: an empty one at s % 37 == 5, the full frame at s % 37 == 11, else a quarter to
    a half of the frame whose corner and size move with s."""
    out = []
    for s in range(S):
        if s % 37 == 5:
            out.append((0, 0, 0, 0))
        elif s % 37 == 11:
            out.append((0, 0, w, h))
        else:
            out.append(((5 * s) % (w // 2), (3 * s) % (h // 2), 1 + w // 4 + (7 * s) % (w // 4), 1 + h // 4 + (11 * s) % (h // 4)))
    return np.array(out, np.int32)


@functools.lru_cache(maxsize=None)
def launch_case(w, h, S, T):
    """-> (records, counts, escapes, rectangles int32[S, 4]).  Random records of a sixteenth to an eighth of the bytes each; a
    stream's later records repeat every second index of the one before with the negated difference, so that sums cancel."""
    n = 3 * w * h
    rng = np.random.default_rng(100000 * w + 1000 * S + T)
    segs = []
    for b in range(S * T):
        cnt = int(rng.integers(n // 16, n // 8))
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
    rects = launch_rects(w, h, S)
    assert -(-n // K) == (1 if w == 40 else 3)
    assert all((rects[s] != rects[s + 1]).any() for s in range(S - 1)), "no two neighbouring streams have the same rectangle"
    named = [s for s in NAMED if s < S]
    assert all((rects[a] != rects[b]).any() for a in named for b in named if a < b), "the named streams differ pairwise"
    assert any((r == (0, 0, 0, 0)).all() for r in rects) and any((r == (0, 0, w, h)).all() for r in rects)
    acc = crop_spec.sums(recs, S, T, n)
    for keep in (False, True):
        want = crop_spec.reference(recs, S, T, w, h, rects, keep_index=keep)
        assert int(want[0][S]) > 0
        assert all(kept_of(want, s).size > 0 for s in (127, 128, 129, 256) if s < S)
        true = lambda s: crop_spec.segment(acc[s], w, h, rects[s], keep)
        if S > LAUNCH:
            by128 = np.roll(rects, LAUNCH, axis=0)                   # stream 128 with stream 0's: launch 0's table again
            assert (by128[LAUNCH] == rects[0]).all()
            for s in (0, LAUNCH):
                assert not same_segment(true(s), crop_spec.segment(acc[s], w, h, by128[s], keep)), (s, "rolled by 128")
            for shift in (1, -1):                                    # h.rect[j - 1], h.rect[j + 1]
                other = np.roll(rects, shift, axis=0)[LAUNCH]
                assert not same_segment(true(LAUNCH), crop_spec.segment(acc[LAUNCH], w, h, other, keep)), "rolled by 1"
    return frozen(recs, counts, escapes, rects)


@pytest.mark.parametrize("S,T", LAUNCH_COUNTS)
@pytest.mark.parametrize("w,h", LAUNCH_FRAMES)
def test_more_streams_than_one_facts_launch(w, h, S, T):
    """127: one launch, not full; 128: one full launch and no second; 129: a second launch of one stream, h.first = 128; (129, 3):
    387 records, four k_cwa_table launches; (257, 2): three launches, the last of one stream.  At 64x48 a stream has three tiles,
    so blockIdx.x / ntiles is not blockIdx.x."""
    recs, counts, escapes, rects = launch_case(w, h, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        for flags in FLAGS:
            check_both_forms(core, recs, (counts, escapes), S, T, w, h, rects, flags)


# ---- 2. more streams than one k_cwc_place round -----------------------------------------------------------------------------
W2, H2, N2 = 15, 1, 45
PLACE_COUNTS = [1024, 1025, 2049]
PLACE_NAMED = (1023, 1024, 1025, 2048)


def place_rect(s):
    return (s % 15, 0, 1 + (7 * s) % (15 - s % 15), 1)


@functools.lru_cache(maxsize=None)
def place_case(S):
    """15x1, T = 1 -> (records, counts, escapes, rectangles, the reference for flags 0).  Record s has (7 * s) % 20 entries, 0
    to 19; the named streams 1023, 1024, 1025 and 2048 also hold the first byte of their rectangle.  A round that is one of the
    named streams alone (stream 1024 at S = 1025, stream 2048 at S = 2049) cannot also be empty: every round that holds another
    stream has one that keeps nothing."""
    rng = np.random.default_rng(S)
    rects = np.array([place_rect(s) for s in range(S)], np.int32)
    segs = []
    for s in range(S):
        x = rng.choice(N2, (7 * s) % 20, replace=False)
        if s in PLACE_NAMED:
            x = np.union1d(x[:18], [3 * (s % 15)])
        x = np.sort(x)
        segs.append((x, 1 + (x * 7 + s) % 255))
    assert {len(x) for x, _ in segs} == set(range(20))
    recs, _ = spec.encode(*packed(segs))
    counts, escapes = spec.headers(recs, S)
    assert (rects[:, 0] + rects[:, 2] <= W2).all() and (rects[:, 2] >= 1).all()
    assert all((rects[s] != rects[s + 1]).any() for s in range(S - 1))
    wants = [crop_spec.reference(recs, S, 1, W2, H2, rects, keep_index=keep) for keep in (False, True)]
    for want in wants:
        sizes = np.diff(want[0].astype(np.int64))
        assert all(sizes[s] > 0 for s in PLACE_NAMED if s < S)
        for r0 in range(0, S, PLACE):
            if set(range(r0, min(r0 + PLACE, S))) - set(PLACE_NAMED):
                assert (sizes[r0:r0 + PLACE] == 0).any(), (r0, "a stream of the round keeps nothing")
        for seam in range(PLACE, S, PLACE):
            assert 0 < int(want[0][seam]) and 0 < int(want[4][seam]) < int(want[4][S])
    return frozen(recs, counts, escapes, rects) + (frozen(*wants[0]),)


@pytest.mark.parametrize("S", PLACE_COUNTS)
def test_more_streams_than_one_place_round(S):
    """1024: one full round of k_cwc_place (eight k_crop_facts launches) and no second; 1025: a second round of one stream;
    2049: seventeen launches and three rounds, the last of one stream."""
    recs, counts, escapes, rects, _ = place_case(S)
    with CUDACore(W2, H2, max_batch=S) as core:
        for flags in FLAGS:
            check_both_forms(core, recs, (counts, escapes), S, 1, W2, H2, rects, flags)


def test_capacity_ends_in_the_second_place_round():
    """S = 2049.  Compact form with one byte too few for record 1029: records 0 to 1028 are written, record 1029 and every one
    behind it is skipped whole, nothing is written at or past the capacity, offsets and frame_pos stay exact.  Arrays form with
    room for the entries of streams 0 to 1499."""
    S = 2049
    recs, counts, escapes, rects, (woff, wxs, wdf, wrecs, wpos) = place_case(S)
    cap, fit = int(wpos[1030]) - 1, int(wpos[1029])
    assert int(wpos[PLACE]) < fit < cap < int(wpos[S]), "the room ends inside record 1029, of the second round"
    ecap = int(woff[1500])
    assert int(woff[PLACE]) < ecap < int(woff[S]) and ecap < int(woff[2 * PLACE])
    with CUDACore(W2, H2, max_batch=S) as core:
        off, pos, out = run_compact(core, recs, (counts, escapes), S, 1, rects, cap=cap)
        assert out.size == cap and np.array_equal(off, woff) and np.array_equal(pos, wpos)
        assert np.array_equal(out[:fit], wrecs[:fit]), "the records that fit"
        assert (out[fit:] == 0x5C).all(), "a record that does not fit is skipped whole, and so is every one behind it"
        off, xs, df = run_arrays(core, recs, (counts, escapes), S, 1, rects, cap=ecap, skew=3)
        assert np.array_equal(off, woff) and np.array_equal(xs, wxs[:ecap]) and np.array_equal(df, wdf[:ecap])


# ---- 3. more tiles than one k_cwc_scan round --------------------------------------------------------------------------------
W3, ROW3 = 1024, 3072
SCAN_SHAPES = {257: 342, 513: 683}     # tiles: rows; row 340 begins at tile 255 and tile 256 at row 341, column byte 1024; tile
#                                        511 begins at row 681, column byte 1024, tile 512 at row 682, column byte 2048


def at(row, col):
    return row * ROW3 + col


def gap_stream(r, d):
    """The rectangle (683, r - 40, 85, 42) -- rows of 255 bytes, column bytes 2049 to 2303 -- with entries at (r - 39, 2100),
    (r, 2100) and (r + 1, 2100 + d).  The second record adds an entry outside the rectangle between each pair, and takes back
    an entry inside it."""
    x = [at(r - 39, 2100), at(r - 20, 2200), at(r, 2100), at(r + 1, 2100 + d)]
    outside = [at(r - 30, 2040), at(r, 2304), at(r + 1, 2048)]          # column bytes in front of 2049 and behind 2303
    second = sorted(outside + [x[1]])
    return (683, r - 40, 85, 42), [(x, [1 + d, 77, 2, 3]), (second, [179 if v == x[1] else 9 for v in second])]


def free_column(nt, least):
    """The first pixel column at or behind `least` that none of the entries `every` (one per tile, 4097 apart) lies in."""
    taken = set(((np.arange(nt) * (K + 1) + 300) % ROW3) // 3)
    return next(c for c in range(least, W3) if c not in taken)


def scan_streams(nt):
    """[(what, rectangle, [T = 2 records as (xs, diff)])] at 1024 x SCAN_SHAPES[nt]; scan_case says what each is for."""
    h = SCAN_SHAPES[nt]
    n = 3 * W3 * h
    every = np.arange(nt) * (K + 1) + 300                              # one per tile
    out = []
    for r in ([340, 681] if nt == 513 else [340]):
        for d in range(3):
            out.append((f"a mapped gap of {254 + d} across the round seam in front of row {r + 1}",) + gap_stream(r, d))
    # rows of the later rounds only: entries in every tile, three in the rectangle's first row and one in the frame's last
    y0 = 341 if nt == 257 else 342
    rect = (400, y0, 500, h - y0)
    extra = [at(y0, 500), at(y0, 1500), at(y0, 2000), at(h - 1, 2500)]  # column bytes 1200 to 2699 are kept
    x = np.union1d(every, extra)
    out.append(("a rectangle whose rows lie behind the first round", rect,
                [(x, 1 + np.arange(x.size) % 255), (every[::2], np.full(every[::2].size, 5))]))
    # one pixel wide over all rows: `every` misses the column, the kept entries lie in the first and in the last round
    c = free_column(nt, 700)
    rows_in = [5, 100, 200, h - 1]
    inside = [at(r, 3 * c + r % 3) for r in rows_in]
    x = np.union1d(every, inside)
    out.append(("a rectangle over all rows, one pixel wide", (c, 0, 1, h),
                [(x, 1 + np.arange(x.size) % 251), (every[1::2], np.full(every[1::2].size, 200))]))
    # dense tiles under a rectangle that cuts them in mid-row
    dense0 = 3 * K + np.arange(K)
    dense1 = (257 * K + np.arange(K)) if nt > 258 else np.arange(256 * K, n)
    x = np.concatenate([[17], dense0, dense1])
    out.append(("dense tiles cut in mid-row", (100, 2, 700, h - 2),
                [(x, 1 + x % 200), (dense0[::5], np.full(dense0[::5].size, 20))]))
    x = np.union1d(every, [0, ROUND - 1, ROUND, n - 1])
    full = [(x, 1 + np.arange(x.size) % 255), (every[::3], np.full(every[::3].size, 255))]
    out.append(("the full frame", (0, 0, W3, h), full))
    out.append(("the empty rectangle", (0, 0, 0, 0), full))
    return out


@functools.lru_cache(maxsize=None)
def scan_case(nt):
    """(S, T, records, counts, escapes, rectangles, what each stream is) of the shape with nt tiles, made once and read-only;
    asserts from the reference that every stream is what its name says."""
    h = SCAN_SHAPES[nt]
    n, T = 3 * W3 * h, 2
    assert -(-n // K) == nt and at(340, 0) == 255 * K and at(341, 1024) == ROUND
    assert nt == 257 or (at(681, 1024) == 511 * K and at(682, 2048) == 2 * ROUND)
    streams = scan_streams(nt)
    S = len(streams)
    names = [what for what, _, _ in streams]
    rects = np.array([rect for _, rect, _ in streams], np.int32)
    recs, _ = spec.encode(*packed([seg for _, _, segs in streams for seg in segs]))
    counts, escapes = spec.headers(recs, S * T)
    want = crop_spec.reference(recs, S, T, W3, h, rects)
    wkeep = crop_spec.reference(recs, S, T, W3, h, rects, keep_index=True)
    woff, wxs, wdf, wrecs, wpos = want
    out_esc = spec.headers(wrecs, S)[1]
    in_pos = np.cumsum([0] + [spec.frame_bytes(a, b) for a, b in zip(counts, escapes)])
    for s, what in enumerate(names):
        x, full = kept_of(want, s), kept_of(wkeep, s)                  # in the rectangle's frame, in the full frame
        assert x.size == full.size
        if what.startswith("a mapped gap"):
            d, r = int(what.split()[4]) - 254, int(what.split()[-1]) - 1
            seam = int(full[2]) // ROUND * ROUND                       # the round of the last entry begins behind the second
            assert seam in (ROUND, 2 * ROUND)
            assert list(full) == [at(r - 39, 2100), at(r, 2100), at(r + 1, 2100 + d)], "the entry taken back and those outside are gone"
            assert list(full // K) == ([226, 255, 256] if r == 340 else [482, 511, 512]) and full[1] < seam <= full[2]
            assert list(spec.gaps(x)) == [306, 9944, 254 + d] and out_esc[s] == (2 if d == 0 else 3)
            assert spec.gaps(full)[2] > 3000, "the input's gap across the seam"
        elif what == "a rectangle whose rows lie behind the first round":
            assert x.size and full.min() >= ROUND, "the facts of all tiles of round 0 are empty"
            assert set(full // ROUND) == set(range(1, -(-nt // 256))), "kept entries in every later round"
            given = np.union1d(*[np.asarray(seg[0]) for seg in streams[s][2]])
            assert set(given // ROUND) == set(range(-(-nt // 256))), "the stream has entries in every round"
            x0, y0, rw, _ = (int(v) for v in rects[s])
            mapped = (int(full[0]) // ROW3 - y0) * 3 * rw + int(full[0]) % ROW3 - 3 * x0
            assert spec.gaps(x)[0] == x[0] == mapped < 3 * rw, "the first kept entry's gap is its mapped index, not a distance"
            assert at(y0, 500) in given and at(y0, 500) not in full and (nt == 513 or at(y0, 500) // K == 255)
        elif what == "a rectangle over all rows, one pixel wide":
            assert x.size == 4 and list(x) == [3 * r + r % 3 for r in (5, 100, 200, h - 1)]
            rounds = set(full // ROUND)
            assert rounds == ({0, 2} if nt == 513 else {0, 1}), "`end` crosses a round of empty facts"
            assert counts[s * T] == nt + 4, "an entry in every tile, outside the column"
        elif what == "dense tiles cut in mid-row":
            for tile in (3, 257 if nt > 258 else 256):
                in_tile = full[full // K == tile]
                assert 0 < in_tile.size < min(K, n - tile * K), tile
                cols = in_tile % ROW3
                assert cols.min() >= 300 and cols.max() == 2399, "cut in mid-row, on either side"
            assert int((full // K == 3).sum()) > 1000
        elif what == "the full frame":
            co = coalesce_reference(recs[int(in_pos[s * T]):], 1, T, n)
            assert np.array_equal(x, co[1]) and np.array_equal(wrecs[int(wpos[s]):int(wpos[s + 1])], co[3]), "the coalescer's record"
            assert np.array_equal(x, full) and {0, ROUND - 1, ROUND, n - 1} <= set(x)
        else:
            assert what == "the empty rectangle" and x.size == 0 and wpos[s + 1] - wpos[s] == 8 and counts[s * T] > nt
    return (S, T) + frozen(recs, counts, escapes, rects) + (names,)


@pytest.mark.parametrize("flags", FLAGS, ids=["reindexed", "keep_index"])
@pytest.mark.parametrize("nt", sorted(SCAN_SHAPES))
def test_more_tiles_than_one_scan_round(nt, flags):
    """257 tiles: the second round of k_cwc_scan is one ragged tile; 513 tiles: the third round takes the first set of LDS words
    again.  The carries n, e and end cross rounds of all-zero facts."""
    S, T, recs, counts, escapes, rects, names = scan_case(nt)
    with CUDACore(W3, SCAN_SHAPES[nt], max_batch=S * T) as core:
        check_both_forms(core, recs, (counts, escapes), S, T, W3, SCAN_SHAPES[nt], rects, flags)


# ---- 4. rows per lane and tiles per row -------------------------------------------------------------------------------------
ROW_SHAPES = {   # (w, h): rows that leave whole tiles of the frame out
    (1, 2000): (1366, 600),      # rows of 3 bytes, 21 to 22 in a lane; tile 1 begins in row 1365
    (2, 700): (683, 17),         # rows of 6 bytes; tile 1 begins in row 682
    (5, 300): (274, 26),         # rows of 15 bytes, four to five in a lane; byte 4096 is row 273, column byte 1
    (10, 140): (137, 3),         # rows of 30 bytes, three in a lane; tile 1 begins in row 136
    (3000, 2): (1, 1),           # rows of 9000 bytes, five tiles; row 1 leaves tiles 0 and 1 out
    (2731, 2): (1, 1),           # rows of 8193 bytes: tile 2 begins one byte in front of row 1
}
WIDE_RECT = (1400, 0, 100, 2)    # column bytes 4200 to 4499: tiles 1 and 3 of both wide shapes


def row_rectangle_sets(w, h):
    """rectangle_sets of test_cwire_crop_gpu, adapted where a shape has one column or two rows; on the narrow frames also every
    pair (x0, width) of columns, three a call, over rows that move with the pair; on the wide ones WIDE_RECT."""
    sets = []
    for what, rects in rectangle_sets(w, h, ROW_SHAPES[(w, h)]):
        if what == "rows that skip whole tiles" and w == 1:
            rects = [(0,) + tuple(r[1:2]) + (1,) + tuple(r[3:]) for r in rects]
        if what == "no column" and h < 3:
            rects = [(w // 2, 1, 0, 1)] * 3
        sets.append((what, [tuple(int(v) for v in r) for r in rects]))
    if w <= 10:
        pairs = [(x0, rw) for x0 in range(w) for rw in range(1, w - x0 + 1)]
        pairs += pairs[:1] * (-len(pairs) % 3)
        rows = [(x0, 1 + i % 3, rw, h - 2 - i % 3 - i % 2) for i, (x0, rw) in enumerate(pairs)]
        sets += [("columns %s" % (rows[i:i + 3],), rows[i:i + 3]) for i in range(0, len(rows), 3)]
    else:
        sets.append(("a band of columns inside tiles 1 and 3", [WIDE_RECT] * 3))
    return sets


def lane_with_a_cut_middle_row(w, h, rect, acc):
    """A lane (64 bytes) that holds bytes of at least three rows of which a middle one is cut by the rectangle -- it keeps some
    of the row's bytes and, unless the row is one pixel, drops others; where the frame is one pixel wide, a row next to it in
    the lane is dropped -- with a nonzero sum on either side of the cut."""
    rb, n = 3 * w, 3 * w * h
    x0, y0, rw, rh = rect
    for lane in range(-(-n // 64)):
        lo, hi = 64 * lane, min(64 * lane + 63, n - 1)
        for r in range(lo // rb + 1, hi // rb):                         # the middle rows: neither the lane's first nor its last
            if not (y0 <= r < y0 + rh and rw):
                continue
            row = acc[r * rb:(r + 1) * rb]
            kept = row[3 * x0:3 * (x0 + rw)]
            if w > 1:
                dropped = np.concatenate([row[:3 * x0], row[3 * (x0 + rw):]])
            else:
                near = [q for q in (r - 1, r + 1) if not y0 <= q < y0 + rh]
                dropped = np.concatenate([acc[q * rb:(q + 1) * rb] for q in near] + [np.empty(0, np.uint8)])
            if kept.any() and dropped.any():
                return lane
    return None


@functools.lru_cache(maxsize=None)
def row_case(w, h):
    """-> (records, counts, escapes, [(what, rectangles)]) for S = 3, T = 2."""
    S, T = 3, 2
    n, rb = 3 * w * h, 3 * w
    recs, counts, escapes = random_records(w, h, S, T, seed=4)
    sets = row_rectangle_sets(w, h)
    acc = crop_spec.sums(recs, S, T, n)
    for what, rects in sets:
        assert len(rects) == S and all(0 <= r[0] and 0 <= r[1] and r[0] + r[2] <= w and r[1] + r[3] <= h and min(r[2:]) >= 0
                                       for r in rects), (what, rects)
    if w <= 10:
        assert rb <= 31, "three rows and more in a lane's 64 bytes"
        columns = [rects for what, rects in sets if what.startswith("columns")]
        pairs = {(r[0], r[2]) for rects in columns for r in rects}
        assert {(x0, rw) for x0 in range(w) for rw in range(1, w - x0 + 1)} == pairs, "every pair of a first and a last column"
        cut = [lane_with_a_cut_middle_row(w, h, rects[s], acc[s]) is not None for rects in columns for s in range(S)
               if w == 1 or rects[s][2] < w]
        assert cut and (all(cut) if w > 1 else any(cut)), "a lane with a middle row that the rectangle cuts"
    else:
        assert rb > 2 * K - 1 and -(-n // K) == 5
        what, rects = sets[-1]
        for s in range(S):
            xs, _ = crop_spec.segment(acc[s], w, h, rects[s], keep_index=True)
            tiles_in = np.bincount(np.flatnonzero(acc[s]) // K, minlength=5)
            assert set(xs // K) == {1, 3}, "bytes are kept in tiles 1 and 3 only"
            inside = [0, 2, 4] if rb == 9000 else [0, 2]                # (tile 4 of 2731x2 holds two bytes)
            assert (tiles_in[inside] > 0).all(), "the tiles inside the rows and outside the columns have input entries"
        assert rb == 9000 or rb == 2 * K + 1, "8193: byte 8192, the first of tile 2, is the last of row 0"
    return frozen(recs, counts, escapes) + (sets,)


@pytest.mark.parametrize("w,h", sorted(ROW_SHAPES))
def test_rows_per_lane_and_tiles_per_row(w, h):
    """test_rectangles of test_cwire_crop_gpu at rows of 3, 6, 15 and 30 bytes (CropMap divides again for every byte behind the
    lane's first row, the mask loop of crop_tile runs 3 to 22 times) and of 9000 and 8193 bytes (whole tiles inside the
    rectangle's rows and outside its columns)."""
    S, T = 3, 2
    recs, counts, escapes, sets = row_case(w, h)
    with CUDACore(w, h, max_batch=S * T) as core:
        for what, rects in sets:
            for flags in FLAGS:
                want = check_both_forms(core, recs, (counts, escapes), S, T, w, h, rects, flags)
                if what in ("no column", "no row"):
                    assert list(want[4]) == [0, 8, 16, 24], what
                elif what not in ("one pixel", "three different rectangles") and not what.startswith("columns"):
                    assert int(want[0][S]) > 0, what


# ---- 5. one call after another on the shared scratch ------------------------------------------------------------------------
W5, H5, N5 = 160, 140, 3 * 160 * 140       # 67200 bytes: 17 tiles of 4096 bytes (66 KiB), the last of 1664
S5, K5, THR5 = 2, 3, 1
GEOM5 = (16, 16, 2)
FAMILIES = ("crop compact", "crop arrays", "coalesce", "budget", "check", "activity", "touched", "refresh")
PAIRS = [(a, b) for a in FAMILIES for b in FAMILIES]


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """The inputs and the references of every family, from numpy alone.  The core's threshold is 1 and the budgets are met at
    thresholds 2 and 3, so the budget call's search sums bins 3, 4 and 5 of a stream's row and its result depends on them: they
    hold three of the six words the crop call leaves there (the last column byte, skip and base), none of them zero.  (Bin 0,
    the rectangle's first row, is summed by no threshold: k_cwb_thr adds the bins above T.)"""
    n, S, T = N5, S5, K5
    rng = np.random.default_rng(55)
    c = SimpleNamespace()
    # the burst: S * K sparse records, every second entry of a record taken back by the next
    segs = []
    for b in range(S * T):
        cnt = 250 + 40 * b
        x, d = np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)
        if b % T:
            px, pd = segs[-1]
            fresh = ~np.isin(x, px[::2])
            x, d = np.concatenate([x[fresh], px[::2]]), np.concatenate([d[fresh], (256 - np.asarray(pd[::2])) % 256])
            o = np.argsort(x)
            x, d = x[o], d[o]
        segs.append((x, d))
    c.burst, _ = spec.encode(*packed(segs))
    c.bhdr = spec.headers(c.burst, S * T)
    assert (c.bhdr[1] > 0).all(), "every record of the burst has escapes"
    c.rects = np.array([(20, 30, 100, 80), (3, 0, 157, 139)], np.int32)
    c.crop = crop_spec.reference(c.burst, S, T, W5, H5, c.rects)
    c.crop_keep = crop_spec.reference(c.burst, S, T, W5, H5, c.rects, keep_index=True)
    c.coalesce = coalesce_reference(c.burst, S, T, n)
    assert 0 < int(c.crop[0][1]) < int(c.coalesce[0][1]) and int(c.crop[0][S]) < int(c.coalesce[0][S])
    assert (spec.headers(c.crop[3], S)[1] > 0).all()
    words = [(y0, y0 + rh, 3 * x0, 3 * (x0 + rw), 3 * W5 - 3 * rw, y0 * 3 * rw + 3 * x0) for x0, y0, rw, rh in c.rects]
    assert all(min(w6[3:]) > 0 for w6 in words), "the crop call's words in bins 3 to 5 of each row are not zero"
    assert all(w6[3] > 0 for w6 in words), "bin 3 with MI355_CROP_KEEP_INDEX too, where skip and base are 0"
    # the tick: states and frames that differ at some 400 bytes by 2 to 60
    pre = rng.integers(60, 196, (S, n), dtype=np.uint8)
    cur = pre.copy()
    for s in range(S):
        x = rng.choice(n, 400 + 30 * s, replace=False)
        a = rng.integers(2, 61, x.size)
        cur[s][x] = pre[s][x] + np.where(rng.random(x.size) < 0.5, a, -a)
    c.pre = pre
    c.tick = numpy_tick(pre, cur, THR5)
    assert (c.tick[3] > 0).all(), "both records of the tick have escapes"
    ns = [len(x) for x, _, _ in c.tick[5]]
    c.budgets = np.array([int((c.tick[5][s][2] > 2 + s).sum()) for s in range(S)], np.uint32)   # what magnitudes above 2 / 3 need
    c.budget = budget_expected(c.tick, pre, THR5, c.budgets)
    assert all(0 < int(c.budgets[s]) < ns[s] for s in range(S)), "both streams exceed their budgets"
    assert list(c.budget[0]) == [2, 3], "the thresholds lie below bins 3 to 5: a count left in them moves the threshold"
    assert list(np.diff(c.budget[1].astype(np.int64))) == list(c.budgets)
    # the record check: the burst's records, the fourth with a code turned into an escape code
    pos = np.cumsum([0] + [spec.frame_bytes(a, b) for a, b in zip(*c.bhdr)])
    cases = []
    for b in range(S * T):
        rec = c.burst[pos[b]:pos[b + 1]].copy()
        if b == 3:
            k = int(np.flatnonzero(rec[8:8 + int(c.bhdr[0][b])] != 255)[5])
            rec[8 + k] = 255
        cases.append((None, rec, int(c.bhdr[0][b]), int(c.bhdr[1][b])))
    c.checked, c.chdr = batch_of(cases)[0], batch_of(cases)[1:]
    c.verdicts = np.array([ref_verdict(rec, k, e, n) for _, rec, k, e in cases], np.uint32)
    assert c.verdicts[3, 0] & CWIRE_BAD_CODES and not c.verdicts[[0, 1, 2, 4, 5], 0].any()
    # activity and touched tiles of the burst
    off, xs, _ = spec.decode(c.burst, S * T)
    c.ncells = activity_cells(W5, H5, GEOM5[0], GEOM5[1])[0]
    c.activity = oracle(W5, H5, GEOM5[0], GEOM5[1], GEOM5[2], S, T, off, xs)
    assert (c.activity[1][:, 0] == [int(off[T]), int(off[2 * T] - off[T])]).all()
    sparse = [np.sort(rng.choice(n, 9, replace=False)) for _ in range(S * T)]
    c.sparse, _ = spec.encode(*packed([(x, np.ones(9, np.uint8)) for x in sparse]))
    c.shdr = spec.headers(c.sparse, S * T)
    c.touched = ws.mask_of(np.stack([ws.touched(n, sparse[s * T:(s + 1) * T]) for s in range(S)]))
    assert all(0 < bin(int(v)).count("1") < ws.tiles(n) for v in c.touched[:, 0])
    # refresh: sender states with zero bytes, a peer whose tiles 0, 7 and 16 (stream 0) and 3 (stream 1) differ
    snd = rng.integers(1, 256, (S, n), dtype=np.uint8)
    snd[rng.random((S, n)) < 0.4] = 0
    c.snd = snd
    peer_states, c.sel = damaged(snd, [(0, 0), (0, 7), (0, 16), (1, 3)])
    c.peer = np.stack([rs.digest(peer_states[s]) for s in range(S)])
    assert np.array_equal(rs.selected_tiles(snd, c.peer), c.sel) and rs.tiles(n) == 17
    c.refresh = rs.refresh(snd, c.sel)
    for v in vars(c).values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


class Chain:
    """The device side of chain_inputs(): the inputs uploaded once into guarded buffers; start(family) makes the family's own
    guarded outputs (and, for the budget call, its own copy of the states it thins), queue() makes the call and nothing else,
    check() compares every output with the reference."""

    def __init__(self, c):
        self.c = c
        self.burst = Guarded(c.burst.size, data=c.burst)
        self.tick = Guarded(c.tick[0].size, data=c.tick[0])
        self.checked = Guarded(c.checked.size, data=c.checked)
        self.sparse = Guarded(c.sparse.size, data=c.sparse)
        self.snd = Region(S5, N5).put(c.snd)
        self.capC, self.capE = cwire_bytes_max(N5, S5), S5 * N5

    def start(self, family):
        S, I32, I64 = S5, torch.int32, torch.int64
        b = SimpleNamespace(family=family)
        if family in ("crop compact", "coalesce", "budget"):
            b.off, b.pos, b.out = Guarded(S + 1, I32), Guarded(S + 1, I64), Guarded(self.capC)
        if family == "budget":
            b.thr, b.states = Guarded(S, I32), Region(S, N5).put(self.c.tick[4])
        if family == "crop arrays":
            b.off, b.xs, b.df = Guarded(S + 1, I32), Guarded(self.capE, I32), Guarded(self.capE, torch.uint8, skew=1)
        if family == "check":
            b.out = Guarded(4 * (S * K5 + 1), I32)
        if family == "activity":
            b.out = Outputs(S + 1, self.c.ncells)
        if family == "touched":
            b.mask = Guarded((S + 1) * ws.mask_words(N5), I32)
        if family == "refresh":
            b.r = Refresh(None, self.snd, S, self.c.peer)
        return b

    def queue(self, core, b):
        c, S, T = self.c, S5, K5
        if b.family == "crop compact":
            core.cwire_crop_cwire_batch(self.burst.ptr, c.bhdr[0], c.bhdr[1], S, T, c.rects, b.off.ptr, b.pos.ptr, b.out.ptr, self.capC)
        elif b.family == "crop arrays":
            core.cwire_crop_batch(self.burst.ptr, c.bhdr[0], c.bhdr[1], S, T, c.rects, b.off.ptr, b.xs.ptr, b.df.ptr, self.capE, flags=KEEP)
        elif b.family == "coalesce":
            core.cwire_coalesce_cwire_batch(self.burst.ptr, c.bhdr[0], c.bhdr[1], S, T, b.off.ptr, b.pos.ptr, b.out.ptr, self.capC)
        elif b.family == "budget":
            core.cwire_budget_cwire_batch(self.tick.ptr, c.tick[2], c.tick[3], b.states.ptr, S, c.budgets, b.thr.ptr, b.off.ptr, b.pos.ptr,
                                          b.out.ptr, self.capC, stride=b.states.stride)
        elif b.family == "check":
            core.cwire_check_batch(self.checked.ptr, c.chdr[0], c.chdr[1], S * T, b.out.ptr)
        elif b.family == "activity":
            core.cwire_activity_batch(self.burst.ptr, c.bhdr[0], c.bhdr[1], S, T, GEOM5[0], GEOM5[1], b.out.cells.ptr, b.out.summ.ptr,
                                      min_count=GEOM5[2])
        elif b.family == "touched":
            core.cwire_touched_tiles_batch(self.sparse.ptr, c.shdr[0], c.shdr[1], S, T, b.mask.ptr)
        else:
            assert b.family == "refresh"
            b.r.call(core, self.snd)

    def check(self, b, what):
        c, S = self.c, S5
        if b.family in ("crop compact", "coalesce"):
            want = c.crop if b.family == "crop compact" else c.coalesce
            assert np.array_equal(b.off.get().view(np.uint32), want[0]) and np.array_equal(b.pos.get().view(np.uint64), want[4]), what
            assert np.array_equal(b.out.get(written=want[3].size)[:want[3].size], want[3]), what
        elif b.family == "crop arrays":
            want, tot = c.crop_keep, int(c.crop_keep[0][S])
            assert np.array_equal(b.off.get().view(np.uint32), want[0]), what
            assert np.array_equal(b.xs.get(written=tot)[:tot], want[1]) and np.array_equal(b.df.get(written=tot)[:tot], want[2]), what
        elif b.family == "budget":
            thr, off, pos, recs, states, _ = c.budget
            assert np.array_equal(b.thr.get().view(np.uint32), thr), (what, b.thr.get(), thr)
            assert np.array_equal(b.off.get().view(np.uint32), off) and np.array_equal(b.pos.get().view(np.uint64), pos), what
            assert np.array_equal(b.out.get(written=recs.size)[:recs.size], recs), what
            assert np.array_equal(b.states.get(), states), what
        elif b.family == "check":
            k = S * K5
            assert np.array_equal(b.out.get(written=4 * k).view(np.uint32)[:4 * k].reshape(k, 4), c.verdicts), what
        elif b.family == "activity":
            cells, summ = b.out.get(S)
            assert np.array_equal(summ, c.activity[1]) and np.array_equal(cells, c.activity[0]), what
        elif b.family == "touched":
            mw = ws.mask_words(N5)
            assert np.array_equal(b.mask.get(written=S * mw).view(np.uint32)[:S * mw].reshape(S, mw), c.touched), what
        else:
            recs, _, _ = check_refresh(b.r, c.snd, c.sel)
            assert np.array_equal(recs, c.refresh[2]), what

    def inputs_unchanged(self):
        c = self.c
        assert np.array_equal(self.burst.get(), c.burst) and np.array_equal(self.tick.get(), c.tick[0])
        assert np.array_equal(self.checked.get(), c.checked) and np.array_equal(self.sparse.get(), c.sparse)
        assert np.array_equal(self.snd.get(), c.snd)


def test_each_family_alone():
    """The solo runs: each family once on a fresh core, synchronised, against its reference."""
    chain = Chain(chain_inputs())
    for family in FAMILIES:
        with CUDACore(W5, H5, max_batch=S5 * K5, threshold=THR5) as core:
            b = chain.start(family)
            torch.cuda.synchronize()
            chain.queue(core, b)
            core.synchronize()
            chain.check(b, family)
    chain.inputs_unchanged()


@pytest.mark.parametrize("first", FAMILIES)
def test_one_call_after_another(first):
    """Every ordered pair (first, B), first itself included, on one core's own stream: the outputs and the budget call's states
    are made, one synchronisation, A and B queued with nothing in between, one synchronisation, every output of both compared.
    With the crop call first the budget call reads histogram rows whose first six words the crop call wrote; with the budget
    call first the crop call's words replace bins that were counted; the facts of each call replace the other's in the chunk
    table."""
    pairs = [p for p in PAIRS if p[0] == first]
    assert len(pairs) == len(FAMILIES) and len(PAIRS) == 64
    chain = Chain(chain_inputs())
    with CUDACore(W5, H5, max_batch=S5 * K5, threshold=THR5) as core:
        for a, b in pairs:
            ba, bb = chain.start(a), chain.start(b)
            torch.cuda.synchronize()
            chain.queue(core, ba)
            chain.queue(core, bb)
            core.synchronize()
            chain.check(ba, f"{a}, in front of {b}")
            chain.check(bb, f"{b}, behind {a}")
    chain.inputs_unchanged()

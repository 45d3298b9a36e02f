"""-m gpu: mi355_cwire_touched_tiles_batch, mi355_wall_compose_batch, mi355_cwire_check_batch and mi355_activity_batch /
mi355_cwire_activity_batch past the fixed counts at which their kernels start another round (csrc/stream_ops.hip):
    k_cw_touched        64 tiles and two mask words per wave: 256x341 (64 tiles, 2 words: one full wave), 256x342 (65, 3: wave 1
                        holds one tile and stores word 2 only), 256x512 (96, 3: wave 1 half full, w + 1 == mask_words), 256x513
                        (97, 4), 256x683 (129, 5: three waves); overwriting and ORing onto a start mask
    wall_band_selected  mask[t >> 5] for t >= 64 in the masked k_wall_compose: 256x342 and 256x513 with only tile 64, only the last
                        tile, or tiles {63, 64} selected, k = 1, 3, 16; the chain apply -> touched tiles -> masked compose at
                        256x342 with changes in tiles 63 and 64 only
    k_cwk_finish        256 chunks of 4096 entries per round (and k_cwa_scan field 0 with its 32-bit carry): records of
                        1 048 679 entries on 1024x343 (257 chunks, two rounds) and of 2 097 155 entries on 1024x683 (513 chunks,
                        three rounds: the LDS words alternate back to the first set); the chunk found at i >= 256, a `before` that
                        holds the carry, 255 codes counted across rounds, the pad test at chunk 256 of a record whose chunk base
                        is not 0, clamped sums carried from round to round: one escape of
                        0xFFFFF000 at entry 1 048 576, where only the carried prefix passes 2^32 and, wrapped, would lie inside
                        the frame
    k_act_entries       1024 x 256 lanes per round: 1024x342 (1 050 624 bytes, 257 tiles) with a record of every byte, five rounds;
                        the offsets in LDS up to 8192 words: 15x1 with (S, T) = (8191, 1) (8192 words, the 32 KiB launch),
                        (8192, 1), (64, 128) and (4096, 2) (8193 words, no LDS)
    k_act_clear         2048 x 256 cells per pass: 1x1 cells at 1024x342, 350 208 cells per stream, 700 416 in the call
    k_act_summary       350 208 cells of one stream, a tie for the peak that resolves to the least index

Every comparison is np.array_equal with numpy: cwire_spec for the records, wall_spec for tiles, masks, thumbnails and required
pixels, ref_verdict / ref_walk of test_cwire_check_host (and mi355_cwire_check_host) for the verdicts, the oracle of
test_activity_gpu for grids and summaries -- never the code under test.  Every buffer the GPU sees is guarded (gpu_util.Guarded /
Region) and starts as a non-zero pattern.  The inputs are made once, read-only, by the builders below; each builder asserts from
the reference alone that its input reaches the seam it is named for, and test_newer_seams_host.py runs every builder without a GPU."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
import wall_spec as ws
from cudavideostream_amd import CWIRE_BAD_CODES, CWIRE_BAD_ESCAPE, CWIRE_BAD_PAD, CWIRE_BAD_RANGE, activity_cells
from gpu_util import GUARD, CUDACore, Guarded, Region
from test_activity_gpu import Outputs, both_forms, oracle, packed, run_arrays, run_compact
from test_cwire_check_gpu import check_records, encoded
from test_cwire_check_host import SAT, put_esc, ref_verdict, ref_walk
from test_wall_gpu import Wall, compose, make_records, mask_buffer, pattern, random_states, row_layout

pytestmark = pytest.mark.gpu

K = 4096                      # bytes of a tile, entries of a chunk
WAVE = 64                     # tiles of a wave of k_cw_touched
SEAM = 256 * K                # entries of a round of k_cwk_finish and k_cwa_scan: 1 048 576
ENTRY_ROUND = 1024 * 256      # entries of a round of k_act_entries
CLEAR_PASS = 2048 * 256       # cells of a pass of k_act_clear
LDS_WORDS = 8192              # offset words k_act_entries searches in LDS


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- 1. touched tiles past one wave -----------------------------------------------------------------------------------------
W1 = 256
TOUCHED = {341: (64, 2), 342: (65, 3), 512: (96, 3), 513: (97, 4), 683: (129, 5)}   # height: (tiles, mask words)


@functools.lru_cache(maxsize=None)
def touched_case(h, T):
    """256 x h, S = 3 streams of T records -> (n, records, counts, escapes, touched bool[3, tiles], start mask uint32[4, words]).
    Stream 0: the last byte of tile 63, the first of tile 64, the frame's last byte and, where they exist, the first and last
    byte of tile 127 and the first of tile 128, spread over the records; stream 1: entries in the tiles of the last wave only;
    stream 2: empty records.  The start mask has bit 5 of every word and, where the last word has room, a bit past `tiles`."""
    S, n = 3, 3 * W1 * h
    t, mw = ws.tiles(n), ws.mask_words(n)
    assert (t, mw) == TOUCHED[h]
    last_wave = (t - 1) // WAVE
    lo = WAVE * last_wave * K                                       # the first byte of the last wave's first tile
    marks = sorted({min(63 * K + K - 1, n - 1), n - 1} | {x for x in (64 * K, 127 * K, 127 * K + K - 1, 128 * K) if x < n})
    rng = np.random.default_rng(10 * h + T)

    def entries(s, r):
        if s == 0:
            return marks[r::T]
        if s == 1:
            return [] if r == 1 else np.unique(rng.integers(lo, n, 2 + 5 * r))
        return []

    recs, counts, escapes, _, lists = make_records(n, S, T, entries)
    want = np.stack([ws.touched(n, lists[s * T:(s + 1) * T]) for s in range(S)])
    words = ws.mask_of(want)
    assert want.shape == (S, t) and words.shape == (S, mw)
    assert want[0, 63] and want[0, t - 1] and not want[0, :63].any(), "tile 63 is touched and no tile below it"
    if t > WAVE:
        assert want[0, 64] and words[0, 2] & 1 and words[0, 1] >> 31, "tiles 63 and 64: the last bit of wave 0, the first of wave 1"
        assert T == 1 or marks.index(63 * K + K - 1) % T != marks.index(64 * K) % T, "they come from different records"
    if t > 2 * WAVE:
        assert want[0, 127] and want[0, 128] and words[0, 4] == 1, "wave 2 holds one tile"
    assert int(want[0].sum()) == len({x // K for x in marks})
    assert want[1].any() and not want[1, :WAVE * last_wave].any(), "stream 1 touches the last wave only"
    assert not want[2].any() and not counts[2 * T:].any()
    start = np.zeros((S + 1, mw), np.uint32)
    start[:] = 1 << 5
    if t % 32:
        start[:, -1] |= np.uint32(1 << 31)
        assert 32 * (mw - 1) + 31 >= t, "a bit past `tiles`"
    assert not want[0, 5::32].any() and not words[2].any(), "streams 0 and 2 set none of the start mask's bits themselves"
    return (n,) + frozen(recs, counts, escapes, want, start)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("h", sorted(TOUCHED))
def test_touched_tiles_past_one_wave(h, T):
    """Overwriting a pattern mask, then ORing onto the start mask: every bit of it is kept, the ones past `tiles` too; the row
    behind the last stream keeps its content in both calls."""
    S = 3
    n, recs, counts, escapes, want, start = touched_case(h, T)
    mw = ws.mask_words(n)
    d_recs = Guarded(recs.size, data=recs)
    mask = Guarded((S + 1) * mw, torch.int32)                        # (the pattern: -7, nearly every bit set)
    acc = mask_buffer(start)
    with CUDACore(W1, h, max_batch=S * T) as core:
        torch.cuda.synchronize()
        core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, T, mask.ptr)
        core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, T, acc.ptr, accumulate=True)
        core.synchronize()
    got = mask.get(written=S * mw).view(np.uint32)[:S * mw].reshape(S, mw)
    assert np.array_equal(got, ws.mask_of(want)), [hex(int(v)) for v in got[0]]
    got_acc = acc.get().view(np.uint32).reshape(S + 1, mw)
    assert np.array_equal(got_acc[:S], ws.mask_of(want) | start[:S])
    assert np.array_equal(got_acc[S], start[S])
    assert np.array_equal(d_recs.get(), recs)


# ---- 2. the masked compose with high tiles ------------------------------------------------------------------------------------
SELECTIONS = {"t64": lambda t: (64,), "last": lambda t: (t - 1,), "t63_64": lambda t: (63, 64)}


@functools.lru_cache(maxsize=None)
def masked_case(h, which):
    """256 x h, S = 2 -> (selected tiles of stream 0 as bool[tiles], mask rows uint32[2, words] by wall_spec.mask_of, states).
    Stream 1's row holds nothing but bits past `tiles`.  No state byte equals the pattern."""
    S, n = 2, 3 * W1 * h
    t, mw = ws.tiles(n), ws.mask_words(n)
    assert (t, mw) == TOUCHED[h] and t > WAVE
    sel = np.zeros((S, t), bool)
    sel[0, list(SELECTIONS[which](t))] = True
    rows = ws.mask_of(sel)
    assert rows.shape == (S, mw) and np.array_equal(ws.selected_of(rows[0], n), sel[0])
    assert sel[0, WAVE:].any() and int(rows[0, 2:].sum()) != 0, "a selected tile at or above 64: a bit in word 2 or above"
    if which != "t63_64":
        assert not rows[0, :2].any(), "words 0 and 1 are empty: an index taken modulo 64 finds nothing"
    else:
        assert list(rows[0, :3]) == [0, 1 << 31, 1]
    assert t % 32 == 1
    rows[1, -1] = 0xFFFFFFFE
    assert not ws.selected_of(rows[1], n).any()
    src = random_states(W1, h, S)
    src = np.where(src == GUARD, np.uint8(GUARD + 1), src)
    return frozen(sel[0].copy(), rows, src)


@pytest.mark.parametrize("which", sorted(SELECTIONS))
@pytest.mark.parametrize("h", [342, 513])
def test_masked_compose_with_high_tiles(h, which):
    """What test_masked_compose_writes_the_required_pixels asserts, with the selected tiles in mask words 1 to 3: every required
    pixel of stream 0 equals the numpy thumbnail, every other pixel of its rectangle is the pattern or that value, stream 1's
    rectangle and everything else still hold the pattern."""
    w, S = W1, 2
    n = 3 * w * h
    sel, rows, src = masked_case(h, which)
    states = Region(S, n, n + 3, 5).put(src)
    mask = mask_buffer(rows)
    with CUDACore(w, h, max_batch=S) as core:
        for k in (1, 3, 16):
            places, wall_w, wall_h = row_layout(w, h, [k, k])
            wall = Wall(wall_w, wall_h)
            torch.cuda.synchronize()
            compose(core, states, S, places, wall, mask)
            core.synchronize()
            got = wall.get()
            full = ws.compose(pattern(wall_w, wall_h), src, w, h, places)
            x, y, tw, th = ws.rect(w, h, places[0])
            req = ws.required(sel, w, h, k)
            assert req.shape == (th, tw) and req.any() and not req.all()
            inside = np.zeros((wall_h, wall_w), bool)
            inside[y:y + th, x:x + tw] = True
            needed = np.zeros((wall_h, wall_w), bool)
            needed[y:y + th, x:x + tw] = req
            assert np.array_equal(got[needed], full[needed]), f"k = {k}: a required pixel is wrong"
            # (a thumbnail byte may itself equal the pattern: that only loosens this side, the required pixels above are exact)
            ok = (got == full) | (got == GUARD)
            assert ok[inside].all(), f"k = {k}: a pixel of the rectangle is neither the pattern nor its value"
            assert (got[~inside] == GUARD).all(), f"k = {k}: written outside stream 0's rectangle"
    assert np.array_equal(mask.get().view(np.uint32).reshape(S, -1), rows)
    assert np.array_equal(states.get(), src)


def test_full_compose_at_65_tiles():
    """256x342 without a mask, k = 1 and k = 5 in one call, against wall_spec.compose."""
    w, h, S = W1, 342, 2
    n = 3 * w * h
    assert ws.tiles(n) == 65
    src = random_states(w, h, S)
    states = Region(S, n, n + 3, 5).put(src)
    places, wall_w, wall_h = row_layout(w, h, [1, 5])
    wall = Wall(wall_w, wall_h)
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        compose(core, states, S, places, wall)
        core.synchronize()
    assert np.array_equal(wall.get(), ws.compose(pattern(wall_w, wall_h), src, w, h, places))
    assert np.array_equal(states.get(), src)


@functools.lru_cache(maxsize=None)
def chain_case():
    """256x342, S = 3, T = 2, k = 2, 3, 1 -> (records, counts, escapes, old, new, places, wall_w, wall_h, the wall of the old
    states, the wall of the new ones, mask words).  Stream 0 changes the 600 bytes around byte 64 * 4096, stream 1 random bytes of
    tiles 63 and 64, stream 2 is a still camera."""
    w, h, S, T = W1, 342, 3, 2
    n = 3 * w * h
    assert ws.tiles(n) == 65 and n - 64 * K == 512
    rng = np.random.default_rng(64)

    def entries(s, r):
        if s == 0:
            return np.arange(64 * K - 300, 64 * K) if r == 0 else np.arange(64 * K - 10, 64 * K + 300)
        if s == 1:
            return np.unique(np.concatenate([rng.integers(63 * K, n, 200), [63 * K, 64 * K - 1, 64 * K, n - 1]]))
        return []

    recs, counts, escapes, delta, lists = make_records(n, S, T, entries)
    old = random_states(w, h, S, seed=9)
    new = old + delta
    touched = np.stack([ws.touched(n, lists[s * T:(s + 1) * T]) for s in range(S)])
    for s in (0, 1):
        assert list(np.flatnonzero(touched[s])) == [63, 64], "the changes lie in tiles 63 and 64 only"
    assert not touched[2].any()
    words = ws.mask_of(touched)
    assert [list(r) for r in words] == [[0, 1 << 31, 1], [0, 1 << 31, 1], [0, 0, 0]]
    places, wall_w, wall_h = row_layout(w, h, [2, 3, 1])
    want_old = ws.compose(pattern(wall_w, wall_h), old, w, h, places)
    want_new = ws.compose(pattern(wall_w, wall_h), new, w, h, places)
    assert not np.array_equal(want_old, want_new)
    for s in (0, 1):                                                 # both tiles change pixels of both thumbnails
        x, y, tw, th = ws.rect(w, h, places[s])
        changed = (want_old != want_new).any(axis=2)[y:y + th, x:x + tw]
        for tile in (63, 64):
            only = np.zeros(65, bool)
            only[tile] = True
            assert (changed & ws.required(only, w, h, int(places[s][2]))).any(), (s, tile)
    return frozen(recs, counts, escapes, old, new, places, want_old, want_new, words) + (wall_w, wall_h)


def test_apply_touched_and_masked_compose_at_65_tiles():
    """The chain of test_apply_touched_and_masked_compose_keep_the_wall_current with the changes in tiles 63 and 64: apply,
    touched tiles, masked compose, once synchronised after every call and once not at all: both runs give the numpy wall of the
    new states."""
    w, h, S, T = W1, 342, 3, 2
    n = 3 * w * h
    recs, counts, escapes, old, new, places, want_old, want_new, words, wall_w, wall_h = chain_case()
    mw = ws.mask_words(n)
    results = []
    with CUDACore(w, h, max_batch=S * T) as core:
        for sync in (True, False):
            step = core.synchronize if sync else (lambda: None)
            states, d_recs, mask = Region(S, n).put(old), Guarded(recs.size, data=recs), Guarded(S * mw, torch.int32)
            wall = Wall(wall_w, wall_h, want_old)
            torch.cuda.synchronize()
            core.apply_multi_stream_cwire_batch(d_recs.ptr, counts, escapes, S, T, states.ptr)
            step()
            core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, T, mask.ptr)
            step()
            compose(core, states, S, places, wall, mask)
            core.synchronize()
            results.append((states.get(), wall.get(), mask.get().view(np.uint32).reshape(S, mw)))
            assert np.array_equal(d_recs.get(), recs)
    for got_states, got_wall, got_mask in results:
        assert np.array_equal(got_states, new)
        assert np.array_equal(got_mask, words)
        assert np.array_equal(got_wall, want_new)


# ---- 3. the check past 256 and 512 chunks -------------------------------------------------------------------------------------
CHECK_SHAPES = {257: (1024, 343), 513: (1024, 683)}   # chunks of the large records: (w, h)


def gapped(n, gaps):
    """n ascending indices, every gap 0 but the gaps {entry: gap} in front of the named entries."""
    g = np.zeros(n, np.int64)
    for k, v in gaps.items():
        g[k] = v
    return np.cumsum(g + 1) - 1


def inc_of(X):
    return np.diff(np.concatenate([[0], X]))


def rank_of(rec, k):
    """The escape rank of entry k (a 255 code)."""
    assert rec[8 + k] == 255
    return int((rec[8:8 + k] == 255).sum())


@functools.lru_cache(maxsize=None)
def check_case(nc):
    """-> (N, names, records [(bytes, n, e)], reference verdicts uint32[records, 4]): one batch, a small clean record before the
    large ones and one behind them (257 chunks; the 513-chunk batch is its two large records alone)."""
    w, h = CHECK_SHAPES[nc]
    N = 3 * w * h
    named = []

    def add(name, rec, n, e):
        rec.setflags(write=False)
        named.append((name, (rec, n, e)))

    if nc == 257:
        n = SEAM + 103
        assert N == 1053696 and n % 4 == 3 and -(-n // K) == 257 and 4900 < N - n < 5100
        gaps = {3 * K + 5: 300, 10 * K + 7: 300, 100 * K: 255, SEAM - 1: 300, SEAM: 300, SEAM + 50: 256}
        diff = (1 + np.arange(n) % 255).astype(np.uint8)
        xs = gapped(n, gaps)
        assert xs[-1] < N
        clean = encoded(xs, diff)
        rec, _, e = clean
        assert e == len(gaps) and all(rec[8 + k] == 255 for k in gaps), "an escape at entry 1 048 575 and at entry 1 048 576"
        assert [rank_of(rec, k) for k in sorted(gaps)] == list(range(e))
        add("small before", *encoded([3, 9, 500, 501, N - 1]))
        add("clean", *clean)
        for k in (SEAM - 1, SEAM, n - 1):
            far = xs.copy()
            far[k:] += N
            add(f"range {k}", *encoded(far, diff))
        p = SEAM + 20                                                # a plain code behind entry 1 048 576
        bad = rec.copy()
        assert bad[8 + p] != 255 and not (bad[8 + SEAM + 51:8 + n] == 255).any()
        bad[8 + p] = 255
        add("codes", bad, n, e)
        bad = rec.copy()
        assert rank_of(bad, SEAM) == 4 and SEAM // K == 256
        put_esc(bad, n, 4, 7)                                        # the escape of entry 1 048 576, chunk 256, is below 255
        add("escape", bad, n, e)
        for name, at in (("pad code", 8 + n), ("pad diff", 8 + spec.pad4(n) + 4 * e + n)):
            bad = rec.copy()
            assert bad[at] == 0
            bad[at] = 9
            add(name, bad, n, e)
        bad = rec.copy()
        put_esc(bad, n, rank_of(bad, 3 * K + 5), SAT)
        add("sat", bad, n, e)
        bad = rec.copy()
        put_esc(bad, n, rank_of(bad, 10 * K + 7), 0x80000000)
        put_esc(bad, n, rank_of(bad, SEAM), 0x80000003)
        add("wrap", bad, n, e)
        bad = rec.copy()
        put_esc(bad, n, rank_of(bad, SEAM), 0xFFFFF000)              # alone in chunk 256: only the carried prefix passes 2^32
        add("carry", bad, n, e)
        add("small behind", *encoded(np.arange(5, 3000, 7)))
    else:
        n = 2 * SEAM + 3
        assert N == 2098176 and -(-n // K) == 513 and N - n < 1024
        gaps = {SEAM - 1: 255, SEAM: 255, 2 * SEAM - 1: 255, 2 * SEAM: 255}       # escapes of exactly 255: the room is 1021 bytes
        diff = (1 + np.arange(n) % 251).astype(np.uint8)
        xs = gapped(n, gaps)
        assert xs[-1] < N
        clean = encoded(xs, diff)
        rec, _, e = clean
        assert e == 4 and all(rec[8 + k] == 255 for k in gaps)
        add("clean", *clean)
        far = xs.copy()
        far[2 * SEAM:] += N
        add(f"range {2 * SEAM}", *encoded(far, diff))
    names = [name for name, _ in named]
    records = [r for _, r in named]
    want = np.array([ref_verdict(r, k, e_, N) for r, k, e_ in records], np.uint32)
    v = dict(zip(names, want))
    assert list(v["clean"]) == [0, e, n, xs[-1] + 1]
    for name in names:
        if name.startswith("range"):
            k = int(name.split()[1])
            X, _, _ = ref_walk(*records[names.index(name)])
            assert X[k] > N and X[k - 1] <= N, "the first out-of-range entry is entry k"
            assert list(v[name][[0, 2]]) == [CWIRE_BAD_RANGE, k] and v[name][3] == xs[-1] + 1 + N
    if nc == 257:
        assert (want[[0, -1], 0] == 0).all() and want[0, 2] == 5 and want[0, 3] == N, "the small records are clean"
        assert list(v["codes"][:3]) == [CWIRE_BAD_CODES, e + 1, n]
        assert list(v["escape"]) == [CWIRE_BAD_ESCAPE, e, n, xs[-1] + 1 - 293]
        assert list(v["pad code"]) == [CWIRE_BAD_PAD, e, n, xs[-1] + 1] and list(v["pad diff"]) == list(v["pad code"])
        assert list(v["sat"]) == [CWIRE_BAD_RANGE, e, 3 * K + 5, SAT] and 3 * K + 5 < SEAM, "the first offender is in round 0"
        # the two escapes of "wrap": no chunk and no round sums to 2^32, the prefix across the round does.  An escape of 2^31
        # is itself past every frame this library takes, so the reference's first offender is the first of the two.
        X, _, _ = ref_walk(*records[names.index("wrap")])
        inc = inc_of(X)
        assert np.add.reduceat(inc, np.arange(0, n, K)).max() < 2 ** 32
        assert X[SEAM - 1] < 2 ** 32 and X[-1] - X[SEAM - 1] < 2 ** 32 and X[SEAM] >= 2 ** 32 and X[-1] % 2 ** 32 <= N
        assert list(v["wrap"]) == [CWIRE_BAD_RANGE, e, 10 * K + 7, SAT]
        # "carry": one escape, of entry 1 048 576.  Everything before it is inside the frame, no chunk and no round sums to
        # 2^32, the prefix across the round does and, taken modulo 2^32, lands inside the frame again: the offender is found in
        # chunk 256 only by a `before` that holds the carry and a `before + sum` that does not wrap.
        X, _, _ = ref_walk(*records[names.index("carry")])
        inc = inc_of(X)
        assert np.add.reduceat(inc, np.arange(0, n, K)).max() < 2 ** 32
        assert X[SEAM - 1] <= N and X[-1] - X[SEAM - 1] < 2 ** 32, "round 0 is inside the frame, round 1 alone is below 2^32"
        assert X[SEAM] >= 2 ** 32 and X[SEAM] % 2 ** 32 <= N and X[-1] % 2 ** 32 <= N, "the wrapped prefix is inside the frame"
        assert list(v["carry"]) == [CWIRE_BAD_RANGE, e, SEAM, SAT], "the first out-of-range entry is entry 1 048 576"
    want.setflags(write=False)
    return N, names, records, want


@pytest.mark.parametrize("nc", sorted(CHECK_SHAPES))
def test_check_past_the_chunk_rounds(nc):
    """257 chunks: the second round of k_cwk_finish and of k_cwa_scan is one chunk, with both carries; 513 chunks: the third
    round takes the first set of LDS words again.  Device form == mi355_cwire_check_host == the numpy reference, all four words."""
    w, h = CHECK_SHAPES[nc]
    N, names, records, want = check_case(nc)
    with CUDACore(w, h, max_batch=len(records)) as core:
        got = check_records(core, N, records)                    # (the GPU and the host form against ref_verdict, inside)
    assert np.array_equal(got, want), names


# ---- 4. activity past its rounds ----------------------------------------------------------------------------------------------
W4, H4, N4 = 1024, 342, 3 * 1024 * 342
BIG_CELLS = [(1, 1), (16, 16), (5000, 5000)]
PEAK0, PEAK1 = 5000, 70001    # the least pixel of the tie for the peak, stream 0 and stream 1


@functools.lru_cache(maxsize=None)
def big_activity():
    """1024x342, S = 2, T = 2 -> the four segments.  Stream 0: every byte, then 300 single bytes of distinct pixels; stream 1:
    every third byte (channel 0 of every pixel), then 1009 bytes (a prime) of distinct pixels."""
    S, T = 2, 2
    assert N4 == 1050624 and ws.tiles(N4) == 257
    segments = list(frozen(np.arange(N4), 3 * (PEAK0 + 997 * np.arange(300)) + 1, np.arange(0, N4, 3),
                           3 * (PEAK1 + 277 * np.arange(1009)) + 2))
    assert all(x[-1] < N4 for x in segments)
    off, xs, _ = packed(segments)
    assert len(segments[0]) == N4 > 4 * ENTRY_ROUND and -(-int(off[-1]) // ENTRY_ROUND) == 6, "five rounds for record 0 alone"
    assert all(len(segments[3]) % d for d in range(2, 32)) and len(segments[3]) < 32 * 32, "a prime count of entries"
    edge = int(off[2])                                               # the first entry of stream 1
    assert edge % 64 and edge % ENTRY_ROUND and int(off[3]) % 64, "the stream boundary falls inside a wave, and inside a round"
    ncells = activity_cells(W4, H4, 1, 1)[0]
    assert ncells == 350208 and S * ncells == 700416 > CLEAR_PASS, "a second pass of k_act_clear"
    cells, summ = oracle(W4, H4, 1, 1, 2, S, T, off, xs)
    assert list(summ[0]) == [N4 + 300, 0, 0, W4 - 1, H4 - 1, ncells, 4, PEAK0] and int((cells[0] == 4).sum()) == 300
    assert list(summ[1, 5:]) == [1009, 2, PEAK1] and int((cells[1] == 2).sum()) == 1009, "a tie for the peak, at the least index"
    assert PEAK1 > 256 and summ[1, 0] == N4 // 3 + 1009
    return segments


@pytest.mark.parametrize("cell", BIG_CELLS, ids=lambda c: "cell%dx%d" % c)
def test_activity_of_a_large_frame(cell):
    """Both forms, identical outputs, equal to the oracle.  1x1: 350 208 cells per stream (k_act_clear's second pass over the
    pattern, k_act_summary's longest scan); 5000x5000: one cell."""
    S, T = 2, 2
    segments = big_activity()
    with CUDACore(W4, H4, max_batch=S * T) as core:
        cells, summ = both_forms(core, W4, H4, cell + (2,), S, T, segments)
    assert int(cells.sum()) == sum(len(x) for x in segments)
    if cell == (1, 1):
        assert list(summ[:, 6]) == [4, 2] and list(summ[:, 7]) == [PEAK0, PEAK1]
    if cell == (5000, 5000):
        assert cells.shape == (S, 1) and (summ[:, 7] == 0).all()


def test_activity_accumulates_onto_a_large_frame():
    """1x1 cells: the call, then one accumulating call of the same records on top of its result, against the oracle's `onto`;
    the row behind the last stream keeps the pattern."""
    S, T, geom = 2, 2, (1, 1, 2)
    segments = big_activity()
    off, xs, df = packed(segments)
    ncells = activity_cells(W4, H4, 1, 1)[0]
    want = oracle(W4, H4, 1, 1, 2, S, T, off, xs)
    twice = oracle(W4, H4, 1, 1, 2, S, T, off, xs, onto=want)
    assert np.array_equal(twice[0], 2 * want[0]) and list(twice[1][:, 6]) == [8, 4] and list(twice[1][:, 7]) == [PEAK0, PEAK1]
    recs, _ = spec.encode(off, xs, df)
    hdr = spec.headers(recs, S * T)
    with CUDACore(W4, H4, max_batch=S * T) as core:
        for form in ("arrays", "compact"):
            out = Outputs(S + 1, ncells)
            for accumulate, expect in ((False, want), (True, twice)):
                if form == "arrays":
                    run_arrays(core, geom, S, T, off, xs, out, accumulate=accumulate)
                else:
                    run_compact(core, geom, S, T, recs, hdr, out, accumulate=accumulate)
                got = out.get(S)
                assert np.array_equal(got[1], expect[1]), (form, accumulate, got[1], expect[1])
                assert np.array_equal(got[0], expect[0]), (form, accumulate)


MANY = [(8191, 1), (8192, 1), (64, 128), (4096, 2)]


@functools.lru_cache(maxsize=None)
def many_segments(S, T):
    """15x1: S * T records of 0 to 5 entries, every seventh empty."""
    n, B = 45, S * T
    rng = np.random.default_rng(S + T)
    segments = [np.sort(rng.choice(n, 0 if b % 7 == 3 else 1 + b % 5, replace=False)) for b in range(B)]
    frozen(*segments)
    words = B + 1
    if (S, T) == (8191, 1):
        assert words == LDS_WORDS, "8192 offset words: the largest launch that searches them in LDS"
    else:
        assert words == LDS_WORDS + 1, "8193 offset words: searched where they are"
    sizes = np.array([len(x) for x in segments])
    assert set(sizes) == set(range(6)) and not sizes[3::7].any() and sizes[-1] > 0 and sizes[:T].sum() > 0
    assert sizes.sum() < ENTRY_ROUND
    return segments


@pytest.mark.parametrize("geom", [(4, 1, 2), (1, 1, 1)], ids=lambda g: "cell%dx%d" % g[:2])
@pytest.mark.parametrize("S,T", MANY)
def test_activity_of_many_segments(S, T, geom):
    """15x1 at max_batch = 8192, both forms: the offsets of 8191 segments are searched in LDS, those of 8192 where they are."""
    w, h = 15, 1
    segments = many_segments(S, T)
    with CUDACore(w, h, max_batch=LDS_WORDS) as core:
        both_forms(core, w, h, geom, S, T, segments)

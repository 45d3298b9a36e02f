"""-m gpu: mi355_cwire_coalesce_batch / _cwire_batch and mi355_cwire_budget_cwire_batch past the fixed counts at which their
kernels and the budget call's host loop start another round (csrc/stream_ops.hip):
    k_cwc_scan      256 tiles of 4096 bytes per round: frames above 1 MiB; the carries n, e, end and two alternating sets of LDS words
    k_cwc_place     1024 streams per round, offsets and frame_pos scanned in place; the carries first, pos
    k_cwb_init      128 budgets per launch (kCwbInitStreams), h.first the row of the launch's first stream
    k_cwb_thr       the ends of its range: core thresholds 254 and 255, one magnitude only, one bin that holds every byte
Frames above 1 MiB carry sparse crafted records (and two dense tiles), the many-stream cases use tiny frames.

Everything is compared np.array_equal with numpy: cwire_spec for the format, a uint8 sum per byte index for the coalescer
(test_cwire_coalesce_gpu.reference), a histogram of |cur - pre| for the threshold (test_cwire_budget_gpu.threshold_for),
spec.encode of the entries above it for the record and `pre at every dropped index` for the state.  Every buffer the GPU sees is
guarded (gpu_util.Guarded / Region) and starts as a non-zero pattern.  Before the GPU is touched each case asserts, from the
reference alone, that its input reaches the seam it is there for."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_bytes_max
from gpu_util import CUDACore, Guarded, Region
from test_cwire_budget_gpu import NOLIMIT, diff_tick, threshold_for
from test_cwire_coalesce_gpu import check_both_forms, packed, reference, run_arrays, run_compact

pytestmark = pytest.mark.gpu

K = 4096                      # bytes of a tile
ROUND = 256 * K               # bytes of a round of k_cwc_scan
PLACE = 1024                  # streams of a round of k_cwc_place
INIT = 128                    # streams of a k_cwb_init launch
SHAPES = {257: (1024, 342), 513: (1024, 683)}   # tiles: (w, h); the last tile holds 2048 / 1024 bytes
E = ([], [])


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def seam_tiles(n):
    """The tiles that start a round of k_cwc_scan behind the first: [256] at 257 tiles, [256, 512] at 513."""
    return list(range(256, -(-n // K), 256))


# ---- 1. tile-round seams, coalescer ---------------------------------------------------------------------------------------
def gap_across(n, g):
    """The last entry of tile r - 1 and the next one exactly g bytes on in tile r, for every round seam r; a decoy in between
    comes and goes."""
    a = [r * K - 100 for r in seam_tiles(n)]
    b = [x + g + 1 for x in a]
    both = sorted(a + b)
    return [([50] + both, [3] + [1 + i for i in range(len(both))]), ([x + 10 for x in a], [9] * len(a)),
            ([x + 10 for x in a], [247] * len(a)), E]


def tile_streams(n):
    """[(what, [T = 4 records as (xs, diff)])] on a frame of n bytes; the checks of tile_case say what each is for.
    At 257 tiles tile 256 is the last one and holds 2048 bytes, so two kinds are partial there: round 1 cannot hold a dense tile
    of 4096 entries with entries behind it (its first 1024 bytes are dense, two entries follow), and the cancelled tile 256 has
    entries in front of it only.  Both are whole at 513 tiles."""
    nt, R = -(-n // K), seam_tiles(n)
    last_len = n - (nt - 1) * K
    edges = sorted([x for r in R for x in (r * K - 1, r * K)])
    every = np.arange(nt) * K + np.arange(nt) + 300           # one per tile, 4097 apart
    assert every[-1] < n
    dense0 = 3 * K + np.arange(K)                              # tile 3, whole
    dense1 = (257 * K + np.arange(K)) if nt > 258 else (256 * K + np.arange(1024))
    behind0 = [100 * K + 7, 255 * K + 4095]
    behind1 = [400 * K + 1, 511 * K + 4095, 512 * K, n - 1] if nt > 258 else [256 * K + 1500, n - 1]
    t256 = 256 * K + np.arange(0, min(K, last_len) if nt == 257 else K, 50)
    sides = [255 * K + 4000] + ([257 * K + 3, 512 * K + 1] if nt > 258 else [])
    gone = sorted([0, 2 * K + 1, n - 1] + edges)
    return [
        ("entries at the last byte of a round's last tile and the first byte of the next round's first",
         [([0] + edges + [n - 1], [1] * (len(edges) + 2)), (edges[::2], [5] * len(edges[::2])), E, ([0, 7], [255, 9])]),
        ("a gap of 254 across a round seam", gap_across(n, 254)),
        ("a gap of 255 across a round seam", gap_across(n, 255)),
        ("a gap of 256 across a round seam", gap_across(n, 256)),
        ("two entries only, in tile 2 and in the last tile",
         [([2 * K + 17], [200]), ([9 * K, (nt - 1) * K + 5], [4, 1]), ([2 * K + 17], [100]), ([9 * K], [252])]),
        ("an empty stream", [E, E, E, E]),
        ("a first entry in the second round",
         [([100], [5]), ([100, 256 * K + 1000], [251, 8]), ([256 * K + 1003], [1]), E]),
        ("a stream that cancels completely",
         [(gone, [1 + i for i in range(len(gone))]), (gone[::2], [255 - 2 * i for i in range(len(gone[::2]))]),
          (gone[1::2], [254 - 2 * i for i in range(len(gone[1::2]))]), E]),
        ("a dense tile in round 0 and a dense run in round 1, sparse entries behind them",
         [(np.concatenate([dense0, behind0]), np.concatenate([1 + dense0 % 200, [1, 2]])),
          (np.concatenate([dense1, behind1]), np.concatenate([1 + dense1 % 199, 1 + np.arange(len(behind1))])),
          (dense0[::5], np.full(len(dense0[::5]), 20)), E]),
        ("tile 256 cancelled whole",
         [(np.concatenate([[255 * K + 4000], t256]), np.concatenate([[1], 1 + np.arange(len(t256)) % 200])),
          (t256, 255 - np.arange(len(t256)) % 200), (sides, [1] * len(sides)), E]),
        ("one entry in every tile, every gap escaped",
         [(every[::2], 1 + np.arange(len(every[::2])) % 255), (every[1::2], 1 + np.arange(len(every[1::2])) % 254),
          (every[::3], np.full(len(every[::3]), 1)), E]),
    ]


@functools.lru_cache(maxsize=None)
def tile_case(nt):
    """(n, S, T, records, reference) of the shape with nt tiles, made once and read-only; asserts from the reference that every
    kind of stream is what its name says."""
    w, h = SHAPES[nt]
    n, T = 3 * w * h, 4
    assert -(-n // K) == nt and n > ROUND * ((nt - 1) // 256), "the last round is one ragged tile"
    streams = tile_streams(n)
    S = len(streams)
    recs, _ = spec.encode(*packed([seg for _, segs in streams for seg in segs]))
    want = reference(recs, S, T, n)
    woff, wxs, wdf, wrecs, wpos = want
    R = seam_tiles(n)
    kept = {what: wxs[int(woff[s]):int(woff[s + 1])].astype(np.int64) for s, (what, _) in enumerate(streams)}
    size = {what: int(wpos[s + 1] - wpos[s]) for s, (what, _) in enumerate(streams)}

    def escapes(x):
        return int((spec.gaps(x) >= 255).sum())

    x = kept["entries at the last byte of a round's last tile and the first byte of the next round's first"]
    assert all(r * K - 1 in x and r * K in x for r in R) and 0 not in x
    for g in (254, 255, 256):
        x = kept[f"a gap of {g} across a round seam"]
        gp = spec.gaps(x)
        for r in R:
            i = int(np.searchsorted(x, r * K))                 # the first entry of tile r
            assert x[i - 1] // K == r - 1 and x[i] // K == r and gp[i] == g, (g, r)
        assert escapes(x) == (2 if g >= 255 else 1) * len(R), "only the seams' gaps differ between the three"
    x = kept["two entries only, in tile 2 and in the last tile"]
    assert list(x // K) == [2, nt - 1] and escapes(x) == 2
    if nt == 513:
        assert x[0] < ROUND and x[1] >= 2 * ROUND, "round 1 is empty: end and e cross it"
    for what in ("an empty stream", "a stream that cancels completely"):
        assert kept[what].size == 0 and size[what] == 8, what
    x = kept["a first entry in the second round"]
    assert x.size == 2 and x[0] >= ROUND and spec.gaps(x)[0] >= 255
    x = kept["a dense tile in round 0 and a dense run in round 1, sparse entries behind them"]
    assert int((x // K == 3).sum()) == K and int((x < ROUND).sum()) > K, "nbefore at the seam is above a tile's worth"
    assert (x // K == 255).any() and x[-1] == n - 1 and int((x >= ROUND).sum()) >= 1024 + 2
    if nt == 513:
        assert int((x // K == 257).sum()) == K and int((x < 2 * ROUND).sum()) > 2 * K and int((x >= 2 * ROUND).sum()) == 2
    x = kept["tile 256 cancelled whole"]
    assert not (x // K == 256).any() and (x // K == 255).any() and (nt == 257 or ((x // K == 257).any() and (x // K == 512).any()))
    x = kept["one entry in every tile, every gap escaped"]
    assert x.size == nt and np.array_equal(x // K, np.arange(nt)) and escapes(x) == nt, "e carries n"
    assert size["one entry in every tile, every gap escaped"] > 8, "the last record has bytes (test_tile_round_capacity)"
    return (n, S, T) + frozen(recs) + (frozen(*want),)


@pytest.mark.parametrize("nt", sorted(SHAPES))
def test_tile_rounds_coalesce(nt):
    """257 tiles: the second round of k_cwc_scan is one ragged tile of 2048 bytes; 513 tiles: the third round, one ragged tile
    of 1024 bytes, is the first that takes a set of LDS words a second time."""
    w, h = SHAPES[nt]
    n, S, T, recs, _ = tile_case(nt)
    with CUDACore(w, h, max_batch=S * T) as core:
        check_both_forms(core, recs, S, T, n)                  # (the GPU against the reference, inside)


def test_tile_round_capacity():
    """513 tiles.  Exactly the needed bytes pass; with one byte fewer the last record -- 513 entries, one per tile -- is
    skipped whole, the earlier ones are intact, offsets and frame_pos exact.  Arrays form: one entry short likewise."""
    nt = 513
    w, h = SHAPES[nt]
    n, S, T, recs, (woff, wxs, wdf, wrecs, wpos) = tile_case(nt)
    hdr = spec.headers(recs, S * T)
    need, fit = int(wpos[S]), int(wpos[S - 1])
    with CUDACore(w, h, max_batch=S * T) as core:
        for cap in (need, need - 1):
            off, pos, out = run_compact(core, recs, hdr, S, T, n, cap=cap)
            assert out.size == cap and np.array_equal(off, woff) and np.array_equal(pos, wpos), cap
            if cap == need:
                assert np.array_equal(out, wrecs)
            else:
                assert np.array_equal(out[:fit], wrecs[:fit]) and (out[fit:] == 0x5C).all(), "the last record is skipped whole"
        tot = int(woff[S])
        off, xs, df = run_arrays(core, recs, hdr, S, T, n, cap=tot - 1, skew=3)
        assert np.array_equal(off, woff) and np.array_equal(xs, wxs[:tot - 1]) and np.array_equal(df, wdf[:tot - 1])


# ---- the budget call against numpy ----------------------------------------------------------------------------------------
def numpy_tick(pre, cur, thr0):
    """One tick of S streams at threshold thr0, stated in numpy -> (records, frame_pos, counts, escapes, states after,
    per stream (xs, diff, a)): the entries are the bytes with a = |cur - pre| > thr0, the state takes cur there."""
    S = len(pre)
    ent = []
    for s in range(S):
        a = np.abs(cur[s].astype(np.int64) - pre[s].astype(np.int64))
        x = np.flatnonzero(a > thr0)
        ent.append((x, (cur[s][x] - pre[s][x]).astype(np.uint8), a[x]))
    recs, pos = spec.encode(*packed([(x, d) for x, d, _ in ent]))
    counts, escapes = spec.headers(recs, S)
    post = np.where(np.abs(cur.astype(np.int64) - pre.astype(np.int64)) > thr0, cur, pre).astype(np.uint8)
    return frozen(recs, pos, counts, escapes, post) + (ent,)


def gpu_tick(w, h, pre, cur, thr0):
    """numpy_tick, the records and states made by mi355_diff_multi_cwire_batch on a fresh core and equal to numpy's."""
    tk = numpy_tick(pre, cur, thr0)
    recs, pos, _, post = diff_tick(w, h, thr0, pre, cur)
    assert np.array_equal(recs, tk[0]) and np.array_equal(pos, tk[1]) and np.array_equal(post, tk[4])
    return frozen(recs, pos) + tk[2:]


def budget_of(kind, n):
    return {"nolimit": NOLIMIT, "n": n, "n-1": max(n - 1, 0), "half": n // 2, "eighth": n // 8, "zero": 0}[kind]


def expected(tk, pre, thr0, budgets):
    """-> (thresholds uint32[S], offsets uint32[S + 1], frame_pos uint64[S + 1], records, states [S][n], kept masks)."""
    post, ent = tk[4], tk[5]
    thr, segs, states, keeps = [], [], [], []
    for s, (x, d, a) in enumerate(ent):
        T = threshold_for(a, thr0, int(budgets[s]))
        keep = a > T
        assert int(keep.sum()) <= int(budgets[s]) and (T == thr0) == (int(budgets[s]) >= len(a))
        state = post[s].copy()
        state[x[~keep]] = pre[s][x[~keep]]
        thr.append(T); segs.append((x[keep], d[keep])); states.append(state); keeps.append(keep)
    off, xs, df = packed(segs)
    recs, pos = spec.encode(off, xs, df)
    return np.array(thr, np.uint32), off, pos, recs, np.stack(states), keeps


def run_budget(core, tk, n, budgets, cap=None):
    """-> (thresholds, offsets, frame_pos, the whole output buffer, states [S][n]); every guard asserted."""
    recs, _, counts, escapes, post, _ = tk
    S = len(post)
    cap = cwire_bytes_max(n, S) if cap is None else cap
    st = Region(S, n).put(post)
    src = Guarded(recs.size, torch.uint8, data=recs)
    thr, off, pos, out = Guarded(S, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_budget_cwire_batch(src.ptr, counts, escapes, st.ptr, S, np.asarray(budgets, np.uint32), thr.ptr, off.ptr, pos.ptr,
                                  out.ptr, cap, stride=st.stride)
    core.synchronize()
    assert np.array_equal(src.get(), recs), "the input records were written"
    return thr.get().view(np.uint32), off.get().view(np.uint32), pos.get().view(np.uint64), out.get(), st.get()


def check_budget(core, tk, n, budgets, want):
    thr, off, pos, out, states = run_budget(core, tk, n, budgets)
    what = [int(b) for b in budgets[:8]]
    assert np.array_equal(thr, want[0]), what
    assert np.array_equal(off, want[1]) and np.array_equal(pos, want[2]), what
    assert np.array_equal(out[:want[3].size], want[3]), what
    assert (out[want[3].size:] == 0x5C).all(), (what, "written behind the last record")
    assert np.array_equal(states, want[4]), what


# ---- 2. tile-round seams, budget call -------------------------------------------------------------------------------------
def seam_cluster(n):
    """The bytes around every round seam: 150 on either side, and those 255, 256 and 600 bytes off."""
    off = np.concatenate([np.arange(-150, 150), [-600, -256, -255, 255, 256, 600]])
    x = np.unique(np.concatenate([r * K + off for r in seam_tiles(n)]))
    assert x[-1] < n
    return x


def spread(n, count, phase):
    """count indices over the whole frame, none within 700 bytes of a round seam."""
    c = np.unique(np.linspace(100 + phase, n - 200, 3 * count).astype(np.int64))
    c = c[np.all([np.abs(c - r * K) > 700 for r in seam_tiles(n)], axis=0)]
    return c[np.linspace(0, c.size - 1, count).astype(np.int64)]


ISO = 2 * K + 500             # the kept entry among dropped neighbours


@functools.lru_cache(maxsize=None)
def tile_tick(nt):
    """(n, pre [3][n], the tick at threshold 20 and what each stream is made of), once per shape and read-only.
    Stream 0: the seam clusters low, as many entries elsewhere high; stream 1: the clusters and ISO high, as many low, twelve of
    them around ISO; stream 2: one entry per tile, the magnitudes cycling."""
    w, h = SHAPES[nt]
    n = 3 * w * h
    cl = seam_cluster(n)
    pre = np.tile((50 + np.arange(n) % 50).astype(np.uint8), (3, 1))
    cur = pre.copy()
    far0 = spread(n, cl.size, 0)
    cur[0][cl] += (21 + np.arange(cl.size) % 30).astype(np.uint8)
    cur[0][far0] += (100 + np.arange(far0.size) % 50).astype(np.uint8)
    run = np.setdiff1d(np.arange(ISO - 6, ISO + 7), [ISO])
    far1 = np.union1d(run, spread(n, cl.size + 1 - run.size, 33))
    high1 = np.union1d(cl, [ISO])
    assert far1.size == high1.size and not np.intersect1d(far1, high1).size and not np.intersect1d(far0, cl).size
    cur[1][high1] += (90 + np.arange(high1.size) % 60).astype(np.uint8)
    cur[1][far1] += (21 + np.arange(far1.size) % 40).astype(np.uint8)
    every = np.arange(nt) * K + np.arange(nt) + 300
    cur[2][every] += (21 + (np.arange(nt) * 37) % 130).astype(np.uint8)
    tk = gpu_tick(w, h, pre, cur, 20)
    return (n,) + frozen(pre, cur, cl, far0, high1, far1) + (tk,)


@functools.lru_cache(maxsize=None)
def reference_core(nt, s, T):
    """Stream s of tile_tick(nt) diffed by a fresh core of threshold T -> (record, n, state after)."""
    w, h = SHAPES[nt]
    pre, cur = tile_tick(nt)[1:3]
    rec, _, off, st = diff_tick(w, h, T, pre[s:s + 1], cur[s:s + 1])
    return rec, int(off[1]), st[0]


@pytest.mark.parametrize("nt", sorted(SHAPES))
def test_tile_rounds_budget(nt):
    """S = 3 at max_batch = 3, two calls on one core: budgets (half, half, zero) and (no limit, zero, half)."""
    w, h = SHAPES[nt]
    n, pre, _, cl, far0, high1, far1, tk = tile_tick(nt)
    ent = tk[5]
    R = seam_tiles(n)
    ns = [len(x) for x, _, _ in ent]
    assert ns == [2 * cl.size, 2 * high1.size, nt]
    calls = [[ns[0] // 2, ns[1] // 2, 0], [NOLIMIT, 0, ns[2] // 2]]
    wants = [expected(tk, pre, 20, b) for b in calls]
    # call 1, stream 0 drops exactly the entries around the round seams, stream 1 keeps exactly those (and ISO)
    k0, k1 = ent[0][0][wants[0][5][0]], ent[1][0][wants[0][5][1]]
    assert np.array_equal(k0, far0) and np.array_equal(k1, high1)
    for r in R:
        assert not ((k0 >= r * K - 700) & (k0 <= r * K + 700)).any() and (k0 < r * K).any() and (k0 >= r * K).any()
        assert r * K - 1 in k1 and r * K in k1
    i_in, i_out = int(np.searchsorted(ent[1][0], ISO)), int(np.searchsorted(k1, ISO))
    assert spec.gaps(ent[1][0])[i_in] == 0 and spec.gaps(k1)[i_out] >= 255, "an escape the input did not have"
    assert wants[0][0][2] == ent[2][2].max() and wants[0][2][3] - wants[0][2][2] == 8, "budget 0: an empty record"
    assert np.array_equal(wants[0][4][2], pre[2]) and np.array_equal(wants[1][4][1], pre[1])
    assert wants[1][0][0] == 20 and np.array_equal(wants[1][4][0], tk[4][0]), "no limit: the core's threshold, the state as it was"
    k2 = ent[2][0][wants[1][5][2]]
    assert 0 < k2.size <= nt // 2 and (k2 < ROUND).any() and (k2 >= R[-1] * K).any(), "kept entries in the first and last round"
    # the reference core, one per distinct (stream, threshold)
    for want in wants:
        for s in range(3):
            T = int(want[0][s])
            if T == 20:
                continue
            rec, cnt, state = reference_core(nt, s, T)
            assert cnt == int(want[1][s + 1] - want[1][s]) and np.array_equal(state, want[4][s])
            assert np.array_equal(rec, want[3][int(want[2][s]):int(want[2][s + 1])])
    with CUDACore(w, h, max_batch=3, threshold=20) as core:
        for budgets, want in zip(calls, wants):
            check_budget(core, tk, n, budgets, want)


# ---- 3. stream-round seams ------------------------------------------------------------------------------------------------
def round_starts(S, size):
    """The first stream of every round of `size` streams behind the first."""
    return tuple(range(size, S, size))


def is_empty(s, starts):
    return s % 7 == 3 or s in starts


def many_records(n, S, T, starts=None):
    """Records that vary by stream; empty ones at s % 7 == 3 and at `starts` (default: the first stream of every later round of
    k_cwc_place).  A second record takes back every other entry of the first (odd s) or is drawn afresh (even s)."""
    starts = round_starts(S, PLACE) if starts is None else starts
    rng = np.random.default_rng(10 * S + T)
    segs = []
    for s in range(S):
        cnt = 0 if is_empty(s, starts) else 1 + (5 * s) % 23
        x, d = np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)
        segs.append((x, d))
        for t in range(1, T):
            if s % 2:
                segs.append((x[::2], (256 - d[::2]) % 256))
            else:
                segs.append((np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)))
    return packed(segs)


def check_seams(S, off, pos, size):
    """There are entries and bytes in front of every seam and bytes behind it (a total that lost a round's cannot be right);
    entries behind it too wherever more than the seam's own stream, an empty one, follows."""
    seams = list(round_starts(S, size))
    for seam in seams:
        assert int(pos[seam]) != 0 and int(pos[S]) != int(pos[seam]) and int(off[seam]) != 0
        assert S - seam == 1 or int(off[S]) != int(off[seam]), seam
    return seams


@pytest.mark.parametrize("S,T", [(1024, 1), (1025, 1), (1025, 2), (2050, 1)])
def test_stream_rounds_coalesce(S, T):
    """1024: one full round of k_cwc_place and no second; 1025: a second round of one stream, an empty one; 2050: three rounds."""
    w, h = 33, 7
    n = 3 * w * h
    recs, _ = spec.encode(*many_records(n, S, T))
    woff, wxs, wdf, wrecs, wpos = reference(recs, S, T, n)
    seams = check_seams(S, woff, wpos, PLACE)
    assert len(seams) == (S - 1) // PLACE and all(wpos[s + 1] - wpos[s] == 8 for s in seams)
    if T > 1:
        assert int(woff[S]) < spec.headers(recs, S * T)[0].sum(), "entries were taken back"
    with CUDACore(w, h, max_batch=S * T) as core:
        check_both_forms(core, recs, S, T, n)


def test_stream_round_capacity():
    """S = 1025: the room ends inside record 1024, the second round's.  The records before it are exact, it is skipped whole."""
    w, h, S = 33, 7, 1025
    n = 3 * w * h
    recs, _ = spec.encode(*many_records(n, S, 1, starts=()))
    hdr = spec.headers(recs, S)
    woff, wxs, wdf, wrecs, wpos = reference(recs, S, 1, n)
    check_seams(S, woff, wpos, PLACE)
    assert int(woff[S]) != int(woff[1024]), "record 1024 has entries"
    fit, cap = int(wpos[1024]), int(wpos[1024]) + 12
    assert fit + 8 < cap < int(wpos[S])
    with CUDACore(w, h, max_batch=S) as core:
        off, pos, out = run_compact(core, recs, hdr, S, 1, n, cap=cap)
    assert out.size == cap and np.array_equal(off, woff) and np.array_equal(pos, wpos)
    assert np.array_equal(out[:fit], wrecs[:fit]) and (out[fit:] == 0x5C).all()


ORDER = ("nolimit", "half", "n-1", "zero", "eighth")


def many_ticks(n, S):
    """(pre [S][n], cur [S][n]): stream s changes 5 + 3s mod 31 bytes by magnitudes from 21 to 60; none at s % 7 == 3
    and at the first stream of the second k_cwb_init launch and of every later round of k_cwc_place."""
    starts = (INIT,) + round_starts(S, PLACE)
    rng = np.random.default_rng(S)
    pre = rng.integers(60, 196, (S, n), dtype=np.uint8)
    cur = pre.copy()
    for s in range(S):
        if is_empty(s, starts):
            continue
        x = rng.choice(n, 5 + (3 * s) % 31, replace=False)
        a = rng.integers(21, 61, x.size)
        cur[s][x] = pre[s][x] + np.where(rng.random(x.size) < 0.5, a, -a)
    return pre, cur


@pytest.mark.parametrize("w,h,S", [(33, 7, 128), (33, 7, 129), (33, 7, 257), (15, 1, 1025)])
def test_stream_rounds_budget(w, h, S):
    """128: one full k_cwb_init launch; 129, 257: a second and third launch whose h.first is not 0; 1025: nine launches and the
    second round of k_cwc_place.  The budgets go nolimit, half, n - 1, zero, eighth, shifted by one per launch, so that a row
    which took another launch's budget of the same lane gives another threshold."""
    n = 3 * w * h
    pre, cur = many_ticks(n, S)
    tk = numpy_tick(pre, cur, 20)
    ent = tk[5]
    budgets = np.array([budget_of(ORDER[(s + s // INIT) % 5], len(ent[s][0])) for s in range(S)], np.uint32)
    want = expected(tk, pre, 20, budgets)
    assert len(check_seams(S, want[1], want[2], INIT)) == (S - 1) // INIT
    assert len(check_seams(S, want[1], want[2], PLACE)) == (S - 1) // PLACE
    for b0 in range(0, S - INIT + 1, INIT):                # every whole block of 128 streams
        blk = want[0][b0:b0 + INIT]
        assert (blk > 20).any() and (blk == 20).any(), b0
    # were every launch's budgets written to rows 0 .., row j would hold those of the last launch that has a lane j
    moved = [j for j in range(min(INIT, S - INIT)) if threshold_for(ent[j][2], 20, int(budgets[(S - 1 - j) // INIT * INIT + j])) != want[0][j]]
    assert bool(moved) == (S > INIT), "a row that took another stream's budget gives another threshold"
    assert len(set(int(t) for t in want[0])) > 10
    with CUDACore(w, h, max_batch=S, threshold=20) as core:
        check_budget(core, tk, n, budgets, want)


# ---- 4. the ends of k_cwb_thr's range, at 64x48 ---------------------------------------------------------------------------
W4, H4, N4 = 64, 48, 3 * 64 * 48


def edge_tick(thr0, pre, cur):
    return gpu_tick(W4, H4, np.stack(pre), np.stack(cur), thr0)


def test_threshold_254_leaves_magnitude_255_alone():
    """Every entry has a = 255 (0 -> 255 and 255 -> 0); the bytes that change by 254 are no entries.  Budget n keeps all of them
    at T = 254; n - 1 and 0 keep none, at T = 255."""
    rng = np.random.default_rng(254)
    pre, cur = [], []
    for s in range(3):
        p = np.where(rng.random(N4) < 0.5, 255, 0).astype(np.uint8)
        c = p.copy()
        x = rng.choice(N4, 900 + s, replace=False)
        c[x[:300 + s]] = 255 - p[x[:300 + s]]
        c[x[300 + s:600]] = np.where(p[x[300 + s:600]] == 255, 1, 254)       # a = 254
        c[x[600:]] = np.where(p[x[600:]] == 255, 155, 100)                    # a = 100
        pre.append(p); cur.append(c)
    tk = edge_tick(254, pre, cur)
    ns = [len(x) for x, _, _ in tk[5]]
    assert ns == [300, 301, 302] and all((a == 255).all() for _, _, a in tk[5])
    budgets = [ns[0], ns[1] - 1, 0]
    want = expected(tk, np.stack(pre), 254, budgets)
    assert list(want[0]) == [254, 255, 255] and list(np.diff(want[1].astype(np.int64))) == [300, 0, 0]
    assert np.array_equal(want[4][0], tk[4][0]) and np.array_equal(want[4][1:], np.stack(pre)[1:])
    with CUDACore(W4, H4, max_batch=3, threshold=254) as core:
        check_budget(core, tk, N4, budgets, want)


def test_threshold_255_has_nothing_to_thin():
    rng = np.random.default_rng(255)
    pre = [rng.integers(0, 256, N4, dtype=np.uint8) for _ in range(3)]
    cur = [rng.integers(0, 256, N4, dtype=np.uint8) for _ in range(3)]
    pre[0][:2], cur[0][:2] = (0, 255), (255, 0)
    tk = edge_tick(255, pre, cur)
    assert not tk[2].any() and tk[0].size == 24 and np.array_equal(tk[4], np.stack(pre))
    budgets = [0, NOLIMIT, 5]
    want = expected(tk, np.stack(pre), 255, budgets)
    assert list(want[0]) == [255, 255, 255] and want[3].size == 24
    with CUDACore(W4, H4, max_batch=3, threshold=255) as core:
        check_budget(core, tk, N4, budgets, want)


def test_one_magnitude_only():
    """All magnitudes equal m > thr0 + 1 and the budget is n - 1: every threshold from thr0 to m - 1 keeps all n entries, so
    T = m and the record is empty.  m = 22 is the least such m at thr0 = 20; 255 the largest."""
    rng = np.random.default_rng(7)
    ms = [100, 22, 255, 100]
    pre, cur = [], []
    for m in ms:
        p = np.full(N4, 0 if m == 255 else 77, np.uint8)
        c = p.copy()
        c[rng.choice(N4, 500, replace=False)] += np.uint8(m)
        pre.append(p); cur.append(c)
    tk = edge_tick(20, pre, cur)
    budgets = [499, 499, 499, 500]
    for (x, d, a), m in zip(tk[5], ms):
        assert len(x) == 500 and (a == m).all()
        assert all(int((a > T).sum()) == 500 for T in range(20, m)), "no threshold below m helps"
    want = expected(tk, np.stack(pre), 20, budgets)
    assert list(want[0]) == [100, 22, 255, 20] and list(np.diff(want[1].astype(np.int64))) == [0, 0, 0, 500]
    with CUDACore(W4, H4, max_batch=4, threshold=20) as core:
        check_budget(core, tk, N4, budgets, want)


def test_dense_streams():
    """Every byte of the frame is an entry.  Streams 0, 1: one bin holds all N = 9216 (budgets N - 1 and N).  Streams 2, 3: bin 60
    holds 8716, bins 61, 90, 120, 200 and 255 a hundred each; the budgets 350 and 8000 fall between two cumulative counts."""
    rng = np.random.default_rng(9)
    pre = [np.full(N4, 0, np.uint8) for _ in range(4)]
    pre[1] = rng.integers(0, 196, N4, dtype=np.uint8)
    cur = [p + np.uint8(60) for p in pre]
    other = rng.permutation(N4)[:500].reshape(5, 100)
    for s in (2, 3):
        for x, m in zip(other, (61, 90, 120, 200, 255)):
            cur[s][x] = m
    tk = edge_tick(20, pre, cur)
    assert all(len(x) == N4 for x, _, _ in tk[5])
    hist = np.bincount(tk[5][2][2], minlength=256)
    assert hist[60] == N4 - 500 and np.bincount(tk[5][0][2], minlength=256)[60] == N4
    budgets = [N4 - 1, N4, 350, 8000]
    want = expected(tk, np.stack(pre), 20, budgets)
    assert list(want[0]) == [60, 20, 90, 60] and list(np.diff(want[1].astype(np.int64))) == [0, N4, 300, 500]
    with CUDACore(W4, H4, max_batch=4, threshold=20) as core:
        check_budget(core, tk, N4, budgets, want)


# ---- 5. the workload's own shape ------------------------------------------------------------------------------------------
W5, H5, N5 = 1920, 1080, 3 * 1920 * 1080
MIB = [x for k in range(1, 6) for x in ((k << 20) - 1, k << 20)]


def test_1080p_coalesce():
    """1519 tiles, six rounds of k_cwc_scan, S = 2, T = 2: some 3000 entries per record over the whole frame and at every MiB
    mark; the second record takes back every third entry of the first and brings 1000 new ones."""
    S, T = 2, 2
    assert -(-N5 // K) == 1519 and N5 > 5 * ROUND
    segs = []
    for s in range(S):
        x = np.union1d(np.linspace(300 + s, N5 - 1, 3000).astype(np.int64), MIB)
        d = np.where(np.isin(x, MIB), 1, 1 + np.arange(x.size) % 255)
        new = np.setdiff1d(np.linspace(5000 + 77 * s, N5 - 4000, 1000).astype(np.int64), x)
        back = np.isin(x, np.setdiff1d(x[::3], MIB))          # taken back; the MiB marks stay, every other one summed to 8
        summed = np.setdiff1d(MIB, MIB[s::2])
        x2 = np.concatenate([x[back], summed, new])
        d2 = np.concatenate([(256 - d[back]) % 256, np.full(summed.size, 7), np.full(new.size, 9)])
        o = np.argsort(x2, kind="stable")
        segs += [(x, d), (x2[o], d2[o])]
    recs, _ = spec.encode(*packed(segs))
    woff, wxs, wdf, wrecs, wpos = reference(recs, S, T, N5)
    for s in range(S):
        x = wxs[int(woff[s]):int(woff[s + 1])].astype(np.int64)
        assert 2500 < x.size < len(segs[2 * s][0]) + 1000, "entries were taken back"
        assert np.array_equal(np.unique(x // ROUND), np.arange(6)) and np.isin(MIB, x).all()
        assert (spec.gaps(x) >= 255).sum() > 1000
    with CUDACore(W5, H5, max_batch=S * T) as core:
        check_both_forms(core, recs, S, T, N5)


def test_1080p_budget():
    """S = 2 at 1080p: some 4000 entries per stream over the six rounds and at every MiB mark, budgets half and an eighth."""
    S = 2
    pre = np.tile((40 + np.arange(N5) % 60).astype(np.uint8), (S, 1))
    cur = pre.copy()
    for s in range(S):
        x = np.union1d(np.linspace(900 + 13 * s, N5 - 1, 4000).astype(np.int64), MIB)
        a = 21 + (np.arange(x.size) * (7 + 4 * s)) % 120
        a[np.isin(x, MIB)] = 150                              # the MiB marks survive both budgets
        cur[s][x] += a.astype(np.uint8)
    tk = gpu_tick(W5, H5, pre, cur, 20)
    ns = [len(x) for x, _, _ in tk[5]]
    budgets = [ns[0] // 2, ns[1] // 8]
    want = expected(tk, pre, 20, budgets)
    for s in range(S):
        k = tk[5][s][0][want[5][s]]
        assert 0 < k.size <= budgets[s] and want[0][s] > 20
        assert np.array_equal(np.unique(k // ROUND), np.arange(6)) and np.isin(MIB, k).all()
    with CUDACore(W5, H5, max_batch=S, threshold=20) as core:
        check_budget(core, tk, N5, budgets, want)

"""The filter kernels (csrc/filters.hip) on guarded buffers: every choice their launchers make from the pointers, the
stride, the frame size and the frame count, in place where the header allows it, red_dense at the edges of its
threshold, and frame counts beyond 65535 (the frame is a grid dimension of every filter kernel).

Every frame buffer is a gpu_util.Region and every histogram / threshold buffer a Guarded: their get() asserts each byte in
front of them, behind them and in the stride gaps, so a store that leaves the frame fails the case even where the values
inside it are right.  The references are oracle/pyoracle.py per frame, compared with np.array_equal."""
import numpy as np
import pytest

from cudavideostream_amd import lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from gpu_util import CUDACore, Guarded, Region  # noqa: E402

ONE_INPUT = {"gray_avg": lib.OP_GRAY_AVG, "gray_weighted": lib.OP_GRAY_WEIGHTED, "binarize": lib.OP_BINARIZE,
             "gray_avg_binarize": lib.OP_GRAY_AVG_BINARIZE, "gray_weighted_binarize": lib.OP_GRAY_WEIGHTED_BINARIZE,
             "conv3x3": lib.OP_CONV3X3, "median5x5": lib.OP_MEDIAN5X5}
TWO_INPUT = {"heat_map": lib.OP_HEAT_MAP, "red_dense": lib.OP_RED_DENSE}
OPS = {**ONE_INPUT, **TWO_INPUT}
BINARIZE_OPS = ("binarize", "gray_avg_binarize", "gray_weighted_binarize")

# 67x17:   1139 pixels = one full wave (1024), 7 full lanes, 3 ragged pixels; rows of 201 bytes: generic conv / median
# 64x17:   1088 pixels, no ragged lane; rows of 192 bytes: the strip kernels when everything is aligned
# 131x127: 16637 pixels = one whole histogram workgroup (16384), 15 full lanes, 13 ragged pixels
SHAPES = [(67, 17), (64, 17), (131, 127)]


def n16(n):
    return (n + 15) & ~15


# (skew_in, skew_in2, skew_out, stride - n16)
POINTER_CASES = [
    (0, 0, 0, 16),     # fast path, with ragged tails and gaps
    (0, 0, 0, 21),
    (3, 0, 0, 16),
    (0, 3, 0, 16),     # two-input ops only
    (0, 0, 3, 16),     # fused chains: fast histogram, byte k_binarize_gray1
    (3, 3, 0, 16),     # the reverse mix
    (8, 8, 8, 8),      # median strip kernel still taken at 64x17; conv strip not
    (16, 16, 16, 16),
]


@pytest.fixture(scope="module")
def cores(po):
    """One core per (frame size, max_batch, threshold) for the whole module."""
    made = {}

    def get(w, h, T, thr=20):
        if (w, h, T, thr) not in made:
            made[(w, h, T, thr)] = CUDACore(w, h, k=po.gaussian_kernel(3, 1.5), max_batch=T, threshold=thr)
        return made[(w, h, T, thr)]

    yield get
    for core in made.values():
        core.close()


def binarize_frames(T, npix, seed):
    """Colour frames for the binarize ops: noise 0..31 plus a ramp (15 per pixel, modulo 224), so that any 16 consecutive
    pixels hold a gray value below 46 and one above 208 -- either side of every threshold in [50, 200]; the first third of
    the pixels is flat at 100 / 170 / 250 (frames 0 to 2; 60 + 37 t % 190 in longer batches, so that frames a few apart have
    thresholds far apart): that bin is the histogram's maximum, which puts the two-max threshold below 100 in one frame and
    above 124 in another."""
    rng = np.random.default_rng(seed)
    ramp = (np.arange(npix) * 15 % 224).astype(np.uint8)
    f = rng.integers(0, 32, (T, npix, 3), dtype=np.uint8) + ramp[None, :, None]
    for t in range(T):
        f[t, :npix // 3] = (100, 170, 250)[t] if t < 3 else 60 + 37 * t % 190
    return f.reshape(T, npix * 3)


def binarized(po, gray3):
    thr = po.two_max_threshold(po.histogram(gray3))
    return po.binarize(gray3, thr), thr


_REF = {}


def reference(po, w, h, T=3):
    """Inputs and per-frame oracle results of every op at one frame size: computed once, shared, never written."""
    if (w, h, T) in _REF:
        return _REF[(w, h, T)]
    n = 3 * w * h
    rng = np.random.default_rng(1000 * w + h)
    cur = rng.integers(0, 256, (T, n), dtype=np.uint8)
    prev = cur.copy()                      # half the bytes differ, by -40 .. 40
    move = rng.random((T, n)) < 0.5
    prev[move] = np.clip(cur[move].astype(np.int32) + rng.integers(-40, 41, int(move.sum())), 0, 255).astype(np.uint8)
    bcur = binarize_frames(T, n // 3, seed=w + h)
    gray3 = np.stack([po.gray_avg(f) for f in bcur])
    k3 = po.gaussian_kernel(3, 1.5)
    r = {"in": {op: cur for op in OPS}, "in2": prev, "want": {}, "thr": {}}
    r["in"].update({"binarize": gray3, "gray_avg_binarize": bcur, "gray_weighted_binarize": bcur})
    r["want"]["gray_avg"] = np.stack([po.gray_avg(f) for f in cur])
    r["want"]["gray_weighted"] = np.stack([po.gray_weighted(f) for f in cur])
    r["want"]["conv3x3"] = np.stack([po.conv3x3(f, w, h, k3) for f in cur])
    r["want"]["median5x5"] = np.stack([po.median5x5(f, w, h) for f in cur])
    r["want"]["heat_map"] = np.stack([po.heat_map(c, p) for c, p in zip(cur, prev)])
    r["want"]["red_dense"] = np.stack([po.red_dense(c, p, 20) for c, p in zip(cur, prev)])
    for op, grays in (("binarize", gray3), ("gray_avg_binarize", gray3),
                      ("gray_weighted_binarize", [po.gray_weighted(f) for f in bcur])):
        outs = [binarized(po, g) for g in grays]
        r["want"][op] = np.stack([o for o, _ in outs])
        r["thr"][op] = [t for _, t in outs]
    for a in (cur, prev, bcur, gray3, *r["want"].values()):
        a.setflags(write=False)
    _REF[(w, h, T)] = r
    return r


def check_binarize_inputs(r, op):
    """From the oracle alone: every frame's result has 0 and 255 among its last 16 pixels (a ragged tail binarized with
    the wrong threshold, or not at all, shows), and the frames of the batch do not share one threshold."""
    for t, want in enumerate(r["want"][op]):
        tail = want[-48:]
        assert (tail == 0).any() and (tail == 255).any(), (op, t)
    assert len(set(r["thr"][op])) >= 2, (op, r["thr"][op])


# ---- A. the dispatch matrix ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("w,h", SHAPES)
def test_filter_batch_dispatch(po, cores, w, h, op):
    """mi355_filter_batch, T = 3, over the pointer and stride cases its launchers choose their kernels from."""
    T, n = 3, 3 * w * h
    r = reference(po, w, h)
    if op in BINARIZE_OPS:
        check_binarize_inputs(r, op)
    core = cores(w, h, T)
    src, src2, want = r["in"][op], r["in2"], r["want"][op]
    for skew_in, skew_in2, skew_out, extra in POINTER_CASES:
        if op not in TWO_INPUT and (skew_in, skew_in2, skew_out, extra) == (0, 3, 0, 16):
            continue   # the same call as the first case
        case = (skew_in, skew_in2, skew_out, extra)
        stride = n16(n) + extra
        rin, rout = Region(T, n, stride, skew_in).put(src), Region(T, n, stride, skew_out)
        rin2 = Region(T, n, stride, skew_in2).put(src2) if op in TWO_INPUT else None
        core.filter_batch(OPS[op], rin.ptr, rout.ptr, T, d_in2=rin2.ptr if rin2 else None, stride=stride)
        core.synchronize()
        got = rout.get()
        for t in range(T):
            assert np.array_equal(got[t], want[t]), (case, t)
        assert np.array_equal(rin.get(), src), case
        if rin2:
            assert np.array_equal(rin2.get(), src2), case


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("w,h", SHAPES)
def test_conv_kxk_dispatch(po, cores, w, h, K):
    """mi355_conv_kxk (single frame) over the same pointer cases."""
    n = 3 * w * h
    src = reference(po, w, h)["in"]["conv3x3"][:1]
    k = po.gaussian_kernel(K, 1.5)
    want = po.conv_kxk(src[0], w, h, k)
    core = cores(w, h, 3)
    for skew_in, skew_out in sorted({(c[0], c[2]) for c in POINTER_CASES}):
        rin, rout = Region(1, n, skew=skew_in).put(src), Region(1, n, skew=skew_out)
        core.conv_kxk(rin.ptr, rout.ptr, k)
        core.synchronize()
        assert np.array_equal(rout.get()[0], want), (skew_in, skew_out)
        assert np.array_equal(rin.get(), src), (skew_in, skew_out)


@pytest.mark.parametrize("w,h", SHAPES)
def test_binarize_chain_single_frame_dispatch(po, cores, w, h):
    """mi355_binarize_chain with the caller's histogram and threshold buffers, all four guarded."""
    n = 3 * w * h
    r = reference(po, w, h)
    check_binarize_inputs(r, "binarize")
    core = cores(w, h, 3)
    for t in range(3):
        src, want = r["in"]["binarize"][t:t + 1], r["want"]["binarize"][t]
        for skew_in, skew_out in sorted({(c[0], c[2]) for c in POINTER_CASES}):
            rin, rout = Region(1, n, skew=skew_in).put(src), Region(1, n, skew=skew_out)
            hist, thr = Guarded(256, torch.int32), Guarded(1, torch.int32)
            core.binarize_chain(rin.ptr, rout.ptr, hist.ptr, thr.ptr)
            core.synchronize()
            case = (t, skew_in, skew_out)
            assert np.array_equal(hist.get(), po.histogram(src[0])), case
            assert int(thr.get()[0]) == r["thr"]["binarize"][t], case
            assert np.array_equal(rout.get()[0], want), case
            assert np.array_equal(rin.get(), src), case


# ---- B. in place -----------------------------------------------------------------------------------------------------------

IN_PLACE = ["gray_avg", "gray_weighted", "binarize", "gray_avg_binarize", "gray_weighted_binarize",
            "heat_map/cur", "heat_map/prev", "red_dense/cur", "red_dense/prev"]


@pytest.mark.parametrize("skew", [0, 3])
@pytest.mark.parametrize("call", IN_PLACE)
@pytest.mark.parametrize("w,h,T", [(64, 17, 1), (131, 127, 3)])
def test_in_place(po, cores, w, h, T, call, skew):
    """out == in (== cur or == prev for the two-input filters): 64x17 as one frame at stride N (N % 16 == 0: the fast
    path when the pointers allow it), through the single-frame entry point where there is one; 131x127 as a batch of three
    at stride n16 + 16.  Then the same with every pointer 3 bytes off."""
    n = 3 * w * h
    op, _, target = call.partition("/")
    r = reference(po, w, h)
    if op in BINARIZE_OPS:
        check_binarize_inputs(r, op)
    core = cores(w, h, 3)
    stride = n if T == 1 else n16(n) + 16
    src, src2, want = r["in"][op][:T], r["in2"][:T], r["want"][op][:T]
    a = Region(T, n, stride, skew).put(src)
    b = Region(T, n, stride, skew).put(src2) if op in TWO_INPUT else None
    out, other, other_src = (b, a, src) if target == "prev" else (a, b, src2)
    if T == 1 and op in ("gray_avg", "gray_weighted"):
        getattr(core, op)(a.ptr, a.ptr)
    elif T == 1 and op == "binarize":
        core.binarize_chain(a.ptr, a.ptr)
    elif T == 1 and op in TWO_INPUT:
        getattr(core, op)(a.ptr, b.ptr, out.ptr)
    else:
        core.filter_batch(OPS[op], a.ptr, out.ptr, T, d_in2=b.ptr if b else None, stride=stride)
    core.synchronize()
    got = out.get()
    for t in range(T):
        assert np.array_equal(got[t], want[t]), t
    if other:
        assert np.array_equal(other.get(), other_src)


@pytest.mark.parametrize("skew", [0, 3])
def test_neighbourhood_filters_refuse_in_place(po, cores, skew):
    w, h, T = 64, 17, 3
    n = 3 * w * h
    src = reference(po, w, h)["in"]["conv3x3"]
    core = cores(w, h, T)
    buf = Region(T, n, n16(n) + 16, skew).put(src)
    calls = [lambda: core.conv3x3(buf.ptr, buf.ptr), lambda: core.median5x5(buf.ptr, buf.ptr),
             lambda: core.conv_kxk(buf.ptr, buf.ptr, po.gaussian_kernel(3, 1.5)),
             lambda: core.conv_kxk(buf.ptr, buf.ptr, po.gaussian_kernel(5, 1.5)),
             lambda: core.filter_batch(lib.OP_CONV3X3, buf.ptr, buf.ptr, T, stride=n16(n) + 16),
             lambda: core.filter_batch(lib.OP_MEDIAN5X5, buf.ptr, buf.ptr, T, stride=n16(n) + 16)]
    for i, call in enumerate(calls):
        with pytest.raises(lib.Mi355Error) as e:
            call()
        assert e.value.code == lib.ERR_INVALID, i
    core.synchronize()
    assert np.array_equal(buf.get(), src)


# ---- C. red_dense at the edges of its threshold ---------------------------------------------------------------------------

def red_edge_frames(T, npix, thr, seed):
    """prev / cur whose pixels differ in ONE channel, by 0, +-1, +-thr, +-(thr + 1) or +-255 (what fits a byte): pixel i
    takes combination i % len(combinations), so every difference meets every channel, and every place in a lane."""
    rng = np.random.default_rng(seed)
    diffs = sorted({s * d for d in (0, 1, thr, thr + 1, 255) if d <= 255 for s in (1, -1)})
    combos = [(ch, d) for d in diffs for ch in range(3)]
    prev = rng.integers(0, 256, (T, npix, 3)).astype(np.int32)
    cur = prev.copy()
    for i in range(npix):
        ch, d = combos[i % len(combos)]
        lo, hi = max(0, -d), min(255, 255 - d)
        prev[:, i, ch] = rng.integers(lo, hi + 1, T)
        cur[:, i, ch] = prev[:, i, ch] + d
    assert prev.min() >= 0 and cur.min() >= 0 and prev.max() <= 255 and cur.max() <= 255
    for t in range(T):
        for ch in range(3):
            assert set(np.unique(cur[t, :, ch] - prev[t, :, ch])) == set(diffs), (t, ch)
    return cur.astype(np.uint8).reshape(T, -1), prev.astype(np.uint8).reshape(T, -1)


@pytest.mark.parametrize("thr", [0, 1, 20, 254, 255])
def test_red_dense_threshold_edges(po, cores, thr):
    """The compare is (uint32_t)(x + thr) > 2 * thr: run where it could wrap or be off by one, as one frame (byte path:
    3417 bytes) and as a batch of three at an aligned stride (fast path, with the ragged lane)."""
    w, h, T = 67, 17, 3
    n = 3 * w * h
    cur, prev = red_edge_frames(T, n // 3, thr, seed=thr)
    want = np.stack([po.red_dense(c, p, thr) for c, p in zip(cur, prev)])
    red = want.reshape(T, -1, 3)
    assert not red[:, :, :2].any()
    assert (red[:, :, 2] == 0).any() and (red[:, :, 2] == 255).any() == (thr < 255)
    core = cores(w, h, T, thr)
    for skew in (0, 3):
        a, b, out = Region(1, n, skew=skew).put(cur[:1]), Region(1, n, skew=skew).put(prev[:1]), Region(1, n, skew=skew)
        core.red_dense(a.ptr, b.ptr, out.ptr)
        core.synchronize()
        assert np.array_equal(out.get()[0], want[0]), skew
        assert np.array_equal(a.get(), cur[:1]) and np.array_equal(b.get(), prev[:1])
    stride = n16(n) + 16
    a, b, out = Region(T, n, stride).put(cur), Region(T, n, stride).put(prev), Region(T, n, stride)
    core.filter_batch(lib.OP_RED_DENSE, a.ptr, out.ptr, T, d_in2=b.ptr, stride=stride)
    core.synchronize()
    assert np.array_equal(out.get(), want)
    assert np.array_equal(a.get(), cur) and np.array_equal(b.get(), prev)


# ---- D. frame counts past a grid dimension -------------------------------------------------------------------------------
# The batch tiles PERIOD distinct frames, frame[t] = base[t % PERIOD]; the oracle runs on those only.  251 is a prime that
# divides neither 65536 nor 65535 (65535 % 251 = 24): the frames behind a seam at either count differ from the frames at
# the head of the batch, so a frame index taken modulo 65536, a grid of at most 65535 frames that does not advance one of
# its pointers (input, second input, output, histogram, threshold, gray scratch, offsets), a slice that runs twice or not
# at all -- each is a mismatch.
PERIOD, MAX_BATCH = 251, 65537
assert 65535 % PERIOD and 65536 % PERIOD
COUNTS = [65535, 65536, 65537]
# (w, h, stride): 15 bytes back to back (byte path), 48 bytes at 64 (fast path)
PIXEL_FRAMES = [(5, 1, 15), (16, 1, 64)]
# rows of 24 bytes: the generic conv kernel; the median's strip kernel at stride 56, its generic one at 51.  (Two rows hold
# at most 10 of a window's 25 values: the median of 8x2 is zero everywhere, whatever the input.  8x6 has windows of 25.)
NEIGHBOUR_FRAMES = [(8, 2, 56), (8, 2, 51), (8, 6, 152)]


@pytest.mark.parametrize("T", COUNTS)
@pytest.mark.parametrize("op", list(OPS))
def test_filter_batch_frame_counts(po, cores, op, T):
    """mi355_filter_batch accepts every nframes <= max_batch: the launchers issue grids of at most 65535 frames."""
    tile = np.arange(T) % PERIOD
    for w, h, stride in (NEIGHBOUR_FRAMES if op in ("conv3x3", "median5x5") else PIXEL_FRAMES):
        n = 3 * w * h
        r = reference(po, w, h, PERIOD)
        core = cores(w, h, MAX_BATCH)
        src, src2, want = r["in"][op][tile], r["in2"][tile], r["want"][op][tile]
        rin, rout = Region(T, n, stride).put(src), Region(T, n, stride)
        rin2 = Region(T, n, stride).put(src2) if op in TWO_INPUT else None
        core.filter_batch(OPS[op], rin.ptr, rout.ptr, T, d_in2=rin2.ptr if rin2 else None, stride=stride)
        core.synchronize()
        got = rout.get()
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, ((w, h, stride), "first wrong frames", bad[:8], "of", bad.size)
        assert np.array_equal(rin.get(), src), (w, h, stride)
        if rin2:
            assert np.array_equal(rin2.get(), src2), (w, h, stride)


@pytest.mark.parametrize("T", COUNTS)
@pytest.mark.parametrize("clear", [0, 1])
def test_red_stream_batch_frame_counts(po, cores, clear, T):
    """mi355_red_stream_batch on a stream with one entry in every 251st frame and in every frame from 65535 on (frame 0 owns
    an entry and frame 1 none; frames 65535 and 65536 own other entries than frame 0), painted onto zeroed frames (clear) or
    onto a canvas that tiles 251 frames."""
    tile = np.arange(T) % PERIOD
    for w, h, stride in PIXEL_FRAMES:
        n = 3 * w * h
        core = cores(w, h, MAX_BATCH)
        rng = np.random.default_rng(n + clear)
        canvas = rng.integers(0, 200, (PERIOD, n), dtype=np.uint8)[tile]
        owners = np.union1d(np.arange(0, T, PERIOD), np.arange(65535, T))
        xs = ((np.arange(owners.size) * 7 + 3) % n).astype(np.int32)
        assert (xs[owners >= 65535] + 2 - xs[owners >= 65535] % 3 != xs[0] + 2 - xs[0] % 3).all()   # other pixels than frame 0's
        counts = np.zeros(T, np.int64)
        counts[owners] = 1
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        want = np.zeros((T, n), np.uint8) if clear else canvas.copy()
        for t, x in zip(owners, xs):
            want[t] = po.red_overlap(want[t], [x])
        d_off, d_xs = Guarded(T + 1, torch.int32, data=off), Guarded(xs.size, torch.int32, data=xs)
        frames = Region(T, n, stride).put(canvas)
        core.red_stream_batch(d_off.ptr, d_xs.ptr, T, frames.ptr, clear=clear, stride=stride)
        core.synchronize()
        got = frames.get()
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, ((w, h, stride), "first wrong frames", bad[:8], "of", bad.size)
        assert np.array_equal(d_off.get(), off) and np.array_equal(d_xs.get(), xs)

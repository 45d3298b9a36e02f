"""Every entry point that takes stride_bytes, out_stride_bytes or wall_pitch, on buffers whose windows lie up to and past
4 GiB apart (include/mi355diff.h bounds a stride from below only).  mi355_create refuses max_batch * N >= 2^32, so an offset
s * stride reaches 2^32 only with a stride far above N: one slab per camera.  Three things are pinned here:
    the pack kernel's 32-bit window (csrc/diff_pack.hip, pack_tile: voff[d] = byte_off + d * stride through one descriptor whose
        length is clamped to 2^32 - 1; csrc/core.hip, run_batch takes that path while 3 * stride + N < 2^32);
    the (size_t)x * stride products of csrc/stream_ops.hip, csrc/filters.hip and csrc/diff_pack.hip;
    the host's span and overlap tests, which multiply the same quantities.

Layouts (LAYOUTS), each at 64x48 (N = 9216: nine whole pack tiles of 1 KiB, two whole apply tiles of 4 KiB and a ragged one,
16-byte aligned) and at 37x11 (N = 1221: one whole pack tile and a ragged one, N no multiple of 4):
    slabs       stride 2^26, 66 windows, aligned: windows 64 and 65 start at 2^32 and 2^32 + 2^26 -- under a 32-bit product
                exactly on windows 0 and 1.  run_batch keeps the vector path (ALIGNED kernels); the descriptor of every
                register group that begins below window 2 is clamped.
    odd_slabs   stride 2^26 + 5, base + 3: the byte paths of every kernel (ALIGNED = false) at the same distances.
    far         stride 2^31 + 16, 3 windows: the third starts past 2^32 and 3 * stride + N >= 2^32 sends run_batch to the
                pointer kernels (ALIGNED = false) although everything is 16-byte aligned.
    window_edge the largest multiple of 16 with 3 * stride + N < 2^32 (ALIGNED) and that plus 16 (not), one frame more than a
                register group.  Stream and segmented forms (groups of 4): the first group's last frame is at voff =
                3 * stride, just below 2^32.  Pair forms (groups of 2): voff stays at stride, about 1.43 GiB, so for them only
                the host's `aligned` decision is on the seam.
Every stream has its own state, frames and changes (sequence()), so an access that lands in another stream's window or in a gap
cannot give the expected bytes; test_the_inputs_discriminate proves that on the host for a product reduced modulo 2^32.
The references are the suite's: pyoracle, cwire_spec, resync_spec, wall_spec, numpy_tick / expected of
test_cwire_round_seams_gpu, numpy_client of test_apply_multi_stream_gpu, the per-frame oracle of test_filters_edges_gpu.
Windows live in gpu_util.FarRegion: only the windows cross to the host, get() asserts every other byte on the device.
(mi355_filter_batch's "conv K x K" family is k_conv3x3_any, which OP_CONV3X3 takes at 37x11 and on unaligned layouts;
k_conv_kxk itself has no strided entry point.)"""
import contextlib
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cwire_spec as spec
import resync_spec as rs
import wall_spec as ws
from cudavideostream_amd import cwire_apply_host, state_digest_host
from oracle import pyoracle as po
from gpu_util import GUARD, CUDACore, FarRegion, Guarded, Region, oracle_pairs
from test_apply_multi_stream_gpu import numpy_client, packed, run_form
from test_cwire_budget_gpu import NOLIMIT
from test_cwire_round_seams_gpu import expected, numpy_tick
from test_filters_edges_gpu import OPS, check_binarize_inputs
from test_filters_edges_gpu import reference as filter_reference
from test_resync_gpu import Refresh, check_refresh, clear_and_apply, damaged, run_digest, sender_states
from test_wall_gpu import Wall, compose, mask_buffer, pattern, random_states

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(64, 48), (37, 11)]
LAYOUTS = {"slabs": ((1 << 26), 66, 0), "odd_slabs": ((1 << 26) + 5, 66, 3), "far": ((1 << 31) + 16, 3, 0)}   # stride, S, skew
OUT = {"slabs": ((1 << 25), 0), "odd_slabs": ((1 << 25) + 7, 1), "far": ((1 << 30) + 16, 0)}   # out_stride, skew: S * K windows
K3 = 3                        # frames per stream of the multi-stream calls
SEAM = (0, 1, 63, 64, 65)     # the streams on both sides of 2^32 at 66 windows of 2^26 bytes
FORMS = ("arrays", "wire", "cwire")
SUFFIX = {"arrays": "_batch", "wire": "_wire_batch", "cwire": "_cwire_batch"}
THR = 20
everywhere = pytest.mark.parametrize("layout", list(LAYOUTS))
sizes = pytest.mark.parametrize("w,h", SIZES)

# entry point -> the tests that run it far apart (test_the_table_is_complete reads the header against this)
COVERED = {
    "mi355_diff_stream_batch": "test_diff_stream, test_window_edge",
    "mi355_diff_stream_wire_batch": "test_diff_stream, test_window_edge",
    "mi355_diff_stream_cwire_batch": "test_diff_stream, test_window_edge",
    "mi355_diff_pairs_batch": "test_diff_pairs, test_window_edge",
    "mi355_diff_multi_batch": "test_diff_multi, test_window_edge",
    "mi355_diff_multi_wire_batch": "test_diff_multi, test_window_edge",
    "mi355_diff_multi_cwire_batch": "test_diff_multi, test_window_edge, test_chain",
    "mi355_diff_multi_stream_batch": "test_diff_multi_stream, test_window_edge",
    "mi355_diff_multi_stream_wire_batch": "test_diff_multi_stream, test_window_edge",
    "mi355_diff_multi_stream_cwire_batch": "test_diff_multi_stream, test_window_edge",
    "mi355_apply_batch": "test_apply",
    "mi355_apply_wire_batch": "test_apply",
    "mi355_apply_cwire_batch": "test_apply",
    "mi355_apply_multi_batch": "test_apply_multi",
    "mi355_apply_multi_wire_batch": "test_apply_multi",
    "mi355_apply_multi_cwire_batch": "test_apply_multi, test_resync, test_chain",
    "mi355_apply_multi_stream_batch": "test_apply_multi_stream",
    "mi355_apply_multi_stream_wire_batch": "test_apply_multi_stream",
    "mi355_apply_multi_stream_cwire_batch": "test_apply_multi_stream",
    "mi355_cwire_budget_cwire_batch": "test_budget",
    "mi355_state_digest_batch": "test_resync, test_chain",
    "mi355_refresh_cwire_batch": "test_resync, test_chain",
    "mi355_state_clear_tiles_batch": "test_resync",
    "mi355_wall_compose_batch": "test_wall_far_states, test_wall_far_pitch",
    "mi355_red_stream_batch": "test_red_stream",
    "mi355_filter_batch": "test_filter_batch",
}
EXCLUDED = {
    "mi355_group_diff_stream_batch": "per-member pointers and one stride for all: run_batch and the kernels of mi355_diff_stream_batch",
    "mi355_group_diff_pairs_batch": "per-member pointers and one stride for all: run_batch and the kernels of mi355_diff_pairs_batch",
}


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sequence(seed, n, T, quiet=False):
    """(base [n], frames [T][n]), read-only.  Every frame changes three bytes of every 1 KiB tile of the one before by 45 .. 119
    and a tenth of the others by up to 3 (below the threshold: the state keeps its byte there); quiet: every frame is the base."""
    rng = np.random.default_rng(seed)
    base = rng.integers(60, 196, n, dtype=np.uint8)
    frames, prev = [], base
    for _ in range(T):
        f = prev.astype(np.int64)
        if not quiet:
            noise = rng.random(n) < 0.1
            f[noise] += rng.integers(-3, 4, int(noise.sum()))
            for lo in range(0, n, 1024):
                x = lo + rng.choice(min(1024, n - lo), 3, replace=False)
                d = rng.integers(45, 120, 3)
                f[x] = np.where(prev[x] < 128, prev[x].astype(np.int64) + d, prev[x].astype(np.int64) - d)
        prev = np.clip(f, 0, 255).astype(np.uint8)
        frames.append(prev)
    out = np.stack(frames)
    for a in (base, out):
        a.setflags(write=False)
    return base, out


@functools.lru_cache(maxsize=None)
def streams(S, n, K):
    """(pre [S][n], frames [S][K][n]) of S unrelated streams, seeded per stream; stream S // 2 does not change at all."""
    per = [sequence(100 + s, n, K, quiet=(s == S // 2)) for s in range(S)]
    pre, frames = np.stack([b for b, _ in per]), np.stack([f for _, f in per])
    pre.setflags(write=False)
    frames.setflags(write=False)
    return pre, frames


@functools.lru_cache(maxsize=None)
def ticks(S, n, K):
    """The K ticks of streams(S, n, K) in numpy -> ((offsets, xs, diff) in batch order b = s * K + t, states after [S][n],
    states after every tick [K][S][n]); asserts what the inputs promise: several entries in every pack tile and apply tile of
    every stream but the quiet one, which has none, and escapes."""
    pre, frames = streams(S, n, K)
    state, ent, after = pre, {}, []
    for t in range(K):
        tk = numpy_tick(state, frames[:, t], THR)
        for s, (x, d, _) in enumerate(tk[5]):
            ent[(s, t)] = (x, d)
            if s == S // 2:
                assert x.size == 0, "the quiet stream"
            else:
                assert (np.bincount(x // 1024, minlength=-(-n // 1024)) >= 2).all(), (s, t)
        assert int(tk[3].sum()) > 0, "no record of the tick has an escape"
        state = tk[4]
        after.append(state)
    off, xs, df = packed([ent[(s, t)] for s in range(S) for t in range(K)])
    for a in (off, xs, df):
        a.setflags(write=False)
    return (off, xs, df), state, np.stack(after)


@functools.lru_cache(maxsize=None)
def one_stream(n, T):
    """One stream of T frames (frame T // 2 repeats the one before) and its oracle result ->
    (base, frames [T][n], (offsets, xs, diff), final state, frames as a client shows them [T][n])."""
    base, fr = sequence(7, n, T)
    frames = fr.copy()
    frames[T // 2] = frames[T // 2 - 1] if T // 2 else base
    off, xs, df, st = po.diff_stream(frames, base, THR)
    counts = np.diff(off.astype(np.int64))
    assert counts[T // 2] == 0 and (np.delete(counts, T // 2) >= 2 * -(-n // 1024)).all()
    shown, _ = numpy_client([base], off, xs, df, 1, T)
    for a in (frames, off, xs, df, st, shown):
        a.setflags(write=False)
    return base, frames, (off, xs, df), st, shown


# ---- far regions that are freed when the test ends ------------------------------------------------------------------------------
@contextlib.contextmanager
def far_regions(*shapes):
    """FarRegions of the (S, n, stride, skew) given, freed on the way out.  Skips only when the device reports less free memory
    than all of them need plus 1 GiB."""
    need = sum(FarRegion.bytes_needed(*shape) for shape in shapes)
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip(f"{need} bytes needed (plus 2^30 of headroom), {free} bytes free")
    made = []
    try:
        for shape in shapes:
            made.append(FarRegion(*shape))
        yield made
    finally:
        for r in made:
            r.free()
        del made[:]
        torch.cuda.empty_cache()


def seam_note(ok):
    return "equal per stream on both sides of 2^32: " + ", ".join(f"{s}: {bool(ok[s])}" for s in SEAM if s < len(ok))


def assert_rows(got, want, what):
    """[S][n] against [S][n], the message naming the first window that differs and the streams around 2^32."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got == want).all(axis=1)
    assert ok.all(), f"{what}: window {int(np.argmin(ok))} is the first that differs; {seam_note(ok)}"


def assert_segments(off, want_off, per, what):
    """Offsets of B = S * per segments, the message naming the first stream whose counts differ."""
    assert off.shape == want_off.shape, what
    ok = (np.diff(off.astype(np.int64)) == np.diff(want_off.astype(np.int64))).reshape(-1, per).all(axis=1)
    assert ok.all() and off[0] == want_off[0], f"{what}: stream {int(np.argmin(ok))} is the first whose counts differ; {seam_note(ok)}"


def run_diff(core, stem, form, lead, stride, B, want, what, per=1):
    """One call of core.<stem><form suffix>(*lead, outputs..., stride=stride) on guarded outputs a little larger than the
    expected (offsets, xs, diff) need; everything compared byte for byte -> the output bytes."""
    off, xs, df = want
    tot = int(off[B])
    o = Guarded(B + 1, torch.int32)
    if form == "arrays":
        a, b = Guarded(tot + 64, torch.int32), Guarded(tot + 64, torch.uint8)
        tail = (o.ptr, a.ptr, b.ptr, tot + 64)
    elif form == "wire":
        ref = po.wire_pack(off, xs, df)
        a = Guarded(ref.size + 64)
        tail = (o.ptr, a.ptr, ref.size + 64)
    else:
        ref, ref_pos = spec.encode(off, xs, df)
        p, a = Guarded(B + 1, torch.int64), Guarded(ref.size + 64)
        tail = (o.ptr, p.ptr, a.ptr, ref.size + 64)
    torch.cuda.synchronize()
    getattr(core, stem + SUFFIX[form])(*lead, *tail, stride=stride)
    core.synchronize()
    what = f"{what}, {form}"
    assert_segments(o.get().view(np.uint32), off, per, what)
    if form == "arrays":
        gx, gd = a.get(tot), b.get(tot)
        assert np.array_equal(gx[:tot], xs) and np.array_equal(gd[:tot], df), what
        return gx[:tot].tobytes() + gd[:tot].tobytes()
    if form == "cwire":
        assert np.array_equal(p.get().view(np.uint64), ref_pos), what
    got = a.get(ref.size)
    assert np.array_equal(got[:ref.size], ref), what
    return got[:ref.size].tobytes()


def upload(values, dtype=torch.uint8):
    """A guarded device copy of a host array of records, offsets, indices or differences, one element longer (never empty)."""
    view = {torch.uint8: np.uint8, torch.int32: np.int32}[dtype]
    return Guarded(np.size(values) + 1, dtype, data=np.append(np.ascontiguousarray(values).view(view).ravel(), view(0)))


# ---- the diff calls -------------------------------------------------------------------------------------------------------------
@gpu
@sizes
@everywhere
def test_diff_stream(layout, w, h):
    """mi355_diff_stream_batch / _wire_ / _cwire_: the frames of one stream far apart, against pyoracle.diff_stream."""
    stride, T, skew = LAYOUTS[layout]
    n = 3 * w * h
    base, frames, want, final, _ = one_stream(n, T)
    with far_regions((T, n, stride, skew)) as (fr,):
        fr.put(frames)
        for form in FORMS:
            with CUDACore(w, h, max_batch=T, threshold=THR, sample_mat_data=base) as core:
                run_diff(core, "diff_stream", form, (fr.ptr, T), stride, T, want, f"{layout} {w}x{h}")
                assert np.array_equal(core.get_state(), final), form
        assert_rows(fr.get(), frames, "the frames are only read")


@gpu
@sizes
@everywhere
def test_diff_pairs(layout, w, h):
    """mi355_diff_pairs_batch with cur and prev in two far regions, and with prev = cur - stride in one, against oracle_pairs."""
    stride, S, skew = LAYOUTS[layout]
    n = 3 * w * h
    pre, frames = streams(S, n, 1)
    cur = frames[:, 0]
    _, line, _, _, _ = one_stream(n, S)
    with far_regions((S, n, stride, skew), (S, n, stride, skew)) as (rc, rp):
        rc.put(cur)
        rp.put(pre)
        with CUDACore(w, h, max_batch=S, threshold=THR) as core:
            run_diff(core, "diff_pairs", "arrays", (rc.ptr, rp.ptr, S), stride, S, oracle_pairs(po, cur, pre, THR),
                     f"{layout} {w}x{h}, two regions")
            assert_rows(rc.get(), cur, "cur is only read")
            assert_rows(rp.get(), pre, "prev is only read")
            rc.put(line)
            run_diff(core, "diff_pairs", "arrays", (rc.ptr + stride, rc.ptr, S - 1), stride, S - 1,
                     oracle_pairs(po, line[1:], line[:-1], THR), f"{layout} {w}x{h}, prev = cur - stride")
            assert_rows(rc.get(), line, "the frames are only read")


@gpu
@sizes
@everywhere
def test_diff_multi(layout, w, h):
    """mi355_diff_multi_batch / _wire_ / _cwire_: frames and states far apart, the states written back, against numpy_tick."""
    stride, S, skew = LAYOUTS[layout]
    n = 3 * w * h
    pre, frames = streams(S, n, 1)
    want, post, _ = ticks(S, n, 1)
    with far_regions((S, n, stride, skew), (S, n, stride, skew)) as (fr, st):
        fr.put(frames[:, 0])
        with CUDACore(w, h, max_batch=S, threshold=THR) as core:
            for form in FORMS:
                st.put(pre)
                run_diff(core, "diff_multi", form, (fr.ptr, st.ptr, S), stride, S, want, f"{layout} {w}x{h}")
                assert_rows(st.get(), post, f"the states after the tick, {form}")
        assert_rows(fr.get(), frames[:, 0], "the frames are only read")


@gpu
@sizes
@everywhere
def test_diff_multi_stream(layout, w, h):
    """mi355_diff_multi_stream_batch / _wire_ / _cwire_, K = 3: S * K frames and S states far apart, against K numpy ticks."""
    stride, S, skew = LAYOUTS[layout]
    n = 3 * w * h
    pre, frames = streams(S, n, K3)
    want, post, _ = ticks(S, n, K3)
    rows = frames.reshape(S * K3, n)
    with far_regions((S * K3, n, stride, skew), (S, n, stride, skew)) as (fr, st):
        fr.put(rows)
        with CUDACore(w, h, max_batch=S * K3, threshold=THR) as core:
            for form in FORMS:
                st.put(pre)
                run_diff(core, "diff_multi_stream", form, (fr.ptr, st.ptr, S, K3), stride, S * K3, want, f"{layout} {w}x{h}", per=K3)
                assert_rows(st.get(), post, f"the states after the burst, {form}")
        assert_rows(fr.get(), rows, "the frames are only read")


def prefetch():
    """(frames per register group of the stream and segmented forms, of the pair forms), read from csrc/diff_pack.hip."""
    text = open(os.path.join(ROOT, "cudavideostream_amd", "csrc", "diff_pack.hip")).read()
    stream = re.search(r"constexpr int kStreamPrefetch = (\d+);", text)
    pair = re.search(r"struct PrefetchOf \{ static constexpr int value = PAIR \? (\d+) : kStreamPrefetch; \};", text)
    assert stream and pair, "PrefetchOf has changed its shape: say here how long a register group is"
    return int(stream.group(1)), int(pair.group(1))


def edge_strides(n):
    lo = ((1 << 32) - 1 - n) // 3 // 16 * 16
    assert 3 * lo + n < (1 << 32) <= 3 * (lo + 16) + n and lo % 16 == 0
    return lo, lo + 16


@gpu
@pytest.mark.parametrize("stem", ["diff_stream", "diff_pairs", "diff_multi", "diff_multi_stream"])
def test_window_edge(stem):
    """The calls that go through run_batch at the largest stride that still takes the pack kernel's 32-bit window and at the
    first that does not, 64x48, one frame more than a register group (5 frames for the stream and segmented forms, 3 for the pair
    forms): the same bytes, the reference's, on both sides.  The window itself is at its edge only for the stream and segmented
    forms (voff = 3 * stride); a pair group's second frame is at voff = stride, so the pair forms cross the host's decision only."""
    w, h = 64, 48
    n = 3 * w * h
    g_stream, g_pair = prefetch()
    B = (g_pair if stem in ("diff_pairs", "diff_multi") else g_stream) + 1
    got = {}
    for stride in edge_strides(n):
        what = f"window_edge, stride {stride}"
        if stem == "diff_stream":
            base, frames, want, final, _ = one_stream(n, B)
            with far_regions((B, n, stride, 0)) as (fr,):
                fr.put(frames)
                for form in FORMS:
                    with CUDACore(w, h, max_batch=B, threshold=THR, sample_mat_data=base) as core:
                        got[(stride, form)] = run_diff(core, stem, form, (fr.ptr, B), stride, B, want, what)
                        assert np.array_equal(core.get_state(), final), (what, form)
                assert_rows(fr.get(), frames, what)
            continue
        pre, frames = streams(B, n, 1)
        cur = frames[:, 0]
        with far_regions((B, n, stride, 0), (B, n, stride, 0)) as (fr, st), CUDACore(w, h, max_batch=B, threshold=THR) as core:
            fr.put(cur)
            if stem == "diff_pairs":
                st.put(pre)
                got[(stride, "arrays")] = run_diff(core, stem, "arrays", (fr.ptr, st.ptr, B), stride, B, oracle_pairs(po, cur, pre, THR), what)
                assert_rows(st.get(), pre, what)
            else:
                want, post, _ = ticks(B, n, 1)
                lead = (fr.ptr, st.ptr, B) if stem == "diff_multi" else (fr.ptr, st.ptr, B, 1)
                for form in FORMS:
                    st.put(pre)
                    got[(stride, form)] = run_diff(core, stem, form, lead, stride, B, want, what)
                    assert_rows(st.get(), post, f"{what}, {form}")
                if stem == "diff_multi_stream":          # ... and the B frames as ONE stream: no exchange inside the call
                    base, line, want1, final, _ = one_stream(n, B)
                    fr.put(line)
                    st.put(np.tile(base, (B, 1)))
                    got[(stride, "one stream")] = run_diff(core, stem, "arrays", (fr.ptr, st.ptr, 1, B), stride, B, want1, what, per=B)
                    assert_rows(st.get(), np.concatenate([final[None], np.tile(base, (B - 1, 1))]), f"{what}, one stream")
                    cur = line
            assert_rows(fr.get(), cur, what)
    lo, hi = edge_strides(n)
    for (stride, form), data in got.items():
        if stride == lo:
            assert data == got[(hi, form)], f"{stem}, {form}: the two sides of the window differ"


# ---- the client calls -----------------------------------------------------------------------------------------------------------
@gpu
@sizes
@everywhere
def test_apply(layout, w, h):
    """mi355_apply_batch / _wire_ / _cwire_: the frames a client shows far apart, against numpy_client and mi355_cwire_apply_host."""
    stride, T, skew = LAYOUTS[layout]
    n = 3 * w * h
    base, _, (off, xs, df), final, shown = one_stream(n, T)
    recs, _ = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, T)
    host = base.copy()
    assert cwire_apply_host(host, recs, T) == recs.size and np.array_equal(host, final) and np.array_equal(shown[-1], final)
    d_off, d_xs, d_df = upload(off, torch.int32), upload(xs, torch.int32), upload(df)
    d_wire, d_recs = upload(po.wire_pack(off, xs, df)), upload(recs)
    with far_regions((T, n, stride, skew)) as (out,):
        for form in FORMS:
            with CUDACore(w, h, max_batch=T, threshold=THR, sample_mat_data=base) as core:
                torch.cuda.synchronize()
                if form == "arrays":
                    core.apply_batch(d_off.ptr, d_xs.ptr, d_df.ptr, T, out.ptr, stride=stride)
                elif form == "wire":
                    core.apply_wire_batch(d_wire.ptr, counts, T, out.ptr, stride=stride)
                else:
                    core.apply_cwire_batch(d_recs.ptr, counts, escapes, T, out.ptr, stride=stride)
                core.synchronize()
                assert_rows(out.get(), shown, f"{layout} {w}x{h}, {form}: the frames")
                assert np.array_equal(core.get_state(), final), form
            out.put(np.full((T, n), 0xA7, np.uint8))
    for g in (d_off, d_xs, d_df, d_wire, d_recs):
        g.get()


@gpu
@sizes
@everywhere
def test_apply_multi(layout, w, h):
    """mi355_apply_multi_batch / _wire_ / _cwire_, each called directly (k_apply_multi, k_apply_multi_wire, k_cwa_apply_multi: not
    the kernels of the multi-stream forms): the receivers' states far apart; segment or record s takes states[s] from the state
    before the tick to the state after it."""
    stride, S, skew = LAYOUTS[layout]
    n = 3 * w * h
    pre, _ = streams(S, n, 1)
    (off, xs, df), post, _ = ticks(S, n, 1)
    _, client = numpy_client(pre, off, xs, df, S, 1)
    assert np.array_equal(client, post)
    recs, _ = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, S)
    assert np.array_equal(counts, np.diff(off.astype(np.int64)))
    d_off, d_xs, d_df = upload(off, torch.int32), upload(xs, torch.int32), upload(df)
    d_wire, d_recs = upload(po.wire_pack(off, xs, df)), upload(recs)
    with far_regions((S, n, stride, skew)) as (st,):
        with CUDACore(w, h, max_batch=S, threshold=THR) as core:
            for form in FORMS:
                st.put(pre)
                torch.cuda.synchronize()
                if form == "arrays":
                    core.apply_multi_batch(d_off.ptr, d_xs.ptr, d_df.ptr, S, st.ptr, stride=stride)
                elif form == "wire":
                    core.apply_multi_wire_batch(d_wire.ptr, counts, S, st.ptr, stride=stride)
                else:
                    core.apply_multi_cwire_batch(d_recs.ptr, counts, escapes, S, st.ptr, stride=stride)
                core.synchronize()
                assert_rows(st.get(), post, f"{layout} {w}x{h}, {form}: the states")
    for g in (d_off, d_xs, d_df, d_wire, d_recs):
        g.get()


@gpu
@sizes
@everywhere
@pytest.mark.parametrize("frames_out", [False, True])
def test_apply_multi_stream(layout, w, h, frames_out):
    """mi355_apply_multi_stream_batch / _wire_ / _cwire_, K = 3: the states far apart and, with frames_out, the S * K output
    frames at a far out_stride of their own."""
    stride, S, skew = LAYOUTS[layout]
    out_stride, out_skew = OUT[layout]
    n = 3 * w * h
    pre, _ = streams(S, n, K3)
    (off, xs, df), post, _ = ticks(S, n, K3)
    shown, client = numpy_client(pre, off, xs, df, S, K3)
    assert np.array_equal(client, post)
    shapes = [(S, n, stride, skew)] + ([(S * K3, n, out_stride, out_skew)] if frames_out else [])
    with far_regions(*shapes) as made:
        st, out = made[0], made[1] if frames_out else None
        with CUDACore(w, h, max_batch=S * K3, threshold=THR) as core:
            for form in ("compact", "wire", "arrays"):
                st.put(pre)
                got, frames = run_form(form, core, st, out, off, xs, df, S, K3)
                assert_rows(got, post, f"{layout} {w}x{h}, {form}: the states")
                if frames_out:
                    ok = (frames == shown).all(axis=1).reshape(S, K3).all(axis=1)
                    assert ok.all(), f"{form}: the frames of stream {int(np.argmin(ok))} are the first that differ; {seam_note(ok)}"
                    out.put(np.full((S * K3, n), 0xA7, np.uint8))


@gpu
@sizes
@everywhere
def test_budget(layout, w, h):
    """mi355_cwire_budget_cwire_batch with budgets that drop entries: the states far apart, reverted in place, against
    expected() of test_cwire_round_seams_gpu."""
    stride, S, skew = LAYOUTS[layout]
    n = 3 * w * h
    pre, frames = streams(S, n, 1)
    tk = numpy_tick(pre, frames[:, 0], THR)
    recs, _, counts, escapes, post, ent = tk
    kinds = (lambda c: c // 2, lambda c: NOLIMIT, lambda c: 0, lambda c: c // 8)
    budgets = np.array([kinds[s % 4](len(ent[s][0])) for s in range(S)], np.uint32)
    w_thr, w_off, w_pos, w_recs, w_states, _ = expected(tk, pre, THR, budgets)
    dropped = [s for s in range(S) if not np.array_equal(w_states[s], post[s])]
    assert set(dropped) >= {s for s in range(S) if s % 4 != 1 and s != S // 2}, "every limited stream reverts bytes"
    src = upload(recs)
    thr, off, pos, out = Guarded(S, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(w_recs.size + 64)
    with far_regions((S, n, stride, skew)) as (st,):
        st.put(post)
        with CUDACore(w, h, max_batch=S, threshold=THR) as core:
            torch.cuda.synchronize()
            core.cwire_budget_cwire_batch(src.ptr, counts, escapes, st.ptr, S, budgets, thr.ptr, off.ptr, pos.ptr, out.ptr,
                                          w_recs.size + 64, stride=stride)
            core.synchronize()
        what = f"{layout} {w}x{h}"
        ok = thr.get().view(np.uint32) == w_thr
        assert ok.all(), f"{what}: the thresholds; {seam_note(ok)}"
        assert_segments(off.get().view(np.uint32), w_off, 1, what)
        assert np.array_equal(pos.get().view(np.uint64), w_pos), what
        assert np.array_equal(out.get(w_recs.size)[:w_recs.size], w_recs), what
        assert_rows(st.get(), w_states, f"{what}: the states, reverted where an entry was dropped")
    src.get()


# ---- resynchronisation and the wall -----------------------------------------------------------------------------------------------
@gpu
@sizes
@everywhere
def test_resync(layout, w, h):
    """mi355_state_digest_batch, mi355_refresh_cwire_batch without and with peer digests, mi355_state_clear_tiles_batch (and the
    apply of the refresh records) on states far apart, against resync_spec and mi355_state_digest_host."""
    stride, S, skew = LAYOUTS[layout]
    n = 3 * w * h
    sender = sender_states(w, h, S)
    t = rs.tiles(n)
    chosen = [s for s in SEAM if s < S][1:]                   # 1, 63, 64, 65 (far: 1, 2): stream 0 is damaged nowhere
    recv, sel = damaged(sender, sorted({(s, k) for s in chosen for k in (0, t - 1)}))
    digests = np.stack([rs.digest(x) for x in sender])
    assert all(np.array_equal(digests[s], state_digest_host(sender[s])) for s in range(S))
    what = f"{layout} {w}x{h}"
    with far_regions((S, n, stride, skew), (S, n, stride, skew)) as (snd, rcv):
        snd.put(sender)
        rcv.put(recv)
        with CUDACore(w, h, max_batch=S, threshold=THR) as core:
            ok = (run_digest(core, snd, S) == digests).all(axis=(1, 2))
            assert ok.all(), f"{what}: the digests of stream {int(np.argmin(ok))} are the first that differ; {seam_note(ok)}"
            check_refresh(Refresh(core, snd, S), sender, np.ones((S, t), bool))            # a key frame of every stream
            peer = np.stack([rs.digest(x) for x in recv])
            assert np.array_equal(rs.selected_tiles(sender, peer), sel)
            r = Refresh(core, snd, S, peer=peer)
            _, counts, escapes = check_refresh(r, sender, sel)
            assert_rows(snd.get(), sender, f"{what}: the sender's states are only read")
            clear_and_apply(core, rcv, r, counts, escapes)
            assert_rows(rcv.get(), sender, f"{what}: the receiver after clear and apply")


def grid_places(w, h, S, k, hidden=()):
    """S thumbnails at scale k on a grid of 11 columns, one pixel apart -> (int32[S, 3], wall_w, wall_h)."""
    tw, th = ws.thumb_size(w, h, k)
    cols = 11
    places = np.array([(1 + (s % cols) * (tw + 1), 1 + (s // cols) * (th + 1), 0 if s in hidden else k) for s in range(S)], np.int32)
    return places, 1 + cols * (tw + 1), 1 + -(-S // cols) * (th + 1)


@gpu
@sizes
@everywhere
def test_wall_far_states(layout, w, h):
    """mi355_wall_compose_batch, full and masked, from states far apart into a small wall, against wall_spec."""
    stride, S, skew = LAYOUTS[layout]
    n = 3 * w * h
    src = random_states(w, h, S)
    places, wall_w, wall_h = grid_places(w, h, S, 4, hidden=(S // 2,))
    chosen = [s for s in SEAM if s < S and s not in (0, S // 2)]
    rows = np.zeros((S, ws.mask_words(n)), np.uint32)
    rows[chosen] = 0xFFFFFFFF
    mask = mask_buffer(rows)
    only = places.copy()
    only[[s for s in range(S) if s not in chosen], 2] = 0
    with far_regions((S, n, stride, skew)) as (st,):
        st.put(src)
        wall, wall_m = Wall(wall_w, wall_h), Wall(wall_w, wall_h)
        with CUDACore(w, h, max_batch=S) as core:
            torch.cuda.synchronize()
            compose(core, st, S, places, wall)
            compose(core, st, S, places, wall_m, mask)
            core.synchronize()
        got, want = wall.get(), ws.compose(pattern(wall_w, wall_h), src, w, h, places)
        for s in range(S):
            if places[s][2]:
                x, y, tw, th = ws.rect(w, h, places[s])
                assert np.array_equal(got[y:y + th, x:x + tw], want[y:y + th, x:x + tw]), f"{layout} {w}x{h}: the thumbnail of stream {s}"
        assert np.array_equal(got, want), "written outside the thumbnails"
        assert np.array_equal(wall_m.get(), ws.compose(pattern(wall_w, wall_h), src, w, h, only)), f"masked: streams {chosen}"
        assert_rows(st.get(), src, "the states are only read")
    mask.get()


@gpu
@sizes
def test_wall_far_pitch(w, h):
    """mi355_wall_compose_batch from small contiguous states into a wall whose rows are 2^27 bytes apart: row 32 starts at 2^32.
    One thumbnail above it, one across it, one below it."""
    S, k, pitch = 3, 8, 1 << 27
    n = 3 * w * h
    tw, th = ws.thumb_size(w, h, k)
    src = random_states(w, h, S)
    places = np.array([(1, 1, k), (2, 32 - th // 2, k), (tw + 4, 33, k)], np.int32)
    wall_w, wall_h = 2 * tw + 6, 34 + th
    assert th >= 2 and places[1][1] < 32 < places[1][1] + th and places[0][1] + th < 32
    states = Region(S, n).put(src)
    with far_regions((wall_h, 3 * wall_w, pitch, 0)) as (wall,):
        with CUDACore(w, h, max_batch=S) as core:
            torch.cuda.synchronize()
            core.wall_compose_batch(states.ptr, S, places, wall.ptr, wall_w, wall_h, wall_pitch=pitch, stride=states.stride)
            core.synchronize()
        got = wall.get().reshape(wall_h, wall_w, 3)
        want = ws.compose(pattern(wall_w, wall_h), src, w, h, places)
        ok = (got == want).all(axis=(1, 2))
        assert ok.all(), f"row {int(np.argmin(ok))} of the wall is the first that differs (row 32 starts at 2^32)"
    assert np.array_equal(states.get(), src)


# ---- the frame filters ----------------------------------------------------------------------------------------------------------
@gpu
@sizes
@everywhere
@pytest.mark.parametrize("clear", [True, False])
def test_red_stream(layout, w, h, clear):
    """mi355_red_stream_batch: the red maps of a batch far apart, on zeroed frames or painted onto given ones, against
    pyoracle.red_overlap per frame."""
    stride, T, skew = LAYOUTS[layout]
    n = 3 * w * h
    _, _, (off, xs, _), _, _ = one_stream(n, T)
    canvas = np.random.default_rng(T + n).integers(0, 200, (T, n), dtype=np.uint8)
    want = np.stack([po.red_overlap(np.zeros(n, np.uint8) if clear else canvas[t], xs[off[t]:off[t + 1]]) for t in range(T)])
    d_off, d_xs = upload(off, torch.int32), upload(xs, torch.int32)
    with far_regions((T, n, stride, skew)) as (out,):
        out.put(canvas)
        with CUDACore(w, h, max_batch=T, threshold=THR) as core:
            torch.cuda.synchronize()
            core.red_stream_batch(d_off.ptr, d_xs.ptr, T, out.ptr, clear=clear, stride=stride)
            core.synchronize()
        assert_rows(out.get(), want, f"{layout} {w}x{h}, clear = {clear}")
    d_off.get(), d_xs.get()


FILTER_OPS = ["gray_weighted", "gray_weighted_binarize", "heat_map", "red_dense", "conv3x3", "median5x5"]


@gpu
@sizes
@everywhere
def test_filter_batch(po, layout, w, h):
    """mi355_filter_batch, one op per kernel family, input and output frames far apart (3 frames at `far`, 66 at the slabs),
    against the per-frame oracle.  conv3x3 is the strip kernel at 64x48 on the aligned layouts and k_conv3x3_any elsewhere."""
    stride, T, skew = LAYOUTS[layout]
    n = 3 * w * h
    r = filter_reference(po, w, h, T)
    check_binarize_inputs(r, "gray_weighted_binarize")
    with far_regions((T, n, stride, skew), (T, n, stride, skew), (T, n, stride, skew)) as (rin, rin2, rout):
        rin2.put(r["in2"])
        with CUDACore(w, h, k=po.gaussian_kernel(3, 1.5), max_batch=T, threshold=THR) as core:
            for op in FILTER_OPS:
                two = op in ("heat_map", "red_dense")
                rin.put(r["in"][op])
                rout.put(np.full((T, n), 0xA7, np.uint8))
                torch.cuda.synchronize()
                core.filter_batch(OPS[op], rin.ptr, rout.ptr, T, d_in2=rin2.ptr if two else None, stride=stride)
                core.synchronize()
                assert_rows(rout.get(), r["want"][op], f"{layout} {w}x{h}, {op}")
                assert_rows(rin.get(), r["in"][op], f"{op}: the input is only read")
        assert_rows(rin2.get(), r["in2"], "the second input is only read")


# ---- one chain without a host wait --------------------------------------------------------------------------------------------------
@gpu
def test_chain():
    """slabs, 64x48, nothing waited for in between: the tick (mi355_diff_multi_cwire_batch), mi355_apply_multi_cwire_batch of its
    records onto a second far region, mi355_state_digest_batch of both, mi355_refresh_cwire_batch of the sender against the
    receiver's digests.  Both regions end as the numpy states and the refresh selects nothing."""
    w, h = 64, 48
    stride, S, skew = LAYOUTS["slabs"]
    n = 3 * w * h
    pre, frames = streams(S, n, 1)
    tk = numpy_tick(pre, frames[:, 0], THR)
    recs, w_pos, counts, escapes, post, _ = tk
    t = rs.tiles(n)
    with far_regions((S, n, stride, skew), (S, n, stride, skew), (S, n, stride, skew)) as (fr, snd, rcv):
        fr.put(frames[:, 0])
        snd.put(pre)
        rcv.put(pre)
        off, pos, cw = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(recs.size + 64)
        dg_s, dg_r = Guarded(2 * S * t, torch.int32), Guarded(2 * S * t, torch.int32)
        r = Refresh(None, snd, S, peer=dg_r)
        with CUDACore(w, h, max_batch=S, threshold=THR) as core:
            torch.cuda.synchronize()
            core.diff_multi_cwire_batch(fr.ptr, snd.ptr, S, off.ptr, pos.ptr, cw.ptr, recs.size + 64, stride=stride)
            core.apply_multi_cwire_batch(cw.ptr, counts, escapes, S, rcv.ptr, stride=stride)      # (the headers: numpy's)
            core.state_digest_batch(snd.ptr, S, dg_s.ptr, stride=stride)
            core.state_digest_batch(rcv.ptr, S, dg_r.ptr, stride=stride)
            r.call(core, snd)
            core.synchronize()
        assert np.array_equal(pos.get().view(np.uint64), w_pos) and np.array_equal(cw.get(recs.size)[:recs.size], recs)
        assert_rows(snd.get(), post, "the sender's states")
        assert_rows(rcv.get(), post, "the receiver's states")
        want = np.stack([rs.digest(x) for x in post]).reshape(-1)
        assert np.array_equal(dg_s.get().view(np.uint32), want) and np.array_equal(dg_r.get().view(np.uint32), want)
        mask, r_off, r_pos, _ = r.results()
        assert not mask.any() and not r_off.any() and np.array_equal(r_pos, 8 * np.arange(S + 1, dtype=np.uint64)), "an empty refresh"
        assert_rows(fr.get(), frames[:, 0], "the frames are only read")


# ---- without a GPU: the inputs discriminate, the table is complete ----------------------------------------------------------------
class WrapMem:
    """The windows of a far region as an implementation sees them that reduces index * stride modulo 2^32: window i is read and
    written at offset (i * stride) % 2^32 behind the base.  Kept per true window: its n bytes and the 2048 guard bytes behind."""

    SLACK = 2048

    def __init__(self, rows, stride):
        rows = np.asarray(rows, np.uint8)
        self.S, self.n, self.stride = rows.shape[0], rows.shape[1], stride
        self.image = np.full((self.S, self.n + self.SLACK), GUARD, np.uint8)
        self.image[:, :self.n] = rows

    def where(self, i):
        j, r = divmod((i * self.stride) % (1 << 32), self.stride)
        assert j < self.S and r <= self.SLACK, (i, j, r)
        return j, r

    def read(self, i):
        j, r = self.where(i)
        return self.image[j, r:r + self.n].copy()

    def write(self, i, row):
        j, r = self.where(i)
        self.image[j, r:r + self.n] = row

    def rows(self):
        return np.stack([self.read(i) for i in range(self.S)])

    @classmethod
    def true_image(cls, rows):
        return cls(rows, 1 << 40).image       # (no product of the tests reaches 2^40: nothing wraps)


def wrapped_reads_differ(rows, stride, result):
    """result(row, i) of what a wrapping implementation reads differs from that of the true operand, for some window."""
    mem = WrapMem(rows, stride)
    return any(not np.array_equal(result(mem.read(i), i), result(rows[i], i)) for i in range(len(rows)))


def wrapped_writes_differ(before, after, stride):
    """Writing the correct result of every window, in order, through wrapping addresses leaves other bytes than the truth."""
    mem = WrapMem(before, stride)
    for i in range(len(after)):
        mem.write(i, after[i])
    return not np.array_equal(mem.image, WrapMem.true_image(after))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("w,h", SIZES)
def test_the_inputs_discriminate(layout, w, h):
    """The test of the tests.  For every class of multi-stream call: were s * stride (b * stride, b * out_stride, y * pitch)
    reduced modulo 2^32 in an operand read, in a state write or in an output-frame write, then a window or a guard byte would
    differ from what the GPU tests expect."""
    stride, S, _ = LAYOUTS[layout]
    out_stride, _ = OUT[layout]
    n = 3 * w * h
    assert (S - 1) * stride >= (1 << 32) and (S * K3 - 1) * out_stride >= (1 << 32), "the layout reaches 2^32"
    for K in (1, K3):
        pre, frames = streams(S, n, K)
        (off, xs, df), post, after = ticks(S, n, K)
        rows = frames.reshape(S * K, n)
        state_of = lambda b: pre[b // K] if b % K == 0 else after[b % K - 1][b // K]

        def entries(frame, b):           # what the tick emits for batch index b when it reads `frame` as that frame
            a = np.abs(frame.astype(np.int64) - state_of(b).astype(np.int64))
            return np.flatnonzero(a > THR).tobytes() + frame[a > THR].tobytes()

        assert wrapped_reads_differ(rows, stride, entries), f"diff_multi{'_stream' if K > 1 else ''}: the frames, read"
        assert wrapped_reads_differ(pre, stride, lambda st, s: np.where(np.abs(frames[s, 0].astype(np.int64) - st) > THR, frames[s, 0], st)), \
            "diff_multi*: the states, read"
        assert wrapped_writes_differ(pre, post, stride), "diff_multi*, apply_multi*: the states, written"
        if K == K3:
            shown, _ = numpy_client(pre, off, xs, df, S, K)
            assert wrapped_writes_differ(np.full((S * K, n), GUARD, np.uint8), shown, out_stride), "apply_multi_stream*: the frames out"
        delta = (post.astype(np.int64) - pre).astype(np.uint8)
        assert wrapped_reads_differ(pre, stride, lambda st, s: st + delta[s]), "apply_multi*: the states, read"
    # the budget's revert: the states after the tick go back to `pre` at the dropped entries
    pre, frames = streams(S, n, 1)
    tk = numpy_tick(pre, frames[:, 0], THR)
    budgets = np.array([0 if s % 2 else NOLIMIT for s in range(S)], np.uint32)
    reverted = expected(tk, pre, THR, budgets)[4]
    assert wrapped_writes_differ(tk[4], reverted, stride), "cwire_budget: the states, reverted"
    assert wrapped_reads_differ(tk[4], stride, lambda st, s: np.abs(st.astype(np.int64) - pre[s])), "cwire_budget: the states, read"
    # digests, refresh records, cleared tiles
    sender = sender_states(w, h, S)
    assert wrapped_reads_differ(sender, stride, lambda st, s: rs.digest(st)), "state_digest, refresh_cwire: the states, read"
    cleared = sender.copy()
    cleared[:, :min(n, rs.TILE)] = 0
    assert wrapped_writes_differ(sender, cleared, stride), "state_clear_tiles: the states, written"
    # the wall: states read, rows written
    src = random_states(w, h, S)
    assert wrapped_reads_differ(src, stride, lambda st, s: ws.thumbnail(st, w, h, 4)), "wall_compose: the states, read"
    if layout == "slabs":
        pitch, th = 1 << 27, ws.thumb_size(w, h, 8)[1]
        wall_rows = np.random.default_rng(5).integers(0, 255, (34 + th, 30), dtype=np.uint8)
        assert wrapped_writes_differ(np.full_like(wall_rows, GUARD), wall_rows, pitch), "wall_compose: the wall's rows"
    # one stream's frames: the stream forms, the one-stream client, the red map, the filters
    base, line, (off, xs, df), final, shown = one_stream(n, S)
    state_before = lambda t: base if t == 0 else shown[t - 1]
    assert wrapped_reads_differ(line, stride, lambda f, t: np.flatnonzero(np.abs(f.astype(np.int64) - state_before(t)) > THR)), \
        "diff_stream, diff_pairs, filter_batch: the frames, read"
    assert wrapped_writes_differ(np.full((S, n), GUARD, np.uint8), shown, stride), "apply, red_stream, filter_batch: the frames out"


def strided_prototypes():
    """The names of the prototypes of include/mi355diff.h that have a parameter whose name contains `stride` or `pitch`."""
    text = open(os.path.join(ROOT, "include", "mi355diff.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = []
    for m in re.finditer(r"\b(mi355_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        if any(re.search(r"(stride|pitch)\w*$", p) for p in params):
            names.append(m.group(1))
    return names


def test_the_table_is_complete():
    """Every strided entry point of the header is run far apart by a test of this module (COVERED) or excluded with a reason;
    a new one fails here until someone covers it."""
    names = strided_prototypes()
    assert len(names) >= len(COVERED) and "mi355_filter_batch" in names and "mi355_wall_compose_batch" in names, names
    assert not set(COVERED) & set(EXCLUDED)
    for name in names:
        assert name in COVERED or (name in EXCLUDED and EXCLUDED[name]), f"{name} takes a stride or a pitch and no far-apart test runs it"
    for name in list(COVERED) + list(EXCLUDED):
        assert name in names, f"{name} is listed here and is no strided prototype of the header"
    for name, tests in COVERED.items():
        for test in tests.split(", "):
            assert callable(globals().get(test)), (name, test)
            assert name[len("mi355_"):] in wrappers_reached(globals()[test]), f"{test} is listed for {name} and never calls it"


def wrappers_reached(test):
    """The CUDACore methods a test of this module calls, read from its source and from the source of the helpers it names (one
    level: run_form, Refresh, run_digest, clear_and_apply, compose, run_diff): every `.name_batch(` there, and for run_diff,
    which puts the name together, every stem the test names as a string times the forms it passes (a variable: all three)."""
    text = inspect.getsource(test)
    helpers = {h for h in re.findall(r"\b([A-Za-z_]\w*)\(", text) if not h.startswith("test_") and
               (inspect.isfunction(globals().get(h)) or inspect.isclass(globals().get(h))) and globals()[h] is not CUDACore}
    found = set(re.findall(r"\.(\w+_batch)\(", text + "".join(inspect.getsource(globals()[h]) for h in sorted(helpers))))
    stems = set(re.findall(r'"(diff_\w+)"', text))
    for stem, form in re.findall(r'run_diff\(core, (\w+|"\w+"), (\w+|"\w+")', text):
        for st in ([stem.strip('"')] if stem.startswith('"') else stems):
            found |= {st + SUFFIX[f] for f in ([form.strip('"')] if form.startswith('"') else FORMS)}
    return found


def test_the_guard_check_of_a_far_region_fires():
    """FarRegion.get() on the host, in pieces of 300 bytes: rows come back as they were put; one byte written into the front
    pad, into a stride gap (in its first and in a later piece), into the last gap and into the tail pad is each reported with its
    offset and the name of where it lies; a byte written inside a window is not a guard's business."""
    S, n, stride, skew = 5, 37, 1000, 3
    r = FarRegion(S, n, stride, skew, device="cpu")
    r.PIECE = 300
    rows = np.arange(S * n, dtype=np.uint8).reshape(S, n)
    rows[rows == GUARD] = 0
    assert r.buf.numel() == FarRegion.bytes_needed(S, n, stride, skew) and np.array_equal(r.put(rows).get(), rows)
    lo = r.lo
    cases = [(0, "the front pad"), (lo - 1, "the front pad"), (lo + n, "the gap behind window 0"),
             (lo + n + 700, "the gap behind window 0"), (lo + stride - 1, "the gap behind window 0"),
             (lo + 3 * stride + n + 301, "the gap behind window 3"), (lo + 4 * stride + n, "the tail pad"),
             (r.buf.numel() - 1, "the tail pad")]
    for at, name in cases:
        r.buf[at] = 1
        with pytest.raises(AssertionError, match=rf"byte {at} of the allocation .* it lies in {name}$"):
            r.get()
        r.buf[at] = GUARD
    r.buf[lo + 2 * stride + 5] = 1
    rows[2, 5] = 1
    assert np.array_equal(r.get(), rows)

"""-m gpu: the diff path at the top of the range mi355_create accepts (ceil(N / 1024) * 1024 * max(max_batch,
code_chunks(max_batch)) < 2^32): frame and stream counts around 65535, record-log offsets from 2^31 to just below 2^32, and
totals with bit 31 set with wire and record positions past 2^32.

Part 1, counts.  Every kernel launch of csrc/ whose grid or by-value table is sized by nframes, nstreams or nrecords, the
count at which it starts another launch or round, and the test that crosses it (test_top_of_range_host.py reads csrc/ against
this table):
    kernel (launcher)                                  sized by                       next launch / round at       crossed by
    k_diff_pack (launch_diff_pack, diff_pack.hip)      grid.x = tiles; frames: a loop none                         test_counts_stream, test_counts_pairs, test_counts_multi
    k_scan_groups (launch_scan)                        grid.x = nframes; 256 / round  257 frames (the last block)  test_counts_stream
    k_expand (launch_expand)                           grid.y = nframes               none: one grid, any count    test_counts_stream, test_counts_pairs, test_counts_multi, test_counts_multi_stream
    k_cwire_items, k_expand_cwire (launch_expand_cwire) grid.y = nframes              none: one grid, any count    test_counts_stream, test_counts_multi, test_counts_multi_stream
    k_cwire_fscan (launch_expand_cwire)                grid.x = nframes               none                         test_counts_stream
    k_cwire_place (launch_expand_cwire)                1024 threads / round           1025 frames                  test_batch_seams_gpu.test_direct_equals_spec, test_counts_stream
    every kernel of filters.hip with a frame dimension grid.y or .z, for_frame_grids  65536 frames                 test_filters_edges_gpu, section D
    k_two_max_threshold (filters.hip)                  grid.x = nframes               none                         test_filters_edges_gpu, section D
    k_cwire_count, k_cwire_scan, k_cwire_emit          grid.y = nframes               refused above 8192 slots     test_batch_seams_gpu.test_encode_refuses_more_frames_than_slots
    k_cwire_decode (stream_ops.hip)                    grid.x = frames of a launch    65 frames (the host's loop)  test_batch_seams_gpu
    k_cwa_table                                        128 headers by value           129 records                  test_batch_seams_gpu, test_newer_seams_gpu
    k_cwa_scan, k_cwk_finish                           grid.x = records               none                         test_cwire_check_gpu, test_newer_seams_gpu
    k_cwa_apply_multi*, k_cwc_sum, k_cwc_emit,         grid.x = tiles * nstreams      none                         test_cwire_round_seams_gpu, test_crop_seams_gpu,
      k_cwb_hist, k_cwb_facts, k_cwb_emit, k_rf_*,                                                                 test_newer_seams_gpu, test_resync_gpu
      k_crop_emit, k_state_*, k_act_tile, k_cw_touched
    k_cwc_scan, k_cwb_thr, k_act_summary               grid.x = nstreams              none                         test_cwire_round_seams_gpu, test_newer_seams_gpu
    k_cwc_place                                        1024 streams / round           1025 streams                 test_cwire_round_seams_gpu
    k_cwb_init, k_crop_facts, k_wall_compose,          128 streams by value           129 streams                  test_cwire_round_seams_gpu, test_crop_seams_gpu,
      k_apply_multi_wire                                                                                           test_wall_gpu, test_batch_seams_gpu
    k_apply_multi_strided, k_apply_multi_show          grid.y = min(nstreams, 65535)  65536 streams (a loop in y)  test_counts_apply_multi_stream
    k_merge_index, k_merge_parts                       grid.x = nframes (/ 256)       none                         test_batch_seams_gpu
    k_cwr_scan, k_cwr_dscan                            grid.x = records; 256 chunks   257 chunks (n > 2^20) /      test_runs_despeckle_seams_gpu.test_records_past_the_chunk_and_workgroup_rounds,
                                                       or workgroups / round          r > 262 144 runs             test_every_byte_runs_encode (513 chunks), test_runs_despeckle_seams_gpu.test_link_positions_past_4_gib
    k_cwr_place                                        256 records / round            257 records                  test_runs_despeckle_seams_gpu.test_records_past_the_place_rounds (257, 513), test_every_byte_runs_encode
    k_cwr_table                                        64 records by value            65 records                   test_cwire_runs_gpu (130), test_runs_despeckle_seams_gpu.test_records_past_the_place_rounds
    k_cws_table                                        128 records by value           129 records                  test_split_seams_gpu (145 records)
    k_dsp_init                                         128 streams by value;          129 streams;                 test_runs_despeckle_seams_gpu.test_streams_past_the_init_launches (129, 257),
                                                       grid.y = nwords / 4096 + 1     nwords 4096                  test_runs_despeckle_seams_gpu.test_a_sparse_call_between_two_dense_ones (2 and 3 blocks)
    k_dsp_mark, k_dsp_keep, k_dsp_facts, k_dsp_emit    grid = tiles or words x        none: one grid               test_runs_despeckle_seams_gpu.test_streams_past_the_init_launches,
                                                       nstreams                                                    test_cwire_despeckle_gpu
The three expansion kernels take the whole batch as ONE grid y dimension, 65536 and 65537 included: the runtime accepts such a
grid (its limit is 2^32 work-items per dimension, and y counts single work-groups here), which test_counts_* pin.
Frames come from a pool of 251 pictures (251 divides neither 65535 nor 65536), frames from index 65535 on from a second pool:
test_top_of_range_host.py proves that a frame index taken modulo 65536, a second grid that does not advance one of its
pointers, and a slice that runs twice or not at all are each a mismatch.

Part 2, record-log offsets.  1000x700 (N = 2 100 000: 2051 pack tiles, the last of 800 bytes) at max_batch = T = 1100 and 2045
(1023 is the least max_batch with max_batch * 2051 * 1024 >= 2^31, 2045 the largest mi355_create accepts).  Tiles 0, 1023, 1024,
2049 and 2050 change in every byte in every frame, so each appends one 1 KiB chunk of records per frame and the last frames'
records lie at byte offsets from 2^31 up to 9216 below 2^32 (dense_case asserts that from the layout rule of
csrc/diff_pack.hip, "the log"); one more tile changes isolated bytes in a few late frames (the code log).

Part 3, totals and positions.  The same shape at T = 1100 with every byte of every frame changed: 2.31e9 entries (offsets with
bit 31 set), xs past 8 GiB, plain-wire positions past 2^32, compact-record positions past 2^32 from record 1023 on.  The
reference is a plain statement (every_byte_reference; the host file checks it against pyoracle and cwire_spec at T = 4);
expected buffers are built on the device and compared there in slices of at most 1 GiB (gpu_util.BigGuarded,
gpu_util.assert_same_on_device).  The consumers of compact records (CONSUMERS) each read that 4.6 GB record buffer; the run-code
pair also writes and reads it as a link of 2.3 GB in the run form, made from runs_spec.to_runs of the zero-difference template.

Every output lies in a guarded buffer that starts as a non-zero pattern, inputs are asserted unchanged, and every expected
value comes from oracle/pyoracle.py, tests/cwire_spec.py and po.wire_pack."""
import functools

import numpy as np
import pytest
import torch

import crop_spec as crop
import cwire_spec as spec
import runs_spec as rs
import split_spec
from cudavideostream_amd import cwire_split_bytes_max, cwire_split_host, cwire_split_pieces_max, lib, state_tiles
from oracle import pyoracle as po
from gpu_util import DEV, BigGuarded, CUDACore, Guarded, Region, assert_same_on_device, to_dev
from test_activity_gpu import oracle as activity_oracle

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64
THR = 20
FORMS = ("arrays", "wire", "cwire")
SUFFIX = {"arrays": "_batch", "wire": "_wire_batch", "cwire": "_cwire_batch"}

class Ref:
    """(offsets, xs, diff) of the oracle and, made from them when first asked for, the plain wire (po.wire_pack) and the compact
    records with their positions (cwire_spec.encode).  Read-only."""

    def __init__(self, off, xs, df):
        self.off, self.xs, self.df = np.asarray(off).astype(np.uint32), np.asarray(xs, np.int32), np.asarray(df, np.uint8)
        for a in (self.off, self.xs, self.df):
            a.setflags(write=False)

    @functools.cached_property
    def wire(self):
        return po.wire_pack(self.off, self.xs, self.df)

    @functools.cached_property
    def _encoded(self):
        return spec.encode(self.off, self.xs, self.df)

    recs = property(lambda self: self._encoded[0])
    pos = property(lambda self: self._encoded[1])


def flat_oracle(cur, prev):
    """pyoracle.diff_pack of S operand pairs in ONE call: the rule is per byte, so the S pairs laid end to end are one frame of
    S * n bytes whose entries, cut at the multiples of n, are the pairs' -> (offsets [S + 1], xs, diff, next states [S][n])."""
    S, n = cur.shape
    _, gx, df, st = (po.diff_pack_mt if cur.size > 1 << 24 else po.diff_pack)(cur.reshape(-1), prev.reshape(-1), THR)
    off = np.searchsorted(gx, np.arange(S + 1, dtype=np.int64) * n)
    return off, (gx.astype(np.int64) % n).astype(np.int32), df, st.reshape(S, n)


# ---- outputs: one guarded set per call ------------------------------------------------------------------------------------------
class Outputs:
    """The guarded outputs of one diff call in `form`, a little larger than the reference needs."""

    def __init__(self, form, ref):
        self.form, self.ref, B = form, ref, ref.off.size - 1
        self.off = Guarded(B + 1, I32)
        tot = int(ref.off[B])
        if form == "arrays":
            self.xs, self.df = Guarded(tot + 64, I32), Guarded(tot + 64)
            self.tail = (self.off.ptr, self.xs.ptr, self.df.ptr, tot + 64)
        elif form == "wire":
            self.wire = Guarded(ref.wire.size + 64)
            self.tail = (self.off.ptr, self.wire.ptr, ref.wire.size + 64)
        else:
            self.pos, self.cw = Guarded(B + 1, I64), Guarded(ref.recs.size + 64)
            self.tail = (self.off.ptr, self.pos.ptr, self.cw.ptr, ref.recs.size + 64)

    def check(self, what):
        ref, B = self.ref, self.ref.off.size - 1
        what = f"{what}, {self.form}"
        off = self.off.get().view(np.uint32)
        if not np.array_equal(off, ref.off):
            first = int(np.argmax(off != ref.off))
            raise AssertionError(f"{what}: offsets[{first}] is {off[first]}, the reference's {ref.off[first]}")
        tot = int(ref.off[B])
        if self.form == "arrays":
            gx, gd = self.xs.get(tot), self.df.get(tot)
            assert_equal(gx[:tot], ref.xs, f"{what}: xs", ref.off)
            assert_equal(gd[:tot], ref.df, f"{what}: diff", ref.off)
        elif self.form == "wire":
            assert_equal(self.wire.get(ref.wire.size)[:ref.wire.size], ref.wire, f"{what}: the wire")
        else:
            assert_equal(self.pos.get().view(np.uint64), ref.pos, f"{what}: frame_pos")
            assert_equal(self.cw.get(ref.recs.size)[:ref.recs.size], ref.recs, f"{what}: the records", ref.pos)


def assert_equal(got, want, what, starts=None):
    """np.array_equal with the first differing element in the message (and, given the segments' starts, its segment)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    first = int(np.argmax(got != want))
    seg = "" if starts is None else f" (segment {int(np.searchsorted(np.asarray(starts).astype(np.int64), first, 'right')) - 1})"
    raise AssertionError(f"{what}: element {first}{seg} is {got[first]}, the reference's {want[first]}")


def require(need):
    """The one reason to skip: the device reports less free memory than the test has computed from its sizes."""
    torch.cuda.empty_cache()          # (what torch holds for reuse is free for this purpose)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{need} bytes of device memory needed, {free} bytes free")


def small_need(rows, n, *refs):
    """Device bytes of a test of Part 1: two regions of `rows` frames, the largest output form of every reference (the wire,
    5 bytes per entry and 4 per frame) twice over, and 1 GiB for the core and the allocator."""
    return 2 * rows * n + sum(2 * (5 * int(r.off[-1]) + 16 * r.off.size) for r in refs) + (1 << 30)


def call(core, stem, form, lead, out, stride):
    getattr(core, stem + SUFFIX[form])(*lead, *out.tail, stride=stride)


# ---- Part 1: 65535, 65536 and 65537 frames or streams -----------------------------------------------------------------------------
POOL = 251
GRID = 65535                      # the frames of one grid, were the launches split as csrc/filters.hip splits them
COUNTS = (65535, 65536, 65537)
SMALL = [(33, 7), (16, 4)]        # N = 693: one ragged tile, odd, the byte paths; N = 192: 16-byte aligned, the vector path
COUNT_CASES = [(w, h, T) for w, h in SMALL for T in COUNTS] + [(5, 1, 2 * 65536 + 1)]
MULTI_STREAM = [(255, 257), (256, 256), (65537, 1), (1, 65537)]


@functools.lru_cache(maxsize=None)
def pools(n):
    """(base [n], pictures [3][251][n]): three pools of 251 pictures around one base.  Most pictures differ from the base in a
    few bytes (by 128); pictures 40, 123 and 206 of every pool differ from it in every byte (by 100 and more: whole tiles of
    records), and picture 100 equals picture 99 (a frame without entries wherever the two follow each other)."""
    rng = np.random.default_rng(1000 + n)
    base = rng.integers(60, 196, n, dtype=np.uint8)
    out = np.empty((3, POOL, n), np.uint8)
    for p in range(3):
        for i in range(POOL):
            pic = base.copy()
            if i % 83 == 40:
                pic += 100 + 10 * p + i % 5
            else:
                x = rng.choice(n, min(n, 2 + (i + p) % 7), replace=False)
                pic[x] ^= 0x80
                pic[i % n] = (int(base[i % n]) + 40 + ((i // n) * 3 + p) % 85) % 256     # by 40 .. 124: no two pictures alike
            out[p, i] = pic
        out[p, 100] = out[p, 99]
    assert len({out[p, i].tobytes() for p in range(3) for i in range(POOL)}) == 3 * (POOL - 1), "the pictures differ"
    base.setflags(write=False)
    out.setflags(write=False)
    return base, out


def pool_frames(n, T, wrong=None):
    """Frame t of T: picture t % 251 of the first pool below frame 65535, of the second pool from there on.  `wrong` (for the
    host's discrimination test) maps the frame indices an implementation would read instead."""
    _, pics = pools(n)
    t = np.arange(T)
    if wrong is not None:
        t = wrong(t)
    return pics[(t >= GRID).astype(np.int64), t % POOL]


def pool_states(n, S):
    """State s of S: picture (5 s + 1) % 251 of the third pool."""
    return pools(n)[1][2, (5 * np.arange(S) + 1) % POOL]


@functools.lru_cache(maxsize=None)
def stream_case(w, h, T):
    """One stream of T pool frames, two batches back to back -> (base, frames, [Ref of batch 1, of batch 2], [state after 1,
    after 2]).  Asserts what the input is for: T crosses the count, the frames from 65535 on have entries, frames without
    entries and whole-tile frames occur, and the state moves in the last grid."""
    n = 3 * w * h
    base = pools(n)[0]
    frames = pool_frames(n, T)
    refs, states, state = [], [], base
    for _ in range(2):
        off, xs, df, state = po.diff_stream(frames, state, THR)
        refs.append(Ref(off, xs, df))
        states.append(state)
    counts = np.diff(refs[0].off.astype(np.int64))
    assert T >= GRID and (counts == 0).any() and (counts == n).any()
    if T > GRID:
        assert all(counts[g] > 0 for g in range(GRID, T, GRID)) and counts[T - 1] > 0, "the first frame of every further grid, and the last"
    assert not np.array_equal(states[0], base) and not np.array_equal(refs[0].df, refs[1].df)
    frames.setflags(write=False)
    return base, frames, refs, states


@functools.lru_cache(maxsize=None)
def pairs_case(w, h, T):
    """T pairs (pool frame t, pool state t) -> (cur, prev, Ref)."""
    n = 3 * w * h
    cur, prev = pool_frames(n, T), pool_states(n, T)
    ref = Ref(*flat_oracle(cur, prev)[:3])
    counts = np.diff(ref.off.astype(np.int64))
    assert (counts[GRID - 1:] > 0).all() and (counts == n).any()
    return cur, prev, ref


@functools.lru_cache(maxsize=None)
def multi_stream_case(w, h, S, K):
    """K pool frames of each of S streams (batch index b = s * K + t is pool frame b), state s = pool state s ->
    (frames [S * K][n], states [S][n], Ref, states after [S][n]).  K = 1 is the case of the mi355_diff_multi_* calls."""
    n = 3 * w * h
    frames, pre = pool_frames(n, S * K), pool_states(n, S)
    if K == 1:
        off, xs, df, post = flat_oracle(frames, pre)
        ref = Ref(off, xs, df)
    else:
        offs, xs, df, post = [np.zeros(1, np.int64)], [], [], np.empty_like(pre)
        for s in range(S):
            o, x, d, post[s] = po.diff_stream(frames[s * K:(s + 1) * K], pre[s], THR)
            offs.append(offs[-1][-1] + o[1:].astype(np.int64)); xs.append(x); df.append(d)
        ref = Ref(np.concatenate(offs), np.concatenate(xs), np.concatenate(df))
    counts = np.diff(ref.off.astype(np.int64))
    assert S * K >= GRID and (counts[GRID - 1:] > 0).all() and (counts == n).any() and not np.array_equal(pre, post)
    post.setflags(write=False)
    return frames, pre, ref, post


SCHEDULES = ("pipelined", "sequential")


def set_schedule(core, schedule):
    """pipelined: the core's own stream as it comes; sequential: MI355_OPT_PIPELINE 0; torch: torch's current stream."""
    if schedule == "sequential":
        core.set_option(lib.OPT_PIPELINE, 0)
    elif schedule == "torch":
        core.use_torch_stream()
    assert core.get_option(lib.OPT_PIPELINE) == (0 if schedule == "sequential" else 1)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("w,h,T", COUNT_CASES)
def test_counts_stream(w, h, T, schedule):
    """mi355_diff_stream_batch / _wire_ / _cwire_ with T frames in one call, two calls back to back (both log sets when
    pipelined), against pyoracle.diff_stream of the whole batch."""
    base, frames, refs, states = stream_case(w, h, T)
    require(small_need(T, frames.shape[1], *refs))
    fr = Region(T, frames.shape[1]).put(frames)
    for form in FORMS:
        outs = [Outputs(form, r) for r in refs]
        with CUDACore(w, h, max_batch=T, threshold=THR, sample_mat_data=base) as core:
            set_schedule(core, schedule)
            torch.cuda.synchronize()
            for out in outs:
                call(core, "diff_stream", form, (fr.ptr, T), out, fr.stride)
            core.synchronize()
            for k, out in enumerate(outs):
                out.check(f"{w}x{h}, {T} frames, {schedule}, batch {k + 1}")
            assert np.array_equal(core.get_state(), states[1]), form
        del outs
    assert np.array_equal(fr.get(), frames), "the frames are only read"


@pytest.mark.parametrize("w,h", SMALL)
@pytest.mark.parametrize("T", COUNTS)
def test_counts_pairs(w, h, T):
    """mi355_diff_pairs_batch with T pairs in one call, against the oracle pair by pair."""
    cur, prev, ref = pairs_case(w, h, T)
    n = cur.shape[1]
    require(small_need(T, n, ref))
    rc, rp, out = Region(T, n).put(cur), Region(T, n).put(prev), Outputs("arrays", ref)
    with CUDACore(w, h, max_batch=T, threshold=THR) as core:
        torch.cuda.synchronize()
        core.diff_pairs_batch(rc.ptr, rp.ptr, T, *out.tail, stride=n)
        core.synchronize()
        out.check(f"{w}x{h}, {T} pairs")
    assert np.array_equal(rc.get(), cur) and np.array_equal(rp.get(), prev), "the operands are only read"


def run_feedback(w, h, S, K, stem, lead_of):
    frames, pre, ref, post = multi_stream_case(w, h, S, K)
    n = frames.shape[1]
    require(small_need(S * K, n, ref))
    fr, st = Region(S * K, n).put(frames), Region(S, n)
    with CUDACore(w, h, max_batch=S * K, threshold=THR) as core:
        for form in FORMS:
            st.put(pre)
            out = Outputs(form, ref)
            torch.cuda.synchronize()
            call(core, stem, form, lead_of(fr, st), out, n)
            core.synchronize()
            out.check(f"{stem} {w}x{h}, S = {S}, K = {K}")
            assert_equal(st.get().reshape(-1), post.reshape(-1), f"{form}: the states afterwards", np.arange(S) * n)
            del out
    assert np.array_equal(fr.get(), frames), "the frames are only read"


@pytest.mark.parametrize("w,h", SMALL)
@pytest.mark.parametrize("S", COUNTS)
def test_counts_multi(w, h, S):
    """mi355_diff_multi_batch / _wire_ / _cwire_ with S streams in one call, the states written back, against the oracle."""
    run_feedback(w, h, S, 1, "diff_multi", lambda fr, st: (fr.ptr, st.ptr, S))


@pytest.mark.parametrize("w,h", SMALL)
@pytest.mark.parametrize("S,K", MULTI_STREAM)
def test_counts_multi_stream(w, h, S, K):
    """mi355_diff_multi_stream_batch / _wire_ / _cwire_ with S * K = 65535, 65536 and 65537 batch indices in one call."""
    run_feedback(w, h, S, K, "diff_multi_stream", lambda fr, st: (fr.ptr, st.ptr, S, K))


@pytest.mark.parametrize("frames_out", [False, True])
@pytest.mark.parametrize("w,h", SMALL)
def test_counts_apply_multi_stream(w, h, frames_out):
    """mi355_apply_multi_stream_batch with 65537 streams of one segment each, without and with output frames: its two kernels
    walk the streams in a grid y of at most 65535 and a loop.  Segment s takes state s from before the tick to after it."""
    S = 65537
    frames, pre, ref, post = multi_stream_case(w, h, S, 1)
    n = frames.shape[1]
    require(small_need(S, n, ref))
    off, xs, df = (Guarded(a.size + 1, t, data=np.append(a, a[:1]).view(v)) for a, t, v in
                   ((ref.off, I32, np.int32), (ref.xs, I32, np.int32), (ref.df, torch.uint8, np.uint8)))
    st, out = Region(S, n).put(pre), Region(S, n) if frames_out else None
    with CUDACore(w, h, max_batch=S, threshold=THR) as core:
        torch.cuda.synchronize()
        core.apply_multi_stream_batch(off.ptr, xs.ptr, df.ptr, S, 1, st.ptr, stride=n, d_frames_out=out.ptr if out else None, out_stride=n)
        core.synchronize()
    assert_equal(st.get().reshape(-1), post.reshape(-1), "the states afterwards", np.arange(S) * n)
    if out:
        assert_equal(out.get().reshape(-1), post.reshape(-1), "the frames out", np.arange(S) * n)
    assert np.array_equal(off.get()[:-1].view(np.uint32), ref.off) and np.array_equal(xs.get()[:-1], ref.xs) and np.array_equal(df.get()[:-1], ref.df)


# ---- Part 2: record-log offsets from 2^31 to just below 2^32 ----------------------------------------------------------------------
BW, BH = 1000, 700
N = 3 * BW * BH                          # 2 100 000
NT = -(-N // 1024)                       # 2051 pack tiles, the last of 800 bytes
DENSE_TILES = (0, 1023, 1024, 2049, 2050)   # both sides of the pipelined split (1024), the last whole tile, the ragged one
CODE_TILE = 512                          # isolated bytes in a few late frames: codes only
SLAB = 44                                # frames per oracle call (divides 220, the frames per stream of the (5, 220) form)
T_LOW, T_TOP = 1100, 2045
MULTI = (5, 220)


def code_chunks(max_batch):
    return (max_batch + 2) // 3 + 1      # csrc/core.hip


def accepted(max_batch, ntiles=NT):
    """mi355_create's rule for the logs' 32-bit byte offsets (csrc/core.hip)."""
    return ntiles * 1024 * max(max_batch, code_chunks(max_batch)) < 1 << 32


def band(t, x):
    """The byte at index x of frame t wherever a frame changes everything (numpy or torch int64 arrays that broadcast): even
    frames in [150, 250), odd frames in [0, 100), so that consecutive frames differ by 51 and more everywhere; the value
    depends on t and on x."""
    k = t // 2
    return (x * (2 * k + 1) + k * 9973 + (x >> 10) * (k + 7)) % 65521 % 100 + 150 * (1 - t % 2)


def tile_span(tile):
    return tile * 1024, min((tile + 1) * 1024, N)


DENSE_COLS = np.concatenate([np.arange(*tile_span(i), dtype=np.int64) for i in DENSE_TILES])


def record_log(multi_lanes, tile, ntiles=NT):
    """The layout rule of the record log (csrc/diff_pack.hip, "the log", LogPos, emit_step): chunk k of a tile is the KiB at
    (k * ntiles + tile) * 1024 and holds 64 records; a frame's records never straddle a chunk -- if they do not fit, the rest of
    the chunk is skipped.  multi_lanes[t] = the tile's lanes with two or more flagged bytes in frame t -> the byte offset of
    every frame's first record."""
    ptr, room, jump, out = tile * 1024, 64, (ntiles - 1) * 1024, []
    for m in multi_lanes:
        if m > room:
            ptr, room = ptr + room * 16 + jump, 64
        out.append(ptr)
        ptr, room = ptr + int(m) * 16, room - int(m)
    return np.array(out, np.int64)


def late_frames(T):
    """The frames that change isolated bytes of CODE_TILE (each is undone by the frame behind it; the last frame undoes)."""
    return (T - 6, T - 4, T - 2)


def isolated_bytes(t):
    """One byte in every third 16-byte lane of CODE_TILE, a place that depends on t."""
    return CODE_TILE * 1024 + 16 * np.arange(0, 64, 3) + t % 16


@functools.lru_cache(maxsize=None)
def dense_case(T):
    """The input of Part 2 and its oracle, slab by slab -> a dict: base [N], vals [T][4896] (the dense tiles' bytes of every
    frame), refs [batch 1, batch 2] (two batches of the same frames back to back), pairs (the Ref of the pairs (frame t - 1,
    frame t), frame -1 = base), final (the state after either batch), states ([T // 220 + 1][N]: the oracle's state in front
    of frame 220 s).  Asserts from the layout rule that the last frames' records lie at offsets of 2^31 and more, and at T = 2045
    that the last chunk ends within 9216 bytes of 2^32."""
    rng = np.random.default_rng(T)
    base = rng.integers(101, 130, N, dtype=np.uint8)              # 21 and more below every even frame's bytes
    t = np.arange(T, dtype=np.int64)
    vals = band(t[:, None], DENSE_COLS[None, :]).astype(np.uint8)
    assert len({v.tobytes() for v in vals}) == T and len({v[:1024].tobytes() for v in vals}) == T, "no two frames hold the same bytes"
    late = late_frames(T)
    slab = np.tile(base, (SLAB, 1))
    lo, hi = tile_span(CODE_TILE)
    state, last, parts, pair_parts, states = base, base, [], [], []
    for t0 in range(0, T, SLAB):
        k = min(SLAB, T - t0)
        slab[:k, DENSE_COLS] = vals[t0:t0 + k]
        slab[:, lo:hi] = base[lo:hi]
        for f in late:
            if t0 <= f < t0 + k:
                slab[f - t0, isolated_bytes(f)] += 100
        if t0 % MULTI[1] == 0:
            states.append(state)
        off, xs, df, state = po.diff_stream_mt(slab[:k], state, THR)       # (the oracle over 8 host threads: identical output)
        parts.append((off, xs, df))
        if T == T_LOW:
            pair_parts.append(flat_oracle(slab[:k], np.concatenate([last[None], slab[:k - 1]]))[:3])
        if t0 == 0:
            first, after_first = slab[:k].copy(), state
        last = slab[k - 1].copy()
    states.append(state)

    def joined(ps):
        off = np.concatenate([np.zeros(1, np.int64)] + [np.asarray(p[0][1:]).astype(np.int64) for p in ps])
        ends = np.cumsum([0] + [int(np.asarray(p[0])[-1]) for p in ps])
        for i, p in enumerate(ps):
            off[1 + i * SLAB:1 + i * SLAB + len(p[0]) - 1] += ends[i]
        return Ref(off, np.concatenate([p[1] for p in ps]), np.concatenate([p[2] for p in ps]))

    ref = joined(parts)
    # the second batch of the same frames starts from the last frame: the oracle again for the first slab; behind it the state
    # is the first batch's, so everything from there on -- the oracle is a function of (state, frames) -- is too
    again = po.diff_stream_mt(first, state, THR)
    assert np.array_equal(again[3], after_first) and not np.array_equal(again[2], parts[0][2])
    ref2 = joined([again[:3]] + parts[1:])
    assert np.array_equal(state, last), "everything that changes is flagged: the state is the last frame"
    # what the input is for
    off = ref.off.astype(np.int64)
    frame_of = np.repeat(np.arange(T), np.diff(off))
    tile_of = ref.xs // 1024
    which = np.full(NT, -1)
    which[list(DENSE_TILES)] = np.arange(len(DENSE_TILES))
    sel = which[tile_of] >= 0
    key = (frame_of[sel] * len(DENSE_TILES) + which[tile_of[sel]]) * 64 + (ref.xs[sel] % 1024) // 16
    per_lane = np.bincount(key, minlength=T * len(DENSE_TILES) * 64).reshape(T, len(DENSE_TILES), 64)
    assert (per_lane[:, :4] == 16).all() and (per_lane[:, 4, :50] == 16).all() and (per_lane[:, 4, 50:] == 0).all(), \
        "every lane of the dense tiles carries 16 flagged bytes in every frame"
    ends = []
    for j, tile in enumerate(DENSE_TILES):
        multi = (per_lane[:, j] >= 2).sum(axis=1)
        at = record_log(multi, tile)
        assert np.array_equal(at, (np.arange(T) * NT + tile) * 1024), "one chunk per frame"
        assert at[T - 1] >= 1 << 31 and (at >= 1 << 31).sum() >= T - 1023, tile
        ends.append(int(at[T - 1]) + 16 * int(multi[T - 1]))
    assert max(ends) < 1 << 32
    if T == T_TOP:
        assert accepted(T) and not accepted(T + 1) and T * NT * 1024 == (1 << 32) - 9216
        assert (T - 1) * NT * 1024 + NT * 1024 == T * NT * 1024 and max(ends) + (1024 - 800) == (1 << 32) - 9216, \
            "the last chunk ends 9216 bytes below 2^32"
    counts = np.bincount(frame_of[tile_of == CODE_TILE], minlength=T)
    assert all(counts[f] == 22 and counts[f + 1] == 22 for f in late) and counts.sum() == 6 * 22, "isolated bytes: codes only"
    assert set(np.unique(tile_of)) == set(DENSE_TILES) | {CODE_TILE}
    out = dict(T=T, base=base, vals=vals, refs=[ref, ref2], final=state, states=np.stack(states),
               pairs=joined(pair_parts) if pair_parts else None)
    for a in (base, vals, state, out["states"]):
        a.setflags(write=False)
    return out


def log_bytes(T, sets):
    """Device bytes of a core's logs at max_batch T (csrc/core.hip, mi355_create and setup_pipeline), `sets` sets of them,
    and a GiB for the core's other scratch and the allocator's slack."""
    per = T * NT * 1024 + code_chunks(T) * NT * 1024 + T * NT * 16 + T * (NT // 16 + 1) * 16 * 2 + T * (N // 4096 + 2) * 64
    return sets * per + (1 << 30)


class DeviceFrames:
    """Rows 0 .. T of N bytes in one guarded device allocation: row 0 is the base, row 1 + t frame t, assembled on the device
    from the base and the per-frame contents (the frames never exist on the host).  check() asserts, on the device, that
    the guards and every row are as they were made."""

    def __init__(self, base, T):
        self.T = T
        self.g = BigGuarded((T + 1) * N)
        self.rows = self.g.t.view(T + 1, N)
        self.rows[:] = to_dev(base)
        self.ptr, self.frames_ptr = self.g.ptr, self.g.ptr + N
        self.copy = self.remake = None

    @staticmethod
    def bytes_needed(T):
        return 2 * BigGuarded.bytes_needed((T + 1) * N)

    def seal(self):
        self.copy = self.g.buf.clone()
        torch.cuda.synchronize()
        return self

    def check(self):
        """Against the copy seal() took or, without one, against remake(row), row by row."""
        torch.cuda.synchronize()
        if self.copy is not None:
            return assert_same_on_device(self.g.buf, self.copy, "the frames are only read")
        self.g.check()
        for r in range(self.T + 1):
            assert torch.equal(self.rows[r], self.remake(r)), f"row {r} of the frames has changed"

    def free(self):
        self.g.free()
        self.rows = self.copy = self.remake = None
        torch.cuda.empty_cache()


def dense_frames(case):
    fr = DeviceFrames(case["base"], case["T"])
    vals, at = to_dev(case["vals"]), 0
    for tile in DENSE_TILES:
        lo, hi = tile_span(tile)
        fr.rows[1:, lo:hi] = vals[:, at:at + hi - lo]
        at += hi - lo
    for f in late_frames(case["T"]):
        x = torch.from_numpy(isolated_bytes(f)).to(DEV)
        fr.rows[1 + f, x] += 100
    return fr.seal()


LOG_SCHEDULES = ("pipelined", "sequential", "torch")


def finish(core, schedule):
    if schedule == "torch":
        torch.cuda.synchronize()
    core.synchronize()


def run_dense_stream(T, schedule, form):
    case = dense_case(T)
    require(DeviceFrames.bytes_needed(T) + log_bytes(T, 2 if schedule == "pipelined" else 1) + 64 * int(case["refs"][0].off[T]))
    fr = dense_frames(case)
    try:
        outs = [Outputs(form, r) for r in case["refs"]]
        with CUDACore(BW, BH, max_batch=T, threshold=THR, sample_mat_data=case["base"]) as core:
            set_schedule(core, schedule)
            torch.cuda.synchronize()
            for out in outs:
                call(core, "diff_stream", form, (fr.frames_ptr, T), out, N)
            finish(core, schedule)
            for k, out in enumerate(outs):
                out.check(f"{T} frames, {schedule}, batch {k + 1}")
            assert np.array_equal(core.get_state(), case["final"])
        fr.check()
    finally:
        fr.free()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("schedule", LOG_SCHEDULES)
def test_log_offsets_stream(schedule, form):
    """mi355_diff_stream_batch / _wire_ / _cwire_ at max_batch = T = 1100, two batches back to back: the last 77 frames' records
    lie at log offsets of 2^31 and more."""
    run_dense_stream(T_LOW, schedule, form)


@pytest.mark.parametrize("form", FORMS)
def test_log_offsets_stream_at_the_largest_batch(form):
    """... and at max_batch = T = 2045, the largest mi355_create accepts for this frame: the record log ends 9216 bytes below
    2^32."""
    run_dense_stream(T_TOP, "pipelined", form)


@pytest.mark.parametrize("schedule", LOG_SCHEDULES)
def test_log_offsets_pairs(schedule):
    """mi355_diff_pairs_batch on the 1100 pairs of consecutive frames (prev = cur - stride), twice."""
    T = T_LOW
    case = dense_case(T)
    require(DeviceFrames.bytes_needed(T) + log_bytes(T, 2 if schedule == "pipelined" else 1) + 64 * int(case["pairs"].off[T]))
    fr = dense_frames(case)
    try:
        outs = [Outputs("arrays", case["pairs"]) for _ in range(2)]
        with CUDACore(BW, BH, max_batch=T, threshold=THR) as core:
            set_schedule(core, schedule)
            torch.cuda.synchronize()
            for out in outs:
                core.diff_pairs_batch(fr.frames_ptr, fr.ptr, T, *out.tail, stride=N)
            finish(core, schedule)
            for k, out in enumerate(outs):
                out.check(f"{T} pairs, {schedule}, call {k + 1}")
        fr.check()
    finally:
        fr.free()


@pytest.mark.parametrize("schedule", LOG_SCHEDULES)
def test_log_offsets_multi_stream(schedule):
    """mi355_diff_multi_stream_cwire_batch with (S, K) = (5, 220) on the same frames: stream s starts from the oracle's state
    in front of frame 220 s, so its records are those of the one stream; twice (the second call from the states the first
    left: those of the next stream, and the last frame for the last -- restored in between)."""
    T = T_LOW
    S, K = MULTI
    case = dense_case(T)
    ref = case["refs"][0]
    require(DeviceFrames.bytes_needed(T) + log_bytes(T, 2 if schedule == "pipelined" else 1) + 64 * int(ref.off[T]))
    fr = dense_frames(case)
    try:
        st = Region(S, N)
        with CUDACore(BW, BH, max_batch=T, threshold=THR) as core:
            set_schedule(core, schedule)
            for k in range(2):
                st.put(case["states"][:S])
                out = Outputs("cwire", ref)
                torch.cuda.synchronize()
                core.diff_multi_stream_cwire_batch(fr.frames_ptr, st.ptr, S, K, *out.tail, stride=N)
                finish(core, schedule)
                out.check(f"(S, K) = {MULTI}, {schedule}, call {k + 1}")
                assert np.array_equal(st.get(), case["states"][1:]), "the states afterwards"
        fr.check()
    finally:
        fr.free()


# ---- Part 3: totals with bit 31 set, wire and record positions past 2^32 ---------------------------------------------------------
REC = 8 + 2 * N                          # a record of N entries without escapes (N is a multiple of 4): 4 200 008 bytes
WIRE = 4 + 5 * N                         # a plain-wire frame of N entries


def every_byte_base():
    return np.random.default_rng(3).integers(101, 130, N, dtype=np.uint8)     # 21 and more below every even frame's bytes


def every_byte_frame(t):
    """Frame t of Part 3 on the host: every byte from band()."""
    return band(t, np.arange(N, dtype=np.int64)).astype(np.uint8)


def every_byte_reference(base, frames):
    """The plain statement that is Part 3's reference: every byte of every frame is flagged, so frame t's entries are
    arange(N) with diff = frame[t] - frame[t - 1] modulo 256 (frame[-1] = the state before the batch), and the state
    afterwards is the last frame -> (Ref, state).  (The host file checks it against pyoracle and cwire_spec at T = 4.)"""
    T = len(frames)
    before = np.concatenate([base[None], frames[:-1]])
    return Ref(N * np.arange(T + 1, dtype=np.int64), np.tile(np.arange(N, dtype=np.int32), T), (frames - before).reshape(-1)), frames[-1]


@functools.lru_cache(maxsize=None)
def templates():
    """(a plain-wire frame, a compact record) of the entries arange(N) with all differences 0, from po.wire_pack and
    cwire_spec.encode_frame: everything but the differences of any frame of Part 3, which lie in the last N bytes of either."""
    xs, zero = np.arange(N, dtype=np.int32), np.zeros(N, np.uint8)
    wire = po.wire_pack(np.array([0, N]), xs, zero)
    rec = np.frombuffer(spec.encode_frame(xs, zero), np.uint8)
    probe = np.arange(N, dtype=np.uint8) | 1
    assert wire.size == WIRE and np.array_equal(po.wire_pack(np.array([0, N]), xs, probe)[WIRE - N:], probe)
    assert rec.size == REC and np.array_equal(np.frombuffer(spec.encode_frame(xs, probe), np.uint8)[REC - N:], probe)
    return wire, rec


def every_byte_seams(T):
    """What Part 3's sizes reach, from the sizes alone."""
    total = T * N
    assert 1 << 31 <= total < 1 << 32, "offsets with bit 31 set"
    assert 4 * total > 8 << 30, "xs byte positions past 8 GiB"
    assert 4 * 409 + 5 * 409 * N < 1 << 32 <= 4 * 410 + 5 * 410 * N and T > 410, "plain-wire positions 4 t + 5 offsets[t] pass 2^32 at frame 410"
    assert 1022 * REC < 1 << 32 <= 1023 * REC and T > 1023, "frame_pos passes 2^32 at record 1023"
    return total


def every_byte_frames(T):
    """Part 3's frames, made on the device frame by frame from band(); a seeded sample of them is compared with the host's."""
    fr = DeviceFrames(every_byte_base(), T)
    x = torch.arange(N, dtype=torch.int64, device=DEV)
    make = lambda t: band(t, x).to(torch.uint8)
    for t in range(T):
        fr.rows[1 + t] = make(t)
    sample = sorted({0, 1, T - 1} | set(np.random.default_rng(T).choice(T, 3, replace=False).tolist()))
    for t in sample:
        assert np.array_equal(fr.rows[1 + t].cpu().numpy(), every_byte_frame(t)), t
    fr.remake = lambda r: to_dev(every_byte_base()) if r == 0 else make(r - 1)
    torch.cuda.synchronize()
    return fr


def slices(T, row_bytes, piece=1 << 30):
    step = max(1, piece // row_bytes)
    return [(a, min(a + step, T)) for a in range(0, T, step)]


def assert_rows_on_device(got, want, what, a, col0=0):
    """got [k][c] against want [c] or [k][c], on the device; the message names the first frame and column that differ."""
    ne = got != want
    if bool(ne.any()):
        r = int(torch.argmax(ne.any(dim=1).to(torch.uint8)))
        c = int(torch.argmax(ne[r].to(torch.uint8)))
        w = want if want.dim() == 1 else want[r]
        raise AssertionError(f"{what}: frame {a + r}, byte or element {col0 + c} is {got[r, c].item()}, the reference's {w[c].item()}")


def run_every_byte(form):
    T = T_LOW
    total = every_byte_seams(T)
    out_bytes = {"arrays": 5 * total, "wire": T * WIRE, "cwire": T * REC}[form]
    require(BigGuarded.bytes_needed((T + 1) * N) + log_bytes(T, 2) + out_bytes + (4 << 30))
    wire_t, rec_t = templates()
    base = every_byte_base()
    fr = every_byte_frames(T)
    made = []
    try:
        off = Guarded(T + 1, I32)
        if form == "arrays":
            xs, df = BigGuarded(total + 64, I32), BigGuarded(total + 64)
            made += [xs, df]
            tail = (off.ptr, xs.ptr, df.ptr, total + 64)
        elif form == "wire":
            wire = BigGuarded(T * WIRE + 64)
            made += [wire]
            tail = (off.ptr, wire.ptr, T * WIRE + 64)
        else:
            pos, cw = Guarded(T + 1, I64), BigGuarded(T * REC + 64)
            made += [cw]
            tail = (off.ptr, pos.ptr, cw.ptr, T * REC + 64)
        with CUDACore(BW, BH, max_batch=T, threshold=THR, sample_mat_data=base) as core:
            torch.cuda.synchronize()
            getattr(core, "diff_stream" + SUFFIX[form])(fr.frames_ptr, T, *tail, stride=N)
            core.synchronize()
            state = core.get_state()
        got_off = off.get().view(np.uint32)
        assert_equal(got_off, (N * np.arange(T + 1, dtype=np.int64)).astype(np.uint32), f"{form}: offsets")
        assert int(got_off[T]) >= 1 << 31
        assert np.array_equal(state, every_byte_frame(T - 1)), "the state afterwards is the last frame"
        diff = lambda a, b: fr.rows[1 + a:1 + b] - fr.rows[a:b]          # uint8: modulo 256
        if form == "arrays":
            xs.check(written=total), df.check(written=total)
            ar = torch.arange(N, dtype=I32, device=DEV)
            for a, b in slices(T, 4 * N):
                assert_rows_on_device(xs.t[a * N:b * N].view(b - a, N), ar, "xs", a)
            for a, b in slices(T, N):
                assert_rows_on_device(df.t[a * N:b * N].view(b - a, N), diff(a, b), "diff", a)
        elif form == "wire":
            wire.check(written=T * WIRE)
            head = to_dev(wire_t[:WIRE - N])
            for a, b in slices(T, WIRE):
                rows = wire.t[a * WIRE:b * WIRE].view(b - a, WIRE)
                assert_rows_on_device(rows[:, :WIRE - N], head, "the wire: count and xs", a)
                assert_rows_on_device(rows[:, WIRE - N:], diff(a, b), "the wire: diff", a, WIRE - N)
        else:
            cw.check(written=T * REC)
            assert_equal(pos.get().view(np.uint64), REC * np.arange(T + 1, dtype=np.uint64), "frame_pos")
            head = to_dev(rec_t[:REC - N])
            for a, b in slices(T, REC):
                rows = cw.t[a * REC:b * REC].view(b - a, REC)
                assert_rows_on_device(rows[:, :REC - N], head, "the records: header and codes", a)
                assert_rows_on_device(rows[:, REC - N:], diff(a, b), "the records: diff", a, REC - N)
        fr.check()
    finally:
        for g in made:
            g.free()
        fr.free()


@pytest.mark.parametrize("form", FORMS)
def test_every_byte_producers(form):
    """mi355_diff_stream_batch / _wire_ / _cwire_ on 1100 frames of 1000x700 that change every byte: 2.31e9 entries, offsets
    with bit 31 set, xs past 8 GiB, the wire 11.6 GB, frame_pos past 2^32 from record 1023 on; compared on the device."""
    run_every_byte(form)


# ---- Part 3, the consumers: one record buffer of 4.6 GB, built from the reference ----------------------------------------------
CONSUMER_SK = (2, 550)
RECTS = np.array([(900, 690, 100, 10), (0, 695, 1000, 5)], np.int32)      # both meet the last rows; the first the last columns too
CELL = (16, 16, 1)                                                       # cell_w, cell_h, min_count
CONSUMERS = {
    "mi355_apply_cwire_batch": "test_every_byte_apply",
    "mi355_cwire_check_batch": "test_every_byte_check",
    "mi355_cwire_decode_batch": "test_every_byte_decode",
    "mi355_apply_multi_stream_cwire_batch": "test_every_byte_apply_multi_stream",
    "mi355_cwire_coalesce_cwire_batch": "test_every_byte_coalesce",
    "mi355_cwire_crop_cwire_batch": "test_every_byte_crop",
    "mi355_cwire_activity_batch": "test_every_byte_activity",
    "mi355_cwire_touched_tiles_batch": "test_every_byte_touched_tiles",
    "mi355_cwire_runs_encode_batch": "test_every_byte_runs_encode",
    "mi355_cwire_split_cwire_batch": "test_every_byte_split",
}
CONSUMERS_EXCLUDED = {
    "mi355_apply_multi_cwire_batch": "one record per stream (4.2 MB each: positions stay far below 2^32 for any accepted count); the directory kernels of mi355_apply_multi_stream_cwire_batch",
    "mi355_cwire_budget_cwire_batch": "one record per stream, as above; the directory kernels of mi355_cwire_coalesce_cwire_batch",
    "mi355_cwire_despeckle_cwire_batch": "one record per stream, as above: positions stay far below 2^32; the budget call's directory and tail",
}


def dense_headers(T):
    return np.full(T, N, np.uint32), np.zeros(T, np.uint32)


def stream_ends(base, frame_of, S, K):
    """(before [S][N], after [S][N]): the state in front of stream s's first frame and its last frame; frame_of(t) on the host."""
    before = np.stack([base if s == 0 else frame_of(s * K - 1) for s in range(S)])
    return before, np.stack([frame_of((s + 1) * K - 1) for s in range(S)])


def dense_coalesced(before, after, w=BW, h=BH, rects=None):
    """Every byte of every record is an entry, so a stream's summed differences are last - initial modulo 256: the coalesced
    (rects: and cropped, re-indexed) burst -> (offsets, xs, diff, records, frame_pos), from crop_spec and cwire_spec."""
    acc = after - before
    segs = [(np.flatnonzero(a), a[np.flatnonzero(a)]) if rects is None else crop.segment(a, w, h, rects[s]) for s, a in enumerate(acc)]
    off, xs, df = crop.packed(segs)
    return (off, xs, df) + spec.encode(off, xs, df)


def dense_activity(w, h, S, K, geom=CELL):
    """Every byte of K records per stream -> (cells [S][cells], summary [S][8]): K times one full frame's grid (the suite's
    numpy oracle on ONE frame), every cell counted, the box the whole frame."""
    n = 3 * w * h
    cells, summ = activity_oracle(w, h, geom[0], geom[1], geom[2], 1, 1, np.array([0, n], np.uint32), np.arange(n, dtype=np.int32))
    cells, summ = (cells.astype(np.int64) * K).astype(np.uint32), summ.copy()
    summ[0, 0], summ[0, 6] = K * n, K * int(summ[0, 6])
    assert K * n < 1 << 32 and summ[0, 5] == cells.size and list(summ[0, 1:5]) == [0, 0, w - 1, h - 1]
    return np.tile(cells, (S, 1)), np.tile(summ, (S, 1))


def all_tiles(n, S):
    """Every tile of 4096 bytes touched: the tile mask, uint32[S][ceil(tiles / 32)]."""
    t = state_tiles(n)
    row = np.zeros(-(-t // 32), np.uint32)
    for k in range(t):
        row[k // 32] |= np.uint32(1 << (k % 32))
    return np.tile(row, (S, 1))


class DenseRecords:
    """Part 3's frames and their 1100 reference records (templates() with every frame's differences) on the device."""

    def __init__(self, T):
        self.T = T
        self.fr = every_byte_frames(T)
        self.g = BigGuarded(T * REC)
        self.rows = self.g.t.view(T, REC)
        self.fill(lambda a, b, head, diff: (self.rows[a:b, :REC - N].copy_(head.expand(b - a, -1)), self.rows[a:b, REC - N:].copy_(diff)))
        self.ptr = self.g.ptr
        self.counts, self.escapes = dense_headers(T)
        torch.cuda.synchronize()

    def fill(self, each):
        head = to_dev(templates()[1][:REC - N])
        for a, b in slices(self.T, REC):
            each(a, b, head, self.fr.rows[1 + a:1 + b] - self.fr.rows[a:b])

    def check(self):
        """The records and the frames are as they were made (rebuilt slice by slice, nothing kept twice)."""
        torch.cuda.synchronize()
        self.g.check()

        def same(a, b, head, diff):
            assert_rows_on_device(self.rows[a:b, :REC - N], head, "the records are only read", a)
            assert_rows_on_device(self.rows[a:b, REC - N:], diff, "the records are only read", a, REC - N)
        self.fill(same)

    def free(self):
        self.g.free()
        self.fr.free()
        self.rows = None


@pytest.fixture(scope="module")
def dense_records():
    """One record buffer for all consumers; freed, after a last check that nothing wrote it, when the module is done."""
    T = T_LOW
    every_byte_seams(T)
    require(BigGuarded.bytes_needed((T + 1) * N) + BigGuarded.bytes_needed(T * REC) + (3 << 30))
    r = DenseRecords(T)
    try:
        yield r
        r.check()
        r.fr.check()
    finally:
        r.free()


def consumer_core(T=T_LOW, **kw):
    return CUDACore(BW, BH, max_batch=T, threshold=THR, **kw)


def test_every_byte_apply(dense_records):
    """mi355_apply_cwire_batch of the 1100 records onto the base: the state afterwards is the last frame."""
    r = dense_records
    require(log_bytes(r.T, 1))
    with consumer_core(sample_mat_data=every_byte_base()) as core:
        torch.cuda.synchronize()
        core.apply_cwire_batch(r.ptr, r.counts, r.escapes, r.T)
        core.synchronize()
        assert np.array_equal(core.get_state(), every_byte_frame(r.T - 1))
    r.check()


def test_every_byte_check(dense_records):
    """mi355_cwire_check_batch: every verdict clean, no 255 code, no entry past the frame, 1 + the last index = N."""
    r = dense_records
    require(log_bytes(r.T, 1))
    verdicts = Guarded(4 * r.T, I32)
    with consumer_core() as core:
        torch.cuda.synchronize()
        core.cwire_check_batch(r.ptr, r.counts, r.escapes, r.T, verdicts.ptr)
        core.synchronize()
    assert_equal(verdicts.get().view(np.uint32), np.tile(np.array([0, 0, N, N], np.uint32), r.T), "verdicts")
    r.check()


def test_every_byte_decode(dense_records):
    """mi355_cwire_decode_batch: offsets with bit 31 set, xs past 8 GiB, compared on the device."""
    r = dense_records
    T, total = r.T, r.T * N
    require(log_bytes(T, 1) + 5 * total + (3 << 30))
    off, xs, df = Guarded(T + 1, I32), BigGuarded(total + 64, I32), BigGuarded(total + 64)
    try:
        with consumer_core() as core:
            torch.cuda.synchronize()
            core.cwire_decode_batch(r.ptr, r.counts, r.escapes, T, off.ptr, xs.ptr, df.ptr, total + 64)
            core.synchronize()
        assert_equal(off.get().view(np.uint32), (N * np.arange(T + 1, dtype=np.int64)).astype(np.uint32), "offsets")
        xs.check(written=total), df.check(written=total)
        ar = torch.arange(N, dtype=I32, device=DEV)
        for a, b in slices(T, 4 * N):
            assert_rows_on_device(xs.t[a * N:b * N].view(b - a, N), ar, "xs", a)
        for a, b in slices(T, N):
            assert_rows_on_device(df.t[a * N:b * N].view(b - a, N), r.rows[a:b, REC - N:], "diff", a)
    finally:
        xs.free(), df.free()
    r.check()


def test_every_byte_apply_multi_stream(dense_records):
    """mi355_apply_multi_stream_cwire_batch, (S, K) = (2, 550), with output frames: every frame comes back, the states end as
    frames 549 and 1099."""
    r = dense_records
    S, K = CONSUMER_SK
    require(log_bytes(r.T, 1) + r.T * N + (3 << 30))
    before, after = stream_ends(every_byte_base(), every_byte_frame, S, K)
    st, out = Region(S, N).put(before), BigGuarded(r.T * N)
    try:
        with consumer_core() as core:
            torch.cuda.synchronize()
            core.apply_multi_stream_cwire_batch(r.ptr, r.counts, r.escapes, S, K, st.ptr, stride=N, d_frames_out=out.ptr, out_stride=N)
            core.synchronize()
        assert np.array_equal(st.get(), after), "the states afterwards"
        out.check()
        for a, b in slices(r.T, N):
            assert_rows_on_device(out.t[a * N:b * N].view(b - a, N), r.fr.rows[1 + a:1 + b], "the frames out", a)
    finally:
        out.free()
    r.check()


def run_relay(r, rects):
    S, K = CONSUMER_SK
    require(log_bytes(r.T, 1) + (1 << 30))
    before, after = stream_ends(every_byte_base(), every_byte_frame, S, K)
    w_off, _, _, w_recs, w_pos = dense_coalesced(before, after, rects=rects)
    assert (after[1] == before[1]).any() and (w_off[1] == N or rects is not None), "sums of 0 are left out; stream 0 keeps every byte"
    off, pos, out = Guarded(S + 1, I32), Guarded(S + 1, I64), Guarded(w_recs.size + 64)
    with consumer_core() as core:
        torch.cuda.synchronize()
        if rects is None:
            core.cwire_coalesce_cwire_batch(r.ptr, r.counts, r.escapes, S, K, off.ptr, pos.ptr, out.ptr, w_recs.size + 64)
        else:
            core.cwire_crop_cwire_batch(r.ptr, r.counts, r.escapes, S, K, rects, off.ptr, pos.ptr, out.ptr, w_recs.size + 64)
        core.synchronize()
    assert_equal(off.get().view(np.uint32), w_off, "offsets")
    assert_equal(pos.get().view(np.uint64), w_pos, "frame_pos")
    assert_equal(out.get(w_recs.size)[:w_recs.size], w_recs, "the records", w_pos)
    r.check()


def test_every_byte_coalesce(dense_records):
    """mi355_cwire_coalesce_cwire_batch, (2, 550): stream s's record is encode_frame of the non-zero last - initial."""
    run_relay(dense_records, None)


def test_every_byte_crop(dense_records):
    """mi355_cwire_crop_cwire_batch, (2, 550), rectangles that meet the last rows (and the last columns)."""
    run_relay(dense_records, RECTS)


def test_every_byte_activity(dense_records):
    """mi355_cwire_activity_batch, (2, 550), cells of 16 x 16 pixels: every count is 550 x the cell's bytes."""
    r = dense_records
    S, K = CONSUMER_SK
    require(log_bytes(r.T, 1) + (1 << 30))
    w_cells, w_summ = dense_activity(BW, BH, S, K)
    cells, summ = Guarded(w_cells.size, I32), Guarded(w_summ.size, I32)
    with consumer_core() as core:
        torch.cuda.synchronize()
        core.cwire_activity_batch(r.ptr, r.counts, r.escapes, S, K, CELL[0], CELL[1], cells.ptr, summ.ptr, min_count=CELL[2])
        core.synchronize()
    assert_equal(summ.get().view(np.uint32), w_summ.reshape(-1), "summary")
    assert_equal(cells.get().view(np.uint32), w_cells.reshape(-1), "cells")
    r.check()


def test_every_byte_touched_tiles(dense_records):
    """mi355_cwire_touched_tiles_batch, (2, 550): every tile of both streams."""
    r = dense_records
    S, K = CONSUMER_SK
    require(log_bytes(r.T, 1) + (1 << 30))
    want = all_tiles(N, S)
    mask = Guarded(want.size, I32)
    with consumer_core() as core:
        torch.cuda.synchronize()
        core.cwire_touched_tiles_batch(r.ptr, r.counts, r.escapes, S, K, mask.ptr)
        core.synchronize()
    assert_equal(mask.get().view(np.uint32), want.reshape(-1), "the tile mask")
    r.check()


@functools.lru_cache(maxsize=None)
def runs_template():
    """(the run form of templates()' compact record as bytes, r) from runs_spec.to_runs: everything but the differences of any
    record of Part 3 on the link -- header, gap[], len[] -- with the differences, all 0 here, in the last N bytes."""
    run, r = rs.to_runs(templates()[1])
    run = np.frombuffer(run, np.uint8)
    q = spec.pad4(r)
    gap, ln = run[12:12 + r], run[12 + q:12 + q + r]
    assert run.size == rs.runs_frame_bytes(N, 0, r) == 12 + 2 * q + N and rs.smaller(N, r), "the run form is the smaller one"
    assert not gap.any() and (ln[:-1] == 255).all() and int(ln[-1]) == (N - 1) % 256 == 31, "runs of 256 entries and one of 32"
    assert (r, run.size) == (8204, 2116420) and -(-N // 4096) == 513, "513 chunks: three rounds of k_cwr_scan"
    assert not run[run.size - N:].any() and 1100 * run.size < 1 << 32
    run.setflags(write=False)
    return run, r


def link_rows(big, T, RUN):
    return big.t[:T * RUN].view(T, RUN)


def assert_link_on_device(rows, r, head, what):
    """rows [T][RUN] against the template's head and the differences of the dense records, in slices."""
    RUN = rows.shape[1]
    for a, b in slices(r.T, RUN):
        assert_rows_on_device(rows[a:b, :RUN - N], head, f"{what}: header, gap and len", a)
        assert_rows_on_device(rows[a:b, RUN - N:], r.rows[a:b, REC - N:], f"{what}: diff", a, RUN - N)


def test_every_byte_runs_encode(dense_records):
    """mi355_cwire_runs_encode_batch, RUNS_WHERE_SMALLER: input positions pass 2^32 at record 1023, every record is 513 chunks;
    every form row is {1, N, 0, 8204}, pos[b] = 2 116 420 b, a record is the template's header, gap[] and len[] and then the
    compact record's differences; compared on the device."""
    r = dense_records
    T = r.T
    run_t, nr = runs_template()
    RUN = run_t.size
    require(log_bytes(T, 1) + BigGuarded.bytes_needed(T * RUN + 64) + (3 << 30))
    forms, pos, out = Guarded(4 * T, I32), Guarded(T + 1, I64), BigGuarded(T * RUN + 64)
    try:
        with consumer_core() as core:
            torch.cuda.synchronize()
            core.cwire_runs_encode_batch(r.ptr, r.counts, r.escapes, T, lib.RUNS_WHERE_SMALLER, forms.ptr, pos.ptr, out.ptr, T * RUN + 64)
            core.synchronize()
        assert_equal(forms.get().view(np.uint32), np.tile(np.array([1, N, 0, nr], np.uint32), T), "forms")
        assert_equal(pos.get().view(np.uint64), RUN * np.arange(T + 1, dtype=np.uint64), "pos")
        out.check(written=T * RUN)
        assert_link_on_device(link_rows(out, T, RUN), r, to_dev(run_t[:RUN - N]), "the link")
    finally:
        out.free()
    r.check()


def test_every_byte_runs_decode(dense_records):
    """mi355_cwire_runs_decode_batch twice: the link of the 1100 records in the run form (built here from the template and the
    records' differences; output positions pass 2^32) and the dense buffer itself under an all-compact table (input and output
    positions both pass 2^32 on the copy path).  Both give the dense records, compared on the device."""
    r = dense_records
    T = r.T
    run_t, nr = runs_template()
    RUN = run_t.size
    require(log_bytes(T, 1) + BigGuarded.bytes_needed(T * RUN) + BigGuarded.bytes_needed(T * REC) + (3 << 30))
    link, out = BigGuarded(T * RUN), BigGuarded(T * REC)
    try:
        rows, head = link_rows(link, T, RUN), to_dev(run_t[:RUN - N])
        for a, b in slices(T, RUN):
            rows[a:b, :RUN - N] = head
            rows[a:b, RUN - N:] = r.rows[a:b, REC - N:]
        back = out.t.view(T, REC)
        with consumer_core() as core:
            for form, src in ((1, link), (0, r.g)):
                table = np.tile(np.array([form, N, 0, nr], np.uint32), (T, 1))
                fpos = Guarded(T + 1, I64)
                out.buf.fill_(out.fill)
                torch.cuda.synchronize()
                core.cwire_runs_decode_batch(src.ptr, table, T, fpos.ptr, out.ptr, T * REC)
                core.synchronize()
                assert_equal(fpos.get().view(np.uint64), REC * np.arange(T + 1, dtype=np.uint64), f"form {form}: frame_pos")
                out.check()
                for a, b in slices(T, REC):
                    assert_rows_on_device(back[a:b], r.rows[a:b], f"form {form}: the records", a)
        link.check()
        assert_link_on_device(rows, r, head, "the link is only read")
    finally:
        link.free(), out.free()
    r.check()


SPLIT_M = 65536


@functools.lru_cache(maxsize=None)
def split_template():
    """One record of Part 3 (the entries arange(N), all differences 0) split at SPLIT_M by mi355_cwire_split_host, and held to
    split_spec's rule -> (pos int64[pieces + 1], [(a, b)] the entries of each piece, the pieces' bytes).  Every record of the
    buffer has these entries, so this is the layout of every record's pieces; only the differences, the last b - a bytes of a
    piece, change."""
    rec = templates()[1]
    counts, escapes = dense_headers(1)
    first, pos, out = cwire_split_host(rec, counts, escapes, N, SPLIT_M)
    P = int(first[1])
    pos = pos[:P + 1].astype(np.int64)
    cuts = split_spec.cuts(np.arange(N, dtype=np.int64), SPLIT_M)
    assert len(cuts) == P and int(pos[0]) == 0
    for p, (a, b) in enumerate(cuts):
        assert (b - a) % 4 == 0 and int(pos[p + 1] - pos[p]) == split_spec.piece_bytes(np.arange(a, b), 0, b - a) <= SPLIT_M, p
        assert bytes(out[int(pos[p]):int(pos[p + 1])]) == spec.encode_frame(np.arange(a, b), np.zeros(b - a, np.uint8)), p
    assert any(a % split_spec.BLOCK == 0 and a for a, _ in cuts) and sum(b - a for a, b in cuts) == N
    assert P <= cwire_split_pieces_max(N, 0, SPLIT_M) and int(pos[P]) <= cwire_split_bytes_max(N, 0, SPLIT_M)
    out = out[:int(pos[P])].copy()
    out.setflags(write=False)
    return pos, cuts, out


def test_every_byte_split(dense_records):
    """mi355_cwire_split_cwire_batch at max_bytes 65536: input positions pass 2^32 at record 1023, and the call's own 64-bit piece
    positions pass 2^32 between two pieces of record 1022.  piece_first is (pieces per record) * arange, piece_pos the template's
    scan plus (bytes out per record) * the record's index, a piece is the template's header, codes and escape and then the matching
    slice of its record's differences; compared on the device."""
    r = dense_records
    T = r.T
    tpos, cuts, tout = split_template()
    P, OUT = len(cuts), int(tpos[-1])
    piece_cap, cap = T * cwire_split_pieces_max(N, 0, SPLIT_M), T * cwire_split_bytes_max(N, 0, SPLIT_M)
    want_pos = (OUT * np.arange(T, dtype=np.int64)[:, None] + tpos[None, :P]).reshape(-1)
    want_pos = np.append(want_pos, T * OUT).astype(np.uint64)
    cross = int(np.searchsorted(want_pos, 1 << 32))
    assert 0 < cross % P and want_pos[cross - 1] < 1 << 32 <= want_pos[cross], "piece_pos passes 2^32 inside a record's pieces"
    assert T * P <= piece_cap and T * OUT <= cap and (T - 1) * REC >= 1 << 32
    require(log_bytes(T, 1) + BigGuarded.bytes_needed(cap) + (3 << 30))
    first, pos, out = Guarded(T + 1, I32), Guarded(piece_cap + 1, I64), BigGuarded(cap)
    try:
        with consumer_core() as core:
            torch.cuda.synchronize()
            core.cwire_split_cwire_batch(r.ptr, r.counts, r.escapes, T, SPLIT_M, first.ptr, pos.ptr, piece_cap, out.ptr, cap)
            core.synchronize()
        assert_equal(first.get().view(np.uint32), (P * np.arange(T + 1)).astype(np.uint32), "piece_first")
        assert_equal(pos.get(written=T * P + 1)[:T * P + 1].view(np.uint64), want_pos, "piece_pos")
        out.check(written=T * OUT)
        rows = out.t[:T * OUT].view(T, OUT)
        for p, (a, b) in enumerate(cuts):
            at, end = int(tpos[p]), int(tpos[p + 1])
            head = to_dev(tout[at:end - (b - a)])
            for lo, hi in slices(T, OUT):
                assert_rows_on_device(rows[lo:hi, at:end - (b - a)], head, f"piece {p} of every record: header, codes, escape", lo, at)
                assert_rows_on_device(rows[lo:hi, end - (b - a):end], r.rows[lo:hi, REC - N + a:REC - N + b],
                                      f"piece {p} of every record: diff", lo, end - (b - a))
    finally:
        out.free()
    r.check()

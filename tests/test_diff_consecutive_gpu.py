"""-m gpu: mi355_diff_consecutive_batch -- T frames and ONE predecessor; frame t against frame t - 1, no feedback, every
frame read once (k_diff_pack's SEQ form: the previous frame of a wave's tile stays in its registers).

Geometries, the smallest that reach each branch of the pack path:
    64x48    9 216 bytes = 9 full tiles            aligned path only, one launch
    50x37    5 550 bytes                           ragged last tile: the byte path for that tile
    160x140  67 200 bytes = 65 full tiles + ragged 64 tiles and more: two launches on the core's own stream (cut = 32)
Frame counts 1, 2, 3, 4, 5, 8, 9: a register group holds 4 frames and the loop alternates two groups, so these lie either
side of each seam.  max_batch is 16.  What is expected comes from gpu_util.oracle_pairs with prevs = [first_prev, frames[0],
..., frames[T - 2]] (the CPU oracle, frame by frame); every output lies in a guarded buffer."""
import functools

import numpy as np
import pytest
import torch

from cudavideostream_amd import CUDACore as ProductCore
from cudavideostream_amd import lib, synth
from gpu_util import DEV, CUDACore, Guarded, Region, oracle_pairs, to_dev

pytestmark = pytest.mark.gpu

GEOMS = [(64, 48), (50, 37), (160, 140)]
COUNTS = [1, 2, 3, 4, 5, 8, 9]
MAX_BATCH = 16
TMAX = max(COUNTS)


@functools.lru_cache(maxsize=None)
def stream(w, h):
    """(base, frames[TMAX + 1]) of the synthetic webcam stream; read-only, shared by the tests."""
    base, frames = synth.webcam_stream(TMAX + 1, w, h, seed=31)
    base.setflags(write=False)
    frames.setflags(write=False)
    return base, frames


@functools.lru_cache(maxsize=None)
def noise(n, rows, seed):
    """rows x n full-range random bytes; read-only."""
    a = np.random.default_rng(seed).integers(0, 256, (rows, n), dtype=np.uint8)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def cores():
    """One core per (width, height, threshold), made when first asked for."""
    made = {}

    def get(w, h, thr=20):
        if (w, h, thr) not in made:
            made[(w, h, thr)] = CUDACore(w, h, threshold=thr, max_batch=MAX_BATCH)
        c = made[(w, h, thr)]
        c.use_own_stream()
        c.set_option(lib.OPT_PIPELINE, 1)
        return c

    yield get
    for c in made.values():
        c.close()


def prevs_of(first_prev, frames):
    return np.concatenate([first_prev[None, :], frames[:-1]]) if len(frames) else frames


class Out:
    """Guarded offsets, indices and difference bytes of one call."""

    def __init__(self, T, cap):
        self.T, self.cap = T, cap
        self.off, self.xs, self.df = Guarded(T + 1, torch.int32), Guarded(cap, torch.int32), Guarded(cap, torch.uint8)

    def get(self):
        """(offsets, xs, diff) cut to min(total, capacity); asserts that nothing beyond that was written."""
        off = self.off.get().view(np.uint32)
        tot = min(int(off[-1]), self.cap)
        return off, self.xs.get(written=tot)[:tot], self.df.get(written=tot)[:tot]

    def untouched(self):
        self.off.get(written=0), self.xs.get(written=0), self.df.get(written=0)


def consecutive(core, first_prev, frames, T, cap=None, stride=None):
    """One call on device addresses, synchronised; returns Out.get()."""
    out = Out(T, T * core.total if cap is None else cap)
    torch.cuda.synchronize()   # the buffers torch has filled are complete (the core's stream is not torch's)
    core.diff_consecutive_batch(first_prev, frames, T, out.off.ptr, out.xs.ptr, out.df.ptr, out.cap, stride=stride)
    core.synchronize()
    return out.get()


def same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [20, 0])
@pytest.mark.parametrize("T", COUNTS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_equals_the_oracle(po, cores, geom, T, thr):
    w, h = geom
    n = 3 * w * h
    base, frames = stream(w, h)
    frames = frames[:T]
    core = cores(w, h, thr)
    state = noise(n, 1, 5)[0]
    core.set_state(state)
    d_frames = Region(T, n).put(frames)
    d_first = Region(1, n).put([base])   # an allocation of its own
    got = consecutive(core, d_first.ptr, d_frames.ptr, T)
    same(got, oracle_pairs(po, frames, prevs_of(base, frames), thr))
    assert np.array_equal(core.get_state(), state), "the core's state was written"
    assert np.array_equal(d_frames.get(), frames) and np.array_equal(d_first.get()[0], base)


# ---- 2. not the stream form, not a fixed comparand -------------------------------------------------------------------------
def test_no_feedback_and_a_moving_comparand(po, cores):
    w, h, T = 64, 48, 8
    n = 3 * w * h
    core = cores(w, h, 20)
    base = (np.arange(n) % 100 + 10).astype(np.uint8)
    ramp = np.stack([base + 15 * t for t in range(T)]).astype(np.uint8)   # at most 109 + 105: no wrap
    d_first, d_ramp = to_dev(base), to_dev(ramp)
    off, xs, df = consecutive(core, d_first.data_ptr(), d_ramp.data_ptr(), T)
    assert off.tolist() == [0] * (T + 1), "steps of 15 against the frame before never pass a threshold of 20"
    # the same frames through the stream form from the state `base` DO emit (the state lags behind): the input discriminates
    core.set_state(base)
    so = Out(T, T * n)
    core.diff_stream_batch(d_ramp, T, so.off.ptr, so.xs.ptr, so.df.ptr, so.cap)
    core.synchronize()
    s_off, _, _ = so.get()
    assert s_off[-1] > 0 and np.array_equal(s_off, po.diff_stream(ramp, base, 20)[0])
    # a step: entries in frame 1 only; a kernel that kept comparing with first_prev would emit in frames 1..7
    step = np.stack([base] + [base + 100] * (T - 1)).astype(np.uint8)
    d_step = to_dev(step)
    off, xs, df = consecutive(core, d_first.data_ptr(), d_step.data_ptr(), T)
    assert off.tolist() == [0, 0] + [n] * (T - 1)
    assert np.array_equal(xs, np.arange(n, dtype=np.int32)) and (df == 100).all()


# ---- 3. equals the pair form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,T", [((160, 140), 9), ((50, 37), 5)], ids=["160x140-9", "50x37-5"])
def test_equals_the_pair_form_on_one_buffer(po, cores, geom, T):
    w, h = geom
    n = 3 * w * h
    base, frames = stream(w, h)
    core = cores(w, h, 20)
    buf = Region(T + 1, n).put(frames[:T + 1])
    got = consecutive(core, buf.ptr, buf.ptr + n, T)   # first_prev = frames - stride
    pair = Out(T, T * n)
    core.diff_pairs_batch(buf.ptr + n, buf.ptr, T, pair.off.ptr, pair.xs.ptr, pair.df.ptr, pair.cap)
    core.synchronize()
    same(got, pair.get())
    same(got, oracle_pairs(po, frames[1:T + 1], frames[:T], 20))
    assert np.array_equal(buf.get(), frames[:T + 1])


# ---- 4. thresholds of the HIGH compare ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [127, 128, 150, 255])
def test_high_thresholds(po, cores, thr):
    w, h, T = 50, 37, 5
    n = 3 * w * h
    rows = noise(n, T + 1, 9)
    core = cores(w, h, thr)
    d = Region(T + 1, n).put(rows)
    got = consecutive(core, d.ptr, d.ptr + n, T)
    want = oracle_pairs(po, rows[1:], rows[:-1], thr)
    same(got, want)
    assert (want[0][-1] > 0) == (thr < 255)


# ---- 5. the byte path by alignment ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["frames+1", "first_prev+1", "stride+8"])
def test_unaligned_operands_take_the_byte_path(po, cores, case):
    w, h, T = 64, 48, 5
    n = 3 * w * h
    base, frames = stream(w, h)
    frames = frames[:T]
    core = cores(w, h, 20)
    d_frames = Region(T, n, stride=n + 8 if case == "stride+8" else n, skew=1 if case == "frames+1" else 0).put(frames)
    d_first = Region(1, n, skew=1 if case == "first_prev+1" else 0).put([base])
    assert (d_frames.ptr % 16 == 1) == (case == "frames+1") and (d_first.ptr % 16 == 1) == (case == "first_prev+1")
    got = consecutive(core, d_first.ptr, d_frames.ptr, T, stride=d_frames.stride)
    same(got, oracle_pairs(po, frames, prevs_of(base, frames), 20))
    assert np.array_equal(d_frames.get(), frames) and np.array_equal(d_first.get()[0], base)


# ---- 6. where the predecessor may lie ------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(50, 37), (160, 140)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_predecessor_in_the_state_and_in_a_ring(po, cores, geom):
    w, h = geom
    n, T = 3 * w * h, 5
    base, frames = stream(w, h)
    frames = frames[:T]
    core = cores(w, h, 20)
    core.set_state(base)
    d_frames = Region(T, n).put(frames)
    got = consecutive(core, core.state_ptr(), d_frames.ptr, T)
    same(got, oracle_pairs(po, frames, prevs_of(base, frames), 20))
    assert np.array_equal(core.get_state(), base), "the core's state was written"
    # a ring: the predecessor of frame 0 is the buffer's last frame
    got = consecutive(core, d_frames.ptr + (T - 1) * n, d_frames.ptr, T)
    same(got, oracle_pairs(po, frames, prevs_of(frames[T - 1], frames), 20))
    assert np.array_equal(d_frames.get(), frames)


# ---- 7. capacity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(50, 37), (160, 140)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_capacity(po, cores, geom):
    w, h = geom
    n, T = 3 * w * h, 5
    base, frames = stream(w, h)
    frames = frames[:T]
    core = cores(w, h, 20)
    eo, exs, edf = oracle_pairs(po, frames, prevs_of(base, frames), 20)
    cap = int(eo[-1]) // 2
    assert 0 < cap < int(eo[-1])
    d_frames, d_first = to_dev(frames), to_dev(base)
    off, xs, df = consecutive(core, d_first.data_ptr(), d_frames.data_ptr(), T, cap=cap)   # (Out.get: nothing behind cap)
    assert np.array_equal(off, eo), "offsets stay exact"
    assert len(xs) == cap and np.array_equal(xs, exs[:cap]) and np.array_equal(df, edf[:cap])
    # capacity 0 with null arrays: accepted like the pair form, offsets exact
    d_off = Guarded(T + 1, torch.int32)
    core.diff_consecutive_batch(d_first.data_ptr(), d_frames.data_ptr(), T, d_off.ptr, None, None, 0)
    core.synchronize()
    assert np.array_equal(d_off.get().view(np.uint32), eo)


# ---- 8. back to back, nothing synchronised in between ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["own stream", "caller's stream", "pipeline off"])
def test_six_calls_back_to_back(po, cores, mode):
    w, h = 160, 140
    n, T, S = 3 * w * h, 9, 5
    base, frames = stream(w, h)
    core = cores(w, h, 20)
    if mode == "caller's stream":
        core.use_torch_stream()
    elif mode == "pipeline off":
        core.set_option(lib.OPT_PIPELINE, 0)
    rnd = noise(n, S, 13)
    state0 = frames[TMAX]
    core.set_state(state0)
    d_all = Region(TMAX + 1, n).put(frames)
    d_base = Region(1, n).put([base])
    d_states = Region(S, n).put(rnd)   # the many-streams call feeds back into these
    at = lambda t: d_all.ptr + t * n
    # what each call is to give, from the CPU oracle
    s_off, s_xs, s_df, s_state = po.diff_stream(frames[2:2 + S], state0, 20)
    m_off, m_xs, m_df, m_states = [0], [], [], []
    for s in range(S):
        c, x, d, st = po.diff_pack(frames[s], rnd[s], 20)
        m_off.append(m_off[-1] + c), m_xs.append(x), m_df.append(d), m_states.append(st)
    want = [oracle_pairs(po, frames[:T], prevs_of(base, frames[:T]), 20),                     # predecessor elsewhere
            (s_off, s_xs, s_df),
            oracle_pairs(po, frames[1:1 + T], frames[:T], 20),                                 # predecessor = frames - stride
            oracle_pairs(po, frames[1:1 + S], frames[:S], 20),
            oracle_pairs(po, frames[:T], prevs_of(s_state, frames[:T]), 20),                   # predecessor = the core's state,
            (np.array(m_off, np.uint32), np.concatenate(m_xs), np.concatenate(m_df))]          # which the stream call has left
    outs = [Out(T, T * n), Out(S, S * n), Out(T, T * n), Out(S, S * n), Out(T, T * n), Out(S, S * n)]
    o = outs
    torch.cuda.synchronize()
    # the product class's own methods: gpu_util's wrappers would drain the device in front of every call
    P = ProductCore
    P.diff_consecutive_batch(core, d_base.ptr, at(0), T, o[0].off.ptr, o[0].xs.ptr, o[0].df.ptr, o[0].cap)
    P.diff_stream_batch(core, at(2), S, o[1].off.ptr, o[1].xs.ptr, o[1].df.ptr, o[1].cap)
    P.diff_consecutive_batch(core, at(0), at(1), T, o[2].off.ptr, o[2].xs.ptr, o[2].df.ptr, o[2].cap)
    P.diff_pairs_batch(core, at(1), at(0), S, o[3].off.ptr, o[3].xs.ptr, o[3].df.ptr, o[3].cap)
    P.diff_consecutive_batch(core, core.state_ptr(), at(0), T, o[4].off.ptr, o[4].xs.ptr, o[4].df.ptr, o[4].cap)
    P.diff_multi_batch(core, at(0), d_states.ptr, S, o[5].off.ptr, o[5].xs.ptr, o[5].df.ptr, o[5].cap)
    core.synchronize()
    for k in range(6):
        same(outs[k].get(), want[k])
    assert np.array_equal(core.get_state(), s_state), "the stream call's final state"
    assert np.array_equal(d_states.get(), np.stack(m_states))
    assert np.array_equal(d_all.get(), frames) and np.array_equal(d_base.get()[0], base)


# ---- 9. empty and single ------------------------------------------------------------------------------------------------
def test_empty_batch_single_frame_and_empty_frames(po, cores):
    w, h = 50, 37
    n = 3 * w * h
    base, frames = stream(w, h)
    core = cores(w, h, 20)
    d_frames, d_first = to_dev(frames[:1]), to_dev(base)
    out = Out(0, 64)
    torch.cuda.synchronize()
    core.diff_consecutive_batch(d_first.data_ptr(), d_frames.data_ptr(), 0, out.off.ptr, out.xs.ptr, out.df.ptr, out.cap)
    core.synchronize()
    off, xs, df = out.get()   # (asserts that no entry was written)
    assert off.tolist() == [0]
    # null frame pointers are no mistake when there is nothing to read
    out = Out(0, 64)
    core.diff_consecutive_batch(None, None, 0, out.off.ptr, None, None, 0)
    core.synchronize()
    assert out.get()[0].tolist() == [0]
    # one frame: one plain pair
    got = consecutive(core, d_first.data_ptr(), d_frames.data_ptr(), 1)
    c, x, d, _ = po.diff_pack(frames[0], base, 20)
    same(got, (np.array([0, c], np.uint32), x, d))
    # frames of zero bytes: as the pair form handles them
    with CUDACore(0, 0, max_batch=2) as empty:
        for call in (lambda o: empty.diff_consecutive_batch(None, None, 2, o.ptr, None, None, 0),
                     lambda o: empty.diff_pairs_batch(None, None, 2, o.ptr, None, None, 0)):
            d_off = Guarded(3, torch.int32)
            call(d_off)
            empty.synchronize()
            assert d_off.get().tolist() == [0, 0, 0]


# ---- 10. refusals ------------------------------------------------------------------------------------------------
REFUSALS = ["null d_first_prev", "null d_frames", "nframes -1", "nframes max_batch+1", "stride N-1", "null d_offsets",
            "null d_xs", "null d_diff"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals(cores, case):
    w, h, T = 64, 48, 3
    n = 3 * w * h
    base, frames = stream(w, h)
    core = cores(w, h, 20)
    state = noise(n, 1, 5)[0]
    core.set_state(state)
    d_frames, d_first = Region(MAX_BATCH + 1, n).put(frames[:T]), Region(1, n).put([base])
    out = Out(MAX_BATCH + 1, 64)
    a = {"first": d_first.ptr, "frames": d_frames.ptr, "stride": n, "T": T, "off": out.off.ptr, "xs": out.xs.ptr,
         "df": out.df.ptr, "cap": out.cap}
    a.update({"null d_first_prev": {"first": None}, "null d_frames": {"frames": None}, "nframes -1": {"T": -1},
              "nframes max_batch+1": {"T": MAX_BATCH + 1}, "stride N-1": {"stride": n - 1}, "null d_offsets": {"off": None},
              "null d_xs": {"xs": None}, "null d_diff": {"df": None}}[case])
    torch.cuda.synchronize()
    L = lib.load()
    rc = L.mi355_diff_consecutive_batch(core._h, a["first"], a["frames"], a["stride"], a["T"], a["off"], a["xs"], a["df"], a["cap"])
    assert rc == lib.ERR_INVALID
    assert L.mi355_last_error(), "no text for the refusal"
    core.synchronize()
    out.untouched()
    assert np.array_equal(core.get_state(), state)
    assert np.array_equal(d_frames.get()[:T], frames[:T]) and np.array_equal(d_first.get()[0], base)

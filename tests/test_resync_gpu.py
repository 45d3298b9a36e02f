"""-m gpu: mi355_state_digest_batch, mi355_refresh_cwire_batch, mi355_state_clear_tiles_batch (include/mi355diff.h,
"Resynchronising a receiver").  The reference of every comparison is numpy: resync_spec (the digest and the refresh record, the
latter encoded by cwire_spec), never the code under test.  States, inputs and outputs live in guarded buffers (gpu_util) that
start as a non-zero pattern.

Shapes, the smallest at which each seam exists: 33x7 (N = 693: one ragged tile, N odd; also stride == N on a skewed base),
64x48 (N = 9216: tile edges), 256x171 (N = 131328: 33 tiles, the mask's second word holds one bit), 800x450 (N = 1080000: 264
tiles with a ragged last, the second round of k_cwc_scan), 33x7 with S = 1025 (the second round of k_cwc_place)."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
import resync_spec as rs
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib, state_digest_host
from gpu_util import GUARD, CUDACore, Guarded, Region

pytestmark = pytest.mark.gpu

SHAPES = [(33, 7), (64, 48), (256, 171), (800, 450)]
# (skew of the base, stride - N): every stream 16-byte aligned where N allows; stride == N on a skewed base; an odd stride
LAYOUTS = [(0, None), (5, 0), (0, 3)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sender_states(w, h, S, zero_tile=1):
    """[S][N] states: random bytes, two in five of them zero; stream 0 holds tile `zero_tile` all zero (where it exists)."""
    n = 3 * w * h
    rng = np.random.default_rng(1000 * w + h + S)
    st = rng.integers(1, 256, (S, n), dtype=np.uint8)
    st[rng.random((S, n)) < 0.4] = 0
    if rs.tiles(n) > zero_tile:
        st[0, zero_tile * rs.TILE:(zero_tile + 1) * rs.TILE] = 0
    st.setflags(write=False)
    return st


def aligned_stride(n, extra):
    """The layout's stride: None -> the next multiple of 16 (every stream aligned), else N + extra."""
    return (n + 15) // 16 * 16 if extra is None else n + extra


def damaged(sender, plan):
    """A copy of the sender's states with, per (stream, tile) of `plan`, the tile's last byte changed -- the last word of the
    tile -- or, where the sender's tile is all zero, the whole tile filled with other bytes.  -> (states, bool[S, tiles])."""
    S, n = sender.shape
    recv = sender.copy()
    sel = np.zeros((S, rs.tiles(n)), bool)
    for s, t in plan:
        lo, hi = t * rs.TILE, min(n, (t + 1) * rs.TILE)
        if sender[s, lo:hi].any():
            recv[s, hi - 1] ^= 0x5A
        else:
            recv[s, lo:hi] = (np.arange(hi - lo) % 251 + 1).astype(np.uint8)
        sel[s, t] = True
    return recv, sel


def plan_for(n, S):
    """Stream 0: the first tile, the last (ragged) tile, tiles 31 and 32, the tile the sender holds all zero; stream 1: its last
    byte only; the last stream: nothing."""
    t = rs.tiles(n)
    plan = {(0, 0), (0, t - 1)} | {(0, k) for k in (1, 31, 32) if k < t}
    if S > 2:
        plan.add((1, t - 1))
    return sorted(plan)


# ---- the calls on guarded buffers -----------------------------------------------------------------------------------------
def run_digest(core, states, S):
    """-> uint32[S, tiles, 2]; the guards of the digests asserted, the states' by the caller."""
    t = rs.tiles(states.n)
    out = Guarded(2 * S * t, torch.int32)
    torch.cuda.synchronize()
    core.state_digest_batch(states.ptr, S, out.ptr, stride=states.stride)
    core.synchronize()
    return out.get().view(np.uint32).reshape(S, t, 2)


class Refresh:
    """One mi355_refresh_cwire_batch call on guarded outputs.  core None: the buffers only, for a caller that makes the call
    itself (call()) inside a chain, behind a synchronisation of its own."""

    def __init__(self, core, snd, S, peer=None, cap=None):
        n = snd.n
        self.S, self.n, self.cap = S, n, cwire_bytes_max(n, S) if cap is None else cap
        self.mask = Guarded(S * rs.mask_words(n), torch.int32)
        self.off, self.pos, self.out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(self.cap)
        if isinstance(peer, np.ndarray):                  # (a Guarded: the digests where mi355_state_digest_batch put them)
            peer = Guarded(peer.size, torch.int32, data=np.ascontiguousarray(peer).view(np.int32).ravel())
        self.peer = peer
        if core is not None:
            torch.cuda.synchronize()
            self.call(core, snd)
            core.synchronize()

    def call(self, core, snd):
        """The call alone: nothing is allocated, filled or synchronised here."""
        core.refresh_cwire_batch(snd.ptr, self.S, None if self.peer is None else self.peer.ptr, self.mask.ptr, self.off.ptr,
                                 self.pos.ptr, self.out.ptr, self.cap, stride=snd.stride)

    def results(self):
        """(mask uint32[S, mask_words], offsets uint32[S + 1], frame_pos uint64[S + 1], the whole record buffer)."""
        if self.peer is not None:
            self.peer.get()
        return (self.mask.get().view(np.uint32).reshape(self.S, rs.mask_words(self.n)), self.off.get().view(np.uint32),
                self.pos.get().view(np.uint64), self.out.get())


def check_refresh(r, sender, sel):
    """The call's outputs against the numpy reference, byte for byte; nothing behind the last record is written.
    -> (records, counts, escapes)."""
    want_mask, want_off, want_recs, want_pos = rs.refresh(sender, sel)
    mask, off, pos, out = r.results()
    assert np.array_equal(mask, want_mask)
    assert np.array_equal(off, want_off) and np.array_equal(pos, want_pos)
    assert np.array_equal(out[:want_recs.size], want_recs)
    assert (out[want_recs.size:] == GUARD).all(), "written behind the last record"
    counts, escapes = spec.headers(want_recs, sender.shape[0])
    return want_recs, counts, escapes


def check_verdicts(core, r, counts, escapes):
    """mi355_cwire_check_batch on the records where they lie: word 0 == 0 for every record."""
    S = len(counts)
    v = Guarded(4 * S, torch.int32)
    torch.cuda.synchronize()
    core.cwire_check_batch(r.out.ptr, counts, escapes, S, v.ptr)
    core.synchronize()
    assert (v.get().view(np.uint32).reshape(S, 4)[:, 0] == 0).all()


def clear_and_apply(core, rcv, r, counts, escapes):
    """The receiver's two calls, on one stream with no synchronisation in between."""
    torch.cuda.synchronize()
    core.state_clear_tiles_batch(rcv.ptr, r.S, r.mask.ptr, stride=rcv.stride)
    core.apply_multi_cwire_batch(r.out.ptr, counts, escapes, r.S, rcv.ptr, stride=rcv.stride)
    core.synchronize()


# ---- 1. the digest --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skew,extra", LAYOUTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_device_digest_equals_host_digest(w, h, skew, extra):
    S, n = 3, 3 * w * h
    sender = sender_states(w, h, S)
    states = Region(S, n, aligned_stride(n, extra), skew).put(sender)
    with CUDACore(w, h, max_batch=S) as core:
        got = run_digest(core, states, S)
    assert np.array_equal(states.get(), sender)          # guards and stride gaps intact, the states only read
    want = np.stack([rs.digest(sender[s]) for s in range(S)])
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], state_digest_host(sender[0]))


# ---- 2. the round trip ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skew,extra", LAYOUTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_round_trip(w, h, skew, extra):
    """Receiver states that equal the sender's but for damaged tiles: the mask is exactly those tiles; records, offsets and
    positions are the reference's; every record is clean; clear + apply restores every state; the undamaged stream's record
    is 8 bytes and its state is untouched."""
    S, n = 3, 3 * w * h
    sender = sender_states(w, h, S)
    recv, sel = damaged(sender, plan_for(n, S))
    stride = aligned_stride(n, extra)
    snd, rcv = Region(S, n, stride, skew).put(sender), Region(S, n, stride, skew).put(recv)
    with CUDACore(w, h, max_batch=S) as core:
        peer = run_digest(core, rcv, S)
        assert np.array_equal(rs.selected_tiles(sender, peer), sel)       # (the reference finds the damage, too)
        r = Refresh(core, snd, S, peer)
        recs, counts, escapes = check_refresh(r, sender, sel)
        assert counts[S - 1] == 0 and int(r.results()[2][S]) - int(r.results()[2][S - 1]) == 8
        check_verdicts(core, r, counts, escapes)
        clear_and_apply(core, rcv, r, counts, escapes)
    assert np.array_equal(rcv.get(), sender)
    assert np.array_equal(snd.get(), sender)
    # a host client: clears the tiles itself and applies the same records
    host = recv.copy()
    host[rs.byte_selection(sel, n)] = 0
    at = 0
    for s in range(S):
        at += cwire_apply_host(host[s], recs[at:], 1)
    assert at == recs.size and np.array_equal(host, sender)


def test_round_trip_behind_the_coalescer():
    """The refresh records through mi355_cwire_coalesce_cwire_batch (a relay) come out as they went in and repair the receiver."""
    w, h, S = 64, 48, 3
    n = 3 * w * h
    sender = sender_states(w, h, S)
    recv, sel = damaged(sender, plan_for(n, S))
    snd, rcv = Region(S, n).put(sender), Region(S, n).put(recv)
    with CUDACore(w, h, max_batch=S) as core:
        r = Refresh(core, snd, S, run_digest(core, rcv, S))
        recs, counts, escapes = check_refresh(r, sender, sel)
        cap = cwire_bytes_max(n, S)
        off, pos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
        torch.cuda.synchronize()
        core.cwire_coalesce_cwire_batch(r.out.ptr, counts, escapes, S, 1, off.ptr, pos.ptr, out.ptr, cap)
        core.state_clear_tiles_batch(rcv.ptr, S, r.mask.ptr)
        core.apply_multi_cwire_batch(out.ptr, counts, escapes, S, rcv.ptr)
        core.synchronize()
    assert np.array_equal(out.get()[:recs.size], recs)
    assert np.array_equal(rcv.get(), sender)


def test_many_streams():
    """S = 1025: the second round of k_cwc_place."""
    w, h, S = 33, 7, 1025
    n = 3 * w * h
    sender = sender_states(w, h, S)
    recv, sel = damaged(sender, [(s, 0) for s in (0, 3, 1023, 1024)])
    snd, rcv = Region(S, n, n, 1).put(sender), Region(S, n, n, 1).put(recv)
    with CUDACore(w, h, max_batch=S) as core:
        r = Refresh(core, snd, S, run_digest(core, rcv, S))
        _, counts, escapes = check_refresh(r, sender, sel)
        check_verdicts(core, r, counts, escapes)
        clear_and_apply(core, rcv, r, counts, escapes)
    assert np.array_equal(rcv.get(), sender)


# ---- 3. a key frame -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(33, 7), (256, 171)])
def test_null_peer_selects_every_tile(w, h):
    S, n = 2, 3 * w * h
    sender = sender_states(w, h, S)
    sel = np.ones((S, rs.tiles(n)), bool)
    snd, rcv = Region(S, n, n + 3, 1).put(sender), Region(S, n, n + 3, 1).put(np.zeros((S, n), np.uint8))
    with CUDACore(w, h, max_batch=S) as core:
        r = Refresh(core, snd, S, None)
        _, counts, escapes = check_refresh(r, sender, sel)
        core.apply_multi_cwire_batch(r.out.ptr, counts, escapes, S, rcv.ptr, stride=rcv.stride)   # zero-filled: nothing to clear
        core.synchronize()
    assert np.array_equal(rcv.get(), sender)


# ---- 4. crafted states ----------------------------------------------------------------------------------------------------
def crafted_states(n):
    """[N = 9216: tiles [0, 4096), [4096, 8192), [8192, 9216)] sparse states, one per row."""
    rows = [
        [100, 355, 611, 868],                       # gaps of exactly 254, 255 and 256 inside a tile
        [4000, 4255, 8000, 8255],                   # 254 across both tile edges
        [4090, 4346, 8190, 8446],                   # 255 across both tile edges
        [4090, 4347, 8190, 8447],                   # 256 across both tile edges
        [3841, 4096, 4352, 4609, 8192],             # 254, 255, 256 from the last byte before / first byte behind an edge
        [4000, 5000, 8200],                         # an escape that spans a skipped tile when tile 1 is not selected
        [4095, 4096, 8191, 8192, n - 1],            # neighbours across the edges; the last byte
        [300],                                      # a first entry >= 255
        [5000],                                     # a first entry in a later tile
        [],                                         # an all-zero state
    ]
    st = np.zeros((len(rows), n), np.uint8)
    for s, xs in enumerate(rows):
        st[s, xs] = (np.arange(len(xs)) * 37 + 1 + s).astype(np.uint8)
    return st


@pytest.mark.parametrize("tiles", [(0, 1, 2), (0, 2), (1,), (1, 2), (0,)], ids=str)
def test_crafted_gaps(tiles):
    """Every stream has the tiles of `tiles` selected (the receiver differs there): the same gaps inside a tile, across a tile
    edge, and across tiles that are not selected -- where the entry on the far side is the next selected tile's."""
    w, h = 64, 48
    n = 3 * w * h
    sender = crafted_states(n)
    S = sender.shape[0]
    recv = sender.copy()
    sel = np.zeros((S, 3), bool)
    for t in tiles:
        recv[:, t * rs.TILE + 7] ^= 0x11             # (byte 7 of a tile is zero in every crafted state)
        sel[:, t] = True
    snd, rcv = Region(S, n).put(sender), Region(S, n).put(recv)
    with CUDACore(w, h, max_batch=S) as core:
        r = Refresh(core, snd, S, run_digest(core, rcv, S))
        _, counts, escapes = check_refresh(r, sender, sel)
        check_verdicts(core, r, counts, escapes)
        clear_and_apply(core, rcv, r, counts, escapes)
    if tiles == (0, 2):
        assert escapes[5] == 2                       # 4000 as a first entry, then 4000 -> 8200 over the skipped tile
    assert np.array_equal(rcv.get(), sender)


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------
def test_a_record_that_does_not_fit_is_skipped_whole():
    w, h, S = 64, 48, 3
    n = 3 * w * h
    sender = sender_states(w, h, S)
    sel = np.ones((S, rs.tiles(n)), bool)
    want_mask, want_off, want_recs, want_pos = rs.refresh(sender, sel)
    snd = Region(S, n).put(sender)
    with CUDACore(w, h, max_batch=S) as core:
        for fit, cap in [(1, int(want_pos[2]) - 4), (1, int(want_pos[1])), (0, int(want_pos[1]) - 4), (2, int(want_pos[3]) - 4),
                         (3, int(want_pos[3]))]:
            mask, off, pos, out = Refresh(core, snd, S, None, cap=cap).results()
            assert np.array_equal(mask, want_mask) and np.array_equal(off, want_off) and np.array_equal(pos, want_pos)
            end = int(want_pos[fit])
            assert np.array_equal(out[:end], want_recs[:end])
            assert (out[end:] == GUARD).all(), "a byte of a record that does not fit was written"
    assert np.array_equal(snd.get(), sender)


# ---- 6. the clear alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,skew,extra", [(33, 7, 5, 0), (64, 48, 3, 5), (256, 171, 0, None), (256, 171, 9, 0),
                                            (1367, 1, 9, 0), (1367, 1, 0, 2), (1, 1, 9, 0), (1, 1, 14, 1)])
def test_clear_zeroes_the_selected_tiles_only(w, h, skew, extra):
    """1367x1 (N = 4101): a last tile of 5 bytes -- on the skewed base it starts 9 + 4096 bytes behind an aligned address and ends
    before the next 16-byte boundary (no whole 16-byte store, head == len), on the odd stride streams 1 and 2 differ; 1x1 (N = 3):
    a state shorter than 16 bytes, inside one 16-byte line and across a boundary (skew 14)."""
    S, n = 3, 3 * w * h
    t, mw = rs.tiles(n), rs.mask_words(n)
    states = sender_states(w, h, S)
    sel = np.zeros((S, t), bool)
    sel[0, [0, t - 1]] = True
    sel[1, ::2] = True
    sel[2, t - 1] = True
    mask = rs.mask_of(sel)
    for s in range(S):                                # bits at or past `tiles` are ignored
        mask[s, mw - 1] |= np.uint32((0xFFFFFFFF << (t - 32 * (mw - 1))) & 0xFFFFFFFF) if t % 32 else np.uint32(0)
    reg = Region(S, n, aligned_stride(n, extra), skew).put(states)
    d_mask = Guarded(S * mw, torch.int32, data=mask.view(np.int32).ravel())
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        core.state_clear_tiles_batch(reg.ptr, S, d_mask.ptr, stride=reg.stride)
        core.synchronize()
    want = states.copy()
    want[rs.byte_selection(sel, n)] = 0
    assert np.array_equal(reg.get(), want)            # (and no guard byte or stride gap was written)
    assert np.array_equal(d_mask.get().view(np.uint32).reshape(S, mw), mask)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, S = 64, 48, 2
    n = 3 * w * h
    t, mw = rs.tiles(n), rs.mask_words(n)
    sender = sender_states(w, h, S)
    cap = cwire_bytes_max(n, S)
    snd = Region(S, n, n + 16).put(sender)
    span = (S - 1) * snd.stride + n
    peer = Guarded(2 * S * t, torch.int32)
    dig, mask, off, pos, out = (Guarded(2 * S * t, torch.int32), Guarded(S * mw, torch.int32), Guarded(S + 1, torch.int32),
                                Guarded(S + 1, torch.int64), Guarded(cap))
    with CUDACore(w, h, max_batch=S) as core:
        torch.cuda.synchronize()
        L, H = core._lib, core._h

        def digest(st=snd.ptr, stride=snd.stride, k=S, d=dig.ptr):
            return L.mi355_state_digest_batch(H, st, stride, k, d)

        def refresh(st=snd.ptr, stride=snd.stride, k=S, p=peer.ptr, m=mask.ptr, o=off.ptr, f=pos.ptr, c=out.ptr, cap=cap):
            return L.mi355_refresh_cwire_batch(H, st, stride, k, p, m, o, f, c, cap)

        def clear(st=snd.ptr, stride=snd.stride, k=S, m=mask.ptr):
            return L.mi355_state_clear_tiles_batch(H, st, stride, k, m)

        refused = [
            digest(k=-1), digest(k=S + 1), digest(st=None), digest(d=None), digest(stride=n - 1), digest(d=dig.ptr + 2),
            digest(d=snd.ptr), digest(d=snd.ptr + span - 4), digest(d=snd.ptr - 8 * S * t + 4),
            refresh(k=-1), refresh(k=S + 1), refresh(st=None), refresh(m=None), refresh(o=None), refresh(f=None), refresh(c=None),
            refresh(stride=n - 1),
            refresh(p=peer.ptr + 2), refresh(m=mask.ptr + 2), refresh(o=off.ptr + 2), refresh(c=out.ptr + 2),   # not 4-byte aligned
            refresh(f=pos.ptr + 4),                                                                             # not 8-byte aligned
            refresh(m=snd.ptr), refresh(o=snd.ptr + span - 4), refresh(f=snd.ptr + 8), refresh(c=snd.ptr - cap + 4),   # the states
            refresh(m=peer.ptr), refresh(o=peer.ptr + 4), refresh(f=peer.ptr + 8 * S * t - 8), refresh(c=peer.ptr - cap + 4),
            refresh(m=off.ptr), refresh(o=out.ptr + 8), refresh(f=out.ptr + cap - 8), refresh(c=mask.ptr - cap + 4),   # each other
            refresh(f=off.ptr - 8),
            clear(k=-1), clear(k=S + 1), clear(st=None), clear(m=None), clear(stride=n - 1), clear(m=mask.ptr + 2),
            clear(m=snd.ptr + 16), clear(m=snd.ptr + span - 4),
        ]
        assert refused == [lib.ERR_INVALID] * len(refused)
        assert digest(k=0) == lib.OK and digest(k=0, st=None, d=None) == lib.OK          # nothing to do
        assert clear(k=0) == lib.OK and clear(k=0, st=None, m=None) == lib.OK
        core.synchronize()
        assert np.array_equal(snd.get(), sender)
        for g in (peer, dig, mask, off, pos, out):
            g.get(written=0)
        # nstreams == 0: offsets[0] = 0 and frame_pos[0] = 0 and nothing else
        assert refresh(k=0) == lib.OK
        core.synchronize()
        assert off.get(written=1)[0] == 0 and pos.get(written=1)[0] == 0
        mask.get(written=0), out.get(written=0)
        # ... and a null d_offsets or d_frame_pos is skipped there, as in the coalescer: nothing is looked at but the alignment
        assert refresh(k=0, st=None, p=None, m=None, o=None, f=None, c=None, cap=0) == lib.OK
        assert refresh(k=0, o=None) == lib.OK and refresh(k=0, f=None) == lib.OK
        assert refresh(k=0, o=off.ptr + 2) == lib.ERR_INVALID and refresh(k=0, f=pos.ptr + 4) == lib.ERR_INVALID
        core.synchronize()
        off.get(written=1), pos.get(written=1)
        # right behind the states is not an overlap
        assert digest(k=1, d=snd.ptr + n + 3) == lib.ERR_INVALID                         # (not aligned)
        assert digest(k=1, stride=n, d=snd.ptr + snd.stride) == lib.OK
        core.synchronize()
    got = snd.buf.cpu().numpy()[snd.lo + snd.stride:snd.lo + snd.stride + 8 * t].view(np.uint32).reshape(t, 2)
    assert np.array_equal(got, rs.digest(sender[0]))


# ---- 8. ordering ----------------------------------------------------------------------------------------------------------
def test_unsynchronised_chain_equals_the_synchronised_run():
    """A sender tick (mi355_diff_multi_cwire_batch), the receiver's digests, the refresh, the clear and the apply on ONE core:
    enqueued back to back they give what they give with a synchronisation behind every call.  Every buffer is made and filled
    before the chain starts; between the five calls of the second run nothing touches the device or waits for it, so the
    refresh reads the states the tick is still writing and the digests the call before it is still making."""
    w, h, S = 256, 171, 3
    n = 3 * w * h
    rng = np.random.default_rng(77)
    base = sender_states(w, h, S)
    frames = base.copy()
    frames[:, rng.integers(0, n, 4000)] += np.uint8(90)          # the tick: about 4000 bytes per stream move past the threshold
    recv0, _ = damaged(base, plan_for(n, S))
    cap = cwire_bytes_max(n, S)
    results = []
    counts = escapes = None
    with CUDACore(w, h, max_batch=S) as core:
        for sync in (True, False):
            snd, rcv, fr = Region(S, n).put(base), Region(S, n).put(recv0), Region(S, n).put(frames)
            t_off, t_pos, t_out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
            dig = Guarded(2 * S * rs.tiles(n), torch.int32)
            r = Refresh(None, snd, S, dig)                        # (the digests where the digest call puts them)
            torch.cuda.synchronize()                              # the last wait of the unsynchronised run before its end
            step = core.synchronize if sync else (lambda: None)
            core.diff_multi_cwire_batch(fr.ptr, snd.ptr, S, t_off.ptr, t_pos.ptr, t_out.ptr, cap)
            step()
            core.state_digest_batch(rcv.ptr, S, dig.ptr)
            step()
            r.call(core, snd)
            step()
            if sync:                                              # the headers of the refresh records, for both runs
                pos = r.pos.get().view(np.uint64)
                counts, escapes = spec.headers(r.out.get()[:int(pos[S])], S)
            core.state_clear_tiles_batch(rcv.ptr, S, r.mask.ptr)
            step()
            core.apply_multi_cwire_batch(r.out.ptr, counts, escapes, S, rcv.ptr)
            core.synchronize()
            results.append((snd.get(), rcv.get(), dig.get(), t_out.get()) + r.results())
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    snd_after, rcv_after = results[0][0], results[0][1]
    assert not np.array_equal(snd_after, base)                    # the tick moved the sender's states ...
    sel = rs.selected_tiles(snd_after, np.stack([rs.digest(recv0[s]) for s in range(S)]))
    want = recv0.copy()
    want[rs.byte_selection(sel, n)] = snd_after[rs.byte_selection(sel, n)]
    assert np.array_equal(rcv_after, want)                        # ... and the receiver has them in every selected tile
    assert np.array_equal(results[0][4], rs.mask_of(sel))

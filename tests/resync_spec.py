"""The tile digest and the refresh record (include/mi355diff.h, "Resynchronising a receiver") stated in numpy: the tests'
reference.  Test infrastructure only; the product never imports it."""
import numpy as np

import cwire_spec as spec

TILE = 4096


def tiles(n):
    return (int(n) + TILE - 1) // TILE


def mask_words(n):
    return (tiles(n) + 31) // 32


def mix(v):
    """The 32-bit finaliser h of the header, on a uint64 array of values below 2^32."""
    m = np.uint64(0xFFFFFFFF)
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x85EBCA6B)) & m
    v = v ^ (v >> np.uint64(13))
    v = (v * np.uint64(0xC2B2AE35)) & m
    return v ^ (v >> np.uint64(16))


def digest(state):
    """uint32[tiles, 2] of a uint8 array: per tile, zero-extended to 4096 bytes and read as little-endian words w_i:
    {sum w_i, sum h(w_i ^ 0x9E3779B9 * (i + 1))}, both mod 2^32."""
    state = np.asarray(state, np.uint8)
    t = tiles(state.size)
    padded = np.zeros(t * TILE, np.uint8)
    padded[:state.size] = state
    w = padded.view("<u4").astype(np.uint64).reshape(t, TILE // 4)
    key = (np.uint64(0x9E3779B9) * np.arange(1, TILE // 4 + 1, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    out = np.empty((t, 2), np.uint32)
    out[:, 0] = (w.sum(axis=1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out[:, 1] = (mix(w ^ key).sum(axis=1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out


def selected_tiles(sender, peer_digests):
    """bool[S, tiles]: either word of the peer's digest differs from the sender's; peer_digests None: every tile."""
    S, n = sender.shape
    if peer_digests is None:
        return np.ones((S, tiles(n)), bool)
    mine = np.stack([digest(sender[s]) for s in range(S)]) if S else np.empty((0, tiles(n), 2), np.uint32)
    return (mine != np.asarray(peer_digests).reshape(S, tiles(n), 2)).any(axis=2)


def mask_of(sel):
    """bool[S, tiles] -> uint32[S, mask_words]."""
    S, t = sel.shape
    out = np.zeros((S, (t + 31) // 32), np.uint32)
    for s, tl in zip(*np.nonzero(sel)):
        out[s, tl >> 5] |= np.uint32(1) << np.uint32(tl & 31)
    return out


def byte_selection(sel, n):
    """bool[S, tiles] -> bool[S, n]: the bytes of the selected tiles."""
    return np.repeat(sel, TILE, axis=1)[:, :n]


def refresh(sender, sel):
    """-> (mask uint32[S, mask_words], offsets uint32[S + 1], records uint8, frame_pos uint64[S + 1]): record s holds
    (x, sender[s][x]) for the nonzero bytes of the selected tiles, ascending, in the canonical encoding of cwire_spec."""
    S, n = sender.shape
    bytes_sel = byte_selection(sel, n)
    off, xs, df = [0], [], []
    for s in range(S):
        x = np.flatnonzero(bytes_sel[s] & (sender[s] != 0))
        xs.append(x.astype(np.int32)); df.append(sender[s][x])
        off.append(off[-1] + x.size)
    xs = np.concatenate(xs + [np.empty(0, np.int32)]).astype(np.int32)
    df = np.concatenate(df + [np.empty(0, np.uint8)]).astype(np.uint8)
    off = np.array(off, np.uint32)
    recs, pos = spec.encode(off, xs, df)
    return mask_of(sel), off, recs, pos

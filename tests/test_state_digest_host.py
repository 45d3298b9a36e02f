"""mi355_state_digest_host, the definition of the tile digest (include/mi355diff.h, "Resynchronising a receiver"): the three
fixed vectors of the format, equality with a numpy statement of the definition (resync_spec.digest) on random states, the two
properties the header states -- an edit inside one word always changes word 0 of that tile and of no other, a swap of two
unequal words changes word 1 and leaves word 0 -- and the refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import resync_spec as rs
from cudavideostream_amd import lib, state_digest_host, state_tiles


def pattern(n):
    return ((7 * np.arange(n) + 3) & 255).astype(np.uint8)


@pytest.mark.parametrize("state,want", [
    (np.zeros(4096, np.uint8), (0x00000000, 0x1C878011)),
    (pattern(4096), (0xFE020400, 0x17B24FFC)),
    (pattern(693), (0xD51B623E, 0xD9F605F8)),        # one ragged tile, N % 4 = 1
], ids=["zeros", "pattern", "ragged"])
def test_fixed_vectors(state, want):
    got = state_digest_host(state)
    assert got.shape == (1, 2) and got.dtype == np.uint32
    assert (int(got[0, 0]), int(got[0, 1])) == want
    assert np.array_equal(rs.digest(state), got)    # (the numpy statement gives the same vectors)


@pytest.mark.parametrize("n", [693, 9216, 131328])
def test_equals_the_numpy_statement_on_random_states(n):
    """693: one ragged tile; 9216: two whole tiles and one of 1024 bytes; 131328: 33 tiles."""
    rng = np.random.default_rng(n)
    for trial in range(3):
        state = rng.integers(0, 256, n, dtype=np.uint8)
        if trial == 1:
            state[rng.random(n) < 0.9] = 0         # mostly zero, like a state of differences
        got = state_digest_host(state)
        assert got.shape == (state_tiles(n), 2)
        assert np.array_equal(got, rs.digest(state))
        # an unaligned view of the same bytes gives the same digests
        shifted = np.empty(n + 1, np.uint8)
        shifted[1:] = state
        assert np.array_equal(state_digest_host(shifted[1:]), got)


def test_digests_of_bytes_and_arrays_agree():
    state = pattern(5000)
    assert np.array_equal(state_digest_host(state.tobytes()), state_digest_host(state))


@pytest.mark.parametrize("n,tile", [(693, 0), (9216, 1), (9216, 2)])
def test_every_single_byte_edit_changes_word_0_of_its_tile_only(n, tile):
    rng = np.random.default_rng(5 + n + tile)
    state = rng.integers(0, 256, n, dtype=np.uint8)
    base = state_digest_host(state)
    lo, hi = tile * rs.TILE, min(n, (tile + 1) * rs.TILE)
    others = np.arange(base.shape[0]) != tile
    for x in range(lo, hi):
        old = state[x]
        state[x] = old ^ (1 + (x % 255))           # every edit differs from the byte it replaces
        d = state_digest_host(state)
        assert d[tile, 0] != base[tile, 0], x
        assert np.array_equal(d[others], base[others]), x
        state[x] = old
    assert np.array_equal(state_digest_host(state), base)


def test_swapping_two_unequal_words_changes_word_1_only():
    rng = np.random.default_rng(11)
    state = rng.integers(0, 256, 9216, dtype=np.uint8)
    base = state_digest_host(state)
    words = state.view("<u4")
    for i, j in [(0, 1), (0, 1023), (5, 700), (1024, 2047), (2048, 2303)]:   # pairs inside one tile each
        assert words[i] != words[j] and i // 1024 == j // 1024
        words[i], words[j] = words[j], words[i]
        d = state_digest_host(state)
        t = i // 1024
        assert d[t, 0] == base[t, 0] and d[t, 1] != base[t, 1], (i, j)
        assert np.array_equal(np.delete(d, t, axis=0), np.delete(base, t, axis=0))
        words[i], words[j] = words[j], words[i]


def test_refusals_leave_the_output_untouched():
    L = lib.load()
    state = pattern(693)
    out = np.full(2, 0xABCDABCD, np.uint32)
    assert L.mi355_state_digest_host(None, 693, out.ctypes.data) == lib.ERR_INVALID
    assert (out == 0xABCDABCD).all()
    assert L.mi355_state_digest_host(state.ctypes.data, 693, None) == lib.ERR_INVALID
    assert L.mi355_state_digest_host(None, 0, None) == lib.OK            # nothing to digest: no pointer is looked at
    assert L.mi355_state_digest_host(state.ctypes.data, 0, out.ctypes.data) == lib.OK
    assert (out == 0xABCDABCD).all()
    assert L.mi355_state_tiles(0) == 0
    assert state_digest_host(np.empty(0, np.uint8)).shape == (0, 2)


def test_output_needs_no_alignment():
    L = lib.load()
    state = pattern(9216)
    raw = np.zeros(3 * 8 + 1, np.uint8)
    assert L.mi355_state_digest_host(state.ctypes.data, state.size, C.c_void_p(raw.ctypes.data + 1)) == lib.OK
    assert np.array_equal(raw[1:].view("<u4").reshape(3, 2), rs.digest(state))

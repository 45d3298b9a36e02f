"""The compact wire format without a GPU: the library's host client (mi355_cwire_apply_host) against the numpy statement of
the format (tests/cwire_spec.py) and the oracle's client, the byte counts of the format, and the host client's refusal of
every kind of malformed record."""
import ctypes as C

import numpy as np
import pytest

import cwire_spec as spec
from conftest import golden
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, cwire_frame_bytes, lib, synth


def frames_stream(frames):
    """list of (xs, diff) per frame -> (offsets, xs, diff)."""
    offs = np.concatenate([[0], np.cumsum([len(x) for x, _ in frames])]).astype(np.uint32)
    xs = np.concatenate([np.asarray(x, np.int32) for x, _ in frames] + [np.empty(0, np.int32)])
    df = np.concatenate([np.asarray(d, np.uint8) for _, d in frames] + [np.empty(0, np.uint8)])
    return offs, xs, df


def host_apply(state, buf, nframes):
    st = state.copy()
    used = cwire_apply_host(st, buf, nframes)
    return st, used


def oracle_apply(po, state, offs, xs, df):
    st = state.copy()
    for t in range(offs.size - 1):
        st = po.client_apply(st, xs[offs[t]:offs[t + 1]], df[offs[t]:offs[t + 1]])
    return st


def boundary_frames(N, rng):
    """Frames at every boundary of the code: gaps 0, 254, 255, 256, xs[0] >= 255, n % 4 in {0,1,2,3}, n = 0, n = N."""
    F = []
    for n in range(1, 9):                                              # n % 4 = 0..3, gaps 0 (consecutive bytes)
        F.append(np.arange(n) + 3)
    F.append(np.array([], np.int64))                                  # n = 0
    F.append(np.arange(N))                                             # n = N
    F.append(np.array([0, 255, 511, 768, 1024]))                 # gaps 0, 254, 255, 256, 255
    F.append(np.array([254]))                                          # g_0 = 254: a code
    F.append(np.array([255, 256]))                                     # g_0 = 255: an escape
    F.append(np.array([256, 512, 1000, 1001, 1003]))                   # g_0 >= 255
    F.append(np.array([N - 1]))                                        # the last byte alone
    F.append(np.sort(rng.choice(N, 97, replace=False)))
    return [(x.astype(np.int32), rng.integers(1, 256, x.size).astype(np.uint8)) for x in F]


def test_spec_round_trip_and_boundaries():
    rng = np.random.default_rng(1)
    N = 3 * 40 * 30
    offs, xs, df = frames_stream(boundary_frames(N, rng))
    buf, pos = spec.encode(offs, xs, df)
    assert buf.size == int(pos[-1]) and buf.size % 4 == 0
    o2, x2, d2 = spec.decode(buf, offs.size - 1)
    assert np.array_equal(o2, offs) and np.array_equal(x2, xs) and np.array_equal(d2, df)
    # the escape rows byte for byte: gaps 0, 254, 255, 256, 255 -> codes 0, 254, 255, 255, 255 + escapes 255, 256, 255
    r = spec.encode_frame(np.array([0, 255, 511, 768, 1024]), np.arange(1, 6, dtype=np.uint8))
    want = (np.array([5, 3], "<u4").tobytes() + bytes([0, 254, 255, 255, 255, 0, 0, 0]) + np.array([255, 256, 255], "<u4").tobytes()
            + bytes([1, 2, 3, 4, 5, 0, 0, 0]))
    assert r == want
    assert spec.encode_frame(np.array([255]), np.array([9], np.uint8)) == (np.array([1, 1], "<u4").tobytes() + bytes([255, 0, 0, 0])
                                                                           + np.array([255], "<u4").tobytes() + bytes([9, 0, 0, 0]))
    assert spec.encode_frame(np.array([], np.int32), np.array([], np.uint8)) == bytes(8)


def test_host_client_equals_oracle_client_on_boundaries(po):
    rng = np.random.default_rng(2)
    N = 3 * 40 * 30
    frames = boundary_frames(N, rng)
    offs, xs, df = frames_stream(frames)
    buf, pos = spec.encode(offs, xs, df)
    base = rng.integers(0, 256, N).astype(np.uint8)
    st, used = host_apply(base, buf, offs.size - 1)
    assert used == buf.size
    assert np.array_equal(st, oracle_apply(po, base, offs, xs, df))


def test_host_client_4k_sized_gaps(po):
    """4K frames (N = 24 883 200): gaps up to N - 1 travel in the escapes (32 bits) unharmed."""
    N = 3 * 3840 * 2160
    xs = np.array([0, 1, 300, 70000, 5_000_000, 24_000_000, N - 2, N - 1], np.int32)
    df = np.arange(1, xs.size + 1, dtype=np.uint8)
    offs = np.array([0, xs.size, xs.size + 1], np.uint32)
    xs = np.append(xs, np.int32(N - 1)); df = np.append(df, np.uint8(200))   # frame 1: one entry with g_0 = N - 1
    buf, _ = spec.encode(offs, xs, df)
    n_, e_ = spec.headers(buf, 2)
    assert list(n_) == [8, 1] and list(e_) == [5, 1]
    base = np.zeros(N, np.uint8)
    st, used = host_apply(base, buf, 2)
    assert used == buf.size
    assert np.array_equal(st, oracle_apply(po, base, offs, xs, df))


def test_oracle_stream_f1f2_reconstructs_and_counts(po):
    g = golden("ref_f1f2_1080p.npz")
    f1, f2 = g["f1"].reshape(-1), g["f2"].reshape(-1)
    c, xs, df, st = po.diff_pack(f2, f1)
    assert c == 369350
    offs = np.array([0, c], np.uint32)
    buf, pos = spec.encode(offs, xs, df)
    assert buf.size == 754264                                  # the issue's table: 2.45x below 1 846 754 wire bytes
    assert po.wire_pack(offs, xs, df).size == 1846754
    assert int(spec.headers(buf, 1)[1][0]) == 3888            # gaps >= 255
    got, used = host_apply(f1, buf, 1)
    assert used == buf.size and np.array_equal(got, st)


def test_oracle_stream_s1_64x48_reconstructs(po):
    w, h, T = 64, 48, 9
    base, frames = synth.webcam_stream(T, w, h, seed=7)
    offs, xs, df, st = po.diff_stream(frames, base)
    buf, pos = spec.encode(offs, xs, df)
    got, used = host_apply(base, buf, T)
    assert used == buf.size == int(pos[-1])
    assert np.array_equal(got, st)
    o2, x2, d2 = spec.decode(buf, T)
    assert np.array_equal(o2, offs) and np.array_equal(x2, xs) and np.array_equal(d2, df)


def test_empty_frame_is_8_bytes():
    assert cwire_frame_bytes(0, 0) == 8
    buf, pos = spec.encode(np.array([0, 0], np.uint32), np.empty(0, np.int32), np.empty(0, np.uint8))
    assert buf.size == 8 and list(pos) == [0, 8]
    st = np.arange(12, dtype=np.uint8)
    got, used = host_apply(st, buf, 1)
    assert used == 8 and np.array_equal(got, st)


@pytest.mark.parametrize("n,e", [(0, 0), (1, 0), (2, 1), (3, 0), (4, 4), (5, 2), (369350, 3888), (6220800, 0)])
def test_frame_bytes_arithmetic(n, e):
    assert cwire_frame_bytes(n, e) == spec.frame_bytes(n, e) == 8 + 2 * ((n + 3) // 4 * 4) + 4 * e


@pytest.mark.parametrize("N,T", [(0, 3), (1, 1), (6, 2), (6220800, 256), (24883200, 64), (7, 0)])
def test_bytes_max_arithmetic(N, T):
    assert cwire_bytes_max(N, T) == T * (8 + 2 * ((N + 3) // 4 * 4))
    # the worst case is the full frame: every other record of such a frame is shorter
    if 0 < N < 100000:
        assert spec.frame_bytes(N, 0) == cwire_bytes_max(N, 1)


def test_bytes_max_bounds_the_worst_escape_frames():
    N = 3 * 64 * 48
    xs = np.arange(255, N, 256)                                # every gap escapes: e = n
    assert spec.frame_bytes(xs.size, xs.size) <= cwire_bytes_max(N, 1)


# ---- malformed input: every refusal, with the bytes of the frames applied before it ---------------------------------
def two_good_frames():
    N = 3 * 8 * 8
    offs = np.array([0, 3, 5], np.uint32)
    xs = np.array([1, 2, 170, 4, 150], np.int32)
    df = np.array([1, 2, 3, 4, 5], np.uint8)
    buf, pos = spec.encode(offs, xs, df)
    return N, bytearray(buf.tobytes()), [int(p) for p in pos]


def refused(state, buf, nframes, what):
    st = state.copy()
    with pytest.raises(lib.Mi355Error) as ei:
        cwire_apply_host(st, bytes(buf), nframes)
    assert ei.value.code == lib.ERR_INVALID
    assert what in str(ei.value), str(ei.value)
    return st, ei.value.consumed


def test_malformed_truncated_record():
    N, buf, pos = two_good_frames()
    st0 = np.zeros(N, np.uint8)
    want, _ = host_apply(st0, bytes(buf[:pos[1]]), 1)
    st, used = refused(st0, buf[:-1], 2, "truncated")             # the second record misses a byte
    assert used == pos[1] and np.array_equal(st, want)
    st, used = refused(st0, buf[:pos[1] + 5], 2, "truncated")     # a header cut in two
    assert used == pos[1] and np.array_equal(st, want)
    st, used = refused(st0, buf, 3, "truncated")                 # a third frame that is not there
    assert used == pos[2]


def test_malformed_n_larger_than_the_frame():
    N, buf, pos = two_good_frames()
    rec = np.array([N + 1, 0], "<u4").tobytes()
    st, used = refused(np.zeros(N, np.uint8), buf + rec, 3, "frame bytes")
    assert used == pos[2]


def test_malformed_more_escapes_than_entries():
    N, buf, pos = two_good_frames()
    rec = np.array([1, 2], "<u4").tobytes() + bytes([255, 0, 0, 0]) + np.array([300, 300], "<u4").tobytes() + bytes(4)
    st, used = refused(np.zeros(N, np.uint8), buf + rec, 3, "escapes")
    assert used == pos[2]


@pytest.mark.parametrize("codes,e", [([255, 255, 0, 0], 1), ([0, 1, 2, 0], 1)])
def test_malformed_escape_count_differs_from_header(codes, e):
    N, buf, pos = two_good_frames()
    rec = np.array([3, e], "<u4").tobytes() + bytes(codes) + np.array([400] * e, "<u4").tobytes() + bytes(4)
    st, used = refused(np.zeros(N, np.uint8), buf + rec, 3, "escape codes")
    assert used == pos[2]


@pytest.mark.parametrize("codes,esc", [([100, 100, 0, 0], []), ([255, 0, 0, 0], [10 ** 9]), ([254, 0, 0, 0], [])])
def test_malformed_index_past_the_frame(codes, esc):
    N, buf, pos = two_good_frames()          # N = 192: 100 + 1 + 100 > N; 10^9; a single gap 254 > N
    n = 2 if codes[1] else 1
    rec = np.array([n, len(esc)], "<u4").tobytes() + bytes(codes) + np.array(esc, "<u4").tobytes() + bytes([7, 7, 0, 0])
    st0 = np.zeros(N, np.uint8)
    want, _ = host_apply(st0, bytes(buf), 2)
    st, used = refused(st0, buf + rec, 3, "index")
    assert used == pos[2] and np.array_equal(st, want)       # the bad frame changed nothing


def test_malformed_nulls_and_negative_nframes():
    L = lib.load()
    st = np.zeros(16, np.uint8)
    buf = np.zeros(8, np.uint8)
    used = C.c_size_t(99)
    assert L.mi355_cwire_apply_host(None, 16, buf.ctypes.data, 8, 1, C.byref(used)) == lib.ERR_INVALID and used.value == 0
    assert L.mi355_cwire_apply_host(st.ctypes.data, 16, None, 8, 1, C.byref(used)) == lib.ERR_INVALID
    assert L.mi355_cwire_apply_host(st.ctypes.data, 16, buf.ctypes.data, 8, 1, None) == lib.ERR_INVALID
    assert L.mi355_cwire_apply_host(st.ctypes.data, 16, buf.ctypes.data, 8, -1, C.byref(used)) == lib.ERR_INVALID
    assert b"nframes" in L.mi355_last_error()
    assert L.mi355_cwire_apply_host(st.ctypes.data, 16, buf.ctypes.data, 8, 0, C.byref(used)) == lib.OK and used.value == 0


def test_device_entry_points_validate_without_gpu():
    L = lib.load()
    fp = np.zeros(2, np.uint64)
    assert L.mi355_cwire_encode_batch(None, 16, 16, 16, 0, 1, fp.ctypes.data, 16, 0) == lib.ERR_INVALID
    cnt = np.zeros(1, np.uint32)
    assert L.mi355_cwire_decode_batch(None, 16, cnt.ctypes.data, cnt.ctypes.data, 1, 16, 16, 16, 0) == lib.ERR_INVALID

"""CPU: mi355_cwire_despeckle_host, the definition of the despeckle call, against the numpy statement of its semantics
(tests/despeckle_spec.py): every shape of the list at every need, mixed needs across streams, hand-made neighbourhoods, the
capacity rule, the stride gap and every refusal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cwire_spec as spec
import despeckle_spec as ds
from cudavideostream_amd import cwire_bytes_max, cwire_despeckle_host, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5C


@pytest.fixture(scope="module")
def built():
    lib.build()
    return lib.load()


def host(w, h, recs, counts, escapes, post, need, stride=None, capacity=None):
    """-> (dropped, offsets, frame_pos, out, states [S, n]); the stride gaps hold FILL before and are asserted after."""
    S, n = len(need), 3 * w * h
    stride = n if stride is None else stride
    buf = np.full(max(S, 1) * stride, FILL, np.uint8)
    rows = buf[:S * stride].reshape(S, stride)
    rows[:, :n] = post
    dropped, off, pos, out = cwire_despeckle_host(w, h, recs, counts, escapes, buf, need, stride=stride, capacity_bytes=capacity)
    assert (rows[:, n:] == FILL).all(), "the stride gap was written"
    return dropped, off, pos, out, rows[:, :n].copy()


def check(w, h, recs, counts, escapes, post, need, **kw):
    want = ds.despeckle(w, h, recs, post, need)
    got = host(w, h, recs, counts, escapes, post, need, **kw)
    what = (w, h, list(need), kw)
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[3][:want[3].size], want[3]) and not got[3][want[3].size:].any(), what
    assert np.array_equal(got[4], want[4]), what
    return want


def covered(want, s=0):
    """(entries kept, entries dropped) of stream s, from the spec."""
    return int(want[5][s].sum()), int(want[0][s])


# ---- 1. every shape at every need -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need", range(9))
@pytest.mark.parametrize("shape", ds.SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_form_against_the_spec(built, shape, need):
    w, h = shape
    pre, frames, recs, counts, escapes, post = ds.tick(w, h, ds.density_for(need))
    want = check(w, h, recs, counts, escapes, post, [need])
    kept, gone = covered(want)
    if need == 0:                                       # passes through byte for byte, the state as it was
        assert gone == 0 and np.array_equal(want[3], recs) and np.array_equal(want[4], post)
    elif ds.degenerate(w, h, need):                     # need >= 3 at width 1 or height 1, need >= 6 at width 2
        assert kept == 0 and gone == int(counts[0]) > 0
        assert np.array_equal(want[4][0], pre[0]), "everything dropped: the state before the tick"
    else:
        assert kept > 0 and gone > 0, (shape, need, kept, gone)


@pytest.mark.parametrize("density", ds.DENSITIES)
@pytest.mark.parametrize("shape", ds.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_density(built, shape, density):
    """The three densities at every need.  The cover condition holds where the numpy statement says it can: density 0.3 at
    need 1..5 and density 0.7 at need 3..8 of the 2-D shapes; the sparse input keeps the solid block and drops the salt at
    need 1 and 2 there."""
    w, h = shape
    pre, frames, recs, counts, escapes, post = ds.tick(w, h, density)
    for need in range(1, 9):
        want = check(w, h, recs, counts, escapes, post, [need])
        kept, gone = covered(want)
        must = (density == 0.3 and need <= 5) or (density == 0.7 and need >= 3) or (density == 0.05 and need <= 2)
        if must and min(w, h) > 2:                      # (1x64, 2x40 and 64x1 are compared all the same)
            assert kept > 0 and gone > 0, (shape, density, need, kept, gone)


def test_tile_and_row_seams_are_in_the_inputs():
    """64x48 has a pixel split by the byte-4096 tile boundary with entries on both sides; 1400x3 has a row longer than a tile."""
    _, _, recs, counts, _, _ = ds.tick(64, 48, 0.7)
    _, xs, _ = spec.decode(recs, 1)
    assert 4096 // 3 == 4097 // 3 == 1365 and 4095 in xs and (4096 in xs or 4097 in xs)
    assert 3 * 1400 > 4096


@pytest.mark.parametrize("shape", [(37, 11), (64, 48), (2, 40)], ids=lambda s: "%dx%d" % s)
def test_mixed_need_across_five_streams(built, shape):
    """Needs from the range each density covers (0.3: 1..5, 0.7: 3..8), a pass-through stream among them."""
    w, h = shape
    n = 3 * w * h
    for density, needs in ((0.7, ([3, 0, 8, 5, 4], [0, 0, 4, 0, 6], [8, 7, 6, 5, 4])), (0.3, ([1, 2, 0, 5, 3], [2, 0, 0, 1, 0]))):
        pre, frames, recs, counts, escapes, post = ds.tick(w, h, density, 5)
        for need in needs:
            want = check(w, h, recs, counts, escapes, post, need)
            for s, nd in enumerate(need):
                kept, gone = covered(want, s)
                if nd == 0:
                    assert gone == 0 and np.array_equal(want[4][s], post[s])
                elif min(w, h) > 2:                     # (2x40 is compared all the same)
                    assert kept > 0 and gone > 0, (shape, density, need, s)
        check(w, h, recs, counts, escapes, post, needs[0], stride=n + 7)


# ---- 2. hand-made neighbourhoods --------------------------------------------------------------------------------------------
def record_of(w, h, entries):
    """entries: {byte index: diff byte} -> (record, counts, escapes, state after the tick: 100 everywhere, + diff at the entries)"""
    xs = np.array(sorted(entries), np.int64)
    df = np.array([entries[int(x)] for x in xs], np.uint8)
    rec = np.frombuffer(spec.encode_frame(xs, df), np.uint8)
    counts, escapes = spec.headers(rec, 1)
    post = np.full((1, 3 * w * h), 100, np.uint8)
    post[0][xs] += df
    return rec, counts, escapes, post


def kept_pixels(w, h, entries, need):
    rec, counts, escapes, post = record_of(w, h, entries)
    want = check(w, h, rec, counts, escapes, post, [need])
    _, xs, _ = spec.decode(want[3], 1)
    assert np.array_equal(want[4][0][list(entries)] == 100, ~np.isin(list(entries), xs)), "dropped entries are reverted"
    return sorted(set(int(x) // 3 for x in xs))


def test_the_pixel_split_by_the_tile_boundary(built):
    """64x48: pixel 1365 holds bytes 4095 (first tile) and 4096, 4097 (second tile).  One changed channel on either side makes
    the pixel changed: its neighbour is kept by it, and it by its neighbour."""
    w, h = 64, 48
    for byte in (4095, 4096, 4097):
        assert byte // 3 == 1365
        assert kept_pixels(w, h, {byte: 50, 3 * 1366 + 1: 60}, 1) == [1365, 1366]
        assert kept_pixels(w, h, {byte: 50, 3 * 1364: 60}, 1) == [1364, 1365]
        assert kept_pixels(w, h, {byte: 50, 3 * (1365 - w) + 2: 60}, 1) == [1365 - w, 1365]
        assert kept_pixels(w, h, {byte: 50}, 1) == []
    # both sides changed: still ONE pixel, which does not count for itself
    assert kept_pixels(w, h, {4095: 50, 4096: 51, 4097: 52}, 1) == []
    assert kept_pixels(w, h, {4095: 50, 4097: 52, 3 * 1366: 9}, 2) == []


def test_a_neighbour_across_a_row_end_does_not_count(built):
    w, h = 37, 11
    last, first = 3 * (w - 1), 3 * w                            # pixel (36, 0) and pixel (0, 1): consecutive indices
    assert kept_pixels(w, h, {last: 50, first: 50}, 1) == []
    assert kept_pixels(w, h, {last: 50, first + 3 * w: 50}, 1) == []             # (36, 0) and (0, 2): index distance width + 1
    assert kept_pixels(w, h, {3 * (2 * w - 1): 50, 3 * (2 * w) + 1: 50}, 1) == []  # (36, 1) and (0, 2)
    assert kept_pixels(w, h, {3 * (w - 1): 50, 3 * (w + w - 2): 50}, 1) == [w - 1, 2 * w - 2]   # (36, 0) and (35, 1): diagonal


def test_frame_corners(built):
    w, h = 37, 11
    for corner, (dx, dy) in (((0, 0), (1, 1)), ((w - 1, 0), (-1, 1)), ((0, h - 1), (1, -1)), ((w - 1, h - 1), (-1, -1))):
        cx, cy = corner
        three = [(cx + dx, cy), (cx, cy + dy), (cx + dx, cy + dy)]
        ent = {3 * (cy * w + cx): 40}
        ent.update({3 * (y * w + x) + 2: 41 for x, y in three})
        assert cy * w + cx in kept_pixels(w, h, ent, 3)          # all four form a 2x2 block: 3 neighbours each
        assert kept_pixels(w, h, ent, 4) == []


@pytest.mark.parametrize("shape", [(37, 11), (33, 9), (5, 4)], ids=lambda s: "%dx%d" % s)
def test_a_full_frame(built, shape):
    """Every byte changed: nothing is dropped at need 1..3 (a corner has 3 neighbours), byte for byte; need 4, 5 drops the
    corners, need 6..8 drops the whole border."""
    w, h = shape
    n = 3 * w * h
    ent = {x: 1 + x % 255 for x in range(n)}
    rec, counts, escapes, post = record_of(w, h, ent)
    for need in (1, 2, 3):
        want = check(w, h, rec, counts, escapes, post, [need])
        assert np.array_equal(want[3], rec) and np.array_equal(want[4], post) and want[0][0] == 0
    corners = {0, w - 1, (h - 1) * w, h * w - 1}
    inner = {y * w + x for y in range(1, h - 1) for x in range(1, w - 1)}
    for need in (4, 5):
        assert kept_pixels(w, h, ent, need) == sorted(set(range(w * h)) - corners)
    for need in (6, 7, 8):
        assert kept_pixels(w, h, ent, need) == sorted(inner)


def test_a_zero_diff_byte_is_no_entry(built):
    """A record another producer made may hold one: it marks nothing, is not written and is not counted as dropped."""
    w, h = 37, 11
    xs, df = np.array([30, 33, 300]), np.array([0, 50, 0], np.uint8)
    rec = np.frombuffer(spec.encode_frame(xs, df), np.uint8)
    post = np.full((1, 3 * w * h), 100, np.uint8)
    d, off, pos, out, st = host(w, h, rec, [3], [1], post, [1])
    assert d[0] == 1 and off[1] == 0 and int(pos[1]) == 8 and st[0][33] == 50 and (np.delete(st[0], 33) == 100).all()
    d, off, pos, out, st = host(w, h, rec, [3], [1], post, [0])
    assert d[0] == 0 and off[1] == 1 and np.array_equal(out[:int(pos[1])], np.frombuffer(spec.encode_frame([33], [50]), np.uint8))


# ---- 3. capacity, stride ----------------------------------------------------------------------------------------------------
def test_capacity_rule(built):
    w, h, S = 64, 48, 3
    pre, frames, recs, counts, escapes, post = ds.tick(w, h, 0.7, 5)
    recs, counts, escapes, post = recs[:int(sum(spec.frame_bytes(n, e) for n, e in zip(counts[:S], escapes[:S])))], counts[:S], escapes[:S], post[:S]
    need = [3, 5, 2]
    want = ds.despeckle(w, h, recs, post, need)
    full = int(want[2][S])
    assert cwire_bytes_max(3 * w * h, S) >= full
    for cap in (full, full - 1, int(want[2][2]) - 1, int(want[2][1]), 0):
        d, off, pos, out, st = host(w, h, recs, counts, escapes, post, need, capacity=cap)
        assert out.size == max(cap, 0)
        assert np.array_equal(d, want[0]) and np.array_equal(off, want[1]) and np.array_equal(pos, want[2]), cap
        assert np.array_equal(st, want[4]), (cap, "the states are reverted whatever fits")
        for s in range(S):
            a, b = int(want[2][s]), int(want[2][s + 1])
            if b <= cap:
                assert np.array_equal(out[a:b], want[3][a:b]), (cap, s)
            else:
                assert not out[min(a, cap):min(b, cap)].any(), (cap, s, "a record that does not fit is skipped whole")


def test_stride_gap_untouched(built):
    w, h = 37, 11
    n = 3 * w * h
    pre, frames, recs, counts, escapes, post = ds.tick(w, h, 0.7, 5)
    for stride in (n, n + 1, n + 11, 2 * n):
        check(w, h, recs, counts, escapes, post, [3, 8, 1, 0, 5], stride=stride)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(built):
    L = built
    w, h, S = 37, 11, 2
    n = 3 * w * h
    pre, frames, recs, counts, escapes, post = ds.tick(w, h, 0.7, 5)
    counts, escapes = counts[:S].copy(), escapes[:S].copy()
    span = int(sum(spec.frame_bytes(a, b) for a, b in zip(counts, escapes)))
    recs = recs[:span].copy()
    states = np.ascontiguousarray(post[:S]).copy()
    need = np.array([3, 2], np.uint32)
    cap = cwire_bytes_max(n, S)
    dropped, off, pos, out = (np.full(S, 77, np.uint32), np.full(S + 1, 77, np.uint32), np.full(S + 1, 77, np.uint64),
                              np.full(cap, FILL, np.uint8))
    p = lambda a: None if a is None else a.ctypes.data

    def call(**kw):
        d = dict(width=w, height=h, cwire=p(recs), cwire_bytes=recs.size, counts=p(counts), escapes=p(escapes), states=p(states),
                 stride=n, S=S, need=p(need), dropped=p(dropped), off=p(off), pos=p(pos), out=p(out), cap=cap)
        d.update(kw)
        return L.mi355_cwire_despeckle_host(*d.values())

    def damaged(at, value):
        bad = recs.copy()
        bad[at] = value
        return bad

    big_n = counts.copy(); big_n[1] = n + 1
    more_e = escapes.copy(); more_e[1] = counts[1] + 1
    less_e = escapes.copy(); less_e[0] = escapes[0] + 1          # one escape more than 255 codes: the record grows, too
    nine = need.copy(); nine[1] = 9
    code0 = 8
    keep = []                                                    # (arrays handed by address stay alive)
    past = damaged(code0, 254)                                   # the first gap 254: every index moves up ...
    past[code0:code0 + int(counts[0])] = 254                     # ... all gaps 254: the running index leaves the frame
    a255 = damaged(code0 + 1, 255)                               # one more 255 code than e
    keep += [past, a255]
    reasons = [
        (dict(S=-1), "nstreams"), (dict(width=0), "width"), (dict(height=0), "height"), (dict(width=-3), "width"),
        (dict(stride=n - 1), "stride"),
        (dict(cwire=None), "null"), (dict(counts=None), "null"), (dict(escapes=None), "null"), (dict(states=None), "null"),
        (dict(need=None), "null"), (dict(dropped=None), "null"), (dict(off=None), "null"), (dict(pos=None), "null"),
        (dict(out=None), "null"),
        (dict(need=p(nine)), "need"), (dict(counts=p(big_n)), "entries"), (dict(escapes=p(more_e)), "escapes"),
        (dict(cwire_bytes=span - 4), "truncated"), (dict(cwire_bytes=7), "truncated"),
        (dict(escapes=p(less_e)), ""), (dict(cwire=p(a255)), "escape codes"), (dict(cwire=p(past)), "index"),
    ]
    for kw, why in reasons:
        assert call(**kw) == lib.ERR_INVALID, kw
        assert why.encode() in L.mi355_last_error(), (kw, L.mi355_last_error())
    assert (dropped == 77).all() and (off == 77).all() and (pos == 77).all() and (out == FILL).all()
    assert np.array_equal(states, post[:S]), "a refusal reverted a state"
    # nstreams == 0 writes the two heads and nothing else, whatever the other pointers are
    assert call(S=0, cwire=None, counts=None, escapes=None, states=None, need=None, dropped=None, out=None) == lib.OK
    assert off[0] == 0 and pos[0] == 0 and (off[1:] == 77).all() and (pos[1:] == 77).all()
    # ... and the arguments as they stand are good
    assert call() == lib.OK
    want = ds.despeckle(w, h, recs, post[:S], need)
    assert np.array_equal(dropped, want[0]) and np.array_equal(pos, want[2]) and np.array_equal(states, want[4])


def test_stand_alone_host_program(built, tmp_path):
    """tests/host/cwire_despeckle_host.cpp: the host form from C++ against a plain count, with its own main."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "cwire_despeckle_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "host", "cwire_despeckle_host.cpp"),
                    "-I", os.path.join(ROOT, "include"), lib.LIB_PATH, "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH)], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "ok" in done.stdout

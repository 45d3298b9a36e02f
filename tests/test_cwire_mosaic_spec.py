"""The laws of mi355_cwire_mosaic_* on its numpy statement (mosaic_spec), against crop_spec and the library's host client
mi355_cwire_apply_host: (a) applying the canvas record changes exactly the covered bytes, each destination as the crop law says;
(b) the crop of the output to a destination is the crop of that stream's input to its source; (c) one full-frame stream is the
coalescer's record and one rectangle at the origin of its own canvas the crop call's; (d) bands stacked vertically are the bands'
records concatenated with index bias s*N.  No GPU."""
import numpy as np
import pytest

import crop_spec
import cwire_spec as spec
import mosaic_spec
from cudavideostream_amd import cwire_apply_host

SHAPES = [(33, 7), (21, 70), (64, 48), (100, 31), (1400, 3)]


def random_records(rng, n, S, T):
    segs = []
    for b in range(S * T):
        cnt = int(rng.integers(0, min(n, 300)))
        segs.append((np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)))
    return spec.encode(*crop_spec.packed(segs))[0]


def grid_2x2(w, h):
    """Four cameras with different source rectangles in a (2w + 1) x (2h + 1) canvas: disjoint, a margin uncovered."""
    cw, ch = 2 * w + 1, 2 * h + 1
    place = [(0, 0, w, h, 0, 0), (w // 4, 0, max(w // 2, 1), h, w + 1, 0), (0, h // 3, w, max(h // 3, 1), 0, h + 1),
             (w - 1, h - 1, 1, 1, 2 * w, 2 * h)]
    return place, cw, ch


@pytest.mark.parametrize("w,h", SHAPES)
def test_laws_a_and_b(w, h):
    n, S, T = 3 * w * h, 4, 3
    rng = np.random.default_rng(w * 1000 + h)
    recs = random_records(rng, n, S, T)
    counts, escapes = spec.headers(recs, S * T)
    pos = np.cumsum([0] + [spec.frame_bytes(a, b) for a, b in zip(counts, escapes)])
    place, cw, ch = grid_2x2(w, h)
    off, xs, df, rec, fp = mosaic_spec.reference(recs, S, T, w, h, place, cw, ch)
    assert list(fp) == [0, rec.size] and list(off) == [0, xs.size]
    # (a) the canvas state after the record = the canvas state with every destination replaced by the stream's new source
    states = rng.integers(0, 256, (S, n), dtype=np.uint8)
    K = rng.integers(0, 256, 3 * cw * ch, dtype=np.uint8)
    for s in range(S):
        mosaic_spec.place_state(K, cw, ch, states[s], w, h, place[s])
    want = K.copy()
    for s in range(S):
        sl = recs[int(pos[s * T]):int(pos[(s + 1) * T])]
        assert cwire_apply_host(states[s], sl, T) == sl.size
        mosaic_spec.place_state(want, cw, ch, states[s], w, h, place[s])
    assert cwire_apply_host(K, rec, 1) == rec.size
    assert np.array_equal(K, want)
    # (b) crop(output, destination) == crop(stream s's input, source), byte for byte
    for s in range(S):
        sx, sy, rw, rh, dx, dy = place[s]
        back = crop_spec.reference(rec, 1, 1, cw, ch, [(dx, dy, rw, rh)])
        sl = recs[int(pos[s * T]):int(pos[(s + 1) * T])]
        src = crop_spec.reference(sl, 1, T, w, h, [(sx, sy, rw, rh)])
        assert np.array_equal(back[3], src[3]), s


def test_law_c_special_cases():
    w, h, T = 64, 48, 3
    recs = random_records(np.random.default_rng(3), 3 * w * h, 1, T)
    full = mosaic_spec.reference(recs, 1, T, w, h, [(0, 0, w, h, 0, 0)], w, h)
    assert np.array_equal(full[3], crop_spec.reference(recs, 1, T, w, h, [(0, 0, w, h)])[3])   # the coalescer's record
    rect = (5, 7, 20, 30)
    part = mosaic_spec.reference(recs, 1, T, w, h, [rect + (0, 0)], 20, 30)
    assert np.array_equal(part[3], crop_spec.reference(recs, 1, T, w, h, [rect])[3])


def test_law_d_bands():
    w, h, S, T = 33, 7, 3, 2
    n = 3 * w * h
    recs = random_records(np.random.default_rng(4), n, S, T)
    out = mosaic_spec.reference(recs, S, T, w, h, [(0, 0, w, h, 0, s * h) for s in range(S)], w, S * h)
    acc = crop_spec.sums(recs, S, T, n)
    xs = np.concatenate([np.flatnonzero(acc[s]) + s * n for s in range(S)])
    assert np.array_equal(out[1], xs.astype(np.int32))
    assert np.array_equal(out[2], np.concatenate([acc[s][np.flatnonzero(acc[s])] for s in range(S)]))


def test_overlapping_negated_streams_give_the_eight_byte_record():
    w, h = 33, 7
    n = 3 * w * h
    rng = np.random.default_rng(5)
    xs = np.sort(rng.choice(n, 200, replace=False))
    d = rng.integers(1, 256, 200).astype(np.uint8)
    recs = spec.encode(*crop_spec.packed([(xs, d), (xs, (256 - d.astype(np.int64)).astype(np.uint8))]))[0]
    out = mosaic_spec.reference(recs, 2, 1, w, h, [(0, 0, w, h, 3, 2)] * 2, w + 5, h + 4)
    assert out[3].size == 8 and not out[3].any() and list(out[4]) == [0, 8]

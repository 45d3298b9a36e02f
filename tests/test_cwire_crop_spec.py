"""The law of mi355_cwire_crop_* on its numpy statement (crop_spec), through the library's host client mi355_cwire_apply_host:
applying cropped record s to the crop of any state equals the crop of applying the stream's records to the state; with
KEEP_INDEX, applying it to the state changes exactly the rectangle, in the same way.  No GPU."""
import numpy as np
import pytest

import crop_spec
import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host

SHAPES = [(33, 7), (21, 70), (64, 48), (100, 31), (1400, 3)]


def random_records(rng, n, S, T):
    segs = []
    for b in range(S * T):
        cnt = int(rng.integers(0, min(n, 300)))
        segs.append((np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)))
    return spec.encode(*crop_spec.packed(segs))[0]


def rectangles(w, h):
    return [(0, 0, w, h), (w // 4, h // 3, max(w // 2, 1), max(h // 3, 1)), (w - 1, h - 1, 1, 1)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_law(w, h):
    n, S, T = 3 * w * h, 2, 3
    rng = np.random.default_rng(w * 1000 + h)
    recs = random_records(rng, n, S, T)
    counts, escapes = spec.headers(recs, S * T)
    pos = np.cumsum([0] + [spec.frame_bytes(a, b) for a, b in zip(counts, escapes)])
    for rect in rectangles(w, h):
        rects = [rect] * S
        small = crop_spec.reference(recs, S, T, w, h, rects)
        keep = crop_spec.reference(recs, S, T, w, h, rects, keep_index=True)
        assert np.array_equal(small[0], keep[0]) and np.array_equal(small[2], keep[2])
        for s in range(S):
            A = rng.integers(0, 256, n, dtype=np.uint8)
            full = A.copy()
            sl = recs[int(pos[s * T]):int(pos[(s + 1) * T])]
            assert cwire_apply_host(full, sl, T) == sl.size
            want = crop_spec.crop_state(full, w, h, rect)
            got = crop_spec.crop_state(A, w, h, rect)
            rec = small[3][int(small[4][s]):int(small[4][s + 1])]
            assert cwire_apply_host(got, rec, 1) == rec.size
            assert np.array_equal(got, want), (rect, s)
            # KEEP_INDEX: the rectangle of the full state as above, every other byte as it was
            kept = A.copy()
            rec = keep[3][int(keep[4][s]):int(keep[4][s + 1])]
            assert cwire_apply_host(kept, rec, 1) == rec.size
            x0, y0, rw, rh = rect
            expect = A.copy().reshape(h, 3 * w)
            expect[y0:y0 + rh, 3 * x0:3 * (x0 + rw)] = full.reshape(h, 3 * w)[y0:y0 + rh, 3 * x0:3 * (x0 + rw)]
            assert np.array_equal(kept, expect.reshape(-1)), (rect, s)


def test_full_frame_of_one_record_is_the_record():
    w, h = 64, 48
    recs = random_records(np.random.default_rng(1), 3 * w * h, 3, 1)
    out = crop_spec.reference(recs, 3, 1, w, h, [(0, 0, w, h)] * 3)
    assert np.array_equal(out[3], recs)


def test_empty_rectangles_give_eight_byte_records():
    w, h = 33, 7
    recs = random_records(np.random.default_rng(2), 3 * w * h, 2, 2)
    out = crop_spec.reference(recs, 2, 2, w, h, [(5, 2, 0, 3), (5, 2, 4, 0)])
    assert list(out[4]) == [0, 8, 16] and not out[3].any()

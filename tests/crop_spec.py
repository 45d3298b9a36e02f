"""mi355_cwire_crop_batch / _cwire_batch (include/mi355diff.h, "A camera cropped") stated in numpy: the tests' reference.  Test
infrastructure only; the product never imports it.

Decode every input record with cwire_spec, sum the differences per stream in uint8, view the N sums as H rows of 3W bytes, keep
the rectangle's slice, take its nonzero bytes in ascending order -- with the byte index of the rectangle's own w x h frame, or
with the full frame's under KEEP_INDEX -- and encode with cwire_spec."""
import numpy as np

import cwire_spec as spec


def sums(recs, S, T, n):
    """The uint8 sum of every stream's differences per byte index: [S][n]."""
    off, xs, df = spec.decode(recs, S * T)
    acc = np.zeros((S, n), np.uint8)
    for s in range(S):
        for t in range(T):
            a, b = int(off[s * T + t]), int(off[s * T + t + 1])
            acc[s][xs[a:b]] += df[a:b]          # indices of a record are distinct; uint8 wraps
    return acc


def crop_state(state, w, h, rect):
    """The rectangle (x0, y0, rw, rh) of an N-byte BGR24 frame of w x h pixels, as a frame of 3*rw*rh bytes."""
    x0, y0, rw, rh = (int(v) for v in rect)
    return np.asarray(state, np.uint8).reshape(h, 3 * w)[y0:y0 + rh, 3 * x0:3 * (x0 + rw)].reshape(-1).copy()


def segment(acc, w, h, rect, keep_index=False):
    """One stream's sums [n] -> (xs, diff) of its cropped segment."""
    x0, y0, rw, rh = (int(v) for v in rect)
    if keep_index:
        mask = np.zeros((h, 3 * w), bool)
        mask[y0:y0 + rh, 3 * x0:3 * (x0 + rw)] = True
        kept = np.where(mask.reshape(-1), acc, 0).astype(np.uint8)
    else:
        kept = crop_state(acc, w, h, rect)
    xs = np.flatnonzero(kept)
    return xs, kept[xs]


def packed(segments):
    off = np.cumsum([0] + [len(x) for x, _ in segments]).astype(np.uint32)
    xs = np.concatenate([np.asarray(x, np.int64) for x, _ in segments] + [np.empty(0, np.int64)]).astype(np.int32)
    df = np.concatenate([np.asarray(d, np.uint8) for _, d in segments] + [np.empty(0, np.uint8)]).astype(np.uint8)
    return off, xs, df


def reference(recs, S, T, w, h, rects, keep_index=False):
    """-> (offsets uint32[S + 1], xs, diff, records, frame_pos uint64[S + 1]) of the cropped burst."""
    acc = sums(recs, S, T, 3 * w * h)
    off, xs, df = packed([segment(acc[s], w, h, rects[s], keep_index) for s in range(S)])
    out, pos = spec.encode(off, xs, df)
    return off, xs, df, out, pos

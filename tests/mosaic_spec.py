"""mi355_cwire_mosaic_batch / _cwire_batch (include/mi355diff.h, "Many cameras on one canvas") stated in numpy: the tests'
reference.  Test infrastructure only; the product never imports it.

Decode every input record with cwire_spec, sum the differences per stream in uint8 (crop_spec.sums), view a stream's N sums as H
rows of 3W bytes, add its source rectangle with += (uint8 wraps) into the destination rectangle of a (canvas_h, 3*canvas_w) array
of zeros, take the nonzero bytes of the canvas in ascending order and encode with cwire_spec."""
import numpy as np

import crop_spec
import cwire_spec as spec


def canvas_sums(acc, w, h, place, cw, ch):
    """[S][N] sums of the streams -> the canvas' Nc sums."""
    canvas = np.zeros((ch, 3 * cw), np.uint8)
    for s, p in enumerate(place):
        sx, sy, rw, rh, dx, dy = (int(v) for v in p)
        if rw == 0 or rh == 0:
            continue
        canvas[dy:dy + rh, 3 * dx:3 * (dx + rw)] += np.asarray(acc[s], np.uint8).reshape(h, 3 * w)[sy:sy + rh, 3 * sx:3 * (sx + rw)]
    return canvas.reshape(-1)


def place_state(canvas, cw, ch, state, w, h, p):
    """The source rectangle of an N-byte state copied into its destination of the Nc-byte canvas state (in place)."""
    sx, sy, rw, rh, dx, dy = (int(v) for v in p)
    np.asarray(canvas).reshape(ch, 3 * cw)[dy:dy + rh, 3 * dx:3 * (dx + rw)] = \
        np.asarray(state, np.uint8).reshape(h, 3 * w)[sy:sy + rh, 3 * sx:3 * (sx + rw)]


def reference(recs, S, T, w, h, place, cw, ch):
    """-> (offsets uint32[2], xs, diff, record, frame_pos uint64[2]) of the ONE canvas record."""
    acc = crop_spec.sums(recs, S, T, 3 * w * h)
    c = canvas_sums(acc, w, h, place, cw, ch)
    xs = np.flatnonzero(c)
    off, xs, df = crop_spec.packed([(xs, c[xs])])
    out, pos = spec.encode(off, xs, df)
    return off, xs, df, out, pos

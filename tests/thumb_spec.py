"""The thumbnail records (include/mi355diff.h, "Thumbnail records") stated in numpy, on top of wall_spec.thumbnail,
wall_spec.required and cwire_spec.encode_frame; the shapes and ticks the tests of the call share.  Test infrastructure only,
the product never imports it."""
import numpy as np

import cwire_spec as spec
import wall_spec as ws


def thumb_bytes(w, h, k):
    tw, th = ws.thumb_size(w, h, k)
    return 3 * tw * th


def required_bytes(sel, w, h, k):
    """bool[N']: the bytes of the required pixels (sel: bool[tiles] of the full-size state, or None: every tile)."""
    tw, th = ws.thumb_size(w, h, k)
    req = np.ones((th, tw), bool) if sel is None else ws.required(np.asarray(sel, bool), w, h, k)
    return np.repeat(req.reshape(-1), 3)


def step(state, thumb, w, h, k, threshold, sel=None, processed=None):
    """One stream: -> (record bytes, held thumbnail after, xs, diff bytes).  processed: bool[N'] of the bytes the call looked at,
    a superset of required_bytes(sel); None: exactly the required ones (the host form)."""
    new = ws.thumbnail(state, w, h, k).reshape(-1)
    thumb = np.asarray(thumb, np.uint8)
    assert thumb.size == new.size
    req = required_bytes(sel, w, h, k)
    if processed is None:
        processed = req
    assert not (req & ~processed).any(), "every required pixel is processed"
    df = new.astype(np.int64) - thumb.astype(np.int64)
    xs = np.flatnonzero(processed & (np.abs(df) > threshold))
    diff = (df[xs] & 255).astype(np.uint8)
    after = thumb.copy()
    after[xs] = new[xs]
    return spec.encode_frame(xs.astype(np.int32), diff), after, xs.astype(np.int32), diff


def batch(states, thumbs, w, h, k, threshold, sel=None, processed=None, capacity=None):
    """states uint8[S, N], thumbs uint8[S, N'], sel bool[S, tiles] or None, processed bool[S, N'] or None ->
    (offsets uint32[S + 1], frame_pos uint64[S + 1], records: list of bytes or None where skipped, thumbs after uint8[S, N']).
    A record with frame_pos[s + 1] > capacity is skipped whole and its held thumbnail stays."""
    S = len(states)
    off, pos, recs, after = [0], [0], [], np.array(thumbs, np.uint8, copy=True)
    for s in range(S):
        rec, t, xs, _ = step(states[s], thumbs[s], w, h, k, threshold, None if sel is None else sel[s],
                             None if processed is None else processed[s])
        off.append(off[-1] + xs.size)
        pos.append(pos[-1] + len(rec))
        if capacity is not None and pos[-1] > capacity:
            recs.append(None)
        else:
            recs.append(rec)
            after[s] = t
    return np.array(off, np.uint32), np.array(pos, np.uint64), recs, after


def apply(thumb, rec):
    """The record applied to a copy of the held thumbnail (mod 256)."""
    _, xs, df = spec.decode(np.frombuffer(rec, np.uint8), 1)
    out = np.array(thumb, np.uint8, copy=True)
    out[xs] = out[xs] + df
    return out


def check_law2(state, before, after, w, h, k, threshold, sel):
    """Law 2: a byte of a required pixel is the new value, or kept with a pending difference within the threshold; any other
    byte is untouched or satisfies the same."""
    new = ws.thumbnail(state, w, h, k).reshape(-1).astype(np.int64)
    before, after = np.asarray(before, np.int64), np.asarray(after, np.int64)
    rule = (after == new) | ((np.abs(new - before) <= threshold) & (after == before))
    req = required_bytes(sel, w, h, k)
    assert rule[req].all()
    assert (rule | (after == before))[~req].all()


# (width, height, k): every geometry the tests of the call use, each the smallest at which one mechanism can go wrong
SHAPES = [(37, 11, 1), (37, 11, 2), (37, 11, 3), (37, 11, 4), (37, 11, 16), (64, 48, 16), (100, 60, 2), (100, 60, 3), (2800, 6, 2)]


def random_states(rng, S, w, h):
    return rng.integers(0, 256, (S, 3 * w * h), dtype=np.uint8)


def tie_state(w, h, k):
    """Every block sums to a / 2 in every channel, one pixel of it carrying the whole sum: the rounding tie, mean 1/2 -> 1.
    k even, k dividing w and h."""
    assert k % 2 == 0 and w % k == 0 and h % k == 0
    img = np.zeros((h, w, 3), np.uint8)
    img[::k, ::k] = k * k // 2
    return img.reshape(-1)


def one_tile_masks(n):
    """bool[tiles, tiles]: exactly one source tile selected, each in turn."""
    return np.eye(ws.tiles(n), dtype=bool)


def touched_sel(before, after):
    """bool[tiles]: the source tiles that hold a byte the tick changed."""
    return ws.touched(before.size, [np.flatnonzero(np.asarray(before) != np.asarray(after))])


def mechanics_ticks(rng, w=100, h=60, k=2):
    """[(name, state before, state after)] at 100 x 60, k = 2 (a thumbnail row is 150 bytes): the record mechanics.
    far : source pixels (0, 0) and (0, 40) change -- entries at j = 0 .. 2 and 3000 .. 3002: a gap >= 255, an escape, n = 6 (pads)
    late: source pixel (0, 4) changes -- the first entry lies at j = 300 >= 255
    wrap: a whole block goes from 250 to 3 -- diff byte 9
    same: nothing changes -- the 8-byte record"""
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    far, late, wrap0, wrap1 = base.copy(), base.copy(), base.copy(), base.copy()
    far[0, 0] += 128
    far[40, 0] += 128
    late[4, 0] += 128
    wrap0[0:k, 2 * k:3 * k] = 250
    wrap1[0:k, 2 * k:3 * k] = 3
    flat = lambda a: a.reshape(-1)
    return [("far", flat(base), flat(far)), ("late", flat(base), flat(late)), ("wrap", flat(wrap0), flat(wrap1)),
            ("same", flat(base), flat(base.copy()))]

"""The wall of many cameras (include/mi355diff.h, "A wall of many cameras") stated in numpy: the box-averaged thumbnail, the
composed wall, the required pixels of a masked compose and the touched tiles of a set of entries.  The tests' reference; test
infrastructure only, the product never imports it."""
import numpy as np

TILE = 4096


def tiles(n):
    return (int(n) + TILE - 1) // TILE


def mask_words(n):
    return (tiles(n) + 31) // 32


def thumb_size(w, h, k):
    return (w + k - 1) // k, (h + k - 1) // k


def thumbnail(state, w, h, k):
    """uint8[th, tw, 3] of the uint8[3*w*h] BGR24 state: per block and channel floor((sum + floor(a / 2)) / a), a the block's
    pixels (the blocks at the right and bottom edges are smaller)."""
    img = np.asarray(state, np.uint8).reshape(h, w, 3).astype(np.int64)
    tw, th = thumb_size(w, h, k)
    xe, ye = np.arange(0, w, k), np.arange(0, h, k)
    sums = np.add.reduceat(np.add.reduceat(img, ye, axis=0), xe, axis=1)
    area = (np.minimum(ye + k, h) - ye)[:, None] * (np.minimum(xe + k, w) - xe)[None, :]
    out = (sums + (area // 2)[:, :, None]) // area[:, :, None]
    assert out.shape == (th, tw, 3) and out.max(initial=0) <= 255
    return out.astype(np.uint8)


def rect(w, h, place):
    """(x, y, tw, th) of a shown stream's thumbnail in the wall."""
    x, y, k = (int(v) for v in place)
    tw, th = thumb_size(w, h, k)
    return x, y, tw, th


def compose(wall, states, w, h, places):
    """wall: uint8[wall_h, wall_w, 3], changed in place and returned: every shown stream's thumbnail at its place."""
    for s, p in enumerate(places):
        if int(p[2]) == 0:
            continue
        x, y, tw, th = rect(w, h, p)
        wall[y:y + th, x:x + tw] = thumbnail(states[s], w, h, int(p[2]))
    return wall


def selected_of(mask_row, n):
    """bool[tiles] of one stream's mask words (bits at or past tiles ignored)."""
    t = tiles(n)
    bits = np.unpackbits(np.asarray(mask_row, "<u4").view(np.uint8), bitorder="little")
    return bits[:t].astype(bool)


def required(sel, w, h, k):
    """bool[th, tw]: the thumbnail pixels whose block contains a source pixel p whose bytes [3p, 3p + 3) meet a selected tile
    (sel: bool[tiles]); a pixel that straddles a tile edge belongs to both tiles."""
    p = np.arange(w * h)
    hit = sel[(3 * p) // TILE] | sel[(3 * p + 2) // TILE]
    img = hit.reshape(h, w).astype(np.int64)
    return np.add.reduceat(np.add.reduceat(img, np.arange(0, h, k), axis=0), np.arange(0, w, k), axis=1) > 0


def touched(n, entry_lists):
    """bool[tiles]: the tiles that hold an index of any of the index arrays -- np.unique(x // 4096)."""
    out = np.zeros(tiles(n), bool)
    for xs in entry_lists:
        out[np.unique(np.asarray(xs, np.int64) // TILE)] = True
    return out


def mask_of(sel):
    """bool[S, tiles] -> uint32[S, mask_words]."""
    S, t = sel.shape
    out = np.zeros((S, (t + 31) // 32), np.uint32)
    for s, tl in zip(*np.nonzero(sel)):
        out[s, tl >> 5] |= np.uint32(1) << np.uint32(tl & 31)
    return out

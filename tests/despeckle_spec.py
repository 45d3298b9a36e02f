"""mi355_cwire_despeckle_* (include/mi355diff.h, "A tick without its speckle") stated in numpy, and the inputs its tests share.
Test infrastructure only; the product never imports it.

record -> pixel mask -> 8-neighbour count on a padded mask -> kept entries, reverted state, canonical record (cwire_spec)."""
import functools

import numpy as np

import cwire_spec as spec
from oracle import pyoracle as po

THR = 20          # the threshold of every core and oracle diff of these tests
SHAPES = [(37, 11), (33, 9), (64, 48), (160, 120), (1400, 3), (1, 64), (2, 40), (64, 1)]
DENSITIES = (0.05, 0.3, 0.7)
# Widths at which a 32-pixel bitmap word holds several row starts (W < 32), exactly one (W = 32), or a row ends one pixel before,
# on and one pixel behind a word; not in SHAPES, whose tests assert keep / drop counts that need not hold for frames this narrow
NARROW = [(3, 50), (5, 41), (7, 33), (16, 19), (31, 13), (32, 11), (63, 9), (65, 7), (96, 5)]


def neighbour_count(mask):
    """mask: bool [h, w] -> the changed pixels among the 8 around every pixel (pixels outside the frame count 0)."""
    h, w = mask.shape
    pad = np.zeros((h + 2, w + 2), np.int64)
    pad[1:-1, 1:-1] = mask
    c = np.zeros((h, w), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                c += pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return c


def keep_entries(width, height, xs, diff, need):
    """Which entries (xs ascending, byte indices < 3*width*height) stay: bool per entry.  A zero diff byte is no entry: it
    neither marks its pixel nor stays."""
    xs, diff = np.asarray(xs, np.int64), np.asarray(diff, np.uint8)
    live = diff != 0
    if need == 0:
        return live
    mask = np.zeros(width * height, bool)
    mask[xs[live] // 3] = True
    c = neighbour_count(mask.reshape(height, width)).reshape(-1)
    return live & (c[xs // 3] >= need)


def despeckle(width, height, recs, states, need, capacity=None):
    """recs: the S records back to back; states: uint8 [S, n] after the tick; need: S values ->
    (dropped uint32[S], offsets uint32[S + 1], frame_pos uint64[S + 1], records, states after [S, n], keep masks per stream).
    With a capacity the records that end past it are left out of `records` (as zero bytes; compare per record)."""
    S = len(need)
    off, xs, df = spec.decode(recs, S)
    states = np.array(states, np.uint8).reshape(S, -1).copy()
    out, ns, dropped, keeps = [], [], [], []
    for s in range(S):
        x, d = xs[int(off[s]):int(off[s + 1])].astype(np.int64), df[int(off[s]):int(off[s + 1])]
        assert (x < 3 * width * height).all()
        keep = keep_entries(width, height, x, d, int(need[s]))
        gone = ~keep & (d != 0)
        states[s][x[gone]] = states[s][x[gone]] - d[gone]            # uint8 arithmetic: the value before the tick
        out.append(np.frombuffer(spec.encode_frame(x[keep], d[keep]), np.uint8))
        ns.append(int(keep.sum())); dropped.append(int(gone.sum())); keeps.append(keep)
    pos = np.cumsum([0] + [r.size for r in out]).astype(np.uint64)
    if capacity is not None:
        out = [r if int(pos[s + 1]) <= capacity else np.zeros(r.size, np.uint8) for s, r in enumerate(out)]
    return (np.array(dropped, np.uint32), np.cumsum([0] + ns).astype(np.uint32), pos,
            np.concatenate(out) if out else np.empty(0, np.uint8), states, keeps)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def frames_for(w, h, density, seed, pre=None):
    """(pre-tick state, frame): a random state (or the given one); the frame is the state plus a perturbation above the
    threshold in one to three channels of the pixels drawn with `density`, plus one solid block."""
    rng = np.random.default_rng(1000 * w + 10 * h + seed)
    P = w * h
    pre = rng.integers(0, 256, 3 * P, dtype=np.uint8) if pre is None else np.asarray(pre, np.uint8)
    pix = rng.random(P) < density
    block = np.zeros((h, w), bool)
    bh, bw = max(1, h // 3), max(1, w // 4)
    y0, x0 = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
    block[y0:y0 + bh, x0:x0 + bw] = True
    chan = rng.random((P, 3)) < 0.6
    chan[np.arange(P), rng.integers(0, 3, P)] = True                     # at least one channel of a changed pixel
    chan[block.reshape(-1)] = True                                        # the block changes whole
    hit = ((pix | block.reshape(-1))[:, None] & chan).reshape(-1)
    step = rng.integers(THR + 1, 120, 3 * P)
    up = pre.astype(np.int64) + step <= 255
    cur = np.where(up, pre.astype(np.int64) + step, pre.astype(np.int64) - step)
    cur = np.where((cur < 0) | (cur > 255), (pre.astype(np.int64) + 128) % 256, cur)   # |cur - pre| = 128
    frame = np.where(hit, cur, pre).astype(np.uint8)
    return pre, frame


def tick_of(pre, frames):
    """The oracle's tick of the S (state, frame) pairs -> (records, counts, escapes, states after [S, n])."""
    offs, xs, df, post = [0], [], [], []
    for p, f in zip(pre, frames):
        c, x, d, st = po.diff_pack(f, p, THR)
        offs.append(offs[-1] + c); xs.append(x); df.append(d); post.append(st)
    recs, _ = spec.encode(np.array(offs, np.uint32), np.concatenate(xs), np.concatenate(df))
    counts, escapes = spec.headers(recs, len(pre))
    return recs, counts, escapes, np.stack(post)


@functools.lru_cache(maxsize=None)
def tick(w, h, density, S=1):
    """(pre [S, n], frames [S, n], records, counts, escapes, states after [S, n]) of S streams, made once and read-only."""
    pre, frames = (np.stack(z) for z in zip(*[frames_for(w, h, density, s) for s in range(S)]))
    out = (pre, frames) + tick_of(pre, frames)
    for z in out:
        z.setflags(write=False)
    return out


def degenerate(w, h, need):
    """Geometry forbids a kept entry: a pixel of a frame one pixel wide or high has at most 2 neighbours, of a frame two
    pixels wide (or high) at most 5."""
    return (min(w, h) == 1 and need >= 3) or (min(w, h) == 2 and need >= 6)


def density_for(need):
    """The density at which every listed 2-D shape keeps and drops something at this need."""
    return 0.3 if need <= 2 else 0.7


def blanked(pre, frames, recs, need, width, height):
    """frames': the tick's frames with every byte of every dropped pixel replaced by the state byte before the tick."""
    S = len(need)
    off, xs, df = spec.decode(recs, S)
    out = np.array(frames, np.uint8).copy()
    for s in range(S):
        x, d = xs[int(off[s]):int(off[s + 1])].astype(np.int64), df[int(off[s]):int(off[s + 1])]
        gone = ~keep_entries(width, height, x, d, int(need[s]))
        pix = np.unique(x[gone] // 3)
        for c in range(3):
            out[s][3 * pix + c] = pre[s][3 * pix + c]
    return out

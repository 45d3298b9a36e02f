"""mi355_cwire_split_* (include/mi355diff.h, "Records for a datagram socket") stated in numpy: the tests' reference for the piece
rule and the two capacity bounds.  Test infrastructure only; the product never imports it.

A record {n, e, code, esc, diff} is cut at every multiple of BLOCK entries; inside a block a piece [a, b) costs
bytes(a, b) = 8 + 2*pad4(b - a) + 4*(F(a) + #{k in (a, b): code[k] == 255}), F(a) = 1 if x_a >= 255 else 0, and from a the piece ends
at the largest b <= B = min(n, end of a's block) with bytes(a, b) <= M where b == B or (b - a) % 4 == 0.  The piece is the record
of the entries (x_k, diff_k), k in [a, b): cwire_spec encodes it."""
import numpy as np

import cwire_spec as spec

BLOCK = 65536


def piece_bytes(xs, a, b):
    """bytes(a, b) of the rule, from the indices alone: code[k] == 255 iff the gap before entry k is at least 255."""
    xs = np.asarray(xs, np.int64)
    inner = int(((xs[a + 1:b] - xs[a:b - 1] - 1) >= 255).sum())
    return 8 + 2 * spec.pad4(b - a) + 4 * (int(xs[a] >= 255) + inner)


def cuts(xs, M):
    """[(a, b)] of the pieces of one record with indices xs."""
    xs = np.asarray(xs, np.int64)
    n = xs.size
    esc = np.zeros(n + 1, np.int64)   # esc[k]: codes 255 among entries 1 .. k-1 ... as a prefix over the gaps of entries >= 1
    if n > 1:
        esc[2:] = np.cumsum((xs[1:] - xs[:-1] - 1) >= 255)
    out, a = [], 0
    while a < n:
        B = min(n, (a // BLOCK + 1) * BLOCK)
        F = int(xs[a] >= 255)
        best = None
        b = a
        while b < B:
            b = min(b + 4, B)
            cost = 8 + 2 * spec.pad4(b - a) + 4 * (F + int(esc[b] - esc[a + 1]))
            if cost > M:
                break
            best = b
        assert best is not None, "M >= 64 always admits four entries"
        out.append((a, best))
        a = best
    return out


def split_record(xs, diff, M):
    """-> [piece bytes] of one record, each the canonical encoding of its run of entries."""
    xs, diff = np.asarray(xs), np.asarray(diff, np.uint8)
    pieces = []
    for a, b in cuts(xs, M):
        p = spec.encode_frame(xs[a:b], diff[a:b])
        assert len(p) == piece_bytes(xs, a, b) <= M
        pieces.append(p)
    return pieces


def reference(recs, nrecords, M):
    """The records `recs` (uint8 array, nrecords canonical records back to back) -> (piece_first uint32[nrecords + 1], piece_pos
    uint64[pieces + 1], out uint8 array)."""
    off, xs, df = spec.decode(recs, nrecords)
    first, pos, out = [0], [0], []
    for r in range(nrecords):
        a, b = int(off[r]), int(off[r + 1])
        for p in split_record(xs[a:b], df[a:b], M):
            out.append(p)
            pos.append(pos[-1] + len(p))
        first.append(len(pos) - 1)
    return np.array(first, np.uint32), np.array(pos, np.uint64), np.frombuffer(b"".join(out), np.uint8).copy()


def records(segments):
    """[(xs, diff)] -> (the records back to back as a uint8 array, counts, escapes)."""
    off = np.cumsum([0] + [len(x) for x, _ in segments]).astype(np.uint32)
    xs = np.concatenate([np.asarray(x, np.int64) for x, _ in segments] + [np.empty(0, np.int64)]).astype(np.int32)
    df = np.concatenate([np.asarray(d, np.uint8) for _, d in segments] + [np.empty(0, np.uint8)]).astype(np.uint8)
    buf = spec.encode(off, xs, df)[0]
    counts, escapes = spec.headers(buf, len(segments))
    return buf, counts, escapes


SMALL, WIDE = (64, 48), (512, 128)   # the cores of the cases: 9216 and 196608 bytes per frame


def _dense(rng, n, start=0):
    return np.arange(start, start + n), rng.integers(1, 256, n)


def cases():
    """name -> ((width, height), [(xs, diff)], M): the shapes both forms are compared on."""
    rng = np.random.default_rng(20240)
    n_small, n_wide = 3 * SMALL[0] * SMALL[1], 3 * WIDE[0] * WIDE[1]
    out = {}
    for n in (0, 1, 3, 4, 5):
        out[f"small_n{n}"] = (SMALL, [(np.sort(rng.choice(n_small, n, replace=False)), rng.integers(1, 256, n))], 64)
    every300 = np.arange(0, n_wide, 300)
    for M in (64, 100):
        out[f"all_escape_M{M}"] = (WIDE, [(every300, rng.integers(1, 256, every300.size))], M)
    mixed = np.sort(np.concatenate([np.arange(10, 90), np.arange(400, 420), np.arange(1000, 9000, 299), np.arange(9001, 9100)]))
    out["mixed_M64"] = (SMALL, [(mixed, rng.integers(1, 256, mixed.size))], 64)
    out["dense_start_M64"] = (SMALL, [_dense(rng, 700)], 64)
    for M in (516, 520, 524):
        out[f"wave_seam_M{M}"] = (SMALL, [_dense(rng, 5000), _dense(rng, 3000, 1000)], M)
    for n in (65535, 65536, 65537, 65540, 131073):
        out[f"block_seam_n{n}"] = (WIDE, [_dense(rng, n, 17)], 1400)
    for R in (129, 1025):
        segs = []
        for r in range(R):
            cnt = 0 if r % 7 == 3 else int(rng.integers(0, 10))
            segs.append((np.sort(rng.choice(n_small, cnt, replace=False)), rng.integers(1, 256, cnt)))
        out[f"records_{R}"] = (SMALL, segs, 64)
    return out


def pieces_max(n, e, M):
    """A sufficient piece count: a piece that is not the last of its block could not take four more entries (at most 24 bytes),
    so it is larger than M - 24 and holds at least M - 35 of the record's 2*pad4(n) + 4e section bytes."""
    return -(-int(n) // BLOCK) + (2 * spec.pad4(n) + 4 * int(e)) // (M - 35)


def bytes_max(n, e, M):
    return spec.frame_bytes(n, e) + 12 * pieces_max(n, e, M)

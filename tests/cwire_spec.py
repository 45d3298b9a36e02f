"""The compact wire format (include/mi355diff.h, "compact wire format") stated in numpy: the tests' reference encoder and
decoder.  Test infrastructure only; the product never imports it.

Per frame, 4-aligned records back to back, little-endian:
    u32 n | u32 e | u8 code[n] | 0[pad4(n) - n] | u32 esc[e] | u8 diff[n] | 0[pad4(n) - n]
g_0 = xs[0], g_k = xs[k] - xs[k-1] - 1; code[k] = g_k if g_k < 255 else 255; esc = the g_k of the codes 255, in order."""
import numpy as np


def pad4(x):
    return (int(x) + 3) & ~3


def frame_bytes(n, e):
    return 8 + 2 * pad4(n) + 4 * int(e)


def gaps(xs):
    xs = np.asarray(xs, dtype=np.int64)
    if xs.size == 0:
        return np.empty(0, np.int64)
    g = np.empty(xs.size, np.int64)
    g[0] = xs[0]
    g[1:] = xs[1:] - xs[:-1] - 1
    assert (g >= 0).all(), "entries must be strictly ascending within a frame"
    return g


def encode_frame(xs, diff):
    xs = np.asarray(xs)
    diff = np.asarray(diff, dtype=np.uint8)
    n = xs.size
    g = gaps(xs)
    esc = g[g >= 255].astype(np.uint32)
    code = np.where(g >= 255, 255, g).astype(np.uint8)
    p = pad4(n) - n
    out = b"".join([np.array([n, esc.size], "<u4").tobytes(), code.tobytes(), bytes(p), esc.astype("<u4").tobytes(),
                    diff.tobytes(), bytes(p)])
    assert len(out) == frame_bytes(n, esc.size)
    return out


def encode(offsets, xs, diff):
    """(offsets[T+1], xs, diff) -> (bytes as uint8 array, frame_pos uint64[T+1])."""
    offsets = np.asarray(offsets).astype(np.int64)
    recs, pos = [], [0]
    for t in range(offsets.size - 1):
        a, b = offsets[t], offsets[t + 1]
        r = encode_frame(xs[a:b], diff[a:b])
        recs.append(r)
        pos.append(pos[-1] + len(r))
    return np.frombuffer(b"".join(recs), np.uint8).copy(), np.array(pos, np.uint64)


def headers(buf, nframes):
    """The (n, e) header of every frame, as a client reads them: (counts, escapes) uint32 arrays."""
    buf = np.asarray(buf, np.uint8)
    at, ns, es = 0, [], []
    for _ in range(nframes):
        n, e = (int(v) for v in buf[at:at + 8].view("<u4"))
        ns.append(n); es.append(e)
        at += frame_bytes(n, e)
    return np.array(ns, np.uint32), np.array(es, np.uint32)


def decode(buf, nframes):
    """bytes -> (offsets uint32[T+1], xs int32, diff uint8); asserts the record is well formed and canonical."""
    buf = np.asarray(buf, np.uint8)
    at, offs, xs_all, df_all = 0, [0], [], []
    for _ in range(nframes):
        n, e = (int(v) for v in buf[at:at + 8].view("<u4"))
        p = pad4(n)
        code = buf[at + 8:at + 8 + n].astype(np.int64)
        assert not buf[at + 8 + n:at + 8 + p].any()
        esc = buf[at + 8 + p:at + 8 + p + 4 * e].view("<u4").astype(np.int64)
        dstart = at + 8 + p + 4 * e
        diff = buf[dstart:dstart + n].copy()
        assert not buf[dstart + n:dstart + p].any()
        assert int((code == 255).sum()) == e
        g = code.copy()
        g[code == 255] = esc
        xs = np.cumsum(g + 1) - 1
        xs_all.append(xs.astype(np.int32)); df_all.append(diff)
        offs.append(offs[-1] + n)
        at += frame_bytes(n, e)
    cat = (lambda a, dt: np.concatenate(a).astype(dt) if a else np.empty(0, dt))
    return np.array(offs, np.uint32), cat(xs_all, np.int32), cat(df_all, np.uint8)

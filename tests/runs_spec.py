"""Run-coded records for the link (include/mi355diff.h, "Run-coded records") stated in numpy on top of cwire_spec: the tests'
reference transcoder.  Test infrastructure only; the product never imports it.

A compact record {n, e, code[n], esc[e], diff[n]} in the run form, 4-aligned, little-endian:
    u32 n | u32 e | u32 r | u8 gap[r] | 0[pad4(r) - r] | u8 len[r] | 0[pad4(r) - r] | u32 esc[e] | u8 diff[n] | 0[pad4(n) - n]
Entry k starts a run when k % 256 == 0 or code[k] != 0; gap = the start's code, len = the run's entries - 1."""
import numpy as np

from cwire_spec import frame_bytes, pad4

WHERE_SMALLER, ALWAYS = 0, 1
FORM_COMPACT, FORM_RUNS = 0, 1


def runs_frame_bytes(n, e, r):
    return 12 + 2 * pad4(r) + 4 * int(e) + pad4(n)


def link_bytes(form, n, e, r):
    return runs_frame_bytes(n, e, r) if form == FORM_RUNS else frame_bytes(n, e)


def smaller(n, r):
    return 4 + 2 * pad4(r) < pad4(n)


def _u8(b):
    return np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else np.asarray(b, np.uint8)


def sections(rec):
    """(n, e, code[n], esc bytes, diff[n]) of one compact record."""
    rec = _u8(rec)
    n, e = (int(v) for v in rec[:8].view("<u4"))
    p = pad4(n)
    return n, e, rec[8:8 + n], rec[8 + p:8 + p + 4 * e], rec[8 + p + 4 * e:8 + p + 4 * e + n]


def runs_of(code):
    """(gap uint8[r], len uint8[r]) of a code section."""
    code = np.asarray(code, np.uint8)
    n = code.size
    start = np.flatnonzero((code != 0) | (np.arange(n) % 256 == 0))
    length = np.diff(np.append(start, n))
    assert n == 0 or (start[0] == 0 and length.min() >= 1 and length.max() <= 256)
    return code[start], (length - 1).astype(np.uint8)


def to_runs(rec):
    """One compact record -> (its run form as bytes, r)."""
    n, e, code, esc, diff = sections(rec)
    gap, ln = runs_of(code)
    r = gap.size
    out = b"".join([np.array([n, e, r], "<u4").tobytes(), gap.tobytes(), bytes(pad4(r) - r), ln.tobytes(), bytes(pad4(r) - r),
                    esc.tobytes(), diff.tobytes(), bytes(pad4(n) - n)])
    assert len(out) == runs_frame_bytes(n, e, r)
    return out, r


def from_runs(run):
    """One record in the run form -> the compact record as bytes."""
    run = _u8(run)
    n, e, r = (int(v) for v in run[:12].view("<u4"))
    q = pad4(r)
    gap, ln = run[12:12 + r], run[12 + q:12 + q + r].astype(np.int64) + 1
    assert int(ln.sum()) == n and int((gap == 255).sum()) == e
    code = np.zeros(n, np.uint8)
    code[np.cumsum(ln) - ln] = gap
    rest = run[12 + 2 * q:]
    out = b"".join([np.array([n, e], "<u4").tobytes(), code.tobytes(), bytes(pad4(n) - n), rest[:4 * e].tobytes(),
                    rest[4 * e:4 * e + n].tobytes(), bytes(pad4(n) - n)])
    assert len(out) == frame_bytes(n, e)
    return out


def encode(buf, nrecords, policy):
    """Compact records back to back -> (forms uint32[nrecords, 4], pos uint64[nrecords + 1], the link bytes as uint8)."""
    buf = _u8(buf)
    at, forms, pos, parts = 0, [], [0], []
    for _ in range(nrecords):
        n, e = (int(v) for v in buf[at:at + 8].view("<u4"))
        rec = buf[at:at + frame_bytes(n, e)]
        run, r = to_runs(rec)
        form = FORM_RUNS if policy == ALWAYS or smaller(n, r) else FORM_COMPACT
        parts.append(run if form == FORM_RUNS else rec.tobytes())
        assert len(parts[-1]) == link_bytes(form, n, e, r)
        forms.append([form, n, e, r])
        pos.append(pos[-1] + len(parts[-1]))
        at += rec.size
    return (np.array(forms, np.uint32).reshape(-1, 4), np.array(pos, np.uint64), np.frombuffer(b"".join(parts), np.uint8).copy())


def decode(link, forms):
    """The link bytes and the sender's table -> (frame_pos uint64[nrecords + 1], compact records as uint8)."""
    link = _u8(link)
    at, pos, parts = 0, [0], []
    for form, n, e, r in np.asarray(forms).reshape(-1, 4).tolist():
        size = link_bytes(form, n, e, r)
        part = link[at:at + size]
        parts.append(from_runs(part) if form == FORM_RUNS else part.tobytes())
        pos.append(pos[-1] + len(parts[-1]))
        at += size
    return np.array(pos, np.uint64), np.frombuffer(b"".join(parts), np.uint8).copy()


# ---- the records the tests share ------------------------------------------------------------------------------------------------
def record(xs, seed=0):
    """The compact record of the ascending indices xs with seeded non-zero differences, as a uint8 array."""
    from cwire_spec import encode_frame
    xs = np.asarray(xs, np.int64)
    diff = (np.random.default_rng(1000 + seed).integers(1, 256, xs.size)).astype(np.uint8)
    return np.frombuffer(encode_frame(xs, diff), np.uint8).copy()


def mixed_xs(N, seed):
    """Runs of 1 .. 700 consecutive indices with gaps that are now and then escaped, inside a frame of N bytes."""
    rng = np.random.default_rng(seed)
    xs, x = [], int(rng.integers(0, 300))
    while True:
        length = int(rng.integers(1, 701)) if rng.random() < 0.5 else int(rng.integers(1, 4))
        if x + length > N:
            break
        xs.append(np.arange(x, x + length))
        x += length + (int(rng.integers(255, 900)) if rng.random() < 0.15 else int(rng.integers(1, 40)))
    return np.concatenate(xs) if xs else np.empty(0, np.int64)


def patterns(N):
    """{name: xs} of the index patterns of the issue that fit a frame of N bytes."""
    p = {
        "empty": np.empty(0, np.int64),
        "first": np.array([0]),
        "last": np.array([N - 1]),
        "whole": np.arange(N),
        "alternating": np.arange(0, N, 2),
        "straddle": np.concatenate([np.arange(0, 256, 2), np.arange(300, 600)]),          # a 300-entry run from entry 128
        "r3": np.array([5, 6, 7, 100, 101, 400]),
        "r4": np.array([5, 6, 7, 100, 101, 400, 900, 901]),
        "r5": np.array([5, 6, 7, 100, 101, 400, 900, 901, 2000]),
    }
    for n in (255, 256, 257, 4095, 4096, 4097):
        p[f"run{n}"] = np.arange(1, 1 + n)
    # a 255 code exactly at entries 256 and 4096: consecutive indices with a jump of 300 in front of those entries
    xs = np.arange(4200, dtype=np.int64)
    xs[256:] += 300
    xs[4096:] += 300
    p["escape_on_cut"] = xs
    for seed in (1, 2, 3):
        p[f"mixed{seed}"] = mixed_xs(N, seed)
    return {k: np.asarray(v, np.int64) for k, v in p.items() if v.size == 0 or v[-1] < N}

"""CPU: mi355_cwire_check_host, the definition of the record check (include/mi355diff.h, "Checking records before they are
used") -- four uint32 words per record: flags, 255 codes, first entry past the frame, 1 + the last index, saturated.

The reference is the decode rule stated in numpy below, on top of cwire_spec's layout: int64 holds every sum exactly (at most
67200 entries of at most 2^32 each), so it is the rule "with unbounded integers".  All comparisons are exact.  The cases are
seeded records built with cwire_spec.encode_frame and then damaged, alone and in pairs; test_cwire_check_gpu.py runs the same
cases through the device form."""
import ctypes as C

import numpy as np
import pytest

import cwire_spec as spec
from cudavideostream_amd import (CWIRE_BAD_CODES, CWIRE_BAD_ESCAPE, CWIRE_BAD_HEADER, CWIRE_BAD_PAD, CWIRE_BAD_RANGE,
                                 cwire_check_host, lib)

SAT = 0xFFFFFFFF
FLAGS = (CWIRE_BAD_CODES, CWIRE_BAD_RANGE, CWIRE_BAD_PAD, CWIRE_BAD_ESCAPE, CWIRE_BAD_HEADER)
SIZES = (1221, 67200)   # 37x11 and 160x140


# ---- the reference ------------------------------------------------------------------------------------------------------------
def sections(rec, n, e):
    """(code[n], code pad, esc[e] as int64, diff[n], diff pad) of the record {n, e} whose bytes are rec."""
    p = spec.pad4(n)
    esc = rec[8 + p:8 + p + 4 * e].copy().view("<u4").astype(np.int64)
    d0 = 8 + p + 4 * e
    return rec[8:8 + n], rec[8 + n:8 + p], esc, rec[d0:d0 + n], rec[d0 + n:d0 + p]


def ref_walk(rec, n, e):
    """The decode rule: (X_k for every k as int64, bad[k]: entry k is an escape ranked at or past e, the number of 255 codes)."""
    code, _, esc, _, _ = sections(rec, n, e)
    is255 = code == 255
    rank = np.cumsum(is255) - is255
    bad = is255 & (rank >= e)
    inc = code.astype(np.int64) + 1
    good = is255 & ~bad
    inc[good] = esc[rank[good]] + 1
    inc[bad] = 0
    return np.cumsum(inc), bad, int(is255.sum())


def ref_verdict(rec, n, e, N):
    """The four words of the record {n, e} (the host's headers) whose bytes are rec, on a frame of N bytes."""
    rec = np.asarray(rec, np.uint8)
    assert rec.size == spec.frame_bytes(n, e)
    _, cpad, esc, _, dpad = sections(rec, n, e)
    X, _, r = ref_walk(rec, n, e)
    over = np.nonzero(X > N)[0]
    first = int(over[0]) if over.size else n
    flags = 0
    if r != e:
        flags |= CWIRE_BAD_CODES
    if first < n:
        flags |= CWIRE_BAD_RANGE
    if cpad.any() or dpad.any():
        flags |= CWIRE_BAD_PAD
    if (esc[:min(e, r)] < 255).any():
        flags |= CWIRE_BAD_ESCAPE
    hn, he = (int(v) for v in rec[:8].copy().view("<u4"))
    if (hn, he) != (n, e):
        flags |= CWIRE_BAD_HEADER
    return np.array([flags, r, first, min(int(X[-1]), SAT) if n else 0], np.uint32)


def ref_decode(rec, n, e, N):
    """What the record decodes to on a frame of N bytes: the entries that are neither a bad escape nor at or past N."""
    X, bad, _ = ref_walk(rec, n, e)
    _, _, _, diff, _ = sections(rec, n, e)
    keep = ~bad & (X <= N)
    return X[keep] - 1, diff[keep]


# ---- records and damage -------------------------------------------------------------------------------------------------------
def make_record(rng, N, n, sparse=False):
    """A well-formed record of n entries on a frame of N bytes -> (bytes, n, e).  sparse: every gap is escaped."""
    if sparse:
        assert n * 256 <= N
        xs = 256 * np.sort(rng.choice(N // 256, n, replace=False)).astype(np.int64) + 255
    else:
        xs = np.sort(rng.choice(N, n, replace=False)).astype(np.int64)
    diff = rng.integers(1, 256, n).astype(np.uint8)
    rec = np.frombuffer(spec.encode_frame(xs, diff), np.uint8).copy()
    return rec, n, int(rec[4:8].view("<u4")[0])


def esc_at(rec, n):
    return 8 + spec.pad4(n)


def put_esc(rec, n, r, value):
    rec[esc_at(rec, n) + 4 * r:esc_at(rec, n) + 4 * r + 4] = np.array([value], "<u4").view(np.uint8)


# Every mutation takes (rec, n, e, N, rng) and returns the damaged copy, or None where the record has no place for it.
def m_code_to_255(rec, n, e, N, rng):
    plain = np.nonzero(rec[8:8 + n] != 255)[0]
    if not plain.size:
        return None
    out = rec.copy()
    out[8 + rng.choice(plain)] = 255
    return out


def m_255_to_7(rec, n, e, N, rng):
    escs = np.nonzero(rec[8:8 + n] == 255)[0]
    if not escs.size:
        return None
    out = rec.copy()
    out[8 + rng.choice(escs)] = 7
    return out


def m_esc_value(value):
    def mutate(rec, n, e, N, rng):
        if not e:
            return None
        out = rec.copy()
        put_esc(out, n, int(rng.integers(e)), value)
        return out
    mutate.__name__ = "m_esc_%x" % value
    return mutate


def m_two_escapes_wrap(rec, n, e, N, rng):
    """esc[0] + 1 + esc[1] + 1 = 2^32 + 5: modulo 2^32 the record stays inside the frame."""
    if e < 2:
        return None
    out = rec.copy()
    put_esc(out, n, 0, 0x80000000)
    put_esc(out, n, 1, 0x80000003)
    return out


def m_pad(section):
    def mutate(rec, n, e, N, rng):
        if n % 4 == 0:
            return None
        out = rec.copy()
        first = 8 + n if section == "code" else 8 + spec.pad4(n) + 4 * e + n
        out[first + int(rng.integers(spec.pad4(n) - n))] = int(rng.integers(1, 256))
        return out
    mutate.__name__ = "m_pad_" + section
    return mutate


def m_header(word):
    def mutate(rec, n, e, N, rng):
        out = rec.copy()
        out[4 * word] ^= 1 << int(rng.integers(8))
        return out
    mutate.__name__ = "m_header_%d" % word
    return mutate


MUTATIONS = [m_code_to_255, m_255_to_7, m_esc_value(3), m_esc_value(254), m_esc_value(SAT), m_two_escapes_wrap, m_pad("code"),
             m_pad("diff"), m_header(0), m_header(1)]


def last_gap_records(rng, N, n):
    """Two records whose last entry makes X exactly N (index N - 1, good) and N + 1 (index N: bad at entry n - 1)."""
    xs = np.sort(rng.choice(N - 1, n - 1, replace=False)).astype(np.int64)
    diff = rng.integers(1, 256, n).astype(np.uint8)
    out = []
    for last in (N - 1, N):
        rec = np.frombuffer(spec.encode_frame(np.append(xs, last), diff), np.uint8).copy()
        out.append((rec, n, int(rec[4:8].view("<u4")[0])))
    return out


def build_cases(N):
    """[(name, bytes, n, e)] for a frame of N bytes: the records as made, each damaged by one mutation, and by two."""
    rng = np.random.default_rng(N)
    cases = []
    counts = [0, 1, 3, 4, 5, 18, 47, 130] + ([600, 4099] if N > 5000 else [401])
    for tag in ["n%d" % n for n in counts] + ["s3", "s4"]:   # (s: a sparse record of that many entries)
        rec, n, e = make_record(rng, N, int(tag[1:]), sparse=tag[0] == "s")
        cases.append((tag, rec, n, e))
        for i, m1 in enumerate(MUTATIONS):
            one = m1(rec, n, e, N, rng)
            if one is None:
                continue
            cases.append(("%s-%s" % (tag, m1.__name__), one, n, e))
            for m2 in MUTATIONS[i + 1:]:
                two = m2(one, n, e, N, rng)
                if two is not None:
                    cases.append(("%s-%s-%s" % (tag, m1.__name__, m2.__name__), two, n, e))
    for n in (1, 2, 37):
        for tag, (rec, n, e) in zip(("exact", "over"), last_gap_records(rng, N, n)):
            cases.append(("n%d-last-%s" % (n, tag), rec, n, e))
    return cases


CASES = {N: build_cases(N) for N in SIZES}


def batch_of(cases):
    """The cases' records back to back -> (bytes, counts, escapes)."""
    buf = np.concatenate([c[1] for c in cases])
    return buf, np.array([c[2] for c in cases], np.uint32), np.array([c[3] for c in cases], np.uint32)


REFERENCE = {N: np.array([ref_verdict(rec, n, e, N) for _, rec, n, e in CASES[N]], np.uint32) for N in SIZES}


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_flag():
    """The reference sees each of the five flags, flag-free records, and the named seams among the cases."""
    for N in SIZES:
        assert len(CASES[N]) >= 200
        ref = REFERENCE[N]
        for f in FLAGS:
            assert (ref[:, 0] & f).any(), (N, f)
        assert (ref[:, 0] == 0).sum() >= 10
        by_name = {c[0]: ref[i] for i, c in enumerate(CASES[N])}
        for n in (0, 1, 3, 4, 5):
            assert list(by_name["n%d" % n][:3]) == [0, by_name["n%d" % n][1], n]
        assert list(by_name["n0"]) == [0, 0, 0, 0]
        for n in (1, 2, 37):
            assert list(by_name["n%d-last-exact" % n][[0, 2, 3]]) == [0, n, N]
            assert list(by_name["n%d-last-over" % n][[0, 2, 3]]) == [CWIRE_BAD_RANGE, n - 1, N + 1]
        wraps = 0
        for (name, rec, n, e), v in zip(CASES[N], ref):
            if name.split("-", 1)[-1] == "m_two_escapes_wrap":   # (that damage alone)
                X, _, _ = ref_walk(rec, n, e)
                # past 2^32 and, modulo 2^32, back inside the frame: only a sum that cannot wrap sees it
                assert X[-1] >= 2 ** 32 and X[-1] % 2 ** 32 <= N
                assert v[0] == CWIRE_BAD_RANGE and v[3] == SAT
                wraps += 1
        assert wraps >= 2


@pytest.mark.parametrize("N", SIZES)
def test_all_four_words_against_the_reference(N):
    buf, counts, escapes = batch_of(CASES[N])
    got = cwire_check_host(buf, counts, escapes, N)
    bad = np.nonzero((got != REFERENCE[N]).any(axis=1))[0]
    assert np.array_equal(got, REFERENCE[N]), [(CASES[N][i][0], list(got[i]), list(REFERENCE[N][i])) for i in bad[:5]]
    # one record at a time, at an odd address: the host form needs no alignment
    for i in range(0, len(CASES[N]), 7):
        _, rec, n, e = CASES[N][i]
        shifted = np.concatenate([np.zeros(1, np.uint8), rec])[1:]
        assert np.array_equal(cwire_check_host(shifted, [n], [e], N)[0], REFERENCE[N][i])


@pytest.mark.parametrize("N", SIZES)
def test_accepted_by_the_host_client_exactly_when_codes_and_range_are_clear(N):
    L = lib.load()
    seen = set()
    for (name, rec, n, e), v in zip(CASES[N], REFERENCE[N]):
        if v[0] & CWIRE_BAD_HEADER:
            continue
        state = np.zeros(N, np.uint8)
        consumed = C.c_size_t(0)
        rc = L.mi355_cwire_apply_host(state.ctypes.data, N, rec.ctypes.data, rec.size, 1, C.byref(consumed))
        assert (rc == lib.OK) == ((int(v[0]) & 3) == 0), (name, rc, list(v))
        seen.add(rc == lib.OK)
    assert seen == {True, False}


@pytest.mark.parametrize("N", SIZES)
def test_flag_free_exactly_when_canonical(N):
    seen = set()
    for (name, rec, n, e), v in zip(CASES[N], REFERENCE[N]):
        xs, diff = ref_decode(rec, n, e, N)
        canonical = spec.encode_frame(xs, diff) == rec.tobytes()
        assert (v[0] == 0) == canonical, (name, list(v))
        seen.add(canonical)
    assert seen == {True, False}


def test_refusals_leave_the_verdicts_untouched():
    L = lib.load()
    N = 1221
    rng = np.random.default_rng(5)
    a, na, ea = make_record(rng, N, 9)
    b, nb, eb = make_record(rng, N, 30)
    buf = np.concatenate([a, b])
    counts, escapes = np.array([na, nb], np.uint32), np.array([ea, eb], np.uint32)
    verdicts = np.full((2, 4), 0xA5A5A5A5, np.uint32)

    def call(frame_bytes=N, cwire=buf.ctypes.data, nbytes=buf.size, c=counts, e=escapes, k=2, v=verdicts.ctypes.data):
        return L.mi355_cwire_check_host(frame_bytes, cwire, nbytes, c.ctypes.data if c is not None else None,
                                        e.ctypes.data if e is not None else None, k, v)

    refused = [
        call(cwire=None), call(c=None), call(e=None), call(v=None),                      # a null pointer with nrecords > 0
        call(k=-1),
        call(e=np.array([ea, nb + 1], np.uint32)),                                       # more escapes than entries
        call(frame_bytes=nb - 1),                                                        # more entries than frame bytes
        call(frame_bytes=2 ** 32 - 1), call(frame_bytes=2 ** 40),
        call(nbytes=buf.size - 1), call(nbytes=a.size), call(nbytes=0),                  # records that end past cwire_bytes
    ]
    assert refused == [lib.ERR_INVALID] * len(refused)
    assert (verdicts == 0xA5A5A5A5).all()
    assert call(k=0, cwire=None, c=None, e=None, v=None) == lib.OK and (verdicts == 0xA5A5A5A5).all()
    assert call(frame_bytes=2 ** 32 - 2) == lib.OK
    assert call() == lib.OK
    assert np.array_equal(verdicts, [ref_verdict(a, na, ea, N), ref_verdict(b, nb, eb, N)])
    with pytest.raises(lib.Mi355Error):
        cwire_check_host(buf[:-4], counts, escapes, N)

"""-m gpu: mi355_cwire_check_batch -- one verdict of four uint32 words per compact record, from the records alone
(include/mi355diff.h, "Checking records before they are used").  Every comparison is exact: the verdicts equal
mi355_cwire_check_host on the same bytes and the numpy statement of the decode rule in test_cwire_check_host.py.  Inputs and
verdicts live in guarded buffers (gpu_util) that start as a non-zero pattern; each case asserts from the reference, before the
launch, that its input reaches the seam it is for."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import (CWIRE_BAD_CODES, CWIRE_BAD_ESCAPE, CWIRE_BAD_HEADER, CWIRE_BAD_PAD, CWIRE_BAD_RANGE,
                                 cwire_bytes_max, cwire_check_host, lib, synth)
from gpu_util import DEV, CUDACore, Guarded, Region
from test_cwire_check_host import CASES, REFERENCE, SAT, batch_of, m_code_to_255, make_record, put_esc, ref_verdict, ref_walk

pytestmark = pytest.mark.gpu

GEOM = {67200: (160, 140), 1221: (37, 11)}
CHUNK = 4096   # codes per workgroup of the chunk table


def run_check(core, buf, counts, escapes, skew=0, spare=2):
    """The device form on the records of buf -> uint32[k, 4]; the input is unchanged, nothing but the k verdicts is written."""
    k = len(counts)
    src = Guarded(buf.size, torch.uint8, skew=skew, data=buf)
    out = Guarded(4 * (k + spare), torch.int32)
    assert src.ptr % 16 == skew
    torch.cuda.synchronize()
    core.cwire_check_batch(src.ptr, counts, escapes, k, out.ptr)
    core.synchronize()
    assert np.array_equal(src.get(), buf)
    return out.get(written=4 * k).view(np.uint32)[:4 * k].reshape(k, 4).copy()


def check_records(core, N, records, skew=0):
    """records: [(bytes, n, e)].  Device form == host form == the numpy reference -> the reference's verdicts."""
    buf, counts, escapes = batch_of([(None,) + tuple(r) for r in records])
    want = np.array([ref_verdict(rec, n, e, N) for rec, n, e in records], np.uint32)
    assert np.array_equal(cwire_check_host(buf, counts, escapes, N), want)
    got = run_check(core, buf, counts, escapes, skew=skew)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert np.array_equal(got, want), [(int(i), records[i][1:], list(got[i]), list(want[i])) for i in bad[:5]]
    return want


def encoded(xs, diff=None):
    xs = np.asarray(xs, np.int64)
    diff = np.ones(xs.size, np.uint8) if diff is None else diff
    rec = np.frombuffer(spec.encode_frame(xs, diff), np.uint8).copy()
    return rec, xs.size, int(rec[4:8].copy().view("<u4")[0])


# ---- 1. the host test's cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", sorted(GEOM))
def test_the_mutations_of_the_host_test(N):
    cases = CASES[N]
    buf, counts, escapes = batch_of(cases)
    assert all((REFERENCE[N][:, 0] & f).any() for f in (CWIRE_BAD_CODES, CWIRE_BAD_RANGE, CWIRE_BAD_PAD, CWIRE_BAD_ESCAPE,
                                                        CWIRE_BAD_HEADER)) and (REFERENCE[N][:, 0] == 0).any()
    w, h = GEOM[N]
    with CUDACore(w, h, max_batch=len(cases)) as core:
        got = run_check(core, buf, counts, escapes)
    bad = np.nonzero((got != REFERENCE[N]).any(axis=1))[0]
    assert np.array_equal(got, REFERENCE[N]), [(cases[i][0], list(got[i]), list(REFERENCE[N][i])) for i in bad[:5]]
    assert np.array_equal(got, cwire_check_host(buf, counts, escapes, N))


# ---- 2. entry counts around the kernels' rounds -------------------------------------------------------------------------------
SEAMS = (255, 256, 1023, 1024, 4095, 4096)   # lanes 63 | 64 of a wave's four-entry step, rounds of 1024, chunks of 4096


def dense_xs(rng, n, escapes_at):
    """n ascending indices with gaps of 0 .. 3, and gaps of 300 (escapes) at the positions escapes_at."""
    g = rng.integers(0, 4, n).astype(np.int64)
    g[np.array([k for k in escapes_at if k < n], np.intp)] = 300
    return np.cumsum(g + 1) - 1


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193])
def test_entry_counts_around_the_rounds(n):
    N = 67200
    rng = np.random.default_rng(n)
    xs = dense_xs(rng, n, SEAMS)
    assert xs[-1] < N
    diff = rng.integers(1, 256, n).astype(np.uint8)
    records, expect = [encoded(xs, diff)], [(0, n)]
    code = records[0][0][8:8 + n]
    assert all(code[k] == 255 for k in SEAMS if k < n)          # an escape on either side of every seam below n
    # the first out-of-range entry: the last of chunk 0, the first of chunk 1, the last of the record
    for k in sorted({min(n, CHUNK) - 1, n - 1} | ({CHUNK} if n > CHUNK else set())):
        far = xs.copy()
        far[k:] += N
        records.append(encoded(far, diff))
        expect.append((CWIRE_BAD_RANGE, k))
    # a bad escape (ranked at e) in chunk 0, no escape code behind it: the entries behind still count, one step lower
    rec, _, e = encoded(dense_xs(rng, n, (10, 20)), diff)
    assert e == 2 and rec[8 + 30] != 255
    rec[8 + 30] = 255
    _, bad, r = ref_walk(rec, n, e)
    assert r == 3 and list(np.nonzero(bad)[0]) == [30] and not (rec[8 + 31:8 + n] == 255).any()
    records.append((rec, n, e))
    expect.append((CWIRE_BAD_CODES, n))
    with CUDACore(160, 140, max_batch=len(records)) as core:
        want = check_records(core, N, records)
    assert [(int(v[0]), int(v[2])) for v in want] == expect
    assert want[0][3] == xs[-1] + 1 and want[0][1] == len([k for k in SEAMS if k < n])


# ---- 3. sums past 2^32 ----------------------------------------------------------------------------------------------------------
def test_sums_past_2_to_32_do_not_wrap():
    N = 67200
    rng = np.random.default_rng(32)
    records, first = [], []

    def add(n, values):
        """A dense record of n entries whose escapes at the positions `values` are given these values."""
        rec, _, e = encoded(dense_xs(rng, n, sorted(values)))
        assert e == len(values)
        for r, k in enumerate(sorted(values)):
            put_esc(rec, n, r, values[k])
        records.append((rec, n, e))

    add(5, {0: 0x80000000, 2: 0x80000003})                       # two escapes of one lane's four entries
    first.append(0)
    add(300, {10: 0x80000000, 20: 0x80000003})                   # ... of one chunk: the chunk's own sum passes 2^32
    first.append(10)
    add(4200, {10: 0x80000000, 4096: 0x80000003})                # ... of two chunks: only the record's prefix passes it
    first.append(10)
    add(8193, {100: SAT, 4100: SAT, 8192: SAT})                  # each escape alone is 2^32: modulo 2^32 it adds nothing
    first.append(100)
    add(4097, {4096: SAT})                                       # ... as the record's last entry, alone in its chunk
    first.append(4096)
    add(1025, {1024: SAT - 1})                                   # 2^32 - 1: does not wrap by itself, saturates word 3
    first.append(1024)
    for (rec, n, e), k in zip(records, first):
        X, _, _ = ref_walk(rec, n, e)
        assert X[-1] >= 2 ** 32 - 1 and X[-1] % 2 ** 32 <= N     # the wrapped sum lands inside the frame
        assert X[k] > N and (k == 0 or X[k - 1] <= N)
    with CUDACore(160, 140, max_batch=len(records)) as core:
        want = check_records(core, N, records)
    assert [list(v[[0, 2, 3]]) for v in want] == [[CWIRE_BAD_RANGE, k, SAT] for k in first]


# ---- 4. record counts across the table launches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 128, 129, 257])
def test_record_counts_across_the_table_launches(count):
    """Headers travel 128 per table launch.  Small records, one of no entries first, last and at every seventh place; one bad
    record among good neighbours, whose verdicts stay clean."""
    N = 1221
    rng = np.random.default_rng(count)
    sizes = [0 if i in (0, count - 1) or i % 7 == 3 else int(rng.integers(1, 60)) for i in range(count)]
    records = [make_record(rng, N, n) for n in sizes]
    bad_at = None
    if count > 1:
        bad_at = max(i for i in range(count // 2 + 1) if sizes[i] > 4)
        rec, n, e = records[bad_at]
        records[bad_at] = (m_code_to_255(rec, n, e, N, rng), n, e)
    with CUDACore(37, 11, max_batch=260) as core:
        want = check_records(core, N, records)
    for i, v in enumerate(want):
        if i == bad_at:
            assert v[0] & CWIRE_BAD_CODES
        else:
            assert v[0] == 0 and v[2] == sizes[i], (i, list(v))
    assert list(want[0]) == [0, 0, 0, 0] and list(want[-1]) == [0, 0, 0, 0]


# ---- 5. alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skew", [0, 4, 8, 12])
def test_every_dword_alignment_of_the_input(skew):
    N = 67200
    rng = np.random.default_rng(skew)
    records = [make_record(rng, N, n) for n in (5, 0, 4099, 130, 3)]
    rec, n, e = records[2]
    damaged = rec.copy()
    damaged[8 + n] = 9                                           # a pad byte of the code section (4099 = 4 * 1024 + 3)
    records.append((damaged, n, e))
    with CUDACore(160, 140, max_batch=8) as core:
        want = check_records(core, N, records, skew=skew)
    assert list(want[:, 0]) == [0, 0, 0, 0, 0, CWIRE_BAD_PAD]


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    N = 1221
    rng = np.random.default_rng(6)
    records = [make_record(rng, N, n) for n in (9, 30)]
    buf, counts, escapes = batch_of([(None,) + r for r in records])
    src = Guarded(buf.size, torch.uint8, data=buf)
    out = Guarded(4 * 4, torch.int32)
    big = np.array([counts[0], N + 1], np.uint32)
    with CUDACore(37, 11, max_batch=3) as core:
        torch.cuda.synchronize()

        def call(cwire=src.ptr, c=counts, e=escapes, k=2, v=out.ptr):
            return core._lib.mi355_cwire_check_batch(core._h, cwire, None if c is None else c.ctypes.data,
                                                     None if e is None else e.ctypes.data, k, v)

        refused = [
            call(k=-1), call(k=4),                                                 # outside [0, max_batch]
            call(cwire=None), call(c=None), call(e=None), call(v=None),            # a null pointer with nrecords > 0
            call(e=np.array([escapes[0], counts[1] + 1], np.uint32)),              # more escapes than entries
            call(c=big),                                                           # more entries than frame bytes
            call(cwire=src.ptr + 1), call(cwire=src.ptr + 2), call(v=out.ptr + 2),  # not 4-byte aligned
            call(v=src.ptr), call(v=src.ptr + buf.size - 4), call(v=src.ptr - 28),  # the verdicts overlap the input span
        ]
        assert refused == [lib.ERR_INVALID] * len(refused)
        assert call(k=0) == lib.OK and call(k=0, cwire=None, c=None, e=None, v=None) == lib.OK   # nothing to do
        core.synchronize()
        assert np.array_equal(src.get(), buf)
        out.get(written=0)
        # right behind the input span is not an overlap
        both = Guarded(buf.size + 32, torch.uint8, data=np.concatenate([buf, np.full(32, 0x5C, np.uint8)]))
        torch.cuda.synchronize()
        assert call(cwire=both.ptr, v=both.ptr + buf.size) == lib.OK
        core.synchronize()
        got = both.get()
        assert np.array_equal(got[:buf.size], buf)
        assert np.array_equal(got[buf.size:].view(np.uint32).reshape(2, 4), [ref_verdict(*r, N) for r in records])


# ---- 7. records of the library's own calls; ordering; scratch reuse -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tick(w, h, S, thr=20):
    """One frame of each of S webcam-like streams -> (bases [S][n], frames [S][n]); read-only."""
    bases, frames = [], []
    for s in range(S):
        base, fr = synth.webcam_stream(1, w, h, seed=3 + 5 * s, device=DEV)
        bases.append(base.cpu().numpy())
        frames.append(fr.cpu().numpy()[0])
    out = (np.stack(bases), np.stack(frames))
    for a in out:
        a.setflags(write=False)
    return out


def last_plus_one(recs, k):
    """Word 3 of k well-formed records: 1 + the last index of each (0 for a record of no entries)."""
    off, xs, _ = spec.decode(recs, k)
    return [int(xs[off[i + 1] - 1]) + 1 if off[i + 1] > off[i] else 0 for i in range(k)]


def test_sender_check_receiver_on_one_core_without_synchronisation():
    """diff_multi_cwire_batch, the check, apply_multi_cwire_batch on ONE core: once with a synchronisation after every call, once
    with none in between.  Same verdicts (all clean, word 3 = 1 + the last index), same states; and the check before the apply
    (they share the chunk scratch) leaves the states bit-identical to the apply alone."""
    w, h, S = 160, 140, 5
    n = 3 * w * h
    bases, frames = tick(w, h, S)
    cap = cwire_bytes_max(n, S)
    fr = Region(S, n).put(frames)
    with CUDACore(w, h, max_batch=S) as core:
        results = []
        for chain in (False, True, None):   # synchronised; unsynchronised; the apply alone (no check at all)
            srv, cli = Region(S, n).put(bases), Region(S, n).put(bases)
            off, pos, cw = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
            out = Guarded(4 * S, torch.int32)
            torch.cuda.synchronize()
            core.diff_multi_cwire_batch(fr.ptr, srv.ptr, S, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
            if not chain:
                core.synchronize()
                nbytes = int(pos.get().view(np.uint64)[S])
                counts, escapes = spec.headers(cw.get()[:nbytes], S)   # (the headers of the chain: the same tick again)
            if chain is not None:
                core.cwire_check_batch(cw.ptr, counts, escapes, S, out.ptr)
            if chain is False:
                core.synchronize()
            core.apply_multi_cwire_batch(cw.ptr, counts, escapes, S, cli.ptr)
            core.synchronize()
            results.append((out.get().view(np.uint32).reshape(S, 4).copy(), cli.get(), srv.get(), cw.get()[:nbytes].copy()))
    (v_sync, c_sync, s_sync, recs), (v_chain, c_chain, s_chain, recs2), (_, c_alone, _, recs3) = results
    assert np.array_equal(recs, recs2) and np.array_equal(recs, recs3) and counts.sum() > 0
    want = np.array([[0, escapes[i], counts[i], x] for i, x in enumerate(last_plus_one(recs, S))], np.uint32)
    assert np.array_equal(v_sync, want) and np.array_equal(v_chain, want)
    assert np.array_equal(want, np.array([ref_verdict(r, k, e, n) for r, k, e in split(recs, counts, escapes)], np.uint32))
    # (a receiver's states are the sender's: the frames up to the threshold)
    assert np.array_equal(s_sync, s_chain) and not np.array_equal(s_sync, bases)
    assert np.array_equal(c_sync, s_sync) and np.array_equal(c_chain, s_sync) and np.array_equal(c_alone, s_sync)
    assert np.abs(c_chain.astype(np.int16) - frames).max() <= 20


def split(recs, counts, escapes):
    at = 0
    for k, e in zip(counts, escapes):
        size = spec.frame_bytes(k, e)
        yield recs[at:at + size], int(k), int(e)
        at += size


def test_records_of_the_coalescer_are_clean():
    w, h, S, T = 160, 140, 3, 4
    n, B = 3 * w * h, 12
    bases, frames = [], []
    for s in range(S):
        base, fr = synth.webcam_stream(T, w, h, seed=11 + 3 * s, device=DEV)
        bases.append(base.cpu().numpy())
        frames.extend(fr.cpu().numpy())
    cap = cwire_bytes_max(n, B)
    srv, fr = Region(S, n).put(bases), Region(B, n).put(frames)
    off, pos, cw = Guarded(B + 1, torch.int32), Guarded(B + 1, torch.int64), Guarded(cap)
    off1, pos1, cw1 = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cwire_bytes_max(n, S))
    with CUDACore(w, h, max_batch=B) as core:
        torch.cuda.synchronize()
        core.diff_multi_stream_cwire_batch(fr.ptr, srv.ptr, S, T, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
        core.synchronize()
        burst = cw.get()[:int(pos.get().view(np.uint64)[B])].copy()
        counts, escapes = spec.headers(burst, B)
        core.cwire_coalesce_cwire_batch(cw.ptr, counts, escapes, S, T, off1.ptr, pos1.ptr, cw1.ptr, cwire_bytes_max(n, S))
        core.synchronize()
        one = cw1.get()[:int(pos1.get().view(np.uint64)[S])].copy()
        for recs, k in ((burst, B), (one, S)):
            c, e = spec.headers(recs, k)
            assert c.sum() > 0
            want = check_records(core, n, list(split(recs, c, e)))
            assert np.array_equal(want, np.array([[0, e[i], c[i], x] for i, x in enumerate(last_plus_one(recs, k))], np.uint32))

"""-m gpu: mi355_cwire_runs_encode_batch / mi355_cwire_runs_decode_batch -- compact records run-coded for the link and back
(include/mi355diff.h, "Run-coded records").  The reference of every comparison is the host form, which test_cwire_runs_abi.py holds
to the numpy statement of the format (tests/runs_spec.py); forms, positions and bytes are compared bit for bit.  Inputs and outputs
live in guarded buffers (gpu_util) that start as a non-zero pattern.  Cores of 64x48 (N = 9216, three chunks of 4096 codes) and
160x120 (N = 57 600, fifteen chunks); the patterns (runs_spec.patterns) reach every cut at 256 entries, the chunk seams, the pads of
gap[] and len[] and the ragged dwords that two chunks share; one call holds 130 records (the record tables take 128 and 64 a
launch)."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
import runs_spec as rs
from cudavideostream_amd import cwire_runs_bytes_max, cwire_runs_decode_host, cwire_runs_encode_host, lib
from gpu_util import GUARD, CUDACore, Guarded, Region, to_dev

pytestmark = pytest.mark.gpu

SIZES = {"small": (64, 48), "wide": (160, 120)}
POLICIES = [lib.RUNS_WHERE_SMALLER, lib.RUNS_ALWAYS]


@pytest.fixture(scope="module")
def cores():
    with CUDACore(*SIZES["small"], max_batch=130) as small, CUDACore(*SIZES["wide"], max_batch=24) as wide:
        yield {"small": small, "wide": wide}


@functools.lru_cache(maxsize=None)
def stream(size):
    """-> (names, records back to back, counts, escapes) of the patterns that fit the frame, made once and read-only."""
    w, h = SIZES[size]
    pats = rs.patterns(3 * w * h)
    buf = np.concatenate([rs.record(xs, i) for i, xs in enumerate(pats.values())])
    counts, escapes = spec.headers(buf, len(pats))
    for a in (buf, counts, escapes):
        a.setflags(write=False)
    return list(pats), buf, counts, escapes


def gpu_encode(core, buf, counts, escapes, policy, cap):
    """-> (forms uint32[R, 4], pos uint64[R + 1], the whole output buffer of cap bytes); guards asserted."""
    R = counts.size
    src = Guarded(buf.size, torch.uint8, data=np.array(buf))
    forms, pos, out = Guarded(4 * R, torch.int32), Guarded(R + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_runs_encode_batch(src.ptr, counts, escapes, R, policy, forms.ptr, pos.ptr, out.ptr, cap)
    core.synchronize()
    assert np.array_equal(src.get(), buf)
    return forms.get().view(np.uint32).reshape(R, 4), pos.get().view(np.uint64), out.get()


def gpu_decode(core, link, forms, cap):
    """-> (frame_pos uint64[R + 1], the whole output buffer of cap bytes); guards asserted."""
    R = forms.shape[0]
    src = Guarded(link.size, torch.uint8, data=np.array(link))
    fpos, out = Guarded(R + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_runs_decode_batch(src.ptr, forms, R, fpos.ptr, out.ptr, cap)
    core.synchronize()
    assert np.array_equal(src.get(), link)
    return fpos.get().view(np.uint64), out.get()


def check_written(got, want, pos, cap, what):
    """Record b is there, byte for byte, iff pos[b + 1] <= cap; every other byte still holds the guard."""
    written = np.zeros(cap, bool)
    for b in range(pos.size - 1):
        a, e = int(pos[b]), int(pos[b + 1])
        if e <= cap:
            written[a:e] = True
            assert got[a:e].tobytes() == want[a:e].tobytes(), f"{what} {b}"
    assert (got[~written] == GUARD).all(), f"bytes outside the {what}s that fit were written"


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("size", sorted(SIZES))
def test_both_calls_equal_the_host_forms(cores, size, policy):
    names, buf, counts, escapes = stream(size)
    w, h = SIZES[size]
    N = 3 * w * h
    wf, wp, wo = cwire_runs_encode_host(buf, counts, escapes, N, policy)
    sf, sp, so = rs.encode(buf, counts.size, policy)
    assert np.array_equal(wf, sf) and np.array_equal(wp, sp) and wo[:so.size].tobytes() == so.tobytes()
    cap = cwire_runs_bytes_max(N, counts.size, policy)
    gf, gp, go = gpu_encode(cores[size], buf, counts, escapes, policy, cap)
    bad = [names[b] for b in range(counts.size) if not np.array_equal(gf[b], wf[b])]
    assert not bad, f"forms differ for {bad}"
    assert np.array_equal(gp, wp)
    check_written(go, wo, wp, cap, "record")
    if policy == lib.RUNS_WHERE_SMALLER:
        assert {names[b] for b in range(counts.size) if wf[b][0]} >= {"whole", "run255", "run4097", "straddle", "escape_on_cut"}
        assert not wf[names.index("alternating")][0] and not wf[names.index("r3")][0]
    else:
        b = names.index("alternating")
        assert int(wp[b + 1] - wp[b]) == 12 + 3 * spec.pad4(int(counts[b]))   # r == n: 1.5x the code bytes
    # ... and back: the decoder gives the input's bytes and positions
    link = wo[:int(wp[-1])]
    fp, cw = cwire_runs_decode_host(link, wf, N)
    assert cw.tobytes() == buf.tobytes()
    gfp, gcw = gpu_decode(cores[size], link, wf, buf.size)
    assert np.array_equal(gfp, fp)
    check_written(gcw, buf, fp, buf.size, "record")


def test_no_records_writes_pos_0_only(cores):
    core = cores["small"]
    forms, pos, out = Guarded(8, torch.int32), Guarded(4, torch.int64), Guarded(64)
    torch.cuda.synchronize()
    none = np.zeros(4, np.uint32)
    core.cwire_runs_encode_batch(out.ptr, none, none, 0, 0, forms.ptr, pos.ptr, out.ptr, 64)
    core.synchronize()
    assert list(pos.get()) == [0, -3, -3, -3] and (forms.get() == -7).all() and (out.get() == GUARD).all()
    pos = Guarded(4, torch.int64)
    torch.cuda.synchronize()
    core.cwire_runs_decode_batch(out.ptr, none, 0, pos.ptr, out.ptr, 64)
    core.synchronize()
    assert list(pos.get()) == [0, -3, -3, -3] and (out.get() == GUARD).all()


@functools.lru_cache(maxsize=None)
def many():
    """130 records of mixed forms for the small core."""
    names, buf, counts, escapes = stream("small")
    pats = rs.patterns(9216)
    order = [n for n in names if n not in ("whole", "alternating")]
    recs = [rs.record(pats[order[i % len(order)]], 100 + i) for i in range(130)]
    recs[64] = rs.record(pats["whole"], 64)
    buf = np.concatenate(recs)
    counts, escapes = spec.headers(buf, 130)
    return buf, counts, escapes


@pytest.mark.parametrize("skip", [False, True])
def test_130_records_in_one_call(cores, skip):
    core = cores["small"]
    buf, counts, escapes = many()
    wf, wp, wo = cwire_runs_encode_host(buf, counts, escapes, 9216, lib.RUNS_WHERE_SMALLER)
    assert 0 < int(wf[:, 0].sum()) < 130
    cap = int(wp[65]) - 4 if skip else int(wp[-1])       # record 64 ends four bytes past the capacity
    gf, gp, go = gpu_encode(core, buf, counts, escapes, lib.RUNS_WHERE_SMALLER, cap)
    assert np.array_equal(gf, wf) and np.array_equal(gp, wp)
    check_written(go, wo, wp, cap, "record")
    link = wo[:int(wp[-1])]
    fp, _ = cwire_runs_decode_host(link, wf, 9216)
    cap = int(fp[65]) - 4 if skip else buf.size
    gfp, gcw = gpu_decode(core, link, wf, cap)
    assert np.array_equal(gfp, fp)
    check_written(gcw, buf, fp, cap, "record")


def run_record(n, e, gap, ln):
    """A record in the run form from its parts, well formed or not -> (bytes, its row of the forms table)."""
    r = len(gap)
    q = spec.pad4(r)
    g, l = np.zeros(q, np.uint8), np.zeros(q, np.uint8)
    g[:r], l[:r] = gap, ln
    d = np.zeros(spec.pad4(n), np.uint8)
    d[:n] = 9
    return np.concatenate([np.array([n, e, r], "<u4").view(np.uint8), g, l, np.full(4 * e, 1, np.uint8), d]), [1, n, e, r]


@pytest.mark.parametrize("name,n,e,gap,ln", [
    ("sum above n", 300, 0, [3, 0, 0, 7, 0], [255, 255, 255, 100, 255]),
    ("sum far above n", 5000, 0, [1] * 2000, [255] * 2000),             # two workgroups of runs, 512 000 entries claimed
    ("sum below n", 5000, 0, [3, 0], [255, 40]),
    ("more 255 gaps than e", 600, 1, [255, 255, 255], [255, 255, 87]),
])
def test_malformed_run_records_stay_inside_their_record(cores, name, n, e, gap, ln):
    """Memory safety on guarded buffers: the bad record's bytes are unspecified, everything around it is exact."""
    core = cores["small"]
    before, after = rs.record(np.arange(1, 700), 1), rs.record(np.arange(5, 9000, 3), 2)
    bad, row = run_record(n, e, gap, ln)
    ok = np.concatenate([before, after])
    c, esc = spec.headers(ok, 2)
    forms, pos, out = cwire_runs_encode_host(ok, c, esc, 9216, lib.RUNS_ALWAYS)
    link = np.concatenate([out[:int(pos[1])], bad, out[int(pos[1]):int(pos[2])]])
    table = np.array([forms[0], row, forms[1]], np.uint32)
    size = spec.frame_bytes(n, e)
    fp, cw = gpu_decode(core, link, table, ok.size + size)
    assert fp.tolist() == [0, before.size, before.size + size, ok.size + size]
    assert cw[:before.size].tobytes() == before.tobytes() and cw[before.size + size:].tobytes() == after.tobytes()
    assert cw[before.size:before.size + 8].view("<u4").tolist() == [n, e]


def test_refusals_that_need_a_core(cores):
    core = cores["small"]
    names, buf, counts, escapes = stream("small")
    R = counts.size
    src = Guarded(buf.size, torch.uint8, data=np.array(buf))
    cap = cwire_runs_bytes_max(9216, R, 1)
    forms, pos, out = Guarded(4 * R, torch.int32), Guarded(R + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()

    def enc(**kw):
        d = dict(d_cwire=src.ptr, counts=counts, escapes=escapes, nrecords=R, policy=0, d_forms=forms.ptr, d_pos=pos.ptr, d_out=out.ptr,
                 capacity_bytes=cap)
        d.update(kw)
        with pytest.raises(lib.Mi355Error) as err:
            core.cwire_runs_encode_batch(*d.values())
        assert err.value.code == lib.ERR_INVALID, kw

    big, more = counts.copy(), escapes.copy()
    big[1], more[1] = 9217, counts[1] + 1
    for kw in (dict(nrecords=-1), dict(nrecords=131, counts=np.resize(counts, 131), escapes=np.zeros(131, np.uint32)), dict(policy=2),
               dict(d_cwire=None), dict(d_forms=None), dict(d_pos=None),
               dict(d_out=None), dict(counts=big), dict(escapes=more), dict(d_cwire=src.ptr + 2), dict(d_out=out.ptr + 1),
               dict(d_forms=forms.ptr + 2), dict(d_pos=pos.ptr + 4), dict(d_out=src.ptr + 64, capacity_bytes=64),
               dict(d_pos=src.ptr + 8)):
        enc(**kw)
    table = cwire_runs_encode_host(buf, counts, escapes, 9216, 0)[0]

    def dec(**kw):
        d = dict(d_in=out.ptr, forms=table, nrecords=R, d_frame_pos=pos.ptr, d_cwire_out=src.ptr, capacity_bytes=buf.size)
        d.update(kw)
        with pytest.raises(lib.Mi355Error) as err:
            core.cwire_runs_decode_batch(*d.values())
        assert err.value.code == lib.ERR_INVALID, kw

    def row(i, v):
        t = table.copy()
        t[1, i] = v
        return t

    for kw in (dict(nrecords=-1), dict(nrecords=131, forms=np.resize(table, (131, 4))), dict(d_in=None), dict(d_frame_pos=None), dict(d_cwire_out=None),
               dict(forms=row(0, 2)), dict(forms=row(1, 9217)), dict(forms=row(2, int(table[1, 1]) + 1)),
               dict(forms=row(3, int(table[1, 1]) + 1)), dict(d_in=out.ptr + 2), dict(d_cwire_out=src.ptr + 2),
               dict(d_frame_pos=pos.ptr + 4), dict(d_cwire_out=out.ptr + 64, capacity_bytes=64)):
        dec(**kw)
    core.synchronize()
    assert (forms.get() == -7).all() and (pos.get() == -3).all() and (out.get() == GUARD).all() and np.array_equal(src.get(), buf)


def frames_of(S, T, N, seed):
    """T ticks of S streams: a still background, a block that moves (dense runs) and a little salt (scattered entries)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (S, N), dtype=np.uint8)
    out = np.empty((T, S, N), np.uint8)
    for t in range(T):
        f = base.copy()
        for s in range(S):
            a = 500 + 900 * t + 100 * s
            f[s, a:a + 2500] = rng.integers(0, 256, 2500, dtype=np.uint8)
            salt = rng.integers(0, N, 40)
            f[s, salt] ^= 0x80
        out[t] = f
    return out


def tick_records(states, frames, thr):
    """The records of one tick as the spec gives them, and the states behind it -> (buf, counts, escapes, new states)."""
    recs, new = [], states.copy()
    for s in range(states.shape[0]):
        df = frames[s].astype(np.int16) - states[s].astype(np.int16)
        xs = np.flatnonzero(np.abs(df) > thr)
        recs.append(np.frombuffer(spec.encode_frame(xs, df[xs].astype(np.uint8)), np.uint8))
        new[s, xs] = frames[s, xs]
    buf = np.concatenate(recs)
    counts, escapes = spec.headers(buf, len(recs))
    return buf, counts, escapes, new


def test_end_to_end_without_synchronisation(cores):
    """diff_multi_cwire -> encode -> decode -> apply_multi_cwire on one stream with nothing in between, three ticks of two
    streams: the receiver's states equal the sender's, and equal what applying the sender's records directly gives."""
    core = cores["small"]
    S, T, N, thr = 2, 3, 9216, 20
    frames = frames_of(S, T, N, 5)
    sender, receiver, direct = Region(S, N).put(np.zeros((S, N), np.uint8)), Region(S, N).put(np.zeros((S, N), np.uint8)), \
        Region(S, N).put(np.zeros((S, N), np.uint8))
    states = np.zeros((S, N), np.uint8)
    cap = cwire_runs_bytes_max(N, S, 0)
    packed = 0
    for t in range(T):
        buf, counts, escapes, states = tick_records(states, frames[t], thr)
        forms_want, pos_want, link_want = rs.encode(buf, S, rs.WHERE_SMALLER)
        packed += int(forms_want[:, 0].sum())
        d_frames = to_dev(frames[t].reshape(-1))
        off, fpos, cw = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
        forms, pos, link = Guarded(4 * S, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
        fpos2, cw2 = Guarded(S + 1, torch.int64), Guarded(cap)
        torch.cuda.synchronize()
        core.diff_multi_cwire_batch(d_frames, sender.ptr, S, off.ptr, fpos.ptr, cw.ptr, cap)
        core.cwire_runs_encode_batch(cw.ptr, counts, escapes, S, lib.RUNS_WHERE_SMALLER, forms.ptr, pos.ptr, link.ptr, cap)
        core.cwire_runs_decode_batch(link.ptr, forms_want, S, fpos2.ptr, cw2.ptr, cap)
        core.apply_multi_cwire_batch(cw2.ptr, counts, escapes, S, receiver.ptr)
        core.apply_multi_cwire_batch(cw.ptr, counts, escapes, S, direct.ptr)
        core.synchronize()
        assert cw.get()[:buf.size].tobytes() == buf.tobytes()
        assert np.array_equal(forms.get().view(np.uint32).reshape(S, 4), forms_want)
        assert np.array_equal(pos.get().view(np.uint64), pos_want)
        assert link.get()[:link_want.size].tobytes() == link_want.tobytes()
        assert np.array_equal(fpos2.get().view(np.uint64), fpos.get().view(np.uint64))
        assert cw2.get()[:buf.size].tobytes() == buf.tobytes()
        got = receiver.get()
        assert np.array_equal(got, direct.get()) and np.array_equal(got, sender.get()) and np.array_equal(got, states)
    assert packed > 0


def test_key_frame_is_all_runs_and_just_over_half(cores):
    core = cores["small"]
    S, N = 2, 9216
    rng = np.random.default_rng(11)
    states = rng.integers(1, 256, (S, N), dtype=np.uint8)
    states[0, 100:140] = 0                                    # a few zero bytes: gaps inside the key frame
    states[1, 5000:5300] = 0                                  # ... and an escaped one
    recs = [np.frombuffer(spec.encode_frame(np.flatnonzero(st), st[np.flatnonzero(st)]), np.uint8) for st in states]
    buf = np.concatenate(recs)
    counts, escapes = spec.headers(buf, S)
    forms_want, pos_want, link_want = rs.encode(buf, S, rs.WHERE_SMALLER)
    assert forms_want[:, 0].tolist() == [rs.FORM_RUNS] * S and int(escapes[1]) == 1
    sender, receiver = Region(S, N).put(states), Region(S, N).put(np.zeros((S, N), np.uint8))
    cap = cwire_runs_bytes_max(N, S, 0)
    mask, off, fpos, cw = Guarded(S * 1, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    forms, pos, link = Guarded(4 * S, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    fpos2, cw2 = Guarded(S + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.refresh_cwire_batch(sender.ptr, S, None, mask.ptr, off.ptr, fpos.ptr, cw.ptr, cap)
    core.cwire_runs_encode_batch(cw.ptr, counts, escapes, S, lib.RUNS_WHERE_SMALLER, forms.ptr, pos.ptr, link.ptr, cap)
    core.cwire_runs_decode_batch(link.ptr, forms_want, S, fpos2.ptr, cw2.ptr, cap)
    core.apply_multi_cwire_batch(cw2.ptr, counts, escapes, S, receiver.ptr)
    core.synchronize()
    assert cw.get()[:buf.size].tobytes() == buf.tobytes()
    assert np.array_equal(forms.get().view(np.uint32).reshape(S, 4), forms_want)
    got_pos = pos.get().view(np.uint64)
    assert np.array_equal(got_pos, pos_want)
    assert link.get()[:link_want.size].tobytes() == link_want.tobytes()
    for s in range(S):
        n, e, r = (int(v) for v in forms_want[s, 1:])
        assert int(got_pos[s + 1] - got_pos[s]) == 12 + 2 * spec.pad4(r) + 4 * e + spec.pad4(n)
    assert 0.5 < int(got_pos[-1]) / buf.size < 0.52
    assert cw2.get()[:buf.size].tobytes() == buf.tobytes()
    assert np.array_equal(receiver.get(), states) and np.array_equal(sender.get(), states)

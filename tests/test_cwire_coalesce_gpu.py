"""-m gpu: mi355_cwire_coalesce_batch / _cwire_batch -- T compact records of each of S streams (batch index b = s*T + t)
summed into ONE segment / record per stream (include/mi355diff.h, "A burst coalesced").  The reference of every comparison is
numpy: decode each input record with cwire_spec, accumulate a uint8 sum per stream, take the nonzero indices ascending, encode
with cwire_spec.  Inputs and outputs live in guarded buffers (gpu_util) that start as a non-zero pattern."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import cwire_apply_host, cwire_bytes_max, lib, synth
from gpu_util import DEV, CUDACore, Guarded, Region

pytestmark = pytest.mark.gpu


# ---- references -----------------------------------------------------------------------------------------------------------
def packed(segments):
    """[(xs, diff)] per batch index -> (offsets uint32[B + 1], xs int32, diff uint8)."""
    off = np.cumsum([0] + [len(x) for x, _ in segments]).astype(np.uint32)
    xs = np.concatenate([np.asarray(x, np.int64) for x, _ in segments] + [np.empty(0, np.int64)]).astype(np.int32)
    df = np.concatenate([np.asarray(d, np.uint8) for _, d in segments] + [np.empty(0, np.uint8)]).astype(np.uint8)
    return off, xs, df


def sums(recs, S, T, n):
    """The uint8 sum of every stream's differences per byte index: [S][n]."""
    off, xs, df = spec.decode(recs, S * T)
    acc = np.zeros((S, n), np.uint8)
    for s in range(S):
        for t in range(T):
            a, b = int(off[s * T + t]), int(off[s * T + t + 1])
            acc[s][xs[a:b]] += df[a:b]          # indices of a record are distinct; uint8 wraps
    return acc


def reference(recs, S, T, n):
    """-> (offsets uint32[S + 1], xs, diff, records, frame_pos uint64[S + 1]) of the coalesced burst."""
    acc = sums(recs, S, T, n)
    segs = [(np.flatnonzero(acc[s]), acc[s][np.flatnonzero(acc[s])]) for s in range(S)]
    off, xs, df = packed(segs)
    out, pos = spec.encode(off, xs, df)
    return off, xs, df, out, pos


@functools.lru_cache(maxsize=None)
def burst(w, h, S, T, thr=20):
    """One burst of a server core on webcam-like frames -> (bases [S][n], records, counts, escapes, the sender's states
    after the burst [S][n]); made once per shape, read-only."""
    n, B = 3 * w * h, S * T
    bases, frames = [], []
    for s in range(S):
        base, fr = synth.webcam_stream(T, w, h, seed=1 + 7 * s, device=DEV)
        bases.append(base.cpu().numpy())
        frames.extend(fr.cpu().numpy())
    cap = cwire_bytes_max(n, B)
    srv, fr = Region(S, n).put(bases), Region(B, n).put(frames)
    off, pos, cw = Guarded(B + 1, torch.int32), Guarded(B + 1, torch.int64), Guarded(cap)
    with CUDACore(w, h, max_batch=B, threshold=thr) as server:
        torch.cuda.synchronize()
        server.diff_multi_stream_cwire_batch(fr.ptr, srv.ptr, S, T, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
        server.synchronize()
    recs = cw.get()[:int(pos.get().view(np.uint64)[B])].copy()
    counts, escapes = spec.headers(recs, B)
    out = (np.stack(bases), recs, counts, escapes, srv.get(), np.stack(frames))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the two forms --------------------------------------------------------------------------------------------------------
def run_compact(core, recs, hdr, S, T, n, cap=None):
    """-> (offsets uint32[S + 1], frame_pos uint64[S + 1], the whole output buffer of cap bytes); guards asserted."""
    cap = cwire_bytes_max(n, S) if cap is None else cap
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, pos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_coalesce_cwire_batch(src.ptr, hdr[0], hdr[1], S, T, off.ptr, pos.ptr, out.ptr, cap)
    core.synchronize()
    assert np.array_equal(src.get(), recs)
    return off.get().view(np.uint32), pos.get().view(np.uint64), out.get()


def run_arrays(core, recs, hdr, S, T, n, cap=None, skew=0):
    """-> (offsets uint32[S + 1], xs, diff: the whole buffers of cap entries); guards asserted."""
    cap = S * n if cap is None else cap
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, xs, df = Guarded(S + 1, torch.int32), Guarded(cap, torch.int32), Guarded(cap, torch.uint8, skew=skew)
    torch.cuda.synchronize()
    core.cwire_coalesce_batch(src.ptr, hdr[0], hdr[1], S, T, off.ptr, xs.ptr, df.ptr, cap)
    core.synchronize()
    assert np.array_equal(src.get(), recs)
    return off.get().view(np.uint32), xs.get(), df.get()


def check_both_forms(core, recs, S, T, n, hdr=None):
    """Both forms against the numpy reference, byte for byte; nothing behind the result is written.  -> the reference."""
    hdr = spec.headers(recs, S * T) if hdr is None else hdr
    want = reference(recs, S, T, n)
    off, pos, out = run_compact(core, recs, hdr, S, T, n)
    assert np.array_equal(off, want[0]) and np.array_equal(pos, want[4])
    assert np.array_equal(out[:want[3].size], want[3])
    assert (out[want[3].size:] == 0x5C).all(), "written behind the last record"
    aoff, axs, adf = run_arrays(core, recs, hdr, S, T, n, skew=1)
    doff, dxs, ddf = spec.decode(out, S)
    tot = int(doff[S])
    assert np.array_equal(aoff, doff) and np.array_equal(axs[:tot], dxs) and np.array_equal(adf[:tot], ddf)
    assert (axs[tot:] == -7).all() and (adf[tot:] == 0x5C).all(), "written behind the last entry"
    return want


# ---- 1. bursts of a server core -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,S,T", [(33, 7, 3, 4), (64, 48, 5, 3), (640, 360, 2, 3)])
def test_oracle_bursts(w, h, S, T):
    """33x7: one partial tile, N = 693 no multiple of 4; 64x48: two whole tiles and one of 1024 bytes; 640x360: 169 tiles, the
    last one ragged."""
    n = 3 * w * h
    _, recs, counts, escapes, _, _ = burst(w, h, S, T)
    with CUDACore(w, h, max_batch=S * T) as core:
        want = check_both_forms(core, recs, S, T, n, (counts, escapes))
    assert int(want[0][S]) > 0


# ---- 2. crafted records ---------------------------------------------------------------------------------------------------
def crafted_streams(n):
    """[(what, [T records as (xs, diff)])] at N = 9216 (tiles [0, 4096), [4096, 8192), [8192, 9216)), T = 4."""
    E = ([], [])
    every = np.arange(n)
    return [
        ("+d then -d on one byte is dropped; 200 + 100 wraps to 44",
         [([10, 500, 5000], [7, 200, 1]), ([10, 500], [249, 100]), E, ([5000], [3])]),
        ("a stream that cancels completely",
         [([0, 4095, 4096, n - 1], [1, 2, 3, 4]), ([0, 4096], [255, 253]), ([4095, n - 1], [254, 252]), E]),
        ("entries at the tile edges",
         [([0, 4095, 4096, 8191, 8192, n - 1], [1, 2, 3, 4, 5, 6]), ([0, 8191], [255, 9]), E, ([4096], [1])]),
        ("gaps of exactly 254, 255 and 256 inside a tile",   # g = 254: 100 -> 355; 255: 355 -> 611; 256: 611 -> 868
         [([100, 355], [1, 1]), ([611], [1]), ([868, 869], [1, 5]), ([869], [251])]),
        ("a gap of exactly 254 across a tile edge; escaped gaps inside a tile and across an edge",
         [([4000, 4255], [1, 1]), ([8000, 8256], [2, 2]), ([3000, 4000], [3, 255]), ([7900, 8000, 8001, 8257], [1, 254, 1, 1])]),
        # -> 3000, 4255 (not 4000), 7900, 8001, 8256, 8257: 8001 -> 8256 is a gap of 254, 7900 -> 8001 of 100
        ("a gap of 255 across a tile edge", [([4090, 4346], [1, 1]), ([4090], [1]), ([4346, 4347], [1, 1]), ([4347], [255])]),
        ("a gap of 256 across a tile edge", [([4090, 4347], [1, 1]), ([5], [1]), ([5], [255]), E]),
        ("a gap across a wholly empty tile", [([4000, 8200], [1, 1]), ([5000], [9]), ([5000], [247]), E]),
        ("a first entry >= 255, in a later tile", [([300], [1]), ([300, 4500], [255, 4]), E, E]),
        ("n = 0 records in the middle of a burst", [([1, 2, 3], [1, 1, 1]), E, E, ([2, 9000], [255, 1])]),
        ("a stream of only n = 0 records", [E, E, E, E]),
        ("a dense record (n = N) plus a sparse one",
         [(every, np.where(every % 7 == 0, 3, 1)), ([0, 7, 4096, n - 1], [253, 253, 255, 255]), E, E]),
    ]


def test_crafted_records():
    w, h, T = 64, 48, 4
    n = 3 * w * h
    streams = crafted_streams(n)
    S = len(streams)
    off, xs, df = packed([seg for _, segs in streams for seg in segs])
    recs, _ = spec.encode(off, xs, df)
    woff, wxs, wdf, wrecs, wpos = reference(recs, S, T, n)
    # the cases are there: every non-trivial stream drops an entry, escapes at tile edges exist, the empty ones are empty
    boundary = 0
    for s, (what, segs) in enumerate(streams):
        entered = set(int(x) for sx, _ in segs for x in sx)
        kept = wxs[int(woff[s]):int(woff[s + 1])]
        if entered:
            assert len(kept) < len(entered), what
        if not len(kept):
            continue
        g = spec.gaps(kept)
        boundary += int(((g >= 255) & ((kept // 4096) != np.concatenate([[-1], kept[:-1] // 4096]))).sum())
    assert boundary >= 4
    names = [what for what, _ in streams]
    for what in ("a stream that cancels completely", "a stream of only n = 0 records"):
        assert wpos[names.index(what) + 1] - wpos[names.index(what)] == 8, what
    for what, want_gap in (("a gap of 255 across a tile edge", 255), ("a gap of 256 across a tile edge", 256)):
        kept = wxs[int(woff[names.index(what)]):int(woff[names.index(what) + 1])]
        assert list(spec.gaps(kept))[1:] == [want_gap] and kept[0] // 4096 != kept[1] // 4096, what
    s3 = wxs[int(woff[3]):int(woff[4])]
    assert list(s3) == [100, 355, 611, 868] and list(spec.gaps(s3)) == [100, 254, 255, 256]
    assert list(wxs[int(woff[0]):int(woff[1])]) == [500, 5000] and list(wdf[int(woff[0]):int(woff[1])]) == [44, 4]
    with CUDACore(w, h, max_batch=S * T) as core:
        check_both_forms(core, recs, S, T, n)


# ---- 3. seams -------------------------------------------------------------------------------------------------------------
def random_burst(rng, n, S, T, most=40):
    """Random sparse records; every third one repeats indices of the one before with the negated difference."""
    segs = []
    for b in range(S * T):
        cnt = 0 if b % 7 == 3 else int(rng.integers(1, most))
        x, d = np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)
        if b % 3 == 2 and b % T and len(segs[-1][0]):
            x, d = segs[-1][0], (256 - np.asarray(segs[-1][1])) % 256
            d = np.where(np.arange(len(x)) % 2 == 0, d, 1)
        segs.append((x, d))
    return packed(segs)


@pytest.mark.parametrize("S,T", [(2, 70), (130, 1)])
def test_seams(S, T):
    """T = 70: more than one ballot pass of 64 records, and 140 records are more than one table launch of 128; S = 130: more
    streams than a table launch holds."""
    w, h = 33, 7
    n = 3 * w * h
    off, xs, df = random_burst(np.random.default_rng(S), n, S, T)
    recs, _ = spec.encode(off, xs, df)
    with CUDACore(w, h, max_batch=S * T) as core:
        want = check_both_forms(core, recs, S, T, n)
    # (one record per stream cannot cancel anything: T = 1 keeps every entry, T = 70 must drop some)
    assert 0 < int(want[0][S]) and (int(want[0][S]) < int(off[S * T]) if T > 1 else int(want[0][S]) == int(off[S * T]))


# ---- 4. identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,S,T", [(33, 7, 3, 4), (64, 48, 5, 3)])
def test_one_record_per_stream_comes_back_byte_for_byte(w, h, S, T):
    n, B = 3 * w * h, S * T
    _, recs, counts, escapes, _, _ = burst(w, h, S, T)
    with CUDACore(w, h, max_batch=B) as core:
        off, pos, out = run_compact(core, recs, (counts, escapes), B, 1, n)
    assert int(pos[B]) == recs.size and np.array_equal(out[:recs.size], recs)
    assert np.array_equal(np.diff(off.astype(np.int64)), counts)


# ---- 5. loop-back and equivalence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,S,T", [(64, 48, 3, 4), (640, 360, 2, 3)])
def test_loop_back_on_one_core_and_equivalence(w, h, S, T):
    """The sender's call and the coalesce on ONE core with no synchronisation in between (the headers are those of the same
    burst made before); the coalesced records applied to the base states give the sender's states after the burst and what
    the burst client makes of the original records; at 64x48 they are the records a threshold-0 core diffs between the two."""
    n, B = 3 * w * h, S * T
    bases, recs, counts, escapes, after, frames = burst(w, h, S, T)
    cap, ocap = cwire_bytes_max(n, B), cwire_bytes_max(n, S)
    srv, fr = Region(S, n).put(bases), Region(B, n).put(frames)
    off, pos, cw = Guarded(B + 1, torch.int32), Guarded(B + 1, torch.int64), Guarded(cap)
    ooff, opos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(ocap)
    with CUDACore(w, h, max_batch=B) as core:
        torch.cuda.synchronize()
        core.diff_multi_stream_cwire_batch(fr.ptr, srv.ptr, S, T, off.ptr, pos.ptr, cw.ptr, cap, stride=fr.stride)
        core.cwire_coalesce_cwire_batch(cw.ptr, counts, escapes, S, T, ooff.ptr, opos.ptr, out.ptr, ocap)
        core.synchronize()
        assert np.array_equal(cw.get()[:recs.size], recs) and np.array_equal(srv.get(), after)
        made = out.get()
        want = reference(recs, S, T, n)
        assert np.array_equal(made[:want[3].size], want[3]) and np.array_equal(opos.get().view(np.uint64), want[4])
        ocounts, oescapes = spec.headers(made, S)          # the headers, downloaded
        one, all_ = Region(S, n).put(bases), Region(S, n).put(bases)
        torch.cuda.synchronize()
        core.apply_multi_cwire_batch(out.ptr, ocounts, oescapes, S, one.ptr, stride=one.stride)
        core.apply_multi_stream_cwire_batch(cw.ptr, counts, escapes, S, T, all_.ptr, stride=all_.stride)
        core.synchronize()
        assert np.array_equal(one.get(), after) and np.array_equal(all_.get(), after)
        # the arrays form through mi355_apply_multi_batch
        aoff, axs, adf = Guarded(S + 1, torch.int32), Guarded(S * n, torch.int32), Guarded(S * n)
        arr = Region(S, n).put(bases)
        torch.cuda.synchronize()
        core.cwire_coalesce_batch(cw.ptr, counts, escapes, S, T, aoff.ptr, axs.ptr, adf.ptr, S * n)
        core.apply_multi_batch(aoff.ptr, axs.ptr, adf.ptr, S, arr.ptr, stride=arr.stride)
        core.synchronize()
        assert np.array_equal(arr.get(), after)
    for s in range(S):                                     # the host client
        host = np.array(bases[s], np.uint8)
        sl = made[int(want[4][s]):int(want[4][s + 1])]
        assert cwire_apply_host(host, sl, 1) == sl.size and np.array_equal(host, after[s]), s
    if (w, h) == (64, 48):
        old, new = Region(S, n).put(bases), Region(S, n).put(after)
        zoff, zpos, zcw = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(ocap)
        with CUDACore(w, h, max_batch=S, threshold=0) as zero:
            torch.cuda.synchronize()
            zero.diff_multi_cwire_batch(new.ptr, old.ptr, S, zoff.ptr, zpos.ptr, zcw.ptr, ocap, stride=new.stride)
            zero.synchronize()
        assert np.array_equal(zpos.get().view(np.uint64), want[4])
        assert np.array_equal(zcw.get()[:want[3].size], want[3]) and np.array_equal(made[:want[3].size], want[3])


# ---- 6. capacity ----------------------------------------------------------------------------------------------------------
def test_capacity():
    """Compact form: a middle record that does not fit is skipped whole, the records behind it that fit under the rule
    (frame_pos[s + 1] <= capacity_bytes) are still written, nothing is written past capacity_bytes, frame_pos stays exact.
    Arrays form: entries past `capacity` are dropped, the offsets stay exact."""
    w, h, S, T = 64, 48, 5, 3
    n = 3 * w * h
    _, recs, counts, escapes, _, _ = burst(w, h, S, T)
    woff, wxs, wdf, wrecs, wpos = reference(recs, S, T, n)
    with CUDACore(w, h, max_batch=S * T) as core:
        for cap in (int(wpos[3]) - 4, int(wpos[2]), 8, 0):
            off, pos, out = run_compact(core, recs, (counts, escapes), S, T, n, cap=max(cap, 0))
            assert np.array_equal(off, woff) and np.array_equal(pos, wpos), cap
            assert out.size == cap
            for s in range(S):
                a, b = int(wpos[s]), int(wpos[s + 1])
                if b <= cap:
                    assert np.array_equal(out[a:b], wrecs[a:b]), (cap, s)
                else:
                    assert (out[a:cap] == 0x5C).all(), (cap, s, "a record that does not fit is skipped whole")
        # a capacity that a later, smaller record fits under cannot exist (positions ascend): the rule is per record all the same
        for cap in (int(woff[2]) + 5, int(woff[S]) - 1, 3, 0):
            off, xs, df = run_arrays(core, recs, (counts, escapes), S, T, n, cap=cap, skew=3)
            assert np.array_equal(off, woff), cap
            assert np.array_equal(xs, wxs[:cap]) and np.array_equal(df, wdf[:cap]), cap


# ---- 7. malformed content -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5, 6])
def test_malformed_content_under_consistent_headers(seed):
    """Random bytes where well-formed records of the same headers stood: the guards around the input span and all outputs
    stay intact, the output parses as canonical records, offsets and frame_pos agree with it."""
    w, h, S, T = 64, 48, 3, 4
    n, B = 3 * w * h, S * T
    rng = np.random.default_rng(seed)
    segs = []
    for b in range(B):
        cnt = [n, 0, 700, 64, 3000, 1][b % 6]
        segs.append((np.sort(rng.choice(n, cnt, replace=False)), rng.integers(1, 256, cnt)))
    good, gpos = spec.encode(*packed(segs))
    counts, escapes = spec.headers(good, B)
    assert int(escapes.sum()) > 0
    bad = rng.integers(0, 256, good.size, dtype=np.uint8)
    if seed == 6:                                       # many escape codes, escapes that run far past N and wrap
        bad[rng.random(good.size) < 0.3] = 255
    with CUDACore(w, h, max_batch=B) as core:
        off, pos, out = run_compact(core, bad, (counts, escapes), S, T, n)
        doff, dxs, ddf = spec.decode(out, S)
        assert np.array_equal(doff, off)
        c2, e2 = spec.headers(out, S)
        assert np.array_equal(pos, np.cumsum([0] + [spec.frame_bytes(a, b) for a, b in zip(c2, e2)]).astype(np.uint64))
        assert (out[int(pos[S]):] == 0x5C).all()
        for s in range(S):
            x = dxs[int(doff[s]):int(doff[s + 1])].astype(np.int64)
            assert (np.diff(x) > 0).all() and (x.size == 0 or (0 <= x[0] and x[-1] < n)), s
            assert (ddf[int(doff[s]):int(doff[s + 1])] != 0).all(), s
            g = spec.gaps(x)
            sl = out[int(pos[s]):int(pos[s + 1])]
            esc = sl[8 + spec.pad4(x.size):8 + spec.pad4(x.size) + 4 * int(e2[s])].view("<u4")
            assert np.array_equal(esc, g[g >= 255]), (s, "canonical: the escaped gaps are exactly those >= 255")
        aoff, axs, adf = run_arrays(core, bad, (counts, escapes), S, T, n)
        tot = int(doff[S])
        assert np.array_equal(aoff, doff) and np.array_equal(axs[:tot], dxs) and np.array_equal(adf[:tot], ddf)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, S, T = 64, 48, 2, 2
    n, B = 3 * w * h, S * T
    rng = np.random.default_rng(3)
    recs, _ = spec.encode(*packed([(np.sort(rng.choice(n, 50, replace=False)), rng.integers(1, 256, 50)) for _ in range(B)]))
    counts, escapes = spec.headers(recs, B)
    cap = cwire_bytes_max(n, S)
    # one buffer that holds the input in front and room behind it, for the overlap cases
    big = Guarded(recs.size + cap + 64, torch.uint8)
    big.t[:recs.size].copy_(torch.from_numpy(recs).to(DEV))
    src = Guarded(recs.size, torch.uint8, data=recs)
    off, pos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
    xs, df = Guarded(S * n, torch.int32), Guarded(S * n, torch.uint8)
    L = lib.load()
    c, e = counts.ctypes.data, escapes.ctypes.data
    inside = big.ptr + recs.size - 8        # 8-aligned (the records are multiples of 4 long: recs.size - 8 may be 4 mod 8)
    inside -= inside % 8
    with CUDACore(w, h, max_batch=B) as core:
        H = core._h
        torch.cuda.synchronize()

        def compact(core_=H, src_=src.ptr, c_=c, e_=e, S_=S, T_=T, off_=off.ptr, pos_=pos.ptr, out_=out.ptr, cap_=cap):
            return L.mi355_cwire_coalesce_cwire_batch(core_, src_, c_, e_, S_, T_, off_, pos_, out_, cap_)

        def arrays(core_=H, src_=src.ptr, c_=c, e_=e, S_=S, T_=T, off_=off.ptr, xs_=xs.ptr, df_=df.ptr, cap_=S * n):
            return L.mi355_cwire_coalesce_batch(core_, src_, c_, e_, S_, T_, off_, xs_, df_, cap_)

        more_e = (escapes + counts + 1).astype(np.uint32)
        more_n = np.full(B, n + 1, np.uint32)
        zero_e = np.zeros(B, np.uint32)
        cases = [
            compact(core_=None), arrays(core_=None),
            compact(S_=-1), compact(T_=-1), arrays(S_=-1), arrays(T_=-1),
            compact(S_=B + 1, T_=1), compact(S_=S, T_=T + 1), arrays(S_=1, T_=B + 1),
            compact(src_=None), compact(c_=None), compact(e_=None), compact(off_=None), compact(pos_=None), compact(out_=None),
            arrays(src_=None), arrays(c_=None), arrays(e_=None), arrays(off_=None), arrays(xs_=None), arrays(df_=None),
            compact(e_=more_e.ctypes.data), arrays(e_=more_e.ctypes.data),
            compact(c_=more_n.ctypes.data, e_=zero_e.ctypes.data), arrays(c_=more_n.ctypes.data, e_=zero_e.ctypes.data),
            compact(src_=src.ptr + 2), compact(out_=out.ptr + 2), compact(off_=off.ptr + 2), compact(pos_=pos.ptr + 4),
            arrays(src_=src.ptr + 1), arrays(off_=off.ptr + 1), arrays(xs_=xs.ptr + 2),
            # the input span [big, big + recs.size) against every output region
            compact(src_=big.ptr, out_=big.ptr + recs.size - 4), compact(src_=big.ptr, out_=big.ptr - 4, cap_=8),
            compact(src_=big.ptr, off_=big.ptr + recs.size - 4), compact(src_=big.ptr, pos_=inside),
            arrays(src_=big.ptr, xs_=big.ptr + recs.size - 4), arrays(src_=big.ptr, df_=big.ptr + recs.size - 1),
            arrays(src_=big.ptr, off_=big.ptr - 4 * S), arrays(src_=big.ptr, df_=big.ptr - 3, cap_=4),
        ]
        assert all(rc == lib.ERR_INVALID for rc in cases), cases
        core.synchronize()
        for g in (off, pos, out, xs, df):
            g.get(written=0)
        assert np.array_equal(src.get(), recs)
        h_big = big.get()
        assert np.array_equal(h_big[:recs.size], recs) and (h_big[recs.size:] == 0x5C).all()
        # nstreams * nframes == 0: offsets[0] = 0 (and frame_pos[0] = 0) and nothing else
        assert compact(S_=0) == lib.OK and arrays(T_=0) == lib.OK
        core.synchronize()
        assert off.get(written=1)[0] == 0 and pos.get(written=1)[0] == 0
        for g in (out, xs, df):
            g.get(written=0)
        # ... and the calls above left the core in order: the burst coalesces
        assert compact() == lib.OK
        core.synchronize()
        want = reference(recs, S, T, n)
        assert np.array_equal(out.get()[:want[3].size], want[3])

"""-m gpu: mi355_cwire_split_cwire_batch -- every compact record cut into pieces of at most max_bytes bytes, each a record of the
same frame (include/mi355diff.h, "Records for a datagram socket").  The reference of every comparison is the host form
mi355_cwire_split_host, which test_cwire_split_spec.py holds to the numpy statement of the rule; pieces, piece_first and piece_pos
are compared bit for bit.  Inputs and outputs live in guarded buffers (gpu_util) that start as a non-zero pattern.  The shapes
(split_spec.cases) are the smallest that reach each seam of the block walk: counts around one dword, records of escapes only,
pieces that begin below and above index 255, pieces of 252, 256 and 260 entries (a round of the walk is 256 dwords, a wave's share
of it 64), records of 65535 .. 131073 entries (a block is 65536), and 129 and 1025 records in one call (the table kernels take
128 a launch)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
import split_spec
from cudavideostream_amd import cwire_split_bytes_max, cwire_split_host, cwire_split_pieces_max, lib
from gpu_util import GUARD, CUDACore, Guarded, Region

pytestmark = pytest.mark.gpu

CASES = split_spec.cases()
POS_FILL = np.uint64(-3 & 0xFFFFFFFFFFFFFFFF)


@functools.lru_cache(maxsize=None)
def prepared(name):
    """-> (records, counts, escapes, M, the host form's (piece_first, piece_pos, out)), made once and read-only."""
    (w, h), segs, M = CASES[name]
    buf, counts, escapes = split_spec.records(segs)
    want = cwire_split_host(buf, counts, escapes, 3 * w * h, M)
    for a in (buf, counts, escapes) + want:
        a.setflags(write=False)
    return buf, counts, escapes, M, want


@pytest.fixture(scope="module")
def cores():
    with CUDACore(*split_spec.SMALL, max_batch=1025) as small, CUDACore(*split_spec.WIDE, max_batch=2) as wide:
        yield {split_spec.SMALL: small, split_spec.WIDE: wide}


def capacities(counts, escapes, M):
    return (sum(cwire_split_pieces_max(n, e, M) for n, e in zip(counts, escapes)),
            sum(cwire_split_bytes_max(n, e, M) for n, e in zip(counts, escapes)))


def run(core, buf, counts, escapes, M, piece_cap, cap):
    """-> (piece_first uint32[R + 1], piece_pos uint64[piece_cap + 1], the whole output buffer of cap bytes); guards asserted."""
    src = Guarded(buf.size, torch.uint8, data=buf)
    first, pos, out = Guarded(counts.size + 1, torch.int32), Guarded(piece_cap + 1, torch.int64), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_split_cwire_batch(src.ptr, counts, escapes, counts.size, M, first.ptr, pos.ptr, piece_cap, out.ptr, cap)
    core.synchronize()
    assert np.array_equal(src.get(), buf)
    return first.get().view(np.uint32), pos.get().view(np.uint64), out.get()


def check(got, want, piece_cap, cap):
    """The device form's outputs against the host form's at the same capacities: the tables as far as they reach, every piece
    that fits, and nothing else written."""
    (gf, gp, go), (wf, wp, wo) = got, want
    total = int(wf[-1])
    reach = min(total, piece_cap)
    assert np.array_equal(gf, wf)
    assert np.array_equal(gp[:reach + 1], wp[:reach + 1])
    assert (gp[reach + 1:] == POS_FILL).all(), "piece_pos written past min(total, piece_capacity)"
    written = np.zeros(cap, bool)
    for p in range(reach):
        a, b = int(wp[p]), int(wp[p + 1])
        if p < piece_cap and b <= cap:
            written[a:b] = True
            assert np.array_equal(go[a:b], wo[a:b]), f"piece {p}"
    assert (go[~written] == GUARD).all(), "bytes outside the pieces that fit were written"


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_identical_to_the_host_form(cores, name):
    buf, counts, escapes, M, want = prepared(name)
    piece_cap, cap = capacities(counts, escapes, M)
    got = run(cores[CASES[name][0]], buf, counts, escapes, M, piece_cap, cap)
    check(got, want, piece_cap, cap)
    total = int(want[0][-1])
    if name.startswith("block_seam"):
        n = int(counts[0])
        assert total >= -(-n // lib.CWIRE_SPLIT_BLOCK) and all(int(want[1][p + 1] - want[1][p]) <= M for p in range(total))
    if name.startswith("wave_seam"):
        lens = {int(v) for v in spec.headers(want[2], total)[0]}
        assert lens & {252, 256, 260}, lens


@pytest.mark.parametrize("name", ["wave_seam_M516", "all_escape_M64", "records_129"])
def test_capacities(cores, name):
    buf, counts, escapes, M, (wf, wp, wo) = prepared(name)
    (w, h), _, _ = CASES[name]
    total, size = int(wf[-1]), int(wp[int(wf[-1])])
    core = cores[(w, h)]
    # piece_capacity one short: the last piece is not written and piece_pos ends one entry earlier
    want = cwire_split_host(buf, counts, escapes, 3 * w * h, M, piece_capacity=total - 1, capacity_bytes=size)
    check(run(core, buf, counts, escapes, M, total - 1, size), want, total - 1, size)
    # capacity_bytes one piece short in the middle: the pieces before it are written, the tables stay exact
    mid = total // 2
    cap = int(wp[mid + 1]) - 4
    want = cwire_split_host(buf, counts, escapes, 3 * w * h, M, piece_capacity=total, capacity_bytes=cap)
    assert np.array_equal(want[1], wp[:total + 1])
    check(run(core, buf, counts, escapes, M, total, cap), want, total, cap)
    # exactly enough of both
    check(run(core, buf, counts, escapes, M, total, size), (wf, wp[:total + 1], wo[:size]), total, size)


def test_no_records_writes_the_two_heads_only(cores):
    core = cores[split_spec.SMALL]
    first, pos, out = Guarded(4, torch.int32), Guarded(4, torch.int64), Guarded(64)
    torch.cuda.synchronize()
    none = np.zeros(1, np.uint32)
    core.cwire_split_cwire_batch(out.ptr, none, none, 0, 64, first.ptr, pos.ptr, 3, out.ptr, 64)
    core.synchronize()
    assert list(first.get()) == [0, -7, -7, -7] and list(pos.get()) == [0, -3, -3, -3] and (out.get() == GUARD).all()


def test_refusals(cores):
    core = cores[split_spec.SMALL]
    buf, counts, escapes, M, (wf, wp, wo) = prepared("mixed_M64")
    total, size = int(wf[-1]), int(wp[int(wf[-1])])
    src = Guarded(buf.size + 64, torch.uint8, data=np.concatenate([buf, np.full(64, GUARD, np.uint8)]))
    first, pos, out = Guarded(2, torch.int32), Guarded(total + 1, torch.int64), Guarded(size)
    torch.cuda.synchronize()
    ok = [src.ptr, counts, escapes, 1, M, first.ptr, pos.ptr, total, out.ptr, size]

    def refused(**kw):
        names = ["d_cwire", "counts", "escapes", "nrecords", "max_bytes", "d_piece_first", "d_piece_pos", "piece_capacity",
                 "d_cwire_out", "capacity_bytes"]
        args = [kw.get(k, v) for k, v in zip(names, ok)]
        with pytest.raises(lib.Mi355Error) as err:
            core.cwire_split_cwire_batch(*args)
        assert err.value.code == lib.ERR_INVALID, kw

    for M_bad in (0, 60, 66, 65540):
        refused(max_bytes=M_bad)
    refused(nrecords=-1)
    refused(nrecords=core.max_batch + 1, counts=np.zeros(core.max_batch + 1, np.uint32), escapes=np.zeros(core.max_batch + 1, np.uint32))
    refused(d_cwire=0)
    refused(d_piece_first=0)
    refused(d_piece_pos=0)
    refused(d_cwire_out=0)
    refused(d_cwire=src.ptr + 2)
    refused(d_cwire_out=out.ptr + 2)
    refused(d_piece_first=first.ptr + 2)
    refused(d_piece_pos=pos.ptr + 4)
    refused(escapes=counts + 1)
    refused(counts=np.array([core.total + 1], np.uint32))
    refused(d_cwire_out=src.ptr + 8)                      # the input span overlapping the pieces,
    refused(d_piece_first=src.ptr + buf.size - 4)        # the piece table
    refused(d_piece_pos=src.ptr + 8)                      # and the positions
    core.synchronize()
    assert (first.get() == -7).all() and (pos.get() == -3).all() and (out.get() == GUARD).all()
    assert np.array_equal(src.get()[:buf.size], buf)


def download(core, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    lib.check(core._lib.mi355_download(core._h, out.ctypes.data, C.c_void_p(ptr), nbytes))
    return out


@pytest.mark.parametrize("mode", ["own", "callers"])
def test_chain_diff_split_apply(mode):
    """mi355_diff_multi_cwire_batch -> split -> mi355_apply_multi_stream_cwire_batch of each camera's pieces in a shuffled order,
    padded with n = 0 records to a common count, two ticks; only the downloads of the headers wait for the device.  The
    receiver's states equal the sender's."""
    w, h, S, M = 64, 48, 3, 64
    n = 3 * w * h
    rng = np.random.default_rng(11)
    bases = rng.integers(0, 256, (S, n), dtype=np.uint8)
    ticks = []
    cur = bases
    for k in range(2):
        nxt = cur.copy()
        for s in range(S):
            lo = int(rng.integers(0, n // 2))
            nxt[s, lo:lo + 600 + 300 * s] ^= 0x80                       # a dense run
            nxt[s, rng.choice(n, 20 * (s + 1), replace=False)] ^= 0x40   # and scattered bytes
        ticks.append(nxt)
        cur = nxt
    rec_cap = spec.frame_bytes(n, 0) * S
    piece_cap, cap = capacities([n] * S, [n] * S, M)   # (more than any record of the frame needs)
    with CUDACore(w, h, max_batch=64) as core, CUDACore(w, h, max_batch=512) as client:
        if mode == "callers":
            core.use_torch_stream()
        sender, receiver = Region(S, n).put(bases), Region(S, n).put(bases)
        for k in range(2):
            frames = Region(S, n).put(ticks[k])
            off, fpos, recs = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(rec_cap)
            first, pos, out = Guarded(S + 1, torch.int32), Guarded(piece_cap + 1, torch.int64), Guarded(cap)
            torch.cuda.synchronize()
            core.diff_multi_cwire_batch(frames.ptr, sender.ptr, S, off.ptr, fpos.ptr, recs.ptr, rec_cap)
            counts = np.diff(download(core, off.ptr, 4 * (S + 1)).view(np.uint32))
            sizes = np.diff(download(core, fpos.ptr, 8 * (S + 1)).view(np.uint64)).astype(np.int64)
            escapes = ((sizes - 8 - 2 * ((counts.astype(np.int64) + 3) & ~3)) // 4).astype(np.uint32)
            assert counts.min() > 0
            core.cwire_split_cwire_batch(recs.ptr, counts, escapes, S, M, first.ptr, pos.ptr, piece_cap, out.ptr, cap)
            pf = download(core, first.ptr, 4 * (S + 1)).view(np.uint32)
            pp = download(core, pos.ptr, 8 * (int(pf[S]) + 1)).view(np.uint64)
            made = download(core, out.ptr, int(pp[-1]))
            K = int(np.diff(pf).max())
            assert 4 < K and S * K <= client.max_batch
            staged, pc, pe = [], [], []
            for s in range(S):
                order = rng.permutation(np.arange(int(pf[s]), int(pf[s + 1])))
                for p in order:
                    piece = made[int(pp[p]):int(pp[p + 1])]
                    staged.append(piece)
                    pc.append(int(piece[:4].view("<u4")[0]))
                    pe.append(int(piece[4:8].view("<u4")[0]))
                for _ in range(K - order.size):
                    staged.append(np.zeros(8, np.uint8))
                    pc.append(0)
                    pe.append(0)
            stage = Guarded(sum(p.size for p in staged), torch.uint8, data=np.concatenate(staged))
            torch.cuda.synchronize()
            client.apply_multi_stream_cwire_batch(stage.ptr, np.array(pc, np.uint32), np.array(pe, np.uint32), S, K, receiver.ptr)
            client.synchronize()
            core.synchronize()
            assert np.array_equal(receiver.get(), sender.get()), k
        assert not np.array_equal(sender.get(), bases)

"""-m gpu: mi355_cwire_fec_batch and mi355_cwire_fec_repair_batch -- parity blocks over groups of the pieces the split call wrote,
and the lost pieces rebuilt from them (include/mi355diff.h, "Parity pieces for the datagram path").  The reference of every
comparison is the host form (mi355_cwire_fec_host, mi355_cwire_fec_repair_host), which test_cwire_fec_spec.py holds to the numpy
statement; fec_first, fec_len and every parity byte are compared bit for bit.  Inputs and outputs live in guarded buffers
(gpu_util) that start as a non-zero pattern.  The shapes (fec_spec.cases) are the smallest that reach each seam: records of 0
and 1 pieces, 12 pieces at group sizes around 12, members of 428 .. 524 bytes (a wave's chunk of a parity block is 64 dwords), a
20-byte member beside 1400-byte ones, 129 and 1025 records in one call, a group of 255 members in front of a short one, and a
parity block of 65536 bytes (256 chunks)."""
import functools

import numpy as np
import pytest
import torch

import fec_spec
import split_spec
from cudavideostream_amd import cwire_fec_groups_max, cwire_fec_host, cwire_fec_repair_host, cwire_split_bytes_max, cwire_split_host
from cudavideostream_amd import cwire_split_pieces_max, lib
from gpu_util import GUARD, CUDACore, Guarded

pytestmark = pytest.mark.gpu

LEN_FILL = np.uint32(-7 & 0xFFFFFFFF)


@pytest.fixture(scope="module")
def cores():
    with CUDACore(*split_spec.SMALL, max_batch=1025) as small, CUDACore(*split_spec.WIDE, max_batch=2) as wide:
        yield {split_spec.SMALL: small, split_spec.WIDE: wide}


def capacities(name, G, K, pitch=None, group_capacity=None, capacity_bytes=None, piece_capacity=None, pieces_bytes=None):
    _, _, _, _, M, first, pos, out = fec_spec.pieces(name)
    pitch = M if pitch is None else pitch
    piece_capacity = pos.size - 1 if piece_capacity is None else piece_capacity
    pieces_bytes = out.size if pieces_bytes is None else pieces_bytes
    if group_capacity is None:
        group_capacity = cwire_fec_groups_max(piece_capacity, first.size - 1, G)
    if capacity_bytes is None:
        capacity_bytes = group_capacity * K * pitch
    return pitch, group_capacity, capacity_bytes, piece_capacity, pieces_bytes


@functools.lru_cache(maxsize=None)
def host(name, G, K, **kw):
    """The host form at the capacities of `kw`, made once and read-only; what it does not write holds GUARD."""
    _, _, _, _, M, first, pos, out = fec_spec.pieces(name)
    pitch, gcap, cap, pcap, pbytes = capacities(name, G, K, **kw)
    got = cwire_fec_host(out, pbytes, first, pos, pcap, G, K, pitch, group_capacity=gcap, capacity_bytes=cap, fill=GUARD)
    for a in got:
        a.setflags(write=False)
    return got


def run(core, name, G, K, **kw):
    """-> (fec_first, fec_len, the whole parity buffer) of the device form; guards and inputs asserted."""
    _, _, _, _, M, first, pos, out = fec_spec.pieces(name)
    pitch, gcap, cap, pcap, pbytes = capacities(name, G, K, **kw)
    src = Guarded(out.size, torch.uint8, data=out)
    pf = Guarded(first.size, torch.int32, data=first.view(np.int32))
    pp = Guarded(pos.size, torch.int64, data=pos.view(np.int64))
    ff, fl, par = Guarded(first.size, torch.int32), Guarded(gcap, torch.int32), Guarded(cap)
    torch.cuda.synchronize()
    core.cwire_fec_batch(src.ptr, pbytes, pf.ptr, pp.ptr, pcap, first.size - 1, G, K, pitch, ff.ptr, fl.ptr, gcap, par.ptr, cap)
    core.synchronize()
    assert np.array_equal(src.get(), out) and np.array_equal(pf.get().view(np.uint32), first) and np.array_equal(pp.get().view(np.uint64), pos)
    return ff.get().view(np.uint32), fl.get().view(np.uint32), par.get()


def check(got, want):
    """The device form's outputs against the host form's at the same capacities: fec_first, fec_len as far as it reaches and
    untouched behind, every parity byte that fits and nothing else written."""
    (gf, gl, go), (wf, wl, wo) = got, want
    reach = min(int(wf[-1]), gl.size)
    assert np.array_equal(gf, wf)
    assert np.array_equal(gl[:reach], wl[:reach])
    assert (gl[reach:] == LEN_FILL).all(), "fec_len written past min(total groups, group_capacity)"
    assert go.shape == wo.shape and np.array_equal(go, wo), "a parity byte differs, or one outside the blocks that fit was written"


@pytest.mark.parametrize("name,G,K", fec_spec.POINTS)
def test_bit_identical_to_the_host_form(cores, name, G, K):
    want = host(name, G, K)
    check(run(cores[fec_spec.CASES[name][0]], name, G, K), want)
    _, _, _, _, M, first, pos, _ = fec_spec.pieces(name)
    if name == "long_group_M64":
        assert int(first[-1]) > 255 and int(want[0][-1]) == -(-int(first[-1]) // 255)
    if name == "long_block_M65536":
        assert int(want[1][:int(want[0][-1])].max()) > 60000
    if name.startswith("small_n"):
        assert int(want[0][-1]) == int(first[-1]) <= 1


@pytest.mark.parametrize("name,G", [("mixed_M64", 3), ("wave_seam_M516", 8)])
def test_capacities_and_void_groups(cores, name, G):
    core = cores[fec_spec.CASES[name][0]]
    _, _, _, _, M, first, pos, out = fec_spec.pieces(name)
    total = int(fec_spec.fec_first(first, G)[-1])
    longest = int(np.diff(pos.astype(np.int64)).max())
    for K in (1, 2):
        for kw in (dict(group_capacity=total - 1),                                          # one group short,
                   dict(group_capacity=total, capacity_bytes=(total // 2 + 1) * K * M - 4),  # one slot short in the middle,
                   dict(pitch=longest), dict(pitch=longest - 4),                             # the longest piece fits / its groups void,
                   dict(piece_capacity=pos.size - 2), dict(pieces_bytes=out.size - 4)):      # the last group void
            if kw.get("pitch", 64) < 64:
                continue
            want = host(name, G, K, **kw)
            check(run(core, name, G, K, **kw), want)
            if "pitch" in kw and kw["pitch"] < longest or "piece_capacity" in kw or "pieces_bytes" in kw:
                assert (want[1][:min(total, want[1].size)] == 0).any(), "a void group was meant"


def test_no_records_writes_fec_first_0_only(cores):
    core = cores[split_spec.SMALL]
    ff, fl, par, src = Guarded(4, torch.int32), Guarded(4, torch.int32), Guarded(256), Guarded(64)
    pf, pp = Guarded(4, torch.int32), Guarded(4, torch.int64)
    torch.cuda.synchronize()
    core.cwire_fec_batch(src.ptr, 64, pf.ptr, pp.ptr, 3, 0, 8, 2, 64, ff.ptr, fl.ptr, 4, par.ptr, 256)
    core.synchronize()
    assert list(ff.get()) == [0, -7, -7, -7] and (fl.get() == -7).all() and (par.get() == GUARD).all()


def test_refusals(cores):
    core = cores[split_spec.SMALL]
    _, _, _, _, M, first, pos, out = fec_spec.pieces("mixed_M64")
    G, K = 3, 2
    pitch, gcap, cap, pcap, pbytes = capacities("mixed_M64", G, K)
    src = Guarded(out.size, torch.uint8, data=out)
    pf = Guarded(first.size, torch.int32, data=first.view(np.int32))
    pp = Guarded(pos.size, torch.int64, data=pos.view(np.int64))
    ff, fl, par = Guarded(first.size, torch.int32), Guarded(gcap, torch.int32), Guarded(cap)
    torch.cuda.synchronize()
    names = ["d_pieces", "pieces_bytes", "d_piece_first", "d_piece_pos", "piece_capacity", "nrecords", "group", "nparity", "pitch",
             "d_fec_first", "d_fec_len", "group_capacity", "d_out", "capacity_bytes"]
    ok = [src.ptr, pbytes, pf.ptr, pp.ptr, pcap, 1, G, K, pitch, ff.ptr, fl.ptr, gcap, par.ptr, cap]

    def refused(**kw):
        assert set(kw) <= set(names)
        with pytest.raises(lib.Mi355Error) as err:
            core.cwire_fec_batch(*[kw.get(k, v) for k, v in zip(names, ok)])
        assert err.value.code == lib.ERR_INVALID, kw

    refused(nrecords=-1)
    refused(nrecords=core.max_batch + 1)
    for bad in (0, 256, -1):
        refused(group=bad)
    for bad in (0, 3):
        refused(nparity=bad)
    for bad in (0, 60, 66, 65540):
        refused(pitch=bad)
    for name in ("d_pieces", "d_piece_first", "d_piece_pos", "d_fec_first", "d_fec_len", "d_out"):
        refused(**{name: 0})
    for name in ("d_pieces", "d_piece_first", "d_fec_first", "d_fec_len", "d_out"):
        refused(**{name: ok[names.index(name)] + 2})
    refused(d_piece_pos=pp.ptr + 4)
    refused(d_out=src.ptr + 8)                                   # the parity blocks in the pieces,
    refused(d_fec_len=pp.ptr + 8)                                # fec_len on piece_pos,
    refused(d_fec_first=pf.ptr)                                  # fec_first on piece_first,
    refused(d_fec_len=par.ptr + 64)                              # and two outputs on each other
    refused(d_fec_first=fl.ptr)
    core.synchronize()
    assert (ff.get() == -7).all() and (fl.get() == -7).all() and (par.get() == GUARD).all()
    assert np.array_equal(src.get(), out)


@pytest.mark.parametrize("mode", ["own", "callers"])
def test_chain_split_then_parity_without_a_synchronisation(mode):
    """mi355_cwire_split_cwire_batch then mi355_cwire_fec_batch on one stream, nothing in between: the host forms' outputs."""
    n, buf, counts, escapes, M, first, pos, out = fec_spec.pieces("wave_seam_M520")
    G, K = 8, 2
    pcap = sum(cwire_split_pieces_max(c, e, M) for c, e in zip(counts, escapes))
    cap = sum(cwire_split_bytes_max(c, e, M) for c, e in zip(counts, escapes))
    gcap = cwire_fec_groups_max(pcap, counts.size, G)
    hf, hp, ho = cwire_split_host(buf, counts, escapes, n, M, piece_capacity=pcap, capacity_bytes=cap)
    total = int(hf[-1])
    # (the host parity form reads piece_pos[p + 1] of the pieces that exist only: the device wrote no more of the table)
    want = cwire_fec_host(ho, cap, hf, hp, pcap, G, K, M, group_capacity=gcap, capacity_bytes=gcap * K * M, fill=GUARD)
    with CUDACore(*split_spec.SMALL, max_batch=4) as core:
        if mode == "callers":
            core.use_torch_stream()
        src = Guarded(buf.size, torch.uint8, data=buf)
        pf, pp, pieces = Guarded(counts.size + 1, torch.int32), Guarded(pcap + 1, torch.int64), Guarded(cap)
        ff, fl, par = Guarded(counts.size + 1, torch.int32), Guarded(gcap, torch.int32), Guarded(gcap * K * M)
        torch.cuda.synchronize()
        core.cwire_split_cwire_batch(src.ptr, counts, escapes, counts.size, M, pf.ptr, pp.ptr, pcap, pieces.ptr, cap)
        core.cwire_fec_batch(pieces.ptr, cap, pf.ptr, pp.ptr, pcap, counts.size, G, K, M, ff.ptr, fl.ptr, gcap, par.ptr, gcap * K * M)
        core.synchronize()
        assert np.array_equal(pf.get().view(np.uint32), first) and np.array_equal(pp.get().view(np.uint64)[:total + 1], pos)
        check((ff.get().view(np.uint32), fl.get().view(np.uint32), par.get()), want)
        groups = int(want[0][-1])
        assert groups == sum(-(-int(c) // G) for c in np.diff(first.astype(np.int64))) >= 2 and (want[1][:groups] > 0).all()


# ---- repair ----------------------------------------------------------------------------------------------------------------
def losses(m):
    """(lost slots, P present, Q present): nothing lost, every single slot with either or both parity blocks, the three pairs."""
    yield (), True, True
    for a in range(m):
        yield (a,), True, True
        yield (a,), True, False
        yield (a,), False, True
    if m >= 2:
        for pair in sorted({(0, 1), (0, m - 1), (m - 2, m - 1)}):
            if pair[0] < pair[1]:
                yield pair, True, True


@functools.lru_cache(maxsize=None)
def repair_jobs():
    """-> (rx bytes, [(slot offsets or None, slot lengths, P offset or None, Q offset or None, fec_len)], [the host form's
    (blocks, verdicts)]): groups of 1, 2, 11 and 255 members with every class of loss, and damaged survivors."""
    rx, jobs, at = [], [], 0

    def put(block):
        nonlocal at
        rx.append(np.asarray(block, np.uint8))
        at += block.size
        return at - block.size

    def group(name, G, g, which=None, damage=None):
        _, _, _, _, M, first, pos, out = fec_spec.pieces(name)
        blocks = [out[int(pos[p]):int(pos[p + 1])].copy() for p in fec_spec.members(first, G, 0, g)]
        _, fl, par = host(name, G, 2)
        L = int(fl[g])
        P, Q = par[2 * g * M:2 * g * M + L], par[(2 * g + 1) * M:(2 * g + 1) * M + L]
        if damage is not None:
            blocks[damage[0]][damage[1]] ^= 0x10
        offs, po, qo = [put(b) for b in blocks], put(P), put(Q)
        for lost, hp, hq in (losses(len(blocks)) if which is None else which):
            jobs.append(([None if i in lost else o for i, o in enumerate(offs)], [b.size for b in blocks], po if hp else None,
                         qo if hq else None, L, [None if i in lost else b for i, b in enumerate(blocks)], P if hp else None, Q if hq else None))
        return blocks

    group("mixed_M64", 1, 0)
    group("mixed_M64", 2, 1)
    group("mixed_M64", 11, 0)
    few = [((0,), True, False), ((254,), False, True), ((0, 1), True, True), ((0, 254), True, True), ((253, 254), True, True), ((), True, True)]
    assert len(group("long_group_M64", 255, 0, which=few)) == 255
    # the short last piece of a block lost and the last word of a long survivor damaged (BAD_TAIL), or its header's n (BAD_HEADER)
    _, _, _, _, _, first, pos, _ = fec_spec.pieces("block_seam_n65537")
    sizes = [int(pos[p + 1] - pos[p]) for p in fec_spec.members(first, 8, 0, 11)]
    short, longer = int(np.argmin(sizes)), int(np.argmax(sizes))
    one = [((short,), True, False), ((short,), False, True)]
    group("block_seam_n65537", 8, 11, which=one, damage=(longer, sizes[longer] - 1))
    group("block_seam_n65537", 8, 11, which=one[:1], damage=(longer, 3))
    want = [cwire_fec_repair_host(slots, p, q, L) for _, _, _, _, L, slots, p, q in jobs]
    return np.concatenate(rx), [j[:5] for j in jobs], want


def test_repair_equals_the_host_form(cores):
    core = cores[split_spec.SMALL]
    rx, jobs, want = repair_jobs()
    njobs = len(jobs)
    assert njobs > 3 * 8 and sum(len(j[0]) for j in jobs) > 4 * 256, "more jobs and more slots than one launch takes were meant"
    pitch = max(j[4] for j in jobs)
    A = lib.FEC_ABSENT
    job_first = np.cumsum([0] + [len(j[0]) for j in jobs]).astype(np.uint32)
    slot_off = np.array([A if o is None else o for j in jobs for o in j[0]], np.uint64)
    slot_len = np.array([n for j in jobs for n in j[1]], np.uint32)
    parity_off = np.array([[A if j[2] is None else j[2], A if j[3] is None else j[3]] for j in jobs], np.uint64)
    fec_len = np.array([j[4] for j in jobs], np.uint32)
    d_rx, d_out, d_vd = Guarded(rx.size, torch.uint8, data=rx), Guarded(2 * njobs * pitch), Guarded(2 * njobs, torch.int32)
    torch.cuda.synchronize()
    core.cwire_fec_repair_batch(d_rx.ptr, rx.size, njobs, job_first, slot_off, slot_len, parity_off, fec_len, d_out.ptr, pitch, d_vd.ptr)
    core.synchronize()
    assert np.array_equal(d_rx.get(), rx)
    got, verdicts = d_out.get(), d_vd.get().view(np.uint32).reshape(njobs, 2)
    expect, seen = np.full(2 * njobs * pitch, GUARD, np.uint8), set()
    for j, (blocks, vd) in enumerate(want):
        for k, b in enumerate(blocks):
            expect[(2 * j + k) * pitch:(2 * j + k) * pitch + b.size] = b
        assert list(verdicts[j]) == list(vd) + [0] * (2 - len(vd)), (j, verdicts[j], vd)
        seen |= {int(v) for v in vd}
    assert np.array_equal(got, expect), "a rebuilt byte differs, or one outside the rebuilt blocks was written"
    assert {0, lib.FEC_BAD_TAIL} <= seen and any(v & lib.FEC_BAD_HEADER for v in seen)


def test_repair_refusals(cores):
    core = cores[split_spec.SMALL]
    A = lib.FEC_ABSENT
    rx = Guarded(512, torch.uint8, data=(np.arange(512) % 251).astype(np.uint8))
    out, vd = Guarded(4 * 64), Guarded(4, torch.int32)
    torch.cuda.synchronize()
    names = ["d_rx", "rx_bytes", "njobs", "job_first", "slot_off", "slot_len", "parity_off", "fec_len", "d_out", "pitch", "d_verdict"]
    # two jobs of three slots of 64, 64 and 32 bytes; the first lost in each; P at 384, Q at 448
    ok = [rx.ptr, 512, 2, [0, 3, 6], [A, 64, 128, A, 192, 256], [64, 64, 32, 64, 64, 32], [[384, A], [384, 448]], [64, 64], out.ptr, 64, vd.ptr]

    def refused(**kw):
        assert set(kw) <= set(names)
        with pytest.raises(lib.Mi355Error) as err:
            core.cwire_fec_repair_batch(*[kw.get(k, v) for k, v in zip(names, ok)])
        assert err.value.code == lib.ERR_INVALID, kw

    refused(njobs=-1)
    refused(njobs=core.max_batch + 1, job_first=np.zeros(core.max_batch + 2, np.uint32), parity_off=np.zeros(2 * core.max_batch + 2, np.uint64),
            fec_len=np.zeros(core.max_batch + 1, np.uint32))
    refused(job_first=[0, 0, 3], slot_off=[A, 192, 256])                              # a job of no members,
    refused(job_first=[0, 3, 259], slot_off=[A, 64, 128] + [A] + [0] * 255, slot_len=[64] * 259)   # of 256,
    refused(job_first=[0, 3, 2])                                                       # the table running backwards
    refused(fec_len=[64, 0])
    refused(fec_len=[64, 62])
    refused(slot_len=[64, 64, 32, 64, 0, 32])
    refused(slot_len=[64, 64, 30, 64, 64, 32])
    refused(slot_len=[64, 68, 32, 64, 64, 32])                                         # a survivor longer than fec_len
    refused(parity_off=[[A, A], [384, 448]])                                           # one lost, no parity
    refused(slot_off=[A, A, 128, A, 192, 256])                                         # two lost, P only
    refused(slot_off=[A, 64, 128, A, A, A])                                            # three lost
    refused(slot_off=[A, 66, 128, A, 192, 256])                                        # a misaligned slot,
    refused(parity_off=[[386, A], [384, 448]])                                         # a misaligned parity block,
    refused(slot_off=[A, 64, 128, A, 192, 484])                                        # a slot reaching past rx_bytes,
    refused(parity_off=[[384, A], [384, 452]])                                         # a parity block reaching past it
    refused(rx_bytes=508)
    refused(pitch=60)                                                                  # fec_len above pitch
    refused(pitch=66, d_out=out.ptr)
    for name in ("d_rx", "d_out", "d_verdict"):
        refused(**{name: 0})
        refused(**{name: ok[names.index(name)] + 2})
    refused(d_out=rx.ptr + 256)                                                        # the rebuilt blocks in d_rx,
    refused(d_verdict=rx.ptr)                                                          # the verdicts in d_rx,
    refused(d_verdict=out.ptr + 128)                                                   # and in the rebuilt blocks
    core.synchronize()
    assert (out.get() == GUARD).all() and (vd.get() == -7).all()
    core.cwire_fec_repair_batch(*ok)
    core.cwire_fec_repair_batch(rx.ptr, 512, 0, [0], [], [], [], [], out.ptr, 64, vd.ptr)   # no jobs: nothing
    core.synchronize()
    h = rx.get()
    got = out.get().reshape(4, 64)
    assert np.array_equal(got[0], h[384:448] ^ h[64:128] ^ np.concatenate([h[128:160], np.zeros(32, np.uint8)]))
    assert (got[1] == GUARD).all() and (got[3] == GUARD).all() and (vd.get()[[1, 3]] == 0).all()

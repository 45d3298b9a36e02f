"""-m gpu: mi355_cwire_fec_batch and mi355_cwire_fec_repair_batch past the counts at which their kernels take another step, lane,
launch or address bit (csrc/stream_ops.hip: k_fec_make, k_fec_repair; csrc/core.hip: the repair's launch packing):
    A  the grid      k_fec_make's waves stride over min(groups, group_capacity) << shift items.  grid_case: 2 * waves + 1 items and
                     more at shift 0 (pitch 64), 8 (pitch 65536) and 3 (pitch 1400, chunk indices 6 and 7 dead), so every wave takes
                     two items and some three; a void group and a chunk past L in front of a live item of the same wave, a group
                     without room behind one; group_capacity one below the groups there are
    B  the members   one record of 8446 pieces of 64 bytes at G = 63, 64, 65, 128, 129 and 255: the lane loop's second to fourth
                     steps and the 4-member batches at every remainder; at G = 255 each of the six ways a member can be malformed at
                     slots 0, 63, 64 and 254 of a group
    C  the repair    two lost at fec_len 8, 1024, 1028, 2048 and 65536 (the 256-thread loop's passes); each verdict pair of the two
                     rebuilt blocks of a two-lost job, the damage on the first dword that has to be zero and on the one before;
                     fec_len 4; launches that end exactly at 256 slots and at 8 jobs
    D  past 2^32     pieces, parity blocks, received blocks and rebuilt blocks at byte offsets above 2^32

The tables are written by hand (the call takes any piece_first and piece_pos; include/mi355diff.h, "Void groups", says what a
malformed member is), the piece bytes are seeded random.  The reference of every comparison is the host form at the same capacities
(for the far layouts: on the same pieces, every position rebased to a small buffer), bit for bit, in guarded buffers that start as
a non-zero pattern.  Every builder asserts, from the tables and the numpy statement (fec_spec) alone, that its input reaches the
seam it is named for; test_fec_seams_host.py runs every builder without a GPU, with the 8192 waves of a 256-CU device, and holds
the host forms to fec_spec.reference and fec_spec.repair on every builder's input.

What a contiguous position table cannot hold, and what the builders do instead (each asserted where it is built):
  * a start that is no multiple of 4 makes the length of the piece before it no multiple of 4 (and the other way round): those two
    kinds come as a pair of neighbouring members of one group, the named one at the named slot; only piece 0 can be alone
  * a piece that ends above pieces_bytes is followed by one that ends above it too or runs backwards: at slot 254 the follower is
    slot 0 of the next group, so that one call has two void groups, not one
  * the slots of the parity blocks rise with the group, so no group behind one without room has room: the live items of that case
    come before the skipped ones of their waves, not behind them
  * two windows 4 GiB apart are joined by a piece longer than the pitch or one that runs backwards: no group that is not void has
    members from both windows; the records do"""
import contextlib
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cwire_spec as spec
import fec_spec
from cudavideostream_amd import cwire_fec_groups_max, cwire_fec_host, cwire_fec_repair_host, lib
from gpu_util import GUARD, BigGuarded, CUDACore, FarRegion, Guarded

pytestmark = pytest.mark.gpu

LEN_FILL = np.uint32(-7 & 0xFFFFFFFF)
CHUNK = 64               # dwords of an item: kFecChunk
WAVES_PER_CU = 32        # core.hip launches cu_count * 8 workgroups of 4 waves
REPAIR_JOBS, REPAIR_SLOTS, REPAIR_THREADS = 8, 256, 256   # kFecRepairJobs, kFecRepairSlots, k_fec_repair's workgroup
T32 = 1 << 32
FAR_N, FAR_STRIDE = 4096, T32 - 1024     # two windows: [0, 4096) and [2^32 - 1024, 2^32 + 3072)
LIVE, DEAD_CHUNK, VOID, PAST_L, NO_ROOM = range(5)   # what k_fec_make does with an item, in the order it decides


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@contextlib.contextmanager
def budget(seconds=5.0):
    """The device part of a test, drained, within `seconds`."""
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    took = time.perf_counter() - t0
    assert took < seconds, f"{took:.2f} s on the device, {seconds} s allowed"


def device_waves():
    return WAVES_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def core():
    with CUDACore(64, 48, max_batch=64) as c:
        yield c


# ---- cases of the parity call -----------------------------------------------------------------------------------------------
def make(pieces, first, pos, G, K, pitch, group_capacity=None, capacity_bytes=None, piece_capacity=None, pieces_bytes=None):
    """A call on hand-written tables and the host form's result at its capacities, read-only."""
    pieces, first, pos = np.asarray(pieces, np.uint8), np.asarray(first, np.uint32), np.asarray(pos, np.uint64)
    pcap = pos.size - 1 if piece_capacity is None else piece_capacity
    pbytes = pieces.size if pieces_bytes is None else pieces_bytes
    gcap = cwire_fec_groups_max(pcap, first.size - 1, G) if group_capacity is None else group_capacity
    cap = gcap * K * pitch if capacity_bytes is None else capacity_bytes
    assert int(first[-1]) <= pos.size - 1, "the position table holds every piece"
    want = cwire_fec_host(pieces, pbytes, first, pos, pcap, G, K, pitch, group_capacity=gcap, capacity_bytes=cap, fill=GUARD)
    frozen(pieces, first, pos, *want)
    return SimpleNamespace(pieces=pieces, first=first, pos=pos, G=G, K=K, pitch=pitch, gcap=gcap, cap=cap, pcap=pcap, pbytes=pbytes,
                           want=want)


def member_lens(pos, pcap, pbytes, pitch):
    """fec_spec.member_len of every piece of the table at once (int64; 0: absent or malformed)."""
    p = np.asarray(pos).astype(np.int64)
    a, b = p[:-1], p[1:]
    ok = (np.arange(a.size) < pcap) & (b <= pbytes) & (b > a) & (a % 4 == 0) & ((b - a) % 4 == 0) & (b - a <= pitch)
    return np.where(ok, b - a, 0)


def group_lens(first, pos, pcap, pbytes, pitch, G):
    """L of every group from the tables alone (0: void) -> int64[groups]."""
    lens = member_lens(pos, pcap, pbytes, pitch)
    ff = fec_spec.fec_first(first, G).astype(np.int64)
    gid = np.concatenate([ff[r] + np.arange(int(first[r + 1]) - int(first[r])) // G for r in range(len(first) - 1)] + [np.empty(0, np.int64)])
    mine = lens[int(first[0]):int(first[-1])]
    L, low = np.zeros(int(ff[-1]), np.int64), np.full(int(ff[-1]), 1 << 40, np.int64)
    np.maximum.at(L, gid.astype(np.int64), mine)
    np.minimum.at(low, gid.astype(np.int64), mine)
    return np.where(low == 0, 0, L)


def items_of(c):
    """(shift, what k_fec_make does with each of its items) from the tables and the capacities."""
    L = group_lens(c.first, c.pos, c.pcap, c.pbytes, c.pitch, c.G)
    ng = min(L.size, c.gcap)
    cpp = -(-(c.pitch // 4) // CHUNK)
    shift = (cpp - 1).bit_length()
    assert 1 << shift >= cpp and (shift == 0 or 1 << (shift - 1) < cpp)
    g, chunk = np.repeat(np.arange(ng), 1 << shift), np.tile(np.arange(1 << shift), ng)
    what = np.full(ng << shift, LIVE)
    what[(g + 1) * c.K * c.pitch > c.cap] = NO_ROOM
    what[chunk * CHUNK * 4 >= L[g]] = PAST_L
    what[L[g] == 0] = VOID
    what[chunk >= cpp] = DEAD_CHUNK
    return shift, what


def same_wave(what, waves, before, behind):
    """The first item that is `before` whose wave's next item is `behind` (None: there is none)."""
    hit = np.flatnonzero((what[:-waves] == before) & (what[waves:] == behind)) if what.size > waves else np.empty(0, np.int64)
    if not hit.size:
        return None
    lo, hi = int(hit[0]), int(hit[0]) + waves
    assert lo % waves == hi % waves and hi > lo
    return lo, hi


def run(core, c):
    """-> (fec_first, fec_len, the whole parity buffer) of the device form; guards and inputs asserted."""
    nrec = c.first.size - 1
    src = Guarded(c.pieces.size, torch.uint8, data=c.pieces)
    pf = Guarded(c.first.size, torch.int32, data=c.first.view(np.int32))
    pp = Guarded(c.pos.size, torch.int64, data=c.pos.view(np.int64))
    ff, fl, par = Guarded(c.first.size, torch.int32), Guarded(c.gcap, torch.int32), Guarded(c.cap)
    torch.cuda.synchronize()
    core.cwire_fec_batch(src.ptr, c.pbytes, pf.ptr, pp.ptr, c.pcap, nrec, c.G, c.K, c.pitch, ff.ptr, fl.ptr, c.gcap, par.ptr, c.cap)
    core.synchronize()
    assert np.array_equal(src.get(), c.pieces) and np.array_equal(pf.get().view(np.uint32), c.first)
    assert np.array_equal(pp.get().view(np.uint64), c.pos)
    return ff.get().view(np.uint32), fl.get().view(np.uint32), par.get()


def check(got, want):
    """The device form's outputs against the host form's at the same capacities: fec_first, fec_len as far as it reaches and
    untouched behind, every parity byte that fits and nothing else written."""
    (gf, gl, go), (wf, wl, wo) = got, want
    reach = min(int(wf[-1]), gl.size)
    assert np.array_equal(gf, wf)
    assert np.array_equal(gl[:reach], wl[:reach]), f"fec_len: group {int(np.argmax(gl[:reach] != wl[:reach]))} is the first that differs"
    assert (gl[reach:] == LEN_FILL).all(), "fec_len written past min(total groups, group_capacity)"
    assert go.shape == wo.shape
    if not np.array_equal(go, wo):
        at = int(np.argmax(go != wo))
        raise AssertionError(f"parity byte {at} is {go[at]}, the host form's {wo[at]}")


# ---- A. the grid and its skipped items -----------------------------------------------------------------------------------------
GRID_LONG = (8, 252, 256, 260, 32768, 65532, 65536)
GRID_POINTS = [(which, K, cut) for which in (1, 2, 3) for K in (1, 2) for cut in ((None,) if which == 2 else (None, "void", "room", "groups"))]


@functools.lru_cache(maxsize=None)
def grid_case(which, waves, K, cut=None):
    """2 * waves + 1 items and more: 1: shift 0 (pitch 64, G 1, pieces of 20 .. 64 bytes in four records, one of them empty);
    2: shift 8 (pitch 65536, G 1, lengths of GRID_LONG: chunks past L between live ones of a wave); 3: shift 3 (pitch 1400, G 2,
    three records whose last group is short: chunk indices 6 and 7 are dead).  cut: "void" a zero-length piece in group 5, "room"
    capacity_bytes 4 bytes short of the middle group's end, "groups" group_capacity one below the groups there are."""
    rng = np.random.default_rng(1000 * which + 7)
    need = 2 * waves + 1
    if which == 1:
        G, pitch, n = 1, 64, need
        lens = 4 * rng.integers(5, 17, n)
        counts = [n // 3, 0, n // 3 + 1, n - 2 * (n // 3) - 1]
    elif which == 2:
        G, pitch, n = 1, 65536, -(-need // 256)
        lens = np.array(GRID_LONG)[rng.integers(0, len(GRID_LONG), n)]
        lens[:len(GRID_LONG)] = GRID_LONG
        counts = [n]
    else:
        G, pitch, groups = 2, 1400, -(-need // 8)
        per = [groups // 3, groups // 3, groups - 2 * (groups // 3)]
        counts = [2 * g - 1 for g in per]
        n = sum(counts)
        lens = 4 * rng.integers(5, 351, n)
    void_group = 5
    if cut == "void":
        lens[void_group * G] = 0
    first = np.concatenate([[0], np.cumsum(counts)])
    pos = np.concatenate([[0], np.cumsum(lens)])
    pieces = rng.integers(1, 256, int(pos[-1]), dtype=np.uint8)
    total = int(fec_spec.fec_first(first, G)[-1])
    kw = {}
    if cut == "room":
        kw = dict(group_capacity=total, capacity_bytes=(total // 2 + 1) * K * pitch - 4)
    if cut == "groups":
        kw = dict(group_capacity=total - 1)
    c = make(pieces, first, pos, G, K, pitch, **kw)
    c.shift, c.what = items_of(c)
    c.waves, c.items = waves, c.what.size
    wf, wl, wo = c.want
    assert c.shift == {1: 0, 2: 8, 3: 3}[which] and pieces.size < 4 << 20
    assert total == (n if G == 1 else groups) and c.items == min(total, c.gcap) << c.shift
    assert c.items >= (need if cut != "groups" else 2 * waves), "every wave takes two items"
    if cut != "groups":
        assert c.items > 2 * waves, "and some a third"
    if which == 1:
        assert 0 in np.diff(first) and lens.min() >= (0 if cut == "void" else 20) and lens.max() == 64
    if which == 2:
        assert set(lens.tolist()) == set(GRID_LONG)
        assert same_wave(c.what, waves, PAST_L, LIVE) and same_wave(c.what, waves, LIVE, PAST_L), "dead chunks between live ones"
    if which == 3:
        assert all(int(n_) % 2 for n_ in counts), "the last group of each record is short"
        assert (c.what.reshape(-1, 8)[:, 6:] == DEAD_CHUNK).all() and (c.what.reshape(-1, 8)[:, :6] != DEAD_CHUNK).all()
        assert cut == "room" or same_wave(c.what, waves, PAST_L, LIVE)
    if cut is None:
        assert VOID not in c.what and NO_ROOM not in c.what
    if cut == "void":
        lo, hi = void_group << c.shift, (void_group << c.shift) + waves
        assert lo < waves and c.what[lo] == VOID and c.what[hi] == LIVE and lo % waves == hi % waves
        assert int(wl[void_group]) == 0 and (wl[:total] == 0).sum() == 1
    if cut == "room":
        gm = total // 2
        assert (c.what[:gm << c.shift] != NO_ROOM).all() and same_wave(c.what, waves, LIVE, NO_ROOM)
        assert (c.what[gm << c.shift:] != LIVE).all(), "the slots rise with the group: nothing behind the middle group has room"
        assert (wl[gm:total] > 0).all(), "fec_len is written for the groups without room"
        assert (wo[:gm * K * pitch].reshape(gm, K, pitch)[:, :, :20] != GUARD).any(axis=2).all(), "the reference writes every group in front"
        assert (wo[gm * K * pitch:] == GUARD).all()
    if cut == "groups":
        assert c.gcap == total - 1 and wl.size == total - 1 and (wl > 0).all()
    return c


@pytest.mark.parametrize("which,K,cut", GRID_POINTS)
def test_grid_stride_takes_further_steps(core, which, K, cut):
    waves = device_waves()
    c = grid_case(which, waves, K, cut)
    print(f"grid_case({which}, K={K}, cut={cut}): {c.items} items on {waves} waves ({waves // WAVES_PER_CU} CUs), shift {c.shift}")
    with budget():
        got = run(core, c)
    check(got, c.want)


# ---- B. the member loop and the void rule ---------------------------------------------------------------------------------------
MEMBER_PIECES, MEMBER_BYTES = 8191 + 255, 64
MEMBER_G = (63, 64, 65, 128, 129, 255)
KINDS = ("zero", "backwards", "start", "length", "long", "past")
SLOTS = (0, 63, 64, 254)
MALFORMED_GROUP = 7     # the group of the malformed member, but for the kinds that at slot 0 only piece 0 can show alone


@functools.lru_cache(maxsize=None)
def member_rows():
    rows = np.random.default_rng(8446).integers(1, 256, (MEMBER_PIECES, MEMBER_BYTES), dtype=np.uint8)
    return frozen(rows)[0]


@functools.lru_cache(maxsize=None)
def member_case(G, K):
    """One record of 8446 pieces of 64 bytes at pitch 64, well-formed."""
    c = make(member_rows().ravel(), [0, MEMBER_PIECES], MEMBER_BYTES * np.arange(MEMBER_PIECES + 1), G, K, MEMBER_BYTES)
    wf, wl, _ = c.want
    total = -(-MEMBER_PIECES // G)
    assert int(wf[-1]) == total and (wl[:total] == 64).all()
    steps = -(-G // 64)                       # of the lane loop i = lane, lane + 64, ...
    assert steps == {63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 255: 4}[G]
    return c


@functools.lru_cache(maxsize=None)
def malformed_case(kind, slot):
    """member_case(255, 2) with the member at `slot` of a group malformed in the way `kind`; every other piece holds the bytes it
    has there, wherever the table puts them -> (the case, the group, the malformed members, the void groups)."""
    N, B, G = MEMBER_PIECES, MEMBER_BYTES, 255
    rows = member_rows()
    g = 0 if slot == 0 and kind in ("start", "backwards") else MALFORMED_GROUP
    p = g * G + slot
    q = np.arange(N + 1)
    pos, bad, pbytes = B * q, {p}, None
    if kind == "zero":
        pos = np.where(q <= p, B * q, B * (q - 1))
    elif kind == "backwards":   # the pieces in front of p high, the pieces behind it low
        pos = np.where(q <= p, B * (N - p) + B * q, B * (q - p - 1))
    elif kind == "start":
        pos = pos.copy()
        pos[p] += 2
        bad = {p} if p == 0 else {p - 1, p}
    elif kind == "length":
        pos = pos.copy()
        if slot == 254:             # (slot 255 is another group: the piece in front pays)
            pos[p] += 2
            bad = {p - 1, p}
        else:
            pos[p + 1] -= 2
            bad = {p, p + 1}
    elif kind == "long":
        pos = np.where(q <= p, B * q, B * q + 4)
    elif kind == "past":            # p the last 64 bytes of a buffer that ends 4 bytes sooner; the piece behind it runs backwards
        pos = np.where(q <= p, B * (N - p + q), B * (q - p - 2))
        pos[p + 1] = B * N + B
        pbytes, bad = B * N + B - 4, {p, p + 1}
    lens = member_lens(pos, N, B * N + 2 * B if pbytes is None else pbytes, B)
    size = int(max(pos.max(), B * N)) if pbytes is None else pbytes + 4
    buf = np.random.default_rng(slot + 1000 * KINDS.index(kind)).integers(1, 256, size, dtype=np.uint8)
    for i in np.flatnonzero(lens):
        buf[int(pos[i]):int(pos[i + 1])] = rows[i][:lens[i]]
    c = make(buf, [0, N], pos, G, 2, B, pieces_bytes=pbytes)
    lens = member_lens(c.pos, c.pcap, c.pbytes, B)
    assert set(np.flatnonzero(lens == 0).tolist()) == bad and p in bad and (lens[sorted(set(range(N)) - bad)] == B).all()
    a, b = int(c.pos[p]), int(c.pos[p + 1])
    assert {"zero": b == a, "backwards": b < a, "start": a % 4 != 0, "length": (b - a) % 4 != 0 and 0 < b - a < B, "long": b - a == B + 4,
            "past": b == c.pbytes + 4 and b - a == B}[kind]
    if len(bad) == 1:
        assert all(fec_spec.member_len(c.pos, c.pcap, c.pbytes, B, i) == B for i in (p - 1, p + 1) if 0 <= i < N)
    void = sorted({i // G for i in bad})
    assert void == ([g, g + 1] if (kind, slot) == ("past", 254) else [g]) and p // G == g and p % G == slot
    L = group_lens(c.first, c.pos, c.pcap, c.pbytes, B, G)
    assert list(np.flatnonzero(L == 0)) == void and list(np.flatnonzero(c.want[1][:L.size] == 0)) == void, "the reference's void groups"
    return c, g, bad, void


@pytest.mark.parametrize("K", (1, 2))
@pytest.mark.parametrize("G", MEMBER_G)
def test_member_loop_at_every_count(core, G, K):
    c = member_case(G, K)
    with budget():
        got = run(core, c)
    check(got, c.want)


@pytest.mark.parametrize("slot", SLOTS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_malformed_member_voids_its_group_alone(core, kind, slot):
    c, g, bad, void = malformed_case(kind, slot)
    well = member_case(255, 2).want
    with budget():
        got = run(core, c)
    check(got, c.want)
    gf, gl, go = got
    blocks, ref = go.reshape(-1, 2 * MEMBER_BYTES), well[2].reshape(-1, 2 * MEMBER_BYTES)
    total = int(gf[-1])
    for v in void:
        assert gl[v] == 0 and (blocks[v] == GUARD).all(), "a void group: fec_len 0 and no parity byte"
    rest = [i for i in range(total) if i not in void]
    assert {g - 1, void[-1] + 1} & set(rest) and np.array_equal(gl[rest], well[1][rest])
    assert np.array_equal(blocks[rest], ref[rest]), "the other groups are those of the well-formed run"


# ---- C. repair -------------------------------------------------------------------------------------------------------------------
A = lib.FEC_ABSENT


def repair_case(groups, pitch):
    """groups: [(the members' blocks in slot order, the lost slots, P present, Q present, damage)]; damage: None or (slot, byte,
    xor) applied to a survivor after the parity was made (fec_spec.parity).  -> the arrays of one call, what each job hands to the
    host form, and the host form's answers."""
    rx, at, jobs, args = [], 0, [], []

    def put(block):
        nonlocal at
        rx.append(np.asarray(block, np.uint8))
        at += block.size
        return at - block.size

    for blocks, lost, hp, hq, damage in groups:
        L, (P, Q) = fec_spec.parity(blocks, 2)
        blocks = [b.copy() for b in blocks]
        if damage is not None:
            assert damage[0] not in lost and damage[1] < blocks[damage[0]].size
            blocks[damage[0]][damage[1]] ^= damage[2]
        offs = [A if i in lost else put(b) for i, b in enumerate(blocks)]
        jobs.append((offs, [b.size for b in blocks], put(P) if hp else A, put(Q) if hq else A, L))
        args.append(([None if i in lost else b for i, b in enumerate(blocks)], P if hp else None, Q if hq else None, L))
    want = [cwire_fec_repair_host(*a) for a in args]
    c = SimpleNamespace(rx=np.concatenate(rx), njobs=len(jobs), pitch=pitch, args=args, want=want,
                        job_first=np.cumsum([0] + [len(j[0]) for j in jobs]).astype(np.uint32),
                        slot_off=np.array([o for j in jobs for o in j[0]], np.uint64),
                        slot_len=np.array([n for j in jobs for n in j[1]], np.uint32),
                        parity_off=np.array([[j[2], j[3]] for j in jobs], np.uint64), fec_len=np.array([j[4] for j in jobs], np.uint32))
    assert max(j[4] for j in jobs) <= pitch
    return c


def launches(members):
    """The jobs of each launch of one call: a launch takes REPAIR_JOBS jobs and REPAIR_SLOTS slots at the most."""
    out, slots = [[]], 0
    for j, m in enumerate(members):
        if len(out[-1]) == REPAIR_JOBS or slots + m > REPAIR_SLOTS:
            out.append([])
            slots = 0
        out[-1].append(j)
        slots += m
    return out


def run_repair(core, c):
    """One call on guarded buffers; every rebuilt byte, every byte that is not one, and every verdict against the host form."""
    d_rx = Guarded(c.rx.size, torch.uint8, data=c.rx)
    d_out, d_vd = Guarded(2 * c.njobs * c.pitch), Guarded(2 * c.njobs, torch.int32)
    torch.cuda.synchronize()
    core.cwire_fec_repair_batch(d_rx.ptr, c.rx.size, c.njobs, c.job_first, c.slot_off, c.slot_len, c.parity_off, c.fec_len, d_out.ptr,
                                c.pitch, d_vd.ptr)
    core.synchronize()
    assert np.array_equal(d_rx.get(), c.rx)
    check_repair(d_out.get(), d_vd.get().view(np.uint32).reshape(c.njobs, 2), c)


def check_repair(got, verdicts, c):
    expect = np.full(2 * c.njobs * c.pitch, GUARD, np.uint8)
    for j, (blocks, vd) in enumerate(c.want):
        for k, b in enumerate(blocks):
            expect[(2 * j + k) * c.pitch:(2 * j + k) * c.pitch + b.size] = b
        assert list(verdicts[j]) == list(vd) + [0] * (2 - len(vd)), (j, list(verdicts[j]), list(vd))
    if not np.array_equal(got, expect):
        at = int(np.argmax(got != expect))
        raise AssertionError(f"byte {at % c.pitch} of block {at // c.pitch} is {got[at]}, the host form's {expect[at]}")


TWO_LOST_LENS = (8, 1024, 1028, 2048, 65536)


@functools.lru_cache(maxsize=None)
def two_lost():
    """A job of two lost members per fec_len of TWO_LOST_LENS: the workgroup's loop over dwords takes one partial pass, exactly one,
    one and a dword, exactly two and 64; every survivor is shorter than fec_len, one ends inside the second pass."""
    rng = np.random.default_rng(2048)
    groups = []
    for L in TWO_LOST_LENS:
        survivors = [max(4, L - 4), max(4, L // 8 * 4), 4] + ([1500] if L >= 2048 else [])
        lens = [L, survivors[0], survivors[1], max(4, L // 16 * 4)] + survivors[2:]
        lost = (0, 3)
        blocks = [rng.integers(1, 256, m, dtype=np.uint8) for m in lens]
        assert all(b.size % 4 == 0 and b.size < L for i, b in enumerate(blocks) if i not in lost) and blocks[0].size == L
        assert L < 2048 or any(4 * REPAIR_THREADS < b.size < 8 * REPAIR_THREADS for i, b in enumerate(blocks) if i not in lost)
        groups.append((blocks, lost, True, True, None))
    c = repair_case(groups, 65536)
    passes = [-(-(L // 4) // REPAIR_THREADS) for L in TWO_LOST_LENS]
    assert passes == [1, 1, 2, 2, 64] and all(len(w[0]) == 2 for w in c.want)
    return c


def record_block(rng, n, e, size):
    """A block that reads as a record {n, e}: its header, a body without a zero byte, nothing behind."""
    assert spec.frame_bytes(n, e) == size
    return np.concatenate([np.array([n, e], "<u4").view(np.uint8), rng.integers(1, 256, size - 8, dtype=np.uint8)])


VERDICT_PAIRS = ((0, 0), (lib.FEC_BAD_TAIL, 0), (0, lib.FEC_BAD_TAIL), (lib.FEC_BAD_TAIL, lib.FEC_BAD_TAIL), (0, lib.FEC_BAD_HEADER))


@functools.lru_cache(maxsize=None)
def verdict_pairs():
    """Two-lost jobs whose rebuilt blocks are records of 1024 and 1504 bytes in blocks of fec_len 2048, in both orders, a survivor
    damaged in one byte: on the first dword that has to be zero of the shorter and of the longer record (flagged), on the dwords
    before them (not flagged), and on the header's e so that only the second block is BAD_HEADER.  One byte of a survivor changes
    that byte of both rebuilt blocks (by two non-zero factors), so which of them is flagged is decided by where their tails begin.
    -> (the case, the expected verdict pair of each job)."""
    rng = np.random.default_rng(1504)
    L = 2048
    short = lambda: record_block(rng, 500, 4, 1024)     # its tail begins at byte 1024: the second pass of the workgroup
    long_ = lambda: record_block(rng, 748, 0, 1504)
    assert 1024 == 4 * REPAIR_THREADS
    survivor = lambda: rng.integers(1, 256, L, dtype=np.uint8)
    TAIL, HEADER = lib.FEC_BAD_TAIL, lib.FEC_BAD_HEADER
    groups, expect = [], []
    for first, second, flagged in ((short, long_, 0), (long_, short, 1)):
        for byte, pair in ((1024, {flagged: TAIL}), (1020, {}), (1504, {0: TAIL, 1: TAIL}), (1500, {flagged: TAIL})):
            groups.append(([survivor(), first(), survivor(), second()], (1, 3), True, True, (2, byte, 0x10)))
            expect.append((pair.get(0, 0), pair.get(1, 0)))
    # e of the first block grows and stays within n and fec_len; e of the second leaves fec_len: the xor is searched in the numpy statement
    blocks = [survivor(), short(), survivor(), long_()]
    found = None
    for x in range(1, 256):
        _, (P, Q) = fec_spec.parity(blocks, 2)
        hit = blocks[2].copy()
        hit[4] ^= x
        if fec_spec.repair([blocks[0], None, hit, None], P, Q, L)[1] == [0, HEADER]:
            found = x
            break
    assert found is not None
    groups.append((blocks, (1, 3), True, True, (2, 4, found)))
    expect.append((0, HEADER))
    c = repair_case(groups, L)
    for a, pair in zip(c.args, expect):
        assert tuple(fec_spec.repair(*a)[1]) == pair, "the numpy statement's verdicts"
    assert set(expect) == set(VERDICT_PAIRS), "each verdict pair is there"
    return c, expect


@functools.lru_cache(maxsize=None)
def four_bytes():
    """fec_len 4: one lost with P, one lost with Q, and two lost (fec_plan takes that too): no header fits, BAD_HEADER alone."""
    rng = np.random.default_rng(4)
    blocks = [rng.integers(1, 256, 4, dtype=np.uint8) for _ in range(3)]
    c = repair_case([(blocks, (0,), True, False, None), (blocks, (1,), False, True, None), (blocks, (0, 2), True, True, None)], 64)
    assert [list(w[1]) for w in c.want] == [[1], [1], [1, 1]] and all(b.size == 4 for w in c.want for b in w[0])
    assert np.array_equal(c.want[0][0][0], blocks[0]) and np.array_equal(c.want[1][0][0], blocks[1])
    return c


PACKINGS = {"255_1": (255, 1), "255_2": (255, 2), "128_128_1": (128, 128, 1), "nine_of_1": (1,) * 9, "eight_of_32_and_one": (32,) * 8 + (5,)}


@functools.lru_cache(maxsize=None)
def packing(name):
    """One call whose jobs have the member counts PACKINGS[name], of the pieces of member_rows; job j loses slot (7 j + 3) mod its
    members, with P or with Q in turn, so every job reads its own slots' offsets and lengths."""
    members = PACKINGS[name]
    rows, at, groups = member_rows(), 0, []
    for j, m in enumerate(members):
        blocks = [rows[at + i][:MEMBER_BYTES - 4 * ((i + j) % 3)] for i in range(m)]
        at += m
        groups.append((blocks, ((7 * j + 3) % m,), j % 2 == 0, j % 2 == 1, None))
    c = repair_case(groups, MEMBER_BYTES)
    want = {"255_1": [[0, 1]], "255_2": [[0], [1]], "128_128_1": [[0, 1], [2]], "nine_of_1": [list(range(8)), [8]],
            "eight_of_32_and_one": [list(range(8)), [8]]}[name]
    assert launches(members) == want
    if name in ("255_1", "eight_of_32_and_one"):
        assert sum(members[:len(want[0])]) == REPAIR_SLOTS, "the first launch is full to the slot"
    lost = [int(np.flatnonzero(c.slot_off[c.job_first[j]:c.job_first[j + 1]] == A)[0]) for j in range(c.njobs)]
    assert len(set(lost)) == len(lost) or name == "nine_of_1"
    return c


def test_repair_two_lost_at_every_pass_count(core):
    c = two_lost()
    with budget():
        run_repair(core, c)


def test_repair_verdicts_of_each_block(core):
    c, expect = verdict_pairs()
    with budget():
        run_repair(core, c)
    assert [tuple(int(v) for v in w[1]) for w in c.want] == expect and set(expect) == set(VERDICT_PAIRS)


def test_repair_fec_len_4(core):
    c = four_bytes()
    with budget():
        run_repair(core, c)


@pytest.mark.parametrize("name", sorted(PACKINGS))
def test_repair_launch_packing(core, name):
    c = packing(name)
    with budget():
        run_repair(core, c)


# ---- D. past 2^32 ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def far_memory(need):
    """Skips only when the device reports less free memory than `need` plus 1 GiB; empties torch's cache on the way out."""
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip(f"{need} bytes needed (plus 2^30 of headroom), {free} bytes free")
    try:
        yield
    finally:
        torch.cuda.empty_cache()


def near(x):
    """A position of the far layout in the small buffer: the window at 2^32 - 1024 begins at 7168."""
    return x if x < FAR_N else x - T32 + 8192


@functools.lru_cache(maxsize=None)
def far_pieces():
    """Pieces in two windows 4 GiB apart at G 3, K 2, pitch 1400 -> (piece_first, the far piece_pos, pieces_bytes, the windows'
    rows, the case of the same pieces with every position rebased to a buffer of 11264 bytes)."""
    T = T32
    records = [[(0, 1400), (1400, 1420), (1420, 2020)],                           # the near window,
               [(2020, T + 2744)],                                                # 2^32 + 724 bytes: void, and 724 in 32 bits
               [(T + 2744, T + 3072)],                                            # wholly above 2^32
               [(T + 3072, T - 1024)],                                            # backwards: void
               [(T - 1024, T - 300), (T - 300, T + 400), (T + 400, T + 1400)],    # one piece from below 2^32 to above it
               [(T + 1400, T - 200)],                                             # backwards: void
               [(T - 200, T), (T, T + 1000), (T + 1000, T + 2400), (T + 2400, T + 3072)]]   # one piece from 2^32 itself
    flat = [p for r in records for p in r]
    assert all(a[1] == b[0] for a, b in zip(flat, flat[1:]))
    first = np.cumsum([0] + [len(r) for r in records])
    pos = np.array([p[0] for p in flat] + [flat[-1][1]], np.uint64)
    pbytes = FAR_STRIDE + FAR_N
    assert pbytes == T + 3072 == int(pos[-1])
    small = np.random.default_rng(32).integers(1, 256, 11264, dtype=np.uint8)
    c = make(small, first, [near(int(x)) for x in pos], 3, 2, 1400)
    rows = np.stack([small[:FAR_N], small[7168:]])
    lens = member_lens(pos, pos.size - 1, pbytes, 1400)
    assert np.array_equal(lens, member_lens(c.pos, c.pcap, c.pbytes, 1400)), "rebasing keeps every length and every void member"
    assert list(np.flatnonzero(lens == 0)) == [3, 5, 9] and int(pos[4] - pos[3]) % T == 724
    assert any(a < T < b for a, b in flat) and any(a == T < b for a, b in flat) and sum(T < a < b for a, b in flat) >= 3
    L = group_lens(first, pos, pos.size - 1, pbytes, 1400, 3)
    assert list(L) == [1400, 0, 328, 0, 1000, 0, 1400, 672] and np.array_equal(c.want[1][:8], L)
    return frozen(first.astype(np.uint32))[0], frozen(pos)[0], pbytes, rows, c


def test_far_pieces(core):
    first, pos, pbytes, rows, c = far_pieces()
    with far_memory(FarRegion.bytes_needed(2, FAR_N, FAR_STRIDE)), budget(10.0):
        src = FarRegion(2, FAR_N, FAR_STRIDE).put(rows)
        try:
            pf = Guarded(first.size, torch.int32, data=first.view(np.int32))
            pp = Guarded(pos.size, torch.int64, data=pos.view(np.int64))
            ff, fl, par = Guarded(first.size, torch.int32), Guarded(c.gcap, torch.int32), Guarded(c.cap)
            torch.cuda.synchronize()
            core.cwire_fec_batch(src.ptr, pbytes, pf.ptr, pp.ptr, c.pcap, first.size - 1, 3, 2, 1400, ff.ptr, fl.ptr, c.gcap, par.ptr, c.cap)
            core.synchronize()
            assert np.array_equal(src.get(), rows), "the pieces"
            assert np.array_equal(pf.get().view(np.uint32), first) and np.array_equal(pp.get().view(np.uint64), pos)
            check((ff.get().view(np.uint32), fl.get().view(np.uint32), par.get()), c.want)
        finally:
            src.free()


FAR_GROUPS = {0: 65536, 32767: 8, 32768: 1400, 32769: 65536, 32770: 260}
FAR_OUT_PIECES, FAR_OUT_PITCH = 32771, 65536


@functools.lru_cache(maxsize=None)
def far_parity():
    """One record of 32771 pieces at G 1, K 2, pitch 65536, all of them empty (void groups) but five: the slot of group 32768 begins
    at 2^32 -> (the case of the five pieces alone, piece_pos of all, the whole fec_len)."""
    lens = np.zeros(FAR_OUT_PIECES, np.int64)
    for g, n in FAR_GROUPS.items():
        lens[g] = n
    pos = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    pieces = np.random.default_rng(32768).integers(1, 256, int(pos[-1]), dtype=np.uint8)
    five = make(pieces, [0, 5], np.concatenate([[0], np.cumsum(list(FAR_GROUPS.values()))]), 1, 2, FAR_OUT_PITCH)
    flen = group_lens([0, FAR_OUT_PIECES], pos, FAR_OUT_PIECES, pieces.size, FAR_OUT_PITCH, 1)
    assert np.array_equal(flen, lens) and list(five.want[1][:5]) == list(FAR_GROUPS.values())
    assert 32768 * 2 * FAR_OUT_PITCH == T32 and 32767 * 2 * FAR_OUT_PITCH + FAR_OUT_PITCH < T32
    return five, frozen(pos)[0], frozen(flen.astype(np.uint32))[0]


def guard_outside(big, written):
    """Every byte of a BigGuarded of bytes outside the [a, b) of `written` (offsets into the buffer) holds GUARD: on the device."""
    big.check()
    at = 0
    for a, b in sorted(written) + [(big.count, big.count)]:
        for lo in range(at, a, BigGuarded.PIECE):
            piece = big.t[lo:min(lo + BigGuarded.PIECE, a)]
            if bool((piece != GUARD).any()):
                raise AssertionError(f"byte {lo + int(torch.argmax((piece != GUARD).to(torch.uint8)))} was written: no block has it")
        at = max(at, b)


def test_far_parity_blocks(core):
    five, pos, flen = far_parity()
    cap = FAR_OUT_PIECES * 2 * FAR_OUT_PITCH
    gcap = FAR_OUT_PIECES + 1
    with far_memory(BigGuarded.bytes_needed(cap)), budget(10.0):
        out = BigGuarded(cap)
        try:
            src = Guarded(five.pieces.size, torch.uint8, data=five.pieces)
            pf = Guarded(2, torch.int32, data=np.array([0, FAR_OUT_PIECES], np.int32))
            pp = Guarded(pos.size, torch.int64, data=pos.view(np.int64))
            for cut in (cap, 32770 * 2 * FAR_OUT_PITCH - 4):
                ff, fl = Guarded(2, torch.int32), Guarded(gcap, torch.int32)
                torch.cuda.synchronize()
                core.cwire_fec_batch(src.ptr, five.pieces.size, pf.ptr, pp.ptr, FAR_OUT_PIECES, 1, 1, 2, FAR_OUT_PITCH, ff.ptr, fl.ptr, gcap,
                                     out.ptr, cut)
                core.synchronize()
                assert list(ff.get().view(np.uint32)) == [0, FAR_OUT_PIECES]
                got = fl.get().view(np.uint32)
                assert np.array_equal(got[:FAR_OUT_PIECES], flen) and got[FAR_OUT_PIECES] == LEN_FILL, "fec_len, in full"
                written = []
                for i, (g, L) in enumerate(FAR_GROUPS.items()):
                    if (g + 1) * 2 * FAR_OUT_PITCH > cut:
                        continue
                    for k in range(2):
                        a, ref = (2 * g + k) * FAR_OUT_PITCH, (2 * i + k) * FAR_OUT_PITCH
                        assert np.array_equal(out.t[a:a + L].cpu().numpy(), five.want[2][ref:ref + L]), f"block {k} of group {g}"
                        written.append((a, a + L))
                assert len(written) == (10 if cut == cap else 6), "the groups 32769 and 32770 have no room in the second call"
                guard_outside(out, written)
                for a, b in written:
                    out.t[a:b].fill_(GUARD)
            assert np.array_equal(src.get(), five.pieces) and np.array_equal(pp.get().view(np.uint64), pos)
        finally:
            out.free()


@functools.lru_cache(maxsize=None)
def far_repair():
    """A group of five members of up to 600 bytes, its survivors below, across and above byte 2^32 of rx and its parity blocks
    above, repaired in the modes 1, 2 and 3 -> (the windows' rows, rx_bytes, the case; its offsets are the far ones)."""
    rng = np.random.default_rng(600)
    blocks = [rng.integers(1, 256, n, dtype=np.uint8) for n in (600, 600, 596, 600, 400)]
    L, (P, Q) = fec_spec.parity(blocks, 2)
    where = {0: 0, 4: 1024, 1: T32 - 300, 2: T32 + 300, "P": T32 + 896, "Q": T32 + 1496}
    rows = np.random.default_rng(601).integers(1, 256, (2, FAR_N), dtype=np.uint8)
    for key, at in where.items():
        b = P if key == "P" else Q if key == "Q" else blocks[key]
        w, o = (0, at) if at < FAR_N else (1, at - FAR_STRIDE)
        assert 0 <= o and o + b.size <= FAR_N and at % 4 == 0
        rows[w, o:o + b.size] = b
    assert where[1] < T32 < where[1] + 600 and where[0] + 600 < T32 < where[2] and where["P"] > T32
    jobs = [((3,), True, False), ((3,), False, True), ((3, 4), True, True)]
    args = [([None if i in lost else b for i, b in enumerate(blocks)], P if hp else None, Q if hq else None, L) for lost, hp, hq in jobs]
    c = SimpleNamespace(njobs=3, pitch=600, args=args, want=[cwire_fec_repair_host(*a) for a in args],
                        job_first=np.array([0, 5, 10, 15], np.uint32),
                        slot_off=np.array([A if i in lost else where[i] for lost, _, _ in jobs for i in range(5)], np.uint64),
                        slot_len=np.array([b.size for _ in jobs for b in blocks], np.uint32),
                        parity_off=np.array([[where["P"] if hp else A, where["Q"] if hq else A] for _, hp, hq in jobs], np.uint64),
                        fec_len=np.array([L] * 3, np.uint32))
    assert L == 600 and [len(w[0]) for w in c.want] == [1, 1, 2]
    assert np.array_equal(c.want[0][0][0], blocks[3]) and np.array_equal(c.want[2][0][1], np.concatenate([blocks[4], np.zeros(200, np.uint8)]))
    return frozen(rows)[0], FAR_STRIDE + FAR_N, c


def test_far_repair_input(core):
    rows, rx_bytes, c = far_repair()
    with far_memory(FarRegion.bytes_needed(2, FAR_N, FAR_STRIDE)), budget(10.0):
        rx = FarRegion(2, FAR_N, FAR_STRIDE).put(rows)
        try:
            d_out, d_vd = Guarded(2 * c.njobs * c.pitch), Guarded(2 * c.njobs, torch.int32)
            torch.cuda.synchronize()
            call = lambda off: core.cwire_fec_repair_batch(rx.ptr, rx_bytes, c.njobs, c.job_first, off, c.slot_len, c.parity_off, c.fec_len,
                                                           d_out.ptr, c.pitch, d_vd.ptr)
            past = c.slot_off.copy()
            past[2] = rx_bytes - int(c.slot_len[2]) + 4     # ends 4 bytes behind rx_bytes, from above 2^32
            assert int(past[2]) > T32 and int(past[2]) % 4 == 0
            with pytest.raises(lib.Mi355Error) as err:
                call(past)
            assert err.value.code == lib.ERR_INVALID
            core.synchronize()
            assert (d_out.get() == GUARD).all() and (d_vd.get() == -7).all(), "a refused call writes nothing"
            past[2] -= 4                                    # (to the byte: taken; the survivor read there is another block)
            call(past)
            call(c.slot_off)
            core.synchronize()
            assert np.array_equal(rx.get(), rows)
            check_repair(d_out.get(), d_vd.get().view(np.uint32).reshape(c.njobs, 2), c)
        finally:
            rx.free()


FAR_JOBS, FAR_JOB_SEAM = 32770, (0, 32767, 32768, 32769)


@functools.lru_cache(maxsize=None)
def far_jobs():
    """32770 jobs on one group of two members of 8 bytes, slot 0 lost and P there, at pitch 65536: block 0 of job 32768 begins at
    byte 2^32 of the output -> (rx, the arrays of the call, the rebuilt block, its verdict)."""
    rng = np.random.default_rng(32770)
    blocks = [rng.integers(1, 256, 8, dtype=np.uint8) for _ in range(2)]
    _, (P, _) = fec_spec.parity(blocks, 2)
    (rebuilt,), (vd,) = cwire_fec_repair_host([None, blocks[1]], P, None, 8)
    assert np.array_equal(rebuilt, blocks[0]) and 2 * 32768 * FAR_OUT_PITCH == T32
    c = SimpleNamespace(rx=np.concatenate([blocks[1], P]), job_first=2 * np.arange(FAR_JOBS + 1, dtype=np.uint32),
                        slot_off=np.tile(np.array([A, 0], np.uint64), FAR_JOBS), slot_len=np.full(2 * FAR_JOBS, 8, np.uint32),
                        parity_off=np.tile(np.array([8, A], np.uint64), FAR_JOBS), fec_len=np.full(FAR_JOBS, 8, np.uint32),
                        args=([None, blocks[1]], P, None, 8))
    return c, rebuilt, int(vd)


def test_far_repair_output():
    c, rebuilt, vd = far_jobs()
    count = 2 * FAR_JOBS * FAR_OUT_PITCH
    with far_memory(BigGuarded.bytes_needed(count)), CUDACore(8, 8, max_batch=FAR_JOBS) as core, budget(10.0):
        out = BigGuarded(count)
        try:
            d_rx, d_vd = Guarded(16, torch.uint8, data=c.rx), Guarded(2 * FAR_JOBS, torch.int32)
            torch.cuda.synchronize()
            core.cwire_fec_repair_batch(d_rx.ptr, 16, FAR_JOBS, c.job_first, c.slot_off, c.slot_len, c.parity_off, c.fec_len, out.ptr,
                                        FAR_OUT_PITCH, d_vd.ptr)
            core.synchronize()
            verdicts = d_vd.get().view(np.uint32).reshape(FAR_JOBS, 2)
            for j in FAR_JOB_SEAM:
                at = 2 * j * FAR_OUT_PITCH
                assert np.array_equal(out.t[at:at + 8].cpu().numpy(), rebuilt) and list(verdicts[j]) == [vd, 0], f"job {j}"
            assert (verdicts == [vd, 0]).all()
            out.check()
            view = out.t.view(FAR_JOBS, 2, FAR_OUT_PITCH)
            want = torch.from_numpy(rebuilt).to(view.device)
            for j in range(0, FAR_JOBS, 4096):      # a strided view of 4096 jobs at a time: nothing crosses to the host
                part = view[j:j + 4096]
                assert bool((part[:, 1, :] == GUARD).all()), f"an odd block of the jobs from {j} was written"
                assert bool((part[:, 0, 8:] == GUARD).all()), f"an even block of the jobs from {j} was written behind byte 8"
                assert bool((part[:, 0, :8] == want).all()), f"a rebuilt block of the jobs from {j} differs"
            assert np.array_equal(d_rx.get(), c.rx)
        finally:
            out.free()

"""CPU: mi355_cwire_fec_host and mi355_cwire_fec_repair_host, the definitions of the parity pieces (include/mi355diff.h, "Parity
pieces for the datagram path"), against the numpy statement (fec_spec, GF(2^8) through log / exp tables) on every case, and the
laws of the header: Horner's rule equals the definition of Q, a group of one member is its own parity, fec_first depends on
piece_first alone, every loss of at most K of a group's datagrams is rebuilt byte for byte, rebuilt pieces are canonical and
apply with the survivors in any order to the record's state, the repair works on the 8-byte prefix, and a damaged survivor shows
in the verdict."""
import numpy as np
import pytest

import cwire_spec as spec
import fec_spec
from cudavideostream_amd import (cwire_apply_host, cwire_check_host, cwire_fec_groups_max, cwire_fec_host, cwire_fec_repair_host,
                                 cwire_split_host, lib)

FILL = 0x5C


def host(name, G, K, pitch=None, **caps):
    _, _, _, _, M, first, pos, out = fec_spec.pieces(name)
    return cwire_fec_host(out, caps.pop("pieces_bytes", out.size), first, pos, caps.pop("piece_capacity", pos.size - 1), G, K,
                          M if pitch is None else pitch, fill=FILL, **caps)


def model(name, G, K, pitch=None, group_capacity=None, capacity_bytes=None, piece_capacity=None, pieces_bytes=None):
    _, _, _, _, M, first, pos, out = fec_spec.pieces(name)
    pitch = M if pitch is None else pitch
    piece_capacity = pos.size - 1 if piece_capacity is None else piece_capacity
    if group_capacity is None:
        group_capacity = fec_spec.groups_max(piece_capacity, first.size - 1, G)
    if capacity_bytes is None:
        capacity_bytes = group_capacity * K * pitch
    return fec_spec.reference(out, out.size if pieces_bytes is None else pieces_bytes, first, pos, piece_capacity, G, K, pitch,
                              group_capacity, capacity_bytes, FILL)


def same(got, want):
    for g, w, what in zip(got, want, ("fec_first", "fec_len", "the parity blocks")):
        assert g.shape == w.shape and np.array_equal(g, w), what


@pytest.mark.parametrize("name,G,K", fec_spec.POINTS)
def test_host_form_equals_the_model(name, G, K):
    same(host(name, G, K), model(name, G, K))


def test_the_split_host_form_makes_the_same_pieces():
    """The cases' pieces come from split_spec.reference; the GPU tests take them from the host form of the split call."""
    for name in ("mixed_M64", "wave_seam_M520"):
        n, buf, counts, escapes, M, first, pos, out = fec_spec.pieces(name)
        hf, hp, ho = cwire_split_host(buf, counts, escapes, n, M)
        total = int(first[-1])
        assert np.array_equal(hf, first) and np.array_equal(hp[:total + 1], pos) and np.array_equal(ho[:out.size], out)


@pytest.mark.parametrize("name,G", [("mixed_M64", 3), ("wave_seam_M516", 8)])
def test_capacities_and_void_groups_equal_the_model(name, G):
    _, _, _, _, M, first, pos, out = fec_spec.pieces(name)
    total = int(fec_spec.fec_first(first, G)[-1])
    longest = int(np.diff(pos.astype(np.int64)).max())
    for K in (1, 2):
        for kw in (dict(group_capacity=total - 1), dict(group_capacity=total, capacity_bytes=(total // 2 + 1) * K * M - 4),
                   dict(pitch=longest), dict(pitch=longest - 4), dict(piece_capacity=pos.size - 2), dict(pieces_bytes=out.size - 4)):
            if kw.get("pitch", 64) < 64:
                continue
            got, want = host(name, G, K, **dict(kw)), model(name, G, K, **kw)
            same(got, want)
            if "pitch" in kw and kw["pitch"] < longest or "piece_capacity" in kw or "pieces_bytes" in kw:
                assert (want[1][:total] == 0).any(), "a void group was meant"


def test_malformed_tables_give_void_groups():
    """Positions that run backwards, are not multiples of 4, or give an empty piece: each voids its group and nothing else."""
    pieces = np.arange(256, dtype=np.uint8)
    first = np.array([0, 8], np.uint32)
    good = np.arange(0, 257, 32).astype(np.uint64)   # eight pieces of 32 bytes
    for at, value in ((3, 200), (3, 98), (5, 128)):
        pos = good.copy()
        pos[at] = value
        got = cwire_fec_host(pieces, 256, first, pos, 8, 2, 2, 64, fill=FILL)
        want = fec_spec.reference(pieces, 256, first, pos, 8, 2, 2, 64, fec_spec.groups_max(8, 1, 2), fec_spec.groups_max(8, 1, 2) * 128, FILL)
        same(got, want)
        assert sorted(np.flatnonzero(got[1][:4] == 0)) in ([1], [1, 2], [2]), got[1]


def test_horner_equals_the_definition():
    """Q = XOR of 2^i * D_i (tables) equals xtime(Q) ^ D_i from the last slot down on packed dwords, for every slot count."""
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, (255, 64), dtype=np.uint8)
    for m in (1, 2, 3, 8, 64, 254, 255):
        q = np.zeros(16, np.uint32)
        for i in range(m - 1, -1, -1):
            q = fec_spec.xtime(q) ^ data[i].view("<u4")
        want = np.bitwise_xor.reduce([fec_spec.gf_mul(data[i], int(fec_spec.EXP[i])) for i in range(m)], axis=0)
        assert np.array_equal(q.view(np.uint8), want), m


def test_a_group_of_one_member_is_its_own_parity():
    _, _, _, _, M, first, pos, out = fec_spec.pieces("mixed_M64")
    ff, fl, par = host("mixed_M64", 1, 2)
    assert int(ff[-1]) == int(first[-1]) > 1
    for p in range(int(first[-1])):
        piece = out[int(pos[p]):int(pos[p + 1])]
        assert int(fl[p]) == piece.size
        assert np.array_equal(par[2 * p * M:2 * p * M + piece.size], piece) and np.array_equal(par[(2 * p + 1) * M:(2 * p + 1) * M + piece.size], piece)


def test_fec_first_depends_on_piece_first_alone():
    _, _, _, _, M, first, pos, out = fec_spec.pieces("records_129")
    rng = np.random.default_rng(6)
    garbage = rng.integers(0, 1 << 62, pos.size, dtype=np.uint64)
    for G in (1, 2, 5):
        ff, fl, par = cwire_fec_host(out, out.size, first, garbage, pos.size - 1, G, 2, M, fill=FILL)
        assert np.array_equal(ff, fec_spec.fec_first(first, G)) and np.array_equal(ff, host("records_129", G, 2)[0])
        assert (par == FILL).all(), "a parity byte of a void group was written"


def group_blocks(name, G, g=0):
    """-> (frame bytes, [the members of group g of record 0], L, P, Q)."""
    n, _, _, _, M, first, pos, out = fec_spec.pieces(name)
    blocks = [out[int(pos[p]):int(pos[p + 1])] for p in fec_spec.members(first, G, 0, g)]
    _, fl, par = host(name, G, 2)
    L = int(fl[g])
    return n, blocks, L, par[2 * g * M:2 * g * M + L], par[(2 * g + 1) * M:(2 * g + 1) * M + L]


def losses(m):
    """(lost slots, P present, Q present): every single slot with either or both parity blocks, and the three pairs."""
    for a in range(m):
        yield (a,), True, True
        yield (a,), True, False
        yield (a,), False, True
    if m >= 2:
        for pair in sorted({(0, 1), (0, m - 1), (m - 2, m - 1)}):
            if pair[0] < pair[1]:
                yield pair, True, True


@pytest.mark.parametrize("name,G,g", [("mixed_M64", 3, 0), ("mixed_M64", 11, 0), ("mixed_M64", 11, 1), ("wave_seam_M516", 8, 1),
                                      ("block_seam_n65537", 8, 11), ("small_n1", 8, 0)])
def test_every_loss_is_rebuilt_byte_for_byte(name, G, g):
    n, blocks, L, P, Q = group_blocks(name, G, g)
    m = len(blocks)
    assert 1 <= m <= G and L == max(b.size for b in blocks)
    if name == "block_seam_n65537":
        assert min(b.size for b in blocks) < L, "a short last piece beside long ones was meant"
    rng = np.random.default_rng(7)
    for lost, hp, hq in losses(m):
        slots = [None if i in lost else b for i, b in enumerate(blocks)]
        outs, verdicts = cwire_fec_repair_host(slots, P if hp else None, Q if hq else None, L)
        mo, mv = fec_spec.repair(slots, P if hp else None, Q if hq else None, L)
        assert len(outs) == len(lost) and list(verdicts) == mv == [0] * len(lost), (lost, hp, hq, verdicts)
        rebuilt = {}
        for i, o, w in zip(lost, outs, mo):
            assert np.array_equal(o, w), (lost, hp, hq)
            assert np.array_equal(o[:blocks[i].size], blocks[i]) and not o[blocks[i].size:].any(), (lost, hp, hq)
            cnt, esc = spec.headers(o, 1)
            size = spec.frame_bytes(int(cnt[0]), int(esc[0]))
            assert size == blocks[i].size and cwire_check_host(o[:size], cnt, esc, n)[0, 0] == 0, "a rebuilt piece is not canonical"
            rebuilt[i] = o[:size]
        # survivors and rebuilt pieces, in a shuffled order, give the state the group's pieces give in order
        want, got = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for b in blocks:
            cwire_apply_host(want, b, 1)
        for i in rng.permutation(m):
            cwire_apply_host(got, rebuilt.get(int(i), blocks[i]), 1)
        assert want.any() and np.array_equal(got, want)


def test_nothing_lost_writes_nothing():
    _, blocks, L, P, Q = group_blocks("mixed_M64", 3)
    outs, verdicts = cwire_fec_repair_host(blocks, P, Q, L)
    assert outs == [] and verdicts.size == 0


def test_repair_on_the_prefix_gives_the_lost_headers():
    _, blocks, L, P, Q = group_blocks("mixed_M64", 11)
    for lost in ((4,), (0, 10), (9, 10)):
        slots = [None if i in lost else b[:8] for i, b in enumerate(blocks)]
        outs, _ = cwire_fec_repair_host(slots, P[:8], Q[:8], 8)
        for i, o in zip(lost, outs):
            assert np.array_equal(o, blocks[i][:8]), lost


def test_a_damaged_survivor_shows_in_the_tail():
    """The shortest member lost and the last word of a longer survivor damaged: the rebuilt block has bytes behind its record."""
    _, blocks, L, P, Q = group_blocks("block_seam_n65537", 8, 11)
    short = int(np.argmin([b.size for b in blocks]))
    longer = next(i for i, b in enumerate(blocks) if b.size == L)
    assert blocks[short].size < L
    slots = [None if i == short else b.copy() for i, b in enumerate(blocks)]
    slots[longer][-1] ^= 0x10
    for p, q in ((P, None), (None, Q), (P, Q)):
        outs, verdicts = cwire_fec_repair_host(slots, p, q, L)
        assert int(verdicts[0]) == lib.FEC_BAD_TAIL == fec_spec.repair(slots, p, q, L)[1][0]
        assert np.array_equal(outs[0][:blocks[short].size], blocks[short])
    # a damaged header word instead: n of the rebuilt header is off
    slots = [None if i == short else b.copy() for i, b in enumerate(blocks)]
    slots[longer][3] ^= 0x80
    outs, verdicts = cwire_fec_repair_host(slots, P, None, L)
    assert int(verdicts[0]) & lib.FEC_BAD_HEADER and int(verdicts[0]) == fec_spec.repair(slots, P, None, L)[1][0]


def test_host_repair_refusals():
    _, blocks, L, P, Q = group_blocks("mixed_M64", 3)
    out = np.full(L, FILL, np.uint8)
    L_ = lib.load()

    def call(slots, lens, p, q, fec_len, out0, out1, verdict, members=None):
        import ctypes as C
        ptrs = (C.c_void_p * 256)(*[None if s is None else s.ctypes.data for s in slots])
        lens = np.asarray(lens + [0], np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data
        return L_.mi355_cwire_fec_repair_host(len(slots) if members is None else members, C.addressof(ptrs), lens.ctypes.data, ptr(p), ptr(q),
                                              fec_len, ptr(out0), ptr(out1), ptr(verdict))

    vd = np.full(2, 77, np.uint32)
    lens = [b.size for b in blocks]
    lost0 = [None] + blocks[1:]
    assert call(lost0, lens, P, None, L, out, None, vd) == lib.OK and np.array_equal(out[:blocks[0].size], blocks[0])
    out[:] = FILL
    vd[:] = 77
    bad = [
        call(lost0, lens, P, Q, L, out, out, vd, members=0), call(lost0, lens, P, Q, L, out, out, vd, members=256),
        call(lost0, lens, P, Q, 0, out, out, vd), call(lost0, lens, P, Q, L + 2, out, out, vd),
        call(lost0, [lens[0], 0, lens[2]], P, Q, L, out, out, vd), call(lost0, [lens[0], lens[1] - 2, lens[2]], P, Q, L, out, out, vd),
        call(lost0, [lens[0], L + 4, lens[2]], P, Q, L, out, out, vd),
        call(lost0, lens, None, None, L, out, out, vd), call([None, None, blocks[2]], lens, P, None, L, out, out, vd),
        call([None, None, None], lens, P, Q, L, out, out, vd),
        call(lost0, lens, P, Q, L, None, out, vd), call([None, None, blocks[2]], lens, P, Q, L, out, None, vd),
        call(lost0, lens, P, Q, L, out, out, None),
    ]
    assert bad == [lib.ERR_INVALID] * len(bad), bad
    assert (out == FILL).all() and (vd == 77).all(), "a refused call wrote"


def test_groups_max():
    for cap, R, G in ((0, 0, 1), (100, 3, 8), (7022, 1, 255), (5, 9, 2)):
        assert cwire_fec_groups_max(cap, R, G) == fec_spec.groups_max(cap, R, G) == cap // G + R
    # never below the groups of any split of `cap` pieces over R records
    rng = np.random.default_rng(8)
    for _ in range(200):
        R, G = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        c = rng.integers(0, 20, R)
        assert int((-(-c // G)).sum()) <= cwire_fec_groups_max(int(c.sum()), R, G)
    assert [cwire_fec_groups_max(10, 1, G) for G in (0, -1, 256)] == [0, 0, 0]

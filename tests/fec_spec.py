"""mi355_cwire_fec_* (include/mi355diff.h, "Parity pieces for the datagram path") stated in numpy: the tests' reference for the
groups, the void rule, the parity blocks and the repair.  Test infrastructure only; the product never imports it.

GF(2^8) modulo x^8 + x^4 + x^3 + x^2 + 1 (0x11D) is done through log / exp tables of the generator 2 -- deliberately not the
shift-and-XOR form the library uses.  Group j of record r has the pieces piece_first[r] + j*G + i, i = 0 .. m - 1; P is the XOR of
the members zero-extended to the longest, Q the XOR of 2^i * member i."""
import functools

import numpy as np

import cwire_spec as spec
import split_spec

BAD_HEADER, BAD_TAIL = 1, 2

EXP = np.zeros(510, np.uint8)
LOG = np.zeros(256, np.int64)
_v = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _v
    LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= 0x11D
assert _v == 1 and len(set(EXP[:255].tolist())) == 255   # 2 generates the group: the powers 2^0 .. 2^254 are distinct


def gf_mul(data, c):
    """Every byte of the uint8 array `data` times the constant c."""
    data = np.asarray(data, np.uint8)
    if c == 0:
        return np.zeros_like(data)
    out = EXP[LOG[data] + int(LOG[c])]
    out[data == 0] = 0
    return out


def gf_inv(c):
    assert c != 0
    return int(EXP[(255 - int(LOG[c])) % 255])


def xtime(v):
    """The library's packed form, on uint32 arrays: only test_cwire_fec_spec.py's Horner check uses it."""
    v = np.asarray(v, np.uint32)
    return ((v & np.uint32(0x7f7f7f7f)) << np.uint32(1)) ^ (((v >> np.uint32(7)) & np.uint32(0x01010101)) * np.uint32(0x1d))


def groups_max(piece_capacity, nrecords, G):
    return piece_capacity // G + nrecords if 1 <= G <= 255 else 0


def fec_first(piece_first, G):
    c = np.diff(np.asarray(piece_first, np.int64))
    return np.concatenate([[0], np.cumsum(-(-c // G))]).astype(np.uint32)


def members(piece_first, G, r, j):
    """The pieces of group j of record r."""
    lo, hi = int(piece_first[r]), int(piece_first[r + 1])
    return list(range(lo + j * G, min(lo + (j + 1) * G, hi)))


def member_len(piece_pos, piece_capacity, pieces_bytes, pitch, p):
    """The length of piece p, 0 when it is absent or malformed (the void rule)."""
    if p >= piece_capacity:
        return 0
    a, b = int(piece_pos[p]), int(piece_pos[p + 1])
    if b > pieces_bytes or b < a or a % 4 or (b - a) % 4 or b == a or b - a > pitch:
        return 0
    return b - a


def parity(blocks, K):
    """[uint8 arrays] (slot order) -> (L, [P] or [P, Q])."""
    L = max(b.size for b in blocks)
    ext = [np.concatenate([b, np.zeros(L - b.size, np.uint8)]) for b in blocks]
    P = np.bitwise_xor.reduce(ext, axis=0)
    Q = np.bitwise_xor.reduce([gf_mul(d, int(EXP[i])) for i, d in enumerate(ext)], axis=0)
    return L, [P, Q][:K]


def reference(pieces, pieces_bytes, piece_first, piece_pos, piece_capacity, G, K, pitch, group_capacity, capacity_bytes, fill):
    """-> (fec_first, fec_len uint32[group_capacity], out uint8[capacity_bytes]); what is not written holds `fill`."""
    first = fec_first(piece_first, G)
    flen = np.full(group_capacity, fill * 0x01010101, np.uint32)
    out = np.full(capacity_bytes, fill, np.uint8)
    for r in range(len(piece_first) - 1):
        for j in range(int(first[r + 1]) - int(first[r])):
            g = int(first[r]) + j
            if g >= group_capacity:
                continue
            lens = [member_len(piece_pos, piece_capacity, pieces_bytes, pitch, p) for p in members(piece_first, G, r, j)]
            if min(lens) == 0:
                flen[g] = 0
                continue
            L, blocks = parity([pieces[int(piece_pos[p]):int(piece_pos[p + 1])] for p in members(piece_first, G, r, j)], K)
            flen[g] = L
            if (g + 1) * K * pitch > capacity_bytes:
                continue
            for q, blk in enumerate(blocks):
                at = (g * K + q) * pitch
                out[at:at + L] = blk
    return first, flen, out


def verdict(block, fec_len):
    """The flags of a rebuilt block of fec_len bytes."""
    if fec_len < 8:
        return BAD_HEADER
    n, e = (int(v) for v in block[:8].view("<u4"))
    size = spec.frame_bytes(n, e)
    flags = BAD_HEADER if n == 0 or e > n or size > fec_len else 0
    if block[min(size, fec_len):fec_len].any():
        flags |= BAD_TAIL
    return flags


def repair(slots, p, q, fec_len):
    """slots: uint8 arrays or None (lost) in slot order; p, q: parity blocks or None -> ([rebuilt blocks of fec_len bytes],
    [verdicts]), by the three formulas of the header."""
    ext = lambda b: np.concatenate([b, np.zeros(fec_len - b.size, np.uint8)])
    lost = [i for i, s in enumerate(slots) if s is None]
    assert len(lost) <= (p is not None) + (q is not None)
    pxy = np.zeros(fec_len, np.uint8) if p is None else p[:fec_len].copy()
    qxy = np.zeros(fec_len, np.uint8) if q is None else q[:fec_len].copy()
    for i, s in enumerate(slots):
        if s is not None:
            pxy ^= ext(s)
            qxy ^= gf_mul(ext(s), int(EXP[i]))
    if not lost:
        return [], []
    if len(lost) == 1:
        a = lost[0]
        out = [pxy if p is not None else gf_mul(qxy, gf_inv(int(EXP[a])))]
    else:
        a, b = lost
        db = gf_mul(qxy ^ gf_mul(pxy, int(EXP[a])), gf_inv(int(EXP[a]) ^ int(EXP[b])))
        out = [pxy ^ db, db]
    return out, [verdict(o, fec_len) for o in out]


# ---- the shapes ----------------------------------------------------------------------------------------------------------
def cases():
    """name -> ((width, height), [(xs, diff)], M, the group sizes it is run at).  All but the last two are split_spec's."""
    base = split_spec.cases()
    rng = np.random.default_rng(4711)
    out = {}
    for name, Gs in (("small_n0", (1, 8)), ("small_n1", (1, 8)), ("mixed_M64", (1, 2, 3, 11, 12, 13)), ("wave_seam_M516", (8,)),
                     ("wave_seam_M520", (8,)), ("wave_seam_M524", (8,)), ("block_seam_n65537", (8,)), ("records_129", (2,)),
                     ("records_1025", (2,))):
        out[name] = base[name] + (Gs,)
    n_wide = 3 * split_spec.WIDE[0] * split_spec.WIDE[1]
    dense = lambda: (np.arange(n_wide), rng.integers(1, 256, n_wide))
    out["long_group_M64"] = (split_spec.WIDE, [dense()], 64, (255,))     # more than 255 pieces: full groups in front of a short one
    out["long_block_M65536"] = (split_spec.WIDE, [dense()], 65536, (4,))  # parity blocks many chunks long
    return out


CASES = cases()
POINTS = [(name, G, K) for name in sorted(CASES) for G in CASES[name][3] for K in (1, 2)]


@functools.lru_cache(maxsize=None)
def pieces(name):
    """-> (frame bytes, the records, counts, escapes, M, piece_first, piece_pos, the pieces) of a case, made once and read-only."""
    (w, h), segs, M, _ = CASES[name]
    buf, counts, escapes = split_spec.records(segs)
    first, pos, out = split_spec.reference(buf, len(segs), M)
    for a in (buf, counts, escapes, first, pos, out):
        a.setflags(write=False)
    return 3 * w * h, buf, counts, escapes, M, first, pos, out

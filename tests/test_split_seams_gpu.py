"""-m gpu: mi355_cwire_split_cwire_batch past the fixed counts at which its kernels start another round, list slot, block or launch
(csrc/stream_ops.hip: k_cws_table, k_cws_count / k_cws_emit through cws_walk and cws_write_piece, k_cws_scan):
    kCwsThreads 1024   a round of cws_walk is 1024 code dwords, 4096 entries.  long_piece: a dense record of 150 000 entries at
                       max_bytes 8196 / 8200 / 8204 / 65536 -- pieces of 4092 entries that begin at a round's dword 1023, pieces of
                       4096 that begin at a fresh round's dword 0 (s_v[0]), and pieces of 32 764 entries that take eight rounds
                       whole, so wave 0 leaves a round with q == nd and no cut and o_d, o_base, o_x, o_rank, o_F live on
    kCwsList 516       a round closes at most kCwsThreads / 2 pieces and the block's last.  list_full: 4591 entries 257 apart at
                       max_bytes 64, every piece two dwords: round 0 closes exactly 512 pieces, the sixteen waves copy 32 listed
                       pieces each; the same indices from 300, where the first piece has F = 1
    kCwsBlock 65536    a block starts from the chunk table's words ch.y (escape rank) and ch.z (running index) at
                       f.cbase + 16 * block.  escapes_late: 80 000 entries whose 224 escapes sit at every round's first entry, at
                       block 0's last entry, at block 1's first entries, on both sides of a round seam of block 1 and in a run of
                       200; so ch.y != 0 in block 1, carry_e != 0 across rounds, pieces open on a 255 code (- 4*[code[4a] == 255])
                       and on a smaller code with x_a >= 255 (+ 4*F(a))
    k_cws_table        bbase[] of a multi-block record behind other records, an n == 0 record's one empty block between them,
      64 threads       f.cbase for record > 0 with block > 0: many_records (blocks [3, 1, 2, 1, 2]).  The j += 64 loop: blocks_65,
                       one record of 4 195 800 entries, 65 blocks
    kCwsTableRecords   145 records are two k_cws_table launches (128 a launch): many_records x 29
      128
    k_cws_scan         256 blocks a round: many_records x 29 is 261 blocks and a two-block record lies on blocks 255 and 256,
      256 threads      its w.y == 0 block in round 0 of the scan and its last in round 1
    capacities         piece_capacity and capacity_bytes that end one piece before, at, and one piece behind the end of block 0 of
                       a three-block and of a two-block record: the p0 / b0 of base[] decide what block 1 may write
    malformed content  a record with 2041 more 255 codes than its header's e, a wrapping running index and an escape of 5 * N
                       between two well-formed records: more pieces and bytes than the capacity helpers allow for
    c->cws_blk,        two and three calls queued on one core with nothing in between, on the core's stream and on the caller's:
    c->cws_base        each call's count, scan and emit passes rewrite the words the call before it left

The reference of every comparison is the host form mi355_cwire_split_host, bit for bit (piece_first, piece_pos, pieces), through
run / check of test_cwire_split_gpu.py: guarded buffers that start as a non-zero pattern.  test_split_seams_host.py holds the host
form to the numpy statement of the rule (split_spec.reference) on every well-formed case here.  The inputs are made once,
read-only, by the builders below; each builder asserts from the host form alone that its input reaches the seam it is named for,
and test_split_seams_host.py runs every builder without a GPU."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cwire_spec as spec
import split_spec
from cudavideostream_amd import cwire_split_bytes_max, cwire_split_host, cwire_split_pieces_max, lib
from gpu_util import GUARD, CUDACore, Guarded
from test_cwire_split_gpu import POS_FILL, capacities, check, run

pytestmark = pytest.mark.gpu

WIDE, LIST, BIG = split_spec.WIDE, (1024, 384), (1400, 999)   # 196 608, 1 179 648 and 4 195 800 bytes per frame
BLOCK = lib.CWIRE_SPLIT_BLOCK
ROUND = 4096          # entries of a round of cws_walk: kCwsThreads dwords
LIST_ROUND = 512      # pieces a round can close beside the block's last: kCwsThreads / 2
SCAN_ROUND = 256      # blocks of a round of k_cws_scan
TABLE_LAUNCH = 128    # records of a k_cws_table launch: kCwsTableRecords
MAX_BATCH = {WIDE: 145, LIST: 1, BIG: 1}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def make(frame, segs, M):
    """The case of the records `segs` on a core of `frame` at max_bytes M: the input and the host form's result at the helpers'
    capacities, read-only."""
    buf, counts, escapes = split_spec.records(segs)
    want = cwire_split_host(buf, counts, escapes, 3 * frame[0] * frame[1], M)
    frozen(buf, counts, escapes, *want)
    return SimpleNamespace(frame=frame, buf=buf, counts=counts, escapes=escapes, M=M, want=want)


def spans(c):
    """(record, first entry, end) of every piece, int64 arrays, from the headers of the host form's pieces."""
    wf, wp, wo = c.want
    total = int(wf[-1])
    assert total + 1 <= wp.size and int(wp[total]) <= wo.size, "the case's capacities hold every piece"
    lens = wo[:int(wp[total])].view("<u4")[(wp[:total] // 4).astype(np.int64)].astype(np.int64)
    rec = np.repeat(np.arange(c.counts.size), np.diff(wf.astype(np.int64)))
    end = np.empty(total, np.int64)
    for r in range(c.counts.size):
        a, b = int(wf[r]), int(wf[r + 1])
        end[a:b] = np.cumsum(lens[a:b])
        assert (int(end[b - 1]) if b > a else 0) == int(c.counts[r]), "a record's pieces hold its entries"
    return rec, end - lens, end


def sizes(c):
    wf, wp, _ = c.want
    return np.diff(wp[:int(wf[-1]) + 1].astype(np.int64))


def sections(c, r):
    """(code uint8[n], esc uint32[e]) of input record r."""
    at = sum(spec.frame_bytes(n, e) for n, e in zip(c.counts[:r], c.escapes[:r]))
    n, e = int(c.counts[r]), int(c.escapes[r])
    return c.buf[at + 8:at + 8 + n], c.buf[at + 8 + spec.pad4(n):at + 8 + spec.pad4(n) + 4 * e].view("<u4")


def blocks_of(counts):
    return [max(1, -(-int(n) // BLOCK)) for n in counts]


def dense(rng, n, start):
    return np.arange(start, start + n), rng.integers(1, 256, n)


# ---- A. the piece list at its bound ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def list_full(start):
    """Every 257th byte of 1024x384 from `start` at max_bytes 64: every entry behind the first is escaped, a piece is eight
    entries, two dwords, and round 0 of the one block closes kCwsThreads / 2 pieces."""
    N = 3 * LIST[0] * LIST[1]
    rng = np.random.default_rng(257 + start)
    xs = np.arange(start, N, 257)
    c = make(LIST, [(xs, rng.integers(1, 256, xs.size))], 64)
    n, e = int(c.counts[0]), int(c.escapes[0])
    assert (n, e) == ((4591, 4590) if start == 0 else (4589, 4589)) and n < BLOCK
    _, a, b = spans(c)
    assert ((b - a)[:-1] == 8).all() and 0 < (b - a)[-1] <= 8
    assert list(sizes(c)[:2]) == [52 if start == 0 else 56, 56] and (sizes(c)[1:-1] == 56).all()
    per_round = np.bincount((b - 1) // ROUND)
    assert list(per_round) == [512, 62] and per_round[0] == LIST_ROUND and a.size == 574
    return c


# ---- B. pieces longer than a round, cuts at a round's first and last dword -------------------------------------------------
LONG_M = (8196, 8200, 8204, 65536)


@functools.lru_cache(maxsize=None)
def long_piece(M):
    """150 000 dense entries from index 17 (e == 0, three blocks) at max_bytes M."""
    c = make(WIDE, [dense(np.random.default_rng(150000), 150000, 17)], M)
    assert list(c.counts) == [150000] and list(c.escapes) == [0]
    _, a, b = spans(c)
    lens, inblock = b - a, a % BLOCK
    if M == 8196:
        assert a.size == 39 and (lens[:15] == 4092).all()
    if M == 8200:
        assert a.size == 39 and lens[0] == 4096 and (lens[1:15] == 4092).all(), "x_0 = 17 < 255: F = 0 on the first piece only"
        assert inblock[1] == 4096 and inblock[2] % ROUND == 4092, "a cut at a round's dword 0, the next at dword 1023"
    if M in (8196, 8200):
        assert (inblock % ROUND == 4092).any(), "a piece that opens at a round's last dword"
    if M == 8204:
        assert a.size == 37 and (lens[:-1] == 4096).all()
        assert ((inblock > 0) & (inblock % ROUND == 0)).sum() >= 30, "pieces behind a block's first that open at a round's dword 0"
    if M == 65536:
        assert list(lens) == [32764, 32760, 12, 32760, 32760, 16, 18928]
        whole = [(int(s), int(t)) for s, t in zip(inblock, inblock + lens) if any(s <= ROUND * j and t >= ROUND * (j + 1) for j in range(16))]
        assert len(whole) == 5, "pieces that cover whole rounds of their block: no cut in those rounds"
        assert lens[2] == 12 and b[2] == BLOCK, "a piece of 12 entries closes block 0"
    return c


# ---- C. escapes at the round and block seams -------------------------------------------------------------------------------
LATE_N = 80000
LATE_ESCAPES = sorted(set(range(ROUND, LATE_N, ROUND)) | {65535, 65536, 65537, 65540, 69631, 69633} | set(range(66000, 66400, 2)))


@functools.lru_cache(maxsize=None)
def late_record():
    """(xs, diff): 80 000 entries, the first at index 3, every other one adjacent to its predecessor but for gaps of
    255 + k % 3 in front of the entries k of LATE_ESCAPES."""
    g = np.zeros(LATE_N, np.int64)
    g[0] = 3
    for k in LATE_ESCAPES:
        g[k] = 255 + k % 3
    xs = np.cumsum(g + 1) - 1
    assert len(LATE_ESCAPES) == 224 and int(xs[-1]) == 137346 < 3 * WIDE[0] * WIDE[1]
    return frozen(xs, np.random.default_rng(224).integers(1, 256, LATE_N))


def late_seams(c, r):
    """The seam assertions of escapes_late for record r of case c (the record of late_record)."""
    code, esc = sections(c, r)
    rec, a, b = spans(c)
    a = a[rec == r]
    assert code.size == LATE_N and esc.size == 224
    assert code[BLOCK] == 255 and code[BLOCK - 1] == 255, "a 255 code at block 1's first entry and at block 0's last"
    assert all(code[k] == 255 for k in range(ROUND, LATE_N, ROUND)), "a 255 code at every round's first entry"
    assert int((code[:BLOCK] == 255).sum()) == 16 > 0, "the escape rank in front of block 1 (ch.y) is not zero"
    assert {BLOCK + ROUND - 1, BLOCK + ROUND, BLOCK + ROUND + 1} <= set(np.flatnonzero(code == 255)), "escapes on both sides of a round seam of block 1"
    in1 = a[a >= BLOCK]
    assert BLOCK in in1 and (code[in1] == 255).any(), "a piece of block 1 opens on a 255 code"
    xs = late_record()[0]
    assert ((code[in1] < 255) & (xs[in1] >= 255)).any(), "a piece of block 1 has F = 1 and a first code below 255 in the input"


@functools.lru_cache(maxsize=None)
def escapes_late(M):
    c = make(WIDE, [late_record()], M)
    assert list(c.counts) == [LATE_N] and list(c.escapes) == [224]
    assert int(c.want[0][-1]) == {64: 3350, 1400: 117}[M]
    late_seams(c, 0)
    return c


# ---- D. multi-block records behind other records ---------------------------------------------------------------------------
def five_records():
    rng = np.random.default_rng(5)
    three = np.array([5, 900, 70000])
    return [dense(rng, 131073, 17), (np.empty(0, np.int64), np.empty(0, np.uint8)), late_record(), (three, rng.integers(1, 256, 3)),
            dense(rng, 70001, 300)]


@functools.lru_cache(maxsize=None)
def many_records(reps):
    """reps == 1: the five records.  reps == 29: the five rotated by two -- escapes_late's, three entries, 70 001 dense,
    131 073 dense, none -- and repeated: 145 records, 261 blocks, the two blocks of a 70 001-entry record are blocks 255 and 256."""
    five = five_records()
    if reps == 1:
        c = make(WIDE, five, 1400)
        assert list(c.counts) == [131073, 0, 80000, 3, 70001] and list(c.escapes) == [0, 0, 224, 2, 1]
        assert int(c.want[0][-1]) == 411 and list(np.diff(c.want[0].astype(np.int64)))[1] == 0
        assert blocks_of(c.counts) == [3, 1, 2, 1, 2], "records 2 and 4: block > 0 at record > 0; record 1: one empty block"
        late_seams(c, 2)
        return c
    c = make(WIDE, (five[2:] + five[:2]) * reps, 1400)
    nb = blocks_of(c.counts)
    first = np.cumsum([0] + nb)
    assert c.counts.size == 145 > TABLE_LAUNCH and c.counts.size <= MAX_BATCH[WIDE] and first[-1] == 261 > SCAN_ROUND
    across = [r for r in range(c.counts.size) if first[r] < SCAN_ROUND <= first[r + 1] - 1]
    assert across == [142] and c.counts[142] == 70001 and (first[142], first[143]) == (255, 257), "a record's first block in the scan's round 0, its last in round 1"
    assert int(c.want[0][-1]) == 411 * reps
    return c


# ---- E. more blocks than the table kernel has threads ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blocks_65():
    N = 3 * BIG[0] * BIG[1]
    c = make(BIG, [dense(np.random.default_rng(65), N, 0)], 8972)
    n = int(c.counts[0])
    assert n == N == 4195800 and -(-n // BLOCK) == 65 > 64 and int(c.want[0][-1]) == 961
    return c


# ---- F. capacities at the block seams --------------------------------------------------------------------------------------
SEAM_CAPACITY_CASES = ("dense_3_blocks", "escapes_late_M64", "escapes_late_M1400")


@functools.lru_cache(maxsize=None)
def seam_capacities(name):
    """-> (case, [(piece_capacity, capacity_bytes)]): piece capacities that end one piece before the end of block 0, at it and
    one piece into block 1; byte capacities 4 short of the end of block 0's last piece and exactly at it."""
    c = make(WIDE, five_records()[:1], 1400) if name == "dense_3_blocks" else escapes_late(int(name.split("_M")[1]))
    wf, wp, _ = c.want
    _, a, b = spans(c)
    total, size = int(wf[-1]), int(wp[int(wf[-1])])
    p0 = int((b <= BLOCK).sum())
    assert 1 < p0 < total - 1 and b[p0 - 1] == BLOCK and a[p0] == BLOCK, "block 0 ends with piece p0 - 1"
    return c, [(p0 - 1, size), (p0, size), (p0 + 1, size), (total, int(wp[p0]) - 4), (total, int(wp[p0]))]


# ---- G. malformed content under consistent headers -------------------------------------------------------------------------
MALFORMED_M = (64, 1400, 65536)
MALFORMED_FIGURES = {64: (3522, 5550, None, None), 1400: (123, 119, 170492, 162332), 65536: (4, None, 169100, 160952)}


@functools.lru_cache(maxsize=None)
def malformed(M):
    """Three records: 300 scattered entries, escapes_late's record damaged under its unchanged header, 70 001 dense entries.
    -> the case (its `want` at ample capacities), the ample capacities, the helpers' capacities and the host form at those."""
    N = 3 * WIDE[0] * WIDE[1]
    rng = np.random.default_rng(7)
    x = np.sort(rng.choice(N, 300, replace=False))
    good = make(WIDE, [(x, rng.integers(1, 256, 300)), late_record(), dense(rng, 70001, 300)], M)
    buf = good.buf.copy()
    at = spec.frame_bytes(good.counts[0], good.escapes[0])
    code, esc = buf[at + 8:at + 8 + LATE_N], buf[at + 8 + LATE_N:at + 8 + LATE_N + 4 * 224].view("<u4")
    code[0] = 255
    code[100:140] = 255
    code[70000:72000] = 255
    esc[0] = 0xFFFFFF00
    esc[5] = 5 * N
    assert int((code == 255).sum()) == 224 + 2041 and spec.headers(buf, 3)[1][1] == 224, "2041 more 255 codes than e"
    ample = tuple(2 * v for v in capacities(good.counts, good.escapes, M))
    want = cwire_split_host(buf, good.counts, good.escapes, N, M, piece_capacity=ample[0], capacity_bytes=ample[1])
    c = SimpleNamespace(frame=WIDE, buf=buf, counts=good.counts, escapes=good.escapes, M=M, want=want)
    frozen(buf, *want)
    wf, wp, _ = want
    total = int(wf[-1])
    assert total <= ample[0] and int(wp[total]) <= ample[1]
    pieces, nbytes = int(wf[2]) - int(wf[1]), int(wp[int(wf[2])]) - int(wp[int(wf[1])])
    pmax, bmax = cwire_split_pieces_max(LATE_N, 224, M), cwire_split_bytes_max(LATE_N, 224, M)
    fp, fpm, fb, fbm = MALFORMED_FIGURES[M]
    assert pieces == fp and (fpm is None or pmax == fpm) and (fb is None or nbytes == fb) and (fbm is None or bmax == fbm)
    for r in (0, 2):   # the records on either side are cut as they are in a call of well-formed records
        assert int(wf[r + 1]) - int(wf[r]) == int(good.want[0][r + 1]) - int(good.want[0][r])
    helper = capacities(c.counts, c.escapes, M)
    want_helper = frozen(*cwire_split_host(buf, c.counts, c.escapes, N, M, piece_capacity=helper[0], capacity_bytes=helper[1]))
    if M == 1400:
        assert pieces > pmax and nbytes > bmax
        assert total > helper[0] or int(wp[total]) > helper[1], "at least one piece does not fit the helpers' capacities"
    return c, ample, helper, want_helper


def check_malformed(got, want, c, piece_cap, cap):
    """(i) the tables as far as they reach, (ii) nothing outside the pieces that fit, (iii) records 0 and 2 bit for bit, (iv) a
    header {len, E} that gives its size on every written piece of record 1.  -> (pieces of record 1 written, their entries,
    pieces of the call that were skipped)."""
    (gf, gp, go), (wf, wp, wo) = got, want
    total = int(wf[-1])
    reach = min(total, piece_cap)
    assert np.array_equal(gf, wf)
    assert np.array_equal(gp[:reach + 1], wp[:reach + 1])
    assert (gp[reach + 1:] == POS_FILL).all(), "piece_pos written past min(total, piece_capacity)"
    written = np.zeros(cap, bool)
    made = entries = 0
    skipped = total - reach
    for p in range(reach):
        a, b = int(wp[p]), int(wp[p + 1])
        if b > cap:
            skipped += 1
            continue
        written[a:b] = True
        if int(wf[1]) <= p < int(wf[2]):
            ln, E = (int(v) for v in go[a:a + 8].view("<u4"))
            assert 8 + 2 * spec.pad4(ln) + 4 * E == b - a <= c.M, f"piece {p}: header {ln}, {E} on {b - a} bytes"
            made, entries = made + 1, entries + ln
        else:
            assert np.array_equal(go[a:b], wo[a:b]), f"piece {p}"
    assert (go[~written] == GUARD).all(), "bytes outside the pieces that fit were written"
    return made, entries, skipped


# ---- H. one call after another on the core's scratch -----------------------------------------------------------------------
def chains():
    """frame -> the cases queued on one core of that frame with nothing in between.  The count pass of each leaves other words
    in block 0's row of c->cws_blk, and the scan other words in c->cws_base, than the call before it."""
    out = {WIDE: [escapes_late(64), many_records(1), escapes_late(1400)], LIST: [list_full(0), list_full(300), list_full(0)]}
    for frame, cs in out.items():
        assert all(c.frame == frame and c.counts.size <= 5 for c in cs)
        for x, y in zip(cs, cs[1:]):
            fx, fy = (int((spans(c)[2][spans(c)[0] == 0] <= BLOCK).sum()) for c in (x, y))
            bx, by = (int(sizes(c)[:f].sum()) for c, f in ((x, fx), (y, fy)))
            assert (fx, bx) != (fy, by), "block 0's pieces and bytes differ from the call before"
    return out


# ---- the GPU side ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cores():
    """frame -> a core of that frame, made when first asked for and kept for the module."""
    with contextlib.ExitStack() as stack:
        made = {}

        def core(frame):
            if frame not in made:
                made[frame] = stack.enter_context(CUDACore(*frame, max_batch=MAX_BATCH[frame]))
            return made[frame]

        yield core


def compare(core, c):
    piece_cap, cap = capacities(c.counts, c.escapes, c.M)
    check(run(core, c.buf, c.counts, c.escapes, c.M, piece_cap, cap), c.want, piece_cap, cap)


@pytest.mark.parametrize("start", [0, 300])
def test_list_full(cores, start):
    """Round 0 lists 512 pieces, every wave writes 32 of them."""
    compare(cores(LIST), list_full(start))


@pytest.mark.parametrize("M", LONG_M)
def test_long_piece(cores, M):
    """Cuts at a round's dword 1023 and dword 0; at 65536 rounds without a cut."""
    compare(cores(WIDE), long_piece(M))


@pytest.mark.parametrize("M", [64, 1400])
def test_escapes_late(cores, M):
    """ch.y and carry_e are not zero; pieces open on 255 codes at the first entry of a round and of block 1."""
    compare(cores(WIDE), escapes_late(M))


@pytest.mark.parametrize("reps", [1, 29])
def test_many_records(cores, reps):
    """Blocks [3, 1, 2, 1, 2]; 29 times: two table launches, 261 blocks, a record on blocks 255 and 256."""
    compare(cores(WIDE), many_records(reps))


def test_blocks_65(cores):
    """65 blocks of one record: thread 0 of k_cws_table writes two rows."""
    compare(cores(BIG), blocks_65())


@pytest.mark.parametrize("name", SEAM_CAPACITY_CASES)
def test_capacities_at_the_block_seams(cores, name):
    """The host form at the same capacities: the tables exact as far as they reach, the pieces that fit, nothing else."""
    c, caps = seam_capacities(name)
    N = 3 * c.frame[0] * c.frame[1]
    for piece_cap, cap in caps:
        want = cwire_split_host(c.buf, c.counts, c.escapes, N, c.M, piece_capacity=piece_cap, capacity_bytes=cap)
        reach = min(int(c.want[0][-1]), piece_cap)
        assert np.array_equal(want[0], c.want[0]) and np.array_equal(want[1], c.want[1][:reach + 1]), "the tables stay exact"
        check(run(cores(WIDE), c.buf, c.counts, c.escapes, c.M, piece_cap, cap), want, piece_cap, cap)


@pytest.mark.parametrize("M", MALFORMED_M)
def test_malformed_content(cores, M):
    """Once with twice the helpers' capacities, once with the helpers' own, which at 1400 are too small."""
    c, ample, helper, want_helper = malformed(M)
    got = run(cores(WIDE), c.buf, c.counts, c.escapes, M, *ample)
    made, entries, skipped = check_malformed(got, c.want, c, *ample)
    assert made == MALFORMED_FIGURES[M][0] and entries == LATE_N and not skipped, "every piece of the damaged record, and its lens sum to n"
    got = run(cores(WIDE), c.buf, c.counts, c.escapes, M, *helper)
    made, _, skipped = check_malformed(got, want_helper, c, *helper)
    assert 0 < made <= MALFORMED_FIGURES[M][0] and (M != 1400 or skipped > 0), "at 1400 the helpers' capacities leave pieces out"


def staged(c):
    """The case's input and its own outputs at the helpers' capacities, in guarded buffers."""
    piece_cap, cap = capacities(c.counts, c.escapes, c.M)
    return SimpleNamespace(c=c, piece_cap=piece_cap, cap=cap, src=Guarded(c.buf.size, torch.uint8, data=c.buf),
                           first=Guarded(c.counts.size + 1, torch.int32), pos=Guarded(piece_cap + 1, torch.int64), out=Guarded(cap))


@pytest.mark.parametrize("mode", ["own", "callers"])
def test_back_to_back_on_one_core(mode):
    """The three cases of each chain queued on one core with nothing in between, each into outputs of its own; one
    synchronisation, then every output against the host form.  escapes_late at 64 (2 blocks), many_records (9), escapes_late at
    1400 (2); and list_full from 0, from 300 and from 0 again on a core of its frame."""
    for frame, cs in chains().items():
        with CUDACore(*frame, max_batch=5) as core:
            if mode == "callers":
                core.use_torch_stream()
            qs = [staged(c) for c in cs]
            torch.cuda.synchronize()
            for q in qs:
                c = q.c
                core.cwire_split_cwire_batch(q.src.ptr, c.counts, c.escapes, c.counts.size, c.M, q.first.ptr, q.pos.ptr, q.piece_cap,
                                             q.out.ptr, q.cap)
            core.synchronize()
            for q in qs:
                assert np.array_equal(q.src.get(), q.c.buf)
                got = q.first.get().view(np.uint32), q.pos.get().view(np.uint64), q.out.get()
                check(got, q.c.want, q.piece_cap, q.cap)

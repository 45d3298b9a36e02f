"""-m gpu: mi355_cwire_runs_encode_batch / _decode_batch and mi355_cwire_despeckle_cwire_batch past the fixed counts at which
their kernels start another round, launch or block (csrc/stream_ops.hip), and the link's positions past 2^32:
    k_cwr_scan      256 chunks of 4096 codes per round: 592x592 (N = 1 051 392), records of 257 chunks; `holes` has run starts in
                    chunks 255 and 256, so chunk 256's first run rank holds the carry of round 0
    k_cwr_dscan     256 workgroups of 1024 runs per round: `alternating` at 592x592 has 525 696 runs, 514 workgroups, three rounds
                    (the LDS words alternate back to the first set)
    k_cwr_expand    one workgroup writing many tiles of 4096 entries: `whole` at 592x592, 1024 runs of 256 entries = 64 tiles
    k_cwr_place     256 records per round: 257 and 513 records at 64x48 (k_cwa_table's 128 and k_cwr_table's 64 a launch are
                    crossed several times on the way), the skipped records starting at record 256
    k_dsp_init      128 needs by value per launch: 129 and 257 streams at 37x11, the needs around the seams all different;
                    grid.y = nwords / 4096 + 1 blocks striding over the changed bitmap: 509x258 (4104 words, 2 blocks) and
                    643x409 (8219 words, 3 blocks), a sparse call between two dense ones on the same stream slots
    k_dsp_keep      the first / last column masks of a word that holds several rows (W = 3 .. 31) or exactly one (W = 32), and
                    W = 63, 65, 96: despeckle_spec.NARROW at every need
    o.out + pos, rec.in_pos, rec.out_pos, pos[], frame_pos[]   1400 records of 3 150 012 bytes at 1000x700: pos passes 2^32 at
                    record 1364 (the encoder's output, the decoder's input)

The reference of every comparison is the host form (mi355_cwire_runs_*_host, mi355_cwire_despeckle_host), which
test_runs_despeckle_seams_host.py holds to the numpy statements (runs_spec, despeckle_spec) on these very inputs; the large link is
built from runs_spec's templates on the device.  Every buffer the GPU sees is guarded (gpu_util) and starts as a non-zero pattern;
inputs are asserted unchanged.  The inputs are made once, read-only, by the builders below; each builder asserts from the
reference alone that its input reaches the seam it is named for, and the host file runs every builder without a GPU and proves,
by mutants stated in numpy, that the inputs tell a kernel that forgets a carry, a launch base or a block from a right one."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
import despeckle_spec as ds
import runs_spec as rs
from cudavideostream_amd import cwire_despeckle_host, cwire_runs_bytes_max, cwire_runs_decode_host, cwire_runs_encode_host, lib
from gpu_util import DEV, GUARD, BigGuarded, CUDACore, Guarded, Region, to_dev
from test_cwire_despeckle_gpu import run as dsp_run
from test_cwire_runs_gpu import POLICIES, check_written, gpu_decode, gpu_encode
from test_top_of_range_gpu import assert_equal, assert_rows_on_device, require, slices

pytestmark = pytest.mark.gpu

K = 4096                      # codes of a chunk, entries of a tile of k_cwr_expand
ROUND = 256                   # chunks, workgroups or records of a round of the three scans
RUNS = 1024                   # runs of a decode workgroup (kCwrRuns)
INIT_STREAMS = 128            # needs of a k_dsp_init launch (kDspInitStreams)
INIT_WORDS = 4096             # bitmap words per block of k_dsp_init's grid.y


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- a. 257 chunks, 514 decode workgroups -------------------------------------------------------------------------------------
BW, BH = 592, 592
BN = 3 * BW * BH              # 1 051 392
HOLES = (5, K * 255 + 7, K * 256 - 1, K * 256, K * 256 + 300, BN - 2)
CHUNK_FORMS = {"whole": [1, 1051392, 0, 4107], "holes": [1, 1051386, 0, 4112], "alternating": [None, 525696, 0, 525696],
               "mixed": [1, 666468, 562, 6349]}


@functools.lru_cache(maxsize=None)
def chunk_case():
    """592x592, four records -> (names, records back to back, counts, escapes).  Asserted from runs_spec alone: the form rows,
    257 chunks for `whole` and `holes`, run starts of `holes` on both sides of entry 2^20 with a non-zero rank carried into
    chunk 256, three rounds of decode workgroups for `alternating`, escapes in `mixed`."""
    assert BN == 1051392 and -(-BN // K) == ROUND + 1
    pats = {"whole": np.arange(BN), "holes": np.setdiff1d(np.arange(BN), HOLES), "alternating": np.arange(0, BN, 2),
            "mixed": rs.mixed_xs(BN, 1)}
    recs = [rs.record(xs, i) for i, xs in enumerate(pats.values())]
    buf = np.concatenate(recs)
    counts, escapes = spec.headers(buf, len(recs))
    for name, rec in zip(pats, recs):
        n, e, code, _, _ = rs.sections(rec)
        gap, ln = rs.runs_of(code)
        want = CHUNK_FORMS[name]
        assert [n, e, gap.size] == want[1:], (name, n, e, gap.size)
        assert rs.smaller(n, gap.size) == (name != "alternating")
        if name in ("whole", "holes"):
            assert n > ROUND * K and -(-n // K) == ROUND + 1, "257 chunks: the second round of k_cwr_scan is one chunk"
        if name == "whole":
            assert gap.size > 4 * RUNS and (ln[:RUNS] == 255).all(), "a decode workgroup of 1024 runs of 256 entries: 64 tiles"
        if name == "holes":
            at = np.flatnonzero(code)
            assert ((at >= 255 * K) & (at < 256 * K)).sum() == 2 and (at >= 256 * K).sum() == 2, "run starts in chunks 255 and 256"
            assert (256 * K - 3) in at and at.size == 5 and code[at].tolist() == [1, 1, 2, 1, 1]
        if name == "alternating":
            wgs = -(-gap.size // RUNS)
            assert wgs == 514 and wgs > 2 * ROUND, "three rounds of k_cwr_dscan, the third of two workgroups"
        if name == "mixed":
            assert e > 0 and (gap == 255).sum() == e
    return (list(pats),) + frozen(buf, counts, escapes)


@pytest.fixture(scope="module")
def chunk_core():
    with CUDACore(BW, BH, max_batch=4) as core:
        yield core


@pytest.mark.parametrize("skip", [False, True], ids=["all", "skip"])
@pytest.mark.parametrize("policy", POLICIES)
def test_records_past_the_chunk_and_workgroup_rounds(chunk_core, policy, skip):
    """One call of the four records, both ways, against the host forms; `skip`: the capacity ends four bytes short of record
    1's end, so records 1 to 3 are skipped whole and record 0 is written."""
    names, buf, counts, escapes = chunk_case()
    wf, wp, wo = cwire_runs_encode_host(buf, counts, escapes, BN, policy)
    for name, row in zip(names, wf):
        want = CHUNK_FORMS[name]
        assert list(row[1:]) == want[1:] and row[0] == (int(policy == lib.RUNS_ALWAYS) if want[0] is None else want[0]), name
    cap = int(wp[2]) - 4 if skip else int(wp[-1])
    gf, gp, go = gpu_encode(chunk_core, buf, counts, escapes, policy, cap)
    assert np.array_equal(gf, wf), [names[b] for b in range(4) if not np.array_equal(gf[b], wf[b])]
    assert np.array_equal(gp, wp)
    check_written(go, wo, wp, cap, "record")
    link = wo[:int(wp[-1])]
    fp, cw = cwire_runs_decode_host(link, wf, BN)
    assert cw.tobytes() == buf.tobytes()
    cap = int(fp[2]) - 4 if skip else buf.size
    gfp, gcw = gpu_decode(chunk_core, link, wf, cap)
    assert np.array_equal(gfp, fp)
    check_written(gcw, buf, fp, cap, "record")


# ---- b. 257 and 513 records ---------------------------------------------------------------------------------------------------
SW, SH, SN = 64, 48, 9216
MANY_MAX = 513
AT_SEAMS = {255: "run4097", 256: "r3", 257: "mixed2", 511: "escape_on_cut", 512: "straddle"}


@functools.lru_cache(maxsize=None)
def many_case():
    """513 records of mixed forms at 64x48, drawn from runs_spec.patterns as test_cwire_runs_gpu.many draws its 130 -> (records,
    counts, escapes, the byte at which each starts).  The records on both sides of 256 and of 512 are of five different sizes,
    on the link and decoded, so a position that restarts or repeats there is another number."""
    pats = rs.patterns(SN)
    order = [n for n in pats if n not in ("whole", "alternating")]
    names = [order[i % len(order)] for i in range(MANY_MAX)]
    names[64] = names[300] = "whole"
    for b, name in AT_SEAMS.items():
        names[b] = name
    recs = [rs.record(pats[name], 100 + i) for i, name in enumerate(names)]
    buf = np.concatenate(recs)
    counts, escapes = spec.headers(buf, MANY_MAX)
    start = np.cumsum([0] + [r.size for r in recs])
    forms, pos, _ = rs.encode(buf, MANY_MAX, rs.WHERE_SMALLER)
    for R in (257, 513):
        assert 0 < int(forms[:R, 0].sum()) < R, "both forms occur"
    sizes = np.diff(pos.astype(np.int64))
    assert len({int(sizes[b]) for b in AT_SEAMS}) == 5 and len({recs[b].size for b in AT_SEAMS}) == 5
    assert int(pos[256]) > 0 and forms[256, 0] != forms[255, 0], "the forms differ across the round, too"
    return frozen(buf, counts, escapes, start)


def many_head(R):
    buf, counts, escapes, start = many_case()
    return buf[:int(start[R])], counts[:R], escapes[:R]


@pytest.fixture(scope="module")
def many_core():
    with CUDACore(SW, SH, max_batch=MANY_MAX) as core:
        yield core


@pytest.mark.parametrize("skip", [False, True], ids=["all", "skip"])
@pytest.mark.parametrize("R", [257, 513])
def test_records_past_the_place_rounds(many_core, R, skip):
    """257 records: the second round of k_cwr_place is one record; 513: the third takes the first set of LDS words again.
    pos[] and frame_pos[] exactly; `skip`: the first record that does not fit is record 256."""
    buf, counts, escapes = many_head(R)
    wf, wp, wo = cwire_runs_encode_host(buf, counts, escapes, SN, lib.RUNS_WHERE_SMALLER)
    assert 0 < int(wf[:, 0].sum()) < R
    cap = int(wp[257]) - 4 if skip else int(wp[-1])
    gf, gp, go = gpu_encode(many_core, buf, counts, escapes, lib.RUNS_WHERE_SMALLER, cap)
    assert np.array_equal(gf, wf)
    assert_equal(gp, wp, "pos")
    check_written(go, wo, wp, cap, "record")
    link = wo[:int(wp[-1])]
    fp, cw = cwire_runs_decode_host(link, wf, SN)
    assert cw.tobytes() == buf.tobytes()
    cap = int(fp[257]) - 4 if skip else buf.size
    gfp, gcw = gpu_decode(many_core, link, wf, cap)
    assert_equal(gfp, fp, "frame_pos")
    check_written(gcw, buf, fp, cap, "record")


def test_514_records_are_refused(many_core):
    """One record more than max_batch, both calls: MI355_ERR_INVALID and nothing written."""
    buf, counts, escapes = many_head(MANY_MAX)
    R = MANY_MAX + 1
    table = cwire_runs_encode_host(buf, counts, escapes, SN, lib.RUNS_WHERE_SMALLER)[0]
    src = Guarded(buf.size, torch.uint8, data=np.array(buf))
    forms, pos, out = Guarded(4 * R, torch.int32), Guarded(R + 1, torch.int64), Guarded(buf.size)
    torch.cuda.synchronize()
    one_more = lambda a: np.concatenate([a, np.zeros_like(a[:1])])
    with pytest.raises(lib.Mi355Error) as err:
        many_core.cwire_runs_encode_batch(src.ptr, one_more(counts), one_more(escapes), R, lib.RUNS_WHERE_SMALLER, forms.ptr, pos.ptr,
                                          out.ptr, buf.size)
    assert err.value.code == lib.ERR_INVALID
    with pytest.raises(lib.Mi355Error) as err:
        many_core.cwire_runs_decode_batch(src.ptr, one_more(table), R, pos.ptr, out.ptr, buf.size)
    assert err.value.code == lib.ERR_INVALID
    many_core.synchronize()
    assert (forms.get() == -7).all() and (pos.get() == -3).all() and (out.get() == GUARD).all() and np.array_equal(src.get(), buf)


# ---- c. a key frame of 257 tiles, nothing waited for ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def key_frame_case():
    """Two random states of 592x592 with a few zero bytes -> (states, their key-frame records, counts, escapes, and
    runs_spec.encode of them: forms, pos, link)."""
    S = 2
    rng = np.random.default_rng(592)
    states = rng.integers(1, 256, (S, BN), dtype=np.uint8)
    states[0, 100:140] = 0                                   # gaps inside the key frame
    states[0, 256 * K - 20:256 * K + 20] = 0                 # ... one across the round of chunks
    states[1, 700000:700300] = 0                             # ... and an escaped one
    recs = [np.frombuffer(spec.encode_frame(np.flatnonzero(st), st[np.flatnonzero(st)]), np.uint8) for st in states]
    buf = np.concatenate(recs)
    counts, escapes = spec.headers(buf, S)
    forms, pos, link = rs.encode(buf, S, rs.WHERE_SMALLER)
    assert forms[:, 0].tolist() == [rs.FORM_RUNS] * S and int(escapes[1]) == 1 and (counts > ROUND * K).all(), "257 chunks each"
    return frozen(states, buf, counts, escapes, forms, pos, link)


def test_key_frames_round_trip_without_synchronisation(chunk_core):
    """refresh_cwire_batch (key frames) -> encode -> decode -> apply_multi_cwire_batch on one stream, one synchronisation at the
    end: the receiver holds the sender's states, and the link bytes are runs_spec.encode of the key frames."""
    core, S = chunk_core, 2
    states, buf, counts, escapes, forms_want, pos_want, link_want = key_frame_case()
    sender, receiver = Region(S, BN).put(states), Region(S, BN).put(np.zeros((S, BN), np.uint8))
    cap = cwire_runs_bytes_max(BN, S, 0)
    mask_words = -(-(-(-BN // K)) // 32)
    mask, off, fpos, cw = Guarded(S * mask_words, torch.int32), Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
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
    assert np.array_equal(pos.get().view(np.uint64), pos_want)
    assert link.get(written=link_want.size)[:link_want.size].tobytes() == link_want.tobytes()
    assert np.array_equal(fpos2.get().view(np.uint64), fpos.get().view(np.uint64))
    assert cw2.get(written=buf.size)[:buf.size].tobytes() == buf.tobytes()
    assert np.array_equal(receiver.get(), states) and np.array_equal(sender.get(), states)


# ---- the despeckle call against its host form, the host form computed once per input ------------------------------------------
def tick_of_seeds(w, h, density, seeds):
    """ds.tick for the streams of the given seeds -> (records, counts, escapes, states after), read-only."""
    pre, frames = (np.stack(z) for z in zip(*[ds.frames_for(w, h, density, s) for s in seeds]))
    return frozen(*ds.tick_of(pre, frames))


def host_form(w, h, recs, counts, escapes, post, need):
    """mi355_cwire_despeckle_host on copies -> (dropped, offsets, frame_pos, records, states [S, n])."""
    states = np.ascontiguousarray(post).copy()
    d, off, pos, out = cwire_despeckle_host(w, h, recs, counts, escapes, states, need)
    return frozen(d, off, pos, out[:int(pos[-1])].copy(), states.reshape(len(need), -1))


def dsp_check(core, w, h, tick, need, want, **layout):
    """One call on guarded buffers against the host form's result `want`."""
    recs, counts, escapes, post = tick
    got = dsp_run(core, w, h, recs, counts, escapes, post, need, **layout)
    what = (w, h, len(need), layout)
    end = int(want[2][-1])
    assert np.array_equal(got[0], want[0]), (what, "dropped", np.flatnonzero(got[0] != want[0])[:8])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (what, "offsets or frame_pos")
    assert np.array_equal(got[3][:end], want[3]), (what, "the records")
    assert (got[3][end:] == GUARD).all(), (what, "written behind the last record")
    assert np.array_equal(got[4], want[4]), (what, "the states", np.flatnonzero((got[4] != want[4]).any(axis=1))[:8])


def spec_results(w, h, tick, need):
    """despeckle_spec.despeckle per stream -> [(dropped, kept entries, the stream's record as bytes)]."""
    recs, counts, escapes, post = tick
    d, off, pos, out, states, keeps = ds.despeckle(w, h, recs, post, need)
    return [(int(d[s]), int(off[s + 1] - off[s]), out[int(pos[s]):int(pos[s + 1])].tobytes()) for s in range(len(need))]


# ---- d. 129 and 257 streams ---------------------------------------------------------------------------------------------------
DW, DH = 37, 11
STREAMS_MAX = 257
NEED_AT = {127: 0, 128: 3, 129: 0, 255: 5, 256: 1}
STREAM_DENSITIES = (0.3, 0.7)


def needs_of(S):
    need = (np.arange(S) * 5 + 3) % 9
    for s, v in NEED_AT.items():
        if s < S:
            need[s] = v
    return need.astype(np.uint32)


def second_needs_of(S):
    """needs_of moved on by 1 + 3 * (s // 128): no stream from 128 on holds the need of stream s - 128 or of stream s % 128."""
    return ((needs_of(S) + 1 + 3 * (np.arange(S) // INIT_STREAMS)) % 9).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def stream_case(density):
    """37x11, 257 streams of one density -> (the tick, need[257], a second set of needs).  Asserted from despeckle_spec: given
    the need of stream s - 128, or of stream s % 128, each of the streams 129, 255 and 256 -- the first stream behind a launch's
    first, and the last stream of the second and of the third launch -- gives another record, and so do most streams from 128 on.
    Stream 128 itself cannot tell: the need it is given, 3, is stream 0's, and at 129 streams it is the second launch's only
    stream.  So every call runs a second time with second_needs_of, under which stream 128 tells as well."""
    S = STREAMS_MAX
    tick = tick_of_seeds(DW, DH, density, range(S))
    need, need2 = needs_of(S), second_needs_of(S)
    assert list(need[[127, 128, 129, 255, 256]]) == [0, 3, 0, 5, 1] and need[128] == need[0]
    late = np.arange(INIT_STREAMS, S)
    assert (need2[late] != need2[late - INIT_STREAMS]).all() and (need2[late] != need2[late % INIT_STREAMS]).all() and need2.max() <= 8
    for nd, tells in ((need, {129, 255, 256}), (need2, {128, 129, 256})):
        right = spec_results(DW, DH, tick, nd)
        for wrong_of in (lambda s: s - INIT_STREAMS, lambda s: s % INIT_STREAMS):
            wrong = nd.copy()
            for s in range(INIT_STREAMS, S):
                wrong[s] = nd[wrong_of(s)]
            got = spec_results(DW, DH, tick, wrong)
            assert got[:INIT_STREAMS] == right[:INIT_STREAMS]
            same = {s for s in range(INIT_STREAMS, S) if got[s] == right[s]}
            assert not tells & same, (tells & same)
            assert len(same) < (S - INIT_STREAMS) // 4, "most streams tell"
    frozen(need, need2)
    return tick, need, need2


def stream_head(tick, S):
    recs, counts, escapes, post = tick
    end = int(sum(spec.frame_bytes(n, e) for n, e in zip(counts[:S], escapes[:S])))
    return recs[:end], counts[:S], escapes[:S], post[:S]


@functools.lru_cache(maxsize=None)
def stream_want(density, S, second):
    tick = stream_case(density)[0]
    return host_form(DW, DH, *stream_head(tick, S), stream_case(density)[1 + second][:S])


@pytest.fixture(scope="module")
def stream_core():
    with CUDACore(DW, DH, max_batch=STREAMS_MAX, threshold=ds.THR) as core:
        yield core


@pytest.mark.parametrize("density", STREAM_DENSITIES)
@pytest.mark.parametrize("S", [129, 257])
def test_streams_past_the_init_launches(stream_core, S, density):
    """129 streams: the second launch of k_dsp_init holds one need; 257: the third.  Both sets of needs, one call after the
    other on one core; at density 0.7 and 257 streams once more with the states 1225 bytes apart (N = 1221) behind a skew of 3."""
    tick = stream_case(density)[0]
    head = stream_head(tick, S)
    for second in (0, 1):
        need, want = stream_case(density)[1 + second][:S], stream_want(density, S, second)
        dsp_check(stream_core, DW, DH, head, need, want)
        if (S, density) == (257, 0.7):
            dsp_check(stream_core, DW, DH, head, need, want, stride=1225, skew=3)


# ---- e. two and three blocks of k_dsp_init --------------------------------------------------------------------------------------
BLOCK_SHAPES = {2: (509, 258), 3: (643, 409)}         # blocks of k_dsp_init's grid.y: (w, h)
NEED_A, NEED_B = (3, 5), (1, 2)


def changed_mask(w, h, xs, diff):
    """The pixels that hold a live entry, bool [w * h]."""
    mask = np.zeros(w * h, bool)
    mask[np.asarray(xs, np.int64)[np.asarray(diff) != 0] // 3] = True
    return mask


def keep_with_stale(w, h, xs, diff, need, stale):
    """despeckle_spec.keep_entries with the changed bitmap ORed onto `stale` (bool [w * h]) before the neighbours are counted:
    what k_dsp_keep gives when k_dsp_init left those bits of an earlier call standing."""
    xs, diff = np.asarray(xs, np.int64), np.asarray(diff, np.uint8)
    live = diff != 0
    c = ds.neighbour_count((changed_mask(w, h, xs, diff) | stale).reshape(h, w)).reshape(-1)
    return live & (c[xs // 3] >= need)


def block_of_pixel(p, blocks):
    """The block of k_dsp_init that zeroes pixel p's bitmap word: word i is block (i >> 8) % blocks's."""
    return ((np.asarray(p) >> 5) >> 8) % blocks


def streams_of(tick, S):
    recs, counts, escapes, post = tick
    off, xs, df = spec.decode(recs, S)
    return [(xs[int(off[s]):int(off[s + 1])].astype(np.int64), df[int(off[s]):int(off[s + 1])]) for s in range(S)]


@functools.lru_cache(maxsize=None)
def block_case(blocks):
    """-> (w, h, tick A of density 0.7, tick B of density 0.05), two streams each.  Asserted from despeckle_spec: the bitmap has
    `blocks` blocks' worth of words, and for both streams and every block k there are pixels of B, in words that block k
    zeroes, that the reference drops and that A's changed bits, were they still set, would keep."""
    w, h = BLOCK_SHAPES[blocks]
    nwords = (w * h + 31) // 32
    assert nwords // INIT_WORDS + 1 == blocks and nwords >= (blocks - 1) * INIT_WORDS
    A, B = tick_of_seeds(w, h, 0.7, (0, 1)), tick_of_seeds(w, h, 0.05, (0, 1))
    for s, ((xa, da), (xb, db)) in enumerate(zip(streams_of(A, 2), streams_of(B, 2))):
        stale = changed_mask(w, h, xa, da)
        right = ds.keep_entries(w, h, xb, db, NEED_B[s])
        wrong = keep_with_stale(w, h, xb, db, NEED_B[s], stale)
        turned = (db != 0) & ~right & wrong
        assert not (right & ~wrong).any() and turned.any()
        hit = np.bincount(block_of_pixel(xb[turned] // 3, blocks), minlength=blocks)
        assert (hit > 0).all(), (blocks, s, hit)
    return (w, h) + (A, B)


@pytest.mark.parametrize("blocks", sorted(BLOCK_SHAPES))
def test_a_sparse_call_between_two_dense_ones(blocks):
    """Call A (density 0.7), call B (density 0.05, need [1, 2]) and A again on one core and the same stream slots, each equal to
    the host form: a block of k_dsp_init that does not run, or strides wrongly, leaves A's bits in B's bitmap and B keeps
    entries the reference drops."""
    w, h, A, B = block_case(blocks)
    want_a, want_b = host_form(w, h, *A, NEED_A), host_form(w, h, *B, NEED_B)
    assert want_b[0].all() and want_a[0].all(), "every stream drops entries in both calls"
    with CUDACore(w, h, max_batch=2, threshold=ds.THR) as core:
        dsp_check(core, w, h, A, NEED_A, want_a)
        dsp_check(core, w, h, B, NEED_B, want_b)
        dsp_check(core, w, h, A, NEED_A, want_a)


# ---- f. narrow and word-aligned widths ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def narrow_case(shape, density):
    """ds.tick of two streams; at need 3 and density 0.7 the reference keeps and drops entries in both streams."""
    w, h = shape
    tick = tuple(ds.tick(w, h, density, 2)[2:])
    if density == 0.7:
        for dropped, kept, _ in spec_results(w, h, tick, [3, 3]):
            assert kept > 0 and dropped > 0, (shape, kept, dropped)
    return tick


@pytest.mark.parametrize("shape", ds.NARROW, ids=lambda s: "%dx%d" % s)
def test_narrow_and_word_aligned_widths(shape):
    """Every need at both densities against the host form: words that hold several rows, exactly one row, and rows that end one
    pixel before, on and one pixel behind a word."""
    w, h = shape
    with CUDACore(w, h, max_batch=2, threshold=ds.THR) as core:
        for density in (0.3, 0.7):
            tick = narrow_case(shape, density)
            for need in range(9):
                want = host_form(w, h, *tick, [need, need])
                dsp_check(core, w, h, tick, [need, need], want)
                if need == 0:
                    assert not want[0].any() and np.array_equal(want[3], tick[0])
                if (need, density) == (3, 0.7):
                    assert want[0].all() and (np.diff(want[1].astype(np.int64)) > 0).all(), "kept and dropped, in the host form too"


# ---- 4. link positions past 4 GiB on the encoder's output ---------------------------------------------------------------------
LW, LH = 1000, 700
LN = 3 * LW * LH              # 2 100 000
LR = 1400                     # records
L_ENTRIES = LN // 2           # 1 050 000: `alternating`
L_IN, L_OUT = 8 + 2 * L_ENTRIES, 12 + 3 * L_ENTRIES
FIRST_PAST = 1364             # the first record that starts past 2^32 on the link (record 1363 lies across it)


@functools.lru_cache(maxsize=None)
def link_templates():
    """(the compact record of arange(0, N, 2), its run form) from runs_spec: everything but the differences of any record of the
    large link, which lie in the last n bytes of either."""
    xs = np.arange(0, LN, 2)
    rec = rs.record(xs, 0)
    run, r = rs.to_runs(rec)
    run = np.frombuffer(run, np.uint8)
    n = L_ENTRIES
    assert xs.size == n and n % 4 == 0 and r == n and rec.size == L_IN == 2100008 and run.size == L_OUT == 3150012
    assert np.array_equal(rec[L_IN - n:], run[L_OUT - n:]), "the differences end both forms"
    other = np.frombuffer(rs.to_runs(rs.record(xs, 1))[0], np.uint8)
    assert np.array_equal(other[:L_OUT - n], run[:L_OUT - n]) and not np.array_equal(other[L_OUT - n:], run[L_OUT - n:])
    assert LR * L_IN < 1 << 32 < LR * L_OUT
    assert (FIRST_PAST - 1) * L_OUT < 1 << 32 <= FIRST_PAST * L_OUT, "pos[1364] is the first position past 2^32"
    assert -(-r // RUNS) == 1026, "1026 decode workgroups a record: five rounds of k_cwr_dscan"
    return frozen(rec, run)


def diff_bytes(a, b):
    """Record b's differences are all 1 + b % 251: the column of rows a .. b, on the device."""
    return (1 + torch.arange(a, b, device=DEV) % 251).to(torch.uint8)[:, None]


@pytest.fixture(scope="module")
def link_core():
    with CUDACore(LW, LH, max_batch=LR) as core:
        yield core


def test_link_positions_past_4_gib(link_core):
    """1400 records of 1 050 000 single-entry runs under RUNS_ALWAYS: 2.94 GB in, 4.41 GB out, compared on the device in slices
    with the run-form template; again with a capacity that ends four bytes short of record 1364's end (records 1364 to 1399
    skipped whole, everything from pos[1364] on still the pattern); then the link decoded (in_pos past 2^32) against the input."""
    rec_t, run_t = link_templates()
    n, R = L_ENTRIES, LR
    require(2 * BigGuarded.bytes_needed(R * L_IN) + BigGuarded.bytes_needed(R * L_OUT) + (8 << 30))
    counts, escapes = np.full(R, n, np.uint32), np.zeros(R, np.uint32)
    table = np.tile(np.array([1, n, 0, n], np.uint32), (R, 1))
    src, out, back = BigGuarded(R * L_IN), BigGuarded(R * L_OUT), None
    try:
        rows_in, rows_out = src.t.view(R, L_IN), out.t.view(R, L_OUT)
        head_in, head_out = to_dev(rec_t[:L_IN - n]), to_dev(run_t[:L_OUT - n])
        for a, b in slices(R, L_IN):
            rows_in[a:b, :L_IN - n] = head_in
            rows_in[a:b, L_IN - n:] = diff_bytes(a, b)
        want_pos = L_OUT * np.arange(R + 1, dtype=np.uint64)

        def unchanged():
            src.check()
            for a, b in slices(R, L_IN):
                assert_rows_on_device(rows_in[a:b, :L_IN - n], head_in, "the input: header and codes", a)
                assert_rows_on_device(rows_in[a:b, L_IN - n:], diff_bytes(a, b).expand(-1, n), "the input: diff", a, L_IN - n)

        for fit in (R, FIRST_PAST):
            cap = R * L_OUT if fit == R else (FIRST_PAST + 1) * L_OUT - 4
            forms, pos = Guarded(4 * R, torch.int32), Guarded(R + 1, torch.int64)
            out.buf.fill_(GUARD)
            torch.cuda.synchronize()
            link_core.cwire_runs_encode_batch(src.ptr, counts, escapes, R, lib.RUNS_ALWAYS, forms.ptr, pos.ptr, out.ptr, cap)
            link_core.synchronize()
            assert_equal(forms.get().view(np.uint32).reshape(R, 4), table, "forms")
            assert_equal(pos.get().view(np.uint64), want_pos, "pos")
            out.check(written=fit * L_OUT)
            for a, b in slices(fit, L_OUT):
                assert_rows_on_device(rows_out[a:b, :L_OUT - n], head_out, "the link: header, gap and len", a)
                assert_rows_on_device(rows_out[a:b, L_OUT - n:], diff_bytes(a, b).expand(-1, n), "the link: diff", a, L_OUT - n)
            unchanged()
        # ... and back: the expected link, rebuilt from the template, decoded
        out.buf.fill_(GUARD)
        for a, b in slices(R, L_OUT):
            rows_out[a:b, :L_OUT - n] = head_out
            rows_out[a:b, L_OUT - n:] = diff_bytes(a, b)
        back = BigGuarded(R * L_IN)
        fpos = Guarded(R + 1, torch.int64)
        torch.cuda.synchronize()
        link_core.cwire_runs_decode_batch(out.ptr, table, R, fpos.ptr, back.ptr, R * L_IN)
        link_core.synchronize()
        assert_equal(fpos.get().view(np.uint64), L_IN * np.arange(R + 1, dtype=np.uint64), "frame_pos")
        back.check()
        rows_back = back.t.view(R, L_IN)
        for a, b in slices(R, L_IN):
            assert_rows_on_device(rows_back[a:b], rows_in[a:b], "the decoded records", a)
        out.check()
        for a, b in slices(R, L_OUT):
            assert_rows_on_device(rows_out[a:b, :L_OUT - n], head_out, "the link is only read", a)
            assert_rows_on_device(rows_out[a:b, L_OUT - n:], diff_bytes(a, b).expand(-1, n), "the link is only read", a, L_OUT - n)
        unchanged()
    finally:
        for g in (src, out, back):
            if g is not None:
                g.free()
        torch.cuda.empty_cache()

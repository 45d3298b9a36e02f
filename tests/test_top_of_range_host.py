"""CPU: the inputs of test_top_of_range_gpu.py.  Every builder of that file asserts, from the layout rules and the reference
alone, that its input reaches the seam it is named for; this file calls each of them, so those assertions run where there is
no GPU.  It also proves that the inputs of Part 1 discriminate (a wrong rule applied to the reference is a mismatch), checks
the plain statement that is Part 3's reference against pyoracle and cwire_spec at T = 4, asserts mi355_create's bounds for
Part 2's shape through the library, and runs the device-side comparison helpers of gpu_util on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import cwire_spec as spec
import test_top_of_range_gpu as top
from cudavideostream_amd import lib
from oracle import pyoracle as po
from gpu_util import PAD, BigGuarded, assert_same_on_device, oracle_pairs

GRID, THR = top.GRID, top.THR


# ---- Part 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,T", top.COUNT_CASES)
def test_stream_inputs_cross_the_count(w, h, T):
    base, frames, refs, states = top.stream_case(w, h, T)
    assert frames.shape == (T, 3 * w * h) and refs[0].off.size == T + 1


@pytest.mark.parametrize("w,h", top.SMALL)
@pytest.mark.parametrize("T", top.COUNTS)
def test_pair_inputs_cross_the_count(w, h, T):
    cur, prev, ref = top.pairs_case(w, h, T)
    assert cur.shape == prev.shape == (T, 3 * w * h) and ref.off.size == T + 1


@pytest.mark.parametrize("w,h", top.SMALL)
@pytest.mark.parametrize("S,K", [(S, 1) for S in top.COUNTS] + [sk for sk in top.MULTI_STREAM if sk[1] != 1])
def test_multi_inputs_cross_the_count(w, h, S, K):
    frames, pre, ref, post = top.multi_stream_case(w, h, S, K)
    assert frames.shape[0] == S * K >= GRID and pre.shape == post.shape == (S, 3 * w * h) and ref.off.size == S * K + 1


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


WRONG = {
    "the frame index modulo 65536": lambda t: t % 65536,
    "a second grid whose frame pointer is not advanced": lambda t: np.where(t >= GRID, t - GRID, t),
}


@pytest.mark.parametrize("w,h,T", [(33, 7, 65537), (16, 4, 65537), (5, 1, 2 * 65536 + 1)])
def test_the_stream_inputs_discriminate(w, h, T):
    """The test of the tests: each wrong rule a split (or unsplit) launch could follow, applied to the reference, gives other
    offsets, entries or states than test_counts_stream expects."""
    n = 3 * w * h
    base, frames, refs, states = top.stream_case(w, h, T)
    want = (refs[0].off, refs[0].xs, refs[0].df, states[0])
    for name, rule in WRONG.items():
        got = po.diff_stream(top.pool_frames(n, T, rule), base, THR)
        assert not same(got[:3], want[:3]), name
    off = refs[0].off.astype(np.int64)
    seg = lambda t: (refs[0].xs[off[t]:off[t + 1]].tobytes(), refs[0].df[off[t]:off[t + 1]].tobytes())
    # an output pointer that is not advanced: frame 65535 + t would be written where frame t is
    assert any(seg(GRID + t) != seg(t) for t in range(T - GRID)), "a second grid whose output pointer is not advanced"
    # a slice that does not run: its entries are missing and the state stays where the slice before left it
    first = po.diff_stream(frames[:GRID], base, THR)
    assert off[T] > off[GRID] and not np.array_equal(first[3], states[0]), "a slice that does not run"
    # a slice that runs twice: the second pass starts from the state the first one left
    again = po.diff_stream(frames[:GRID], first[3], THR)
    assert same(first[:3], (refs[0].off[:GRID + 1], refs[0].xs[:off[GRID]], refs[0].df[:off[GRID]])) and not same(again[:3], first[:3]), \
        "a slice that runs twice"


@pytest.mark.parametrize("w,h", top.SMALL)
def test_the_multi_inputs_discriminate(w, h):
    """65537 streams: a state (or frame) index taken modulo 65536 or not advanced in a second grid reads another picture, and
    its stream's entries and state afterwards differ."""
    n, S = 3 * w * h, 65537
    frames, pre, ref, post = top.multi_stream_case(w, h, S, 1)
    off = ref.off.astype(np.int64)
    assert all(int(rule(np.array([S - 1]))[0]) != S - 1 for rule in WRONG.values())
    for name, rule in WRONG.items():
        for s in range(GRID, S):
            j = int(rule(np.array([s]))[0])
            if j == s:
                continue          # (65535 modulo 65536)
            c, xs, df, st = po.diff_pack(frames[s], pre[j], THR)
            assert not (np.array_equal(xs, ref.xs[off[s]:off[s + 1]]) and np.array_equal(df, ref.df[off[s]:off[s + 1]])), (name, s, "state")
            c, xs, df, st = po.diff_pack(frames[j], pre[s], THR)
            assert not (np.array_equal(xs, ref.xs[off[s]:off[s + 1]]) and np.array_equal(df, ref.df[off[s]:off[s + 1]])), (name, s, "frame")
            assert not np.array_equal(post[j], post[s]), (name, s, "a state written to the wrong place")


def test_one_flat_oracle_call_equals_the_oracle_pair_by_pair():
    """flat_oracle lays S pairs end to end for ONE pyoracle.diff_pack call: the same entries and states as S calls."""
    n, S = 693, 300
    cur, prev = top.pool_frames(n, S), top.pool_states(n, S)
    off, xs, df, st = top.flat_oracle(cur, prev)
    w_off, w_xs, w_df = oracle_pairs(po, cur, prev, THR)
    assert np.array_equal(off, w_off) and np.array_equal(xs, w_xs) and np.array_equal(df, w_df)
    assert all(np.array_equal(st[s], po.diff_pack(cur[s], prev[s], THR)[3]) for s in range(S))


# ---- Part 2 ---------------------------------------------------------------------------------------------------------------------
def test_the_record_log_rule():
    """record_log on cases small enough to read: 64 records fill a chunk, a frame that does not fit skips the rest of it."""
    nt = 7
    assert list(top.record_log([64, 64, 64], 2, nt)) == [2048, 2048 + nt * 1024, 2048 + 2 * nt * 1024]
    assert list(top.record_log([50, 50, 14, 1], 0, nt)) == [0, nt * 1024, nt * 1024 + 800, 2 * nt * 1024]
    assert list(top.record_log([0, 3, 0, 61, 1], 1, nt)) == [1024, 1024, 1072, 1072, 1024 + nt * 1024]


@pytest.mark.parametrize("T", [top.T_LOW, top.T_TOP])
def test_dense_inputs_reach_the_log_offsets(T):
    case = top.dense_case(T)
    assert case["vals"].shape == (T, 4 * 1024 + 800) and case["states"].shape[0] == -(-T // top.MULTI[1]) + 1
    a, b = case["refs"]
    k = int(a.off[top.SLAB])        # the second batch meets the last frame's state: other entries in its first slab only
    assert not np.array_equal(a.df[:k], b.df[:int(b.off[top.SLAB])]) and np.array_equal(a.df[k:], b.df[int(b.off[top.SLAB]):])
    assert np.array_equal(a.off, b.off) == (T % 2 == 0), "an odd T ends in the first frame's band: not every byte of frame 0 is flagged again"
    if T == top.T_LOW:
        assert case["states"].shape[0] == top.MULTI[0] + 1 and np.array_equal(case["states"][-1], case["final"])
        assert np.array_equal(case["pairs"].off, case["refs"][0].off) and np.array_equal(case["pairs"].xs, case["refs"][0].xs)


def test_create_accepts_the_dense_shape_up_to_2045_frames():
    """mi355_create itself: 1000x700 is refused at max_batch 2046 and passes validation at 2045 and at 1023, the least
    max_batch whose record log reaches 2^31 bytes (without a GPU, past validation means MI355_ERR_HIP)."""
    L = lib.load()
    assert top.NT == 2051 and 1022 * top.NT * 1024 < 1 << 31 <= 1023 * top.NT * 1024
    for max_batch, ok in ((1023, True), (2045, True), (2046, False)):
        assert top.accepted(max_batch) == ok
        h, cfg = C.c_void_p(), lib.Config(top.BW, top.BH, THR, max_batch, -1, 0, 0, 0)
        rc = L.mi355_create(C.byref(cfg), C.byref(h))
        if ok:
            assert rc == (lib.OK if torch.cuda.is_available() else lib.ERR_HIP), (max_batch, rc, L.mi355_last_error())
            if rc == lib.OK:
                L.mi355_destroy(h)
        else:
            assert rc == lib.ERR_INVALID and b"2^32" in L.mi355_last_error() and not h.value


# ---- Part 3 ---------------------------------------------------------------------------------------------------------------------
def test_the_plain_statement_equals_the_oracle_at_four_frames():
    """Part 3's reference -- entries arange(N), diff = frame[t] - frame[t - 1], the state the last frame; wire frames and records
    that are the templates with those differences in their last N bytes -- against pyoracle, po.wire_pack and cwire_spec."""
    T, n = 4, top.N
    base = top.every_byte_base()
    frames = np.stack([top.every_byte_frame(t) for t in range(T)])
    ref, state = top.every_byte_reference(base, frames)
    off, xs, df, st = po.diff_stream(frames, base, THR)
    assert np.array_equal(ref.off, off) and np.array_equal(ref.xs, xs) and np.array_equal(ref.df, df) and np.array_equal(state, st)
    wire_t, rec_t = top.templates()
    recs, pos = spec.encode(off, xs, df)
    assert np.array_equal(pos, top.REC * np.arange(T + 1, dtype=np.uint64))
    wire = po.wire_pack(off, xs, df)
    for t in range(T):
        d = df[t * n:(t + 1) * n]
        assert np.array_equal(recs[t * top.REC:(t + 1) * top.REC], np.concatenate([rec_t[:top.REC - n], d]))
        assert np.array_equal(wire[t * top.WIRE:(t + 1) * top.WIRE], np.concatenate([wire_t[:top.WIRE - n], d]))
    counts, escapes = spec.headers(recs, T)
    assert np.array_equal(counts, top.dense_headers(T)[0]) and np.array_equal(escapes, top.dense_headers(T)[1])
    top.every_byte_seams(top.T_LOW)


def test_the_run_form_template_is_the_spec():
    """runs_template asserts its figures from runs_spec.to_runs; a record of Part 3 with real differences is the template's head
    and then those differences, and decodes to the compact record -- what test_every_byte_runs_* compare with on the device."""
    import runs_spec as rs
    run_t, r = top.runs_template()
    rec_t = top.templates()[1]
    diff = top.every_byte_frame(1) - top.every_byte_frame(0)
    rec = np.concatenate([rec_t[:top.REC - top.N], diff])
    run, r2 = rs.to_runs(rec)
    assert r2 == r and run == np.concatenate([run_t[:run_t.size - top.N], diff]).tobytes() and rs.from_runs(run) == rec.tobytes()
    forms, pos, link = rs.encode(np.concatenate([rec, rec_t]), 2, rs.WHERE_SMALLER)
    assert forms.tolist() == [[1, top.N, 0, r]] * 2 and pos.tolist() == [0, run_t.size, 2 * run_t.size]


def test_the_split_template_is_the_spec():
    """split_template asserts its layout from split_spec's rule; a record of Part 3 with real differences splits into the
    template's heads, each followed by the matching slice of those differences -- what test_every_byte_split compares with on
    the device -- and the piece positions of the 1100 records pass 2^32 inside record 1022."""
    from cudavideostream_amd import cwire_split_host
    tpos, cuts, tout = top.split_template()
    diff = top.every_byte_frame(1) - top.every_byte_frame(0)
    rec = np.concatenate([top.templates()[1][:top.REC - top.N], diff])
    first, pos, out = cwire_split_host(rec, *top.dense_headers(1), top.N, top.SPLIT_M)
    assert int(first[1]) == len(cuts) and np.array_equal(pos[:len(cuts) + 1].astype(np.int64), tpos)
    for p, (a, b) in enumerate(cuts):
        at, end = int(tpos[p]), int(tpos[p + 1])
        assert np.array_equal(out[at:end - (b - a)], tout[at:end - (b - a)]) and np.array_equal(out[end - (b - a):end], diff[a:b]), p
    OUT = int(tpos[-1])
    r, inside = divmod(1 << 32, OUT)
    assert r == 1022 < top.T_LOW and 0 < int(np.searchsorted(tpos, inside)) < len(cuts)


def test_bands_differ_by_more_than_the_threshold():
    x = np.arange(top.N, dtype=np.int64)
    f = [top.band(t, x) for t in (0, 1, 2, 549, 1098, 1099)]
    assert all(150 <= v.min() and v.max() < 250 for v in (f[0], f[2], f[4])) and all(0 <= v.min() and v.max() < 100 for v in (f[1], f[3], f[5]))
    assert top.every_byte_base().min() >= 101 and top.every_byte_base().max() <= 129
    assert not np.array_equal(f[0], f[2]) and not np.array_equal(f[1], f[5])
    assert np.array_equal(top.band(torch.tensor(7), torch.from_numpy(x)).numpy(), top.band(7, x)), "numpy and torch agree"


# ---- the device-side helpers, on the host -----------------------------------------------------------------------------------------
def test_the_guard_check_of_a_big_buffer_fires():
    g = BigGuarded(1000, torch.int32, device="cpu")
    g.PIECE = 256
    g.check(written=0)
    g.t[:10] = 1
    g.check(written=10)
    with pytest.raises(AssertionError, match="element 9 .* behind the part that was to be written"):
        g.check(written=9)
    for at, name in ((PAD - 1, "before the buffer"), (PAD + 1000, "behind the buffer"), (2 * PAD + 999, "behind the buffer")):
        g.buf[at] = 5
        with pytest.raises(AssertionError, match=rf"element {at - PAD} .* it lies {name}$"):
            g.check()
        g.buf[at] = g.fill
    g.check()


def test_the_comparison_on_the_device_names_the_first_difference():
    a = torch.arange(1000, dtype=torch.uint8)
    b = a.clone()
    assert_same_on_device(a, b, "equal", piece=64)
    b[700], b[900] = 1, 2
    with pytest.raises(AssertionError, match="x: element 700 is 188, the reference's 1$"):
        assert_same_on_device(a, b, "x", piece=64)
    got = torch.zeros(6, 10, dtype=torch.uint8)
    want = torch.zeros(10, dtype=torch.uint8)
    top.assert_rows_on_device(got, want, "rows", 3)
    got[4, 7] = 9
    with pytest.raises(AssertionError, match="rows: frame 7, byte or element 12 is 9, the reference's 0$"):
        top.assert_rows_on_device(got, want, "rows", 3, col0=5)


# ---- Part 3, the consumers: what density implies, against the suite's numpy references at small sizes ----------------------------
def small_burst(w, h, S, K):
    """K frames of each of S streams that change every byte (band()), as records -> (base, frame_of, records, B)."""
    n = 3 * w * h
    base = np.random.default_rng(5).integers(101, 130, n, dtype=np.uint8)
    frame_of = lambda t: top.band(t, np.arange(n, dtype=np.int64)).astype(np.uint8)
    frames = np.stack([frame_of(t) for t in range(S * K)])
    off, xs, df, st = po.diff_stream(frames, base, THR)
    assert np.array_equal(off, n * np.arange(S * K + 1)) and np.array_equal(st, frames[-1])
    return base, frame_of, spec.encode(off, xs, df)[0], (off, xs, df)


def test_density_implies_the_relays_results():
    """dense_coalesced against the coalescer's and the crop's numpy references (decode, sum, select, encode)."""
    from test_cwire_coalesce_gpu import reference as coalesce_reference
    w, h, S, K = 40, 12, 2, 5
    base, frame_of, recs, _ = small_burst(w, h, S, K)
    before, after = top.stream_ends(base, frame_of, S, K)
    want = coalesce_reference(recs, S, K, 3 * w * h)
    assert all(np.array_equal(a, b) for a, b in zip(top.dense_coalesced(before, after, w, h), want))
    rects = np.array([(30, 9, 10, 3), (0, 10, 40, 2)], np.int32)
    want = top.crop.reference(recs, S, K, w, h, rects)
    assert all(np.array_equal(a, b) for a, b in zip(top.dense_coalesced(before, after, w, h, rects), want))
    assert all(int(r[1] + r[3]) == top.BH for r in top.RECTS) and int(top.RECTS[0][0] + top.RECTS[0][2]) == top.BW, "the last rows"


def test_density_implies_the_grids_and_the_tile_masks():
    """dense_activity against the activity oracle on all entries, all_tiles against the entries' tiles, the clean verdict
    against mi355_cwire_check_host, the client's state against mi355_cwire_apply_host."""
    from cudavideostream_amd import cwire_apply_host, cwire_check_host
    w, h, S, K = 40, 37, 2, 5
    n = 3 * w * h
    base, frame_of, recs, (off, xs, df) = small_burst(w, h, S, K)
    cells, summ = top.activity_oracle(w, h, 16, 16, 1, S, K, off.astype(np.uint32), xs)
    got = top.dense_activity(w, h, S, K, (16, 16, 1))
    assert np.array_equal(got[0], cells) and np.array_equal(got[1], summ)
    mask = top.all_tiles(n, S)
    tiles = np.unique(xs // 4096)
    assert tiles.size == top.state_tiles(n) and sum(bin(int(v)).count("1") for v in mask[0]) == tiles.size and np.array_equal(mask[0], mask[1])
    counts, escapes = spec.headers(recs, S * K)
    assert np.array_equal(cwire_check_host(recs, counts, escapes, n), np.tile(np.array([0, 0, n, n], np.uint32), (S * K, 1)))
    state = base.copy()
    assert cwire_apply_host(state, recs, S * K) == recs.size and np.array_equal(state, frame_of(S * K - 1))


def test_the_consumer_table_is_complete():
    """Every entry point of the header that reads compact records is run on the 4.6 GB buffer or excluded with a reason."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355diff.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    readers = [m.group(1) for m in re.finditer(r"\b(mi355_\w+)\s*\(([^;{}]*?)\)\s*;", text)
               if re.search(r"const\s+void\s*\*\s*d_cwire(_in)?\b", m.group(2)) or re.search(r"const\s+uint8_t\s*\*\s*d_cwire(_in)?\b", m.group(2))]
    listed = set(top.CONSUMERS) | set(top.CONSUMERS_EXCLUDED)
    assert len(readers) >= 13 and {"mi355_cwire_runs_encode_batch", "mi355_cwire_despeckle_cwire_batch"} <= set(readers), readers
    for name in top.CONSUMERS:
        assert callable(getattr(top, top.CONSUMERS[name])), name
    covered_elsewhere = {"mi355_cwire_coalesce_batch": "the arrays form of the coalescer: mi355_cwire_coalesce_cwire_batch's kernels with another sink",
                         "mi355_cwire_crop_batch": "the arrays form of the crop: mi355_cwire_crop_cwire_batch's kernels with another sink",
                         "mi355_cwire_mosaic_cwire_batch": "test_top_of_range_mosaic_gpu.test_every_byte_mosaic, on the same buffer",
                         "mi355_cwire_mosaic_batch": "the arrays form of the mosaic: mi355_cwire_mosaic_cwire_batch's kernels with another sink"}
    import test_top_of_range_mosaic_gpu
    assert callable(test_top_of_range_mosaic_gpu.test_every_byte_mosaic)
    for name in readers:
        assert name in listed or name in covered_elsewhere, f"{name} reads compact records and is neither run on the large buffer nor excluded"


def test_the_launcher_table_is_complete():
    """The docstring's table of test_top_of_range_gpu.py against csrc/: every kernel launched on a grid (or with a by-value
    table) sized by a frame, stream or record count is named there -- literally or by a `k_prefix*` row -- and every test the
    table names exists."""
    import glob
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = top.__doc__
    table = doc[doc.index("kernel (launcher)"):doc.index("The three expansion kernels")]
    named = set(re.findall(r"\bk_\w+\*?", table))
    sized = re.compile(r"\b(nframes|nstreams|nrecords|ns|nf|cnt|tiles|grid|g|per_record|per_tile|per_word|part|nr)\b")
    seen = set()
    for path in sorted(glob.glob(os.path.join(root, "cudavideostream_amd", "csrc", "*.hip"))):
        text = open(path).read()
        for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*(k_\w+)(.*?), 0, s\b", text, flags=re.S):
            kernel, grid = m.group(1), m.group(2).split("dim3(256)")[0].split("dim3(64)")[0]
            if not sized.search(grid) and kernel not in ("k_cwire_place", "k_cwc_place", "k_cwr_place", "k_cwire_scan"):
                continue
            seen.add(kernel)
            if os.path.basename(path) == "filters.hip":
                continue          # one row: every kernel there goes through for_frame_grids (or has the frames in grid.x)
            assert kernel in named or any(k.endswith("*") and kernel.startswith(k[:-1]) for k in named), \
                f"{kernel} ({os.path.basename(path)}) is launched on a grid sized by a count and the table does not name it"
    assert {"k_expand", "k_expand_cwire", "k_cwire_items", "k_scan_groups", "k_diff_pack", "k_apply_multi_strided"} <= seen
    assert {"k_cwr_scan", "k_cwr_dscan", "k_cwr_place", "k_cwr_table", "k_cws_table", "k_dsp_init", "k_dsp_mark", "k_dsp_keep",
            "k_dsp_facts", "k_dsp_emit"} <= seen, "the launches of the run-code, split and despeckle calls are read"
    assert "filters.hip" in table and "for_frame_grids" in open(os.path.join(root, "cudavideostream_amd", "csrc", "filters.hip")).read()
    for name in set(re.findall(r"\btest_counts_\w+", table)):
        assert callable(getattr(top, name)), name
    for name in set(re.findall(r"\b(test_\w+_gpu)\b", table)):
        assert os.path.exists(os.path.join(root, "tests", name + ".py")), name
    for module, name in set(re.findall(r"\b(test_\w+_gpu)\.(test_\w+)", table)):
        assert callable(getattr(__import__(module), name)), (module, name)
    for name in set(re.findall(r"(?<![.\w])test_every_byte_\w+", table)):
        assert callable(getattr(top, name)), name

"""CPU: the inputs of test_runs_despeckle_seams_gpu.py.  Every builder of that file asserts, from the numpy statements alone, that
its input reaches the seam it is named for; this file calls each of them, so those assertions run where there is no GPU.  It
holds the host forms (mi355_cwire_runs_encode_host / _decode_host, mi355_cwire_despeckle_host), the references of the GPU
comparisons, to runs_spec and despeckle_spec on those inputs.  And it proves that the inputs discriminate: each mutant below
is the numpy statement with one carry, base or mask forgotten, as a kernel that mishandles the seam would compute it, and on the
chosen input its result differs from the reference's."""
import numpy as np
import pytest

import cwire_spec as spec
import despeckle_spec as ds
import runs_spec as rs
import test_runs_despeckle_seams_gpu as seams
from cudavideostream_amd import cwire_runs_decode_host, cwire_runs_encode_host

K, ROUND, RUNS = seams.K, seams.ROUND, seams.RUNS


# ---- the builders, and the host forms on their inputs ---------------------------------------------------------------------------
def runs_host_forms_are_the_model(buf, counts, escapes, N, policy):
    wf, wp, wo = cwire_runs_encode_host(buf, counts, escapes, N, policy)
    sf, sp, so = rs.encode(buf, counts.size, policy)
    assert np.array_equal(wf, sf) and np.array_equal(wp, sp) and wo[:so.size].tobytes() == so.tobytes()
    fp, cw = cwire_runs_decode_host(so, sf, N)
    mp, mc = rs.decode(so, sf)
    assert np.array_equal(fp, mp) and cw.tobytes() == mc.tobytes() == np.asarray(buf).tobytes()
    return sf


@pytest.mark.parametrize("policy", [rs.WHERE_SMALLER, rs.ALWAYS])
def test_chunk_records_on_the_host(policy):
    names, buf, counts, escapes = seams.chunk_case()
    forms = runs_host_forms_are_the_model(buf, counts, escapes, seams.BN, policy)
    for name, row in zip(names, forms):
        want = seams.CHUNK_FORMS[name]
        assert list(row[1:]) == want[1:] and row[0] == (int(policy == rs.ALWAYS) if want[0] is None else want[0]), name


@pytest.mark.parametrize("R", [257, 513])
def test_many_records_on_the_host(R):
    buf, counts, escapes = seams.many_head(R)
    assert counts.size == R
    forms = runs_host_forms_are_the_model(buf, counts, escapes, seams.SN, rs.WHERE_SMALLER)
    assert 0 < int(forms[:, 0].sum()) < R


def test_key_frames_on_the_host():
    states, buf, counts, escapes, forms, pos, link = seams.key_frame_case()
    runs_host_forms_are_the_model(buf, counts, escapes, seams.BN, rs.WHERE_SMALLER)
    assert 0.5 < int(pos[-1]) / buf.size < 0.52


def test_link_templates():
    rec, run = seams.link_templates()
    assert rs.from_runs(run) == rec.tobytes()


def despeckle_host_form_is_the_model(w, h, tick, need):
    recs, counts, escapes, post = tick
    d, off, pos, out, states = seams.host_form(w, h, recs, counts, escapes, post, need)
    wd, woff, wpos, wout, wstates, _ = ds.despeckle(w, h, recs, post, need)
    assert np.array_equal(d, wd) and np.array_equal(off, woff) and np.array_equal(pos, wpos)
    assert np.array_equal(out, wout) and np.array_equal(states, wstates)
    return wd, woff


@pytest.mark.parametrize("density", seams.STREAM_DENSITIES)
def test_stream_cases_on_the_host(density):
    tick, need, need2 = seams.stream_case(density)
    for S in (129, 257):
        for nd in (need, need2):
            despeckle_host_form_is_the_model(seams.DW, seams.DH, seams.stream_head(tick, S), nd[:S])


@pytest.mark.parametrize("blocks", sorted(seams.BLOCK_SHAPES))
def test_block_cases_on_the_host(blocks):
    w, h, A, B = seams.block_case(blocks)
    despeckle_host_form_is_the_model(w, h, B, seams.NEED_B)


@pytest.mark.parametrize("shape", ds.NARROW, ids=lambda s: "%dx%d" % s)
def test_narrow_cases_on_the_host(shape):
    w, h = shape
    for density in (0.3, 0.7):
        tick = seams.narrow_case(shape, density)
        for need in range(9):
            wd, woff = despeckle_host_form_is_the_model(w, h, tick, [need, need])
            if (need, density) == (3, 0.7):
                assert wd.all() and (np.diff(woff.astype(np.int64)) > 0).all()


# ---- the mutants ------------------------------------------------------------------------------------------------------------
def scan_with_restarts(sums, restarts):
    """The exclusive scan of `sums` whose carry is forgotten in front of every index of `restarts`."""
    before = np.cumsum(sums) - sums
    out = before.copy()
    for at in restarts:
        if at < sums.size:
            out[at:] = before[at:] - before[at]
    return out


def run_sections(code, restarts=()):
    """gap[] and len[] as k_cwr_count / k_cwr_scan / k_cwr_emit place them: a chunk's runs at the chunk's first rank (the scan
    of the chunks' counts) plus their rank in the chunk; -1 where nothing was written."""
    code = np.asarray(code, np.uint8)
    gap, ln = rs.runs_of(code)
    start = np.flatnonzero((code != 0) | (np.arange(code.size) % 256 == 0))
    chunk = start // K
    counts = np.bincount(chunk, minlength=-(-code.size // K))
    right, first = scan_with_restarts(counts, ()), scan_with_restarts(counts, restarts)
    at = first[chunk] + (np.arange(start.size) - right[chunk])
    g, l = np.full(gap.size, -1), np.full(gap.size, -1)
    g[at], l[at] = gap, ln
    return g, l


def expanded_codes(gap, ln, n, restarts=()):
    """code[n] as k_cwr_sums / k_cwr_dscan / k_cwr_expand place it: a workgroup's 1024 runs from the workgroup's first entry (the
    scan of the workgroups' sums) on."""
    L = ln.astype(np.int64) + 1
    wg = np.arange(gap.size) // RUNS
    sums = np.bincount(wg, L).astype(np.int64)
    right, first = scan_with_restarts(sums, ()), scan_with_restarts(sums, restarts)
    at = first[wg] + (np.cumsum(L) - L - right[wg])
    code = np.zeros(n, np.uint8)
    code[at] = gap                                            # (in order: a later workgroup overwrites an earlier one)
    return code


def test_run_ranks_that_restart_at_chunk_256_are_another_record():
    names, buf, counts, escapes = seams.chunk_case()
    at = 0
    for name, n, e in zip(names, counts, escapes):
        size = spec.frame_bytes(int(n), int(e))
        code = rs.sections(buf[at:at + size])[2]
        at += size
        gap, ln = rs.runs_of(code)
        g, l = run_sections(code)
        assert np.array_equal(g, gap) and np.array_equal(l, ln), "the model without a mutation is runs_spec"
        if -(-int(n) // K) > ROUND:
            mg, ml = run_sections(code, (ROUND,))
            differs = not (np.array_equal(mg, gap) and np.array_equal(ml, ln))
            assert differs, name
            if name == "holes":
                assert not np.array_equal(mg[mg >= 0], gap[mg >= 0]), "not only by the unwritten runs: a gap lands on another"


def test_entry_offsets_that_restart_at_workgroup_256_or_512_are_another_record():
    names, buf, counts, escapes = seams.chunk_case()
    at = 0
    for name, n, e in zip(names, counts, escapes):
        size = spec.frame_bytes(int(n), int(e))
        code = rs.sections(buf[at:at + size])[2]
        at += size
        gap, ln = rs.runs_of(code)
        assert np.array_equal(expanded_codes(gap, ln, int(n)), code), "the model without a mutation is runs_spec"
        if name == "alternating":
            for restarts in ((ROUND,), (2 * ROUND,), (ROUND, 2 * ROUND)):
                assert not np.array_equal(expanded_codes(gap, ln, int(n), restarts), code), restarts
    assert "alternating" in names


@pytest.mark.parametrize("R", [257, 513])
def test_positions_that_restart_at_record_256_are_other_positions(R):
    buf, counts, escapes = seams.many_head(R)
    forms, pos, link = rs.encode(buf, R, rs.WHERE_SMALLER)
    sizes = np.diff(pos.astype(np.int64))
    assert np.array_equal(scan_with_restarts(sizes, ()), pos[:-1].astype(np.int64))
    for restarts in ((ROUND,), (2 * ROUND,)):
        if restarts[0] < R:
            wrong = scan_with_restarts(sizes, restarts)
            assert wrong[restarts[0]] == 0 != pos[restarts[0]] and not np.array_equal(wrong, pos[:-1].astype(np.int64))
    fp, _ = rs.decode(link, forms)
    assert scan_with_restarts(np.diff(fp.astype(np.int64)), (ROUND,))[ROUND] != fp[ROUND]


@pytest.mark.parametrize("density", seams.STREAM_DENSITIES)
def test_a_need_taken_modulo_128_is_another_result(density):
    """At 257 streams with the needs as given; at 129 streams, whose second launch is stream 128 alone, with the second set of
    needs, in which stream 128 does not repeat stream 0."""
    tick, need, need2 = seams.stream_case(density)
    for S, nd in ((257, need), (257, need2), (129, need2)):
        head = seams.stream_head(tick, S)
        right = seams.spec_results(seams.DW, seams.DH, head, nd[:S])
        wrong = seams.spec_results(seams.DW, seams.DH, head, nd[np.arange(S) % seams.INIT_STREAMS])
        assert right != wrong and right[S - 1] != wrong[S - 1], "the last stream, the only one of its launch, differs"


@pytest.mark.parametrize("blocks", sorted(seams.BLOCK_SHAPES))
def test_a_block_of_the_bitmap_that_keeps_its_bits_is_another_result(blocks):
    """A's changed bits left in the words of ONE block of k_dsp_init, for every block and both streams: B keeps entries the
    reference drops."""
    w, h, A, B = seams.block_case(blocks)
    for s, ((xa, da), (xb, db)) in enumerate(zip(seams.streams_of(A, 2), seams.streams_of(B, 2))):
        right = ds.keep_entries(w, h, xb, db, seams.NEED_B[s])
        for k in range(blocks):
            stale = seams.changed_mask(w, h, xa, da) & (seams.block_of_pixel(np.arange(w * h), blocks) == k)
            wrong = seams.keep_with_stale(w, h, xb, db, seams.NEED_B[s], stale)
            assert (wrong & ~right).any(), (blocks, s, k)


def linear_keep(w, h, xs, diff, need, first, last):
    """keep_entries as k_dsp_keep computes it: the eight neighbours by shifts of the LINEAR bitmap of w * h pixels (distance 1
    and w - 1, w, w + 1), the left ones masked where `first` is set, the right ones where `last` is."""
    xs, diff = np.asarray(xs, np.int64), np.asarray(diff, np.uint8)
    P = w * h
    m = seams.changed_mask(w, h, xs, diff)

    def shifted(k):                                          # bit p of the result is bit p + k of the bitmap
        out = np.zeros(P, bool)
        if k >= 0:
            out[:P - k] = m[k:]
        else:
            out[-k:] = m[:P + k]
        return out

    c = np.zeros(P, np.int64)
    for k, mask in ((-w - 1, first), (-w, None), (-w + 1, last), (-1, first), (1, last), (w - 1, first), (w, None), (w + 1, last)):
        if abs(k) < P:
            c += shifted(k) & ~mask if mask is not None else shifted(k)
    return (diff != 0) & (c[xs // 3] >= need)


def first_in_word_only(flags):
    """Of the set flags of every 32-pixel word, the first alone."""
    out = np.zeros_like(flags)
    for p in np.flatnonzero(flags):
        if not flags[p // 32 * 32:p].any():
            out[p] = True
    return out


@pytest.mark.parametrize("shape", [s for s in ds.NARROW if s[0] < 32], ids=lambda s: "%dx%d" % s)
def test_column_masks_of_the_first_row_in_a_word_only_are_another_result(shape):
    """Over the needs and densities that test_narrow_and_word_aligned_widths runs (at W = 31 one pixel alone, pixel 31, shares
    its word with an earlier row start, so a single need may not show it)."""
    w, h = shape
    col = np.arange(w * h) % w
    first, last = col == 0, col == w - 1
    wrong_first, wrong_last = first_in_word_only(first), first_in_word_only(last)
    assert (wrong_first != first).any() or (wrong_last != last).any()
    differs = 0
    for density in (0.3, 0.7):
        tick = seams.narrow_case(shape, density)
        for xs, df in seams.streams_of(tick, 2):
            for need in range(1, 9):
                right = ds.keep_entries(w, h, xs, df, need)
                assert np.array_equal(linear_keep(w, h, xs, df, need, first, last), right), "the model without a mutation is despeckle_spec"
                differs += int((linear_keep(w, h, xs, df, need, wrong_first, wrong_last) != right).sum())
    assert differs > 0, shape

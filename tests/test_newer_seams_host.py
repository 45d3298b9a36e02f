"""CPU: the inputs of test_newer_seams_gpu.py.  Every builder of that file asserts, from the numpy reference alone, that its
input reaches the seam it is named for; this file calls each of them, so those assertions run where there is no GPU.  For the
record check it also compares mi355_cwire_check_host with the numpy reference on the 257-chunk and the 513-chunk batch."""
import numpy as np
import pytest

import test_newer_seams_gpu as seams
from cudavideostream_amd import cwire_check_host
from test_cwire_check_host import batch_of


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("h", sorted(seams.TOUCHED))
def test_touched_inputs_reach_their_waves(h, T):
    n, recs, counts, escapes, want, start = seams.touched_case(h, T)
    assert n == 3 * 256 * h and counts.size == 3 * T and want.shape[0] == 3 and start.shape[0] == 4


@pytest.mark.parametrize("which", sorted(seams.SELECTIONS))
@pytest.mark.parametrize("h", [342, 513])
def test_masked_compose_inputs_select_high_tiles(h, which):
    sel, rows, src = seams.masked_case(h, which)
    assert sel[64:].any() and rows.dtype == np.uint32 and not (src == seams.GUARD).any()


def test_chain_input_changes_tiles_63_and_64_only():
    recs, counts, escapes, old, new = seams.chain_case()[:5]
    changed = np.flatnonzero((old != new).any(axis=0))
    assert changed.size and set(changed // seams.K) == {63, 64}


@pytest.mark.parametrize("nc", sorted(seams.CHECK_SHAPES))
def test_check_host_past_the_chunk_rounds(nc):
    N, names, records, want = seams.check_case(nc)
    assert max(-(-n // seams.K) for _, n, _ in records) == nc
    buf, counts, escapes = batch_of([(None,) + tuple(r) for r in records])
    got = cwire_check_host(buf, counts, escapes, N)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert np.array_equal(got, want), [(names[i], list(got[i]), list(want[i])) for i in bad]


def test_activity_inputs_reach_their_rounds():
    segments = seams.big_activity()
    assert len(segments) == 4 and len(segments[0]) > 4 * seams.ENTRY_ROUND
    for S, T in seams.MANY:
        assert len(seams.many_segments(S, T)) == S * T

"""CPU: the inputs of test_crop_seams_gpu.py.  Every builder of that file asserts, from the numpy reference alone, that its input
reaches the seam it is named for; this file calls each of them, so those assertions run where there is no GPU."""
import numpy as np
import pytest

import test_crop_seams_gpu as seams


@pytest.mark.parametrize("S,T", seams.LAUNCH_COUNTS)
@pytest.mark.parametrize("w,h", seams.LAUNCH_FRAMES)
def test_launch_inputs_tell_the_launches_apart(w, h, S, T):
    recs, counts, escapes, rects = seams.launch_case(w, h, S, T)
    assert counts.size == S * T and rects.shape == (S, 4) and -(-S // seams.LAUNCH) == {127: 1, 128: 1, 129: 2, 257: 3}[S]


@pytest.mark.parametrize("S", seams.PLACE_COUNTS)
def test_place_inputs_reach_their_rounds(S):
    recs, counts, escapes, rects, want = seams.place_case(S)
    assert counts.size == S and counts.max() <= 19 and -(-S // seams.PLACE) == {1024: 1, 1025: 2, 2049: 3}[S]
    assert int(want[0][S]) > 0


@pytest.mark.parametrize("nt", sorted(seams.SCAN_SHAPES))
def test_scan_inputs_cross_the_round_seams(nt):
    S, T, recs, counts, escapes, rects, names = seams.scan_case(nt)
    assert S == len(names) == (8 if nt == 257 else 11) and T == 2
    assert sum(name.startswith("a mapped gap") for name in names) == 3 * (nt // 256)


@pytest.mark.parametrize("w,h", sorted(seams.ROW_SHAPES))
def test_row_inputs_put_rows_in_a_lane_and_tiles_in_a_row(w, h):
    recs, counts, escapes, sets = seams.row_case(w, h)
    assert counts.size == 6 and len(sets) >= 10
    if w <= 10:
        assert sum(what.startswith("columns") for what, _ in sets) == -(-(w * (w + 1) // 2) // 3)


def test_chain_pairs_are_all_there():
    assert len(seams.PAIRS) == 64 and len(set(seams.PAIRS)) == 64
    assert {a for a, _ in seams.PAIRS} == {b for _, b in seams.PAIRS} == set(seams.FAMILIES) and len(seams.FAMILIES) == 8
    c = seams.chain_inputs()
    assert int(c.budget[0][0]) > seams.THR5 and c.verdicts.shape == (6, 4) and np.array_equal(c.refresh[0], seams.rs.mask_of(c.sel))

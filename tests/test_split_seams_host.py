"""CPU: the inputs of test_split_seams_gpu.py.  Every builder of that file asserts, from the host form alone, that its input reaches
the seam it is named for; this file calls each of them, so those assertions run where there is no GPU, and holds the host form to
the numpy statement of the piece rule (split_spec.reference) on every well-formed case, so that the reference of the GPU
comparisons is itself pinned at these shapes."""
import numpy as np
import pytest

import split_spec
import test_split_seams_gpu as seams


def host_form_is_the_model(c):
    wf, wp, wo = split_spec.reference(c.buf, c.counts.size, c.M)
    gf, gp, go = c.want
    total = int(wf[-1])
    assert np.array_equal(gf, wf)
    assert np.array_equal(gp[:total + 1], wp)
    assert np.array_equal(go[:int(wp[-1])], wo)
    assert not go[int(wp[-1]):].any()
    assert all(int(wp[p + 1] - wp[p]) <= c.M for p in range(total))


@pytest.mark.parametrize("start", [0, 300])
def test_list_full_fills_the_list(start):
    c = seams.list_full(start)
    assert c.M == 64 and seams.LIST_ROUND + 4 == 516
    host_form_is_the_model(c)


@pytest.mark.parametrize("M", seams.LONG_M)
def test_long_pieces_cross_the_rounds(M):
    c = seams.long_piece(M)
    assert c.M == M and -(-int(c.counts[0]) // seams.BLOCK) == 3
    host_form_is_the_model(c)


@pytest.mark.parametrize("M", [64, 1400])
def test_late_escapes_sit_on_the_seams(M):
    c = seams.escapes_late(M)
    assert c.M == M and seams.blocks_of(c.counts) == [2]
    host_form_is_the_model(c)


def test_many_records_have_blocks_behind_records():
    c = seams.many_records(1)
    host_form_is_the_model(c)
    # the 145 records are these five, rotated and repeated: each one's pieces are the same bytes, where the sizes before put them
    big = seams.many_records(29)
    wf, wp, wo = c.want
    gf, gp, go = big.want
    order = [2, 3, 4, 0, 1]
    assert np.array_equal(big.counts, np.tile(c.counts[order], 29)) and np.array_equal(big.escapes, np.tile(c.escapes[order], 29))
    per = [(int(wf[r + 1]) - int(wf[r]), wo[int(wp[int(wf[r])]):int(wp[int(wf[r + 1])])]) for r in order] * 29
    assert np.array_equal(gf, np.cumsum([0] + [p for p, _ in per]))
    total = int(gf[-1])
    assert np.array_equal(go[:int(gp[total])], np.concatenate([b for _, b in per])) and not go[int(gp[total]):].any()
    sizes = np.concatenate([np.diff(wp[int(wf[r]):int(wf[r + 1]) + 1].astype(np.int64)) for r in order] * 29)
    assert np.array_equal(gp[:total + 1], np.concatenate([[0], np.cumsum(sizes)]))


def test_blocks_65_has_more_blocks_than_the_table_kernel_has_threads():
    c = seams.blocks_65()
    assert seams.blocks_of(c.counts) == [65]
    host_form_is_the_model(c)


@pytest.mark.parametrize("name", seams.SEAM_CAPACITY_CASES)
def test_capacities_end_at_the_block_seam(name):
    c, caps = seams.seam_capacities(name)
    total = int(c.want[0][-1])
    assert len(caps) == 5 and [p for p, _ in caps][:3] == [caps[1][0] - 1, caps[1][0], caps[1][0] + 1] and caps[3][0] == caps[4][0] == total
    assert caps[4][1] - caps[3][1] == 4 and caps[4][1] == int(c.want[1][caps[1][0]])


@pytest.mark.parametrize("M", seams.MALFORMED_M)
def test_malformed_record_exceeds_the_helpers(M):
    c, ample, helper, want_helper = seams.malformed(M)
    assert c.counts.size == 3 and ample[0] >= int(c.want[0][-1]) and np.array_equal(want_helper[0], c.want[0])
    reach = min(int(c.want[0][-1]), helper[0])
    assert np.array_equal(want_helper[1][:reach + 1], c.want[1][:reach + 1]), "the host form's tables do not depend on the capacities"


def test_chains_rewrite_the_scratch():
    chains = seams.chains()
    assert set(chains) == {seams.WIDE, seams.LIST} and all(len(cs) == 3 for cs in chains.values())

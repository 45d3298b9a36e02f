"""CPU: the inputs of test_fec_seams_gpu.py.  Every builder of that file asserts, from the tables and the numpy statement alone, that
its input reaches the seam it is named for; this file calls each of them, so those assertions run where there is no GPU (the grid
cases with the 8192 waves of a 256-CU device), and holds the host forms mi355_cwire_fec_host and mi355_cwire_fec_repair_host to
the numpy statement (fec_spec.reference, fec_spec.repair) on every builder's input, so that the reference of the GPU comparisons is
itself pinned at these shapes."""
import numpy as np
import pytest

import fec_spec
import test_fec_seams_gpu as seams
from gpu_util import GUARD

WAVES = 8192


def host_form_is_the_model(c):
    wf, wl, wo = fec_spec.reference(c.pieces, c.pbytes, c.first, c.pos, c.pcap, c.G, c.K, c.pitch, c.gcap, c.cap, GUARD)
    gf, gl, go = c.want
    assert np.array_equal(gf, wf) and np.array_equal(gl, wl)
    assert np.array_equal(go, wo), "a parity byte differs, or one outside the blocks that fit was written"
    L = seams.group_lens(c.first, c.pos, c.pcap, c.pbytes, c.pitch, c.G)
    reach = min(L.size, c.gcap)
    assert np.array_equal(gl[:reach], L[:reach]), "the builders' own reading of the tables"


def repair_is_the_model(c):
    for args, (blocks, verdicts) in zip(c.args, c.want):
        want_blocks, want_verdicts = fec_spec.repair(*args)
        assert len(blocks) == len(want_blocks) == sum(s is None for s in args[0]) and list(verdicts) == want_verdicts
        for got, want in zip(blocks, want_blocks):
            assert got.size == args[3] and np.array_equal(got, want)


@pytest.mark.parametrize("which,K,cut", seams.GRID_POINTS)
def test_grid_cases_take_every_wave_past_its_first_item(which, K, cut):
    c = seams.grid_case(which, WAVES, K, cut)
    assert c.waves == WAVES and c.items >= 2 * WAVES + (cut != "groups")
    per_wave = np.bincount(np.arange(c.items) % WAVES, minlength=WAVES)
    assert per_wave.min() >= 2 and (cut == "groups" or per_wave.max() >= 3)
    host_form_is_the_model(c)


def test_member_counts_reach_every_remainder():
    """Full groups of G and the short last one: the 4-member batches end on 0, 1, 2 and 3 members."""
    last = {G: seams.MEMBER_PIECES % G or G for G in seams.MEMBER_G}
    assert {G % 4 for G in seams.MEMBER_G} | {m % 4 for m in last.values()} == {0, 1, 2, 3}


@pytest.mark.parametrize("K", (1, 2))
@pytest.mark.parametrize("G", seams.MEMBER_G)
def test_member_cases(G, K):
    host_form_is_the_model(seams.member_case(G, K))


@pytest.mark.parametrize("slot", seams.SLOTS)
@pytest.mark.parametrize("kind", seams.KINDS)
def test_malformed_cases_have_their_void_group(kind, slot):
    c, g, bad, void = seams.malformed_case(kind, slot)
    host_form_is_the_model(c)
    well = seams.member_case(255, 2).want
    rest = [i for i in range(int(c.want[0][-1])) if i not in void]
    blocks = lambda out: out.reshape(-1, 2 * seams.MEMBER_BYTES)
    assert np.array_equal(blocks(c.want[2])[rest], blocks(well[2])[rest]) and (blocks(c.want[2])[void] == GUARD).all()
    assert len(void) == 1 or (kind, slot) == ("past", 254)


def test_two_lost_cases():
    repair_is_the_model(seams.two_lost())


def test_verdict_pair_cases():
    c, expect = seams.verdict_pairs()
    repair_is_the_model(c)
    assert [tuple(int(v) for v in w[1]) for w in c.want] == expect


def test_four_byte_cases():
    repair_is_the_model(seams.four_bytes())


@pytest.mark.parametrize("name", sorted(seams.PACKINGS))
def test_packing_cases(name):
    c = seams.packing(name)
    repair_is_the_model(c)
    assert [len(a[0]) for a in c.args] == list(seams.PACKINGS[name])


def test_far_piece_case():
    first, pos, pbytes, rows, c = seams.far_pieces()
    host_form_is_the_model(c)
    assert pbytes > seams.T32 and rows.shape == (2, seams.FAR_N) and int(c.want[0][-1]) == 8


def test_far_parity_case():
    five, pos, flen = seams.far_parity()
    host_form_is_the_model(five)
    lens = [fec_spec.member_len(pos, seams.FAR_OUT_PIECES, five.pieces.size, seams.FAR_OUT_PITCH, p) for p in range(seams.FAR_OUT_PIECES)]
    assert np.array_equal(flen, lens) and int(np.count_nonzero(flen)) == 5


def test_far_repair_cases():
    rows, rx_bytes, c = seams.far_repair()
    repair_is_the_model(c)
    assert rx_bytes > seams.T32 and int(c.slot_off[c.slot_off != seams.A].max()) > seams.T32 and int(c.parity_off.min()) > seams.T32
    c, rebuilt, vd = seams.far_jobs()
    blocks, verdicts = fec_spec.repair(*c.args)
    assert np.array_equal(blocks[0], rebuilt) and verdicts == [vd]

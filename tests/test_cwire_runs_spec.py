"""The run form of compact records (include/mi355diff.h, "Run-coded records") as tests/runs_spec.py states it: the header's worked
example byte for byte, the size formula, the packing rule at its boundary, canonical uniqueness and the cut at every 256 entries.
No library, no GPU."""
import numpy as np
import pytest

import cwire_spec as spec
import runs_spec as rs


def rec_of(xs, diff=None):
    xs = np.asarray(xs, np.int64)
    diff = np.arange(1, xs.size + 1, dtype=np.uint8) if diff is None else diff
    return np.frombuffer(spec.encode_frame(xs, diff), np.uint8)


def test_worked_example_as_literal_bytes():
    rec = rec_of([3, 4, 5, 300, 301, 1000], np.array([10, 20, 30, 40, 50, 60], np.uint8))
    assert rec.tobytes() == bytes([6, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 255, 0, 255, 0, 0, 38, 1, 0, 0, 186, 2, 0, 0,
                                   10, 20, 30, 40, 50, 60, 0, 0])
    run, r = rs.to_runs(rec)
    assert r == 3
    assert run == bytes([6, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0,      # n, e, r
                         3, 255, 255, 0,                          # gap, pad
                         2, 1, 0, 0,                              # len, pad
                         38, 1, 0, 0, 186, 2, 0, 0,               # esc 294, 698
                         10, 20, 30, 40, 50, 60, 0, 0])           # diff, pad
    assert len(run) == 36 and rec.size == 32 and not rs.smaller(6, 3)
    forms, pos, link = rs.encode(rec, 1, rs.WHERE_SMALLER)
    assert forms.tolist() == [[rs.FORM_COMPACT, 6, 2, 3]] and pos.tolist() == [0, 32] and link.tobytes() == rec.tobytes()
    forms, pos, link = rs.encode(rec, 1, rs.ALWAYS)
    assert forms.tolist() == [[rs.FORM_RUNS, 6, 2, 3]] and pos.tolist() == [0, 36] and link.tobytes() == run
    assert rs.from_runs(run) == rec.tobytes()


@pytest.mark.parametrize("n,e,r", [(0, 0, 0), (1, 0, 1), (1, 1, 1), (6, 2, 3), (256, 0, 1), (257, 0, 2), (4097, 3, 17), (691168, 0, 2700)])
def test_size_formula(n, e, r):
    assert rs.runs_frame_bytes(n, e, r) == 12 + 2 * ((r + 3) // 4 * 4) + 4 * e + (n + 3) // 4 * 4
    assert (rs.runs_frame_bytes(n, e, r) < spec.frame_bytes(n, e)) == rs.smaller(n, r)


def test_size_formula_on_real_records():
    for name, xs in rs.patterns(9216).items():
        rec = rs.record(xs)
        run, r = rs.to_runs(rec)
        n, e = (int(v) for v in rec[:8].view("<u4"))
        assert len(run) == rs.runs_frame_bytes(n, e, r), name
        assert (len(run) < rec.size) == rs.smaller(n, r), name


def test_packing_rule_at_its_boundary():
    # one run of n entries from index 1: r = ceil(n / 256); 4 + 2*pad4(1) = 12 < pad4(n) first holds at n = 13
    for n, packed in ((12, False), (13, True), (16, True)):
        forms, pos, link = rs.encode(rec_of(np.arange(1, 1 + n)), 1, rs.WHERE_SMALLER)
        assert forms.tolist() == [[int(packed), n, 0, 1]], n
        assert int(pos[1]) == (rs.runs_frame_bytes(n, 0, 1) if packed else spec.frame_bytes(n, 0))
    # five runs of four entries: n = 20, r = 5: 4 + 16 = 20 < 20 is false (equal sizes stay compact); n = 21 tips it
    xs = np.concatenate([np.arange(10 * i, 10 * i + 4) for i in range(5)])
    forms, pos, _ = rs.encode(rec_of(xs), 1, rs.WHERE_SMALLER)
    assert forms.tolist() == [[rs.FORM_COMPACT, 20, 0, 5]] and rs.runs_frame_bytes(20, 0, 5) == spec.frame_bytes(20, 0) == 48
    forms, pos, _ = rs.encode(rec_of(np.append(xs, 44)), 1, rs.WHERE_SMALLER)
    assert forms.tolist() == [[rs.FORM_RUNS, 21, 0, 5]] and int(pos[1]) == 52 < spec.frame_bytes(21, 0) == 56


@pytest.mark.parametrize("policy", [rs.WHERE_SMALLER, rs.ALWAYS])
def test_canonical_by_re_encoding_a_decode(policy):
    pats = rs.patterns(9216)
    buf = np.concatenate([rs.record(xs, i) for i, xs in enumerate(pats.values())])
    forms, pos, link = rs.encode(buf, len(pats), policy)
    frame_pos, back = rs.decode(link, forms)
    assert back.tobytes() == buf.tobytes()
    assert frame_pos.tolist() == np.cumsum([0] + [rs.record(xs, i).size for i, xs in enumerate(pats.values())]).tolist()
    forms2, pos2, link2 = rs.encode(back, len(pats), policy)
    assert np.array_equal(forms, forms2) and np.array_equal(pos, pos2) and link.tobytes() == link2.tobytes()
    if policy == rs.WHERE_SMALLER:
        assert link.size <= buf.size and 0 < int(forms[:, 0].sum()) < len(pats)   # some packed, some not, never larger


def test_the_cut_rule():
    gap, ln = rs.runs_of(rec_of(np.arange(600))[8:608])
    assert (ln.astype(int) + 1).tolist() == [256, 256, 88] and gap.tolist() == [0, 0, 0]
    xs = np.concatenate([np.arange(0, 256, 2), np.arange(300, 900)])   # 128 isolated entries, then 600 consecutive
    gap, ln = rs.runs_of(rec_of(xs)[8:8 + xs.size])
    assert (ln.astype(int) + 1).tolist() == [1] * 128 + [128, 256, 216]
    assert gap.tolist() == [0] + [1] * 127 + [45, 0, 0]


def test_empty_record():
    rec = rec_of([])
    run, r = rs.to_runs(rec)
    assert r == 0 and run == bytes(12) and rs.from_runs(run) == bytes(8)
    assert rs.encode(rec, 1, rs.WHERE_SMALLER)[0].tolist() == [[rs.FORM_COMPACT, 0, 0, 0]]

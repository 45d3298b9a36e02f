"""The planner of the record-call chain (tests/record_chain.py) alone, on a CPU: the sweep leaves no ordered pair out, the table
names every entry point that takes record headers from the host, and the inputs of the sweep and of the random chains reach what
they are there for.  These are conditions on the inputs, asserted from the reference alone; no GPU is touched."""
import os
import re

import numpy as np
import pytest

import crop_spec
import record_chain as rc
import split_spec
import wall_spec as ws
import test_record_chain_gpu as gpu

NAMES = list(rc.FAMILIES)


def test_the_sweep_is_complete():
    """14 x 14 ordered pairs, (A, A) included, in both orientations; and every entry point of include/mi355diff.h that takes
    h_counts and h_escapes is queued by a family of the table or left out for a reason of its own."""
    assert len(NAMES) == 14
    for orientation in (0, 1):
        pairs = {(seq[0], seq[1]) for A in NAMES for seq in rc.sweep_sequences(A, orientation)}
        ka, kb = rc.KINDS[orientation], rc.KINDS[1 - orientation]
        assert pairs == {((A, ka), (B, kb)) for A in NAMES for B in NAMES}
        assert all(len(seq) == 2 for A in NAMES for seq in rc.sweep_sequences(A, orientation))
    assert gpu.SWEEP_CASES == NAMES, "one case of the GPU sweep per family"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "mi355diff.h")).read(), flags=re.S)
    takers = {m.group(1) for m in re.finditer(r"\b(mi355_\w+)\s*\(([^;{}]*?)\)\s*;", text)
              if re.search(r"\bh_counts\b", m.group(2)) and re.search(r"\bh_escapes\b", m.group(2))}
    declared = set(re.findall(r"\b(mi355_\w+)\s*\(", text))
    queued = {name for f in rc.FAMILIES.values() for name in f.calls}
    assert len(takers) >= 21 and queued <= declared, sorted(queued - declared)
    assert not (queued & set(rc.LEFT_OUT)) and all(len(why) > 20 for why in rc.LEFT_OUT.values())
    assert takers <= queued | set(rc.LEFT_OUT), sorted(takers - queued - set(rc.LEFT_OUT))
    assert set(rc.LEFT_OUT) <= takers, "an exclusion the header no longer needs"
    for letter in rc.FAMILIES:
        assert callable(getattr(rc.Planner, "plan_" + letter))


def chains():
    """name -> [(planner, the rounds it plans)] of every chain the GPU module runs, with the seeds and draws it uses."""
    out = {"sweep": lambda: [(rc.Planner(draws=ord(A), **gpu.SWEEP), [seq for o in (0, 1) for seq in rc.sweep_sequences(A, o)]) for A in NAMES],
           "small sweep": lambda: [(rc.Planner(**gpu.SMALL), [seq for A in NAMES for seq in rc.sweep_sequences(A, 0)])]}
    for mode in rc.MODES:
        def random(mode=mode):
            p = rc.Planner(mode=mode, **gpu.RANDOM[mode])
            return [(p, [p.random_sequence() for _ in range(gpu.ROUNDS)])]
        out[f"random {mode}"] = random
    return out


def merged(stats):
    """The planners' statistics of one chain together: counts added, sets united."""
    out = {}
    for st in stats:
        for k, v in st.items():
            if isinstance(v, dict):
                out[k] = {f: out.get(k, {}).get(f, 0) + c for f, c in v.items()}
            elif isinstance(v, set):
                out[k] = out.get(k, set()) | v
            else:
                out[k] = out.get(k, 0) + v
    return out


@pytest.mark.parametrize("name", list(chains()))
def test_the_chains_are_not_trivial(name):
    """The conditions on the inputs that the chains are there for, over the sweep's inputs (its 14 cases together) and the seeds
    of the random chains."""
    runs = chains()[name]()
    for p, seqs in runs:
        for seq in seqs:
            p.plan_round(seq)
    st, p = merged([p.stats for p, _ in runs]), runs[0][0]
    inp, S, K, n = p.inp, p.S, p.K, p.n
    assert all(st["ops"][f] > 0 for f in rc.FAMILIES), (name, st["ops"])
    loud, quiet = inp.kind["loud"], inp.kind["quiet"]
    for which_ in ("burst", "tick"):
        assert (loud[which_]["counts"] >= 0.9 * n).all(), (name, "loud records have n >= 0.9 N")
        q = quiet[which_]
        assert q["escapes"].max() > 0 and (q["counts"] == 0).any() and (q["counts"] > 0).any(), (name, "an escape and an empty record")
        o = q["off"].astype(np.int64)
        k_ = q["B"] // S
        touched = np.stack([ws.touched(n, [q["xs"][o[s * k_]:o[(s + 1) * k_]]]) for s in range(S)])
        assert not touched.all(), (name, "a tile no record lands in")
        if n >= 12 * 4096:
            assert (touched.sum(axis=1) <= 3).all() and touched.any(axis=0).sum() < ws.tiles(n)
    assert st["over_budget"] > 0, (name, "the budget call goes over its limit")
    for kind in rc.KINDS:
        assert st["kept"][kind] > 0 and st["dropped"][kind] > 0, (name, kind, "despeckle keeps and drops")
        acc = crop_spec.sums(inp.kind[kind]["burst"]["recs"], S, K, n)
        for s in range(S):
            total = int((acc[s] != 0).sum())
            if total:                                                 # (the quiet stream that never changes has no entry to contain)
                inside = len(crop_spec.segment(acc[s], p.w, p.h, inp.rects[s])[0])
                assert 0 < inside < total, (name, kind, s, "the rectangle contains an entry and excludes one")
    assert ws.tiles(p.nc) > ws.tiles(n) and p.B >= 4, (name, "the canvas has more tiles than a frame")
    pieces = dict(st["split"])
    assert pieces["quiet"] > 1, (name, "a quiet record makes more than one piece")
    if n > split_spec.BLOCK:
        t = loud["tick"]
        assert (t["counts"] > split_spec.BLOCK).all()
        cuts = split_spec.cuts(t["xs"][:int(t["off"][1])], rc.SPLIT_M["loud"])
        assert any(a == split_spec.BLOCK for a, _ in cuts), (name, "a loud record is cut at its 65536-entry block")
    assert st["rebuilt"] > 0, (name, "a parity group loses a piece and is rebuilt")
    assert st["forms"] == {0, 1}, (name, "the run coder picks both forms")
    assert "some" in st["refresh"], (name, "the refresh selects some tiles and not all")
    assert st["thumb_entries"] > 0 and st["cancelled"] > 0, name

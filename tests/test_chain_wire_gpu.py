"""-m gpu: the chain soak of the compact-wire and many-streams family (tests/soak_chain.py, run_wire) in short form.

Random part: a dozen rounds of 3 to 8 operations per mode on a sender core and a relay/client core, and on ONE core in every
role, at 160x140 (66 tiles: every pipelined pack is split over two streams) and a few rounds at 37x11 with stride = N = 1221
(the byte paths, the unaligned state rule).  Nothing synchronises inside a round; every output, every set of states and the
cores' own states are compared np.array_equal with a reference computed on the CPU before the round's first call, in guarded
buffers (gpu_util).

Deterministic part: every ordered pair (A, B) of the operation families a..j -- what A and B need is made first (a tick, a
burst and/or a one-stream batch), then A and B run with nothing between them, then one synchronisation and the comparison.  This
pins the sentences of include/mi355diff.h that speak of EVERY later entry point ("every later entry point of this core that
reads the states finds them complete", "the two may alternate without a synchronisation", "behind the last expansion of this
core as every consumer of a packed stream is").

test_the_chains_are_not_trivial checks on the host, from the planner alone, that the seeds below reach what they are there for."""
import numpy as np
import pytest

import soak_chain
from cudavideostream_amd import lib

pytestmark = pytest.mark.gpu

ROUNDS, SMALL_ROUNDS = 12, 6
SEEDS = {"own": 2, "sequential": 5, "callers": 10}          # two cores
ONE_CORE_SEEDS = {"own": 8, "callers": 12}
SMALL = dict(w=37, h=11)                                     # N = 1221: no multiple of 4, stride = N
SWEEP_K = 3


@pytest.mark.parametrize("mode", soak_chain.MODES)
def test_chain_wire_short(mode):
    assert soak_chain.run_wire(ROUNDS, SEEDS[mode], mode=mode, verbose=False)
    assert soak_chain.run_wire(SMALL_ROUNDS, SEEDS[mode] + 60, mode=mode, verbose=False, **SMALL)
    if mode == "own":                                        # the core's streams in their own priority class
        assert soak_chain.run_wire(4, SEEDS[mode] + 70, flags=lib.FLAG_OWN_QUEUES, verbose=False)


def test_chain_wire_one_core():
    """Sender, relay and client are the same core: every consumer reads what the call before it wrote."""
    for mode, seed in ONE_CORE_SEEDS.items():
        assert soak_chain.run_wire(ROUNDS, seed, mode=mode, one_core=True, verbose=False)
    assert soak_chain.run_wire(SMALL_ROUNDS, 77, one_core=True, verbose=False, **SMALL)


# ---- every ordered pair of families ---------------------------------------------------------------------------------------
def needs(fam):
    """What a family consumes: a tick ('a'), a burst ('b'), either ('t'), a one-stream batch ('f'), or nothing."""
    return {"c": "t", "d": "b", "e": "a", "g": "f", "j": "f"}.get(fam)


def sequence_for(A, B):
    """-> [(family, hint)]: the priming calls, then A, then B; None if B's precondition cannot hold behind A.  Compact forms
    throughout (the consumers of the other forms are c's, and the random part draws them); f in the form that decodes."""
    hint = {"a": {"form": "cwire"}, "b": {"form": "cwire"}, "f": {"direct": False},
            "i": {"form": "cwire", "K": SWEEP_K if "d" in (A, B) else 1}}
    have = {"a": {"a", "t"}, "b": {"b", "t"}, "i": {"b", "t"} if "d" in (A, B) else {"a", "t"}, "e": {"t"}, "f": {"f"}}
    for prime in (["a"], ["b"], ["f"], ["a", "f"], ["b", "f"]):
        seq, ok, got = prime + [A, B], True, set()
        for fam in seq:
            if needs(fam) and needs(fam) not in got:
                ok = False
            if fam in "abi":
                got -= {"a", "b", "t"}                       # a new tick replaces the one before
            if fam == "e":
                got -= {"a"}                                 # a thinned tick is not thinned again
            got |= have.get(fam, set())
        if ok:
            return [(fam, hint.get(fam, {})) for fam in seq]
    return None


IMPOSSIBLE = {("a", "d"), ("b", "e"), ("d", "e"), ("e", "d"), ("e", "e")}
# a / b in front of d / e: the new tick is not the kind the consumer takes; d and e take different kinds; e thins a tick once


def test_the_pair_sweep_leaves_out_only_what_cannot_be():
    missing = {(A, B) for A in soak_chain.FAMILIES for B in soak_chain.FAMILIES if sequence_for(A, B) is None}
    assert missing == IMPOSSIBLE


@pytest.mark.parametrize("A", list(soak_chain.FAMILIES))
def test_every_pair_of_families_without_synchronisation(A):
    """160x140, S = 2, K = 3, the core's own streams, one core in every role: (priming, A, B, one synchronisation, comparison)
    for every family B."""
    p = soak_chain.WirePlanner(900 + ord(A), 160, 140, 2, SWEEP_K, "own", one_core=True)
    E = soak_chain.WireEnv(p)
    try:
        for B in soak_chain.FAMILIES:
            seq = sequence_for(A, B)
            if seq is None:
                assert (A, B) in IMPOSSIBLE
                continue
            R = p.plan_round(forced=seq)
            assert R is not None, (A, B, "a precondition the sequence was to meet is not met")
            assert [op[0] for op in R.ops][-2:] == [A, B]
            bad = E.run_round(R)
            assert not bad, (A, B, bad, R.ops)
    finally:
        E.close()


# ---- the chains are worth running -----------------------------------------------------------------------------------------
def test_the_chains_are_not_trivial():
    """Host only.  Each short random run above reaches every operation a..k, puts a budget over its limit, cancels a coalesced
    index, has a record with an escape, and at least half of its records are non-empty; the two-core runs on the cores' own
    streams read staged references across the cores, the others what the GPU wrote."""
    runs = [(dict(mode=m), SEEDS[m]) for m in soak_chain.MODES] + [(dict(mode=m, one_core=True), s) for m, s in ONE_CORE_SEEDS.items()]
    for kw, seed in runs:
        st = soak_chain.wire_stats(ROUNDS, seed, **kw)
        assert all(st["ops"][c] > 0 for c in soak_chain.FAMILIES + "k"), (kw, st["ops"])
        assert st["over_budget"] > 0 and st["cancelled"] > 0 and st["escaped_records"] > 0, (kw, st)
        assert 2 * st["nonempty"] >= st["records"] > 0, (kw, st)
        assert (st["staged"] == 0) == bool(kw.get("one_core")), (kw, st)
    every = {c: 0 for c in soak_chain.FAMILIES}
    for mode in soak_chain.MODES:                            # the unaligned shape: all three modes together reach every family
        st = soak_chain.wire_stats(SMALL_ROUNDS, SEEDS[mode] + 60, mode=mode, **SMALL)
        assert 2 * st["nonempty"] >= st["records"] > 0
        for c in every:
            every[c] += st["ops"][c]
    assert all(every.values()), every

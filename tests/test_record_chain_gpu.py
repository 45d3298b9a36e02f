"""-m gpu: the record-call chain (tests/record_chain.py) -- the calls that read compact records, queued behind each other on one
long-lived core without host synchronisation, so that each runs on the scratch (record table, chunk facts, tile directory,
per-stream rows, split and run-coder tables, the despeckle bitmap) that a call of another family, on another kind of input, has
just used, and behind whatever that call left queued.

Deterministic part: every ordered pair (A, B) of the 14 families, (A, A) included, in both orientations -- the producers P, then A
on the loud records and B on the quiet ones, and in the next round A on the quiet and B on the loud; one synchronisation per
round, then every output, every set of states and every guard byte is compared np.array_equal with what the planner computed on
the CPU before the round's first call.  One core per case, made without PREPARE_DESPECKLE: its first despeckle call allocates in
the middle of queued work.  The same sweep in one orientation at 37x11 (N = 1221 = stride: the byte paths).

Random part: a dozen rounds of 4 to 8 families per mode on one core; a second core, prepared with everything, serves the last.

tests/test_record_chain_host.py checks on the host, from the planner alone, that no pair is left out and that the inputs reach
what they are there for."""
import pytest

import record_chain as rc
from cudavideostream_amd import lib

pytestmark = pytest.mark.gpu

SWEEP = dict(seed=11, w=160, h=140, S=3, K=4)                # 17 tiles a stream: every pipelined pack is split over two streams
SMALL = dict(seed=12, w=37, h=11, S=3, K=4)                  # N = 1221: no multiple of 4, stride = N
RANDOM = {"own": dict(seed=11, draws=1), "sequential": dict(seed=11, draws=2), "callers": dict(seed=13, draws=3)}
ROUNDS, PREPARED_ROUNDS = 12, 4
SWEEP_CASES = list(rc.FAMILIES)


@pytest.mark.parametrize("A", SWEEP_CASES)
def test_every_pair_without_synchronisation(A):
    """160x140, S = 3, K = 4, the core's own streams, pipelined: for every family B the rounds (P, A on loud, B on quiet) and
    (P, A on quiet, B on loud)."""
    p = rc.Planner(draws=ord(A), **SWEEP)
    E = rc.Env(p)
    try:
        for orientation in (0, 1):
            bad = rc.run_sequences(p, E, rc.sweep_sequences(A, orientation), f"A = {A}, A on {rc.KINDS[orientation]}")
            assert not bad, bad
    finally:
        E.close()


def test_every_pair_small_unaligned():
    p = rc.Planner(**SMALL)
    E = rc.Env(p)
    try:
        for A in SWEEP_CASES:
            bad = rc.run_sequences(p, E, rc.sweep_sequences(A, 0), f"A = {A}")
            assert not bad, bad
    finally:
        E.close()


@pytest.mark.parametrize("mode", rc.MODES)
def test_random_chains(mode):
    p = rc.Planner(mode=mode, **RANDOM[mode])
    seqs = [p.random_sequence() for _ in range(ROUNDS)]
    E = rc.Env(p)
    try:
        bad = rc.run_sequences(p, E, seqs[:ROUNDS - PREPARED_ROUNDS], f"random, {mode}")
        assert not bad, bad
        F = rc.Env(p, prepare=lib.PREPARE_ALL | lib.PREPARE_DESPECKLE)
        try:
            bad = rc.run_sequences(p, F, seqs[ROUNDS - PREPARED_ROUNDS:], f"random, {mode}, the prepared core")
            assert not bad, bad
        finally:
            F.close()
    finally:
        E.close()

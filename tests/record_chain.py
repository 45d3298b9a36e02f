"""The record-call chain: every call that reads compact records shares a few scratch buffers of its core ("The
record-call chain"), and this module queues those calls behind each other on ONE long-lived core WITHOUT host synchronisation,
in the manner of soak_chain.WirePlanner / WireEnv but table-driven: FAMILIES has one entry per family -- its entry points and
its plan, which simulates the family on the host, queues its GPU calls and lists its checks.  Not a test module:
tests/test_record_chain_gpu.py runs it on the GPU, tests/test_record_chain_host.py runs the planner alone.

A round: every set of states is uploaded as it was at the planner's start (the scratch under test lives in the core and is never
reset), the producers P make a burst (S x K records) and a tick (S records) of BOTH kinds of input on the sender states,
pipelined, then the round's families run, each on the records of one kind, with nothing in between; one synchronisation, and
every output of the round -- guard bytes included -- is compared np.array_equal with what the planner computed before the first
call.  Every consumer reads what the GPU producer wrote; the host passes only headers (counts, escapes, forms, tables) taken from
the reference.  Nothing expected comes from a GPU call.

The two kinds of input (Inputs):
  loud   nearly every byte of every frame changes (a few still pixels): records of n close to N, at 160x140 17 chunks and 2 split
         blocks per record, runs cut at 256 -- every row of the scratch is filled
  quiet  a 3x3 pixel cluster and a few isolated bytes, at most three tiles of a stream, gaps of 255 and more (escapes); stream 1
         does not change at all (its records are empty: one empty chunk), most tiles have no record landing in them

Data flow the planner follows, and nothing else: B and D revert the sender states of their kind at dropped entries (twice on one
tick: the rule applied twice, from the states as they then are); A moves the client states; Y's clear zeroes tiles of them; H moves
the held thumbnails.  T and H need the state they read to be unchanged outside their mask (the masked repaint and law 3 of the
thumbnail records are only then unique): their mask is the touched tiles of their own burst ORed, on the GPU, with the touched
tiles of every record set that moved the client states since the round began, and the planner asserts that this covers every
changed tile."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from cudavideostream_amd import (cwire_apply_host, cwire_bytes_max, cwire_check_host, cwire_fec_groups_max,  # noqa: E402
                                 cwire_runs_bytes_max, cwire_split_bytes_max, cwire_split_pieces_max, activity_cells, lib)
from oracle import pyoracle as po  # noqa: E402  (checker)

import crop_spec  # noqa: E402
import cwire_spec as spec  # noqa: E402
import despeckle_spec  # noqa: E402
import fec_spec  # noqa: E402
import mosaic_spec  # noqa: E402
import resync_spec  # noqa: E402
import runs_spec  # noqa: E402
import split_spec  # noqa: E402
import thumb_spec  # noqa: E402
import wall_spec as ws  # noqa: E402

GUARD = 0x5C                                  # gpu_util.GUARD (asserted in Env)
NOLIMIT = 0xFFFFFFFF
KINDS = ("loud", "quiet")
MODES = ("own", "sequential", "callers")      # the core's streams pipelined, OPT_PIPELINE 0, the caller's (torch's) stream
CELL = (16, 8, 2)                             # cell_w, cell_h, min_count of V
THUMB_K, THUMB_THR = 2, 3                     # H
WALL_KS = (2, 3, 4)                           # T: the scale of stream s is WALL_KS[s % 3]
FEC_G, FEC_K = 4, 2                           # S: pieces per group, parity blocks per group
SPLIT_M = {"loud": 8972, "quiet": 64}         # S: both documented; the loud records are cut at their 65536-entry block too
NEEDS = {"loud": (8, 0, 6), "quiet": (4, 0, 3)}   # D: need of stream s is NEEDS[kind][s % 3]
MAX_JOBS = 6
I32, I64, U8 = "i32", "i64", "u8"


def _refs():
    """The numpy statements that live in test modules (imported on first use)."""
    from test_activity_gpu import oracle as activity_oracle
    from test_cwire_budget_gpu import threshold_for
    from test_cwire_coalesce_gpu import reference as coalesce_reference
    from test_cwire_round_seams_gpu import numpy_tick
    return activity_oracle, threshold_for, coalesce_reference, numpy_tick


# ---- the inputs ------------------------------------------------------------------------------------------------------------
def quiet_positions(w, h, s):
    """The byte indices stream s changes in every quiet frame: a 3x3 pixel cluster, and isolated bytes in the middle and at the
    end of the frame, 290 and more apart."""
    n, row = 3 * w * h, 3 * w
    cx, cy = w // 3 + 7 * s, h // 7 + s
    assert cx + 3 <= w and cy + 3 <= h
    cluster = [(cy + dy) * row + 3 * (cx + dx) + c for dy in range(3) for dx in range(3) for c in range(3)]
    many = n >= 12 * 4096
    mid = n * 7 // 16 + 37 * s + 301 * np.arange(10 if many else 1)
    end = n - 7 - 3 * s - 290 * np.arange(5 if many else 2)
    return np.unique(np.concatenate([cluster, mid, end])).astype(np.int64)


def _records(off, xs, df, B):
    recs, pos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, B)
    assert np.array_equal(counts, np.diff(off.astype(np.int64)))
    out = dict(off=off, xs=xs, df=df, recs=recs, pos=pos, counts=counts, escapes=escapes, B=B)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def produce(burst_frames, tick_frames, states, S, K, thr):
    """What the producers write: the burst of K frames per stream (the oracle's diff_stream) and then the tick (numpy_tick) on
    the states -> (the burst's records, the tick's records, the states afterwards)."""
    numpy_tick = _refs()[3]
    offs, xs, df, mid = [0], [], [], []
    for s in range(S):
        o, x, v, st = po.diff_stream(burst_frames[s * K:(s + 1) * K], states[s], thr)
        offs += [offs[-1] + int(c) for c in o[1:]]; xs.append(x); df.append(v); mid.append(st)
    burst = _records(np.array(offs, np.uint32), np.concatenate(xs).astype(np.int32), np.concatenate(df).astype(np.uint8), S * K)
    tk = numpy_tick(np.stack(mid), tick_frames, thr)
    off, txs, tdf = spec.decode(tk[0], S)
    tick = _records(off, txs, tdf, S)
    assert np.array_equal(tick["recs"], tk[0]) and np.array_equal(tick["pos"], tk[1])
    return burst, tick, np.array(tk[4], np.uint8)


class Inputs:
    """The frames of both kinds and everything that depends on them alone: what P writes, and its decoded entries."""

    def __init__(self, seed, w, h, S, K, thr):
        rng = np.random.default_rng(seed)
        self.w, self.h, self.S, self.K, self.thr = w, h, S, K, thr
        self.n = n = 3 * w * h
        self.base = rng.integers(0, 256, (S, n), dtype=np.uint8)
        self.kind = {}
        for kind in KINDS:
            frames = np.empty((S, K + 1, n), np.uint8)                # K burst frames and the tick's frame, per stream
            for s in range(S):
                prev = self.base[s]
                q = quiet_positions(w, h, s)
                for k in range(K + 1):
                    delta = np.zeros(n, np.uint8)
                    if kind == "loud":
                        delta[:] = rng.integers(21, 236, n)
                        delta[np.repeat(rng.random(w * h) < 0.012, 3)] = 0          # still pixels
                        if k < K:                                                   # a few bytes come back: the coalescer cancels them
                            z = np.arange(5 + s, n, 97)
                            delta[z] = 60 if k % 2 == 0 else (196 if k else 0)
                            if k == K - 1 and K % 2:
                                delta[z] = 0
                    elif s != 1:
                        delta[q] = 30 + k + (np.arange(q.size) % 50 if k == K else 0)
                        if k < K:                                                   # one isolated byte goes and comes back
                            delta[q[-1]] = (50 if k % 2 == 0 else 206) if not (k == K - 1 and K % 2) else 0
                    prev = prev + delta
                    frames[s, k] = prev
            d = dict(kind=kind, burst_frames=np.ascontiguousarray(frames[:, :K].reshape(S * K, n)),
                     tick_frames=np.ascontiguousarray(frames[:, K]))
            d["burst"], d["tick"], d["snd"] = produce(d["burst_frames"], d["tick_frames"], self.base, S, K, thr)
            self.kind[kind] = d
        first = np.stack([ws.thumbnail(self.base[s], w, h, THUMB_K).reshape(-1) for s in range(S)])
        held = np.clip(first.astype(int) + rng.integers(-THUMB_THR, THUMB_THR + 1, first.shape), 0, 255).astype(np.uint8)
        tw = ws.thumb_size(w, h, THUMB_K)[0]
        for s in range(S):                                            # far off where every mask of H requires the pixel
            if s != 1:
                cx, cy = w // 3 + 7 * s + 1, h // 7 + s + 1
                j = 3 * ((cy // THUMB_K) * tw + cx // THUMB_K)
                held[s, j:j + 3] = first[s, j:j + 3] + 128
        self.held = held
        self.places, x = [], 0
        for s in range(S):
            k = WALL_KS[s % 3]
            self.places.append((x, s % 2, k))
            x += ws.thumb_size(w, h, k)[0] + 1
        self.wall_w, self.wall_h = x, max(ws.thumb_size(w, h, k)[1] for k in WALL_KS) + 1
        self.wall0 = ws.compose(np.full((self.wall_h, self.wall_w, 3), GUARD, np.uint8), self.base, w, h, self.places)
        self.cw_, self.ch_ = 2 * w + 1, 2 * h + 1                     # the mosaic canvas
        self.mosaic_place = np.array([(0, 0, w, h, (s % 2) * (w + 1), ((s // 2) % 2) * (h + 1)) for s in range(S)], np.int32)
        self.rects = np.array([(w // 3 + 7 * s + 1, h // 7 + s + 1, w // 4, h // 4) for s in range(S)], np.int32)
        self.cache = {}                                               # what the planners derive from the inputs alone


@functools.lru_cache(maxsize=None)
def inputs_for(seed, w, h, S, K, thr):
    """Made once per seed and shape and shared by every planner on them; read-only."""
    return Inputs(seed, w, h, S, K, thr)


# ---- the planner -----------------------------------------------------------------------------------------------------------
class _Round:
    def __init__(self):
        self.ops, self.calls, self.need, self.stages, self.checks, self.frames, self.applied = [], [], {}, [], [], [], []


class Planner:
    """The CPU side: simulates a round's families on numpy copies of the states, the held thumbnails and the walls BEFORE anything
    runs, so that every host-side argument and every expected output exist up front.  It touches no GPU."""

    def __init__(self, seed, w=160, h=140, S=3, K=4, mode="own", thr=20, draws=0):
        """seed: of the inputs; draws: of the planner's own choices (forms, budgets, random sequences)."""
        assert mode in MODES
        self.rng = np.random.default_rng([seed, draws])
        self.w, self.h, self.S, self.K, self.B, self.mode, self.thr = w, h, S, K, S * K, mode, thr
        self.n = n = 3 * w * h
        self.stride = n + 32 if n % 16 == 0 else n                    # a stride gap where the fast path allows one; else stride = N
        self.inp = inputs_for(seed, w, h, S, K, thr)
        self.nt = thumb_spec.thumb_bytes(w, h, THUMB_K)
        self.tiles, self.mw = ws.tiles(n), ws.mask_words(n)
        self.nc = 3 * self.inp.cw_ * self.inp.ch_
        self.capC = max(cwire_bytes_max(n, self.B), cwire_bytes_max(self.nc, 1))
        self.capE = max(self.B * n, self.nc)
        self.cache, self.deck = self.inp.cache, []
        self.stats = dict(ops={f: 0 for f in FAMILIES}, over_budget=0, kept={k: 0 for k in KINDS}, dropped={k: 0 for k in KINDS},
                          forms=set(), rebuilt=0, refresh=set(), thumb_entries=0, cancelled=0, split=set())

    # -- helpers ---------------------------------------------------------------------------------------------------------
    def buf(self, R, slot, name, count, dtype=U8):
        key = (slot, name)
        assert R.need.setdefault(key, (int(count), dtype)) == (int(count), dtype), key
        return key

    def check(self, R, what, key, want, view=None):
        R.checks.append((what, key, np.ascontiguousarray(want), view))

    def cached(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def records_out(self, R, slot, what, off, pos, recs, nrec, call):
        """The three outputs of a call that writes compact records: offsets, frame positions, records."""
        o, p, c = self.buf(R, slot, "off", self.B + 1, I32), self.buf(R, slot, "pos", self.B + 1, I64), self.buf(R, slot, "cw", self.capC)
        R.calls.append(lambda E: call(E, E.p(o), E.p(p), E.p(c), self.capC))
        self.check(R, what + " offsets", o, off, np.uint32)
        self.check(R, what + " frame_pos", p, pos, np.uint64)
        self.check(R, what + " records", c, recs)
        return c

    def arrays_out(self, R, slot, what, off, xs, df, call):
        o, x, d = self.buf(R, slot, "off", self.B + 1, I32), self.buf(R, slot, "xs", self.capE, I32), self.buf(R, slot, "df", self.capE)
        R.calls.append(lambda E: call(E, E.p(o), E.p(x), E.p(d), self.capE))
        self.check(R, what + " offsets", o, off, np.uint32)
        self.check(R, what + " xs", x, xs)
        self.check(R, what + " diff", d, df)

    def src(self, kind, which):
        """(the planner's record set, the key of the device buffer P wrote it to)."""
        return self.inp.kind[kind][which], ("P", f"{kind}_{which}_cw")

    def cover(self, R, slot, kind):
        """Queues the touched-tiles calls that make a mask covering the own burst and everything that moved the client states;
        -> (mask key, bool[S, tiles])."""
        S, K, n = self.S, self.K, self.n
        m = self.buf(R, slot, "mask", S * self.mw, I32)
        b, bkey = self.src(kind, "burst")
        sets = [(bkey, b, S, K)] + R.applied
        sel = np.zeros((S, self.tiles), bool)
        for i, (key, r, s_, k_) in enumerate(sets):
            R.calls.append(lambda E, key=key, r=r, k_=k_, acc=i > 0: E.core.cwire_touched_tiles_batch(
                E.p(key), r["counts"], r["escapes"], S, k_, E.p(m), accumulate=acc))
            o = r["off"].astype(np.int64)
            for s in range(S):
                sel[s] |= ws.touched(n, [r["xs"][o[s * k_]:o[(s + 1) * k_]]])
        changed = (self.cli != self.inp.base).reshape(S, -1)
        pad = np.zeros((S, self.tiles * ws.TILE), bool)
        pad[:, :n] = changed
        dirty = pad.reshape(S, self.tiles, ws.TILE).any(axis=2)
        assert not (dirty & ~sel).any(), "a tile of the client states changed that the mask does not cover"
        self.check(R, "tile mask", m, ws.mask_of(sel).reshape(-1), np.uint32)
        return m, sel

    # -- P -----------------------------------------------------------------------------------------------------------------
    def _produce(self, R, slot, kind, burst, tick):
        """The two producer calls of one kind into the buffers of `slot`, and their checks."""
        S, K, n, stride = self.S, self.K, self.n, self.stride
        for which, r in (("burst", burst), ("tick", tick)):
            nrec = r["B"]
            cap = cwire_bytes_max(n, nrec)
            o = self.buf(R, slot, f"{kind}_{which}_off", nrec + 1, I32)
            p = self.buf(R, slot, f"{kind}_{which}_pos", nrec + 1, I64)
            c = self.buf(R, slot, f"{kind}_{which}_cw", cap)
            if which == "burst":
                R.calls.append(lambda E, o=o, p=p, c=c, cap=cap: E.core.diff_multi_stream_cwire_batch(
                    E.frames[kind + "_burst"].ptr, E.st["snd_" + kind].ptr, S, K, E.p(o), E.p(p), E.p(c), cap, stride=stride))
            else:
                R.calls.append(lambda E, o=o, p=p, c=c, cap=cap: E.core.diff_multi_cwire_batch(
                    E.frames[kind + "_tick"].ptr, E.st["snd_" + kind].ptr, S, E.p(o), E.p(p), E.p(c), cap, stride=stride))
            self.check(R, f"{kind} {which} offsets", o, r["off"], np.uint32)
            self.check(R, f"{kind} {which} frame_pos", p, r["pos"], np.uint64)
            self.check(R, f"{kind} {which} records", c, r["recs"])

    def prime(self, R):
        """The start of every round: burst and tick of both kinds into the slot "P", which every consumer of the round reads."""
        for kind in KINDS:
            d = self.inp.kind[kind]
            self._produce(R, "P", kind, d["burst"], d["tick"])
        return "burst and tick of both kinds"

    def plan_P(self, R, slot, kind):
        """The producers once more, as a family of the round: the same frames against the sender states as they are by then (so
        mostly what did not pass the threshold before, and what B or D reverted), into buffers of its own.  The consumers behind
        it still read the priming records; what it is there for is a pipelined producer directly in front of them."""
        d, st = self.inp.kind[kind], self.snd[kind]
        burst, tick, after = self.cached(("P", kind, hash(st.tobytes())),
                                         lambda: produce(d["burst_frames"], d["tick_frames"], st, self.S, self.K, self.thr))
        self.snd[kind] = after.copy()
        self._produce(R, slot, kind, burst, tick)
        return f"the {kind} frames again: {int(burst['off'][-1])} and {int(tick['off'][-1])} entries"

    # -- A -----------------------------------------------------------------------------------------------------------------
    def plan_A(self, R, slot, kind):
        S, K, n, stride = self.S, self.K, self.n, self.stride
        form = int(self.rng.integers(0, 3))                           # the tick, the burst, the burst with output frames
        which, k_ = ("tick", 1) if form == 0 else ("burst", K)
        r, key = self.src(kind, which)
        shown = []
        for s in range(S):
            for k in range(k_):
                b = s * k_ + k
                cwire_apply_host(self.cli[s], r["recs"][int(r["pos"][b]):int(r["pos"][b + 1])], 1)
                shown.append(self.cli[s].copy())
        if form == 0:
            R.calls.append(lambda E: E.core.apply_multi_cwire_batch(E.p(key), r["counts"], r["escapes"], S, E.st["cli"].ptr, stride))
        else:
            fo = self.buf(R, slot, "fo", self.B, "frames") if form == 2 else None
            R.calls.append(lambda E: E.core.apply_multi_stream_cwire_batch(E.p(key), r["counts"], r["escapes"], S, K, E.st["cli"].ptr,
                                                                           stride, E.p(fo) if fo else None, stride))
            if fo:
                R.frames.append(("shown frames", fo, np.stack(shown)))
        R.applied.append((key, r, S, k_))
        return f"the {kind} {which}" + (" +frames" if form == 2 else "")

    # -- C, R, M -----------------------------------------------------------------------------------------------------------
    def plan_C(self, R, slot, kind):
        S, K, n = self.S, self.K, self.n
        r, key = self.src(kind, "burst")
        off, xs, df, out, pos = self.cached(("C", kind), lambda: _refs()[2](r["recs"], S, K, n))
        o = r["off"].astype(np.int64)
        self.stats["cancelled"] += sum(np.unique(r["xs"][o[s * K]:o[(s + 1) * K]]).size for s in range(S)) - int(off[S])
        compact = bool(self.rng.integers(0, 2))
        if compact:
            self.records_out(R, slot, "coalesced", off, pos, out, S, lambda E, a, b, c, cap: E.core.cwire_coalesce_cwire_batch(
                E.p(key), r["counts"], r["escapes"], S, K, a, b, c, cap))
        else:
            self.arrays_out(R, slot, "coalesced", off, xs, df, lambda E, a, b, c, cap: E.core.cwire_coalesce_batch(
                E.p(key), r["counts"], r["escapes"], S, K, a, b, c, cap))
        return f"the {kind} burst, " + ("records" if compact else "arrays")

    def plan_R(self, R, slot, kind):
        S, K = self.S, self.K
        r, key = self.src(kind, "burst")
        keep, compact = bool(self.rng.integers(0, 2)), bool(self.rng.integers(0, 2))
        rects = self.inp.rects
        off, xs, df, out, pos = self.cached(("R", kind, keep), lambda: crop_spec.reference(r["recs"], S, K, self.w, self.h, rects, keep))
        flags = lib.CROP_KEEP_INDEX if keep else 0
        if compact:
            self.records_out(R, slot, "cropped", off, pos, out, S, lambda E, a, b, c, cap: E.core.cwire_crop_cwire_batch(
                E.p(key), r["counts"], r["escapes"], S, K, rects, a, b, c, cap, flags=flags))
        else:
            self.arrays_out(R, slot, "cropped", off, xs, df, lambda E, a, b, c, cap: E.core.cwire_crop_batch(
                E.p(key), r["counts"], r["escapes"], S, K, rects, a, b, c, cap, flags=flags))
        return f"the {kind} burst, " + ("records" if compact else "arrays") + (", full-frame index" if keep else "")

    def plan_M(self, R, slot, kind):
        S, K, inp = self.S, self.K, self.inp
        r, key = self.src(kind, "burst")
        place, cw_, ch_ = inp.mosaic_place, inp.cw_, inp.ch_
        off, xs, df, out, pos = self.cached(("M", kind), lambda: mosaic_spec.reference(r["recs"], S, K, self.w, self.h, place, cw_, ch_))
        compact = bool(self.rng.integers(0, 2))
        if compact:
            self.records_out(R, slot, "canvas", off, pos, out, 1, lambda E, a, b, c, cap: E.core.cwire_mosaic_cwire_batch(
                E.p(key), r["counts"], r["escapes"], S, K, place, cw_, ch_, a, b, c, cap))
        else:
            self.arrays_out(R, slot, "canvas", off, xs, df, lambda E, a, b, c, cap: E.core.cwire_mosaic_batch(
                E.p(key), r["counts"], r["escapes"], S, K, place, cw_, ch_, a, b, c, cap))
        return f"the {kind} burst, " + ("records" if compact else "arrays")

    # -- B, D --------------------------------------------------------------------------------------------------------------
    def plan_B(self, R, slot, kind):
        """The header's rule from the records and the states as they are: a = |cur - prev| with cur the state's byte and prev =
        cur - diff; T_s from numpy's histogram (threshold_for) when the budget is below the count, the core's otherwise; above the
        core's threshold the entries with a <= T_s go and the state takes prev there."""
        threshold_for = _refs()[1]
        S, n, stride, thr0 = self.S, self.n, self.stride, self.thr
        r, key = self.src(kind, "tick")
        st = self.snd[kind]
        ns = [int(c) for c in r["counts"]]
        budgets = np.array([(NOLIMIT, c // 2, 1, 0)[int(self.rng.integers(0, 4))] for c in ns], np.uint32)
        budgets[0] = ns[0] // 2
        o = r["off"].astype(np.int64)
        thrs, segs = [], []
        for s in range(S):
            x, d = r["xs"][o[s]:o[s + 1]].astype(np.int64), r["df"][o[s]:o[s + 1]]
            cur = st[s][x].astype(np.int64)
            prev = (cur - d) & 255
            a = np.abs(cur - prev)
            T = threshold_for(a, thr0, int(budgets[s])) if int(budgets[s]) < ns[s] else thr0
            keep = a > T if T > thr0 else np.ones(x.size, bool)
            self.stats["over_budget"] += int(T > thr0)
            st[s][x[~keep]] = prev[~keep].astype(np.uint8)
            thrs.append(T); segs.append((x[keep], d[keep]))
        off, xs, df = crop_spec.packed(segs)
        recs, pos = spec.encode(off, xs, df)
        t = self.buf(R, slot, "aux", S, I32)
        self.records_out(R, slot, "budget", off, pos, recs, S, lambda E, a, b, c, cap: E.core.cwire_budget_cwire_batch(
            E.p(key), r["counts"], r["escapes"], E.st["snd_" + kind].ptr, S, budgets, E.p(t), a, b, c, cap, stride=stride))
        self.check(R, "thresholds", t, np.array(thrs, np.uint32), np.uint32)
        return f"the {kind} tick, budgets {[int(b) for b in budgets]} of {ns}"

    def plan_D(self, R, slot, kind):
        S, stride = self.S, self.stride
        r, key = self.src(kind, "tick")
        need = np.array([NEEDS[kind][s % 3] for s in range(S)], np.uint32)
        dropped, off, pos, recs, after, keeps = despeckle_spec.despeckle(self.w, self.h, r["recs"], self.snd[kind], need)
        self.snd[kind] = after
        self.stats["kept"][kind] += int(off[S])
        self.stats["dropped"][kind] += int(dropped.sum())
        t = self.buf(R, slot, "aux", S, I32)
        self.records_out(R, slot, "despeckled", off, pos, recs, S, lambda E, a, b, c, cap: E.core.cwire_despeckle_cwire_batch(
            E.p(key), r["counts"], r["escapes"], E.st["snd_" + kind].ptr, S, need, E.p(t), a, b, c, cap, stride=stride))
        self.check(R, "dropped", t, dropped, np.uint32)
        return f"the {kind} tick, need {[int(v) for v in need]}, dropped {[int(v) for v in dropped]}"

    # -- K, V --------------------------------------------------------------------------------------------------------------
    def plan_K(self, R, slot, kind):
        r, key = self.src(kind, "burst")
        want = self.cached(("K", kind), lambda: cwire_check_host(r["recs"], r["counts"], r["escapes"], self.n))
        assert not want[:, 0].any()
        v = self.buf(R, slot, "verd", 4 * self.B, I32)
        R.calls.append(lambda E: E.core.cwire_check_batch(E.p(key), r["counts"], r["escapes"], self.B, E.p(v)))
        self.check(R, "verdicts", v, want.reshape(-1), np.uint32)
        return f"the {kind} burst"

    def plan_V(self, R, slot, kind):
        oracle = _refs()[0]
        S, K, w, h = self.S, self.K, self.w, self.h
        cw_, ch_, mc = CELL
        ncells = activity_cells(w, h, cw_, ch_)[0]
        b, bkey = self.src(kind, "burst")
        t, tkey = self.src(kind, "tick")
        acc = bool(self.rng.integers(0, 2))
        c, m = self.buf(R, slot, "cells", S * ncells, I32), self.buf(R, slot, "summ", S * 8, I32)

        def make():
            first = oracle(w, h, cw_, ch_, mc, S, 1, t["off"], t["xs"])
            return first, oracle(w, h, cw_, ch_, mc, S, K, b["off"], b["xs"]), oracle(w, h, cw_, ch_, mc, S, K, b["off"], b["xs"], onto=first)
        first, alone, both = self.cached(("V", kind), make)
        if acc:                                                       # the tick clearing, then the burst on top of it
            R.calls.append(lambda E: E.core.cwire_activity_batch(E.p(tkey), t["counts"], t["escapes"], S, 1, cw_, ch_, E.p(c), E.p(m), mc))
        R.calls.append(lambda E: E.core.cwire_activity_batch(E.p(bkey), b["counts"], b["escapes"], S, K, cw_, ch_, E.p(c), E.p(m), mc, acc))
        want = both if acc else alone
        self.check(R, "cells", c, want[0].reshape(-1), np.uint32)
        self.check(R, "summary", m, want[1].reshape(-1), np.uint32)
        return f"the {kind} burst" + (" onto the tick's grid" if acc else "")

    # -- T, H, Y -----------------------------------------------------------------------------------------------------------
    def plan_T(self, R, slot, kind):
        S, inp, stride = self.S, self.inp, self.stride
        m, sel = self.cover(R, slot, kind)
        wl = self.buf(R, slot, "wall", inp.wall0.size)
        R.stages.append((wl, inp.wall0.reshape(-1)))
        places = np.array(inp.places, np.int32)
        R.calls.append(lambda E: E.core.wall_compose_batch(E.st["cli"].ptr, S, places, E.p(wl), inp.wall_w, inp.wall_h, d_tile_mask=E.p(m),
                                                           stride=stride))
        want = ws.compose(inp.wall0.copy(), self.cli, self.w, self.h, inp.places)
        self.check(R, "wall", wl, want.reshape(-1))
        return f"mask of the {kind} burst and {len(R.applied)} applied sets, {int(sel.sum())} tiles"

    def plan_H(self, R, slot, kind):
        S, stride = self.S, self.stride
        m, sel = self.cover(R, slot, kind)
        off, pos, recs, after = thumb_spec.batch(self.cli, self.held, self.w, self.h, THUMB_K, THUMB_THR, sel)
        self.held = after
        self.stats["thumb_entries"] += int(off[S])
        cap = cwire_bytes_max(self.nt, S)
        o, p, c = self.buf(R, slot, "off", self.B + 1, I32), self.buf(R, slot, "pos", self.B + 1, I64), self.buf(R, slot, "cw", self.capC)
        R.calls.append(lambda E: E.core.thumb_cwire_batch(E.st["cli"].ptr, S, THUMB_K, THUMB_THR, E.st["held"].ptr, E.p(o), E.p(p), E.p(c), cap,
                                                          d_tile_mask=E.p(m), stride=stride, thumb_stride=E.st["held"].stride))
        self.check(R, "thumbnail offsets", o, off, np.uint32)
        self.check(R, "thumbnail frame_pos", p, pos, np.uint64)
        self.check(R, "thumbnail records", c, np.frombuffer(b"".join(recs), np.uint8))
        return f"mask of the {kind} burst and {len(R.applied)} applied sets, {int(off[S])} entries"

    def plan_Y(self, R, slot, kind):
        S, n, stride = self.S, self.n, self.stride
        dig = np.stack([resync_spec.digest(self.cli[s]) for s in range(S)])
        sel = resync_spec.selected_tiles(self.snd[kind], dig)
        mask, off, recs, pos = resync_spec.refresh(self.snd[kind], sel)
        self.stats["refresh"].add("none" if not sel.any() else "all" if sel.all() else "some")
        self.cli[resync_spec.byte_selection(sel, n)] = 0
        d, m = self.buf(R, slot, "dig", 2 * S * self.tiles, I32), self.buf(R, slot, "mask", S * self.mw, I32)
        R.calls.append(lambda E: E.core.state_digest_batch(E.st["cli"].ptr, S, E.p(d), stride=stride))
        c = self.records_out(R, slot, "refresh", off, pos, recs, S, lambda E, a, b, c, cap: E.core.refresh_cwire_batch(
            E.st["snd_" + kind].ptr, S, E.p(d), E.p(m), a, b, c, cap, stride=stride))
        R.calls.append(lambda E: E.core.state_clear_tiles_batch(E.st["cli"].ptr, S, E.p(m), stride=stride))
        self.check(R, "digests", d, dig.reshape(-1), np.uint32)
        self.check(R, "refresh mask", m, mask.reshape(-1), np.uint32)
        counts, escapes = spec.headers(recs, S)
        _, xs, _ = spec.decode(recs, S)
        R.applied.append((c, dict(counts=counts, escapes=escapes, off=off, xs=xs), S, 1))   # what a later mask must cover
        return f"against the {kind} senders, {int(sel.sum())} of {sel.size} tiles"

    # -- S -----------------------------------------------------------------------------------------------------------------
    def split_sizes(self):
        """(piece capacity, piece bytes, group capacity, pitch): the largest over both kinds, so a slot's buffers keep their size."""
        out = []
        for kind in KINDS:
            r, M = self.inp.kind[kind]["tick"], SPLIT_M[kind]
            pcap = sum(cwire_split_pieces_max(c, e, M) for c, e in zip(r["counts"], r["escapes"]))
            out.append((pcap, sum(cwire_split_bytes_max(c, e, M) for c, e in zip(r["counts"], r["escapes"])),
                        cwire_fec_groups_max(pcap, self.S, FEC_G), M))
        return tuple(max(v) for v in zip(*out))

    def plan_S(self, R, slot, kind):
        S, M = self.S, SPLIT_M[kind]
        r, key = self.src(kind, "tick")
        pcap, capP, gcap, pitch_max = self.cached("split sizes", self.split_sizes)
        pitch = M
        capF = gcap * FEC_K * pitch_max

        def make():
            first, pos, out = split_spec.reference(r["recs"], S, M)
            total = int(first[S])
            assert total <= pcap and out.size <= capP and capP % 4 == 0
            ffirst, flen, par = fec_spec.reference(out, capP, first, pos, pcap, FEC_G, FEC_K, pitch, gcap, capF, GUARD)
            groups = int(ffirst[S])
            jobs, g = [], 0
            for rr in range(S):
                for j in range(int(ffirst[rr + 1]) - int(ffirst[rr])):
                    mem = fec_spec.members(first, FEC_G, rr, j)
                    if len(jobs) < MAX_JOBS and int(flen[g]):            # P alone, Q alone, both for two lost (one, in a group of one)
                        lost, hp, hq = [((0,), True, False), ((len(mem) - 1,), False, True), ((0, len(mem) - 1), True, True)][len(jobs) % 3]
                        jobs.append((g, mem, tuple(sorted(set(lost))), hp, hq))
                    g += 1
            tables = dict(job_first=np.cumsum([0] + [len(j[1]) for j in jobs]).astype(np.uint32),
                          slot_off=np.array([lib.FEC_ABSENT if i in j[2] else int(pos[p]) for j in jobs for i, p in enumerate(j[1])], np.uint64),
                          slot_len=np.array([int(pos[p + 1] - pos[p]) for j in jobs for p in j[1]], np.uint32),
                          parity_off=np.array([[capP + (j[0] * FEC_K) * pitch if j[3] else lib.FEC_ABSENT,
                                                capP + (j[0] * FEC_K + 1) * pitch if j[4] else lib.FEC_ABSENT] for j in jobs], np.uint64),
                          fec_len=np.array([int(flen[j[0]]) for j in jobs], np.uint32))
            rebuilt = np.full(2 * MAX_JOBS * pitch_max, GUARD, np.uint8)
            verdicts = np.zeros((len(jobs), 2), np.uint32)
            for i, (g, mem, lost, hp, hq) in enumerate(jobs):
                L = int(flen[g])
                slots = [None if k in lost else out[int(pos[p]):int(pos[p + 1])] for k, p in enumerate(mem)]
                P = par[(g * FEC_K) * pitch:(g * FEC_K) * pitch + L] if hp else None
                Q = par[(g * FEC_K + 1) * pitch:(g * FEC_K + 1) * pitch + L] if hq else None
                blocks, vd = fec_spec.repair(slots, P, Q, L)
                for k, blk in enumerate(blocks):
                    piece = out[int(pos[mem[lost[k]]]):int(pos[mem[lost[k]] + 1])]
                    assert np.array_equal(blk[:piece.size], piece) and not blk[piece.size:].any() and vd[k] == 0, "the lost piece comes back"
                    rebuilt[(2 * i + k) * pitch:(2 * i + k) * pitch + L] = blk
                    verdicts[i, k] = vd[k]
            sx = np.full(capP + capF, GUARD, np.uint8)
            sx[:out.size] = out
            sx[capP:] = par
            return first, pos[:total + 1], sx, ffirst, flen[:groups], jobs, tables, rebuilt, verdicts
        first, pos, sx, ffirst, flen, jobs, tb, rebuilt, verdicts = self.cached(("S", kind), make)
        self.stats["rebuilt"] += sum(len(j[2]) for j in jobs)
        self.stats["split"].add((kind, int(np.diff(first.astype(np.int64)).max())))
        pf, pp, x = self.buf(R, slot, "pf", S + 1, I32), self.buf(R, slot, "pp", pcap + 1, I64), self.buf(R, slot, "sx", capP + capF)
        ff, fl = self.buf(R, slot, "ff", S + 1, I32), self.buf(R, slot, "fl", gcap, I32)
        rp, vd = self.buf(R, slot, "rep", 2 * MAX_JOBS * pitch_max), self.buf(R, slot, "vd", 2 * MAX_JOBS, I32)
        R.calls.append(lambda E: E.core.cwire_split_cwire_batch(E.p(key), r["counts"], r["escapes"], S, M, E.p(pf), E.p(pp), pcap, E.p(x), capP))
        R.calls.append(lambda E: E.core.cwire_fec_batch(E.p(x), capP, E.p(pf), E.p(pp), pcap, S, FEC_G, FEC_K, pitch, E.p(ff), E.p(fl), gcap,
                                                        E.p(x) + capP, capF))
        if jobs:
            R.calls.append(lambda E: E.core.cwire_fec_repair_batch(E.p(x), capP + capF, len(jobs), tb["job_first"], tb["slot_off"], tb["slot_len"],
                                                                   tb["parity_off"], tb["fec_len"], E.p(rp), pitch, E.p(vd)))
        self.check(R, "piece_first", pf, first, np.uint32)
        self.check(R, "piece_pos", pp, pos, np.uint64)
        self.check(R, "pieces and parity", x, sx)
        self.check(R, "fec_first", ff, ffirst, np.uint32)
        self.check(R, "fec_len", fl, flen, np.uint32)
        if jobs:
            self.check(R, "rebuilt pieces", rp, rebuilt[:2 * len(jobs) * pitch])
            self.check(R, "repair verdicts", vd, verdicts.reshape(-1), np.uint32)
        return f"the {kind} tick at {M} bytes: {int(first[S])} pieces, {int(ffirst[S])} groups, {len(jobs)} repair jobs"

    # -- U -----------------------------------------------------------------------------------------------------------------
    def plan_U(self, R, slot, kind):
        B, n = self.B, self.n
        r, key = self.src(kind, "burst")
        forms, pos, link = self.cached(("U", kind), lambda: runs_spec.encode(r["recs"], B, runs_spec.WHERE_SMALLER))
        self.stats["forms"] |= {int(f) for f in forms[:, 0]}
        fpos, back = runs_spec.decode(link, forms)
        assert np.array_equal(back, r["recs"]) and np.array_equal(fpos, r["pos"]), "the decode returns the input byte for byte"
        capL = cwire_runs_bytes_max(n, B, lib.RUNS_WHERE_SMALLER)
        f, p, l = self.buf(R, slot, "forms", 4 * B, I32), self.buf(R, slot, "pos", B + 1, I64), self.buf(R, slot, "link", capL)
        p2, c2 = self.buf(R, slot, "pos2", B + 1, I64), self.buf(R, slot, "cw", self.capC)
        R.calls.append(lambda E: E.core.cwire_runs_encode_batch(E.p(key), r["counts"], r["escapes"], B, lib.RUNS_WHERE_SMALLER, E.p(f), E.p(p),
                                                                E.p(l), capL))
        R.calls.append(lambda E: E.core.cwire_runs_decode_batch(E.p(l), forms, B, E.p(p2), E.p(c2), self.capC))
        self.check(R, "forms", f, forms.reshape(-1), np.uint32)
        self.check(R, "link positions", p, pos, np.uint64)
        self.check(R, "link bytes", l, link)
        self.check(R, "decoded frame_pos", p2, r["pos"], np.uint64)
        self.check(R, "decoded records", c2, r["recs"])
        return f"the {kind} burst, forms {sorted({int(v) for v in forms[:, 0]})}"

    # -- a round -----------------------------------------------------------------------------------------------------------
    def plan_round(self, seq):
        """seq: [(family, kind)] behind P -> the planned round."""
        inp = self.inp
        R = _Round()
        self.snd = {k: inp.kind[k]["snd"].copy() for k in KINDS}
        self.cli, self.held = inp.base.copy(), inp.held.copy()
        R.ops.append("prime: " + self.prime(R))
        for slot, (fam, kind) in enumerate(seq):
            assert fam in FAMILIES and kind in KINDS
            what = getattr(self, "plan_" + fam)(R, slot, kind)
            self.stats["ops"][fam] += 1
            R.ops.append(f"{fam} [slot {slot}] {what}")
        R.states = {"snd_loud": self.snd["loud"].copy(), "snd_quiet": self.snd["quiet"].copy(), "cli": self.cli.copy(),
                    "held": self.held.copy()}
        return R

    def random_sequence(self):
        """4 to 8 (family, kind) drawn without replacement from the 28 there are; the deck is shuffled anew when it runs out, so
        a dozen rounds reach every family on both kinds."""
        out = []
        for _ in range(int(self.rng.integers(4, 9))):
            if not self.deck:
                self.deck = [(f, k) for f in FAMILIES for k in KINDS]
                self.rng.shuffle(self.deck)
            out.append(tuple(self.deck.pop()))
        return out


class Family:
    def __init__(self, name, calls, reads):
        self.name, self.calls, self.reads = name, calls, reads


# One entry per family: its name, the entry points it queues (Planner.plan_<letter> holds the plan, the calls and the checks), and
# what of the producers' output it reads.
FAMILIES = {
    "P": Family("produce", ("mi355_diff_multi_stream_cwire_batch", "mi355_diff_multi_cwire_batch"), None),
    "A": Family("apply", ("mi355_apply_multi_cwire_batch", "mi355_apply_multi_stream_cwire_batch"), "tick or burst"),
    "C": Family("coalesce", ("mi355_cwire_coalesce_cwire_batch", "mi355_cwire_coalesce_batch"), "burst"),
    "B": Family("budget", ("mi355_cwire_budget_cwire_batch",), "tick"),
    "D": Family("despeckle", ("mi355_cwire_despeckle_cwire_batch",), "tick"),
    "R": Family("crop", ("mi355_cwire_crop_cwire_batch", "mi355_cwire_crop_batch"), "burst"),
    "M": Family("mosaic", ("mi355_cwire_mosaic_cwire_batch", "mi355_cwire_mosaic_batch"), "burst"),
    "K": Family("check", ("mi355_cwire_check_batch",), "burst"),
    "V": Family("activity", ("mi355_cwire_activity_batch",), "tick and burst"),
    "T": Family("touched + wall", ("mi355_cwire_touched_tiles_batch", "mi355_wall_compose_batch"), "burst"),
    "H": Family("thumb", ("mi355_cwire_touched_tiles_batch", "mi355_thumb_cwire_batch"), "burst"),
    "Y": Family("resync", ("mi355_state_digest_batch", "mi355_refresh_cwire_batch", "mi355_state_clear_tiles_batch"), None),
    "S": Family("datagram", ("mi355_cwire_split_cwire_batch", "mi355_cwire_fec_batch", "mi355_cwire_fec_repair_batch"), "tick"),
    "U": Family("runs", ("mi355_cwire_runs_encode_batch", "mi355_cwire_runs_decode_batch"), "burst"),
}
# The entry points of include/mi355diff.h that take h_counts and h_escapes and are in no family, each with its reason
LEFT_OUT = {
    "mi355_cwire_decode_batch": "chained by the older sweep (soak_chain family f) on the one-stream records this chain does not make",
    "mi355_apply_cwire_batch": "chained by the older sweep (soak_chain family g): it moves the core's own state, which no call here reads",
    "mi355_cwire_split_host": "a host form: no core, no scratch",
    "mi355_cwire_runs_encode_host": "a host form: no core, no scratch",
    "mi355_cwire_despeckle_host": "a host form: no core, no scratch",
    "mi355_cwire_check_host": "a host form: no core, no scratch",
}


def sweep_sequences(A, orientation):
    """The sweep's rounds of case A in one orientation: for every family B the round (A on one kind, B on the other)."""
    ka, kb = KINDS[orientation], KINDS[1 - orientation]
    return [[(A, ka), (B, kb)] for B in FAMILIES]


# ---- the GPU side ----------------------------------------------------------------------------------------------------------
class Env:
    """The core (the product class, so nothing synchronises behind the chain's back), the frames, the sets of states and the
    output buffers, every one guarded (tests/gpu_util.py)."""

    def __init__(self, p, prepare=0, core=None):
        import gpu_util
        from cudavideostream_amd import CUDACore
        assert gpu_util.GUARD == GUARD
        self.plan, self.bufs = p, {}
        self.core = CUDACore(p.w, p.h, max_batch=p.B, threshold=p.thr) if core is None else core
        if prepare:
            self.core.prepare(prepare)
        if p.mode == "sequential":
            self.core.set_option(lib.OPT_PIPELINE, 0)
        if p.mode == "callers":
            self.core.use_torch_stream()
        n, S, stride = p.n, p.S, p.stride
        self.frames = {}
        for kind in KINDS:
            d = p.inp.kind[kind]
            self.frames[kind + "_burst"] = gpu_util.Region(p.B, n, stride).put(d["burst_frames"])
            self.frames[kind + "_tick"] = gpu_util.Region(S, n, stride).put(d["tick_frames"])
        self.st = {k: gpu_util.Region(S, n, stride) for k in ("snd_loud", "snd_quiet", "cli")}
        self.st["held"] = gpu_util.Region(S, p.nt, p.nt + 16 if p.nt % 16 == 0 else p.nt + 5, 0 if p.nt % 16 == 0 else 1)

    def p(self, key):
        return self.bufs[key].ptr

    def close(self):
        self.core.close()

    def run_round(self, R):
        """Uploads, one torch synchronisation, the calls with nothing in between, one synchronisation of the core and one of
        torch; then -> the list of mismatches (empty: the round is right)."""
        import torch
        from gpu_util import Guarded, Region, to_dev
        p, inp = self.plan, self.plan.inp
        dt = {I32: torch.int32, I64: torch.int64, U8: torch.uint8}
        for key, (count, dtype) in R.need.items():
            b = self.bufs.get(key)
            if b is None:
                b = self.bufs[key] = Region(count, p.n, p.stride) if dtype == "frames" else Guarded(count, dt[dtype])
            assert (b.S if dtype == "frames" else b.count) == count, key
            b.buf.fill_(GUARD if dtype == "frames" else b.fill)
        for key, data in R.stages:
            self.bufs[key].t[:len(data)].copy_(to_dev(data))
        for k in KINDS:
            self.st["snd_" + k].put(inp.base)
        self.st["cli"].put(inp.base)
        self.st["held"].put(inp.held)
        torch.cuda.synchronize()
        for call in R.calls:
            call(self)
        self.core.synchronize()
        torch.cuda.synchronize()
        bad = []
        try:
            for what, key, want, view in R.checks:
                got = self.bufs[key].get(written=len(want))[:len(want)]
                if not np.array_equal(got.view(view) if view else got, want):
                    bad.append(f"{what} (slot {key[0]})")
            wrote = {key: (what, rows) for what, key, rows in R.frames}
            for key, (count, dtype) in R.need.items():
                if dtype == "frames":
                    got = self.bufs[key].get()
                    what, rows = wrote[key]
                    if not np.array_equal(got[:len(rows)], rows) or not (got[len(rows):] == GUARD).all():
                        bad.append(f"{what} (slot {key[0]})")
            for k, want in R.states.items():
                if not np.array_equal(self.st[k].get(), want):
                    bad.append(f"the states {k}")
            for k, fr in self.frames.items():
                kind, which = k.split("_")
                if not np.array_equal(fr.get(), inp.kind[kind][which + "_frames"]):
                    bad.append(f"the input frames {k}")
        except AssertionError as e:                                  # a guard of gpu_util
            bad.append(f"guard bytes: {e}")
        return bad


def run_sequences(p, E, seqs, label):
    """Plans and runs the rounds one by one; -> None, or the report of the first round that is wrong."""
    for i, seq in enumerate(seqs):
        R = p.plan_round(seq)
        bad = E.run_round(R)
        if bad:
            return (f"{label}, round {i} ({p.w}x{p.h}, S {p.S}, K {p.K}, mode {p.mode}): wrong: " + "; ".join(bad) +
                    "\n  operations:\n    " + "\n    ".join(R.ops))
    return None

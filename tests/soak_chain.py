#!/usr/bin/env python3
"""Chain soak: random sequences of entry points on long-lived cores, queued WITHOUT host synchronisation between them, through
buffers that are reused all the time.  A round is synchronised once at its end and every output of the round compared with a
reference that was computed before the round's first call.  What it is after: ordering between the streams a pipelined batch
uses inside the library (core.hip, run_batch / use_device) and the reuse of per-core scratch, not arithmetic.

Two runners.  run(): ONE core -- frame filter into a scratch, stream batch out of that scratch, pair batches of both operand
forms, dense batches (after which the library stops overlapping batches until the input is sparse again), the red map of a
batch's packed stream, switches between the core's stream and a caller's.  run_wire(): the compact-wire and many-streams family
-- ticks and bursts of caller-held states in their three forms, their GPU clients, the coalescer, the budget call, the one-stream
compact forms with encoder and decoder, pairs over the caller's states -- on a sender core and a relay/client core, or on one
core in all roles (the operations are listed above WirePlanner).

Part of the suite in short form: tests/test_diff_pack_gpu.py::test_chain_soak_short runs run(), tests/test_chain_wire_gpu.py
runs run_wire() in every mode, a deterministic sweep over every ordered pair of its operation families, and the host-side
checks that the random chains are not trivial.  The long form is this script:
    python tests/soak_chain.py [rounds] [seed]      exits non-zero on the first mismatch"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudavideostream_amd import CUDACore, lib, synth  # noqa: E402
from oracle import pyoracle as po  # noqa: E402  (checker)

DEV = "cuda:0"


def oracle_pairs(cur, prev):
    offs, xs, df = [0], [], []
    for t in range(cur.shape[0]):
        c, x, d, _ = po.diff_pack(cur[t], prev[t], 20)
        offs.append(offs[-1] + c); xs.append(x); df.append(d)
    return (np.array(offs, np.uint32), np.concatenate(xs) if xs else np.empty(0, np.int32),
            np.concatenate(df) if df else np.empty(0, np.uint8))


def run(rounds, seed, w=320, h=180, T=5, verbose=True, flags=0):
    rng = np.random.default_rng(seed)
    n = 3 * w * h
    k9 = po.gaussian_kernel(3, 1.5)
    base, pool = synth.webcam_stream(64, w, h, seed=seed + 1)
    pool = np.ascontiguousarray(pool)
    d_pool = torch.from_numpy(pool).to(DEV)
    noise = rng.integers(0, 256, (2 * T, n), dtype=np.uint8)   # dense input: nearly every byte changes (the library then stops
    d_noise = torch.from_numpy(noise).to(DEV)                  # overlapping batches once such a batch's total has arrived)
    scratch = torch.empty((T, n), dtype=torch.uint8, device=DEV)      # filter output = batch input, rewritten every time
    vis = torch.empty((T, n), dtype=torch.uint8, device=DEV)
    nout = 6
    outs = [(torch.zeros(T + 1, dtype=torch.int32, device=DEV), torch.empty(T * n, dtype=torch.int32, device=DEV),
             torch.empty(T * n, dtype=torch.uint8, device=DEV)) for _ in range(nout)]
    core = CUDACore(w, h, k=k9, max_batch=T, sample_mat_data=base, flags=flags)
    state = base.copy()
    own = True
    for rnd in range(rounds):
        checks = []   # (what, output slot, expectation)
        red_expect = None
        nops = int(rng.integers(2, nout + 1))
        torch.cuda.synchronize()
        for i in range(nops):
            op = int(rng.integers(0, 7))
            if int(rng.integers(0, 24)) == 0:
                op = 7       # (rarely: the oracle sorts 25 bytes per output byte)
            if int(rng.integers(0, 16)) == 0:   # (round 6) mi355_prepare in the middle of queued work: blocking, changes nothing
                mask = int(rng.integers(1, 32))
                if os.environ.get("SOAK_PREPARE", "1") != "0":
                    core.prepare(mask)
            if int(rng.integers(0, 40)) == 0:   # (round 6) the index kernel's launch tag put in front of its wrap: the totals are cleared
                left = int(rng.integers(1, 4))
                if os.environ.get("SOAK_EPOCH", "1") != "0":
                    core.set_option(lib.OPT_SCAN_EPOCH_LEFT, left)   # (set_option completes what is queued)
            f0 = int(rng.integers(0, 64 - 2 * T))
            o = outs[i]
            if op == 0:      # stream batch straight from the pool
                core.diff_stream_batch(d_pool[f0:f0 + T], T, *o, T * n)
                eo, exs, edf, state = po.diff_stream(pool[f0:f0 + T], state)
                checks.append(("stream", o, (eo, exs, edf)))
            elif op == 1:    # noise filter into the scratch, stream batch out of it
                core.filter_batch(lib.OP_CONV3X3, d_pool[f0:f0 + T], scratch, T)
                core.diff_stream_batch(scratch, T, *o, T * n)
                filt = np.stack([po.conv3x3(f, w, h, k9) for f in pool[f0:f0 + T]])
                eo, exs, edf, state = po.diff_stream(filt, state)
                checks.append(("conv+stream", o, (eo, exs, edf)))
            elif op == 7:    # 5x5 median (column-strip kernel: 960-byte rows) into the scratch, stream batch out of it
                core.filter_batch(lib.OP_MEDIAN5X5, d_pool[f0:f0 + T], scratch, T)
                core.diff_stream_batch(scratch, T, *o, T * n)
                filt = np.stack([po.median5x5(f, w, h) for f in pool[f0:f0 + T]])
                eo, exs, edf, state = po.diff_stream(filt, state)
                checks.append(("median+stream", o, (eo, exs, edf)))
            elif op == 2:    # pairs of consecutive frames
                core.diff_pairs_batch(d_pool[f0 + 1:f0 + T + 1], d_pool[f0:f0 + T], T, *o, T * n)
                checks.append(("pairs", o, oracle_pairs(pool[f0 + 1:f0 + T + 1], pool[f0:f0 + T])))
            elif op == 3:    # pairs that share no frame
                blk, hb = d_pool[f0:f0 + 2 * T], pool[f0:f0 + 2 * T]
                core.diff_pairs_batch(blk[1::2], blk[0::2], T, *o, T * n, stride=2 * n)
                checks.append(("pairs apart", o, oracle_pairs(hb[1::2], hb[0::2])))
            elif op == 4 and checks and checks[-1][0] in ("stream", "conv+stream", "median+stream"):   # red map of the batch before
                prev_o = checks[-1][1]
                core.red_stream_batch(prev_o[0], prev_o[1], T, vis, True)
                eo, exs, _ = checks[-1][2]
                red_expect = np.zeros((T, n), np.uint8)
                for t in range(T):
                    red_expect[t] = po.red_overlap(red_expect[t], exs[eo[t]:eo[t + 1]])
            elif op == 6:    # a dense stream batch
                g0 = int(rng.integers(0, T + 1))
                core.diff_stream_batch(d_noise[g0:g0 + T], T, *o, T * n)
                eo, exs, edf, state = po.diff_stream(noise[g0:g0 + T], state)
                checks.append(("dense stream", o, (eo, exs, edf)))
            else:            # switch streams (a synchronising call by contract)
                own = not own
                (core.use_own_stream if own else core.use_torch_stream)()
        core.synchronize()
        torch.cuda.synchronize()
        for what, o, exp in checks:
            eo, exs, edf = exp
            tot = int(eo[-1])
            ok = (np.array_equal(o[0].cpu().numpy().view(np.uint32), eo) and np.array_equal(o[1][:tot].cpu().numpy(), exs)
                  and np.array_equal(o[2][:tot].cpu().numpy(), edf))
            if not ok:
                print(f"MISMATCH in round {rnd} ({what}); seed {seed}")
                return False
        if red_expect is not None and not np.array_equal(vis.cpu().numpy(), red_expect):   # the round's last red map
            print(f"MISMATCH in round {rnd} (red map); seed {seed}")
            return False
        if not np.array_equal(core.get_state(), state):
            print(f"MISMATCH in round {rnd} (state); seed {seed}")
            return False
        if verbose and rnd % 25 == 0:
            print(f"round {rnd} ok", flush=True)
    core.close()
    return True


# ---- the compact-wire and many-streams family -------------------------------------------------------------------------------
NOLIMIT = 0xFFFFFFFF
MODES = ("own", "sequential", "callers")      # the core's streams pipelined, OPT_PIPELINE 0, the caller's (torch's) stream
FAMILIES = "abcdefghij"
_WEIGHTED = "aabbcccdddeeeffgghijj"      # the consumers (c, d, e, g, j) are redrawn often: their shares make up for it
NSLOTS = 8


def _refs():
    """The numpy statements the suite already has (imported on first use: they live in test modules)."""
    import cwire_spec as spec
    from cudavideostream_amd import cwire_apply_host, cwire_bytes_max
    from test_cwire_coalesce_gpu import reference as coalesce_reference
    from test_cwire_round_seams_gpu import expected as budget_expected, numpy_tick
    return spec, cwire_apply_host, cwire_bytes_max, coalesce_reference, numpy_tick, budget_expected


class _Round:
    """One planned round: the calls (functions of the environment that holds cores and buffers), what to upload before the first
    of them, and what every output buffer must hold after the synchronisation."""

    def __init__(self):
        self.ops, self.calls, self.stages, self.checks, self.frames, self.dirty = [], [], [], [], [], set()


class WirePlanner:
    """The CPU side of run_wire: draws a round's operations and simulates them on numpy states BEFORE anything runs, so that
    every header the GPU calls take from the host (h_counts, h_escapes, h_budget) and every expected output exist up front.
    It touches no GPU: wire_stats() and the validity test of tests/test_chain_wire_gpu.py run it alone.

    Core 0 is the sender, core 1 the relay/client (core 0 again with one_core).  Caller-held states: `snd` (the sender's, core
    0), `rly` (a relay that checks what it forwards, core 0), `cli` and `thd` (a client and the receiver of coalesced records,
    core 1); each core's own state.  Operations, one output slot each:
      a  tick            diff_multi_{cwire,-,wire}_batch of S frames on snd
      b  burst           diff_multi_stream_{cwire,-,wire}_batch(S, K) on snd
      c  relay check     apply_multi_* / apply_multi_stream_* (with or without output frames) of the latest a / b / e / i
                         onto rly (core 0) or cli (core 1)
      d  coalesce        cwire_coalesce_{cwire_,}batch of the latest compact burst on core 0; compact: then
                         apply_multi_cwire_batch of its records onto thd on core 1
      e  budget          cwire_budget_cwire_batch of the latest compact tick on snd (no limit, half the count, 1, 0); its
                         thinned records are what a later c applies, and the next a / b diffs against the thinned states
      f  one stream      diff_stream_cwire_batch(K) on core 0's own state, or diff_stream_batch + cwire_encode_batch +
                         cwire_decode_batch
      g  client          apply_cwire_batch of the latest f onto core 1's own state
      h  pairs           diff_pairs_batch of S frames against snd (either operand)
      i  dense           a or b on random frames (nearly every byte changes: the adaptive schedule stops overlapping)
      j  red map         red_stream_batch over the stream f decoded
      k  rarely          prepare(mask), OPT_SCAN_EPOCH_LEFT 1..3, OPT_PIPELINE 0 / 1, own stream <-> torch's stream
    A consumer on another core than its producer's is ordered by the library only when both cores are on torch's stream
    (include/mi355diff.h, "Streams"); otherwise it reads a staged copy of the REFERENCE's bytes, uploaded before the round --
    the records a receiver took from its sockets.  On one core, and on a caller's stream, every consumer reads what the GPU
    call before it wrote."""

    def __init__(self, seed, w=160, h=140, S=3, K=4, mode="own", one_core=False, thr=20):
        assert mode in MODES
        self.rng = np.random.default_rng(seed)
        self.w, self.h, self.S, self.K, self.B, self.mode, self.one_core, self.thr = w, h, S, K, S * K, mode, one_core, thr
        self.n = n = 3 * w * h
        self.stride = n + 32 if n % 16 == 0 else n          # a stride gap where the fast path allows one; else stride = N
        distinct = np.stack([synth.webcam_frame(t, w, h, seed=seed + 1) for t in range(6)])
        self.base = synth.webcam_frame(-1, w, h, seed=seed + 1)
        # few distinct pictures in random order: a burst sees a picture come back, so differences cancel in the coalescer
        self.pool = np.ascontiguousarray(distinct[self.rng.integers(0, 6, 4 * self.B)])
        self.noise = self.rng.integers(0, 256, (self.B + 4, n), dtype=np.uint8)
        self.snd, self.rly, self.cli, self.thd = (np.tile(self.base, (S, 1)) for _ in range(4))
        self.own = [self.base.copy(), self.base.copy()]
        self.Y = 0 if one_core else 1
        self.on_torch = [mode == "callers"] * 2
        self.pipeline = [mode != "sequential"] * 2
        self.stats = dict(ops={c: 0 for c in FAMILIES + "k"}, records=0, nonempty=0, escapes=0, escaped_records=0,
                          over_budget=0, cancelled=0, staged=0)

    # -- helpers ---------------------------------------------------------------------------------------------------------
    def _staged(self, producer, consumer):
        return producer != consumer and not (self.on_torch[producer] and self.on_torch[consumer])

    def _count(self, counts, escapes=None):
        st = self.stats
        st["records"] += len(counts)
        st["nonempty"] += int((np.asarray(counts) > 0).sum())
        if escapes is not None:
            st["escapes"] += int(np.asarray(escapes).sum())
            st["escaped_records"] += int((np.asarray(escapes) > 0).sum())

    def _source(self, R, src, consumer):
        """-> the name prefix of the buffers a consumer of `src` (a tick or a one-stream batch) reads: the producer's outputs,
        or the staged reference."""
        if not self._staged(src["core"], consumer):
            return ""
        self.stats["staged"] += 1
        if src["form"] == "arrays":
            R.stages += [(src["slot"], "s_off", src["off"].view(np.int32)), (src["slot"], "s_xs", src["xs"]),
                         (src["slot"], "s_df", src["df"])]
        else:
            R.stages.append((src["slot"], "s_b", src["recs"] if src["form"] == "cwire" else src["wire"]))
        return "s_"

    # -- a, b, i ---------------------------------------------------------------------------------------------------------
    def _tick(self, R, slot, K, dense, form=None):
        spec = _refs()[0]
        rng, S, n, thr, stride = self.rng, self.S, self.n, self.thr, self.stride
        B = S * K
        name, src = ("noise", self.noise) if dense else ("pool", self.pool)
        f0 = int(rng.integers(0, len(src) - B + 1))
        frames, pre = src[f0:f0 + B], self.snd.copy()
        offs, xs, df = [0], [], []
        for s in range(S):
            o, x, d, st = po.diff_stream(frames[s * K:(s + 1) * K], self.snd[s], thr)
            offs += [offs[-1] + int(v) for v in o[1:]]; xs.append(x); df.append(d)
            self.snd[s] = st
        off, xs, df = np.array(offs, np.uint32), np.concatenate(xs).astype(np.int32), np.concatenate(df).astype(np.uint8)
        form = form or ("cwire", "cwire", "cwire", "cwire", "arrays", "wire")[int(rng.integers(0, 6))]
        t = dict(kind="a" if K == 1 else "b", K=K, form=form, slot=slot, off=off, xs=xs, df=df, pre=pre, frames=frames, core=0,
                 budgeted=False)
        capE, capC, capW = self.B * n, self.capC, self.capW
        fr = lambda E: getattr(E, name).ptr + f0 * stride
        R.checks.append(("offsets", slot, "off", off, np.uint32))
        if form == "cwire":
            t["recs"], t["pos"] = spec.encode(off, xs, df)
            t["counts"], t["escapes"] = spec.headers(t["recs"], B)
            assert np.array_equal(t["counts"], np.diff(off.astype(np.int64)))
            self._count(t["counts"], t["escapes"])
            if K == 1:
                R.calls.append(lambda E: E.core[0].diff_multi_cwire_batch(fr(E), E.st["snd"].ptr, S, E.p(slot, "off"), E.p(slot, "pos"),
                                                                          E.p(slot, "cw"), capC, stride=stride))
            else:
                R.calls.append(lambda E: E.core[0].diff_multi_stream_cwire_batch(fr(E), E.st["snd"].ptr, S, K, E.p(slot, "off"),
                                                                                 E.p(slot, "pos"), E.p(slot, "cw"), capC, stride=stride))
            R.checks += [("frame_pos", slot, "pos", t["pos"], np.uint64), ("records", slot, "cw", t["recs"], None)]
        elif form == "arrays":
            self._count(np.diff(off.astype(np.int64)))
            if K == 1:
                R.calls.append(lambda E: E.core[0].diff_multi_batch(fr(E), E.st["snd"].ptr, S, E.p(slot, "off"), E.p(slot, "xs"),
                                                                    E.p(slot, "df"), capE, stride=stride))
            else:
                R.calls.append(lambda E: E.core[0].diff_multi_stream_batch(fr(E), E.st["snd"].ptr, S, K, E.p(slot, "off"), E.p(slot, "xs"),
                                                                           E.p(slot, "df"), capE, stride=stride))
            R.checks += [("xs", slot, "xs", xs, None), ("diff", slot, "df", df, None)]
        else:
            t["wire"] = po.wire_pack(off, xs, df)
            self._count(np.diff(off.astype(np.int64)))
            if K == 1:
                R.calls.append(lambda E: E.core[0].diff_multi_wire_batch(fr(E), E.st["snd"].ptr, S, E.p(slot, "off"), E.p(slot, "wire"),
                                                                         capW, stride=stride))
            else:
                R.calls.append(lambda E: E.core[0].diff_multi_stream_wire_batch(fr(E), E.st["snd"].ptr, S, K, E.p(slot, "off"),
                                                                                E.p(slot, "wire"), capW, stride=stride))
            R.checks.append(("wire bytes", slot, "wire", t["wire"], None))
        self.tick = t
        return f"{form} K={K}" + (" dense" if dense else "")

    def op_a(self, R, slot, hint):
        return self._tick(R, slot, 1, False, hint.get("form"))

    def op_b(self, R, slot, hint):
        return self._tick(R, slot, self.K, False, hint.get("form"))

    def op_i(self, R, slot, hint):
        K = hint.get("K") or (1 if int(self.rng.integers(0, 2)) else self.K)
        return self._tick(R, slot, K, True, hint.get("form"))

    # -- c ---------------------------------------------------------------------------------------------------------------
    def op_c(self, R, slot, hint):
        apply_host = _refs()[1]
        t, rng, S, n, stride = self.tick, self.rng, self.S, self.n, self.stride
        if t is None:
            return None
        K, form, src = t["K"], t["form"], t["slot"]
        core = 0 if int(rng.integers(0, 2)) else self.Y
        which = ("rly", "cli")[int(rng.integers(0, 2))] if self.one_core else ("rly" if core == 0 else "cli")
        burst = K > 1 or bool(rng.integers(0, 2))
        out = burst and bool(rng.integers(0, 2))
        st, off, shown = getattr(self, which), t["off"].astype(np.int64), []
        for s in range(S):
            for k in range(K):
                b = s * K + k
                if form == "cwire":
                    apply_host(st[s], t["recs"][int(t["pos"][b]):int(t["pos"][b + 1])], 1)
                else:
                    st[s][t["xs"][off[b]:off[b + 1]]] += t["df"][off[b]:off[b + 1]]
                shown.append(st[s].copy())
        pre = self._source(R, t, core)
        fo = (lambda E: E.slot[slot]["fo"].ptr) if out else (lambda E: None)
        counts = np.diff(off).astype(np.uint32)
        if form == "cwire":
            cw = "s_b" if pre else "cw"
            if burst:
                R.calls.append(lambda E: E.core[core].apply_multi_stream_cwire_batch(E.p(src, cw), t["counts"], t["escapes"], S, K,
                                                                                      E.st[which].ptr, stride, fo(E), stride))
            else:
                R.calls.append(lambda E: E.core[core].apply_multi_cwire_batch(E.p(src, cw), t["counts"], t["escapes"], S,
                                                                               E.st[which].ptr, stride))
        elif form == "arrays":
            a = [pre + x for x in ("off", "xs", "df")]
            if burst:
                R.calls.append(lambda E: E.core[core].apply_multi_stream_batch(E.p(src, a[0]), E.p(src, a[1]), E.p(src, a[2]), S, K,
                                                                                E.st[which].ptr, stride, fo(E), stride))
            else:
                R.calls.append(lambda E: E.core[core].apply_multi_batch(E.p(src, a[0]), E.p(src, a[1]), E.p(src, a[2]), S,
                                                                         E.st[which].ptr, stride))
        else:
            wb = "s_b" if pre else "wire"
            if burst:
                R.calls.append(lambda E: E.core[core].apply_multi_stream_wire_batch(E.p(src, wb), counts, S, K, E.st[which].ptr, stride,
                                                                                     fo(E), stride))
            else:
                R.calls.append(lambda E: E.core[core].apply_multi_wire_batch(E.p(src, wb), counts, S, E.st[which].ptr, stride))
        if out:
            R.frames.append(("shown frames", slot, np.stack(shown)))
        return f"{form} of slot {src} onto {which} on core {core}" + (" burst form" if burst else "") + (" +frames" if out else "") + \
            (" staged" if pre else "")

    # -- d ---------------------------------------------------------------------------------------------------------------
    def op_d(self, R, slot, hint):
        spec, apply_host, _, coalesce_reference = _refs()[:4]
        t, rng, S, n, stride = self.tick, self.rng, self.S, self.n, self.stride
        if t is None or t["kind"] != "b" or t["form"] != "cwire":
            return None
        K, src = t["K"], t["slot"]
        off, xs, df, out, pos = coalesce_reference(t["recs"], S, K, n)
        toff = t["off"].astype(np.int64)
        for s in range(S):
            touched = np.unique(t["xs"][toff[s * K]:toff[(s + 1) * K]]).size
            self.stats["cancelled"] += touched - int(off[s + 1] - off[s])
        compact = hint.get("form", "cwire" if int(rng.integers(0, 3)) else "arrays") == "cwire"
        capE, capC = self.B * n, self.capC
        R.checks.append(("coalesced offsets", slot, "off", off, np.uint32))
        if not compact:
            R.calls.append(lambda E: E.core[0].cwire_coalesce_batch(E.p(src, "cw"), t["counts"], t["escapes"], S, K, E.p(slot, "off"),
                                                                    E.p(slot, "xs"), E.p(slot, "df"), capE))
            R.checks += [("coalesced xs", slot, "xs", xs, None), ("coalesced diff", slot, "df", df, None)]
            return f"arrays of slot {src}"
        counts, escapes = spec.headers(out, S)
        self._count(counts, escapes)
        R.calls.append(lambda E: E.core[0].cwire_coalesce_cwire_batch(E.p(src, "cw"), t["counts"], t["escapes"], S, K, E.p(slot, "off"),
                                                                      E.p(slot, "pos"), E.p(slot, "cw"), capC))
        R.checks += [("coalesced frame_pos", slot, "pos", pos, np.uint64), ("coalesced records", slot, "cw", out, None)]
        me = dict(core=0, slot=slot, form="cwire", recs=out)
        pre = self._source(R, me, self.Y)
        for s in range(S):
            apply_host(self.thd[s], out[int(pos[s]):int(pos[s + 1])], 1)
        Y, cw = self.Y, "s_b" if pre else "cw"
        R.calls.append(lambda E: E.core[Y].apply_multi_cwire_batch(E.p(slot, cw), counts, escapes, S, E.st["thd"].ptr, stride))
        return f"compact of slot {src}, applied onto thd on core {Y}" + (" staged" if pre else "")

    # -- e ---------------------------------------------------------------------------------------------------------------
    def op_e(self, R, slot, hint):
        spec, _, _, _, numpy_tick, budget_expected = _refs()
        t, rng, S, n, stride, thr0 = self.tick, self.rng, self.S, self.n, self.stride, self.thr
        if t is None or t["kind"] != "a" or t["form"] != "cwire" or t["budgeted"]:
            return None
        src = t["slot"]
        tk = numpy_tick(t["pre"], t["frames"], thr0)
        assert np.array_equal(tk[0], t["recs"]) and np.array_equal(tk[4], self.snd), "the oracle and numpy disagree on the tick"
        ns = [int(c) for c in t["counts"]]
        budgets = np.array([(NOLIMIT, c // 2, 1, 0)[int(rng.integers(0, 4))] for c in ns], np.uint32)
        self.stats["over_budget"] += sum(int(b) < c for b, c in zip(budgets, ns))
        thrs, off, pos, recs, states, _ = budget_expected(tk, t["pre"], thr0, budgets)
        capC = self.capC
        R.calls.append(lambda E: E.core[0].cwire_budget_cwire_batch(E.p(src, "cw"), t["counts"], t["escapes"], E.st["snd"].ptr, S, budgets,
                                                                    E.p(slot, "thr"), E.p(slot, "off"), E.p(slot, "pos"), E.p(slot, "cw"),
                                                                    capC, stride=stride))
        R.checks += [("thresholds", slot, "thr", thrs, np.uint32), ("budget offsets", slot, "off", off, np.uint32),
                     ("budget frame_pos", slot, "pos", pos, np.uint64), ("budget records", slot, "cw", recs, None)]
        self.snd = states.copy()
        counts, escapes = spec.headers(recs, S)
        self._count(counts, escapes)
        _, xs, df = spec.decode(recs, S)
        self.tick = dict(kind="a", K=1, form="cwire", slot=slot, off=off, xs=xs, df=df, pre=t["pre"], frames=t["frames"], core=0,
                         budgeted=True, recs=recs, pos=pos, counts=counts, escapes=escapes)
        return f"slot {src}, budgets {[int(b) for b in budgets]} of {ns}"

    # -- f, g, j ---------------------------------------------------------------------------------------------------------
    def op_f(self, R, slot, hint):
        spec = _refs()[0]
        rng, K, n, stride = self.rng, self.K, self.n, self.stride
        f0 = int(rng.integers(0, len(self.pool) - K + 1))
        off, xs, df, self.own[0] = po.diff_stream(self.pool[f0:f0 + K], self.own[0], self.thr)
        recs, pos = spec.encode(off, xs, df)
        counts, escapes = spec.headers(recs, K)
        self._count(counts, escapes)
        direct = hint.get("direct", bool(rng.integers(0, 2)))
        capE, capC = self.B * n, self.capC
        fr = lambda E: E.pool.ptr + f0 * stride
        R.checks += [("offsets", slot, "off", off, np.uint32), ("frame_pos", slot, "pos", pos, np.uint64),
                     ("records", slot, "cw", recs, None)]
        if direct:
            R.calls.append(lambda E: E.core[0].diff_stream_cwire_batch(fr(E), K, E.p(slot, "off"), E.p(slot, "pos"), E.p(slot, "cw"), capC,
                                                                       stride=stride))
        else:
            R.calls.append(lambda E: E.core[0].diff_stream_batch(fr(E), K, E.p(slot, "off"), E.p(slot, "xs"), E.p(slot, "df"), capE,
                                                                 stride=stride))
            R.calls.append(lambda E: E.core[0].cwire_encode_batch(E.p(slot, "off"), E.p(slot, "xs"), E.p(slot, "df"), capE, K,
                                                                  E.p(slot, "pos"), E.p(slot, "cw"), capC))
            R.calls.append(lambda E: E.core[0].cwire_decode_batch(E.p(slot, "cw"), counts, escapes, K, E.p(slot, "off2"), E.p(slot, "xs2"),
                                                                  E.p(slot, "df2"), capE))
            R.checks += [("xs", slot, "xs", xs, None), ("diff", slot, "df", df, None), ("decoded offsets", slot, "off2", off, np.uint32),
                         ("decoded xs", slot, "xs2", xs, None), ("decoded diff", slot, "df2", df, None)]
        self.rec1 = dict(slot=slot, core=0, form="cwire", recs=recs, pos=pos, counts=counts, escapes=escapes, off=off, xs=xs,
                         decoded=not direct)
        return "straight into records" if direct else "arrays, encoder, decoder"

    def op_g(self, R, slot, hint):
        apply_host = _refs()[1]
        r, rng, K, stride, Y = self.rec1, self.rng, self.K, self.stride, self.Y
        if r is None:
            return None
        src, out, shown = r["slot"], bool(rng.integers(0, 2)), []
        for t in range(K):
            apply_host(self.own[Y], r["recs"][int(r["pos"][t]):int(r["pos"][t + 1])], 1)
            shown.append(self.own[Y].copy())
        pre = self._source(R, r, Y)
        cw = "s_b" if pre else "cw"
        fo = (lambda E: E.slot[slot]["fo"].ptr) if out else (lambda E: None)
        R.calls.append(lambda E: E.core[Y].apply_cwire_batch(E.p(src, cw), r["counts"], r["escapes"], K, fo(E), stride))
        if out:
            R.frames.append(("client frames", slot, np.stack(shown)))
        return f"slot {src} onto the state of core {Y}" + (" +frames" if out else "") + (" staged" if pre else "")

    def op_h(self, R, slot, hint):
        rng, S, n, stride = self.rng, self.S, self.n, self.stride
        f0 = int(rng.integers(0, len(self.pool) - S + 1))
        swap = bool(rng.integers(0, 2))
        cur, prev = (self.snd, self.pool[f0:f0 + S]) if swap else (self.pool[f0:f0 + S], self.snd)
        offs, xs, df = [0], [], []
        for s in range(S):
            c, x, d, _ = po.diff_pack(cur[s], prev[s], self.thr)
            offs.append(offs[-1] + c); xs.append(x); df.append(d)
        capE = self.B * n
        a = (lambda E: E.st["snd"].ptr, lambda E: E.pool.ptr + f0 * stride)
        pc, pp = a if swap else a[::-1]
        R.calls.append(lambda E: E.core[0].diff_pairs_batch(pc(E), pp(E), S, E.p(slot, "off"), E.p(slot, "xs"), E.p(slot, "df"), capE,
                                                            stride=stride))
        R.checks += [("pair offsets", slot, "off", np.array(offs, np.uint32), np.uint32),
                     ("pair xs", slot, "xs", np.concatenate(xs).astype(np.int32), None),
                     ("pair diff", slot, "df", np.concatenate(df).astype(np.uint8), None)]
        return "the states are the frames" if swap else "the states are the previous frames"

    def op_j(self, R, slot, hint):
        r, K, n, stride = self.rec1, self.K, self.n, self.stride
        if r is None or not r["decoded"]:
            return None
        src, clear = r["slot"], bool(self.rng.integers(0, 2))
        canvas = np.zeros(n, np.uint8) if clear else np.full(n, GUARD, np.uint8)
        off = r["off"].astype(np.int64)
        R.calls.append(lambda E: E.core[0].red_stream_batch(E.p(src, "off2"), E.p(src, "xs2"), K, E.slot[slot]["fo"].ptr, clear, stride))
        R.frames.append(("red maps", slot, np.stack([po.red_overlap(canvas, r["xs"][off[t]:off[t + 1]]) for t in range(K)])))
        return f"slot {src}" + (" cleared" if clear else "")

    # -- k ---------------------------------------------------------------------------------------------------------------
    def rare(self, R):
        rng = self.rng
        for kind in range(4):
            if int(rng.integers(0, 16)):
                continue
            c = int(rng.integers(0, 2)) if not self.one_core else 0
            self.stats["ops"]["k"] += 1
            if kind == 0:
                mask = int(rng.integers(1, 32))
                R.calls.append(lambda E, c=c, mask=mask: E.core[c].prepare(mask))
                R.ops.append(f"k prepare({mask}) on core {c}")
            elif kind == 1:
                left = int(rng.integers(1, 4))
                R.calls.append(lambda E, c=c, left=left: E.core[c].set_option(lib.OPT_SCAN_EPOCH_LEFT, left))
                R.ops.append(f"k OPT_SCAN_EPOCH_LEFT {left} on core {c}")
            elif kind == 2:
                v = int(rng.integers(0, 2))
                self.pipeline[c] = bool(v)
                R.calls.append(lambda E, c=c, v=v: E.core[c].set_option(lib.OPT_PIPELINE, v))
                R.ops.append(f"k OPT_PIPELINE {v} on core {c}")
            else:
                self.on_torch[c] = not self.on_torch[c]
                to = self.on_torch[c]
                R.calls.append(lambda E, c=c, to=to: (E.core[c].use_torch_stream if to else E.core[c].use_own_stream)())
                R.ops.append(f"k core {c} onto {'the caller' if to else 'its own'} stream")

    # -- a round ---------------------------------------------------------------------------------------------------------
    def plan_round(self, forced=None):
        """forced: [(family, hint)] -- exactly these operations, no rare draws; None if a precondition is not met."""
        spec, _, cwire_bytes_max = _refs()[:3]
        self.capC = cwire_bytes_max(self.n, self.B)
        self.capW = 4 * self.B + 5 * self.B * self.n
        R = _Round()
        R.restore = [(c, self.on_torch[c] != (self.mode == "callers"), self.pipeline[c] != (self.mode != "sequential"))
                     for c in range(1 if self.one_core else 2)]
        self.on_torch = [self.mode == "callers"] * 2
        self.pipeline = [self.mode != "sequential"] * 2
        self.tick = self.rec1 = None          # a round consumes only what it made itself
        nops = len(forced) if forced else int(self.rng.integers(3, NSLOTS + 1))
        for slot in range(nops):
            if forced:
                fam, hint = forced[slot]
                what = getattr(self, "op_" + fam)(R, slot, hint)
                if what is None:
                    return None
            else:
                self.rare(R)
                what = None
                while what is None:           # an operation whose precondition is not met is redrawn
                    fam = _WEIGHTED[int(self.rng.integers(0, len(_WEIGHTED)))]
                    what = getattr(self, "op_" + fam)(R, slot, {})
            self.stats["ops"][fam] += 1
            R.ops.append(f"{fam} [slot {slot}] {what}")
        R.states = {k: getattr(self, k).copy() for k in ("snd", "rly", "cli", "thd")}
        R.own = [s.copy() for s in self.own]
        return R


def wire_stats(rounds, seed, **kw):
    """The statistics of the chain run_wire(rounds, seed, ...) runs, from the planner alone (no GPU)."""
    p = WirePlanner(seed, **kw)
    for _ in range(rounds):
        p.plan_round()
    return p.stats


GUARD = 0x5C          # gpu_util.GUARD (asserted in WireEnv)
_SLOT_BUFFERS = ("off", "off2", "pos", "thr", "xs", "xs2", "df", "df2", "cw", "wire", "fo")


class WireEnv:
    """The GPU side: the cores (the product class, so nothing synchronises behind the chain's back), the frame pools, the four
    sets of caller-held states and NSLOTS output slots, every buffer guarded (tests/gpu_util.py)."""

    def __init__(self, p, flags=0):
        import gpu_util
        from gpu_util import Guarded, Region
        assert gpu_util.GUARD == GUARD
        self.plan, n, B, S, stride = p, p.n, p.B, p.S, p.stride
        _, _, cwire_bytes_max = _refs()[:3]
        capE, capC, capW = B * n, cwire_bytes_max(n, B), 4 * B + 5 * B * n
        self.core = [CUDACore(p.w, p.h, max_batch=B, threshold=p.thr, sample_mat_data=p.base, flags=flags)
                     for _ in range(1 if p.one_core else 2)]
        if p.one_core:
            self.core.append(self.core[0])
        for c in self.core[:1 if p.one_core else 2]:
            if p.mode == "sequential":
                c.set_option(lib.OPT_PIPELINE, 0)
            if p.mode == "callers":
                c.use_torch_stream()
        self.pool = Region(len(p.pool), n, stride).put(p.pool)
        self.noise = Region(len(p.noise), n, stride).put(p.noise)
        self.st = {k: Region(S, n, stride).put(getattr(p, k)) for k in ("snd", "rly", "cli", "thd")}
        I32, I64, U8 = torch.int32, torch.int64, torch.uint8
        self.slot = []
        for _ in range(NSLOTS):
            self.slot.append(dict(
                off=Guarded(B + 1, I32), off2=Guarded(B + 1, I32), pos=Guarded(B + 1, I64), thr=Guarded(S, I32),
                xs=Guarded(capE, I32), xs2=Guarded(capE, I32), df=Guarded(capE, U8), df2=Guarded(capE, U8),
                cw=Guarded(capC, U8), wire=Guarded(capW, U8), fo=Region(B, n, stride),
                s_off=Guarded(B + 1, I32), s_xs=Guarded(capE, I32), s_df=Guarded(capE, U8), s_b=Guarded(max(capC, capW), U8)))

    def p(self, slot, name):
        return self.slot[slot][name].ptr

    def close(self):
        for c in self.core[:1 if self.plan.one_core else 2]:
            c.close()

    def run_round(self, R):
        """Uploads, one torch synchronisation, the calls with nothing in between, one synchronisation per core and one of torch;
        then -> the list of mismatches (empty: the round is right)."""
        from gpu_util import to_dev
        for c, stream, pipe in R.restore:                        # the rare draws of the round before
            if stream:
                (self.core[c].use_torch_stream if self.plan.mode == "callers" else self.core[c].use_own_stream)()
            if pipe:
                self.core[c].set_option(lib.OPT_PIPELINE, 0 if self.plan.mode == "sequential" else 1)
        for slot in range(len(self.slot)):                       # every output slot starts a round as guard bytes
            for name in _SLOT_BUFFERS:
                b = self.slot[slot][name]
                b.buf.fill_(GUARD if name == "fo" else b.fill)
        for slot, name, data in R.stages:
            if len(data):
                self.slot[slot][name].t[:len(data)].copy_(to_dev(data))
        torch.cuda.synchronize()
        for call in R.calls:
            call(self)
        for c in self.core[:1 if self.plan.one_core else 2]:
            c.synchronize()
        torch.cuda.synchronize()
        bad = []
        try:
            for what, slot, name, want, view in R.checks:
                got = self.slot[slot][name].get(written=len(want))[:len(want)]
                if not np.array_equal(got.view(view) if view else got, want):
                    bad.append(f"{what} of slot {slot}")
            wrote = {slot: (what, rows) for what, slot, rows in R.frames}
            for slot in range(len(self.slot)):
                got = self.slot[slot]["fo"].get()
                what, rows = wrote.get(slot, ("frames", np.empty((0, self.plan.n), np.uint8)))
                if not np.array_equal(got[:len(rows)], rows):
                    bad.append(f"{what} of slot {slot}")
                if not (got[len(rows):] == GUARD).all():
                    bad.append(f"frames of slot {slot} that no call was to write")
            for k, want in R.states.items():
                if not np.array_equal(self.st[k].get(), want):
                    bad.append(f"the states {k}")
            for c in range(1 if self.plan.one_core else 2):
                if not np.array_equal(self.core[c].get_state(), R.own[c]):
                    bad.append(f"the own state of core {c}")
            if not (np.array_equal(self.pool.get(), self.plan.pool) and np.array_equal(self.noise.get(), self.plan.noise)):
                bad.append("the input frames")
        except AssertionError as e:                              # a guard of gpu_util
            bad.append(f"guard bytes: {e}")
        return bad


def run_wire(rounds, seed, w=160, h=140, S=3, K=4, mode="own", flags=0, verbose=True, one_core=False):
    """`rounds` random rounds of the operations a..k (WirePlanner) on a sender and a relay/client core, or with one_core on a
    single core in every role.  -> False at the first mismatch, after printing the round, the seed and the operations."""
    p = WirePlanner(seed, w, h, S, K, mode, one_core)
    E = WireEnv(p, flags)
    try:
        for rnd in range(rounds):
            R = p.plan_round()
            bad = E.run_round(R)
            if bad:
                print(f"MISMATCH in round {rnd}; seed {seed}, {w}x{h}, S {S}, K {K}, mode {mode}, flags {flags}, one_core {one_core}")
                print("  wrong: " + "; ".join(bad))
                print("  operations:\n    " + "\n    ".join(R.ops))
                return False
            if verbose and rnd % 25 == 0:
                print(f"wire round {rnd} ok ({mode}{', one core' if one_core else ''})", flush=True)
    finally:
        E.close()
    return True


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    ok = (run(rounds, seed) and run(max(rounds // 4, 1), seed + 100, w=640, h=360, T=4)
          and run(max(rounds // 4, 1), seed + 200, flags=lib.FLAG_OWN_QUEUES))   # the core's streams in their own priority class
    for i, mode in enumerate(MODES):
        ok = (ok and run_wire(rounds, seed + 300 + i, mode=mode) and run_wire(max(rounds // 4, 1), seed + 310 + i, mode=mode, one_core=True)
              and run_wire(max(rounds // 4, 1), seed + 320 + i, w=37, h=11, mode=mode))
    ok = ok and run_wire(max(rounds // 4, 1), seed + 400, flags=lib.FLAG_OWN_QUEUES)
    print("chain soak ok" if ok else "chain soak FAILED")
    sys.exit(0 if ok else 1)

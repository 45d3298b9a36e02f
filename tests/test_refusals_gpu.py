"""-m gpu: which calls the entry points that take compact records or camera states refuse, pinned call by call through the
C-ABI (include/mi355diff.h): overlapping regions, batch sizes around max_batch, bad headers, misaligned records, and which of
two mistakes is reported.

Every call lays its input and outputs in ONE device buffer (Arena), a slot of 128 KiB each, and then one region at a time is
moved against another one (positions()):
    home            disjoint                                                        accepted
    before / after  ending exactly where the other begins, on either side            accepted
    before+1 / after-1   one byte into it from either side                           refused
    before+a / after-a   one alignment unit into it, where the moved pointer must be aligned (a > 1): there a pointer one byte
                    further is refused for its alignment before any overlap test     refused, and the text says "overlap"
    nested          containing it, or contained in it when it is the smaller one     refused
    empty           zero bytes and strictly inside it                                per call: Call.empty
What is expected at every position but the last comes from interval arithmetic done here (refused()), over the pairs of regions
the header says the call tests and the alignments it asks for.  The last one is the one case in which the library's calls differ,
read from csrc/core.hip: a call that compares addresses as they are refuses an empty region that lies inside another one, the
resynchronisation calls say that an empty region overlaps nothing.  With frames of more than zero bytes an empty region is an
output of capacity 0 (the arrays, the records).
Accepted calls run on valid inputs of two streams and two frames and are synchronised; what they compute is the business of
the other tests.  The cores: 40x30 (3600 bytes, one 4 KiB tile) and 64x48 (9216 bytes, three tiles, the last one short) with
max_batch = 8, which also takes the cases at max_batch and one above."""
import functools

import numpy as np
import pytest
import torch

import cwire_spec as spec
from cudavideostream_amd import lib
from gpu_util import DEV, CUDACore

pytestmark = pytest.mark.gpu

SLOT, HOME, SLOTS = 1 << 17, 1 << 15, 12
GEOMS = [(40, 30), (64, 48)]
MAX_BATCH = 8
CAP = 1024                    # entries of an arrays output
CAP_BYTES = 4096              # bytes of a records output
CELL = 8
TILE = 4096
NOLIMIT = 0xFFFFFFFF
REFUSED, ACCEPTED = True, False


class Arena:
    """One device allocation of SLOTS slots; region i of a call is at home(i), HOME bytes into slot i + 1."""

    def __init__(self):
        self.buf = torch.zeros(SLOTS * SLOT, dtype=torch.uint8, device=DEV)
        self.base = self.buf.data_ptr()
        assert self.base % 256 == 0

    def home(self, i):
        assert i + 2 < SLOTS
        return self.base + (i + 1) * SLOT + HOME

    def write(self, at, data):
        lo = at - self.base
        assert 0 <= lo and lo + data.size <= self.buf.numel()
        self.buf[lo:lo + data.size].copy_(torch.from_numpy(data))

    def holds(self, at, nbytes):
        return self.base <= at and at + nbytes <= self.base + self.buf.numel()


@pytest.fixture(scope="module")
def arena():
    return Arena()


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def core(request):
    w, h = request.param
    with CUDACore(w, h, max_batch=MAX_BATCH) as c:
        yield c


class Reg:
    """A region of a call: its bytes as the library counts them, the alignment its pointer is placed with, whether the library
    refuses a pointer without it, and the bytes an accepted call finds there."""

    def __init__(self, nbytes, align=1, asked=False, data=None):
        self.nbytes, self.align, self.asked, self.data = int(nbytes), align, asked, data
        assert data is None or data.size <= self.nbytes
        assert self.nbytes <= SLOT - HOME


class Call:
    def __init__(self, name, regs, pairs, fn, empty=None):
        self.name = name        # the entry point
        self.regs = regs        # {region: Reg}, in slot order
        self.pairs = pairs      # the pairs of regions the call tests against each other
        self.fn = fn            # fn(L, handle, p, nb) -> return code; p: {region: address}, nb: {region: bytes}
        self.empty = empty or {}   # {(moved, other): (the regions that capacity 0 empties, REFUSED | ACCEPTED)}

    def homes(self, arena):
        return {r: arena.home(i) for i, r in enumerate(self.regs)}

    def sizes(self):
        return {r: reg.nbytes for r, reg in self.regs.items()}


def refused(call, p, nb):
    """Interval arithmetic: a pointer without the alignment asked of it, or two regions of a tested pair that share a byte."""
    if any(reg.asked and p[r] % reg.align for r, reg in call.regs.items()):
        return True
    return any(nb[a] > 0 and nb[b] > 0 and p[a] < p[b] + nb[b] and p[b] < p[a] + nb[a] for a, b in call.pairs)


def last_error(L):
    return L.mi355_last_error().decode(errors="replace")


def run(L, core, arena, call, p, nb, want, word=None, where=""):
    """One call at the addresses p; want: REFUSED (word: a word its text must hold) or ACCEPTED (runs, and is synchronised)."""
    for r in call.regs:
        assert arena.holds(p[r], nb[r]), (call.name, where, r)
    if want == ACCEPTED:
        for r, reg in call.regs.items():
            if reg.data is not None and nb[r]:
                arena.write(p[r], reg.data)
        torch.cuda.synchronize()
    rc = call.fn(L, core._h, p, nb)
    if want == REFUSED:
        assert rc == lib.ERR_INVALID, (call.name, where, rc)
        assert last_error(L), (call.name, where)
        if word:
            assert word in last_error(L), (call.name, where, last_error(L))
    else:
        assert rc == lib.OK, (call.name, where, last_error(L))
        assert L.mi355_synchronize(core._h) == lib.OK, (call.name, where, last_error(L))


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch(n, B):
    """B records of 8 entries for frames of n bytes: (compact bytes, counts, escapes, wire bytes, wire counts); the host arrays
    have an element even for B = 0."""
    rng = np.random.default_rng(1000 * n + B)
    recs = []
    for _ in range(B):                       # two gaps of 300 (escapes) in every record: 32 bytes each, indices below 800
        gaps = rng.integers(0, 20, 8)
        gaps[[3, 6]] = 300
        recs.append((np.cumsum(gaps + 1) - 1, rng.integers(1, 256, 8).astype(np.uint8)))
    cw = np.frombuffer(b"".join(spec.encode_frame(x, d) for x, d in recs), np.uint8).copy()
    counts, escapes = spec.headers(cw, B)
    wire = np.frombuffer(b"".join(np.array([8], "<u4").tobytes() + x.astype("<i4").tobytes() + d.tobytes() for x, d in recs),
                         np.uint8).copy()
    pad = (lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros(1, np.uint32)]).astype(np.uint32)))
    assert cw.size == 32 * B and wire.size == 44 * B and n >= 800
    return cw, pad(counts), pad(escapes), wire, pad(np.full(B, 8, np.uint32))


class Geom:
    def __init__(self, core, S, K):
        self.w, self.h, self.n = core.width, core.height, core.total
        self.S, self.K, self.B = S, K, S * K
        self.stride, self.ostride = self.n + 40, self.n + 24
        self.tiles = (self.n + TILE - 1) // TILE
        self.mask_words = (self.tiles + 31) // 32

    def span(self, count, stride):
        return (count - 1) * stride + self.n if count > 0 else 0

    def rows(self, count, changed):
        """count frames `stride` apart: one base frame each, five bytes of it changed by 100 where `changed`."""
        rng = np.random.default_rng(self.n)
        base = rng.integers(0, 256, self.n, dtype=np.uint8)
        out = np.zeros(self.span(count, self.stride), np.uint8)
        for b in range(count):
            row = base.copy()
            if changed:
                row[np.arange(5) * 701 % self.n + b] += 100
            out[b * self.stride:b * self.stride + self.n] = row
        return out

    def states(self):
        return Reg(self.span(self.S, self.stride), data=self.rows(self.S, False))

    def out_frames(self):
        return Reg(self.span(self.B, self.ostride))

    def cwire(self):
        cw = batch(self.n, self.B)[0]
        return Reg(cw.size, 4, True, cw)

    def wire(self):
        wr = batch(self.n, self.B)[3]
        return Reg(wr.size, 4, False, wr)

    def heads(self):
        """(offsets, frame_pos) of S records or segments"""
        return Reg(4 * (self.S + 1), 4, True), Reg(8 * (self.S + 1), 8, True)

    def mask(self, asked=True):
        return Reg(4 * self.S * self.mask_words, 4, asked, np.zeros(4 * self.S * self.mask_words, np.uint8))


def both(pairs):
    """Every pair, and every pair the other way round: each of its two regions is moved against the other."""
    return pairs + [(b, a) for a, b in pairs]


def hp(a):
    return a.ctypes.data


# ---- the calls ------------------------------------------------------------------------------------------------------------
def diff_multi(g, form, stream):
    """mi355_diff_multi(_stream)_{,wire_,cwire_}batch: the states against the frames; the outputs are not compared"""
    nfr = g.B if stream else g.S          # frames, and entries of offsets - 1
    name = f"mi355_diff_multi{'_stream' if stream else ''}{form}batch"
    regs = {"frames": Reg(g.span(nfr, g.stride), data=g.rows(nfr, True)), "states": g.states(), "offsets": Reg(4 * (nfr + 1), 4)}
    if form == "_":
        regs.update(xs=Reg(4 * CAP, 4), diff=Reg(CAP))
    elif form == "_wire_":
        regs.update(wire=Reg(4 * nfr + 5 * CAP, 4))
    else:
        regs.update(frame_pos=Reg(8 * (nfr + 1), 8, True), cwire=Reg(CAP_BYTES, 4, True))
        regs["offsets"].asked = True
    counts = (g.S, g.K) if stream else (g.S,)

    def fn(L, h, p, nb):
        head = (h, p["frames"], p["states"], g.stride) + counts + (p["offsets"],)
        if form == "_":
            return getattr(L, name)(*head, p["xs"], p["diff"], CAP)
        if form == "_wire_":
            return getattr(L, name)(*head, p["wire"], nb["wire"])
        return getattr(L, name)(*head, p["frame_pos"], p["cwire"], nb["cwire"])

    return Call(name, regs, both([("frames", "states")]), fn)


def apply_multi(g, form):
    """mi355_apply_multi_{wire,cwire}_batch: the input against the states"""
    cw, counts, escapes, _, wcounts = batch(g.n, g.S)
    regs = {"in": g.cwire() if form == "cwire" else g.wire(), "states": g.states()}

    def fn(L, h, p, nb):
        if form == "cwire":
            return L.mi355_apply_multi_cwire_batch(h, p["in"], hp(counts), hp(escapes), g.S, p["states"], g.stride)
        return L.mi355_apply_multi_wire_batch(h, p["in"], hp(wcounts), g.S, p["states"], g.stride)

    return Call(f"mi355_apply_multi_{form}_batch", regs, both([("in", "states")]), fn)


def apply_multi_stream(g, form):
    """mi355_apply_multi_stream_{wire,cwire}_batch: the states against the output frames, the input against both"""
    cw, counts, escapes, _, wcounts = batch(g.n, g.B)
    regs = {"in": g.cwire() if form == "cwire" else g.wire(), "states": g.states(), "out": g.out_frames()}

    def fn(L, h, p, nb):
        tail = (g.S, g.K, p["states"], g.stride, p["out"], g.ostride)
        if form == "cwire":
            return L.mi355_apply_multi_stream_cwire_batch(h, p["in"], hp(counts), hp(escapes), *tail)
        return L.mi355_apply_multi_stream_wire_batch(h, p["in"], hp(wcounts), *tail)

    return Call(f"mi355_apply_multi_stream_{form}_batch", regs, both([("states", "out"), ("in", "states"), ("in", "out")]), fn)


def apply_cwire(g):
    """mi355_apply_cwire_batch: K records onto the core's own state; no two regions are compared, K may pass max_batch"""
    cw, counts, escapes, _, _ = batch(g.n, g.B)
    regs = {"in": g.cwire(), "out": g.out_frames()}

    def fn(L, h, p, nb):
        return L.mi355_apply_cwire_batch(h, p["in"], hp(counts), hp(escapes), g.B, p["out"], g.ostride)

    return Call("mi355_apply_cwire_batch", regs, [], fn)


def coalesce(g, cwire):
    cw, counts, escapes, _, _ = batch(g.n, g.B)
    offsets, frame_pos = g.heads()
    if cwire:
        regs = {"in": g.cwire(), "offsets": offsets, "frame_pos": frame_pos, "cwire_out": Reg(CAP_BYTES, 4, True)}
        empty = {("cwire_out", "in"): (("cwire_out",), REFUSED)}
    else:
        regs = {"in": g.cwire(), "offsets": offsets, "xs": Reg(4 * CAP, 4, True), "diff": Reg(CAP)}
        empty = {("xs", "in"): (("xs", "diff"), REFUSED), ("diff", "in"): (("xs", "diff"), REFUSED)}

    def fn(L, h, p, nb):
        head = (h, p["in"], hp(counts), hp(escapes), g.S, g.K, p["offsets"])
        if cwire:
            return L.mi355_cwire_coalesce_cwire_batch(*head, p["frame_pos"], p["cwire_out"], nb["cwire_out"])
        return L.mi355_cwire_coalesce_batch(*head, p["xs"], p["diff"], nb["diff"])

    return Call(f"mi355_cwire_coalesce_{'cwire_' if cwire else ''}batch", regs, [(r, "in") for r in list(regs)[1:]], fn, empty)


def budget(g):
    cw, counts, escapes, _, _ = batch(g.n, g.S)
    offsets, frame_pos = g.heads()
    budgets = np.full(g.S + 1, NOLIMIT, np.uint32)
    regs = {"in": g.cwire(), "states": g.states(), "offsets": offsets, "thresholds": Reg(4 * g.S, 4, True), "frame_pos": frame_pos,
            "cwire_out": Reg(CAP_BYTES, 4, True)}
    outs = list(regs)[2:]

    def fn(L, h, p, nb):
        return L.mi355_cwire_budget_cwire_batch(h, p["in"], hp(counts), hp(escapes), p["states"], g.stride, g.S, hp(budgets),
                                                p["thresholds"], p["offsets"], p["frame_pos"], p["cwire_out"], nb["cwire_out"])

    pairs = both([("states", "in")]) + [(o, i) for o in outs for i in ("in", "states")] + [("states", "offsets"), ("in", "cwire_out")]
    empty = {("cwire_out", "in"): (("cwire_out",), REFUSED), ("cwire_out", "states"): (("cwire_out",), REFUSED)}
    return Call("mi355_cwire_budget_cwire_batch", regs, pairs, fn, empty)


def activity(g, L):
    cw, counts, escapes, _, _ = batch(g.n, g.B)
    cells = L.mi355_activity_cells(g.w, g.h, CELL, CELL, None, None)
    regs = {"in": g.cwire(), "cells": Reg(4 * g.S * cells, 4, True), "summary": Reg(32 * g.S, 4, True)}

    def fn(L, h, p, nb):
        return L.mi355_cwire_activity_batch(h, p["in"], hp(counts), hp(escapes), g.S, g.K, CELL, CELL, 1, 0, p["cells"], p["summary"])

    return Call("mi355_cwire_activity_batch", regs, [("cells", "in"), ("summary", "in"), ("in", "cells")], fn)


def check(g):
    cw, counts, escapes, _, _ = batch(g.n, g.B)
    regs = {"in": g.cwire(), "verdicts": Reg(16 * g.B, 4, True)}

    def fn(L, h, p, nb):
        return L.mi355_cwire_check_batch(h, p["in"], hp(counts), hp(escapes), g.B, p["verdicts"])

    return Call("mi355_cwire_check_batch", regs, both([("verdicts", "in")]), fn)


def touched(g):
    cw, counts, escapes, _, _ = batch(g.n, g.B)
    regs = {"in": g.cwire(), "mask": g.mask()}

    def fn(L, h, p, nb):
        return L.mi355_cwire_touched_tiles_batch(h, p["in"], hp(counts), hp(escapes), g.S, g.K, 0, p["mask"])

    return Call("mi355_cwire_touched_tiles_batch", regs, both([("mask", "in")]), fn)


def digest(g):
    regs = {"states": g.states(), "digests": Reg(8 * g.S * g.tiles, 4, True)}

    def fn(L, h, p, nb):
        return L.mi355_state_digest_batch(h, p["states"], g.stride, g.S, p["digests"])

    return Call("mi355_state_digest_batch", regs, both([("digests", "states")]), fn)


def refresh(g):
    offsets, frame_pos = g.heads()
    regs = {"states": g.states(), "peer": Reg(8 * g.S * g.tiles, 4, True, np.zeros(8 * g.S * g.tiles, np.uint8)), "mask": g.mask(),
            "offsets": offsets, "frame_pos": frame_pos, "cwire_out": Reg(CAP_BYTES, 4, True)}
    outs = list(regs)[2:]

    def fn(L, h, p, nb):
        return L.mi355_refresh_cwire_batch(h, p["states"], g.stride, g.S, p["peer"], p["mask"], p["offsets"], p["frame_pos"],
                                           p["cwire_out"], nb["cwire_out"])

    pairs = [(o, i) for o in outs for i in ("states", "peer")] + [(a, b) for k, a in enumerate(outs) for b in outs[k + 1:]]
    pairs += [("states", "mask"), ("peer", "cwire_out")]
    empty = {("cwire_out", other): (("cwire_out",), ACCEPTED) for other in ("states", "peer", "frame_pos")}
    return Call("mi355_refresh_cwire_batch", regs, pairs, fn, empty)


def clear_tiles(g):
    regs = {"states": g.states(), "mask": g.mask()}

    def fn(L, h, p, nb):
        return L.mi355_state_clear_tiles_batch(h, p["states"], g.stride, g.S, p["mask"])

    return Call("mi355_state_clear_tiles_batch", regs, both([("mask", "states")]), fn)


def wall(g):
    """Thumbnails of a quarter of the size, side by side in a wall of 160 x 32 pixels"""
    W, H, pitch = 160, 32, 3 * 160 + 8
    place = np.zeros((g.S + 1, 3), np.int32)
    for s in range(g.S):
        place[s] = ((g.w + 3) // 4 * s, 0, 4)
    assert g.S > MAX_BATCH or g.S * ((g.w + 3) // 4) <= W
    regs = {"states": g.states(), "mask": g.mask(), "wall": Reg((H - 1) * pitch + 3 * W)}

    def fn(L, h, p, nb):
        return L.mi355_wall_compose_batch(h, p["states"], g.stride, g.S, hp(place), p["mask"], p["wall"], W, H, pitch)

    return Call("mi355_wall_compose_batch", regs, both([("wall", "states"), ("mask", "states"), ("wall", "mask")]), fn)


def calls(core, L, S=2, K=2):
    """Every entry point of this file at S streams of K records (one record each for the calls without nframes)"""
    g, g1 = Geom(core, S, K), Geom(core, S, 1)
    out = [diff_multi(g1, form, False) for form in ("_", "_wire_", "_cwire_")]
    out += [diff_multi(g, form, True) for form in ("_", "_wire_", "_cwire_")]
    out += [apply_multi(g1, "wire"), apply_multi(g1, "cwire"), apply_multi_stream(g, "wire"), apply_multi_stream(g, "cwire")]
    out += [apply_cwire(Geom(core, 1, S * K)), coalesce(g, False), coalesce(g, True), budget(g1), activity(g, L), check(Geom(core, S * K, 1)),
            touched(g), digest(g1), refresh(g1), clear_tiles(g1), wall(g1)]
    return out


CWIRE_INPUT = ("mi355_apply_cwire_batch", "mi355_apply_multi_cwire_batch", "mi355_apply_multi_stream_cwire_batch",
               "mi355_cwire_coalesce_batch", "mi355_cwire_coalesce_cwire_batch", "mi355_cwire_budget_cwire_batch",
               "mi355_cwire_activity_batch", "mi355_cwire_check_batch", "mi355_cwire_touched_tiles_batch")
TWO_COUNTS = ("mi355_diff_multi_stream_batch", "mi355_diff_multi_stream_wire_batch", "mi355_diff_multi_stream_cwire_batch",
              "mi355_apply_multi_stream_wire_batch", "mi355_apply_multi_stream_cwire_batch", "mi355_cwire_coalesce_batch",
              "mi355_cwire_coalesce_cwire_batch", "mi355_cwire_activity_batch", "mi355_cwire_touched_tiles_batch")


@pytest.fixture(scope="module")
def L():
    return lib.load()


def test_the_table_names_every_call(core, L):
    names = [c.name for c in calls(core, L)]
    assert len(names) == len(set(names)) == 21 and set(CWIRE_INPUT) <= set(names) and set(TWO_COUNTS) <= set(names)
    assert all(hasattr(L, n) for n in names)
    g = Geom(core, 2, 2)
    assert (g.n, g.tiles) in ((3600, 1), (9216, 3)) and g.n % TILE


# ---- 1. one region moved against another ----------------------------------------------------------------------------------
def positions(a, b, at_b):
    """[(name, address of the moved region a)] against the region b at at_b"""
    step = a.align
    before, after = at_b - a.nbytes, at_b + b.nbytes
    assert before % step == 0 and after % step == 0
    out = [("before", before), ("after", after), ("before+1", before + 1), ("after-1", after - 1)]
    if step > 1:
        out += [("before+a", before + step), ("after-a", after - step)]
    if a.nbytes >= b.nbytes + 2 * step:
        out.append(("nested", at_b - step))
    elif b.nbytes >= a.nbytes + 2 * step:
        out.append(("nested", at_b + step))
    else:
        out.append(("nested", at_b))
    return out


def test_one_region_moved_against_another(core, L, arena):
    seen = set()
    for call in calls(core, L):
        home, nb = call.homes(arena), call.sizes()
        assert not refused(call, home, nb)
        run(L, core, arena, call, home, nb, ACCEPTED, where="home")
        for a, b in call.pairs:
            for where, at in positions(call.regs[a], call.regs[b], home[b]):
                p = dict(home, **{a: at})
                want = refused(call, p, nb)
                assert want == (where not in ("before", "after")), (call.name, a, b, where)
                aligned = at % call.regs[a].align == 0
                run(L, core, arena, call, p, nb, want, "overlap" if want and aligned else None, f"{a} {where} {b}")
                seen.add(where)
    assert seen == {"before", "after", "before+1", "after-1", "before+a", "after-a", "nested"}


def test_an_empty_region_inside_another(core, L, arena):
    """Capacity 0, and the output it empties strictly inside another region: Call.empty, as csrc/core.hip answers it."""
    answers = {}
    for call in calls(core, L):
        home = call.homes(arena)
        for (a, b), (emptied, want) in call.empty.items():
            nb = dict(call.sizes(), **{r: 0 for r in emptied})
            p = dict(home, **{a: home[b] + call.regs[a].align})
            assert home[b] < p[a] < home[b] + nb[b] and not refused(call, p, nb)       # interval arithmetic: nothing is shared
            run(L, core, arena, call, p, nb, want, "overlap" if want == REFUSED else None, f"empty {a} inside {b}")
            run(L, core, arena, call, home, nb, ACCEPTED, where=f"empty {a} at home")     # capacity 0 alone is no mistake
            answers.setdefault(call.name, set()).add(want)
    assert answers == {"mi355_cwire_coalesce_batch": {REFUSED}, "mi355_cwire_coalesce_cwire_batch": {REFUSED},
                       "mi355_cwire_budget_cwire_batch": {REFUSED}, "mi355_refresh_cwire_batch": {ACCEPTED}}


# ---- 2. batch sizes around max_batch --------------------------------------------------------------------------------------
COUNTS = [((0, 1), ACCEPTED), ((0, 2), ACCEPTED), ((2, 0), ACCEPTED), ((8, 1), ACCEPTED), ((2, 4), ACCEPTED), ((4, 2), ACCEPTED),
          ((9, 1), REFUSED), ((3, 3), REFUSED)]


def test_batch_sizes_around_max_batch(L, arena):
    """nstreams, and nstreams * nframes, at 0, at max_batch and one above; a call with one count takes the (S, 1) cases.
    mi355_apply_cwire_batch alone takes more records than max_batch, in slices."""
    ran = 0
    with CUDACore(64, 48, max_batch=MAX_BATCH) as core:
        for (S, K), want in COUNTS:
            for call in calls(core, L, S, K):
                if K != 1 and call.name not in TWO_COUNTS:
                    continue
                sliced = call.name == "mi355_apply_cwire_batch"
                run(L, core, arena, call, call.homes(arena), call.sizes(), ACCEPTED if sliced else want, where=f"S = {S}, K = {K}")
                ran += 1
    assert ran == 21 * 3 + 9 * 5


# ---- 3. headers, alignment ------------------------------------------------------------------------------------------------
def test_bad_headers_and_misaligned_records(core, L, arena):
    done = set()
    for call in calls(core, L):
        if call.name not in CWIRE_INPUT:
            continue
        home, nb = call.homes(arena), call.sizes()
        n = core.total
        B = {"mi355_apply_multi_cwire_batch": 2, "mi355_cwire_budget_cwire_batch": 2}.get(call.name, 4)
        cw, counts, escapes, _, _ = batch(n, B)
        keep = counts.copy(), escapes.copy()
        try:
            escapes[B - 1] = counts[B - 1] + 1                       # e > n
            run(L, core, arena, call, home, nb, REFUSED, "header", "e > n")
            escapes[:] = keep[1]
            counts[B - 1] = n + 1                                    # n > frame bytes
            run(L, core, arena, call, home, nb, REFUSED, "header", "n > frame bytes")
        finally:
            counts[:], escapes[:] = keep
        for skew in (1, 2, 3):
            run(L, core, arena, call, dict(home, **{"in": home["in"] + skew}), nb, REFUSED, "align", f"d_cwire + {skew}")
        run(L, core, arena, call, home, nb, ACCEPTED, where="the headers restored")
        done.add(call.name)
    assert done == set(CWIRE_INPUT)


# ---- 4. wrong in two ways -------------------------------------------------------------------------------------------------
def test_which_of_two_mistakes_is_reported(core, L, arena):
    n = core.total
    over = {c.name: c for c in calls(core, L, 3, 3)}                  # 9 records, or 3 streams
    for call in calls(core, L):
        if not call.pairs:
            continue
        a, b = call.pairs[0]
        home, nb = call.homes(arena), call.sizes()
        p = dict(home, **{a: positions(call.regs[a], call.regs[b], home[b])[-1][1]})
        assert refused(call, p, nb)

        # no core, and an overlap: the core is looked at first
        rc = call.fn(L, None, p, nb)
        assert rc == lib.ERR_INVALID and "core" in last_error(L) and "overlap" not in last_error(L), (call.name, last_error(L))

        # too many records, and an overlap: the count is looked at first
        if call.name in TWO_COUNTS or call.name == "mi355_cwire_check_batch":
            big = over[call.name]
            rc = big.fn(L, core._h, p, big.sizes())
            assert rc == lib.ERR_INVALID and "overlap" not in last_error(L), (call.name, last_error(L))
            if call.name in TWO_COUNTS:
                assert "nframes" in last_error(L), (call.name, last_error(L))

        # a bad header, and an overlap: the headers are looked at first
        if call.name in CWIRE_INPUT:
            B = {"mi355_apply_multi_cwire_batch": 2, "mi355_cwire_budget_cwire_batch": 2}.get(call.name, 4)
            _, counts, escapes, _, _ = batch(n, B)
            keep = escapes.copy()
            a2, b2 = next(pair for pair in call.pairs if "in" in pair)     # the record's length comes from its headers
            p2 = dict(home, **{a2: positions(call.regs[a2], call.regs[b2], home[b2])[-1][1]})
            try:
                escapes[0] = counts[0] + 1
                run(L, core, arena, call, p2, nb, REFUSED, "header", "a bad header and an overlap with the input")
                assert "overlap" not in last_error(L)
                if (a, b) == ("states", "out"):                           # regions of the arguments alone come before the headers
                    run(L, core, arena, call, p, nb, REFUSED, "overlap", "a bad header and the states in the output frames")
            finally:
                escapes[:] = keep

        # a misaligned pointer, and an overlap: a call that asks for alignment says so first
        if call.regs[a].asked and call.regs[a].align > 1:
            run(L, core, arena, call, dict(p, **{a: p[a] + 1}), nb, REFUSED, "align", "misaligned and overlapping")
            assert "overlap" not in last_error(L)

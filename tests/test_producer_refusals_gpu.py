"""-m gpu: the order in which mi355_cwire_coalesce_(cwire_)batch, mi355_cwire_crop_(cwire_)batch and mi355_cwire_mosaic_(cwire_)batch
refuse, rung by rung through the C-ABI (include/mi355diff.h).  The six forms share one ladder (csrc/core.hip):

     1  null core
     2  nstreams or nframes < 0
     3  nstreams * nframes above max_batch
     4  crop: an unknown flag bit.  mosaic: canvas_w or canvas_h < 1, a canvas of 2^31 bytes or more, a canvas of too many tiles
     5  a pointer that must be 4-byte aligned is not
     6  d_frame_pos is not 8-byte aligned
     7  an empty batch: OK, offsets[0] = 0 and (compact form) frame_pos[0] = 0 written, nothing else, null inputs allowed
     8  null stream pointer
     9  crop: null h_rects.  mosaic: null h_place
    10  null output pointer
    11  crop: a rectangle with a negative member, outside the frame.  mosaic: a placement with a negative member, its source
        outside the frame, its destination outside the canvas -- stream by stream
    12  the frame headers: more escapes than entries, more entries than frame bytes
    13  an output that overlaps the input: d_offsets, d_frame_pos, d_cwire_out, d_xs, d_diff, in this order
    14  the launch

A case breaks rung k and, greedily in ladder order, every later rung whose arguments rung k (and the rungs taken before it) left
free, and asks for rung k's text exactly; nothing is enqueued by a refused call.  Rung 14 is one valid call of 2 streams x 2
records per form, compared with the numpy statement of the call (crop_spec, mosaic_spec).  One 64x48 core (9216 bytes, three
tiles) with max_batch = 4."""
import numpy as np
import pytest
import torch

import crop_spec
import cwire_spec as spec
import mosaic_spec
from cudavideostream_amd import lib
from gpu_util import DEV, CUDACore

pytestmark = pytest.mark.gpu

W, H, N, MAX_BATCH = 64, 48, 3 * 64 * 48, 4
S, K = 2, 2
CANVAS_W, CANVAS_H = 96, 64              # 18432 bytes: 5 tiles of the 12 that max_batch frames hold
SLOT = 4096
IN, OFFSETS, FRAME_POS, OUT, DIFF, SLOTS = 0, 1, 2, 3, 4, 6
CAP, CAP_BYTES = 256, 1024               # entries of d_xs / d_diff, bytes of d_cwire_out
FILL = 0xA5
FORMS = [(kind, cwire) for kind in ("coalesce", "crop", "mosaic") for cwire in (False, True)]
RECTS = np.array([[0, 0, W, H], [16, 8, 32, 24], [0, 0, 1, 1], [0, 0, 1, 1]], np.int32)
PLACE = np.array([[0, 0, 32, 24, 0, 0], [8, 8, 32, 24, 40, 20], [0, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0]], np.int32)


def form_id(form):
    return f"{form[0]}{'_cwire' if form[1] else ''}"


def records():
    """2 streams x 2 records: escapes (gaps of 293 and more), an index both records of a stream hold, a sum that wraps to 0;
    every stream has entries inside its rectangle of RECTS and of PLACE and entries outside it."""
    recs = [([5, 6, 300, 4100], [1, 2, 3, 4]), ([6, 700, N - 1], [250, 9, 7]),
            ([0, 1970, 8200], [200, 200, 5]), ([1970, 1971, 3940], [56, 77, 1])]
    buf = np.frombuffer(b"".join(spec.encode_frame(np.array(x), np.array(d, np.uint8)) for x, d in recs), np.uint8).copy()
    counts, escapes = spec.headers(buf, S * K)
    assert escapes[0] == 2 and buf.size <= SLOT
    return buf, counts, escapes


RECS, COUNTS, ESCAPES = records()


@pytest.fixture(scope="module")
def L():
    return lib.load()


@pytest.fixture(scope="module")
def core():
    with CUDACore(W, H, max_batch=MAX_BATCH) as c:
        yield c


@pytest.fixture(scope="module")
def arena():
    buf = torch.empty(SLOTS * SLOT, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    return buf


def valid(form, core, arena):
    """The arguments of a valid call; the host arrays have spare elements behind the S * K (S) the call reads."""
    kind, cwire = form
    at = (lambda slot: arena.data_ptr() + slot * SLOT)
    pad = (lambda a: np.concatenate([a, np.zeros(4, np.uint32)]).astype(np.uint32))
    return {"core": core._h, "d_in": at(IN), "counts": pad(COUNTS), "escapes": pad(ESCAPES), "S": S, "K": K,
            "table": {"coalesce": None, "crop": RECTS.copy(), "mosaic": PLACE.copy()}[kind], "flags": 0, "canvas": (CANVAS_W, CANVAS_H),
            "offsets": at(OFFSETS), "frame_pos": at(FRAME_POS) if cwire else None, "out": at(OUT), "diff": None if cwire else at(DIFF),
            "cap": CAP_BYTES if cwire else CAP}


def call(L, form, a):
    kind, cwire = form
    hp = (lambda x: None if x is None else x.ctypes.data)
    head = (a["core"], a["d_in"], hp(a["counts"]), hp(a["escapes"]), a["S"], a["K"])
    mid = {"coalesce": (), "crop": (hp(a["table"]), a["flags"]), "mosaic": (hp(a["table"]),) + tuple(a["canvas"])}[kind]
    tail = (a["offsets"], a["frame_pos"], a["out"], a["cap"]) if cwire else (a["offsets"], a["out"], a["diff"], a["cap"])
    return getattr(L, f"mi355_cwire_{kind}_{'cwire_' if cwire else ''}batch")(*head, *mid, *tail)


def last_error(L):
    return L.mi355_last_error().decode(errors="replace")


# ---- the ladder ---------------------------------------------------------------------------------------------------------
def put(**kv):
    return lambda a, base: a.update(kv)


def row0(*members):
    def f(a, base):
        a["table"][0, :len(members)] = members
    return f


def head0(key, value):
    def f(a, base):
        a[key][0] = value
    return f


def at_input(key, off):
    def f(a, base):
        a[key] = base + off
    return f


ALIGN4 = "d_cwire, d_cwire_out, d_offsets and d_xs must be 4-byte aligned"
FAR = 1 << 30   # a destination no canvas of the ladder reaches


def ladder(form):
    """[(name, the arguments it sets, how, the text)] in the order of the refusals; base: the aligned address of the input."""
    kind, cwire = form
    out = [("core", {"core"}, put(core=None), "null core"),
           ("negative", {"S", "K"}, put(S=-1, K=-5), "nstreams or nframes < 0"),          # (-1 * -5 is above max_batch, too)
           ("count", {"S", "K"}, put(S=3, K=2), "nstreams * nframes above max_batch")]
    if kind == "crop":
        out += [("flag", {"flags"}, put(flags=2), "unknown flag bit (MI355_CROP_KEEP_INDEX is the only one)")]
    if kind == "mosaic":
        out += [("canvas_0", {"canvas"}, put(canvas=(0, CANVAS_H)), "canvas_w or canvas_h < 1"),
                ("canvas_2^31", {"canvas"}, put(canvas=(32768, 32768)), "canvas of 2^31 bytes or more"),
                ("canvas_tiles", {"canvas"}, put(canvas=(128, 129)),   # 49536 bytes: 13 tiles, max_batch frames hold 12
                 "canvas of more 4096-byte tiles than max_batch frames hold: create the core with a larger max_batch")]
    out += [("align_in", {"d_in"}, at_input("d_in", 1), ALIGN4),
            ("align_offsets", {"offsets"}, at_input("offsets", OFFSETS * SLOT + 2), ALIGN4),
            ("align_out", {"out"}, at_input("out", OUT * SLOT + 1), ALIGN4)]
    if cwire:
        out += [("align_frame_pos", {"frame_pos"}, at_input("frame_pos", FRAME_POS * SLOT + 4), "d_frame_pos must be 8-byte aligned")]
    out += [("null_counts", {"counts"}, put(counts=None), "null stream pointer"),
            ("null_escapes", {"escapes"}, put(escapes=None), "null stream pointer"),
            ("null_in", {"d_in"}, put(d_in=None), "null stream pointer")]
    if kind != "coalesce":
        out += [("null_table", {"table"}, put(table=None), "null h_rects" if kind == "crop" else "null h_place")]
    out += [("null_offsets", {"offsets"}, put(offsets=None), "null output pointer")]
    if cwire:
        out += [("null_frame_pos", {"frame_pos"}, put(frame_pos=None), "null output pointer")]
    out += [("null_out", {"out"}, put(out=None), "null output pointer")]
    if not cwire:
        out += [("null_diff", {"diff"}, put(diff=None), "null output pointer")]
    if kind == "crop":
        out += [("rect_negative", {"table"}, row0(-1, 0, 100, 100), "rectangle with a negative member"),
                ("rect_outside", {"table"}, row0(60, 0, 10, 10), "rectangle outside the frame")]
    if kind == "mosaic":
        out += [("place_negative", {"table"}, row0(-1, 0, 100, 100, FAR, FAR), "placement with a negative member"),
                ("place_source", {"table"}, row0(60, 0, 10, 10, FAR, FAR), "source rectangle outside the frame"),
                ("place_destination", {"table"}, row0(0, 0, 10, 10, FAR, 0), "destination rectangle outside the canvas")]
    out += [("header_escapes", {"escapes"}, head0("escapes", 0xFFFFFFFF), "frame header: more escapes than entries"),
            ("header_entries", {"counts"}, head0("counts", N + 1), "frame header: more entries than frame bytes"),
            ("overlap_offsets", {"offsets"}, at_input("offsets", 4), "d_offsets and the input stream overlap")]
    if cwire:
        out += [("overlap_frame_pos", {"frame_pos"}, at_input("frame_pos", 8), "d_frame_pos and the input stream overlap"),
                ("overlap_out", {"out"}, at_input("out", 4), "d_cwire_out and the input stream overlap")]
    else:
        out += [("overlap_out", {"out"}, at_input("out", 4), "d_xs and the input stream overlap"),
                ("overlap_diff", {"diff"}, at_input("diff", 5), "d_diff and the input stream overlap")]
    return out


CASES = [(form, k) for form in FORMS for k in range(len(ladder(form)))]


@pytest.mark.parametrize("form,k", CASES, ids=[f"{form_id(form)}-{ladder(form)[k][0]}" for form, k in CASES])
def test_rung_wins_over_every_later_rung(L, core, arena, form, k):
    rungs = ladder(form)
    a = valid(form, core, arena)
    taken, broken = set(), []
    for name, keys, how, _ in rungs[k:]:
        if taken & keys:
            continue
        how(a, arena.data_ptr())
        taken |= keys
        broken.append(name)
    assert broken[0] == rungs[k][0] and (len(broken) > 1 or k == len(rungs) - 1), broken
    rc = call(L, form, a)
    assert rc == lib.ERR_INVALID, (broken, rc)
    assert last_error(L) == rungs[k][3], broken


@pytest.mark.parametrize("kind", ["crop", "mosaic"])
@pytest.mark.parametrize("cwire", [False, True], ids=["arrays", "compact"])
def test_rung_11_goes_stream_by_stream(L, core, arena, kind, cwire):
    """Stream 0 outside the frame, stream 1 with a negative member: stream 0's mistake is the one reported."""
    a = valid((kind, cwire), core, arena)
    a["table"][0, :4] = (60, 0, 10, 10)
    a["table"][1, 0] = -1
    assert call(L, (kind, cwire), a) == lib.ERR_INVALID
    assert last_error(L) == ("rectangle outside the frame" if kind == "crop" else "source rectangle outside the frame")


# ---- rung 7: the empty batch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=form_id)
@pytest.mark.parametrize("S0,K0", [(0, 2), (2, 0)], ids=["no_streams", "no_frames"])
def test_empty_batch_writes_the_heads_and_nothing_else(L, core, arena, form, S0, K0):
    arena.fill_(FILL)
    torch.cuda.synchronize()
    a = valid(form, core, arena)
    a.update(S=S0, K=K0, d_in=None, counts=None, escapes=None, table=None)
    assert call(L, form, a) == lib.OK, last_error(L)
    core.synchronize()
    got = arena.cpu().numpy()
    want = np.full(got.size, FILL, np.uint8)
    want[OFFSETS * SLOT:OFFSETS * SLOT + 4] = 0
    if form[1]:
        want[FRAME_POS * SLOT:FRAME_POS * SLOT + 8] = 0
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


# ---- rung 14: the launch --------------------------------------------------------------------------------------------------
def reference(kind):
    """-> (offsets, xs, diff, records, frame_pos) of the valid call, segments (one for the mosaic) in stream order."""
    if kind == "mosaic":
        return mosaic_spec.reference(RECS, S, K, W, H, PLACE[:S], CANVAS_W, CANVAS_H)
    rects = RECTS[:S] if kind == "crop" else [(0, 0, W, H)] * S
    return crop_spec.reference(RECS, S, K, W, H, rects)


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_valid_call_launches(L, core, arena, form):
    kind, cwire = form
    off, xs, df, out, pos = reference(kind)
    assert 0 < off[-1] <= CAP and out.size <= CAP_BYTES and (kind == "mosaic" or off[1] < off[2])
    arena.fill_(FILL)
    arena[:RECS.size].copy_(torch.from_numpy(RECS))
    torch.cuda.synchronize()
    assert call(L, form, valid(form, core, arena)) == lib.OK, last_error(L)
    core.synchronize()
    got = arena.cpu().numpy()
    slot = (lambda i, nbytes, dtype: got[i * SLOT:i * SLOT + nbytes].view(dtype))
    want = np.full(got.size, FILL, np.uint8)
    want[:RECS.size] = RECS
    want[OFFSETS * SLOT:OFFSETS * SLOT + 4 * off.size] = off.view(np.uint8)
    assert np.array_equal(slot(OFFSETS, 4 * off.size, np.uint32), off)
    if cwire:
        assert np.array_equal(slot(FRAME_POS, 8 * pos.size, np.uint64), pos)
        assert np.array_equal(slot(OUT, out.size, np.uint8), out)
        want[FRAME_POS * SLOT:FRAME_POS * SLOT + 8 * pos.size] = pos.view(np.uint8)
        want[OUT * SLOT:OUT * SLOT + out.size] = out
    else:
        assert np.array_equal(slot(OUT, 4 * xs.size, np.int32), xs)
        assert np.array_equal(slot(DIFF, df.size, np.uint8), df)
        want[OUT * SLOT:OUT * SLOT + 4 * xs.size] = xs.view(np.uint8)
        want[DIFF * SLOT:DIFF * SLOT + df.size] = df
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]   # (and not a byte anywhere else)

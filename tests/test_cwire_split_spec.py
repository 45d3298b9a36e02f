"""mi355_cwire_split_host against the piece rule stated in numpy (split_spec), and the rule's laws through the library's host
checker and host client: every piece is canonical, the pieces applied in any order give the state the record gives, and a subset
touches only its own indices.  The capacity helpers are never below what the rule produces.  No GPU."""
import numpy as np
import pytest

import cwire_spec as spec
import split_spec
from cudavideostream_amd import (cwire_apply_host, cwire_check_host, cwire_split_bytes_max, cwire_split_host,
                                 cwire_split_pieces_max, lib)

CASES = split_spec.cases()


@pytest.fixture(scope="module")
def results():
    """name -> (frame bytes, records, counts, escapes, M, the model's tables and bytes, the host form's): made once."""
    out = {}
    for name, ((w, h), segs, M) in CASES.items():
        buf, counts, escapes = split_spec.records(segs)
        out[name] = (3 * w * h, buf, counts, escapes, M, split_spec.reference(buf, len(segs), M),
                     cwire_split_host(buf, counts, escapes, 3 * w * h, M))
    return out


def piece_list(first, pos, out):
    total = int(first[-1])
    return [out[int(pos[p]):int(pos[p + 1])] for p in range(total)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_form_is_the_model(results, name):
    n, buf, counts, escapes, M, (wf, wp, wo), (gf, gp, go) = results[name]
    total = int(wf[-1])
    assert np.array_equal(gf, wf)
    assert np.array_equal(gp[:total + 1], wp)
    assert np.array_equal(go[:int(wp[-1])], wo)
    assert not go[int(wp[-1]):].any()
    assert all(int(wp[p + 1] - wp[p]) <= M for p in range(total))


@pytest.mark.parametrize("name", sorted(CASES))
def test_helpers_are_sufficient(results, name):
    n, buf, counts, escapes, M, (wf, wp, wo), _ = results[name]
    for r, (cnt, e) in enumerate(zip(counts, escapes)):
        pieces = int(wf[r + 1]) - int(wf[r])
        size = int(wp[int(wf[r + 1])]) - int(wp[int(wf[r])])
        assert cwire_split_pieces_max(cnt, e, M) == split_spec.pieces_max(cnt, e, M) >= pieces
        assert cwire_split_bytes_max(cnt, e, M) == split_spec.bytes_max(cnt, e, M) >= size


def test_helpers_on_random_records():
    rng = np.random.default_rng(7)
    N = 3 * 512 * 128
    for i in range(200):
        cnt = int(rng.integers(0, 3000))
        if i % 3 == 0:      # sparse: nearly every entry escaped
            xs = np.sort(rng.choice(N, cnt, replace=False))
        elif i % 3 == 1:    # runs
            xs = np.unique(np.concatenate([np.arange(s, s + int(rng.integers(1, 40))) for s in rng.integers(0, N - 40, max(cnt // 20, 1))]))
        else:               # dense
            xs = np.arange(cnt) + int(rng.integers(0, 1000))
        M = int(rng.choice([64, 68, 100, 256, 1400, 8972, 65536]))
        g = spec.gaps(xs)
        e = int((g >= 255).sum())
        pieces = split_spec.split_record(xs, np.ones(xs.size, np.uint8), M)
        assert cwire_split_pieces_max(xs.size, e, M) >= len(pieces)
        assert cwire_split_bytes_max(xs.size, e, M) >= sum(len(p) for p in pieces)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_piece_is_canonical(results, name):
    n, buf, counts, escapes, M, _, (gf, gp, go) = results[name]
    pieces = piece_list(gf, gp, go)
    if not pieces:
        return
    pc, pe = spec.headers(go, len(pieces))
    verdicts = cwire_check_host(go[:int(gp[len(pieces)])], pc, pe, n)
    assert not verdicts[:, 0].any()
    # back to back the pieces decode to the records' (xs, diff)
    _, xs, df = spec.decode(go, len(pieces))
    _, wxs, wdf = spec.decode(buf, counts.size)
    assert np.array_equal(xs, wxs) and np.array_equal(df, wdf)


@pytest.mark.parametrize("name", sorted(n for n in CASES if not n.startswith("records_")))
def test_shuffled_apply_and_subsets(results, name):
    n, buf, counts, escapes, M, _, (gf, gp, go) = results[name]
    rng = np.random.default_rng(len(name))
    at = 0
    for r in range(counts.size):
        rec = buf[at:at + spec.frame_bytes(counts[r], escapes[r])]
        at += rec.size
        pieces = piece_list(gf, gp, go)[int(gf[r]):int(gf[r + 1])]
        A = rng.integers(0, 256, n, dtype=np.uint8)
        want = A.copy()
        assert cwire_apply_host(want, rec, 1) == rec.size
        got = A.copy()
        for i in rng.permutation(len(pieces)):
            assert cwire_apply_host(got, pieces[i], 1) == pieces[i].size
        assert np.array_equal(got, want)
        # a subset: exactly its own indices change, to the record's values
        keep = [i for i in range(len(pieces)) if rng.integers(0, 2)]
        part = A.copy()
        mine = np.zeros(n, bool)
        for i in keep:
            assert cwire_apply_host(part, pieces[i], 1) == pieces[i].size
            mine[spec.decode(pieces[i], 1)[1]] = True
        assert np.array_equal(part, np.where(mine, want, A))


def test_a_record_that_fits_comes_back_byte_for_byte():
    rng = np.random.default_rng(3)
    xs = np.sort(rng.choice(9216, 200, replace=False))
    buf, counts, escapes = split_spec.records([(xs, rng.integers(1, 256, xs.size))])
    first, pos, out = cwire_split_host(buf, counts, escapes, 9216, 65536)
    assert list(first) == [0, 1] and int(pos[1]) == buf.size
    assert np.array_equal(out[:buf.size], buf)


def test_capacities_skip_whole_pieces():
    (w, h), segs, M = CASES["wave_seam_M516"]
    buf, counts, escapes = split_spec.records(segs)
    wf, wp, wo = split_spec.reference(buf, len(segs), M)
    total = int(wf[-1])
    # one piece short in the table: the last piece is not written, the tables are exact as far as they reach
    gf, gp, go = cwire_split_host(buf, counts, escapes, 3 * w * h, M, piece_capacity=total - 1, capacity_bytes=int(wp[-1]))
    assert np.array_equal(gf, wf) and np.array_equal(gp, wp[:total])
    assert np.array_equal(go[:int(wp[total - 1])], wo[:int(wp[total - 1])]) and not go[int(wp[total - 1]):].any()
    # bytes for all but the last piece: the same
    gf, gp, go = cwire_split_host(buf, counts, escapes, 3 * w * h, M, piece_capacity=total, capacity_bytes=int(wp[-1]) - 4)
    assert np.array_equal(gf, wf) and np.array_equal(gp, wp)
    assert np.array_equal(go[:int(wp[total - 1])], wo[:int(wp[total - 1])]) and not go[int(wp[total - 1]):].any()


def _host(buf, counts, escapes, nrecords, M, first, pos, cap, out, capb, frame=9216, nbytes=None):
    L = lib.load()
    ptr = (lambda a: None if a is None else a.ctypes.data)
    return L.mi355_cwire_split_host(frame, ptr(buf), buf.size if nbytes is None else nbytes, ptr(counts), ptr(escapes), nrecords, M,
                                    ptr(first), ptr(pos), cap, ptr(out), capb)


def test_refusals():
    rng = np.random.default_rng(5)
    buf, counts, escapes = split_spec.records([(np.arange(40), rng.integers(1, 256, 40))])
    first, pos, out = np.full(2, 77, np.uint32), np.full(9, 77, np.uint64), np.full(256, 77, np.uint8)
    ok = (buf, counts, escapes, 1, 64, first, pos, 8, out, 256)
    assert _host(*ok) == lib.OK
    first[:], pos[:], out[:] = 77, 77, 77

    def refused(*args, **kw):
        assert _host(*args, **kw) == lib.ERR_INVALID
        assert (first == 77).all() and (pos == 77).all() and (out == 77).all()

    for M in (0, 60, 66, 65540, 1 << 20):
        refused(buf, counts, escapes, 1, M, first, pos, 8, out, 256)
    refused(buf, counts, escapes, -1, 64, first, pos, 8, out, 256)
    refused(None, counts, escapes, 1, 64, first, pos, 8, out, 256, nbytes=buf.size)
    refused(buf, None, escapes, 1, 64, first, pos, 8, out, 256)
    refused(buf, counts, None, 1, 64, first, pos, 8, out, 256)
    refused(buf, counts, escapes, 1, 64, None, pos, 8, out, 256)
    refused(buf, counts, escapes, 1, 64, first, None, 8, out, 256)
    refused(buf, counts, escapes, 1, 64, first, pos, 8, None, 256)
    refused(buf, counts, escapes + 41, 1, 64, first, pos, 8, out, 256)              # more escapes than entries
    refused(buf, counts, escapes, 1, 64, first, pos, 8, out, 256, frame=39)         # more entries than frame bytes
    refused(buf, counts, escapes, 1, 64, first, pos, 8, out, 256, nbytes=buf.size - 1)
    refused(buf, counts, escapes, 1, 64, first, pos, 8, out, 256, frame=0xFFFFFFFF)
    # the input span overlapping an output region
    both = np.full(1024, 77, np.uint8)
    both[:buf.size] = buf
    L = lib.load()
    rc = L.mi355_cwire_split_host(9216, both.ctypes.data, buf.size, counts.ctypes.data, escapes.ctypes.data, 1, 64, first.ctypes.data,
                                  pos.ctypes.data, 8, both.ctypes.data + 16, 256)
    assert rc == lib.ERR_INVALID and np.array_equal(both[:buf.size], buf) and (both[buf.size:] == 77).all()
    # nrecords == 0: the two heads and nothing else
    assert _host(buf, counts, escapes, 0, 64, first, pos, 8, out, 256) == lib.OK
    assert list(first) == [0, 77] and int(pos[0]) == 0 and (pos[1:] == 77).all() and (out == 77).all()
    assert cwire_split_pieces_max(100, 0, 60) == 0 and cwire_split_bytes_max(100, 0, 1 << 20) == 0

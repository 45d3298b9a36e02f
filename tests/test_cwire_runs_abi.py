"""CPU-side checks of the run-coded records (mi355_cwire_runs_*): the library exports the entry points, the header declares them
and the binding lists them; the host forms against tests/runs_spec.py on the shared patterns under both policies, the round trip,
the capacity skip, every refusal of the host forms, the refusals of the batch forms that need no device, the size helpers and
their bound, the ABI number and its history, and the stand-alone C++ program under tests/host/.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cudavideostream_amd
import cwire_spec as spec
import runs_spec as rs
from cudavideostream_amd import (CUDACore, cwire_bytes_max, cwire_runs_bytes_max, cwire_runs_decode_host, cwire_runs_encode_host,
                                 cwire_runs_frame_bytes, lib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_cwire_runs_frame_bytes": 3, "mi355_cwire_runs_bytes_max": 3, "mi355_cwire_runs_encode_host": 11,
         "mi355_cwire_runs_encode_batch": 10, "mi355_cwire_runs_decode_host": 8, "mi355_cwire_runs_decode_batch": 7}
N = 9216
FILL = 0x5C
POLICIES = [lib.RUNS_WHERE_SMALLER, lib.RUNS_ALWAYS]


@pytest.fixture(scope="module")
def built():
    lib.build()
    return lib.load()


@pytest.fixture(scope="module")
def stream():
    """(the shared patterns' records back to back, counts, escapes)."""
    pats = rs.patterns(N)
    buf = np.concatenate([rs.record(xs, i) for i, xs in enumerate(pats.values())])
    counts, escapes = spec.headers(buf, len(pats))
    return buf, counts, escapes


def declared_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/mi355diff.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(NAMES))
def test_symbol_is_exported_declared_and_bound(built, name):
    assert hasattr(built, name), f"{name} is not exported by the built library"
    assert name in lib.SYMBOLS
    assert declared_args(name) == len(lib.SYMBOLS[name][1]) == NAMES[name]


def test_python_surface_and_constants():
    assert callable(CUDACore.cwire_runs_encode_batch) and callable(CUDACore.cwire_runs_decode_batch)
    for name in ("cwire_runs_encode_host", "cwire_runs_decode_host", "cwire_runs_frame_bytes", "cwire_runs_bytes_max"):
        assert callable(getattr(cudavideostream_amd, name))
    text = open(HEADER).read()
    for name, value in (("RUNS_WHERE_SMALLER", 0), ("RUNS_ALWAYS", 1), ("RUNS_FORM_COMPACT", 0), ("RUNS_FORM_RUNS", 1)):
        assert int(re.search(r"#define MI355_" + name + r" (\d+)u?\b", text).group(1)) == getattr(lib, name) == value
    assert (rs.WHERE_SMALLER, rs.ALWAYS, rs.FORM_COMPACT, rs.FORM_RUNS) == (0, 1, 0, 1)


def test_abi_version_is_still_10_and_the_history_names_the_additions(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    text = open(HEADER).read()
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", text)
    assert m and int(m.group(1)) == 10
    history = text[text.index("ABI version of this header"):m.start()]
    for name in NAMES:
        assert name in history, name
    assert "MI355_RUNS_* (additions only)" in history


@pytest.mark.parametrize("policy", POLICIES)
def test_host_forms_against_the_spec_and_round_trip(built, stream, policy):
    buf, counts, escapes = stream
    want_forms, want_pos, want = rs.encode(buf, counts.size, policy)
    forms, pos, out = cwire_runs_encode_host(buf, counts, escapes, N, policy)
    assert np.array_equal(forms, want_forms) and np.array_equal(pos, want_pos)
    assert out[:want.size].tobytes() == want.tobytes() and not out[want.size:].any()
    frame_pos, back = cwire_runs_decode_host(out[:want.size], forms, N)
    assert back.tobytes() == buf.tobytes()
    assert np.array_equal(frame_pos, rs.decode(want, want_forms)[0])
    assert int(frame_pos[-1]) == buf.size


@pytest.mark.parametrize("policy", POLICIES)
def test_a_record_that_does_not_fit_is_skipped_whole(built, stream, policy):
    """Record b is written iff pos[b + 1] <= capacity_bytes, on either side of the link; the positions are exact regardless and no
    byte of a skipped record, or behind the capacity, is written."""
    buf, counts, escapes = stream
    n = counts.size
    forms, pos, full = cwire_runs_encode_host(buf, counts, escapes, N, policy)
    b = n // 2                                                        # a record in the middle
    cap = int(pos[b + 1]) - 4
    f2, p2, out = np.zeros_like(forms), np.zeros_like(pos), np.full(int(pos[-1]) + 64, FILL, np.uint8)
    lib.check(built.mi355_cwire_runs_encode_host(N, buf.ctypes.data, buf.size, counts.ctypes.data, escapes.ctypes.data, n, policy,
                                                 f2.ctypes.data, p2.ctypes.data, out.ctypes.data, cap))
    assert np.array_equal(f2, forms) and np.array_equal(p2, pos)
    assert out[:int(pos[b])].tobytes() == full[:int(pos[b])].tobytes() and (out[int(pos[b]):] == FILL).all()
    link = full[:int(pos[-1])]
    fp_full, _ = cwire_runs_decode_host(link, forms, N)
    out = np.full(buf.size + 64, FILL, np.uint8)
    frame_pos, _ = cwire_runs_decode_host(link, forms, N, capacity_bytes=int(fp_full[b + 1]) - 4, out=out)
    assert np.array_equal(frame_pos, fp_full)
    assert out[:int(fp_full[b])].tobytes() == buf[:int(fp_full[b])].tobytes() and (out[int(fp_full[b]):] == FILL).all()


def test_the_capacity_rule_record_by_record(built):
    """Three records, the middle one large, at three capacities: each record is written exactly when its end lies inside."""
    recs = [rs.record([7]), rs.record(np.arange(1000)), rs.record([5])]
    buf = np.concatenate(recs)
    counts, escapes = spec.headers(buf, 3)
    forms, pos, link = cwire_runs_encode_host(buf, counts, escapes, N, lib.RUNS_WHERE_SMALLER)
    assert forms[:, 0].tolist() == [0, 1, 0]
    for cap in (recs[0].size, recs[0].size + recs[1].size - 4, buf.size):
        out = np.full(buf.size, FILL, np.uint8)
        frame_pos, _ = cwire_runs_decode_host(link[:int(pos[-1])], forms, N, capacity_bytes=cap, out=out)
        assert frame_pos.tolist() == [0, 16, 16 + recs[1].size, buf.size]
        for i in range(3):
            a, b = int(frame_pos[i]), int(frame_pos[i + 1])
            assert (out[a:b].tobytes() == buf[a:b].tobytes()) if b <= cap else (out[a:b] == FILL).all(), (cap, i)


def run_record(n, e, gap, ln, diff=None):
    """A record in the run form from its parts, well formed or not."""
    r = len(gap)
    q = spec.pad4(r)
    g, l = np.zeros(q, np.uint8), np.zeros(q, np.uint8)
    g[:r], l[:r] = gap, ln
    d = np.zeros(spec.pad4(n), np.uint8)
    d[:n] = 1 if diff is None else diff
    return np.concatenate([np.array([n, e, r], "<u4").view(np.uint8), g, l, np.zeros(4 * e, np.uint8), d]), [1, n, e, r]


def test_decode_host_refusals(built):
    good, row = run_record(300, 0, [3, 0], [255, 43])
    first = rs.record([1, 2, 3])
    link = np.concatenate([first, good])
    ok_forms = np.array([[0, 3, 0, 1], row], np.uint32)
    frame_pos, back = cwire_runs_decode_host(link, ok_forms, N)
    assert back[:first.size].tobytes() == first.tobytes() and int(frame_pos[-1]) == first.size + spec.frame_bytes(300, 0)

    def refused(link, forms, why):
        out = np.full(4096, FILL, np.uint8)
        with pytest.raises(lib.Mi355Error) as err:
            cwire_runs_decode_host(link, forms, N, out=out)
        assert err.value.code == lib.ERR_INVALID and why in str(err.value), (why, str(err.value))
        return out

    out = refused(link[:-4], ok_forms, "truncated")
    assert out[:first.size].tobytes() == first.tobytes()          # the record before the bad one stays written
    refused(link, [[0, 3, 0, 1], [2, 300, 0, 2]], "form")
    refused(link, [[0, 3, 0, 1], [1, N + 1, 0, 2]], "entries")
    refused(link, [[0, 3, 4, 1], row], "escapes")
    refused(link, [[0, 3, 0, 4], row], "runs")
    for gap, ln, e, why in (([3, 0], [254, 44], 0, "crosses"),     # 255 + 45: the second run crosses entry 256
                            ([3, 0], [255, 42], 0, "sum"),         # 299 entries
                            ([3, 0, 0], [255, 43, 0], 0, "sum"),   # 301 entries
                            ([3, 255], [255, 43], 0, "255"),       # one 255 gap, e = 0
                            ([3, 0], [255, 43], 1, "255")):        # no 255 gap, e = 1
        bad, brow = run_record(300, e, gap, ln)
        out = refused(np.concatenate([first, bad]), [[0, 3, 0, 1], brow], why)
        assert out[:first.size].tobytes() == first.tobytes() and (out[first.size:] == FILL).all()


def test_host_forms_refuse_bad_arguments(built, stream):
    buf, counts, escapes = stream
    L, n = built, counts.size
    forms, pos, out = np.zeros((n, 4), np.uint32), np.zeros(n + 1, np.uint64), np.zeros(cwire_runs_bytes_max(N, n, 1), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data

    def enc(**kw):
        d = dict(frame_bytes=N, cwire=p(buf), cwire_bytes=buf.size, counts=p(counts), escapes=p(escapes), nrecords=n, policy=0,
                 forms=p(forms), pos=p(pos), out=p(out), capacity=out.size)
        d.update(kw)
        return L.mi355_cwire_runs_encode_host(*d.values())

    assert enc() == lib.OK
    big = counts.copy(); big[1] = N + 1
    more = escapes.copy(); more[1] = counts[1] + 1
    for kw in (dict(nrecords=-1), dict(policy=2), dict(policy=-1), dict(cwire=None), dict(counts=None), dict(escapes=None),
               dict(forms=None), dict(pos=None), dict(out=None), dict(cwire_bytes=buf.size - 4), dict(counts=p(big)),
               dict(escapes=p(more)), dict(out=p(buf) + 8, capacity=64), dict(frame_bytes=2 ** 32)):
        assert enc(**kw) == lib.ERR_INVALID, kw
    pos[:] = 77
    assert enc(nrecords=0, cwire=None, forms=None, out=None) == lib.OK and int(pos[0]) == 0 and int(pos[1]) == 77
    fp = np.full(n + 1, 77, np.uint64)

    def dec(**kw):
        d = dict(frame_bytes=N, inp=p(out), in_bytes=out.size, forms=p(forms), nrecords=n, frame_pos=p(fp), cwire=p(buf), capacity=buf.size)
        d.update(kw)
        return L.mi355_cwire_runs_decode_host(*d.values())

    back = buf.copy()
    assert dec(cwire=p(back)) == lib.OK and back.tobytes() == buf.tobytes()
    for kw in (dict(nrecords=-1), dict(inp=None), dict(forms=None), dict(frame_pos=None), dict(cwire=None),
               dict(cwire=p(out) + 16, capacity=64), dict(frame_bytes=2 ** 32)):
        assert dec(**kw) == lib.ERR_INVALID, kw
    fp[:] = 77
    assert dec(nrecords=0, inp=None, forms=None, cwire=None) == lib.OK and int(fp[0]) == 0 and int(fp[1]) == 77


def test_batch_forms_refuse_without_a_core(built):
    assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
    assert b"core" not in built.mi355_last_error()
    assert built.mi355_cwire_runs_encode_batch(None, None, None, None, 0, 0, None, None, None, 0) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()
    built.mi355_cwire_apply_host(None, 0, None, 0, 0, None)
    assert built.mi355_cwire_runs_decode_batch(None, None, None, 0, None, None, 0) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()


def test_size_helpers_against_the_spec(built):
    for n, e, r in ((0, 0, 0), (1, 1, 1), (6, 2, 3), (4097, 3, 17), (N, 0, N), (N, 0, 36)):
        assert cwire_runs_frame_bytes(n, e, r) == rs.runs_frame_bytes(n, e, r)
    assert cwire_runs_bytes_max(N, 3, lib.RUNS_ALWAYS) == 3 * (12 + 3 * spec.pad4(N))
    assert cwire_runs_bytes_max(N + 1, 1, lib.RUNS_ALWAYS) == 12 + 3 * (N + 4)
    assert cwire_runs_bytes_max(N, 3, lib.RUNS_WHERE_SMALLER) == cwire_bytes_max(N, 3)
    assert cwire_runs_bytes_max(N, 3, 2) == 0 and cwire_runs_bytes_max(N, 0, 0) == 0 and cwire_runs_bytes_max(N, -1, 1) == 0
    # the bound holds, with equality impossible to beat, on the two extremes: every entry its own run, and the full dense frame
    for xs in (np.arange(0, N, 2), np.arange(N), np.arange(1, N, 2)):
        rec = rs.record(xs)
        c, e = spec.headers(rec, 1)
        for policy in POLICIES:
            forms, pos, _ = cwire_runs_encode_host(rec, c, e, N, policy)
            assert int(pos[1]) <= cwire_runs_bytes_max(N, 1, policy), (xs.size, policy)
    alt = rs.record(np.arange(0, N, 2))
    c, e = spec.headers(alt, 1)
    forms, pos, _ = cwire_runs_encode_host(alt, c, e, N, lib.RUNS_ALWAYS)
    assert forms.tolist() == [[1, N // 2, 0, N // 2]] and int(pos[1]) == 12 + 3 * (N // 2)   # r == n: 1.5x the code bytes
    forms, pos, _ = cwire_runs_encode_host(alt, c, e, N, lib.RUNS_WHERE_SMALLER)
    assert forms.tolist() == [[0, N // 2, 0, N // 2]] and int(pos[1]) == alt.size
    dense = rs.record(np.arange(N))
    c, e = spec.headers(dense, 1)
    forms, pos, _ = cwire_runs_encode_host(dense, c, e, N, lib.RUNS_WHERE_SMALLER)
    assert forms.tolist() == [[1, N, 0, N // 256]] and int(pos[1]) == 12 + 2 * (N // 256) + N   # just over half of 8 + 2N


def test_stand_alone_host_program(built, tmp_path):
    """tests/host/cwire_runs_host.cpp: the two host forms over the same kinds of patterns from C++, with its own main."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "cwire_runs_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "host", "cwire_runs_host.cpp"),
                    "-I", os.path.join(ROOT, "include"), lib.LIB_PATH, "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH)], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "ok" in done.stdout

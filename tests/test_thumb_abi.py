"""CPU-side checks of the thumbnail records (mi355_thumb_cwire_host, mi355_thumb_cwire_batch): the library exports the two entry
points, the header declares them, the binding lists them with matching argument counts, the ABI version is still 10 (additions
only), the device form refuses a null core, the host form -- the definition -- equals the numpy statement byte for byte at every
shape of the GPU tests, refuses what the header says it refuses, leaves everything untouched when the record does not fit, and
the C++ drop-in has CUDACore::thumb_cwire_multi."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cudavideostream_amd as pkg
import thumb_spec as ts
import wall_spec as ws
from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_thumb_cwire_host": 12, "mi355_thumb_cwire_batch": 13}


@pytest.fixture(scope="module")
def built():
    lib.build()
    return lib.load()


def declared_args(name):
    """Number of arguments of `name`'s prototype in the header."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/mi355diff.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(NAMES))
def test_symbol_is_exported_declared_and_bound(built, name):
    assert hasattr(built, name), f"{name} is not exported by the built library"
    assert name in lib.SYMBOLS
    assert declared_args(name) == len(lib.SYMBOLS[name][1]) == NAMES[name]


def test_python_layer_has_the_calls():
    assert callable(CUDACore.thumb_cwire_batch) and callable(pkg.thumb_cwire_host)


def test_header_has_the_section():
    text = open(HEADER).read()
    assert "Thumbnail records" in text and "ITS STREAM'S HELD THUMBNAIL IS NOT WRITTEN AT ALL" in text


def test_abi_version_is_still_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_device_form_refuses_without_a_core(built):
    call = lambda n: built.mi355_thumb_cwire_batch(None, None, 0, n, 1, 0, None, None, 0, None, None, None, 0)
    assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
    assert b"core" not in built.mi355_last_error()
    assert call(1) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()
    assert call(0) == lib.ERR_INVALID


def host(built, state, w, h, k, thr, thumb, mask, capacity, guard=16):
    """The raw call on guarded copies: -> (rc, out bytes with guards, thumb after with guards, n, e, bytes)."""
    out = np.full(capacity + 2 * guard, 0xA5, np.uint8)
    th = np.full(thumb.size + 2 * guard, 0x5A, np.uint8)
    th[guard:guard + thumb.size] = thumb
    n, e, nb = C.c_uint32(77), C.c_uint32(78), C.c_size_t(79)
    rc = built.mi355_thumb_cwire_host(state.ctypes.data, w, h, k, thr, None if mask is None else mask.ctypes.data,
                                      th.ctypes.data + guard, out.ctypes.data + guard, capacity, C.byref(n), C.byref(e), C.byref(nb))
    return rc, out, th, n.value, e.value, nb.value


def masks_of(rng, w, h):
    n = 3 * w * h
    sels = [None, np.zeros(ws.tiles(n), bool), rng.random(ws.tiles(n)) < 0.5]
    if (w, h) == (100, 60):
        sels += list(ts.one_tile_masks(n))
    return sels


@pytest.mark.parametrize("w,h,k", ts.SHAPES)
def test_host_form_is_the_spec(built, w, h, k):
    rng = np.random.default_rng(11 * w + k)
    nt, guard = ts.thumb_bytes(w, h, k), 16
    state = ts.random_states(rng, 1, w, h)[0]
    inputs = [(state, rng.integers(0, 256, nt, dtype=np.uint8)), (state, ws.thumbnail(state, w, h, k).reshape(-1).copy())]
    if (w, h, k) == (64, 48, 16):
        inputs += [(np.full(state.size, 255, np.uint8), np.zeros(nt, np.uint8)), (ts.tie_state(w, h, k), np.zeros(nt, np.uint8))]
    for st, thumb in inputs:
        for sel in masks_of(rng, w, h):
            for thr in (0, 20, 255):
                want, after, xs, _ = ts.step(st, thumb, w, h, k, thr, sel)
                mask = None if sel is None else ws.mask_of(sel[None, :])[0]
                cap = pkg.cwire_bytes_max(nt, 1)
                rc, out, th, n, e, nb = host(built, st, w, h, k, thr, thumb, mask, cap)
                assert rc == lib.OK and (n, nb) == (xs.size, len(want))
                assert out[guard:guard + nb].tobytes() == want and e == int(np.frombuffer(want[4:8], "<u4")[0])
                assert (out[:guard] == 0xA5).all() and (out[guard + nb:] == 0xA5).all()
                assert np.array_equal(th[guard:guard + nt], after) and (th[:guard] == 0x5A).all() and (th[guard + nt:] == 0x5A).all()
                # the python wrapper, and one byte short: exact sizes, nothing written
                t2 = thumb.copy()
                assert pkg.thumb_cwire_host(st, w, h, k, thr, t2, mask) == (want, n, e) and np.array_equal(t2, after)
                rc, out, th, n2, e2, nb2 = host(built, st, w, h, k, thr, thumb, mask, nb - 1)
                assert rc == lib.OK and (n2, e2, nb2) == (n, e, nb)
                assert (out == 0xA5).all() and np.array_equal(th[guard:guard + nt], thumb)


def test_host_form_mechanics(built):
    for name, a, b in ts.mechanics_ticks(np.random.default_rng(3)):
        held = ws.thumbnail(a, 100, 60, 2).reshape(-1).copy()
        sel = ts.touched_sel(a, b)
        want, after, _, _ = ts.step(b, held, 100, 60, 2, 0, sel)
        rec, n, e = pkg.thumb_cwire_host(b, 100, 60, 2, 0, held, ws.mask_of(sel[None, :])[0])
        assert rec == want and np.array_equal(held, after), name


def test_host_form_refusals(built):
    w, h, k = 37, 11, 2
    state = np.zeros(3 * w * h, np.uint8)
    thumb = np.full(ts.thumb_bytes(w, h, k), 9, np.uint8)
    out = np.full(4096, 0xA5, np.uint8)
    n, e, nb = C.c_uint32(77), C.c_uint32(78), C.c_size_t(79)
    good = dict(state=state.ctypes.data, w=w, h=h, k=k, thr=0, mask=None, thumb=thumb.ctypes.data, out=out.ctypes.data, cap=out.size,
                n=C.byref(n), e=C.byref(e), nb=C.byref(nb))
    bad = [dict(state=None), dict(thumb=None), dict(n=None), dict(e=None), dict(nb=None), dict(out=None), dict(w=0), dict(h=0),
           dict(w=-3), dict(w=32768, h=21846), dict(k=0), dict(k=17), dict(thr=-1), dict(thr=256)]
    assert 3 * 32768 * 21846 >= 2 ** 31 > 3 * 32768 * 21845
    for change in bad:
        a = dict(good, **change)
        rc = built.mi355_thumb_cwire_host(a["state"], a["w"], a["h"], a["k"], a["thr"], a["mask"], a["thumb"], a["out"], a["cap"],
                                          a["n"], a["e"], a["nb"])
        assert rc == lib.ERR_INVALID, change
        assert (out == 0xA5).all() and (thumb == 9).all() and (n.value, e.value, nb.value) == (77, 78, 79), change
    a = dict(good, out=None, cap=0)   # a null out with no capacity is a size query
    assert built.mi355_thumb_cwire_host(a["state"], w, h, k, 0, None, a["thumb"], None, 0, a["n"], a["e"], a["nb"]) == lib.OK
    assert (n.value, nb.value) == (thumb.size, 8 + 2 * ((thumb.size + 3) & ~3) + 4 * e.value) and (thumb == 9).all()


def test_drop_in_method_compiles_and_links(built, tmp_path):
    """diff::cuda::CUDACore::thumb_cwire_multi is declared in the drop-in's header and defined in libmi355compat.a (a program that
    only takes its address: nothing runs, no device is needed); the object keeps the reference's 160 bytes."""
    compat = os.path.join(ROOT, "cudavideostream_amd", "compat")
    subprocess.run(["make", "-C", compat, "-s"], check=True)
    src = tmp_path / "link_thumb.cpp"
    src.write_text('#include "kernels.cuh"\n'
                   "using diff::cuda::CUDACore;\n"
                   "typedef void (CUDACore::*fn_thumb)(const void *, size_t, int, int, int, const void *, void *, size_t, void *, void *,"
                   " void *, size_t);\n"
                   'static_assert(sizeof(CUDACore) == 160, "object size");\n'
                   "int main() {\n"
                   "    volatile fn_thumb a = &CUDACore::thumb_cwire_multi;\n"
                   "    return a ? 0 : 1;\n"
                   "}\n")
    exe = tmp_path / "link_thumb"
    libd = os.path.join(ROOT, "cudavideostream_amd")
    subprocess.run(["g++", "-std=c++11", "-I", os.path.join(compat, "include"), "-o", str(exe), str(src),
                    os.path.join(compat, "libmi355compat.a"), "-L", libd, "-lmi355diff", f"-Wl,-rpath,{libd}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0

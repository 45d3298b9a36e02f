"""CPU-side checks of the motion grids (mi355_activity_batch, mi355_cwire_activity_batch, mi355_activity_cells): the library
exports the three entry points, the header declares them, the binding lists them with matching argument counts, the ABI version
is still 10 (additions only), both device calls refuse a null core, the C++ drop-in has CUDACore::activity_multi, and the
host-only mi355_activity_cells agrees with a brute-force loop."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cudavideostream_amd import CUDACore, activity_cells, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_activity_cells": 6, "mi355_activity_batch": 11, "mi355_cwire_activity_batch": 12}


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
    assert callable(CUDACore.activity_batch) and callable(CUDACore.cwire_activity_batch) and callable(activity_cells)


def test_abi_version_is_still_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


@pytest.mark.parametrize("name,args", [
    ("mi355_activity_batch", (None, None, None, 1, 1, 16, 16, 1, 0, None, None)),
    ("mi355_cwire_activity_batch", (None, None, None, None, 1, 1, 16, 16, 1, 0, None, None)),
])
def test_refuse_without_a_core(built, name, args):
    assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
    assert b"core" not in built.mi355_last_error()
    assert getattr(built, name)(*args) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()


def test_drop_in_activity_multi_compiles_and_links(built, tmp_path):
    """diff::cuda::CUDACore::activity_multi is declared in the drop-in's header and defined in libmi355compat.a (a program that
    only takes its address: nothing runs, no device is needed); the object keeps the reference's 160 bytes."""
    compat = os.path.join(ROOT, "cudavideostream_amd", "compat")
    subprocess.run(["make", "-C", compat, "-s"], check=True)
    src = tmp_path / "link_activity_multi.cpp"
    src.write_text('#include "kernels.cuh"\n'
                   "typedef void (diff::cuda::CUDACore::*fn)(const void *, const uint32_t *, const uint32_t *, int, int, int, int, "
                   "uint32_t, int, void *, void *);\n"
                   'static_assert(sizeof(diff::cuda::CUDACore) == 160, "object size");\n'
                   "int main() { volatile fn f = &diff::cuda::CUDACore::activity_multi; return f ? 0 : 1; }\n")
    exe = tmp_path / "link_activity_multi"
    libd = os.path.join(ROOT, "cudavideostream_amd")
    subprocess.run(["g++", "-std=c++11", "-I", os.path.join(compat, "include"), "-o", str(exe), str(src),
                    os.path.join(compat, "libmi355compat.a"), "-L", libd, "-lmi355diff", f"-Wl,-rpath,{libd}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


# ---- mi355_activity_cells -------------------------------------------------------------------------------------------------
def brute(size, cell):
    """Cells along one axis: the number of different values of x // cell over the axis' pixels."""
    return len({x // cell for x in range(size)})


def test_activity_cells_against_brute_force(built):
    along = {(size, cell): brute(size, cell) for size in range(1, 41) for cell in range(1, 46)}
    for w in range(1, 41):
        for cw in range(1, 46):
            for h, ch in ((w, cw), (41 - w, 46 - cw), (7, 5), (40, 45)):
                assert activity_cells(w, h, cw, ch) == (along[w, cw] * along[h, ch], along[w, cw], along[h, ch]), (w, h, cw, ch)
    for h in range(1, 41):
        for ch in range(1, 46):
            assert activity_cells(37, h, 16, ch) == (3 * along[h, ch], 3, along[h, ch])


def test_activity_cells_refuses_and_takes_null_pointers(built):
    for bad in ((0, 5, 2, 2), (5, 0, 2, 2), (5, 5, 0, 2), (5, 5, 2, 0), (-1, 5, 2, 2), (5, -3, 2, 2), (5, 5, -2, 2), (5, 5, 2, -2)):
        assert activity_cells(*bad) == (0, 0, 0), bad
    gw, gh = C.c_int(-1), C.c_int(-1)
    assert built.mi355_activity_cells(50, 37, 16, 16, None, None) == 12
    assert built.mi355_activity_cells(50, 37, 16, 16, C.byref(gw), None) == 12 and gw.value == 4
    assert built.mi355_activity_cells(50, 37, 16, 16, None, C.byref(gh)) == 12 and gh.value == 3
    assert built.mi355_activity_cells(1920, 1080, 16, 16, None, None) == 120 * 68
    assert built.mi355_activity_cells(50, 37, 1000, 1000, C.byref(gw), C.byref(gh)) == 1 and (gw.value, gh.value) == (1, 1)

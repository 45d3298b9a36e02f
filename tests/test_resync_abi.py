"""CPU-side checks of the resynchronisation calls (mi355_state_tiles, mi355_state_digest_host, mi355_state_digest_batch,
mi355_refresh_cwire_batch, mi355_state_clear_tiles_batch): the library exports the five entry points, the header declares them,
the binding lists them with matching argument counts, the ABI version is still 10 (additions only), the device forms refuse a
null core, and the C++ drop-in has CUDACore::digest_multi, refresh_multi and clear_tiles_multi."""
import os
import re
import subprocess

import pytest

import cudavideostream_amd as pkg
from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_state_tiles": 1, "mi355_state_digest_host": 3, "mi355_state_digest_batch": 5, "mi355_refresh_cwire_batch": 10,
         "mi355_state_clear_tiles_batch": 5}


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
    for method in ("state_digest_batch", "refresh_cwire_batch", "state_clear_tiles_batch"):
        assert callable(getattr(CUDACore, method))
    assert callable(pkg.state_tiles) and callable(pkg.state_digest_host)


def test_header_has_the_section():
    text = open(HEADER).read()
    assert "Resynchronising a receiver" in text
    assert "not cryptographic" in text.lower()


def test_abi_version_is_still_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_state_tiles(built):
    assert [pkg.state_tiles(v) for v in (0, 1, 693, 4095, 4096, 4097, 9216, 131328, 1080000)] == [0, 1, 1, 1, 1, 2, 3, 33, 264]


def test_device_forms_refuse_without_a_core(built):
    calls = [
        lambda n: built.mi355_state_digest_batch(None, None, 0, n, None),
        lambda n: built.mi355_refresh_cwire_batch(None, None, 0, n, None, None, None, None, None, 0),
        lambda n: built.mi355_state_clear_tiles_batch(None, None, 0, n, None),
    ]
    for call in calls:
        assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
        assert b"core" not in built.mi355_last_error()
        assert call(1) == lib.ERR_INVALID
        assert b"core" in built.mi355_last_error()
        assert call(0) == lib.ERR_INVALID


def test_drop_in_methods_compile_and_link(built, tmp_path):
    """diff::cuda::CUDACore::digest_multi, refresh_multi and clear_tiles_multi are declared in the drop-in's header and defined in
    libmi355compat.a (a program that only takes their addresses: nothing runs, no device is needed); the object keeps the
    reference's 160 bytes."""
    compat = os.path.join(ROOT, "cudavideostream_amd", "compat")
    subprocess.run(["make", "-C", compat, "-s"], check=True)
    src = tmp_path / "link_resync.cpp"
    src.write_text('#include "kernels.cuh"\n'
                   "using diff::cuda::CUDACore;\n"
                   "typedef void (CUDACore::*fn_digest)(const void *, size_t, int, void *);\n"
                   "typedef void (CUDACore::*fn_refresh)(const void *, size_t, int, const void *, void *, void *, void *, void *,"
                   " size_t);\n"
                   "typedef void (CUDACore::*fn_clear)(void *, size_t, int, const void *);\n"
                   'static_assert(sizeof(CUDACore) == 160, "object size");\n'
                   "int main() {\n"
                   "    volatile fn_digest a = &CUDACore::digest_multi;\n"
                   "    volatile fn_refresh b = &CUDACore::refresh_multi;\n"
                   "    volatile fn_clear c = &CUDACore::clear_tiles_multi;\n"
                   "    return a && b && c ? 0 : 1;\n"
                   "}\n")
    exe = tmp_path / "link_resync"
    libd = os.path.join(ROOT, "cudavideostream_amd")
    subprocess.run(["g++", "-std=c++11", "-I", os.path.join(compat, "include"), "-o", str(exe), str(src),
                    os.path.join(compat, "libmi355compat.a"), "-L", libd, "-lmi355diff", f"-Wl,-rpath,{libd}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0

"""CPU-side checks of the despeckle call (mi355_cwire_despeckle_host, mi355_cwire_despeckle_cwire_batch): the library exports the
two entry points, the header declares them, the binding lists them with matching argument counts (15 and 13), the ABI version
is still 10 (additions only), MI355_PREPARE_DESPECKLE is 64 beside an unchanged MI355_PREPARE_ALL of 31, the batch call
refuses a null core, and the C++ drop-in has CUDACore::despeckle_multi in an object of 160 bytes."""
import os
import re
import subprocess

import pytest

import cudavideostream_amd
from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_cwire_despeckle_host": 15, "mi355_cwire_despeckle_cwire_batch": 13}


@pytest.fixture(scope="module")
def built():
    lib.build()
    return lib.load()


def declared_args(name):
    """Number of arguments of `name`'s prototype in the header."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/mi355diff.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(NAMES))
def test_symbol_is_exported_declared_and_bound(built, name):
    assert hasattr(built, name), f"{name} is not exported by the built library"
    assert name in lib.SYMBOLS
    assert declared_args(name) == len(lib.SYMBOLS[name][1]) == NAMES[name]
    assert callable(getattr(CUDACore, "cwire_despeckle_cwire_batch")) and callable(cudavideostream_amd.cwire_despeckle_host)


def test_abi_version_is_still_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_prepare_bits(built):
    text = open(HEADER).read()
    assert re.search(r"#define MI355_PREPARE_DESPECKLE 64u\b", text) and re.search(r"#define MI355_PREPARE_ALL 31u\b", text)
    assert lib.PREPARE_DESPECKLE == 64 and lib.PREPARE_ALL == 31 and lib.PREPARE_EXEC_CWIRE == 32


def test_refuse_without_a_core(built):
    args = (None, None, None, None, None, 0, 1, None, None, None, None, None, 0)
    assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
    assert b"core" not in built.mi355_last_error()
    assert built.mi355_cwire_despeckle_cwire_batch(*args) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()


def test_drop_in_despeckle_multi_compiles_and_links(built, tmp_path):
    """diff::cuda::CUDACore::despeckle_multi is declared in the drop-in's header and defined in libmi355compat.a (a program that
    only takes its address: nothing runs, no device is needed); the object keeps the reference's 160 bytes."""
    compat = os.path.join(ROOT, "cudavideostream_amd", "compat")
    subprocess.run(["make", "-C", compat, "-s"], check=True)
    src = tmp_path / "link_despeckle_multi.cpp"
    src.write_text('#include "kernels.cuh"\n'
                   "typedef void (diff::cuda::CUDACore::*fn)(const void *, const uint32_t *, const uint32_t *, void *, size_t, int, "
                   "const uint32_t *, void *, void *, void *, void *, size_t);\n"
                   'static_assert(sizeof(diff::cuda::CUDACore) == 160, "object size");\n'
                   "int main() { volatile fn f = &diff::cuda::CUDACore::despeckle_multi; return f ? 0 : 1; }\n")
    exe = tmp_path / "link_despeckle_multi"
    libd = os.path.join(ROOT, "cudavideostream_amd")
    subprocess.run(["g++", "-std=c++11", "-I", os.path.join(compat, "include"), "-o", str(exe), str(src),
                    os.path.join(compat, "libmi355compat.a"), "-L", libd, "-lmi355diff", f"-Wl,-rpath,{libd}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0

"""CPU-side checks of the record check (mi355_cwire_check_host, mi355_cwire_check_batch): the library exports both entry points,
the header declares them and the five MI355_CWIRE_BAD_* flags, the binding lists them with matching argument counts, the ABI
version is still 10 (additions only), the device form refuses a null core, and the C++ drop-in has CUDACore::check_multi."""
import os
import re
import subprocess

import pytest

import cudavideostream_amd as pkg
from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_cwire_check_host": 7, "mi355_cwire_check_batch": 6}
FLAGS = {"CODES": 1, "RANGE": 2, "PAD": 4, "ESCAPE": 8, "HEADER": 16}


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
    assert callable(CUDACore.cwire_check_batch) and callable(pkg.cwire_check_host)


def test_flags_are_declared_and_exported():
    text = open(HEADER).read()
    for name, value in FLAGS.items():
        m = re.search(r"#define MI355_CWIRE_BAD_%s\s+(\d+)u" % name, text)
        assert m and int(m.group(1)) == value, name
        assert getattr(pkg, "CWIRE_BAD_" + name) == getattr(lib, "CWIRE_BAD_" + name) == value


def test_abi_version_is_still_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_device_form_refuses_without_a_core(built):
    assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
    assert b"core" not in built.mi355_last_error()
    assert built.mi355_cwire_check_batch(None, None, None, None, 1, None) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()
    assert built.mi355_cwire_check_batch(None, None, None, None, 0, None) == lib.ERR_INVALID


def test_drop_in_check_multi_compiles_and_links(built, tmp_path):
    """diff::cuda::CUDACore::check_multi is declared in the drop-in's header and defined in libmi355compat.a (a program that
    only takes its address: nothing runs, no device is needed); the object keeps the reference's 160 bytes."""
    compat = os.path.join(ROOT, "cudavideostream_amd", "compat")
    subprocess.run(["make", "-C", compat, "-s"], check=True)
    src = tmp_path / "link_check_multi.cpp"
    src.write_text('#include "kernels.cuh"\n'
                   "typedef void (diff::cuda::CUDACore::*fn)(const void *, const uint32_t *, const uint32_t *, int, void *);\n"
                   'static_assert(sizeof(diff::cuda::CUDACore) == 160, "object size");\n'
                   "int main() { volatile fn f = &diff::cuda::CUDACore::check_multi; return f ? 0 : 1; }\n")
    exe = tmp_path / "link_check_multi"
    libd = os.path.join(ROOT, "cudavideostream_amd")
    subprocess.run(["g++", "-std=c++11", "-I", os.path.join(compat, "include"), "-o", str(exe), str(src),
                    os.path.join(compat, "libmi355compat.a"), "-L", libd, "-lmi355diff", f"-Wl,-rpath,{libd}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0

"""CPU-side checks of the tick budget (mi355_cwire_budget_cwire_batch, mi355_cwire_budget_entries): the library exports the two
entry points, the header declares them, the binding lists them with matching argument counts, the ABI version is still 10
(additions only), the batch call refuses a null core, the C++ drop-in has CUDACore::budget_multi, and the host-only
mi355_cwire_budget_entries agrees with a brute-force loop over the record size."""
import os
import re
import subprocess

import pytest

from cudavideostream_amd import CUDACore, cwire_budget_entries, cwire_frame_bytes, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_cwire_budget_cwire_batch": 13, "mi355_cwire_budget_entries": 2}


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
    assert callable(getattr(CUDACore, "cwire_budget_cwire_batch")) and callable(cwire_budget_entries)


def test_abi_version_is_still_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_refuse_without_a_core(built):
    args = (None, None, None, None, None, 0, 1, None, None, None, None, None, 0)
    assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
    assert b"core" not in built.mi355_last_error()
    assert built.mi355_cwire_budget_cwire_batch(*args) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()


def test_drop_in_budget_multi_compiles_and_links(built, tmp_path):
    """diff::cuda::CUDACore::budget_multi is declared in the drop-in's header and defined in libmi355compat.a (a program that
    only takes its address: nothing runs, no device is needed); the object keeps the reference's 160 bytes."""
    compat = os.path.join(ROOT, "cudavideostream_amd", "compat")
    subprocess.run(["make", "-C", compat, "-s"], check=True)
    src = tmp_path / "link_budget_multi.cpp"
    src.write_text('#include "kernels.cuh"\n'
                   "typedef void (diff::cuda::CUDACore::*fn)(const void *, const uint32_t *, const uint32_t *, void *, size_t, int, "
                   "const uint32_t *, void *, void *, void *, void *, size_t);\n"
                   'static_assert(sizeof(diff::cuda::CUDACore) == 160, "object size");\n'
                   "int main() { volatile fn f = &diff::cuda::CUDACore::budget_multi; return f ? 0 : 1; }\n")
    exe = tmp_path / "link_budget_multi"
    libd = os.path.join(ROOT, "cudavideostream_amd")
    subprocess.run(["g++", "-std=c++11", "-I", os.path.join(compat, "include"), "-o", str(exe), str(src),
                    os.path.join(compat, "libmi355compat.a"), "-L", libd, "-lmi355diff", f"-Wl,-rpath,{libd}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


# ---- mi355_cwire_budget_entries -------------------------------------------------------------------------------------------
def pad4(n):
    return (n + 3) & ~3


def worst(n, N):
    """Bytes of the largest record of n entries of a frame of N bytes."""
    return 8 + 2 * pad4(n) + 4 * min(n, N // 256)


def brute(N, nbytes):
    """The largest n <= N whose worst record fits, by walking up (the size rises with n); 0 below a header."""
    if nbytes < 8:
        return 0
    if worst(N, N) <= nbytes:              # (everything fits: no walk over six million counts)
        return N
    n = 0
    while n < N and worst(n + 1, N) <= nbytes:
        n += 1
    return n


FRAMES = [45, 1221, 9216, 6220800]


def byte_budgets(N):
    return [0, 7, 8, 9, 15, 16, worst(N, N), worst(N, N) + 1]


@pytest.mark.parametrize("N", FRAMES)
def test_budget_entries_against_brute_force(built, N):
    for nbytes in byte_budgets(N):
        assert cwire_budget_entries(N, nbytes) == brute(N, nbytes), (N, nbytes)
    assert cwire_budget_entries(N, worst(N, N)) == N and cwire_budget_entries(N, worst(N, N) - 1) < N


@pytest.mark.parametrize("N", FRAMES)
def test_budget_entries_is_tight(built, N):
    """A record of the returned n entries fits with as many escapes as the frame allows; one of n + 1 does not, unless n == N."""
    for nbytes in byte_budgets(N) + [600, 4096, 100000]:
        n = cwire_budget_entries(N, nbytes)
        assert 0 <= n <= N
        if nbytes >= 8:
            assert cwire_frame_bytes(n, min(n, N // 256)) <= nbytes, (N, nbytes, n)
        else:
            assert n == 0
        if n < N:
            assert cwire_frame_bytes(n + 1, min(n + 1, N // 256)) > nbytes, (N, nbytes, n)

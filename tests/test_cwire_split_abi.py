"""CPU-side checks of the split calls (mi355_cwire_split_host / _cwire_batch and the two capacity helpers): the library exports
the entry points, the header declares them, the binding lists them with matching argument counts, the ABI version is still 10
(additions only), the block constant matches the header, and the device form refuses what needs no device to refuse."""
import os
import re

import numpy as np
import pytest

import cudavideostream_amd
from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_cwire_split_host": 12, "mi355_cwire_split_cwire_batch": 11, "mi355_cwire_split_pieces_max": 3,
         "mi355_cwire_split_bytes_max": 3}


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


def test_python_surface():
    assert callable(CUDACore.cwire_split_cwire_batch)
    for name in ("cwire_split_host", "cwire_split_pieces_max", "cwire_split_bytes_max"):
        assert callable(getattr(cudavideostream_amd, name))


def test_block_constant_matches_the_header():
    m = re.search(r"#define MI355_CWIRE_SPLIT_BLOCK (\d+)u", open(HEADER).read())
    assert m and int(m.group(1)) == lib.CWIRE_SPLIT_BLOCK == 65536


def test_abi_version_is_still_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_device_form_refuses_without_a_core(built):
    args = (None, None, None, None, 1, 64, None, None, 0, None, 0)
    assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
    assert b"core" not in built.mi355_last_error()
    assert built.mi355_cwire_split_cwire_batch(*args) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()


def test_helpers_need_no_device(built):
    # ceil(n / 65536) + floor((2*pad4(n) + 4e) / (M - 35)); record bytes + 12 per piece
    assert built.mi355_cwire_split_pieces_max(0, 0, 1400) == 0
    assert built.mi355_cwire_split_pieces_max(1, 0, 64) == 1
    assert built.mi355_cwire_split_pieces_max(65537, 10, 1400) == 2 + (2 * 65540 + 40) // 1365
    assert built.mi355_cwire_split_bytes_max(65537, 10, 1400) == 8 + 2 * 65540 + 40 + 12 * (2 + (2 * 65540 + 40) // 1365)
    for bad in (0, 63, 65537, 1 << 40):
        assert built.mi355_cwire_split_pieces_max(100, 1, bad) == 0 and built.mi355_cwire_split_bytes_max(100, 1, bad) == 0


def test_host_form_refuses_bad_limits(built):
    first, pos, out = np.zeros(2, np.uint32), np.zeros(2, np.uint64), np.zeros(64, np.uint8)
    rec = np.zeros(8, np.uint8)
    zero = np.zeros(1, np.uint32)
    for bad in (0, 60, 62, 65540):
        rc = built.mi355_cwire_split_host(100, rec.ctypes.data, 8, zero.ctypes.data, zero.ctypes.data, 1, bad, first.ctypes.data,
                                          pos.ctypes.data, 1, out.ctypes.data, 64)
        assert rc == lib.ERR_INVALID and b"max_bytes" in built.mi355_last_error()
    rc = built.mi355_cwire_split_host(100, rec.ctypes.data, 8, zero.ctypes.data, zero.ctypes.data, 1, 64, first.ctypes.data,
                                      pos.ctypes.data, 1, out.ctypes.data, 64)
    assert rc == lib.OK and list(first) == [0, 0] and int(pos[0]) == 0

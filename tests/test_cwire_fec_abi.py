"""CPU-side checks of the parity calls (mi355_cwire_fec_*): the library exports the entry points, the header declares them, the
binding lists them with matching argument counts, the ABI version is still 10 and the history names the addition, the constants
match the header, both device forms refuse a null core, the host form refuses what the device form refuses (shape, null
pointers, overlapping regions) with its outputs untouched, nrecords == 0 writes fec_first[0] only, and the capacity helper.  The
refusals of the device forms that need a core are in tests/test_cwire_fec_gpu.py."""
import os
import re

import numpy as np
import pytest

import cudavideostream_amd
from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_cwire_fec_groups_max": 3, "mi355_cwire_fec_host": 14, "mi355_cwire_fec_batch": 15, "mi355_cwire_fec_repair_host": 9,
         "mi355_cwire_fec_repair_batch": 12}
FILL = 0x5C


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
    assert callable(CUDACore.cwire_fec_batch) and callable(CUDACore.cwire_fec_repair_batch)
    for name in ("cwire_fec_host", "cwire_fec_repair_host", "cwire_fec_groups_max"):
        assert callable(getattr(cudavideostream_amd, name))


def test_constants_match_the_header():
    text = open(HEADER).read()
    assert int(re.search(r"#define MI355_FEC_BAD_HEADER (\d+)u", text).group(1)) == lib.FEC_BAD_HEADER == 1
    assert int(re.search(r"#define MI355_FEC_BAD_TAIL (\d+)u", text).group(1)) == lib.FEC_BAD_TAIL == 2
    assert re.search(r"#define MI355_FEC_ABSENT UINT64_MAX", text) and lib.FEC_ABSENT == 2 ** 64 - 1


def test_abi_version_is_still_10_and_the_history_names_the_addition(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    text = open(HEADER).read()
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", text)
    assert m and int(m.group(1)) == 10
    history = text[text.index("ABI version of this header"):m.start()]
    assert "+ mi355_cwire_fec_* (additions only)" in history


def test_device_forms_refuse_without_a_core(built):
    assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
    assert b"core" not in built.mi355_last_error()
    assert built.mi355_cwire_fec_batch(None, None, 0, None, None, 0, 1, 8, 2, 1400, None, None, 0, None, 0) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()
    built.mi355_cwire_apply_host(None, 0, None, 0, 0, None)
    assert built.mi355_cwire_fec_repair_batch(None, None, 0, 1, None, None, None, None, None, None, 64, None) == lib.ERR_INVALID
    assert b"core" in built.mi355_last_error()


def test_groups_max_needs_no_device(built):
    assert built.mi355_cwire_fec_groups_max(201, 1, 8) == 26
    assert built.mi355_cwire_fec_groups_max(0, 0, 255) == 0 and built.mi355_cwire_fec_groups_max(0, 5, 1) == 5
    assert [built.mi355_cwire_fec_groups_max(100, 2, G) for G in (0, 256, -3)] == [0, 0, 0]
    assert built.mi355_cwire_fec_groups_max(100, -1, 8) == 0


class Buffers:
    """Two pieces of 64 and 32 bytes of one record, and outputs that start as FILL."""

    def __init__(self):
        self.pieces = np.arange(96, dtype=np.uint8)
        self.first = np.array([0, 2], np.uint32)
        self.pos = np.array([0, 64, 96], np.uint64)
        self.ff = np.full(2, FILL * 0x01010101, np.uint32)
        self.fl = np.full(4, FILL * 0x01010101, np.uint32)
        self.out = np.full(1024, FILL, np.uint8)

    def args(self, **kw):
        p = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data
        d = dict(pieces=self.pieces, pieces_bytes=96, piece_first=self.first, piece_pos=self.pos, piece_capacity=2, nrecords=1, group=2,
                 nparity=2, pitch=64, fec_first=self.ff, fec_len=self.fl, group_capacity=4, out=self.out, capacity_bytes=1024)
        d.update(kw)
        return [p(v) for v in d.values()]

    def untouched(self):
        return (self.ff == FILL * 0x01010101).all() and (self.fl == FILL * 0x01010101).all() and (self.out == FILL).all()


def test_host_form_refusals_leave_the_outputs_untouched(built):
    b = Buffers()
    bad = [dict(nrecords=-1), dict(group=0), dict(group=256), dict(nparity=0), dict(nparity=3), dict(pitch=60), dict(pitch=66),
           dict(pitch=65540), dict(pieces=None), dict(piece_first=None), dict(piece_pos=None), dict(fec_first=None), dict(fec_len=None),
           dict(out=None),
           dict(out=b.pieces.ctypes.data + 32, capacity_bytes=32),    # the parity blocks inside the pieces,
           dict(fec_len=b.first.ctypes.data + 4, group_capacity=1),   # fec_len on piece_first,
           dict(fec_first=b.pos.ctypes.data + 8),                     # fec_first on piece_pos,
           dict(fec_len=b.out.ctypes.data + 512, group_capacity=4),   # and two outputs on each other
           dict(fec_first=b.fl.ctypes.data + 8)]
    for kw in bad:
        assert built.mi355_cwire_fec_host(*b.args(**kw)) == lib.ERR_INVALID, kw
        assert b.untouched(), kw
    assert built.mi355_cwire_fec_host(*b.args()) == lib.OK
    assert list(b.ff) == [0, 1] and int(b.fl[0]) == 64 and (b.fl[1:] == FILL * 0x01010101).all()
    assert np.array_equal(b.out[:32], b.pieces[:32] ^ b.pieces[64:]) and np.array_equal(b.out[32:64], b.pieces[32:64])
    assert (b.out[128:] == FILL).all()


def test_no_records_writes_fec_first_0_only(built):
    b = Buffers()
    assert built.mi355_cwire_fec_host(*b.args(nrecords=0)) == lib.OK
    assert int(b.ff[0]) == 0 and int(b.ff[1]) == FILL * 0x01010101 and (b.fl == FILL * 0x01010101).all() and (b.out == FILL).all()

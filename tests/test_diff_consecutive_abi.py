"""CPU-side checks of mi355_diff_consecutive_batch (consecutive frames, the predecessor kept in registers): the header
declares it, the built library exports it, the binding lists it with nine arguments, and the ABI version is still 10
(an addition only) with the call named in the header's version history."""
import os
import re
import subprocess

import pytest

from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAME = "mi355_diff_consecutive_batch"


@pytest.fixture(scope="module")
def built():
    lib.build()
    return lib.load()


def test_header_declares_the_call_with_nine_arguments():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in include/mi355diff.h"
    args = [a.strip() for a in m.group(1).split(",") if a.strip()]
    assert len(args) == 9
    # the order: core, the first frame's predecessor, the frames, the step between frames, count, the three outputs, capacity
    assert [re.sub(r".*?(\w+)$", r"\1", a) for a in args] == ["core", "d_first_prev", "d_frames", "frame_step_bytes", "nframes",
                                                              "d_offsets", "d_xs", "d_diff", "capacity"]


def test_library_exports_the_call(built):
    assert hasattr(built, NAME), f"{NAME} is not exported by the built library"
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in {l.split()[-1] for l in out.splitlines() if " T " in l}   # unmangled extern "C"


def test_binding_lists_nine_arguments():
    assert NAME in lib.SYMBOLS
    restype, argtypes = lib.SYMBOLS[NAME]
    assert len(argtypes) == 9 and argtypes == lib.SYMBOLS["mi355_diff_pairs_batch"][1]   # the pair form's types, reordered alike
    assert hasattr(CUDACore, "diff_consecutive_batch")


def test_abi_version_is_still_10_and_the_history_names_the_call(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    text = open(HEADER).read()
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", text)
    assert m and int(m.group(1)) == 10
    history = text[text.index("ABI version of this header"):m.start()]
    assert NAME in history


def test_refused_without_a_core(built):
    assert getattr(built, NAME)(None, None, None, 0, 1, None, None, None, 0) == lib.ERR_INVALID
    assert built.mi355_last_error()

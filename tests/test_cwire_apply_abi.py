"""CPU-side checks of mi355_apply_cwire_batch (ABI 10): the library exports it, the binding knows its prototype, and the
library, the header and the binding agree on the ABI version."""
import os
import re

import pytest

from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")


@pytest.fixture(scope="module")
def built():
    lib.build()
    return lib.load()


def test_apply_cwire_batch_is_exported(built):
    assert hasattr(built, "mi355_apply_cwire_batch")
    assert "mi355_apply_cwire_batch" in lib.SYMBOLS
    assert hasattr(CUDACore, "apply_cwire_batch")


def test_abi_version_is_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_refuses_without_a_core(built):
    assert built.mi355_apply_cwire_batch(None, None, None, None, 1, None, 0) == lib.ERR_INVALID

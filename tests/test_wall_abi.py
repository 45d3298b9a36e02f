"""CPU-side checks of the wall calls (mi355_wall_thumb_size, mi355_wall_compose_batch, mi355_cwire_touched_tiles_batch): the
library exports the three entry points, the header declares them, the binding lists them with matching argument counts, the ABI
version is still 10 (additions only), the device forms refuse a null core, the host form gives the thumbnail sizes, and the C++
drop-in has CUDACore::wall_compose_multi and touched_tiles_multi."""
import os
import re
import subprocess

import numpy as np
import pytest

import cudavideostream_amd as pkg
import wall_spec as ws
from cudavideostream_amd import CUDACore, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355diff.h")
NAMES = {"mi355_wall_thumb_size": 5, "mi355_wall_compose_batch": 10, "mi355_cwire_touched_tiles_batch": 8}


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
    for method in ("wall_compose_batch", "cwire_touched_tiles_batch"):
        assert callable(getattr(CUDACore, method))
    assert callable(pkg.wall_thumb_size)


def test_header_has_the_section():
    text = open(HEADER).read()
    assert "A wall of many cameras" in text
    assert "floor((sum of the block's channel-c bytes + floor(a / 2)) / a)" in text


def test_abi_version_is_still_10(built):
    assert lib.ABI_VERSION == built.mi355_abi_version() == 10
    m = re.search(r"#define MI355_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_thumb_size(built):
    assert pkg.wall_thumb_size(7, 5, 16) == (1, 1, 1)
    assert pkg.wall_thumb_size(33, 7, 3) == (33, 11, 3)
    assert pkg.wall_thumb_size(64, 48, 5) == (130, 13, 10)
    assert pkg.wall_thumb_size(1920, 1080, 1) == (1920 * 1080, 1920, 1080)
    for w, h, k in [(7, 5, 16), (33, 7, 3), (64, 48, 5), (256, 171, 2), (1, 1, 16)]:       # ... and the numpy statement agrees
        assert pkg.wall_thumb_size(w, h, k)[1:] == ws.thumb_size(w, h, k)
    for bad in [(0, 5, 1), (5, 0, 1), (-1, 5, 2), (5, 5, 0), (5, 5, 17), (5, 5, -1)]:
        assert pkg.wall_thumb_size(*bad) == (0, 0, 0)
    assert built.mi355_wall_thumb_size(33, 7, 3, None, None) == 33                          # null pointers are skipped


def test_spec_thumbnail_is_the_stated_block_average():
    """wall_spec.thumbnail against the definition written as plain loops."""
    rng = np.random.default_rng(5)
    for w, h, k in [(7, 5, 2), (7, 5, 3), (7, 5, 16), (9, 4, 1), (8, 8, 4)]:
        st = rng.integers(0, 256, 3 * w * h, dtype=np.uint8)
        img = st.reshape(h, w, 3).astype(int)
        tw, th = ws.thumb_size(w, h, k)
        want = np.zeros((th, tw, 3), np.uint8)
        for v in range(th):
            for u in range(tw):
                blk = img[v * k:min(h, (v + 1) * k), u * k:min(w, (u + 1) * k)]
                a = blk.shape[0] * blk.shape[1]
                for c in range(3):
                    want[v, u, c] = (int(blk[:, :, c].sum()) + a // 2) // a
        assert np.array_equal(ws.thumbnail(st, w, h, k), want)


def test_device_forms_refuse_without_a_core(built):
    calls = [
        lambda n: built.mi355_wall_compose_batch(None, None, 0, n, None, None, None, 1, 1, 3),
        lambda n: built.mi355_cwire_touched_tiles_batch(None, None, None, None, n, n, 0, None),
    ]
    for call in calls:
        assert built.mi355_cwire_apply_host(None, 0, None, 0, 0, None) == lib.ERR_INVALID   # (another text in the slot first)
        assert b"core" not in built.mi355_last_error()
        assert call(1) == lib.ERR_INVALID
        assert b"core" in built.mi355_last_error()
        assert call(0) == lib.ERR_INVALID


def test_drop_in_methods_compile_and_link(built, tmp_path):
    """diff::cuda::CUDACore::wall_compose_multi and touched_tiles_multi are declared in the drop-in's header and defined in
    libmi355compat.a (a program that only takes their addresses: nothing runs, no device is needed); the object keeps the
    reference's 160 bytes."""
    compat = os.path.join(ROOT, "cudavideostream_amd", "compat")
    subprocess.run(["make", "-C", compat, "-s"], check=True)
    src = tmp_path / "link_wall.cpp"
    src.write_text('#include "kernels.cuh"\n'
                   "using diff::cuda::CUDACore;\n"
                   "typedef void (CUDACore::*fn_compose)(const void *, size_t, int, const int32_t *, const void *, void *, int, int,"
                   " size_t);\n"
                   "typedef void (CUDACore::*fn_touched)(const void *, const uint32_t *, const uint32_t *, int, int, bool, void *);\n"
                   'static_assert(sizeof(CUDACore) == 160, "object size");\n'
                   "int main() {\n"
                   "    volatile fn_compose a = &CUDACore::wall_compose_multi;\n"
                   "    volatile fn_touched b = &CUDACore::touched_tiles_multi;\n"
                   "    return a && b ? 0 : 1;\n"
                   "}\n")
    exe = tmp_path / "link_wall"
    libd = os.path.join(ROOT, "cudavideostream_amd")
    subprocess.run(["g++", "-std=c++11", "-I", os.path.join(compat, "include"), "-o", str(exe), str(src),
                    os.path.join(compat, "libmi355compat.a"), "-L", libd, "-lmi355diff", f"-Wl,-rpath,{libd}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0

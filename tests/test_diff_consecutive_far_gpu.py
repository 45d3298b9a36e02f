"""-m gpu: mi355_diff_consecutive_batch on frames that lie up to and past 4 GiB apart -- the layouts, inputs, guarded far
regions and the comparison of tests/test_far_strides_gpu.py, which runs every other call that goes through run_batch the
same way.  The call shares the stream form's register groups of four frames (one descriptor per group, voff = d * step), so
the window's edge is where that form has it; what is its own is the one predecessor, which lies in a region of its own or
one step in front of the frames."""
import numpy as np
import pytest

from oracle import pyoracle as po
from gpu_util import CUDACore, oracle_pairs
from test_far_strides_gpu import (LAYOUTS, SIZES, THR, assert_rows, edge_strides, far_regions, one_stream, prefetch,
                                  run_diff)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_diff_consecutive(layout, w, h):
    """The frames of one sequence far apart, the first one's predecessor in a region of its own and as the frame one step in
    front of the frames in their region, against oracle_pairs."""
    stride, T, skew = LAYOUTS[layout]
    n = 3 * w * h
    base, line, _, _, _ = one_stream(n, T)
    with far_regions((T, n, stride, skew), (1, n, stride, skew)) as (fr, fp):
        fr.put(line)
        fp.put([base])
        with CUDACore(w, h, max_batch=T, threshold=THR) as core:
            run_diff(core, "diff_consecutive", "arrays", (fp.ptr, fr.ptr, T), stride, T,
                     oracle_pairs(po, line, np.concatenate([base[None], line[:-1]]), THR), f"{layout} {w}x{h}, a predecessor elsewhere")
            run_diff(core, "diff_consecutive", "arrays", (fr.ptr, fr.ptr + stride, T - 1), stride, T - 1,
                     oracle_pairs(po, line[1:], line[:-1], THR), f"{layout} {w}x{h}, the predecessor in front of the frames")
        assert_rows(fr.get(), line, "the frames are only read")
        assert_rows(fp.get(), base[None], "the predecessor is only read")


def test_diff_consecutive_window_edge():
    """At the largest step that still takes the pack kernel's 32-bit window and at the first that does not, 64x48, one frame
    more than a register group of the stream form (the first group's last frame is at voff = 3 * step): the reference's bytes
    on both sides."""
    w, h = 64, 48
    n = 3 * w * h
    B = prefetch()[0] + 1
    base, line, _, _, _ = one_stream(n, B)
    want = oracle_pairs(po, line, np.concatenate([base[None], line[:-1]]), THR)
    got = []
    for stride in edge_strides(n):
        with far_regions((B, n, stride, 0), (1, n, stride, 0)) as (fr, fp), CUDACore(w, h, max_batch=B, threshold=THR) as core:
            fr.put(line)
            fp.put([base])
            got.append(run_diff(core, "diff_consecutive", "arrays", (fp.ptr, fr.ptr, B), stride, B, want, f"window_edge, step {stride}"))
            assert_rows(fr.get(), line, "the frames are only read")
    assert got[0] == got[1], "the two sides of the window differ"

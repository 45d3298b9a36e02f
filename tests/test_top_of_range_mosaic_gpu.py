"""-m gpu: the mosaic call at the top of the range, beside test_top_of_range_gpu.py's consumers of its 4.6 GB record buffer:
mi355_cwire_mosaic_cwire_batch on the 1100 records of 1000x700 that change every byte, (S, K) = (2, 550), record positions past
2^32 from record 1023 on.  The two streams are placed as bands, {0, 0, W, H, 0, s*H} on a 1000 x 1400 canvas, so the canvas
record is the non-zero last - initial of the streams one behind the other, with index bias s*N (law (d) of the header).
The call reads records only through the decode loop it shares with the coalescer (cwa_block_load, cwa_walk_record) and indexes
the directory in 64 bits; this is the run that shows it.  Its own kernels' grid is sized by the canvas alone; its by-value table
of 128 placements is crossed at 129 streams by test_cwire_mosaic_gpu.py."""
import numpy as np
import pytest
import torch

import cwire_spec as spec
import test_top_of_range_gpu as top
from gpu_util import Guarded
from test_top_of_range_gpu import dense_records   # noqa: F401  (the module-scoped fixture: this module's own buffer)

pytestmark = pytest.mark.gpu


def test_every_byte_mosaic(dense_records):   # noqa: F811
    r = dense_records
    S, K = top.CONSUMER_SK
    n = top.N
    top.require(top.log_bytes(r.T, 1) + (1 << 30))
    before, after = top.stream_ends(top.every_byte_base(), top.every_byte_frame, S, K)
    acc = (after - before).reshape(-1)                        # uint8: the bands' sums one behind the other
    xs = np.flatnonzero(acc)
    assert (acc == 0).any() and xs.size > n, "sums of 0 are left out; both bands hold entries"
    w_off = np.array([0, xs.size], np.uint32)
    w_recs, w_pos = spec.encode(w_off, xs.astype(np.int32), acc[xs])
    place = [(0, 0, top.BW, top.BH, 0, s * top.BH) for s in range(S)]
    off, pos, out = Guarded(2, top.I32), Guarded(2, top.I64), Guarded(w_recs.size + 64)
    with top.consumer_core() as core:
        torch.cuda.synchronize()
        core.cwire_mosaic_cwire_batch(r.ptr, r.counts, r.escapes, S, K, place, top.BW, S * top.BH, off.ptr, pos.ptr, out.ptr,
                                      w_recs.size + 64)
        core.synchronize()
    top.assert_equal(off.get().view(np.uint32), w_off, "offsets")
    top.assert_equal(pos.get().view(np.uint64), w_pos, "frame_pos")
    top.assert_equal(out.get(w_recs.size)[:w_recs.size], w_recs, "the record", w_pos)
    r.check()

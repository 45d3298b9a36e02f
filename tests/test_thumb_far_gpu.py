"""-m gpu: mi355_thumb_cwire_batch with its states and its held thumbnails far apart, in the layouts of test_far_strides_gpu.py
(windows 2^26 bytes apart across 2^32, aligned and on the byte paths; 2^31 + 16 bytes apart), whose regions, guards and messages
it uses: gpu_util.FarRegion keeps only the windows on the host and asserts every other byte on the device.  The reference is
thumb_spec."""
import numpy as np
import pytest
import torch

import thumb_spec as ts
import wall_spec as ws
from cudavideostream_amd import cwire_bytes_max
from gpu_util import CUDACore, Guarded
from test_far_strides_gpu import LAYOUTS, SEAM, SIZES, assert_rows, far_regions
from test_wall_gpu import mask_buffer, random_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_thumb_far(layout, w, h):
    """k = 4, with a mask of the streams around 2^32 and then without one, from states far apart against held thumbnails just as
    far apart: records, frame positions, the held thumbnails after each call; every byte between the windows of both regions
    keeps its guard."""
    spacing, S, skew = LAYOUTS[layout]
    n, k = 3 * w * h, 4
    nt = ts.thumb_bytes(w, h, k)
    src = random_states(w, h, S)
    held = np.random.default_rng(n + S).integers(0, 256, (S, nt), dtype=np.uint8)
    chosen = [s for s in SEAM if s < S and s != 0]
    sel = np.zeros((S, ws.tiles(n)), bool)
    sel[chosen] = True
    rows = np.zeros((S, ws.mask_words(n)), np.uint32)
    rows[chosen] = 0xFFFFFFFF
    mask = mask_buffer(rows)
    cap = cwire_bytes_max(nt, S)
    what = f"{layout} {w}x{h}"
    with far_regions((S, n, spacing, skew), (S, nt, spacing, skew)) as (st, th):
        st.put(src)
        th.put(held)
        with CUDACore(w, h, max_batch=S) as core:
            for d_mask, selected in ((mask, sel), (None, None)):
                off, pos, out = Guarded(S + 1, torch.int32), Guarded(S + 1, torch.int64), Guarded(cap)
                torch.cuda.synchronize()
                core.thumb_cwire_batch(st.ptr, S, k, 0, th.ptr, off.ptr, pos.ptr, out.ptr, cap,
                                       d_tile_mask=None if d_mask is None else d_mask.ptr, stride=spacing, thumb_stride=spacing)
                core.synchronize()
                want_off, want_pos, recs, held = ts.batch(src, held, w, h, k, 0, selected)
                assert np.array_equal(off.get().view(np.uint32), want_off) and np.array_equal(pos.get().view(np.uint64), want_pos), what
                end = int(want_pos[-1])
                assert out.get(written=end)[:end].tobytes() == b"".join(recs), f"{what}: the records"
                assert_rows(th.get(), held, f"{what}: the held thumbnails, {'masked' if selected is not None else 'no mask'}")
        assert_rows(st.get(), src, f"{what}: the states are only read")
    mask.get()
    assert np.array_equal(held, np.stack([ws.thumbnail(x, w, h, k).reshape(-1) for x in src]))

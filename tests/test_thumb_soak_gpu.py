"""-m gpu: the thumbnail records in unsynchronised chains, soak style.  A few dozen rounds; each draws a scale, a threshold, a
layout and a shape, then enqueues three ticks of a relay -- apply_multi_cwire_batch of records made here, touched tiles of the same
records, mi355_thumb_cwire_batch with that mask -- with no synchronisation inside the round, and compares every tick's records,
frame positions and the held thumbnails at the end with the numpy statement (thumb_spec).  The held thumbnails start within the
threshold of the first thumbnails and only this call moves them, under masks that cover every change: the invariant of law 3
holds, so the output is unique.  Bounded: small shapes, 24 rounds."""
import numpy as np
import pytest
import torch

import cwire_spec as spec
import thumb_spec as ts
import wall_spec as ws
from cudavideostream_amd import cwire_bytes_max
from gpu_util import CUDACore, Guarded, Region
from test_thumb_gpu import LAYOUTS, Out, S, assert_equals_spec, regions, thumb_call, tick

pytestmark = pytest.mark.gpu

ROUNDS, TICKS = 24, 3
GEOMETRIES = [(37, 11), (100, 60), (64, 48), (2800, 6)]


def test_soak_chain_of_ticks():
    rng = np.random.default_rng(2024)
    cores = {}
    try:
        for rnd in range(ROUNDS):
            w, h = GEOMETRIES[rnd % len(GEOMETRIES)]
            k, thr, layout = int(rng.integers(1, 17)), int(rng.choice([0, 0, 3, 20, 255])), LAYOUTS[int(rng.integers(0, 2))]
            n, nt, mw = 3 * w * h, ts.thumb_bytes(w, h, k), ws.mask_words(3 * w * h)
            if (w, h) not in cores:
                cores[(w, h)] = CUDACore(w, h, max_batch=S)
            core = cores[(w, h)]
            states = [ts.random_states(rng, S, w, h)]
            first = np.stack([ws.thumbnail(states[0][s], w, h, k).reshape(-1) for s in range(S)])
            held = np.clip(first.astype(int) + rng.integers(-thr, thr + 1, first.shape), 0, 255).astype(np.uint8)
            st, th = regions(layout, n, nt, states[0], held)
            ticks, want = [], []
            for t in range(TICKS):
                sel = rng.random((S, ws.tiles(n))) < 0.5
                nxt = tick(rng, states[-1], sel)
                recs = []
                for s in range(S):
                    xs = np.flatnonzero(states[-1][s] != nxt[s])
                    recs.append(spec.encode_frame(xs.astype(np.int32), (nxt[s][xs] - states[-1][s][xs]).astype(np.uint8)))
                buf = np.frombuffer(b"".join(recs), np.uint8).copy()
                counts, escapes = spec.headers(buf, S)
                touched = np.stack([ts.touched_sel(states[-1][s], nxt[s]) for s in range(S)])
                want.append(ts.batch(nxt, held, w, h, k, thr, touched))
                held = want[-1][3]
                ticks.append((Guarded(buf.size, data=buf), counts, escapes, Out(S, cwire_bytes_max(nt, S))))
                states.append(nxt)
            mask = Guarded(S * mw, torch.int32)
            torch.cuda.synchronize()
            for d_recs, counts, escapes, o in ticks:
                core.apply_multi_cwire_batch(d_recs.ptr, counts, escapes, S, st.ptr, stride=st.stride)
                core.cwire_touched_tiles_batch(d_recs.ptr, counts, escapes, S, 1, mask.ptr)
                thumb_call(core, k, thr, st, th, mask, o)
            core.synchronize()
            after = th.get()
            for t, (_, _, _, o) in enumerate(ticks):
                held_t = want[t][3] if t + 1 < TICKS else after   # (the thumbnails in between were never on the host)
                assert_equals_spec(o.results() + (held_t,), want[t], f"round {rnd} ({w}x{h}, k {k}, threshold {thr}, {layout[0]}), tick {t}")
            assert np.array_equal(st.get(), states[-1])
    finally:
        for core in cores.values():
            core.close()

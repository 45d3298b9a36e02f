"""The numpy statement of the thumbnail records (thumb_spec) checked against itself: laws 1, 2, 5 and 6 of include/mi355diff.h,
"Thumbnail records", at the shapes the GPU tests use, and that every shape really produces the condition it is there for.  No
library, no GPU."""
import numpy as np
import pytest

import cwire_spec as spec
import resync_spec as rs
import thumb_spec as ts
import wall_spec as ws


@pytest.mark.parametrize("w,h,k", ts.SHAPES)
def test_laws_1_and_2_without_the_invariant(w, h, k):
    rng = np.random.default_rng(w * 100 + k)
    S, n, nt = 3, 3 * w * h, ts.thumb_bytes(w, h, k)
    states, thumbs = ts.random_states(rng, S, w, h), rng.integers(0, 256, (S, nt), dtype=np.uint8)
    for thr in (0, 20):
        sel = rng.random((S, ws.tiles(n))) < 0.4
        req = np.stack([ts.required_bytes(sel[s], w, h, k) for s in range(S)])
        processed = req | (rng.random((S, nt)) < 0.3)
        for proc in (None, processed):
            _, _, recs, after = ts.batch(states, thumbs, w, h, k, thr, sel, proc)
            for s in range(S):
                assert np.array_equal(ts.apply(thumbs[s], recs[s]), after[s])                 # law 1
                ts.check_law2(states[s], thumbs[s], after[s], w, h, k, thr, sel[s])          # law 2


@pytest.mark.parametrize("w,h,k", ts.SHAPES)
def test_law_5_key_record(w, h, k):
    rng = np.random.default_rng(7)
    state = ts.random_states(rng, 1, w, h)[0]
    state[rng.random(state.size) < 0.5] = 0
    rec, after, xs, df = ts.step(state, np.zeros(ts.thumb_bytes(w, h, k), np.uint8), w, h, k, 0)
    t = ws.thumbnail(state, w, h, k).reshape(-1)
    assert np.array_equal(xs, np.flatnonzero(t)) and np.array_equal(df, t[xs]) and np.array_equal(after, t)


@pytest.mark.parametrize("w,h", [(37, 11), (100, 60)])
def test_law_6_scale_one_is_the_refresh_record(w, h):
    rng = np.random.default_rng(9)
    states = ts.random_states(rng, 3, w, h)
    states[rng.random(states.shape) < 0.7] = 0
    off, pos, recs, after = ts.batch(states, np.zeros_like(states), w, h, 1, 0)
    _, roff, rrecs, rpos = rs.refresh(states, rs.selected_tiles(states, None))
    assert np.array_equal(off, roff) and np.array_equal(pos, rpos) and b"".join(recs) == rrecs.tobytes()
    assert np.array_equal(after, states)


def test_the_shapes_produce_their_conditions():
    assert ws.tiles(3 * 37 * 11) == 1
    assert 3 * ws.thumb_size(37, 11, 4)[0] == 30 and 37 % 4 and 11 % 4        # ragged right and bottom, rows of 30 < 64 bytes
    assert ws.thumb_size(37, 11, 16) == (3, 1)
    full = np.full(3 * 64 * 48, 255, np.uint8)                                  # the 16-bit sums at their top, still 255
    assert (ws.thumbnail(full, 64, 48, 16) == 255).all() and 256 * 255 + 128 < 2 ** 32 and 16 * 255 < 2 ** 16
    assert (ws.thumbnail(ts.tie_state(64, 48, 16), 64, 48, 16) == 1).all()      # the tie rounds up
    n = 3 * 100 * 60
    assert n == 18000 and ws.tiles(n) == 5 and 3 * 1365 < 4096 <= 3 * 1365 + 2  # source pixel 1365 straddles tiles 0 and 1
    assert ts.thumb_bytes(100, 60, 2) == 4500 and ts.thumb_bytes(100, 60, 3) == 2040
    y, x = divmod(1365, 100)
    for tile in (0, 1):                                                         # ... and its block is required from both sides
        assert ws.required(ts.one_tile_masks(n)[tile], 100, 60, 2)[y // 2, x // 2]
    assert 3 * ws.thumb_size(2800, 6, 2)[0] == 4200 and ts.thumb_bytes(2800, 6, 2) == 12600


def test_the_mechanics_ticks_produce_their_records():
    ticks = {name: (a, b) for name, a, b in ts.mechanics_ticks(np.random.default_rng(3))}
    out = {}
    for name, (a, b) in ticks.items():
        held = ws.thumbnail(a, 100, 60, 2).reshape(-1)
        rec, after, xs, df = ts.step(b, held, 100, 60, 2, 0, ts.touched_sel(a, b))
        assert np.array_equal(after, ws.thumbnail(b, 100, 60, 2).reshape(-1))
        out[name] = (rec, xs, df, held)
    rec, xs, df, _ = out["far"]
    assert list(xs) == [0, 1, 2, 3000, 3001, 3002] and spec.headers(np.frombuffer(rec, np.uint8), 1)[1][0] == 1 and len(xs) % 4
    assert out["late"][1][0] == 300
    rec, xs, df, held = out["wrap"]
    assert held[xs[0]] == 250 and df[0] == 9
    assert len(out["same"][0]) == 8

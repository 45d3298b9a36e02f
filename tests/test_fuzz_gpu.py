"""-m gpu: seeded random geometries against the oracle, through the C-ABI -- sizes, batch lengths, thresholds,
frame strides, pointer alignments and change densities nobody picked by hand."""
import numpy as np
import pytest

import cwire_spec as spec
from cudavideostream_amd import CUDACore as RawCore, cwire_apply_host, lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from gpu_util import DEV, CUDACore, Guarded, Region, oracle_pairs, to_dev  # noqa: E402


def _frames(rng, base, T, density, thr, inside=None):
    """inside: a mask of the bytes that may change at all (the clustered mode of test_random_compact_and_multi)."""
    n = base.size
    out = np.empty((T, n), np.uint8)
    prev = base
    for t in range(T):
        f = prev.astype(np.int16) + (rng.integers(-min(thr, 6), min(thr, 6) + 1, n) if inside is None else 0)
        hit = rng.random(n) < density
        if inside is not None:
            hit &= inside
        f[hit] = rng.integers(0, 256, int(hit.sum()))
        out[t] = f.clip(0, 255).astype(np.uint8)
        prev = out[t]
    return out


@pytest.mark.parametrize("seed", range(24))
def test_random_streams(po, seed):
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(1, 260)), int(rng.integers(1, 48))
    if seed % 6 == 0:
        w, h = int(rng.integers(300, 700)), int(rng.integers(60, 200))     # several expander groups
    T = int(rng.integers(1, 10))
    thr = int(rng.choice([0, 1, 5, 20, 20, 20, 64, 127]))
    density = float(rng.choice([0.0, 0.002, 0.02, 0.1, 0.5, 1.0]))
    n = 3 * w * h
    pad = int(rng.choice([0, 0, 16, 5, 64]))                               # frame stride = n + pad
    skew = int(rng.choice([0, 0, 16, 1, 7]))                               # byte offset of the first frame
    base = rng.integers(0, 256, n, dtype=np.uint8)
    frames = _frames(rng, base, T, density, thr)
    off, xs, df, st = po.diff_stream(frames, base, thr)
    buf = np.zeros(skew + T * (n + pad) + 64, np.uint8)
    for t in range(T):
        buf[skew + t * (n + pad): skew + t * (n + pad) + n] = frames[t]
    d_buf = to_dev(buf)
    cap = int(off[-1]) + 3
    d_off = torch.full((T + 1,), -1, dtype=torch.int32, device=DEV)
    d_xs = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    d_df = torch.full((cap,), 0xA5, dtype=torch.uint8, device=DEV)
    with CUDACore(w, h, threshold=thr, sample_mat_data=base, max_batch=T) as core:
        core.diff_stream_batch(d_buf.data_ptr() + skew, T, d_off, d_xs, d_df, cap, stride=n + pad)
        core.synchronize()
        assert np.array_equal(d_off.cpu().numpy().view(np.uint32), off)
        tot = int(off[-1])
        assert np.array_equal(d_xs.cpu().numpy()[:tot], xs) and (d_xs.cpu().numpy()[tot:] == -7).all()
        assert np.array_equal(d_df.cpu().numpy()[:tot], df) and (d_df.cpu().numpy()[tot:] == 0xA5).all()
        assert np.array_equal(core.get_state(), st)
        # the same stream as wire bytes, then through the client
        core.set_state(base)
        want = po.wire_pack(off, xs, df)
        d_wire = torch.full((want.size + 8,), 0x5C, dtype=torch.uint8, device=DEV)
        core.diff_stream_wire_batch(d_buf.data_ptr() + skew, T, d_off, d_wire, want.size, stride=n + pad)
        core.synchronize()
        wire = d_wire.cpu().numpy()
        assert np.array_equal(wire[:want.size], want) and (wire[want.size:] == 0x5C).all()
    with CUDACore(w, h, sample_mat_data=base, max_batch=T) as client:
        client.apply_wire_batch(d_wire, np.diff(off.astype(np.int64)).astype(np.uint32), T)
        client.synchronize()
        assert np.array_equal(client.get_state(), st)


@pytest.mark.parametrize("seed", range(12))
def test_random_filters(po, seed):
    rng = np.random.default_rng(2000 + seed)
    w, h = int(rng.integers(1, 200)), int(rng.integers(1, 40))
    if seed % 4 == 0:
        w = 16 * int(rng.integers(1, 24))                                   # 16-byte rows: the vector paths
    elif seed % 4 == 2:
        w, h = 8 * int(rng.integers(1, 48)), int(rng.integers(1, 90))       # 8-byte rows: the median's column strips, several bands
    n = 3 * w * h
    cur = rng.integers(0, 256, n, dtype=np.uint8)
    prev = np.where(rng.random(n) < 0.7, cur, rng.integers(0, 256, n)).astype(np.uint8)
    k = rng.random(9).astype(np.float32)
    k = (k / k.sum()).astype(np.float32)
    if seed % 2:
        k = po.gaussian_kernel(3, float(rng.uniform(0.6, 2.5)))
    with CUDACore(w, h, k=k) as core:
        d_cur, d_prev = to_dev(cur), to_dev(prev)

        def run(fn, *args):
            d_o = torch.full((n + 16,), 0x3C, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize()    # the fill runs on torch's stream, the core on its own
            fn(*args, d_o)
            core.synchronize()
            got = d_o.cpu().numpy()
            assert (got[n:] == 0x3C).all()
            return got[:n]

        assert np.array_equal(run(core.gray_avg, d_cur), po.gray_avg(cur))
        gw = po.gray_weighted(cur)
        assert np.array_equal(run(core.gray_weighted, d_cur), gw)
        assert np.array_equal(run(core.heat_map, d_cur, d_prev), po.heat_map(cur, prev))
        assert np.array_equal(run(core.red_dense, d_cur, d_prev), po.red_dense(cur, prev))
        assert np.array_equal(run(core.conv3x3, d_cur), po.conv3x3(cur, w, h, k))
        assert np.array_equal(run(core.median5x5, d_cur), po.median5x5(cur, w, h))
        thr = po.two_max_threshold(po.histogram(gw))
        assert np.array_equal(run(core.binarize_chain, to_dev(gw)), po.binarize(gw, thr))
        d_o = torch.zeros((1, n), dtype=torch.uint8, device=DEV)
        core.filter_batch(lib.OP_GRAY_WEIGHTED_BINARIZE, d_cur, d_o, 1)
        core.synchronize()
        assert np.array_equal(d_o.cpu().numpy()[0], po.binarize(gw, thr))


# ---- the compact wire format, the GPU clients and the many-streams forms --------------------------------------------------
_COUNTS = list(range(1, 10)) + [63, 64, 65, 66, 127, 128, 129, 130]   # either side of a wave, a decode launch, a table launch


def _near_a_seam(rng, nmax):
    """(w, h) with 3 w h within 3 bytes of a multiple of 16, of the pack tile (1024), of kCwaTile / kCwaChunk (4096), of an
    expander item (16384) or of 64 tiles (65536: the pipelined pack is split into two launches)."""
    while True:
        m = int(rng.choice([16, 1024, 4096, 16384, 65536]))
        if m > nmax:
            continue
        near = int(rng.integers(1, nmax // m + 1)) * m + rng.permutation(np.arange(-3, 4))
        target = int(near[near % 3 == 0][0])
        p = target // 3
        h = int(rng.choice([d for d in range(1, 49) if p % d == 0]))
        return p // h, h


def _host_client(state, recs, T):
    st, out, at = state.copy(), [], 0
    for _ in range(T):
        at += cwire_apply_host(st, recs[at:], 1)
        out.append(st.copy())
    return np.stack(out), st


@pytest.mark.parametrize("seed", range(24))
def test_random_compact_and_multi(po, seed):
    """One chain per seed through the entry points behind the arrays and sender's-wire forms, every link against the oracle,
    the numpy statement of the compact format, the host client and `state[xs] += diff`; every output in a guarded buffer.
    On the caller's stream nothing synchronises between the links -- one torch synchronisation before the read-back."""
    rng = np.random.default_rng(3000 + seed)
    T, S = int(rng.choice(_COUNTS)), int(rng.choice(_COUNTS))
    nmax = min(200_000, (12 << 20) // max(T, S))      # (host time of the references: T N bytes stay below 12 MiB)
    if rng.random() < 2 / 3:
        w, h = _near_a_seam(rng, nmax)
    else:
        w, h = int(rng.integers(1, 260)), int(rng.integers(1, 48))
    thr = int(rng.choice([0, 1, 5, 20, 20, 20, 64, 127]))
    density = float(rng.choice([0.0, 0.002, 0.02, 0.1, 0.5, 1.0]))
    n = 3 * w * h
    pad = int(rng.choice([0, 0, 16, 5, 64]))
    skew = int(rng.choice([0, 0, 16, 1, 7]))
    inside = None
    if rng.random() < 0.4:                            # clustered: untouched 4096-byte tiles beside touched ones
        inside = np.zeros(n, bool)
        for tile in rng.integers(0, (n + 4095) // 4096, int(rng.integers(1, 3))):
            inside[4096 * int(tile):4096 * int(tile) + 4096] = True
    schedule = int(rng.integers(0, 3))                # 0 own stream, 1 own stream and OPT_PIPELINE 0, 2 the caller's stream
    stride = n + pad
    base = rng.integers(0, 256, n, dtype=np.uint8)
    frames = _frames(rng, base, T, density, thr, inside)

    # the references
    off, xs, df, st = po.diff_stream(frames, base, thr)
    tot = int(off[T])
    recs, pos = spec.encode(off, xs, df)
    counts, escapes = spec.headers(recs, T)
    d_off, d_xs, d_df = spec.decode(recs, T)
    assert np.array_equal(d_off, off) and np.array_equal(d_xs, xs) and np.array_equal(d_df, df)
    shown, shown_state = _host_client(base, recs, T)
    assert np.array_equal(shown_state, st)
    canvas = rng.integers(0, 200, (T, n), dtype=np.uint8)
    p_off, p_xs, p_df = oracle_pairs(po, frames[1:], frames[:-1], thr)
    pool = [base] + list(frames)                      # stream s: the state is image s of the pool, its frame the next one
    m_states = np.stack([pool[s % (T + 1)] for s in range(S)])
    m_frames = np.stack([pool[(s + 1) % (T + 1)] for s in range(S)])
    ticks = [po.diff_pack(m_frames[s], m_states[s], thr) for s in range(S)]
    m_off = np.concatenate([[0], np.cumsum([c for c, _, _, _ in ticks])]).astype(np.uint32)
    m_xs = np.concatenate([x for _, x, _, _ in ticks]).astype(np.int32)
    m_df = np.concatenate([d for _, _, d, _ in ticks]).astype(np.uint8)
    m_next = np.stack([s for _, _, _, s in ticks])
    m_tot = int(m_off[S])
    applied = m_states.copy()
    for s in range(S):
        a, b = int(m_off[s]), int(m_off[s + 1])
        applied[s][m_xs[a:b]] += m_df[a:b]
    assert np.array_equal(applied, m_next)
    m_wire = po.wire_pack(m_off, m_xs, m_df)
    m_recs, m_pos = spec.encode(m_off, m_xs, m_df)
    m_counts, m_escapes = spec.headers(m_recs, S)

    # every buffer of the chain, before the first call
    I32, I64 = torch.int32, torch.int64
    fr = Region(T, n, stride, skew).put(frames)
    o1, x1, f1 = Guarded(T + 1, I32), Guarded(tot + 3, I32), Guarded(tot + 3)
    pos1, cw1 = Guarded(T + 1, I64), Guarded(recs.size + 4)
    o2, pos2, cw2 = Guarded(T + 1, I32), Guarded(T + 1, I64), Guarded(recs.size + 4)
    o3, x3, f3 = Guarded(T + 1, I32), Guarded(tot + 3, I32), Guarded(tot + 3)
    out4 = Region(T, n, stride, skew)
    red0, red1 = Region(T, n, stride, skew).put(canvas), Region(T, n, stride, skew).put(canvas)
    o6, x6, f6 = Guarded(T, I32), Guarded(p_xs.size + 3, I32), Guarded(p_xs.size + 3)
    m_fr = Region(S, n, stride, skew).put(m_frames)
    srv_a, srv_w, srv_c, cli_a, cli_w, cli_c = (Region(S, n, stride, (skew + 5) % 16).put(m_states) for _ in range(6))
    o7a, x7, f7 = Guarded(S + 1, I32), Guarded(m_tot + 3, I32), Guarded(m_tot + 3)
    o7w, wire7 = Guarded(S + 1, I32), Guarded(m_wire.size + 4)
    o7c, pos7, cw7 = Guarded(S + 1, I32), Guarded(S + 1, I64), Guarded(m_recs.size + 4)

    mb = T if seed % 2 else (T + 1) // 2              # the GPU client in slices of max_batch, every other seed
    with RawCore(w, h, threshold=thr, sample_mat_data=base, max_batch=T) as srv, \
            RawCore(w, h, threshold=thr, sample_mat_data=base, max_batch=T) as srv2, \
            RawCore(w, h, sample_mat_data=base, max_batch=mb) as cli, RawCore(w, h, threshold=thr, max_batch=S) as multi:
        cores = (srv, srv2, cli, multi)
        for c in cores:
            if schedule == 1:
                c.set_option(lib.OPT_PIPELINE, 0)
            if schedule == 2:
                c.use_torch_stream()
        torch.cuda.synchronize()                      # the uploads and fills above

        def fence():                                  # cores on streams of their own are ordered by the caller
            if schedule != 2:
                for c in cores:
                    c.synchronize()

        # 1. arrays, then the encoder
        srv.diff_stream_batch(fr.ptr, T, o1.ptr, x1.ptr, f1.ptr, tot + 3, stride=stride)
        srv.cwire_encode_batch(o1.ptr, x1.ptr, f1.ptr, tot + 3, T, pos1.ptr, cw1.ptr, recs.size + 4)
        # 2. the same frames straight into records, 3. decoded again, 5. red maps of the decoded stream
        srv2.diff_stream_cwire_batch(fr.ptr, T, o2.ptr, pos2.ptr, cw2.ptr, recs.size + 4, stride=stride)
        srv2.cwire_decode_batch(cw2.ptr, counts, escapes, T, o3.ptr, x3.ptr, f3.ptr, tot + 3)
        srv2.red_stream_batch(o3.ptr, x3.ptr, T, red0.ptr, clear=False, stride=stride)
        srv2.red_stream_batch(o3.ptr, x3.ptr, T, red1.ptr, clear=True, stride=stride)
        fence()
        # 4. the GPU client on the encoder's records
        cli.apply_cwire_batch(cw1.ptr, counts, escapes, T, out4.ptr, stride)
        # 6. pairs of consecutive frames
        if T > 1:
            srv.diff_pairs_batch(fr.ptr + stride, fr.ptr, T - 1, o6.ptr, x6.ptr, f6.ptr, p_xs.size + 3, stride=stride)
        # 7. one tick of S streams in the three forms, 8. applied to a second set of states, on one core with nothing in between
        multi.diff_multi_batch(m_fr.ptr, srv_a.ptr, S, o7a.ptr, x7.ptr, f7.ptr, m_tot + 3, stride=stride)
        multi.diff_multi_wire_batch(m_fr.ptr, srv_w.ptr, S, o7w.ptr, wire7.ptr, m_wire.size + 4, stride=stride)
        multi.diff_multi_cwire_batch(m_fr.ptr, srv_c.ptr, S, o7c.ptr, pos7.ptr, cw7.ptr, m_recs.size + 4, stride=stride)
        multi.apply_multi_batch(o7a.ptr, x7.ptr, f7.ptr, S, cli_a.ptr, stride=stride)
        multi.apply_multi_wire_batch(wire7.ptr, np.diff(m_off.astype(np.int64)), S, cli_w.ptr, stride=stride)
        multi.apply_multi_cwire_batch(cw7.ptr, m_counts, m_escapes, S, cli_c.ptr, stride=stride)
        fence()
        torch.cuda.synchronize()

        what = (seed, w, h, T, S, thr, density, pad, skew, schedule)
        assert np.array_equal(fr.get(), frames), what
        # 1
        assert np.array_equal(o1.get().view(np.uint32), off), what
        assert np.array_equal(x1.get(written=tot)[:tot], xs) and np.array_equal(f1.get(written=tot)[:tot], df), what
        assert np.array_equal(srv.get_state(), st), what
        assert np.array_equal(pos1.get().view(np.uint64), pos), what
        assert np.array_equal(cw1.get(written=recs.size)[:recs.size], recs), what
        # 2
        assert np.array_equal(o2.get().view(np.uint32), off) and np.array_equal(pos2.get().view(np.uint64), pos), what
        assert np.array_equal(cw2.get(written=recs.size)[:recs.size], recs), what
        assert np.array_equal(srv2.get_state(), st), what
        # 3
        assert np.array_equal(o3.get().view(np.uint32), off), what
        assert np.array_equal(x3.get(written=tot)[:tot], xs) and np.array_equal(f3.get(written=tot)[:tot], df), what
        # 4
        assert np.array_equal(out4.get(), shown), what
        assert np.array_equal(cli.get_state(), st), what
        # 5
        got0, got1 = red0.get(), red1.get()
        for t in range(T):
            x = xs[int(off[t]):int(off[t + 1])]
            assert np.array_equal(got0[t], po.red_overlap(canvas[t], x)), (what, t)
            assert np.array_equal(got1[t], po.red_overlap(np.zeros(n, np.uint8), x)), (what, t)
        # 6
        if T > 1:
            assert np.array_equal(o6.get().view(np.uint32), p_off), what
            assert np.array_equal(x6.get(written=p_xs.size)[:p_xs.size], p_xs), what
            assert np.array_equal(f6.get(written=p_xs.size)[:p_xs.size], p_df), what
            assert np.array_equal(srv.get_state(), st), what
        # 7
        assert np.array_equal(m_fr.get(), m_frames), what
        for o in (o7a, o7w, o7c):
            assert np.array_equal(o.get().view(np.uint32), m_off), what
        assert np.array_equal(x7.get(written=m_tot)[:m_tot], m_xs) and np.array_equal(f7.get(written=m_tot)[:m_tot], m_df), what
        assert np.array_equal(wire7.get(written=m_wire.size)[:m_wire.size], m_wire), what
        assert np.array_equal(pos7.get().view(np.uint64), m_pos), what
        assert np.array_equal(cw7.get(written=m_recs.size)[:m_recs.size], m_recs), what
        # 8: the server's states and the client's, all six the oracle's
        for r in (srv_a, srv_w, srv_c, cli_a, cli_w, cli_c):
            assert np.array_equal(r.get(), m_next), what

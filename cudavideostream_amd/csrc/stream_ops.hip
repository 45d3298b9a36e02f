// stream_ops.hip -- the two small operators either side of the packed stream:
//
//   k_apply / k_apply_all : the client's reconstruction, client/opencv.cpp:64-66
//                           (`frame2.data[xs[i]] += buffer[i]` for the pos entries of a frame);
//   k_apply_multi(_wire)  : the same for one segment of each of many streams, onto the caller's states
//                           (k_apply_multi_strided: segment s*T + t of each, one launch per t of a burst);
//   k_merge_parts         : concatenation of the streams of the row bands of ONE video stream that
//                           several cores (GPUs) packed independently into
//                           the single stream the sender would have produced;
//   k_cwire_*             : the compact wire format's encoder (packed stream -> gap-coded records) and decoder;
//   k_cwa_*               : the compact records applied straight to a client core's state (mi355_apply_cwire_batch) or,
//                           one record per stream, to the caller's states (mi355_apply_multi_cwire_batch), or a burst of
//                           records per stream, with the frames in between (mi355_apply_multi_stream_cwire_batch);
//   k_cwc_*               : a burst of compact records per stream summed into ONE record / segment per stream, from the records
//                           alone (mi355_cwire_coalesce_batch / _cwire_batch);
//   k_cwb_*               : one record per stream thinned to an entry budget, the caller's states reverted where entries are
//                           dropped (mi355_cwire_budget_cwire_batch);
//   k_dsp_*               : one record per stream without the entries of isolated pixels (fewer than `need` changed pixels among
//                           the 8 around them), the caller's states reverted there (mi355_cwire_despeckle_cwire_batch);
//   k_crop_*              : a stream's coalesced records cut to a rectangle and re-indexed to the rectangle's frame
//                           (mi355_cwire_crop_batch / _cwire_batch);
//   k_mosaic_*            : the coalesced records of many streams placed side by side into ONE record of a canvas frame
//                           (mi355_cwire_mosaic_batch / _cwire_batch);
//   k_act_*               : where the entries of each stream's records land: a grid of counts per cell, a bounding box and the
//                           peak cell per stream (mi355_cwire_activity_batch; mi355_activity_batch from the arrays).
//   k_cwk_*               : one verdict of four words per compact record -- is it well-formed and canonical, and where not --
//                           from the records alone, with sums that cannot wrap (mi355_cwire_check_batch).
//   k_cws_*               : every compact record cut into pieces of at most a datagram's bytes, each a record of the same frame
//                           (mi355_cwire_split_cwire_batch).
//
// The first two are index-driven byte scatter/copy: HBM-latency work with 5 bytes of traffic per entry, no
// arithmetic worth naming.
#include "cwire_common.h"

namespace mi355 {

__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// One frame.  Indices of a frame are distinct (strictly ascending, tests/cuda_streaming/test.cu:563-573),
// so plain byte read-modify-writes do not race.  count comes from the device (offsets) or the host.
// xs is read with byte alignment because the wire format puts it at any address.
__global__ __launch_bounds__(256) void k_apply(uint8_t *frame, uint32_t nbytes, const uint8_t *xs,
                                               const uint8_t *diff, const uint32_t *d_offsets, int t,
                                               uint32_t host_count) {
    uint32_t first = 0, count = host_count;
    if (d_offsets) {
        first = d_offsets[t];
        count = d_offsets[t + 1] - first;
    }
    const uint32_t step = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += step) {
        const uint32_t x = load_u32_unaligned(xs + 4 * (size_t)(first + i));
        if (x < nbytes) frame[x] = (uint8_t)(frame[x] + diff[first + i]);   // opencv.cpp:65
    }
}

// All frames of a batch at once, final frame only: per-byte addition modulo 256 commutes, so entries of
// different frames may land in any order as long as each add is atomic on its byte -- a 32-bit
// compare-and-swap on the containing dword (the frame buffer is dword padded by the allocator).
__global__ __launch_bounds__(256) void k_apply_all(uint8_t *frame, uint32_t nbytes, const int32_t *xs,
                                                   const uint8_t *diff, const uint32_t *d_offsets,
                                                   int nframes) {
    const uint32_t count = d_offsets[nframes];
    const uint32_t step = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += step) {
        const uint32_t x = (uint32_t)xs[i];
        if (x >= nbytes) continue;
        const uint32_t d = diff[i];
        uint32_t *p = (uint32_t *)(frame + (x & ~3u));
        const uint32_t sh = 8u * (x & 3u);
        uint32_t old = *p, assumed;
        do {
            assumed = old;
            const uint32_t byte = ((assumed >> sh) + d) & 0xffu;
            old = atomicCAS(p, assumed, (assumed & ~(0xffu << sh)) | (byte << sh));
        } while (old != assumed);
    }
}

hipError_t launch_apply(uint8_t *frame, uint32_t nbytes, const void *xs, const void *diff,
                        const uint32_t *d_offsets, int t, uint32_t host_count, hipStream_t s) {
    uint32_t blocks = 512;   // device-side counts: a fixed grid strides over whatever the frame holds
    if (!d_offsets) {
        if (host_count == 0) return hipSuccess;
        blocks = (host_count + 255u) / 256u;
        if (blocks > 2048u) blocks = 2048u;
    }
    hipLaunchKernelGGL(k_apply, dim3(blocks), dim3(256), 0, s, frame, nbytes, (const uint8_t *)xs,
                       (const uint8_t *)diff, d_offsets, t, host_count);
    return hipGetLastError();
}

hipError_t launch_apply_all(uint8_t *frame, uint32_t nbytes, const int32_t *xs, const uint8_t *diff,
                            const uint32_t *d_offsets, int nframes, hipStream_t s) {
    hipLaunchKernelGGL(k_apply_all, dim3(4096), dim3(256), 0, s, frame, nbytes, xs, diff, d_offsets, nframes);
    return hipGetLastError();
}

// ---- mi355_apply_multi_batch / _wire_batch: segment s onto the caller's state s --------------------------------------------
// One launch strides over the entries of all segments; a lane finds its segment by binary search in the segments' first
// entries, which the workgroup keeps in LDS.  Indices of a segment are distinct and segments go to different states, so
// plain byte read-modify-writes do not race -- and a byte store cannot touch the neighbouring state, which a dword
// compare-and-swap at the edge of two states stride == N apart would.
// off[0 .. nseg] ascending, off[0] <= i < off[nseg]: the segment s with off[s] <= i < off[s + 1] (the last such)
template <class T>
__device__ __forceinline__ uint32_t apply_multi_segment(const T *off, uint32_t nseg, T i) {
    uint32_t lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// lds != 0: the nstreams + 1 offsets fit the launch's dynamic LDS
__global__ __launch_bounds__(256) void k_apply_multi(uint8_t *states, size_t stride, uint32_t nbytes, const uint32_t *offsets,
                                                     const int32_t *xs, const uint8_t *diff, uint32_t nstreams, int lds) {
    extern __shared__ uint32_t s_off[];
    const uint32_t *off = offsets;
    if (lds) {
        for (uint32_t j = threadIdx.x; j <= nstreams; j += 256) s_off[j] = offsets[j];
        __syncthreads();
        off = s_off;
    }
    const uint32_t first = off[0], end = off[nstreams];
    const uint32_t step = gridDim.x * 256u;
    for (uint64_t i64 = (uint64_t)first + blockIdx.x * 256u + threadIdx.x; i64 < end; i64 += step) {
        const uint32_t i = (uint32_t)i64;
        const uint32_t x = (uint32_t)xs[i];
        if (x >= nbytes) continue;
        uint8_t *p = states + (size_t)apply_multi_segment(off, nstreams, i) * stride + x;
        *p = (uint8_t)(*p + diff[i]);   // opencv.cpp:65
    }
}

// The wire form: segment j of this launch is stream h.first + j, {u32 n, i32 xs[n], u8 diff[n]} at wire + h.pos[j], with
// h.cum[j] entries in the segments before it (the host's headers; the header words in the buffer are not read).  xs is
// read with byte alignment, as k_apply does.
__global__ __launch_bounds__(256) void k_apply_multi_wire(uint8_t *states, size_t stride, uint32_t nbytes, const uint8_t *wire,
                                                          const ApplyMultiWireArgs h) {
    __shared__ uint64_t s_cum[kApplyMultiWireStreams + 1], s_pos[kApplyMultiWireStreams];
    const uint32_t nseg = (uint32_t)h.count;
    for (uint32_t j = threadIdx.x; j <= nseg; j += 256) {
        s_cum[j] = h.cum[j];
        if (j < nseg) s_pos[j] = h.pos[j];
    }
    __syncthreads();
    const uint64_t end = s_cum[nseg];
    const uint32_t step = gridDim.x * 256u;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < end; i += step) {
        const uint32_t seg = apply_multi_segment(s_cum, nseg, i);
        const uint64_t j = i - s_cum[seg], cnt = s_cum[seg + 1] - s_cum[seg];
        const uint8_t *rec_xs = wire + s_pos[seg] + 4, *rec_diff = rec_xs + 4 * cnt;   // opencv.cpp:52-62
        const uint32_t x = load_u32_unaligned(rec_xs + 4 * j);
        if (x >= nbytes) continue;
        uint8_t *p = states + (size_t)(h.first + seg) * stride + x;
        *p = (uint8_t)(*p + rec_diff[j]);
    }
}

hipError_t launch_apply_multi(uint8_t *states, size_t stride, uint32_t nbytes, const uint32_t *d_offsets, const int32_t *xs,
                              const uint8_t *diff, int nstreams, hipStream_t s) {
    // device-side counts: a fixed grid strides over whatever the segments hold
    const size_t words = (size_t)nstreams + 1;
    const bool lds = words <= 8192;   // 32 KiB; more streams than that search the offsets where they are
    hipLaunchKernelGGL(k_apply_multi, dim3(1024), dim3(256), lds ? words * sizeof(uint32_t) : 0, s, states, stride, nbytes,
                       d_offsets, xs, diff, (uint32_t)nstreams, lds ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_apply_multi_wire(uint8_t *states, size_t stride, uint32_t nbytes, const uint8_t *wire,
                                   const ApplyMultiWireArgs &h, hipStream_t s) {
    const uint64_t total = h.cum[h.count];
    if (total == 0) return hipSuccess;
    const uint64_t blocks = (total + 255u) / 256u;
    hipLaunchKernelGGL(k_apply_multi_wire, dim3((uint32_t)(blocks > 2048u ? 2048u : blocks)), dim3(256), 0, s, states, stride,
                       nbytes, wire, h);
    return hipGetLastError();
}

// ---- mi355_apply_multi_stream_batch / _wire_batch: nframes records of each stream, batch index b = s*nframes + t -------------
// Records of ONE stream may hit the same byte, so the argument above does not reach across t: the host issues one launch per
// t, and launch t takes the segments s*nframes + t of all streams -- one per state, race-free as above.  The segments of a
// launch are not neighbours in the offsets, so the grid is (x, streams) and a workgroup strides over its stream's segment;
// the wire form keeps k_apply_multi_wire (its segments' places are kernel arguments anyway).
__global__ __launch_bounds__(256) void k_apply_multi_strided(uint8_t *states, size_t stride, uint32_t nbytes, const uint32_t *offsets,
                                                             const int32_t *xs, const uint8_t *diff, uint32_t nstreams,
                                                             uint32_t nframes, uint32_t t) {
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t s = blockIdx.y; s < nstreams; s += gridDim.y) {
        const size_t b = (size_t)s * nframes + t;
        const uint32_t first = offsets[b], end = offsets[b + 1];
        uint8_t *state = states + (size_t)s * stride;
        for (uint64_t i = (uint64_t)first + blockIdx.x * 256u + threadIdx.x; i < end; i += step) {
            const uint32_t x = (uint32_t)xs[i];
            if (x >= nbytes) continue;
            state[x] = (uint8_t)(state[x] + diff[i]);   // opencv.cpp:65
        }
    }
}

// State s -> output frame s*nframes + t (what the client shows after record t): the N bytes and nothing else; 16-byte words
// when both addresses allow.
__global__ __launch_bounds__(256) void k_apply_multi_show(const uint8_t *states, size_t stride, uint32_t nbytes, uint8_t *out,
                                                          size_t out_stride, uint32_t nstreams, uint32_t nframes, uint32_t t) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    for (uint32_t s = blockIdx.y; s < nstreams; s += gridDim.y) {
        const uint8_t *src = states + (size_t)s * stride;
        uint8_t *dst = out + ((size_t)s * nframes + t) * out_stride;
        const uint32_t q = (((uintptr_t)src | (uintptr_t)dst) & 15u) ? 0u : nbytes / 16u;
        for (uint32_t i = gid; i < q; i += step) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
        for (uint32_t i = 16 * q + gid; i < nbytes; i += step) dst[i] = src[i];
    }
}

// a grid of (x, streams) workgroups, about 1024 in all, no more along x than the frame has 256-byte pieces
static dim3 apply_multi_strided_grid(uint32_t nbytes, int nstreams) {
    const uint32_t y = nstreams < 65535 ? (uint32_t)nstreams : 65535u;
    uint32_t x = 1024u / y, most = (nbytes + 255u) / 256u;
    if (x > most) x = most;
    return dim3(x ? x : 1u, y);
}

hipError_t launch_apply_multi_strided(uint8_t *states, size_t stride, uint32_t nbytes, const uint32_t *d_offsets, const int32_t *xs,
                                      const uint8_t *diff, int nstreams, int nframes, int t, hipStream_t s) {
    hipLaunchKernelGGL(k_apply_multi_strided, apply_multi_strided_grid(nbytes, nstreams), dim3(256), 0, s, states, stride, nbytes,
                       d_offsets, xs, diff, (uint32_t)nstreams, (uint32_t)nframes, (uint32_t)t);
    return hipGetLastError();
}

hipError_t launch_apply_multi_show(const uint8_t *states, size_t stride, uint32_t nbytes, uint8_t *out, size_t out_stride,
                                   int nstreams, int nframes, int t, hipStream_t s) {
    hipLaunchKernelGGL(k_apply_multi_show, apply_multi_strided_grid(nbytes, nstreams), dim3(256), 0, s, states, stride, nbytes, out,
                       out_stride, (uint32_t)nstreams, (uint32_t)nframes, (uint32_t)t);
    return hipGetLastError();
}

// ---- export of one packed frame into host-mapped (pinned) buffers ---------------------------------------
// The pipelined per-frame path has no host synchronisation between the pack and the copies back
// (the reference reads the count, synchronises, then sizes two cudaMemcpy with it,
// server/src/kernels.cu:507-524): the count stays on the device and this kernel stores exactly `count`
// entries, and the count itself, through the PCIe-mapped pointers.
__global__ __launch_bounds__(256) void k_export(const uint32_t *offsets, const int32_t *xs, const uint8_t *diff,
                                                int32_t *h_xs, uint8_t *h_diff, uint32_t *h_count) {
    const uint32_t count = offsets[1] - offsets[0];
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    if (gid == 0) *h_count = count;
    // 16-byte stores where the host pointers allow (the device arrays are allocation aligned)
    if (((uintptr_t)h_xs & 15u) == 0) {
        const uint32_t q = count / 4;
        for (uint32_t i = gid; i < q; i += step) ((uint4 *)h_xs)[i] = ((const uint4 *)xs)[i];
        for (uint32_t i = 4 * q + gid; i < count; i += step) h_xs[i] = xs[i];
    } else {
        for (uint32_t i = gid; i < count; i += step) h_xs[i] = xs[i];
    }
    if (((uintptr_t)h_diff & 15u) == 0) {
        const uint32_t q = count / 16;
        for (uint32_t i = gid; i < q; i += step) ((uint4 *)h_diff)[i] = ((const uint4 *)diff)[i];
        for (uint32_t i = 16 * q + gid; i < count; i += step) h_diff[i] = diff[i];
    } else {
        for (uint32_t i = gid; i < count; i += step) h_diff[i] = diff[i];
    }
}

hipError_t launch_export(const uint32_t *offsets, const int32_t *xs, const uint8_t *diff, int32_t *h_xs,
                         uint8_t *h_diff, uint32_t *h_count, hipStream_t s) {
    hipLaunchKernelGGL(k_export, dim3(256), dim3(256), 0, s, offsets, xs, diff, h_xs, h_diff, h_count);
    return hipGetLastError();
}

// The same for ONE compact record (mi355_exec_cwire / mi355_pipe_submit_cwire): the record the encoder has just written at
// rec[0 .. frame_pos[1]) of the core's record buffer goes to the mapped host pointer, its {n, e, bytes low, bytes high} to
// four pinned words.  The size is read from the device word -- no host round trip -- and clamped to rec_bytes, the
// size both buffers are known to have (the caller's capacity was checked against it), so that a wrong word could never run
// past either.  Whole 16-byte stores when the host pointer allows (rec is allocation aligned and padded to 16), dwords
// otherwise and for the tail; no byte at or past the record's end is written.
__global__ __launch_bounds__(256) void k_export_record(const uint64_t *frame_pos, const uint32_t *rec, uint64_t rec_bytes,
                                                       uint32_t *h_record, uint32_t *h_words) {
    uint64_t bytes = frame_pos[1];
    if (bytes > rec_bytes) bytes = rec_bytes;
    const uint64_t dwords = bytes / 4;   // (a record is a whole number of dwords)
    const uint64_t gid = blockIdx.x * 256u + threadIdx.x, step = (uint64_t)gridDim.x * 256u;
    if (gid == 0) {
        h_words[0] = dwords >= 2 ? rec[0] : 0u;
        h_words[1] = dwords >= 2 ? rec[1] : 0u;
        h_words[2] = (uint32_t)(4 * dwords);
        h_words[3] = (uint32_t)((4 * dwords) >> 32);
    }
    if (((uintptr_t)h_record & 15u) == 0) {
        const uint64_t q = dwords / 4;
        for (uint64_t i = gid; i < q; i += step) ((uint4 *)h_record)[i] = ((const uint4 *)rec)[i];
        for (uint64_t i = 4 * q + gid; i < dwords; i += step) h_record[i] = rec[i];
    } else {
        for (uint64_t i = gid; i < dwords; i += step) h_record[i] = rec[i];
    }
}

hipError_t launch_export_record(const uint64_t *frame_pos, const uint8_t *rec, uint64_t rec_bytes, uint32_t *h_record,
                                uint32_t *h_words, hipStream_t s) {
    hipLaunchKernelGGL(k_export_record, dim3(256), dim3(256), 0, s, frame_pos, (const uint32_t *)rec, rec_bytes, h_record, h_words);
    return hipGetLastError();
}

// ---- merge of row-band streams -------------------------------------------------------------------------
// Part p (a row band, bands ordered top to bottom) holds its own packed stream of the same T frames:
// index part_off[p][0..T], entries at xs_all/diff_all[part_base[p] + ...], byte indices relative to
// the band.  Frame t of the merged stream is the parts' frame-t segments in part order with
// xs + xs_bias[p]: the ascending order of tests/cuda_streaming/test.cu:563-573 over the whole frame.
//   k_merge_index : out_offsets[t] = sum_p part_off[p][t]           (grid-stride over t)
//   k_merge_parts : workgroup (t, p) copies its segment              (grid = (T, nparts))
__global__ __launch_bounds__(256) void k_merge_index(const uint32_t *part_off, int nparts, int nframes,
                                                     uint32_t *out_offsets) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t <= nframes; t += gridDim.x * blockDim.x) {
        uint32_t acc = 0;
        for (int p = 0; p < nparts; p++) acc += part_off[(size_t)p * (nframes + 1) + t];
        out_offsets[t] = acc;
    }
}

__global__ __launch_bounds__(256) void k_merge_parts(const MergeArgs a) {
    const int t = blockIdx.x, p = blockIdx.y;
    const uint32_t *po = a.part_off + (size_t)p * (a.nframes + 1);
    const uint32_t src0 = po[t], cnt = po[t + 1] - src0;
    uint32_t dst = 0;   // entries of all parts in frames < t, plus parts < p in frame t
    for (int q = 0; q < a.nparts; q++) {
        const uint32_t *qo = a.part_off + (size_t)q * (a.nframes + 1);
        dst += q < p ? qo[t + 1] : qo[t];
    }
    const size_t src = (size_t)a.part_base[p] + src0;
    const int32_t bias = a.xs_bias[p];
    for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
        if ((size_t)dst + i < a.capacity) {
            a.out_xs[dst + i] = a.xs_all[src + i] + bias;
            a.out_diff[dst + i] = a.diff_all[src + i];
        }
    }
}

hipError_t launch_merge(const MergeArgs &a, uint32_t *out_offsets, hipStream_t s) {
    hipLaunchKernelGGL(k_merge_index, dim3((a.nframes + 256) / 256), dim3(256), 0, s, a.part_off, a.nparts,
                       a.nframes, out_offsets);
    if (a.nframes > 0 && a.nparts > 0)
        hipLaunchKernelGGL(k_merge_parts, dim3(a.nframes, a.nparts), dim3(256), 0, s, a);
    return hipGetLastError();
}


// ---- compact wire format (include/mi355diff.h, "compact wire"): encoder and decoder ------------------------------
// The record, its arithmetic and the steps all of these kernels share: cwire_common.h.
// The encoder is three launches, none of which waits on another workgroup:
//   k_cwire_count (grid (bpf, T)): workgroup (b, t) owns a contiguous range of frame t's code dwords and counts its
//                                  escapes into cnt[t*bpf + b];
//   k_cwire_scan  (one workgroup): cnt -> exclusive prefix within each frame, e_t, frame_pos (exclusive scan of the
//                                  record sizes);
//   k_cwire_emit  (grid (bpf, T)): each lane builds one dword of codes and one of diffs (4 entries), ranks its escapes
//                                  with __ballot + popcount, and stores dwords only.
// Guard of every kernel: offsets[T] > entries_capacity (a diff batch that dropped entries) or a frame whose offsets run
// backwards or past offsets[T] -> nothing is read from xs / diff, nothing written but frame_pos[T] = UINT64_MAX.
__device__ __forceinline__ bool cwire_frame_ok(const uint32_t *off, int t, uint64_t total, uint32_t *lo, uint32_t *n) {
    const uint32_t a = off[t], b = off[t + 1];
    *lo = a;
    *n = b - a;
    return a <= b && b <= total;
}

// the escape flags and codes of the (up to) 4 entries of code dword d of a frame whose entries start at xs
__device__ __forceinline__ uint32_t cwire_codes(const int32_t *xs, uint32_t n, uint32_t d, uint32_t g[4], bool esc[4]) {
    const uint32_t i0 = 4 * d;
    uint32_t x[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        ok[j] = i0 + j < n;
        x[j] = ok[j] ? (uint32_t)xs[i0 + j] : 0u;
    }
    return cwire_encode4(x, ok, i0 ? (uint32_t)xs[i0 - 1] + 1u : 0u, g, esc);
}

__global__ __launch_bounds__(256) void k_cwire_count(const uint32_t *offsets, const int32_t *xs, uint64_t entries_capacity,
                                                     int nframes, uint32_t *cnt) {
    __shared__ uint32_t wsum[4];
    const int t = blockIdx.y, b = blockIdx.x, bpf = gridDim.x;
    const uint64_t total = offsets[nframes];
    uint32_t lo, n;
    if (total > entries_capacity || !cwire_frame_ok(offsets, t, total, &lo, &n)) return;
    const uint64_t D = cwire_dwords(n);
    const uint32_t d0 = (uint32_t)(D * b / bpf), d1 = (uint32_t)(D * (b + 1) / bpf);
    uint32_t mine = 0;   // wave-uniform
    for (uint32_t base = d0; base < d1; base += 256) {
        const uint32_t d = base + threadIdx.x;
        uint32_t g[4];
        bool esc[4] = {false, false, false, false};
        if (d < d1) cwire_codes(xs + lo, n, d, g, esc);
#pragma unroll
        for (int j = 0; j < 4; j++) mine += (uint32_t)__popcll(__ballot(esc[j]));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) cnt[(size_t)t * bpf + b] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

constexpr int kCwScanThreads = 1024;

__global__ __launch_bounds__(kCwScanThreads) void k_cwire_scan(const uint32_t *offsets, uint64_t entries_capacity, int nframes,
                                                               int bpf, uint32_t *cnt, uint64_t *frame_pos) {
    extern __shared__ uint32_t s_cnt[];   // nframes * bpf
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const uint64_t total = offsets[nframes];
    if (tid == 0) s_bad = total > entries_capacity;
    __syncthreads();
    if (s_bad) {
        if (tid == 0) frame_pos[nframes] = ~0ull;
        return;
    }
    for (int t = tid; t < nframes; t += kCwScanThreads) {
        uint32_t lo, n;
        if (!cwire_frame_ok(offsets, t, total, &lo, &n)) s_bad = 1;
    }
    const int ncnt = nframes * bpf;
    for (int i = tid; i < ncnt; i += kCwScanThreads) s_cnt[i] = cnt[i];
    __syncthreads();
    if (s_bad) {
        if (tid == 0) frame_pos[nframes] = ~0ull;
        return;
    }
    cwire_scan_frame_pos<kCwScanThreads>(
        nframes, frame_pos,
        [&](int t, uint32_t &n, uint32_t &e) {
            for (int b = 0; b < bpf; b++) {   // exclusive prefix of the frame's escapes per workgroup of the emit kernel
                const uint32_t c = s_cnt[t * bpf + b];
                cnt[(size_t)t * bpf + b] = e;
                e += c;
            }
            n = offsets[t + 1] - offsets[t];
        },
        [](int, uint64_t, uint32_t, uint32_t) {});
}

__global__ __launch_bounds__(256) void k_cwire_emit(const uint32_t *offsets, const int32_t *xs, const uint8_t *diff,
                                                    uint64_t entries_capacity, int nframes, const uint32_t *cnt,
                                                    const uint64_t *frame_pos, uint8_t *out, uint64_t capacity_bytes) {
    __shared__ uint32_t s_wave[2][4];
    const int t = blockIdx.y, b = blockIdx.x, bpf = gridDim.x;
    const uint64_t total = offsets[nframes];
    uint32_t lo, n;
    if (total > entries_capacity || frame_pos[nframes] == ~0ull || !cwire_frame_ok(offsets, t, total, &lo, &n)) return;
    const uint64_t fp0 = frame_pos[t], fp1 = frame_pos[t + 1];
    if (fp1 > capacity_bytes) return;   // the frame does not fit: skipped whole
    const uint64_t D = cwire_dwords(n);
    const uint32_t e = cwire_record_escapes(fp1 - fp0, n);
    uint32_t *hdr = (uint32_t *)(out + fp0);
    const CwireSections<uint8_t> sec(out, fp0, n, e);
    uint32_t *code = sec.code32(), *esc = sec.esc32(), *dif = sec.diff32();
    if (b == 0 && threadIdx.x == 0) {
        hdr[0] = n;
        hdr[1] = e;
    }
    const int32_t *fx = xs + lo;
    const uint8_t *fd = diff + lo;
    const uint32_t d0 = (uint32_t)(D * b / bpf), d1 = (uint32_t)(D * (b + 1) / bpf);
    uint32_t carry = cnt[(size_t)t * bpf + b];   // escapes of the frame before this workgroup's range
    int buf = 0;
    for (uint32_t base = d0; base < d1; base += 256, buf ^= 1) {
        const uint32_t d = base + threadIdx.x;
        const bool live = d < d1;
        uint32_t g[4];
        bool fl[4] = {false, false, false, false};
        uint32_t word = 0, dw = 0;
        if (live) {
            word = cwire_codes(fx, n, d, g, fl);
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (4 * d + j < n) dw |= (uint32_t)fd[4 * d + j] << (8 * j);
        }
        uint32_t wtot;   // escapes of the lanes below this one in the wave, and of the whole wave
        const uint32_t before = cwire_rank4(fl, wtot);
        const uint32_t rank = block_waves_before<4>(wtot, 0, s_wave[buf], carry) + before;
        if (live) {
            code[d] = word;
            dif[d] = dw;
            cwire_store_escapes<false>(esc, e, rank, g, fl);
        }
    }
}

// Workgroups per frame of the count / emit kernels: about 8192 in all, at most 256 per frame.
int cwire_blocks_per_frame(int nframes) {
    int b = kCwireSlots / (nframes > 0 ? nframes : 1);
    return b < 1 ? 1 : (b > 256 ? 256 : b);
}

hipError_t launch_cwire_encode(const uint32_t *offsets, const int32_t *xs, const uint8_t *diff, uint64_t entries_capacity,
                               int nframes, uint32_t *cnt, uint64_t *frame_pos, uint8_t *out, uint64_t capacity_bytes,
                               hipStream_t s) {
    const int bpf = cwire_blocks_per_frame(nframes);
    if (nframes > 0)
        hipLaunchKernelGGL(k_cwire_count, dim3(bpf, nframes), dim3(256), 0, s, offsets, xs, entries_capacity, nframes, cnt);
    hipLaunchKernelGGL(k_cwire_scan, dim3(1), dim3(kCwScanThreads), sizeof(uint32_t) * (size_t)nframes * bpf, s, offsets,
                       entries_capacity, nframes, bpf, cnt, frame_pos);
    if (nframes > 0)
        hipLaunchKernelGGL(k_cwire_emit, dim3(bpf, nframes), dim3(256), 0, s, offsets, xs, diff, entries_capacity, nframes,
                           cnt, frame_pos, out, capacity_bytes);
    return hipGetLastError();
}

// Decoder: one workgroup per frame, frames described by the host (positions follow from the headers the client read).
// The frame's entries are scanned in tiles of 1024 (4 per lane): escape rank = escapes before the entry (ballot), index =
// running sum of g + 1, minus 1.  Reads stay inside the record [pos, pos + cwire_record_bytes(n, e)); an escape ranked at or past e
// decodes to 0xFFFFFFFF (and adds nothing to the running sum); entries at or past `capacity` are not written.
__global__ __launch_bounds__(256) void k_cwire_decode(const CwireDecodeArgs a) {
    __shared__ uint32_t s_esc[2][4], s_sum[2][4];
    const CwireFrame f = a.frame[blockIdx.x];
    if (threadIdx.x == 0) {
        if (a.first_frame + blockIdx.x == 0) a.offsets[0] = 0;
        a.offsets[a.first_frame + blockIdx.x + 1] = f.out + f.n;
    }
    const uint32_t D = cwire_dwords(f.n);
    const CwireSections<const uint8_t> sec(a.cwire, f.pos, f.n, f.e);
    const uint32_t *code = sec.code32(), *esc = sec.esc32(), *dif = sec.diff32();
    uint32_t carry_e = 0, carry_x = 0;
    int buf = 0;
    for (uint32_t base = 0; base < D; base += 256, buf ^= 1) {
        const uint32_t d = base + threadIdx.x;
        const bool live = d < D;
        const uint32_t word = live ? code[d] : 0u, dw = live ? dif[d] : 0u;
        bool in[4], fl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) in[j] = live && 4 * d + j < f.n;
        uint32_t wtot;
        const uint32_t before = cwire_escapes_before(word, in, fl, wtot);
        const uint32_t rank = block_waves_before<4>(wtot, 0, s_esc[buf], carry_e) + before;
        uint32_t inc[4], rk[4];
        bool bad[4];
        const uint32_t lsum = cwire_decode4(word, in, fl, rank, f.e, esc, inc, bad, rk);
        uint32_t x = block_exclusive_scan<4>(lsum, s_sum[buf], carry_x);
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t i = 4 * d + j;
                if (i >= f.n) break;
                x += inc[j];
                const uint64_t o = (uint64_t)f.out + i;
                if (o < a.capacity) {
                    a.xs[o] = bad[j] ? (int32_t)0xFFFFFFFFu : (int32_t)(x - 1u);
                    a.diff[o] = (uint8_t)(dw >> (8 * j));
                }
            }
        }
    }
}

hipError_t launch_cwire_decode(const CwireDecodeArgs &a, int nframes, hipStream_t s) {
    if (nframes > 0) hipLaunchKernelGGL(k_cwire_decode, dim3(nframes), dim3(256), 0, s, a);
    return hipGetLastError();
}


// ---- mi355_apply_cwire_batch: compact records (include/mi355diff.h, "compact wire") applied straight to a
// client core's state, client/opencv.cpp:50-66, without expanding them into (offsets, xs, diff) first.
//
// Tile-major.  The state is cut into byte tiles of kCwaTile bytes; one single-wave workgroup owns a tile for the whole
// slice of frames: it keeps the tile in LDS, adds the tile's own entries of frame 0, 1, ... in order and stores the
// tile to each output frame, then to the state once.  What a tile workgroup needs to start decoding frame t in the middle
// of the record -- the first entry at or past the tile, the escape rank there and the running index before it -- is a
// directory word dir[t][tile] that four small kernels make from the records beforehand:
//   k_cwa_table  (grid: frames)  : the frames' headers (kernel arguments, host) -> ftab; chunk -> frame map
//   k_cwa_facts  (grid: chunks)  : per chunk of kCwaChunk codes: escape codes, sum of g + 1 over the other codes
//   k_cwa_scan   (grid: frames)  : exclusive scan over the frame's chunks (escape counts, then running sums)
//   k_cwa_escsum (grid: chunks)  : adds the chunk's escaped gaps (esc[r] + 1 for its ranks r < e) to its sum
//   k_cwa_dir    (grid: chunks)  : decodes the chunk once; entry k writes dir[t][tile] for every tile whose first byte
//                                  lies in (x[k-1], x[k]]; the frame's last chunk writes k = n into the tiles past x[n-1]
//   k_cwa_apply  (grid: tiles)   : the tile loop above
// No workgroup waits on another; nothing but the state and the output frames' bytes is written outside the core's
// scratch.  Decoding follows k_cwire_decode (stream_ops.hip): an escape ranked at or past e adds nothing to the running
// index and changes nothing, indices outside the tile are not applied, reads stay inside [pos, pos + record bytes).
typedef uint32_t cwa_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t cwa_wave_sum(uint32_t v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
    return v;
}

__device__ __forceinline__ uint64_t cwa_ceil_tile(uint32_t x) { return ((uint64_t)x + kCwaTile - 1) / kCwaTile; }

__device__ __forceinline__ CwireSections<const uint8_t> cwa_sections(const CwaArgs &a, const CwaFrame &f) {
    return CwireSections<const uint8_t>(a.cwire, f.pos, f.n, f.e);
}

// ---- headers -> ftab, chunk -> frame ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cwa_table(const CwaArgs a, const CwaTableArgs h) {
    const int i = blockIdx.x;
    const CwaFrame f = h.frame[i];
    if (threadIdx.x == 0) a.ftab[h.first + i] = f;
    for (uint32_t j = threadIdx.x; j < f.nc; j += 256) a.chunk[f.cbase + j] = make_uint4(0u, 0u, 0u, (uint32_t)(h.first + i));
}

// ---- per chunk: escape codes (x) and sum of g + 1 over the non-escaped codes (z) --------------------------------------------
__global__ __launch_bounds__(256) void k_cwa_facts(const CwaArgs a) {
    __shared__ uint32_t s_cnt[4], s_sum[4];
    const uint32_t c = blockIdx.x;
    const uint32_t t = a.chunk[c].w;
    const CwaFrame f = a.ftab[t];
    const uint32_t k0 = (c - f.cbase) * kCwaChunk;
    const uint32_t k1 = f.n - k0 < kCwaChunk ? f.n : k0 + kCwaChunk;
    const uint32_t *code = cwa_sections(a, f).code32();
    uint32_t cnt = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < (int)(kCwaChunk / 1024); i++) {
        const uint32_t d = k0 / 4 + threadIdx.x + 256 * i;
        if (4 * d < k1) {
            const uint32_t w = code[d];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t g = (w >> (8 * j)) & 255u;
                if (4 * d + j < k1) {
                    if (g == 255u) cnt++;
                    else sum += g + 1u;
                }
            }
        }
    }
    cnt = cwa_wave_sum(cnt);
    sum = cwa_wave_sum(sum);
    if ((threadIdx.x & 63) == 0) {
        s_cnt[threadIdx.x >> 6] = cnt;
        s_sum[threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.chunk[c].x = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        a.chunk[c].z = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    }
}

// ---- per frame: exclusive scan over its chunks; field 0: x (escape codes) -> y (first escape rank), field 1: z -> z ------
__global__ __launch_bounds__(256) void k_cwa_scan(const CwaArgs a, int field) {
    __shared__ uint32_t s_wave[2][4];
    const CwaFrame f = a.ftab[blockIdx.x];
    uint32_t carry = 0;
    int buf = 0;
    for (uint32_t i0 = 0; i0 < f.nc; i0 += 256, buf ^= 1) {
        const uint32_t i = i0 + threadIdx.x;
        uint4 *ch = a.chunk + f.cbase + i;
        const uint32_t v = i < f.nc ? (field == 0 ? ch->x : ch->z) : 0u;
        const uint32_t before = block_exclusive_scan<4>(v, s_wave[buf], carry);
        if (i < f.nc) {
            if (field == 0) ch->y = before;
            else ch->z = before;
        }
    }
}

// ---- per chunk: + sum of esc[r] + 1 over its escape ranks r in [y, y + x) below e ---------------------------------------
__global__ __launch_bounds__(256) void k_cwa_escsum(const CwaArgs a) {
    __shared__ uint32_t s_sum[4];
    const uint32_t c = blockIdx.x;
    const uint4 ch = a.chunk[c];
    const CwaFrame f = a.ftab[ch.w];
    const uint32_t r0 = ch.y < f.e ? ch.y : f.e;
    const uint32_t r1 = f.e - r0 < ch.x ? f.e : r0 + ch.x;
    const uint32_t *esc = cwa_sections(a, f).esc32();
    uint32_t sum = 0;
    for (uint32_t r = r0 + threadIdx.x; r < r1; r += 256) sum += esc[r] + 1u;
    sum = cwa_wave_sum(sum);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) a.chunk[c].z = ch.z + s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// ---- per chunk: the directory words of the tiles its entries open ---------------------------------------------------------
__global__ __launch_bounds__(256) void k_cwa_dir(const CwaArgs a) {
    __shared__ uint32_t s_esc[2][4], s_sum[2][4];
    const uint32_t c = blockIdx.x;
    const uint4 ch = a.chunk[c];
    const uint32_t t = ch.w;
    const CwaFrame f = a.ftab[t];
    const uint32_t cl = c - f.cbase;
    const uint32_t k0 = cl * kCwaChunk;
    const uint32_t k1 = f.n - k0 < kCwaChunk ? f.n : k0 + kCwaChunk;
    const CwireSections<const uint8_t> sec = cwa_sections(a, f);
    const uint32_t *code = sec.code32(), *esc = sec.esc32();
    uint4 *dir = a.dir + (size_t)t * a.ntiles;
    uint32_t carry_e = ch.y, carry_x = ch.z;   // escape rank and running index (sum of g + 1) before the chunk
    int buf = 0;
    for (uint32_t base = k0; base < k1; base += 1024, buf ^= 1) {
        const uint32_t d = base / 4 + threadIdx.x;
        const bool live = 4 * d < k1;
        const uint32_t word = live ? code[d] : 0u;
        bool in[4], fl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) in[j] = live && 4 * d + j < k1;
        uint32_t wtot;
        const uint32_t before = cwire_escapes_before(word, in, fl, wtot);
        const uint32_t rank = block_waves_before<4>(wtot, 0, s_esc[buf], carry_e) + before;
        uint32_t inc[4], rk[4];
        bool bad[4];
        const uint32_t lsum = cwire_decode4(word, in, fl, rank, f.e, esc, inc, bad, rk);
        uint32_t x = block_exclusive_scan<4>(lsum, s_sum[buf], carry_x);
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t k = 4 * d + j;
                if (k >= k1) break;
                const uint32_t xn = x + inc[j];
                // tiles whose first byte s has x <= s < xn, i.e. x[k-1] < s <= x[k] (none when the sum wrapped)
                uint64_t lo = cwa_ceil_tile(x), hi = cwa_ceil_tile(xn);
                if (hi > a.ntiles) hi = a.ntiles;
                for (uint64_t tl = lo; tl < hi; tl++) dir[tl] = make_uint4(k, rk[j], x, 0u);
                x = xn;
            }
        }
    }
    if (cl + 1 == f.nc)   // the tiles past the frame's last entry (all of them for n = 0)
        for (uint64_t tl = cwa_ceil_tile(carry_x) + threadIdx.x; tl < a.ntiles; tl += 256)
            dir[tl] = make_uint4(f.n, carry_e, carry_x, 0u);
}

// ---- per tile: the slice's frames in order, in LDS -------------------------------------------------------------------------
// Bytes [lo, lo + len) of src -> LDS, or LDS -> dst: whole 16-byte words where the global address allows, bytes otherwise.
__device__ __forceinline__ void cwa_tile_load(uint8_t *s, const uint8_t *src, uint32_t len, int lane) {
    const uint32_t q = ((uintptr_t)src & 15u) ? 0u : len / 16u;
    for (uint32_t i = lane; i < q; i += 64) ((cwa_u32x4 *)s)[i] = ((const cwa_u32x4 *)src)[i];
    for (uint32_t i = 16 * q + lane; i < len; i += 64) s[i] = src[i];
}

__device__ __forceinline__ void cwa_tile_store(uint8_t *dst, const uint8_t *s, uint32_t len, int lane) {
    const uint32_t q = ((uintptr_t)dst & 15u) ? 0u : len / 16u;
    for (uint32_t i = lane; i < q; i += 64) __builtin_nontemporal_store(((const cwa_u32x4 *)s)[i], (cwa_u32x4 *)dst + i);
    for (uint32_t i = 16 * q + lane; i < len; i += 64) __builtin_nontemporal_store(s[i], dst + i);
}

// The first block of a frame's entries for the tile: 256 entries from k & ~3, four per lane (code and diff dwords).
struct CwaBlock {
    uint32_t word, dw;
};

// DIFF == false: the codes only (dw stays 0), for the walks that do not look at the differences (k_act_tile).
template <bool DIFF = true>
__device__ __forceinline__ CwaBlock cwa_block_load(const CwaArgs &a, const CwaFrame &f, uint32_t k, int lane) {
    const uint32_t d = k / 4 + lane;
    CwaBlock b{0u, 0u};
    if (k < f.n && 4 * d < f.n) {
        const CwireSections<const uint8_t> sec = cwa_sections(a, f);
        b.word = sec.code32()[d];
        if (DIFF) b.dw = sec.diff32()[d];
    }
    return b;
}

// Record f's entries from directory word dr = {first entry, its escape rank, running index before it} on: op(idx, diff byte)
// for every entry with lo <= idx < hi.  b: the first block (cwa_block_load at dr.x).  One wave.  The decode loop of the GPU
// clients, once: k_cwa_apply runs it per frame of a slice, k_cwa_apply_multi per stream, the coalescer, the budget and the
// motion grid per record of a tile.  DIFF == false: the differences are not loaded and op gets 0.
template <bool DIFF, class Op>
__device__ __forceinline__ void cwa_walk_record(const CwaArgs &a, const CwaFrame &f, const uint4 dr, CwaBlock b, uint32_t lo,
                                                uint32_t hi, int lane, Op op) {
    const CwireSections<const uint8_t> sec = cwa_sections(a, f);
    const uint32_t *code = sec.code32(), *esc = sec.esc32(), *dif = sec.diff32();
    uint32_t k = dr.x, rank = dr.y, x = dr.z;
    bool first = true;
    while (k < f.n) {
        const uint32_t ka = k & ~3u, d = ka / 4 + lane;
        if (!first) {
            b.word = 4 * d < f.n ? code[d] : 0u;
            if (DIFF) b.dw = 4 * d < f.n ? dif[d] : 0u;
        }
        first = false;
        bool in[4], fl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) in[j] = 4 * d + j >= k && 4 * d + j < f.n;
        uint32_t wtot;
        const uint32_t before = cwire_escapes_before(b.word, in, fl, wtot);
        uint32_t inc[4], rk[4];
        bool bad[4];
        const uint32_t lsum = cwire_decode4(b.word, in, fl, rank + before, f.e, esc, inc, bad, rk);
        rank += wtot;
        uint32_t xi = block_exclusive_scan<1>(lsum, (uint32_t *)nullptr, x);   // a single wave: no LDS, no barrier
#pragma unroll
        for (int j = 0; j < 4; j++) {
            xi += inc[j];
            const uint32_t idx = xi - 1u;   // (inc 0: a bad escape or a masked entry, nothing to apply)
            if (inc[j] && idx >= lo && idx < hi) op(idx, (uint8_t)(b.dw >> (8 * j)));
        }
        k = ka + 256;
        if (x >= hi) break;   // the next entry's index is at least x
    }
}

// ... added to the tile [lo, hi) in LDS (s[0] is byte lo)
__device__ __forceinline__ void cwa_apply_record(uint8_t *s, const CwaArgs &a, const CwaFrame &f, const uint4 dr, CwaBlock b,
                                                 uint32_t lo, uint32_t hi, int lane) {
    cwa_walk_record<true>(a, f, dr, b, lo, hi, lane, [=](uint32_t idx, uint8_t d) { s[idx - lo] = (uint8_t)(s[idx - lo] + d); });
}

__global__ __launch_bounds__(64) void k_cwa_apply(const CwaArgs a, int nframes) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    const uint32_t hi = lo + len;
    cwa_tile_load(s, a.state + lo, len, lane);
    // while frame t is applied, frame t + 1's first block and frame t + 2's directory word are in flight
    CwaFrame f1 = a.ftab[0], f2 = f1;
    uint4 d1 = a.dir[tile], d2 = d1;
    CwaBlock b1 = cwa_block_load(a, f1, d1.x, lane);
    if (nframes > 1) {
        f2 = a.ftab[1];
        d2 = a.dir[(size_t)a.ntiles + tile];
    }
    __syncthreads();
    for (int t = 0; t < nframes; t++) {
        const CwaFrame f = f1;
        const uint4 dr = d1;
        const CwaBlock b = b1;
        if (t + 1 < nframes) {
            f1 = f2;
            d1 = d2;
            b1 = cwa_block_load(a, f1, d1.x, lane);
        }
        if (t + 2 < nframes) {
            f2 = a.ftab[t + 2];
            d2 = a.dir[(size_t)(t + 2) * a.ntiles + tile];
        }
        cwa_apply_record(s, a, f, dr, b, lo, hi, lane);
        __syncthreads();
        if (a.out) cwa_tile_store(a.out + (size_t)t * a.stride + lo, s, len, lane);
        __syncthreads();
    }
    const uint32_t q = len / 16u;   // the state is allocation aligned
    for (uint32_t i = lane; i < q; i += 64) ((cwa_u32x4 *)(a.state + lo))[i] = s_q[i];
    for (uint32_t i = 16 * q + lane; i < len; i += 64) a.state[lo + i] = s[i];
}

// ---- mi355_apply_multi_cwire_batch: record s onto the caller's state s, one record each ------------------------------------
// Grid of tiles x streams (workgroup w: stream w / ntiles, tile w % ntiles); a.state / a.stride are the caller's states.  The
// directory says which entries of record s land in the tile -- [dir[s][tile].x, dir[s][tile + 1].x), the last tile's up to
// n -- before a state byte is touched: a workgroup with none returns, so the traffic follows the changes and not N.  The
// others load the tile, run the decode loop above once and store the tile back, non-temporal: whole 16-byte words when
// the tile's address allows it (states and stride multiples of 16), bytes otherwise.  No store leaves the tile's own
// [lo, hi) of states[s], so neighbouring states (stride == N, N odd) and the stride gap are never touched.
__global__ __launch_bounds__(64) void k_cwa_apply_multi(const CwaArgs a) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const CwaFrame f = a.ftab[st];
    const uint4 *dir = a.dir + (size_t)st * a.ntiles + tile;
    const uint4 dr = dir[0];
    const uint32_t kend = tile + 1 < a.ntiles ? dir[1].x : f.n;
    if (dr.x >= kend || dr.x >= f.n) return;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    uint8_t *tile_bytes = a.state + (size_t)st * a.stride + lo;
    const CwaBlock b = cwa_block_load(a, f, dr.x, lane);
    cwa_tile_load(s, tile_bytes, len, lane);
    __syncthreads();
    cwa_apply_record(s, a, f, dr, b, lo, lo + len, lane);
    __syncthreads();
    cwa_tile_store(tile_bytes, s, len, lane);
}

// ---- mi355_apply_multi_stream_cwire_batch: records s*nframes .. (s + 1)*nframes - 1 onto the caller's state s, in order ----
// Grid of tiles x streams as above.  Lane j asks the directory whether record t = j of its stream (passes of 64 records) has
// an entry in the tile, and a ballot gives the pass's set of records that do.  The tile is loaded from states[s] once, when
// the first pass with a record for it comes (at once when frames go out), and stored back once, non-temporal, if a record
// touched it: a tile that none of the stream's records lands in is neither read nor written when no frames go out.  The
// walk over t runs cwa_apply_record for the records of the set only -- the others cost neither a directory word nor a code
// load -- with the next such record's header, directory word and first block in flight, and with output frames stores the
// tile to frame s*nframes + t after every t.  No store leaves the tile's own [lo, hi) of its state or of its output frame;
// the states are the caller's (any alignment), so the write-back is cwa_tile_store, not k_cwa_apply's aligned epilogue.
__global__ __launch_bounds__(64) void k_cwa_apply_multi_stream(const CwaArgs a, int nframes, size_t out_stride) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    const uint32_t hi = lo + len;
    const size_t b0 = (size_t)st * nframes;   // the stream's first batch index
    uint8_t *tile_bytes = a.state + (size_t)st * a.stride + lo;
    bool loaded = false, dirty = false;
    for (int base = 0; base < nframes; base += 64) {
        bool touch = false;
        if (base + lane < nframes) {
            const size_t b = b0 + base + lane;
            const uint32_t fn = a.ftab[b].n;
            const uint4 *dir = a.dir + b * a.ntiles + tile;
            const uint32_t k0 = dir[0].x, kend = tile + 1 < a.ntiles ? dir[1].x : fn;
            touch = k0 < kend && k0 < fn;
        }
        const uint64_t set = __ballot(touch);
        if (!set && !a.out) continue;
        if (!loaded) {
            cwa_tile_load(s, tile_bytes, len, lane);
            loaded = true;
        }
        const int cnt = nframes - base < 64 ? nframes - base : 64;
        // while record j is applied, the header, directory word and first block of the set's next record are in flight
        CwaFrame f1{};
        uint4 d1{};
        CwaBlock b1{};
        int j = a.out ? 0 : __ffsll((unsigned long long)set) - 1, jn = set ? __ffsll((unsigned long long)set) - 1 : cnt;
        if (jn < cnt) {
            f1 = a.ftab[b0 + base + jn];
            d1 = a.dir[(b0 + base + jn) * a.ntiles + tile];
            b1 = cwa_block_load(a, f1, d1.x, lane);
        }
        __syncthreads();
        while (j < cnt) {
            if (j == jn) {
                const CwaFrame f = f1;
                const uint4 dr = d1;
                const CwaBlock b = b1;
                const uint64_t rest = set & ~((2ull << j) - 1ull);   // (j = 63: 2 << 63 is 0, rest = 0)
                jn = rest ? __ffsll((unsigned long long)rest) - 1 : cnt;
                if (jn < cnt) {
                    f1 = a.ftab[b0 + base + jn];
                    d1 = a.dir[(b0 + base + jn) * a.ntiles + tile];
                    b1 = cwa_block_load(a, f1, d1.x, lane);
                }
                cwa_apply_record(s, a, f, dr, b, lo, hi, lane);
                dirty = true;
                __syncthreads();
            }
            if (a.out) {
                cwa_tile_store(a.out + (b0 + base + j) * out_stride + lo, s, len, lane);
                __syncthreads();
                j++;
            } else {
                j = jn;
            }
        }
    }
    if (dirty) cwa_tile_store(tile_bytes, s, len, lane);
}

// ---- mi355_cwire_coalesce_(cwire_)batch: records s*nframes .. (s + 1)*nframes - 1 -> ONE record / segment per stream ---------
// The sum (mod 256) of a stream's differences at every byte index, the indices whose sum is not 0 in ascending order.  Nothing
// but the records is read: the tile machinery above applied to a ZEROED tile in LDS gives the sums, and the tile is encoded
// from LDS.  Behind the directory of the nstreams*nframes records:
//   k_cwc_sum   (grid: tiles x streams, one wave) : the summed tile -> one fact word per (stream, tile) in the chunk scratch
//                                                   (free once k_cwa_dir has run: the tile kernels read ftab and dir only):
//                                                   {nonzero bytes, index of the first, index of the last, gaps >= 255
//                                                   between consecutive nonzero bytes inside the tile}; a tile no record
//                                                   lands in writes an all-zero word (the scratch holds stale data) and returns
//   k_cwc_scan  (grid: streams)                   : over the stream's tiles: fact word -> {nonzero bytes, entries before the
//                                                   tile, escapes before it, 1 + the last index before it (0: none)}; the
//                                                   stream's n to offsets[s + 1], its e to frame_pos[s + 1] (unscanned)
//   k_cwc_place (one workgroup)                   : offsets, frame_pos scanned in place; the records' headers and pad bytes
//   k_cwc_emit  (grid: tiles x streams, one wave) : a tile with no nonzero byte returns before it touches anything; the others
//                                                   build the summed tile again (record bytes, not N) and write their entries
// A lane owns 64 consecutive bytes of the tile: only its first nonzero byte can be an escape (the others' gaps are below 64).
// No workgroup waits on another.  The entries of a tile are compacted in LDS at the alignment of their place in the output and
// stored as dwords inside, bytes at the ragged edges: neighbouring workgroups share dwords of the code and diff sections and
// never read-modify-write one.  Malformed content: both tile kernels compute the same tile from the same bytes, so the facts
// and the record agree whatever the records held.
// The records of stream st that have an entry in the tile, in order: the ballot passes and the walk of
// k_cwa_apply_multi_stream without a state and output frames.  clear() runs once, before the first such record, and
// record(f, dr, b) per record (the caller's LDS: a barrier follows clear and every record); false: no record has an entry in
// the tile and neither ran.  DIFF: cwa_block_load's.
template <bool DIFF, class Clear, class Record>
__device__ __forceinline__ bool cwa_tile_records(const CwaArgs &a, int nframes, uint32_t st, uint32_t tile, int lane, Clear clear,
                                                 Record record) {
    const size_t b0 = (size_t)st * nframes;   // the stream's first batch index
    bool any = false;
    for (int base = 0; base < nframes; base += 64) {
        bool touch = false;
        if (base + lane < nframes) {
            const size_t b = b0 + base + lane;
            const uint32_t fn = a.ftab[b].n;
            const uint4 *dir = a.dir + b * a.ntiles + tile;
            const uint32_t k0 = dir[0].x, kend = tile + 1 < a.ntiles ? dir[1].x : fn;
            touch = k0 < kend && k0 < fn;
        }
        const uint64_t set = __ballot(touch);
        if (!set) continue;
        if (!any) {
            clear();
            any = true;
        }
        const int cnt = nframes - base < 64 ? nframes - base : 64;
        // while record j is applied, the header, directory word and first block of the set's next record are in flight
        int jn = __ffsll((unsigned long long)set) - 1;
        CwaFrame f1 = a.ftab[b0 + base + jn];
        uint4 d1 = a.dir[(b0 + base + jn) * a.ntiles + tile];
        CwaBlock b1 = cwa_block_load<DIFF>(a, f1, d1.x, lane);
        __syncthreads();
        while (jn < cnt) {
            const int j = jn;
            const CwaFrame f = f1;
            const uint4 dr = d1;
            const CwaBlock b = b1;
            const uint64_t rest = set & ~((2ull << j) - 1ull);   // (j = 63: 2 << 63 is 0, rest = 0)
            jn = rest ? __ffsll((unsigned long long)rest) - 1 : cnt;
            if (jn < cnt) {
                f1 = a.ftab[b0 + base + jn];
                d1 = a.dir[(b0 + base + jn) * a.ntiles + tile];
                b1 = cwa_block_load<DIFF>(a, f1, d1.x, lane);
            }
            record(f, dr, b);
            __syncthreads();
        }
    }
    return any;
}

// The stream's summed tile [lo, hi) in LDS (s: kCwaTile bytes; s[0] is byte lo); false: no record has an entry in the tile
// and s was not touched.
__device__ __forceinline__ bool cwc_sum_tile(uint8_t *s, const CwaArgs &a, int nframes, uint32_t st, uint32_t tile, uint32_t lo,
                                             uint32_t hi, int lane) {
    return cwa_tile_records<true>(
        a, nframes, st, tile, lane,
        [=]() {
            for (uint32_t i = lane; i < kCwaTile / 16; i += 64) ((cwa_u32x4 *)s)[i] = cwa_u32x4{0u, 0u, 0u, 0u};
        },
        [&](const CwaFrame &f, const uint4 dr, const CwaBlock b) { cwa_apply_record(s, a, f, dr, b, lo, hi, lane); });
}

// What a lane's 64 bytes of the summed tile hold: bit i of the mask = byte 64*lane + i is not 0
__device__ __forceinline__ uint64_t cwc_lane_mask(const uint8_t *s, int lane) {
    const uint32_t *w = (const uint32_t *)s + 16 * lane;
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t v = w[i];
        const uint32_t nz = ((v & 0xffu) ? 1u : 0u) | ((v & 0xff00u) ? 2u : 0u) | ((v & 0xff0000u) ? 4u : 0u) | ((v & 0xff000000u) ? 8u : 0u);
        m |= (uint64_t)nz << (4 * i);
    }
    return m;
}

// The index an entry of the tile is written with: its byte index x itself (the crop call maps x into its rectangle's frame:
// any map that ascends with x and never widens the distance of two kept bytes can stand here, so that a gap >= 255 still opens
// between lanes only)
struct CwcIdentity {
    __device__ __forceinline__ uint32_t operator()(uint32_t x) const { return x; }
};

// 1 + the written index of the last nonzero byte of the lanes below this one that hold any (0: none does); lanes: the ballot
// of the lanes that hold one
template <class Map>
__device__ __forceinline__ uint32_t cwc_end_before(uint64_t m, uint64_t lanes, int lane, uint32_t lo, const Map &map) {
    const uint32_t my_end = m ? map(lo + 64u * lane + 63u - (uint32_t)__builtin_clzll(m)) + 1u : 0u;
    const uint64_t below = lanes & ((1ull << lane) - 1ull);
    const int src = below ? 63 - __builtin_clzll(below) : 0;
    const uint32_t end = (uint32_t)__shfl((int)my_end, src, 64);
    return below ? end : 0u;
}

// The four facts of the tile in LDS (s[0] is byte lo): {nonzero bytes, index of the first, index of the last, gaps >= 255 inside},
// indices and gaps as `map` writes them
template <class Map = CwcIdentity>
__device__ __forceinline__ uint4 cwc_tile_facts(const uint8_t *s, uint32_t lo, int lane, const Map map = Map()) {
    const uint64_t m = cwc_lane_mask(s, lane);
    const uint64_t lanes = __ballot(m != 0);
    const uint32_t count = cwa_wave_sum((uint32_t)__popcll(m));
    const uint32_t end = cwc_end_before(m, lanes, lane, lo, map);
    const uint32_t my_first = m ? map(lo + 64u * lane + (uint32_t)__builtin_ctzll(m)) : 0u;
    // the gap in front of a lane's first nonzero byte, where a lane below holds one (the tile's first has no gap inside the tile)
    const bool wide = m && end && my_first - end >= 255u;
    const uint32_t gaps = (uint32_t)__popcll(__ballot(wide));
    uint32_t first = 0, last = 0;
    if (lanes) {
        const int l0 = __ffsll((unsigned long long)lanes) - 1, l1 = 63 - __builtin_clzll(lanes);
        const uint32_t my_last = m ? map(lo + 64u * lane + 63u - (uint32_t)__builtin_clzll(m)) : 0u;
        first = (uint32_t)__shfl((int)my_first, l0, 64);
        last = (uint32_t)__shfl((int)my_last, l1, 64);
    }
    return make_uint4(count, first, last, gaps);
}

__global__ __launch_bounds__(64) void k_cwc_sum(const CwaArgs a, int nframes) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    uint4 *fact = a.chunk + (size_t)st * a.ntiles + tile;
    if (!cwc_sum_tile(s, a, nframes, st, tile, lo, lo + len, lane)) {
        if (lane == 0) *fact = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4 f = cwc_tile_facts(s, lo, lane);
    if (lane == 0) *fact = f;
}

// carry = max(carry, every value); returns the max of carry and the values of the threads below this one.  One barrier
// (none for a single wave); s_wave as block_waves_before.
template <int NW>
__device__ __forceinline__ uint32_t cwc_block_exclusive_max(uint32_t v, uint32_t *s_wave, uint32_t &carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)incl, k, 64);
        if (lane >= k && u > incl) incl = u;
    }
    uint32_t before = (uint32_t)__shfl_up((int)incl, 1, 64);
    if (lane == 0) before = 0;
    if (before < carry) before = carry;
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    for (int w = 0; w < NW; w++) {
        const uint32_t u = s_wave[w];
        if (w < wave && u > before) before = u;
        if (u > carry) carry = u;
    }
    return before;
}

template <bool CWIRE>
__global__ __launch_bounds__(256) void k_cwc_scan(const CwaArgs a, const CwcOut o) {
    __shared__ uint32_t s_n[2][4], s_e[2][4], s_end[2][4];
    const uint32_t st = blockIdx.x;
    uint4 *facts = a.chunk + (size_t)st * a.ntiles;
    uint32_t n = 0, e = 0, end = 0;   // entries, escapes and 1 + the last index of the tiles before the round
    int buf = 0;
    for (uint32_t i0 = 0; i0 < a.ntiles; i0 += 256, buf ^= 1) {
        const uint32_t i = i0 + threadIdx.x;
        const uint4 f = i < a.ntiles ? facts[i] : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t nbefore = block_exclusive_scan<4>(f.x, s_n[buf], n);
        const uint32_t prev_end = cwc_block_exclusive_max<4>(f.x ? f.z + 1u : 0u, s_end[buf], end);
        // the tile's first entry: g_0 = xs[0] for the stream's first, else the gap across the tile edge (and any empty tiles)
        const uint32_t esc = f.x ? f.w + (f.y - prev_end >= 255u ? 1u : 0u) : 0u;
        const uint32_t ebefore = block_exclusive_scan<4>(esc, s_e[buf], e);
        if (i < a.ntiles) facts[i] = make_uint4(f.x, nbefore, ebefore, prev_end);
    }
    if (threadIdx.x == 0) {
        o.offsets[st + 1] = n;
        if (CWIRE) o.frame_pos[st + 1] = e;
    }
}

constexpr int kCwcPlaceThreads = 1024;

// offsets[s + 1] = n_s, frame_pos[s + 1] = e_s -> the exclusive scans, in place (a thread reads its stream's two words before
// the round's barrier and writes behind it); compact form: header and zero pad bytes of every record that fits
template <bool CWIRE>
__global__ __launch_bounds__(kCwcPlaceThreads) void k_cwc_place(const CwcOut o, int nstreams) {
    __shared__ uint32_t s_n[kCwcPlaceThreads / 64];
    __shared__ uint64_t s_pos[kCwcPlaceThreads / 64];
    const int tid = threadIdx.x;
    uint32_t first = 0;
    uint64_t pos = 0;
    for (int s0 = 0; s0 < nstreams; s0 += kCwcPlaceThreads) {
        const int s = s0 + tid;
        const bool live = s < nstreams;
        const uint32_t n = live ? o.offsets[s + 1] : 0u;
        const uint32_t e = live && CWIRE ? (uint32_t)o.frame_pos[s + 1] : 0u;
        const uint64_t rec = live && CWIRE ? cwire_record_bytes(n, e) : 0;
        const uint32_t my_first = block_exclusive_scan<kCwcPlaceThreads / 64>(n, s_n, first);
        uint64_t my_pos = 0;
        if (CWIRE) my_pos = block_exclusive_scan<kCwcPlaceThreads / 64>(rec, s_pos, pos);
        if (live) {
            o.offsets[s] = my_first;
            if (CWIRE) {
                o.frame_pos[s] = my_pos;
                if (my_pos + rec <= o.capacity) {
                    uint32_t *hdr = (uint32_t *)(o.cwire + my_pos);
                    hdr[0] = n;
                    hdr[1] = e;
                    const CwireSections<uint8_t> sec(o.cwire, my_pos, n, e);
                    for (uint32_t k = n; k < (uint32_t)cwire_pad4(n); k++) {
                        sec.code[k] = 0;
                        sec.diff[k] = 0;
                    }
                }
            }
        }
        __syncthreads();   // the scans' LDS words are rewritten by the next round
    }
    if (tid == 0) {
        o.offsets[nstreams] = first;
        if (CWIRE) o.frame_pos[nstreams] = pos;
    }
}

// cnt bytes of LDS at s + sh -> g, where sh = g & 3: bytes up to g's first dword, whole dwords, bytes behind the last
__device__ __forceinline__ void cwc_store_bytes(uint8_t *g, const uint8_t *s, uint32_t sh, uint32_t cnt, int lane) {
    const uint32_t head = (4u - sh) & 3u;
    if (cnt <= head) {
        if ((uint32_t)lane < cnt) __builtin_nontemporal_store(s[sh + lane], g + lane);
        return;
    }
    const uint32_t q = (cnt - head) / 4u, tail = head + 4u * q;
    if ((uint32_t)lane < head) __builtin_nontemporal_store(s[sh + lane], g + lane);
    const uint32_t *sw = (const uint32_t *)(s + sh + head);   // sh + head is 0 or 4
    uint32_t *gw = (uint32_t *)(g + head);
    for (uint32_t i = lane; i < q; i += 64) __builtin_nontemporal_store(sw[i], gw + i);
    if ((uint32_t)lane < cnt - tail) __builtin_nontemporal_store(s[sh + tail + lane], g + tail + lane);
}

// The entries of the tile in LDS (s[0] is byte lo; fact: its scanned word {nonzero bytes, entries before, escapes before, end
// before}) to their place in stream st's record {n, e} at fp0 (compact form) or segment at `seg` (arrays form).  s_code / s_diff:
// kCwaTile + 8 bytes of LDS each (s_code unused in the arrays form).  One wave.  map: the facts' (end before included).
template <bool CWIRE, class Map = CwcIdentity>
__device__ __forceinline__ void cwc_emit_tile(const uint8_t *s, uint8_t *s_code, uint8_t *s_diff, const uint4 fact, const CwcOut &o,
                                              uint32_t seg, uint32_t n, uint64_t fp0, uint32_t e, uint32_t lo, int lane,
                                              const Map map = Map()) {
    const uint64_t m = cwc_lane_mask(s, lane);
    const uint64_t lanes = __ballot(m != 0);
    uint32_t zero = 0;
    const uint32_t r0 = block_exclusive_scan<1>((uint32_t)__popcll(m), (uint32_t *)nullptr, zero);   // tile-relative rank
    const uint32_t before = cwc_end_before(m, lanes, lane, lo, map);
    uint32_t end = before ? before : fact.w;   // 1 + the index of the entry before the lane's first
    // where the tile's entries go, and the alignment of that place
    uint8_t *g_code = nullptr, *g_diff;
    uint32_t *g_esc = nullptr;
    uint64_t room = fact.x;   // entries of the tile that are written
    if (CWIRE) {
        const CwireSections<uint8_t> sec(o.cwire, fp0, n, e);
        g_code = sec.code + fact.y;
        g_diff = sec.diff + fact.y;
        g_esc = sec.esc32();
    } else {
        const uint64_t at = (uint64_t)seg + fact.y;
        room = at < o.capacity ? (o.capacity - at < room ? o.capacity - at : room) : 0;
        g_diff = o.diff + at;
    }
    const uint32_t sh_code = (uint32_t)((uintptr_t)g_code & 3u), sh_diff = (uint32_t)((uintptr_t)g_diff & 3u);
    const uint32_t first_gap = m ? map(lo + 64u * lane + (uint32_t)__builtin_ctzll(m)) - end : 0u;
    const bool escaped = CWIRE && m && first_gap >= 255u;
    const uint32_t erank = fact.z + (uint32_t)__popcll(__ballot(escaped) & ((1ull << lane) - 1ull));
    if (escaped && erank < e) __builtin_nontemporal_store(first_gap, g_esc + erank);
    uint32_t r = r0;
    const uint32_t *w = (const uint32_t *)s + 16 * lane;
    for (int i = 0; i < 16 && m; i++) {
        const uint32_t v = w[i];
        if (!v) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t d = (v >> (8 * j)) & 255u;
            if (!d) continue;
            const uint32_t x = map(lo + 64u * lane + 4u * i + j);
            if (CWIRE) {
                const uint32_t g = x - end;
                s_code[sh_code + r] = (uint8_t)(g < 255u ? g : 255u);
            } else if (r < room) {
                __builtin_nontemporal_store((int32_t)x, o.xs + (uint64_t)seg + fact.y + r);
            }
            s_diff[sh_diff + r] = (uint8_t)d;
            end = x + 1u;
            r++;
        }
    }
    __syncthreads();
    if (CWIRE) cwc_store_bytes(g_code, s_code, sh_code, (uint32_t)room, lane);
    cwc_store_bytes(g_diff, s_diff, sh_diff, (uint32_t)room, lane);
}

template <bool CWIRE>
__global__ __launch_bounds__(64) void k_cwc_emit(const CwaArgs a, const CwcOut o, int nframes) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    __shared__ uint32_t s_code32[CWIRE ? kCwaTile / 4 + 2 : 1], s_diff32[kCwaTile / 4 + 2];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint4 fact = a.chunk[(size_t)st * a.ntiles + tile];   // {nonzero bytes, entries before, escapes before, end before}
    if (fact.x == 0) return;
    const uint32_t seg = o.offsets[st], n = o.offsets[st + 1] - seg;
    uint64_t fp0 = 0;
    uint32_t e = 0;
    if (CWIRE) {
        fp0 = o.frame_pos[st];
        const uint64_t fp1 = o.frame_pos[st + 1];
        if (fp1 > o.capacity) return;   // the record does not fit: skipped whole, by every workgroup alike
        e = cwire_record_escapes(fp1 - fp0, n);
    }
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    if (!cwc_sum_tile(s, a, nframes, st, tile, lo, lo + len, lane)) return;   // (the facts say otherwise)
    cwc_emit_tile<CWIRE>(s, (uint8_t *)s_code32, (uint8_t *)s_diff32, fact, o, seg, n, fp0, e, lo, lane);
}

// ---- mi355_cwire_budget_cwire_batch: record s of a tick thinned to h_budget[s] entries, the caller's state s reverted where ----
// an entry is dropped.  An entry (x, d) of stream s changed state[s][x] from prev = cur - d to cur; its magnitude a = |cur -
// prev| (as integers: the diff byte alone does not give it) is above the threshold T0 that made the record.  The entries with
// a > T are the record of the same tick at threshold T >= T0, and the state of that tick holds prev at the others.  Behind the
// directory of the nstreams records (hist: [nstreams][kCwbWords] words of the core, zeroed and given the budgets by k_cwb_init):
//   k_cwb_hist  (grid: tiles x streams, one wave) : streams over their budget only; the tile of differences in LDS (cwc_sum_tile,
//                                                   one record), the same tile of the state, a per bin of a 256-bin histogram in LDS,
//                                                   then ONE global atomic per nonzero bin
//   k_cwb_thr   (grid: streams)                   : T_s = the least T in [T0, 255] with at most `budget` entries of a > T
//   k_cwb_facts (grid: tiles x streams, one wave) : k_cwc_sum on the tile with the entries of a <= T_s zeroed
//   k_cwc_scan, k_cwc_place                       : the coalescer's, unchanged
//   k_cwb_emit  (grid: tiles x streams, one wave) : the filtered tile again, from the same bytes: the state is read by all three
//                                                   tile passes and written by this, the last one, alone -- prev at the dropped
//                                                   entries, single byte stores by the lanes that own them, also where the record
//                                                   is skipped for lack of room; then k_cwc_emit's tile
// A stream with T_s == T0 is not filtered (every entry of a record made at T0 has a > T0): its state is not even read.
// The lane's 64 bytes of the tile of differences s against the same bytes of the state sv: HIST: hist[a]++ per entry; else the
// entries with a <= thr are zeroed in s and, REVERT, state[x] = prev is stored to g (the tile's place in the state).
template <bool HIST, bool REVERT>
__device__ __forceinline__ void cwb_lane_bytes(uint8_t *s, const uint8_t *sv, uint32_t thr, uint32_t *hist, uint8_t *g, int lane) {
    uint32_t *w = (uint32_t *)s + 16 * lane;
    const uint32_t *wv = (const uint32_t *)sv + 16 * lane;
    for (int i = 0; i < 16; i++) {
        const uint32_t v = w[i];
        if (!v) continue;
        const uint32_t cv = wv[i];
        uint32_t keep = v;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t d = (v >> (8 * j)) & 255u;
            if (!d) continue;
            const uint32_t cur = (cv >> (8 * j)) & 255u, prev = (cur - d) & 255u;
            const uint32_t mag = cur > prev ? cur - prev : prev - cur;   // 1 .. 255
            if (HIST) {
                atomicAdd(hist + mag, 1u);
            } else if (mag <= thr) {
                keep &= ~(255u << (8 * j));
                if (REVERT) g[64 * lane + 4 * i + j] = (uint8_t)prev;
            }
        }
        if (!HIST) w[i] = keep;
    }
}

__global__ __launch_bounds__(256) void k_cwb_init(uint32_t *hist, const CwbInitArgs h) {
    uint32_t *row = hist + (size_t)(h.first + blockIdx.x) * kCwbWords;
    row[threadIdx.x] = 0u;
    if (threadIdx.x == 0) {
        row[kCwbBudget] = h.budget[blockIdx.x];
        row[kCwbThr] = h.thr0;
    }
}

__global__ __launch_bounds__(64) void k_cwb_hist(const CwaArgs a, uint32_t *hist) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16], s_v[kCwaTile / 16];
    __shared__ uint32_t s_hist[256];
    uint8_t *s = (uint8_t *)s_q, *sv = (uint8_t *)s_v;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    uint32_t *row = hist + (size_t)st * kCwbWords;
    if (row[kCwbBudget] >= a.ftab[st].n) return;   // within its budget whatever the magnitudes are
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    if (!cwc_sum_tile(s, a, 1, st, tile, lo, lo + len, lane)) return;
    for (int i = lane; i < 256; i += 64) s_hist[i] = 0u;
    cwa_tile_load(sv, a.state + (size_t)st * a.stride + lo, len, lane);
    __syncthreads();
    cwb_lane_bytes<true, false>(s, sv, 0u, s_hist, nullptr, lane);
    __syncthreads();
    for (int i = lane; i < 256; i += 64) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(row + i, v);
    }
}

__global__ __launch_bounds__(256) void k_cwb_thr(uint32_t *hist, uint32_t thr0, uint32_t *thresholds) {
    __shared__ uint32_t s_bin[256];
    uint32_t *row = hist + (size_t)blockIdx.x * kCwbWords;
    const uint32_t T = threadIdx.x, budget = row[kCwbBudget];
    s_bin[T] = row[T];
    __syncthreads();
    uint32_t above = 0;   // entries with a > T
    for (uint32_t k = T + 1; k < 256; k++) above += s_bin[k];
    // `above` falls with T: the T in [thr0, 255) that are over the budget are the first ones
    const int over = __syncthreads_count(T >= thr0 && T < 255u && above > budget);
    if (T == 0) {
        row[kCwbThr] = thr0 + (uint32_t)over;
        thresholds[blockIdx.x] = thr0 + (uint32_t)over;
    }
}

// The tile of stream st in LDS, filtered where `filter` says so; false: no entry of the record lands in the tile (s untouched).
// REVERT: the dropped entries' state bytes are stored.
template <bool REVERT>
__device__ __forceinline__ bool cwb_tile(uint8_t *s, uint8_t *sv, const CwaArgs &a, uint32_t thr, bool filter, uint32_t st, uint32_t tile,
                                         uint32_t lo, uint32_t len, int lane) {
    if (!cwc_sum_tile(s, a, 1, st, tile, lo, lo + len, lane)) return false;
    if (filter) {
        uint8_t *g = a.state + (size_t)st * a.stride + lo;
        cwa_tile_load(sv, g, len, lane);
        __syncthreads();
        cwb_lane_bytes<false, REVERT>(s, sv, thr, nullptr, g, lane);
        __syncthreads();
    }
    return true;
}

__global__ __launch_bounds__(64) void k_cwb_facts(const CwaArgs a, const uint32_t *hist, uint32_t thr0) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16], s_v[kCwaTile / 16];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t thr = hist[(size_t)st * kCwbWords + kCwbThr];
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    uint4 *fact = a.chunk + (size_t)st * a.ntiles + tile;
    if (!cwb_tile<false>(s, (uint8_t *)s_v, a, thr, thr > thr0, st, tile, lo, len, lane)) {
        if (lane == 0) *fact = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4 f = cwc_tile_facts(s, lo, lane);
    if (lane == 0) *fact = f;
}

__global__ __launch_bounds__(64) void k_cwb_emit(const CwaArgs a, const CwcOut o, const uint32_t *hist, uint32_t thr0) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16], s_v[kCwaTile / 16];
    __shared__ uint32_t s_code32[kCwaTile / 4 + 2], s_diff32[kCwaTile / 4 + 2];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t thr = hist[(size_t)st * kCwbWords + kCwbThr];
    const bool filter = thr > thr0;
    const uint4 fact = a.chunk[(size_t)st * a.ntiles + tile];   // {kept bytes, entries before, escapes before, end before}
    const uint32_t seg = o.offsets[st], n = o.offsets[st + 1] - seg;
    const uint64_t fp0 = o.frame_pos[st], fp1 = o.frame_pos[st + 1];
    const bool write = fact.x != 0 && fp1 <= o.capacity;   // (a record that does not fit is skipped whole, by every workgroup alike)
    if (!write && !filter) return;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    if (!cwb_tile<true>(s, (uint8_t *)s_v, a, thr, filter, st, tile, lo, len, lane)) return;
    if (!write) return;
    cwc_emit_tile<true>(s, (uint8_t *)s_code32, (uint8_t *)s_diff32, fact, o, seg, n, fp0, cwire_record_escapes(fp1 - fp0, n), lo, lane);
}

// ---- mi355_(cwire_)activity_batch: where the entries of a stream's records land, as a grid of counts and a box ----------------
// An entry with byte index x < N is a changed byte of pixel p = x / 3, column p % width, row p / width; it counts 1 in cell
// (row / cell_h) * grid_w + column / cell_w of its stream's grid.  Nothing but the records is read.  Behind the directory of the
// nstreams*nframes records:
//   k_act_clear   (skipped when the call accumulates)  : the grids to 0, the summaries to the empty values
//   k_act_tile    (grid: tiles x streams, one wave)    : a tile no record lands in returns on its directory words; the others
//                                                        count their entries per PIXEL in LDS (a tile holds at most 1366 pixels;
//                                                        an LDS atomic per entry, no global one), then fold the pixels to cells:
//                                                        64 consecutive pixels a round, the runs of one cell summed with a scan
//                                                        (indices ascend, so the cells along a row form runs) and ONE global
//                                                        atomic per run; entries and box: a wave reduction, then one atomic per
//                                                        word and tile
//   k_act_summary (grid: streams)                      : active cells, peak and its least index from the finished grid
// The arrays form (k_act_entries) replaces the tile kernel: a lane per entry, its segment by binary search in the offsets as in
// k_apply_multi, equal neighbouring cells merged by the same scan.  It is not tuned further.
// All divisors are uniform across a launch: ActDiv holds floor(2^32 / d), the quotient estimate mulhi(n, m) is at most 1 short
// (n * m / 2^32 > n / d - 1 for every n < 2^32), and one comparison mends it -- exact for every width and cell size.
__device__ __forceinline__ uint32_t act_div(uint32_t n, const ActDiv dv) {
    const uint32_t q = __umulhi(n, dv.m);
    return n - q * dv.d >= dv.d ? q + 1u : q;
}

// The cell of pixel p, and its column and row
__device__ __forceinline__ uint32_t act_cell(uint32_t p, const ActGeom &g, uint32_t &px, uint32_t &py) {
    py = act_div(p, g.width);
    px = p - py * g.width.d;
    return act_div(py, g.cell_h) * g.grid_w + act_div(px, g.cell_w);
}

// c is added to *dst, the lanes of a wave that follow each other with the same dst (a run) by ONE atomic of the run's first lane.
// Every lane of the wave calls; dst == nullptr with c == 0 for a lane that has nothing.
__device__ __forceinline__ void act_add_runs(uint32_t *dst, uint32_t c, int lane) {
    const uint64_t prev = __shfl_up((unsigned long long)(uintptr_t)dst, 1, 64);
    const bool head = lane == 0 || prev != (uint64_t)(uintptr_t)dst;
    const uint64_t heads = __ballot(head);
    const uint32_t incl = wave_inclusive_scan_shfl(c);
    const uint64_t above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);   // the heads of the runs behind this lane's
    const int last = above ? __ffsll((unsigned long long)above) - 2 : 63;          // the run's last lane
    const uint32_t run = (uint32_t)__shfl((int)incl, last, 64) - incl + c;
    if (head && run) atomicAdd(dst, run);
}

// What a lane saw -> the stream's summary words 0 .. 4, one atomic per word by lane 0 (nothing when the wave counted nothing)
struct ActBox {
    uint32_t total = 0, x0 = ~0u, y0 = ~0u, x1 = 0, y1 = 0;
    __device__ __forceinline__ void add(uint32_t c, uint32_t px, uint32_t py) {
        total += c;
        x0 = px < x0 ? px : x0;
        y0 = py < y0 ? py : y0;
        x1 = px > x1 ? px : x1;
        y1 = py > y1 ? py : y1;
    }
    __device__ __forceinline__ void flush(uint32_t *sum, int lane) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) {
            const uint32_t ox0 = __shfl_xor(x0, k, 64), oy0 = __shfl_xor(y0, k, 64), ox1 = __shfl_xor(x1, k, 64), oy1 = __shfl_xor(y1, k, 64);
            total += __shfl_xor(total, k, 64);
            x0 = ox0 < x0 ? ox0 : x0;
            y0 = oy0 < y0 ? oy0 : y0;
            x1 = ox1 > x1 ? ox1 : x1;
            y1 = oy1 > y1 ? oy1 : y1;
        }
        if (lane == 0 && total) {
            atomicAdd(sum + 0, total);
            atomicMin(sum + 1, x0);
            atomicMin(sum + 2, y0);
            atomicMax(sum + 3, x1);
            atomicMax(sum + 4, y1);
        }
    }
};

__global__ __launch_bounds__(256) void k_act_clear(uint32_t *cells, uint32_t *summary, size_t ncells /* of all streams */, uint32_t nstreams) {
    const size_t gid = (size_t)blockIdx.x * 256u + threadIdx.x, step = (size_t)gridDim.x * 256u;
    for (size_t i = gid; i < ncells; i += step) cells[i] = 0u;
    for (size_t i = gid; i < 8 * (size_t)nstreams; i += step) summary[i] = (i & 7u) == 1u || (i & 7u) == 2u ? ~0u : 0u;
}

constexpr uint32_t kActPixels = (kCwaTile + 2) / 3 + 1;   // pixels a tile can touch: byte 4096*t is channel t % 3 of its pixel

__global__ __launch_bounds__(64) void k_act_tile(const CwaArgs a, int nframes, const ActGeom g, uint32_t *cells, uint32_t *summary) {
    __shared__ uint32_t s_cnt[kActPixels];
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    const uint32_t hi = lo + len;
    const uint32_t p0 = lo / 3u, np = (hi - 1u) / 3u - p0 + 1u;   // the tile's pixels: p0 .. p0 + np - 1, np <= kActPixels
    const bool any = cwa_tile_records<false>(
        a, nframes, st, tile, lane,
        [&]() {
            for (uint32_t i = lane; i < kActPixels; i += 64) s_cnt[i] = 0u;
        },
        [&](const CwaFrame &f, const uint4 dr, const CwaBlock b) {
            cwa_walk_record<false>(a, f, dr, b, lo, hi, lane, [&](uint32_t idx, uint8_t) { atomicAdd(&s_cnt[idx / 3u - p0], 1u); });
        });
    if (!any) return;
    uint32_t *grid = cells + (size_t)st * g.cells;
    ActBox box;
    for (uint32_t q0 = 0; q0 < np; q0 += 64) {
        const uint32_t q = q0 + lane;
        const uint32_t c = q < np ? s_cnt[q] : 0u;
        if (!__ballot(c != 0u)) continue;
        uint32_t *dst = nullptr;
        if (q < np) {   // (p < N / 3 = width * height: a cell of the grid, also where c is 0)
            uint32_t px, py;
            dst = grid + act_cell(p0 + q, g, px, py);
            if (c) box.add(c, px, py);
        }
        act_add_runs(dst, c, lane);
    }
    box.flush(summary + 8 * (size_t)st, lane);
}

// lds != 0: the nseg + 1 offsets fit the launch's dynamic LDS (k_apply_multi's rule)
__global__ __launch_bounds__(256) void k_act_entries(const uint32_t *offsets, const int32_t *xs, uint32_t nseg, const ActDiv nframes,
                                                     const ActGeom g, uint32_t *cells, uint32_t *summary, int lds) {
    extern __shared__ uint32_t s_off[];
    const uint32_t *off = offsets;
    if (lds) {
        for (uint32_t j = threadIdx.x; j <= nseg; j += 256) s_off[j] = offsets[j];
        __syncthreads();
        off = s_off;
    }
    const int lane = threadIdx.x & 63;
    const uint32_t first = off[0], end = off[nseg];
    const uint32_t step = gridDim.x * 256u;
    // a wave takes 64 consecutive entries a round, all of its lanes every round (the merge below is a wave operation)
    for (uint64_t base = (uint64_t)first + blockIdx.x * 256u + (threadIdx.x & ~63u); base < end; base += step) {
        const uint64_t i = base + lane;
        const uint32_t x = i < end ? (uint32_t)xs[i] : ~0u;
        const bool live = i < end && x < g.n;
        uint32_t st = 0, px = 0, py = 0;
        uint32_t *dst = nullptr;
        if (live) {
            st = act_div(apply_multi_segment(off, nseg, (uint32_t)i), nframes);
            dst = cells + (size_t)st * g.cells + act_cell(x / 3u, g, px, py);
        }
        act_add_runs(dst, live ? 1u : 0u, lane);
        // entries and box: one set of atomics for the wave when its entries are of one stream, else one per lane
        const uint64_t lives = __ballot(live);
        if (!lives) continue;
        const uint32_t st0 = (uint32_t)__shfl((int)st, __ffsll((unsigned long long)lives) - 1, 64);
        ActBox box;
        if (live) box.add(1u, px, py);
        if (__ballot(live && st != st0)) {
            if (live) {
                uint32_t *sum = summary + 8 * (size_t)st;
                atomicAdd(sum + 0, 1u);
                atomicMin(sum + 1, px);
                atomicMin(sum + 2, py);
                atomicMax(sum + 3, px);
                atomicMax(sum + 4, py);
            }
        } else {
            box.flush(summary + 8 * (size_t)st0, lane);
        }
    }
}

// Words 5 .. 7 of the stream's summary from its grid: cells of at least min_count, the largest count and the least index that has it
__global__ __launch_bounds__(256) void k_act_summary(const uint32_t *cells, uint32_t *summary, uint32_t ncells /* of a stream */,
                                                     uint32_t min_count) {
    __shared__ uint32_t s_active[4];
    __shared__ uint64_t s_best[4];
    const uint32_t *grid = cells + (size_t)blockIdx.x * ncells;
    uint32_t active = 0;
    uint64_t best = 0;   // {count, ~index}: the greatest is the largest count at the least index; 0: no cell counts anything
    for (uint32_t i = threadIdx.x; i < ncells; i += 256) {
        const uint32_t v = grid[i];
        active += v >= min_count ? 1u : 0u;
        const uint64_t key = ((uint64_t)v << 32) | (uint32_t)~i;
        if (v && key > best) best = key;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        active += __shfl_xor(active, k, 64);
        const uint64_t o = __shfl_xor((unsigned long long)best, k, 64);
        if (o > best) best = o;
    }
    if ((threadIdx.x & 63) == 0) {
        s_active[threadIdx.x >> 6] = active;
        s_best[threadIdx.x >> 6] = best;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            active += s_active[w];
            if (s_best[w] > best) best = s_best[w];
        }
        uint32_t *sum = summary + 8 * (size_t)blockIdx.x;
        sum[5] = active;
        sum[6] = (uint32_t)(best >> 32);
        sum[7] = best ? ~(uint32_t)best : 0u;
    }
}

// ---- mi355_cwire_despeckle_cwire_batch: record s of a tick without its isolated changes, the caller's state s reverted there ----
// A pixel is changed when record s holds an entry (nonzero difference, index < N) in one of its three bytes; an entry stays when at
// least need[s] of the 8 pixels around its pixel (inside the frame) changed too.  The budget call with the histogram replaced by
// two bitmaps of one bit per pixel (changed, keep: g.words words per stream each, scratch of the core made on first use).  The
// per-stream word (need) lies in the budget call's rows, as the crop's words do.  Behind the directory of the nstreams records:
//   k_dsp_init  (grid: streams x blocks)          : need -> the stream's row, dropped[s] = 0, the changed bitmap of the streams
//                                                   that are filtered (need != 0) zeroed: nothing of an earlier call is seen
//   k_dsp_mark  (grid: tiles x streams, one wave) : filtered streams only; a tile no entry lands in returns on its directory
//                                                   word.  The tile of differences in LDS (cwc_sum_tile, one record), its changed
//                                                   pixels as bits of at most 44 words in LDS, then ONE global atomic OR per
//                                                   nonzero word: a pixel or a word at a tile's end is shared with the next tile
//   k_dsp_keep  (grid: words x streams)           : a lane per 32 pixels, the bitmap alone: keep = changed & (neighbours >= need),
//                                                   the eight neighbour bitmaps by bit shifts of the changed bitmap (distance 1 and
//                                                   width -1, 0, +1; left / right masked in the first / last column), added bit-
//                                                   parallel into four planes and compared with need.  Every word of the keep
//                                                   bitmap of a filtered stream is written.  N/24 bytes read and written per
//                                                   filtered stream: the only cost of the call that follows N and not the entries
//   k_dsp_facts (grid: tiles x streams, one wave) : k_cwc_sum on the tile with the entries of the pixels not kept zeroed; the
//                                                   dropped entries counted, ONE atomic per tile that drops any
//   k_cwc_scan, k_cwc_place                       : the coalescer's, unchanged
//   k_dsp_emit  (grid: tiles x streams, one wave) : the filtered tile again, from the same bytes; state[x] -= d at the dropped
//                                                   entries, one byte load and one byte store by the lane that owns the byte (the
//                                                   state is touched nowhere else, not even read), also where the record is skipped
//                                                   for lack of room; then k_cwc_emit's tile
// A stream with need == 0 is not filtered: its state and the bitmaps are not touched.  Malformed content: both tile passes filter
// the same tile by the same keep words, so the facts and the record agree; an index >= N and a bad escape contribute nothing.
constexpr uint32_t kDspTileWords = 48;   // bitmap words a tile's pixels span: at most 1367 pixels from bit <= 31 on, 44 words

__global__ __launch_bounds__(256) void k_dsp_init(uint32_t *words, uint32_t *dropped, uint32_t *changed, uint32_t nwords,
                                                  const DspInitArgs h) {
    const uint32_t st = (uint32_t)h.first + blockIdx.x, need = h.need[blockIdx.x];
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        words[(size_t)st * kCwbWords] = need;
        dropped[st] = 0u;
    }
    if (!need) return;
    uint32_t *bm = changed + (size_t)st * nwords;
    for (uint32_t i = blockIdx.y * 256u + threadIdx.x; i < nwords; i += gridDim.y * 256u) bm[i] = 0u;
}

__global__ __launch_bounds__(64) void k_dsp_mark(const CwaArgs a, const uint32_t *words, uint32_t *changed, uint32_t nwords) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    __shared__ uint32_t s_bits[kDspTileWords];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    if (!words[(size_t)st * kCwbWords]) return;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    if (!cwc_sum_tile(s, a, 1, st, tile, lo, lo + len, lane)) return;
    if ((uint32_t)lane < kDspTileWords) s_bits[lane] = 0u;
    __syncthreads();
    const uint32_t wb = lo / 96u;   // the word of the tile's first pixel
    const uint32_t *w = (const uint32_t *)s + 16 * lane;
    uint32_t at = 0, acc = 0;       // the lane's pixels lie in at most two words: one LDS atomic each
    for (int i = 0; i < 16; i++) {
        const uint32_t v = w[i];
        if (!v) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!((v >> (8 * j)) & 255u)) continue;
            const uint32_t p = (lo + 64u * lane + 4u * i + j) / 3u, wi = p / 32u - wb;
            if (wi != at) {
                if (acc) atomicOr(s_bits + at, acc);
                at = wi;
                acc = 0;
            }
            acc |= 1u << (p & 31u);
        }
    }
    if (acc) atomicOr(s_bits + at, acc);
    __syncthreads();
    if ((uint32_t)lane < kDspTileWords && wb + lane < nwords) {
        const uint32_t v = s_bits[lane];
        if (v) atomicOr(changed + (size_t)st * nwords + wb + lane, v);
    }
}

// Bits [32*i + k, 32*i + k + 32) of the bitmap b of nwords words, as one word; bits outside the bitmap are 0
__device__ __forceinline__ uint32_t dsp_bits_at(const uint32_t *b, uint32_t nwords, uint32_t i, int64_t k) {
    const int64_t q = 32 * (int64_t)i + k;
    const int64_t j = q >> 5;   // floor, also below 0
    const uint32_t r = (uint32_t)(q & 31);
    const uint32_t lo = j >= 0 && j < (int64_t)nwords ? b[j] : 0u;
    if (!r) return lo;
    const uint32_t hi = j + 1 >= 0 && j + 1 < (int64_t)nwords ? b[j + 1] : 0u;
    return (lo >> r) | (hi << (32u - r));
}

// x + y + z of three planes of one-bit numbers: the sum's low plane, carry: its high plane
__device__ __forceinline__ uint32_t dsp_add3(uint32_t x, uint32_t y, uint32_t z, uint32_t &carry) {
    const uint32_t t = x ^ y;
    carry = (x & y) | (z & t);
    return t ^ z;
}

__global__ __launch_bounds__(256) void k_dsp_keep(const uint32_t *words, const uint32_t *changed, uint32_t *keep, uint32_t nwords,
                                                  const ActDiv width) {
    const uint32_t st = blockIdx.y, need = words[(size_t)st * kCwbWords];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (!need || i >= nwords) return;
    const uint32_t *b = changed + (size_t)st * nwords;
    uint32_t *out = keep + (size_t)st * nwords;
    const uint32_t c = b[i];
    if (!c) {
        out[i] = 0u;
        return;
    }
    // the word's pixels in the first column (no left neighbours) and in the last (no right ones)
    const uint32_t W = width.d, px0 = 32u * i - act_div(32u * i, width) * W;
    uint32_t first = 0, last = 0;
    for (uint32_t k = px0 ? W - px0 : 0u; k < 32u; k += W) first |= 1u << k;
    for (uint32_t k = W - 1u - px0; k < 32u; k += W) last |= 1u << k;
    const int64_t row = (int64_t)W;
    const uint32_t n0 = dsp_bits_at(b, nwords, i, -row - 1) & ~first, n1 = dsp_bits_at(b, nwords, i, -row),
                   n2 = dsp_bits_at(b, nwords, i, -row + 1) & ~last, n3 = dsp_bits_at(b, nwords, i, -1) & ~first,
                   n4 = dsp_bits_at(b, nwords, i, 1) & ~last, n5 = dsp_bits_at(b, nwords, i, row - 1) & ~first,
                   n6 = dsp_bits_at(b, nwords, i, row), n7 = dsp_bits_at(b, nwords, i, row + 1) & ~last;
    // carry-save: the count of the eight, 0 .. 8, as the planes p3 p2 p1 p0
    uint32_t c0, c1, c2, c3, d0, d1;
    const uint32_t s0 = dsp_add3(n0, n1, n2, c0), s1 = dsp_add3(n3, n4, n5, c1), s2 = dsp_add3(n6, n7, 0u, c2);
    const uint32_t p0 = dsp_add3(s0, s1, s2, c3);
    const uint32_t t = dsp_add3(c0, c1, c2, d0);
    const uint32_t p1 = dsp_add3(t, c3, 0u, d1);
    const uint32_t p2 = d0 ^ d1, p3 = d0 & d1;
    // count >= need, from the top plane down
    const uint32_t plane[4] = {p0, p1, p2, p3};
    uint32_t gt = 0, eq = ~0u;
#pragma unroll
    for (int k = 3; k >= 0; k--) {
        const uint32_t nk = (need >> k) & 1u ? ~0u : 0u;
        gt |= eq & plane[k] & ~nk;
        eq &= ~(plane[k] ^ nk);
    }
    out[i] = c & (gt | eq);
}

// The keep words of the tile's pixels -> s_keep (kDspTileWords words; word 0 holds the pixel of byte lo)
__device__ __forceinline__ void dsp_keep_load(uint32_t *s_keep, const uint32_t *keep, uint32_t nwords, uint32_t st, uint32_t lo, int lane) {
    const uint32_t wb = lo / 96u;
    if ((uint32_t)lane < kDspTileWords) s_keep[lane] = wb + lane < nwords ? keep[(size_t)st * nwords + wb + lane] : 0u;
}

// The lane's 64 bytes of the tile of differences s: the entries of the pixels not kept are zeroed and, REVERT, state[x] -= d is
// stored to g (the tile's place in the state).  Returns the entries zeroed.
template <bool REVERT>
__device__ __forceinline__ uint32_t dsp_lane_bytes(uint8_t *s, const uint32_t *s_keep, uint32_t lo, uint8_t *g, int lane) {
    uint32_t *w = (uint32_t *)s + 16 * lane;
    const uint32_t wb = lo / 96u;
    uint32_t gone = 0;
    for (int i = 0; i < 16; i++) {
        const uint32_t v = w[i];
        if (!v) continue;
        uint32_t keep = v;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t d = (v >> (8 * j)) & 255u;
            if (!d) continue;
            const uint32_t at = 64u * lane + 4u * i + j, p = (lo + at) / 3u;
            if ((s_keep[p / 32u - wb] >> (p & 31u)) & 1u) continue;
            keep &= ~(255u << (8 * j));
            gone++;
            if (REVERT) g[at] = (uint8_t)(g[at] - d);
        }
        w[i] = keep;
    }
    return gone;
}

// The tile of stream st in LDS, filtered where `filter` says so; false: no entry of the record lands in the tile (s untouched).
// gone: the entries the wave dropped.
template <bool REVERT>
__device__ __forceinline__ bool dsp_tile(uint8_t *s, uint32_t *s_keep, const CwaArgs &a, const uint32_t *keep, uint32_t nwords, bool filter,
                                         uint32_t st, uint32_t tile, uint32_t lo, uint32_t len, int lane, uint32_t &gone) {
    gone = 0;
    if (!cwc_sum_tile(s, a, 1, st, tile, lo, lo + len, lane)) return false;
    if (filter) {
        dsp_keep_load(s_keep, keep, nwords, st, lo, lane);
        __syncthreads();
        gone = cwa_wave_sum(dsp_lane_bytes<REVERT>(s, s_keep, lo, a.state + (size_t)st * a.stride + lo, lane));
        __syncthreads();
    }
    return true;
}

__global__ __launch_bounds__(64) void k_dsp_facts(const CwaArgs a, const uint32_t *words, const uint32_t *keep, uint32_t nwords,
                                                  uint32_t *dropped) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    __shared__ uint32_t s_keep[kDspTileWords];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const bool filter = words[(size_t)st * kCwbWords] != 0u;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    uint4 *fact = a.chunk + (size_t)st * a.ntiles + tile;
    uint32_t gone;
    if (!dsp_tile<false>(s, s_keep, a, keep, nwords, filter, st, tile, lo, len, lane, gone)) {
        if (lane == 0) *fact = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4 f = cwc_tile_facts(s, lo, lane);
    if (lane == 0) {
        *fact = f;
        if (gone) atomicAdd(dropped + st, gone);
    }
}

__global__ __launch_bounds__(64) void k_dsp_emit(const CwaArgs a, const CwcOut o, const uint32_t *words, const uint32_t *keep,
                                                 uint32_t nwords) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    __shared__ uint32_t s_keep[kDspTileWords];
    __shared__ uint32_t s_code32[kCwaTile / 4 + 2], s_diff32[kCwaTile / 4 + 2];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const bool filter = words[(size_t)st * kCwbWords] != 0u;
    const uint4 fact = a.chunk[(size_t)st * a.ntiles + tile];   // {kept bytes, entries before, escapes before, end before}
    const uint32_t seg = o.offsets[st], n = o.offsets[st + 1] - seg;
    const uint64_t fp0 = o.frame_pos[st], fp1 = o.frame_pos[st + 1];
    const bool write = fact.x != 0 && fp1 <= o.capacity;   // (a record that does not fit is skipped whole, by every workgroup alike)
    if (!write && !filter) return;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    uint32_t gone;
    if (!dsp_tile<true>(s, s_keep, a, keep, nwords, filter, st, tile, lo, len, lane, gone)) return;
    if (!write) return;
    cwc_emit_tile<true>(s, (uint8_t *)s_code32, (uint8_t *)s_diff32, fact, o, seg, n, fp0, cwire_record_escapes(fp1 - fp0, n), lo, lane);
}

// ---- mi355_cwire_crop_(cwire_)batch: the coalesced records of stream s cut to its rectangle, re-indexed to the rectangle's frame -----
// The coalescer with a filter on the tile, as the budget call is: behind the directory of the nstreams*nframes records
//   k_crop_facts (grid: tiles x streams, one wave) : the rectangles {x0, y0, w, h} of its streams are kernel arguments (kCropStreams
//                                                    per launch); a stream's first tile leaves the six words made of them
//                                                    in the budget call's per-stream rows (the two calls are ordered on one
//                                                    stream) for k_crop_emit.  A tile whose bytes miss the rectangle's rows stores
//                                                    the all-zero fact and reads no record byte; the others sum their records in
//                                                    LDS (cwc_sum_tile), zero the bytes outside the rectangle and take the four
//                                                    facts in MAPPED indices
//   k_cwc_scan, k_cwc_place                        : the coalescer's, unchanged (they see indices, whatever frame they are of)
//   k_crop_emit  (grid: tiles x streams, one wave) : the same tile from the same bytes, its entries written with mapped indices
// The map: byte x of row r = x / 3W, column byte x - r*3W, is byte (r - y0)*3w + column byte - 3*x0 of the rectangle's frame
// = x - r*(3W - 3w) - (y0*3w + 3*x0).  It ascends with x over the kept bytes and never widens a distance, so the lane-local
// reasoning of the coalescer's tile functions holds (CwcIdentity above).  MI355_CROP_KEEP_INDEX: skip = base = 0; a rectangle
// as wide as the frame has skip = 0 too, and no division is made.  Otherwise a lane divides once, for its first byte, and again
// only for a byte of a later row.
struct CropWords {
    uint32_t row0, row1;   // rows [row0, row1) (row0 == row1: nothing is kept)
    uint32_t col0, col1;   // column bytes [col0, col1) of a row
    uint32_t skip, base;   // 3W - 3w, y0*3w + 3*x0
};

__device__ __forceinline__ CropWords crop_words(const CropArgs &h, uint32_t j) {
    const uint32_t x0 = (uint32_t)h.rect[j][0], y0 = (uint32_t)h.rect[j][1], w = (uint32_t)h.rect[j][2], ht = (uint32_t)h.rect[j][3];
    CropWords c;
    c.row0 = y0;
    c.row1 = w ? y0 + ht : y0;   // (no column: no row either, and every tile returns on its rows)
    c.col0 = 3u * x0;
    c.col1 = 3u * (x0 + w);
    c.skip = h.keep_index ? 0u : h.row_bytes - 3u * w;
    c.base = h.keep_index ? 0u : y0 * 3u * w + 3u * x0;
    return c;
}

struct CropMap {
    ActDiv row;            // bytes of a full row, 3W
    uint32_t skip, base;
    uint32_t shift0, next;   // of the row r0 of the lane's first byte: r0*skip + base, and the first byte of the row behind it
    __device__ __forceinline__ CropMap(const ActDiv row_, const CropWords &c, uint32_t r0)
        : row(row_), skip(c.skip), base(c.base), shift0(r0 * c.skip + c.base), next((r0 + 1u) * row_.d) {}
    // x: a byte of the lane, so never before its first
    __device__ __forceinline__ uint32_t operator()(uint32_t x) const {
        if (skip == 0u) return x - base;   // (uniform)
        return x < next ? x - shift0 : x - act_div(x, row) * skip - base;
    }
};

// Stream st's summed tile [lo, lo + len) in LDS with the bytes outside its rectangle zeroed; false: the tile misses the
// rectangle's rows (no record byte was read) or no record has an entry in it, and s was not touched.  r0: the row of the lane's
// first byte, lo + 64*lane.
__device__ __forceinline__ bool crop_tile(uint8_t *s, const CwaArgs &a, int nframes, const CropWords &c, uint32_t rb, uint32_t r0,
                                          uint32_t st, uint32_t tile, uint32_t lo, uint32_t len, int lane) {
    // rows [row0, row1) are bytes [rb*row0, rb*row1) of the frame, at most N < 2^32
    const uint32_t last = lo + (len - 1u);
    if (c.row0 >= c.row1 || last < rb * c.row0 || lo >= rb * c.row1) return false;
    if (!cwc_sum_tile(s, a, nframes, st, tile, lo, lo + len, lane)) return false;
    if (c.col0 == 0u && c.col1 == rb && lo >= rb * c.row0 && last < rb * c.row1) return true;   // every byte of the tile is kept
    // the lane's 64 bytes, row by row (several rows when 3W < 64, a part of one when 3W > 64): bit p of keep = byte p stays.
    // Bytes past the frame's end are 0 already, whatever the mask says of them.
    uint32_t r = r0, col = lo + 64u * lane - r0 * rb;   // col < rb
    uint64_t keep = 0;
    for (uint32_t p = 0; p < 64u; r++, col = 0u) {
        const uint32_t seg = rb - col < 64u - p ? rb - col : 64u - p;   // >= 1
        if (r >= c.row0 && r < c.row1) {
            const uint32_t k0 = col > c.col0 ? col : c.col0, k1 = col + seg < c.col1 ? col + seg : c.col1;
            if (k0 < k1) {
                const uint32_t cnt = k1 - k0;   // <= 64
                keep |= (cnt == 64u ? ~0ull : (1ull << cnt) - 1ull) << (p + k0 - col);
            }
        }
        p += seg;
    }
    if (keep != ~0ull) {
        uint32_t *w = (uint32_t *)s + 16 * lane;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t nib = (uint32_t)(keep >> (4 * i)) & 15u;
            if (nib == 15u) continue;
            w[i] &= ((nib & 1u) ? 0xffu : 0u) | ((nib & 2u) ? 0xff00u : 0u) | ((nib & 4u) ? 0xff0000u : 0u) | ((nib & 8u) ? 0xff000000u : 0u);
        }
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(64) void k_crop_facts(const CwaArgs a, int nframes, uint32_t *words, const CropArgs h, const ActDiv row) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles, st = (uint32_t)h.first + j;
    const CropWords c = crop_words(h, j);
    if (tile == 0 && lane == 0) {
        uint32_t *rw = words + (size_t)st * kCwbWords;
        rw[0] = c.row0, rw[1] = c.row1, rw[2] = c.col0, rw[3] = c.col1, rw[4] = c.skip, rw[5] = c.base;
    }
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    const uint32_t r0 = act_div(lo + 64u * lane, row);
    uint4 *fact = a.chunk + (size_t)st * a.ntiles + tile;
    if (!crop_tile(s, a, nframes, c, row.d, r0, st, tile, lo, len, lane)) {
        if (lane == 0) *fact = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4 f = cwc_tile_facts(s, lo, lane, CropMap(row, c, r0));
    if (lane == 0) *fact = f;
}

template <bool CWIRE>
__global__ __launch_bounds__(64) void k_crop_emit(const CwaArgs a, const CwcOut o, int nframes, const uint32_t *words, const ActDiv row) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    __shared__ uint32_t s_code32[CWIRE ? kCwaTile / 4 + 2 : 1], s_diff32[kCwaTile / 4 + 2];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint4 fact = a.chunk[(size_t)st * a.ntiles + tile];   // {kept bytes, entries before, escapes before, mapped end before}
    const uint32_t *rw = words + (size_t)st * kCwbWords;         // (loaded beside the fact, not behind it)
    const CropWords c{rw[0], rw[1], rw[2], rw[3], rw[4], rw[5]};
    if (fact.x == 0) return;
    const uint32_t seg = o.offsets[st], n = o.offsets[st + 1] - seg;
    uint64_t fp0 = 0;
    uint32_t e = 0;
    if (CWIRE) {
        fp0 = o.frame_pos[st];
        const uint64_t fp1 = o.frame_pos[st + 1];
        if (fp1 > o.capacity) return;   // the record does not fit: skipped whole, by every workgroup alike
        e = cwire_record_escapes(fp1 - fp0, n);
    }
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    const uint32_t r0 = act_div(lo + 64u * lane, row);
    if (!crop_tile(s, a, nframes, c, row.d, r0, st, tile, lo, len, lane)) return;   // (the facts say otherwise)
    cwc_emit_tile<CWIRE>(s, (uint8_t *)s_code32, (uint8_t *)s_diff32, fact, o, seg, n, fp0, e, lo, lane, CropMap(row, c, r0));
}

// ---- mi355_cwire_mosaic_(cwire_)batch: the coalesced records of nstreams cameras placed on a canvas, ONE record out ------------
// The opposite of the crop: the tile grid runs over the CANVAS (Nc = 3 * canvas_w * canvas_h bytes, cwa_tiles(Nc) tiles) and a tile
// gathers from every stream whose destination it meets.  Behind the directory of the nstreams*nframes records:
//   k_mosaic_table (one workgroup per launch)        : the placements {sx, sy, w, h, dx, dy} are kernel arguments (kMosaicStreams
//                                                      per launch) and become six words per stream in the budget call's per-stream
//                                                      rows (the two calls are ordered on one stream): the destination's rows and
//                                                      column bytes on the canvas, the source's first row and column byte
//   k_mosaic_facts (grid: canvas tiles, one wave)    : lanes test 64 streams a round -- do the tile's rows meet the destination's,
//                                                      and does the tile hold a byte of its columns -- and take the source byte
//                                                      range [slo, shi) the tile's bytes come from; per hit, lanes test 64 records
//                                                      a round on the directory words of the source tiles that range meets; per
//                                                      record with an entry there, ONE walk (cwa_walk_record from the first source
//                                                      tile's directory word) whose op keeps the entries of the source rectangle
//                                                      and adds them at their canvas byte into a ZEROED tile in LDS.  A barrier
//                                                      stands between walks: two streams (or two records) may hit one byte, the
//                                                      entries of one record never do.  A tile nothing lands in stores the
//                                                      all-zero fact, the others cwc_tile_facts: the tile is in canvas indices
//                                                      already, so the map is the identity
//   k_cwc_scan, k_cwc_place                          : the coalescer's, unchanged, for ONE stream of cwa_tiles(Nc) tiles
//   k_mosaic_emit  (grid: canvas tiles, one wave)    : the same tile from the same bytes, its entries written by cwc_emit_tile
// The facts live where the coalescer's do (the chunk scratch, max_batch * cwa_chunks(N) words: the caller refuses a canvas of more
// tiles).  Source byte x of row r = x / 3W, column byte c = x - r*3W, is canvas byte (r - sy + dy) * 3*canvas_w + c - 3*sx + 3*dx:
// the row comes from the exact multiply-and-correct division of the motion grid (act_div), once per kept entry of a walk.  The walk
// range is exact in its first and last row and spans whole source rows between them, so a canvas narrower than the source frame
// walks over entries it drops; the op decides.  Malformed content: the walk's own guarantees (nothing read outside the record,
// no index at or past N), and both tile kernels build the same tile from the same bytes, so facts and record agree.
struct MosaicWords {
    uint32_t drow0, drow1;   // canvas rows [drow0, drow1) (drow0 == drow1: nothing is placed)
    uint32_t dcol0, dcol1;   // canvas column bytes [dcol0, dcol1) of a row
    uint32_t srow0, scol0;   // the source's first row and column byte
};

__global__ __launch_bounds__(kMosaicStreams) void k_mosaic_table(uint32_t *words, const MosaicArgs h) {
    const int j = threadIdx.x;
    if (j >= h.count) return;
    const uint32_t sx = (uint32_t)h.place[j][0], sy = (uint32_t)h.place[j][1], w = (uint32_t)h.place[j][2], ht = (uint32_t)h.place[j][3];
    const uint32_t dx = (uint32_t)h.place[j][4], dy = (uint32_t)h.place[j][5];
    uint32_t *rw = words + (size_t)(h.first + j) * kCwbWords;
    rw[0] = dy, rw[1] = w ? dy + ht : dy;   // (no column: no row either)
    rw[2] = 3u * dx, rw[3] = 3u * (dx + w);
    rw[4] = sy, rw[5] = 3u * sx;
}

// The canvas tile [lo, lo + len) in LDS (s: kCwaTile bytes; s[0] is canvas byte lo): the sum over the streams that cover a byte of
// their summed differences there.  false: nothing lands in the tile and s was not touched.  rs: 3W, rc: 3 * canvas_w.
__device__ __forceinline__ bool mosaic_tile(uint8_t *s, const CwaArgs &a, int nstreams, int nframes, const uint32_t *words,
                                            const ActDiv rs, const ActDiv rc, uint32_t lo, uint32_t len, int lane) {
    const uint32_t last = lo + (len - 1u);
    const uint32_t R0 = act_div(lo, rc), R1 = act_div(last, rc);     // the tile's first and last canvas row
    const uint32_t q0 = lo - R0 * rc.d, q1 = last - R1 * rc.d;       // column bytes of its first and last byte
    bool any = false;
    for (int sb = 0; sb < nstreams; sb += 64) {
        // the source bytes [slo, shi) that the tile's bytes of stream sb + lane come from (empty: the tile misses its destination)
        uint32_t slo = 0, shi = 0;
        if (sb + lane < nstreams) {
            const uint32_t *rw = words + (size_t)(sb + lane) * kCwbWords;
            const MosaicWords p{rw[0], rw[1], rw[2], rw[3], rw[4], rw[5]};
            uint32_t ra = R0 > p.drow0 ? R0 : p.drow0, rb = R1 + 1u < p.drow1 ? R1 + 1u : p.drow1;   // rows [ra, rb)
            // the tile's bytes of its first row may all lie behind the columns, those of its last row all before them
            if (ra < rb && ra == R0 && q0 >= p.dcol1) ra++;
            if (ra < rb && rb - 1u == R1 && q1 < p.dcol0) rb--;
            if (ra < rb && p.dcol0 < p.dcol1) {
                const uint32_t c0 = ra == R0 && q0 > p.dcol0 ? q0 : p.dcol0;
                const uint32_t c1 = rb - 1u == R1 && q1 + 1u < p.dcol1 ? q1 + 1u : p.dcol1;
                slo = (p.srow0 + (ra - p.drow0)) * rs.d + p.scol0 + (c0 - p.dcol0);
                shi = (p.srow0 + (rb - 1u - p.drow0)) * rs.d + p.scol0 + (c1 - p.dcol0);
            }
        }
        uint64_t hits = __ballot(slo < shi);
        for (; hits; hits &= hits - 1ull) {
            const int js = __ffsll((unsigned long long)hits) - 1;
            const uint32_t st = (uint32_t)(sb + js);
            const uint32_t ulo = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)slo, js, 64));
            const uint32_t uhi = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)shi, js, 64));
            const uint32_t *rw = words + (size_t)st * kCwbWords;
            const MosaicWords p{rw[0], rw[1], rw[2], rw[3], rw[4], rw[5]};
            const uint32_t ft = ulo / kCwaTile, lt = (uhi - 1u) / kCwaTile;   // the source tiles the range meets
            const size_t b0 = (size_t)st * nframes;                           // the stream's first batch index
            for (int base = 0; base < nframes; base += 64) {
                bool touch = false;
                if (base + lane < nframes) {
                    const size_t b = b0 + base + lane;
                    const uint32_t fn = a.ftab[b].n;
                    const uint4 *dir = a.dir + b * a.ntiles;
                    const uint32_t k0 = dir[ft].x, kend = lt + 1u < a.ntiles ? dir[lt + 1u].x : fn;
                    touch = k0 < kend && k0 < fn;
                }
                const uint64_t set = __ballot(touch);
                if (!set) continue;
                if (!any) {
                    for (uint32_t i = lane; i < kCwaTile / 16; i += 64) ((cwa_u32x4 *)s)[i] = cwa_u32x4{0u, 0u, 0u, 0u};
                    any = true;
                }
                const int cnt = nframes - base < 64 ? nframes - base : 64;
                // while record j is walked, the header, directory word and first block of the set's next record are in flight
                int jn = __ffsll((unsigned long long)set) - 1;
                CwaFrame f1 = a.ftab[b0 + base + jn];
                uint4 d1 = a.dir[(b0 + base + jn) * a.ntiles + ft];
                CwaBlock b1 = cwa_block_load(a, f1, d1.x, lane);
                __syncthreads();
                while (jn < cnt) {
                    const int j = jn;
                    const CwaFrame f = f1;
                    const uint4 dr = d1;
                    const CwaBlock blk = b1;
                    const uint64_t rest = set & ~((2ull << j) - 1ull);   // (j = 63: 2 << 63 is 0, rest = 0)
                    jn = rest ? __ffsll((unsigned long long)rest) - 1 : cnt;
                    if (jn < cnt) {
                        f1 = a.ftab[b0 + base + jn];
                        d1 = a.dir[(b0 + base + jn) * a.ntiles + ft];
                        b1 = cwa_block_load(a, f1, d1.x, lane);
                    }
                    cwa_walk_record<true>(a, f, dr, blk, ulo, uhi, lane, [=](uint32_t idx, uint8_t d) {
                        const uint32_t r = act_div(idx, rs), col = idx - r * rs.d;
                        if (r < p.srow0 || col < p.scol0) return;
                        const uint32_t R = r - p.srow0 + p.drow0, q = col - p.scol0 + p.dcol0;
                        if (R >= p.drow1 || q >= p.dcol1) return;
                        const uint32_t y = R * rc.d + q;   // < Nc
                        if (y < lo || y - lo >= len) return;
                        s[y - lo] = (uint8_t)(s[y - lo] + d);
                    });
                    __syncthreads();
                }
            }
        }
    }
    return any;
}

__global__ __launch_bounds__(64) void k_mosaic_facts(const CwaArgs a, int nstreams, int nframes, const uint32_t *words, const ActDiv rs,
                                                     const ActDiv rc, uint32_t nc) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = nc - lo < kCwaTile ? nc - lo : kCwaTile;
    uint4 *fact = a.chunk + tile;
    if (!mosaic_tile(s, a, nstreams, nframes, words, rs, rc, lo, len, lane)) {
        if (lane == 0) *fact = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4 f = cwc_tile_facts(s, lo, lane);
    if (lane == 0) *fact = f;
}

template <bool CWIRE>
__global__ __launch_bounds__(64) void k_mosaic_emit(const CwaArgs a, const CwcOut o, int nstreams, int nframes, const uint32_t *words,
                                                    const ActDiv rs, const ActDiv rc, uint32_t nc) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    __shared__ uint32_t s_code32[CWIRE ? kCwaTile / 4 + 2 : 1], s_diff32[kCwaTile / 4 + 2];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const uint4 fact = a.chunk[tile];   // {nonzero bytes, entries before, escapes before, end before}
    if (fact.x == 0) return;
    const uint32_t seg = o.offsets[0], n = o.offsets[1] - seg;
    uint64_t fp0 = 0;
    uint32_t e = 0;
    if (CWIRE) {
        fp0 = o.frame_pos[0];
        const uint64_t fp1 = o.frame_pos[1];
        if (fp1 > o.capacity) return;   // the record does not fit: skipped whole, by every workgroup alike
        e = cwire_record_escapes(fp1 - fp0, n);
    }
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = nc - lo < kCwaTile ? nc - lo : kCwaTile;
    if (!mosaic_tile(s, a, nstreams, nframes, words, rs, rc, lo, len, lane)) return;   // (the facts say otherwise)
    cwc_emit_tile<CWIRE>(s, (uint8_t *)s_code32, (uint8_t *)s_diff32, fact, o, seg, n, fp0, e, lo, lane);
}

// ---- mi355_cwire_check_batch: one verdict of four words per record, from the records alone (include/mi355diff.h) ---------------
// The chunk table of the directory (k_cwa_table, k_cwa_facts, k_cwa_scan field 0: per chunk of kCwaChunk codes the 255 codes, the
// sum of g + 1 over the others -- at most 4096 * 255, it cannot wrap -- and the chunk's first escape rank), then two kernels of
// its own, in which NO sum wraps: everything that can reach 2^32 is added in 64 bits and travels through the 32-bit chunk word
// clamped to 0xFFFFFFFF.  Clamped addition of non-negative values is associative, so a prefix of clamped chunk sums, clamped,
// is the clamped true prefix: exact below 2^32, stuck at the top above it -- all that a comparison with N < 2^32 - 1 needs.
//   k_cwk_escsum (grid: chunks)  : + esc[r] + 1 for the chunk's ranks r < e, clamped; a used escape value < 255 and, in the
//                                  record's last chunk, a nonzero pad byte of either section are noted in bits 16, 17 of chunk.x
//   k_cwk_finish (grid: records) : scans the record's chunk sums (64-bit), which gives the total and the one chunk whose inclusive
//                                  prefix is the first above N; walks that chunk with the decode step of the GPU clients for the
//                                  least such entry; compares the header words; lane 0 stores the four words
// No workgroup waits on another; nothing is written but the core's chunk scratch and the verdicts; reads stay inside
// [pos, pos + record bytes) of every record: code dwords below pad4(n) / 4, escape words below e, the two header words.
constexpr uint32_t kCwkPadBit = 1u << 16, kCwkLowBit = 1u << 17;   // beside the chunk's count of 255 codes (<= 4096) in chunk.x
// the verdict's flags (MI355_CWIRE_BAD_* of include/mi355diff.h)
constexpr uint32_t kCwkBadCodes = 1u, kCwkBadRange = 2u, kCwkBadPad = 4u, kCwkBadEscape = 8u, kCwkBadHeader = 16u;

__global__ __launch_bounds__(256) void k_cwk_escsum(const CwaArgs a) {
    __shared__ uint64_t s_sum[4];
    __shared__ uint32_t s_low[4];
    const uint32_t c = blockIdx.x;
    const uint4 ch = a.chunk[c];
    const CwaFrame f = a.ftab[ch.w];
    const uint32_t r0 = ch.y < f.e ? ch.y : f.e;
    const uint32_t r1 = f.e - r0 < ch.x ? f.e : r0 + ch.x;
    const CwireSections<const uint8_t> sec = cwa_sections(a, f);
    const uint32_t *esc = sec.esc32();
    uint64_t sum = 0;
    bool low = false;
    for (uint32_t r = r0 + threadIdx.x; r < r1; r += 256) {
        const uint32_t g = esc[r];
        sum += (uint64_t)g + 1u;
        low = low || g < 255u;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) sum += __shfl_xor((unsigned long long)sum, k, 64);
    const uint64_t lows = __ballot(low);
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_low[threadIdx.x >> 6] = lows ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t total = (uint64_t)ch.z + s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];   // <= 4096 * 2^32
        uint32_t bits = (s_low[0] | s_low[1] | s_low[2] | s_low[3]) ? kCwkLowBit : 0u;
        if (c - f.cbase + 1 == f.nc && (f.n & 3u)) {   // the pad bytes: the top of the last dword of either section
            const uint32_t d = f.n / 4u, used = 8u * (f.n & 3u);
            if ((sec.code32()[d] | sec.diff32()[d]) >> used) bits |= kCwkPadBit;
        }
        a.chunk[c].x = ch.x | bits;
        a.chunk[c].z = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;
    }
}

__global__ __launch_bounds__(256) void k_cwk_finish(const CwaArgs a, uint32_t *verdicts) {
    __shared__ uint64_t s_pre[2][4], s_sum[2][4], s_before;
    __shared__ uint32_t s_esc[2][4], s_chunk, s_rank, s_bits, s_cnt, s_k;
    const uint32_t b = blockIdx.x;
    const CwaFrame f = a.ftab[b];
    if (threadIdx.x == 0) {
        s_chunk = ~0u;
        s_bits = 0u;
        s_cnt = 0u;
        s_k = f.n;
    }
    __syncthreads();
    // the record's chunks: 255 codes, flag bits, and the prefix of the clamped sums
    uint64_t total = 0;
    uint32_t bits = 0, cnt = 0;
    int buf = 0;
    for (uint32_t i0 = 0; i0 < f.nc; i0 += 256, buf ^= 1) {
        const uint32_t i = i0 + threadIdx.x;
        const uint4 ch = i < f.nc ? a.chunk[f.cbase + i] : make_uint4(0u, 0u, 0u, 0u);
        const uint64_t before = block_exclusive_scan<4>((uint64_t)ch.z, s_pre[buf], total);
        bits |= ch.x >> 16;
        cnt += ch.x & 0xffffu;
        // prefixes only grow: at most one chunk starts at or below N and ends above it
        if (i < f.nc && before <= a.n && before + ch.z > a.n) {
            s_chunk = i;
            s_before = before;
            s_rank = ch.y;
        }
    }
    if (bits) atomicOr(&s_bits, bits);
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    const uint32_t ci = s_chunk;
    if (ci != ~0u) {   // that chunk once more, for the least k with X_k > N
        const uint32_t k0 = ci * kCwaChunk;
        const uint32_t k1 = f.n - k0 < kCwaChunk ? f.n : k0 + kCwaChunk;
        const CwireSections<const uint8_t> sec = cwa_sections(a, f);
        const uint32_t *code = sec.code32(), *esc = sec.esc32();
        uint32_t carry_e = s_rank;
        uint64_t carry_x = s_before;
        for (uint32_t base = k0; base < k1; base += 1024, buf ^= 1) {
            const uint32_t d = base / 4 + threadIdx.x;
            const bool live = 4 * d < k1;
            const uint32_t word = live ? code[d] : 0u;
            bool in[4], fl[4];
#pragma unroll
            for (int j = 0; j < 4; j++) in[j] = live && 4 * d + j < k1;
            uint32_t wtot;
            const uint32_t before = cwire_escapes_before(word, in, fl, wtot);
            const uint32_t rank = block_waves_before<4>(wtot, 0, s_esc[buf], carry_e) + before;
            uint32_t inc[4], rk[4];
            bool bad[4];
            cwire_decode4(word, in, fl, rank, f.e, esc, inc, bad, rk);
            // a live entry that is not a bad escape adds g + 1 >= 1: an increment of 0 is 0xFFFFFFFF + 1 wrapped
            uint64_t inc64[4], lsum = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                inc64[j] = in[j] && !bad[j] && inc[j] == 0u ? 0x100000000ull : inc[j];
                lsum += inc64[j];
            }
            uint64_t x = block_exclusive_scan<4>(lsum, s_sum[buf], carry_x);
            uint32_t mine = ~0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                x += inc64[j];
                if (in[j] && x > a.n && mine == ~0u) mine = 4 * d + j;
            }
            if (mine != ~0u) atomicMin(&s_k, mine);
            if (carry_x > a.n) break;   // (the same for every thread) the entry is in this round
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t *hdr = (const uint32_t *)(a.cwire + f.pos);
        const uint32_t n255 = s_cnt, k = s_k, sb = s_bits;
        uint32_t w0 = 0;
        if (n255 != f.e) w0 |= kCwkBadCodes;
        if (k < f.n) w0 |= kCwkBadRange;
        if (sb & (kCwkPadBit >> 16)) w0 |= kCwkBadPad;
        if (sb & (kCwkLowBit >> 16)) w0 |= kCwkBadEscape;
        if (hdr[0] != f.n || hdr[1] != f.e) w0 |= kCwkBadHeader;
        uint32_t *v = verdicts + 4 * (size_t)b;
        v[0] = w0;
        v[1] = n255;
        v[2] = k;
        v[3] = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;
    }
}

// ---- mi355_state_digest_batch, mi355_refresh_cwire_batch, mi355_state_clear_tiles_batch: resynchronising a receiver ------------
// The digest of a tile (include/mi355diff.h, mi355_state_digest_host, is the definition): the tile extended with zero bytes to
// kCwaTile bytes, read as 1024 little-endian words w_i: {sum of w_i, sum of rf_mix(w_i ^ kRfGolden * (i + 1))}, both mod 2^32.
// Both sums commute, so a lane folds whichever words it holds and the wave adds the lanes.
//   k_state_digest      (grid: tiles x streams, one wave) : a whole tile at a 16-byte aligned address: four 16-byte loads per lane
//                                                           (quad 64*i + lane: each load of the wave is 1 KiB in one piece);
//                                                           any other tile through LDS (cwa_tile_load, the rest zeroed)
//   k_rf_facts          (grid: tiles x streams, one wave) : the sender's tile in LDS, its digest against the peer's (no peer: every
//                                                           tile is selected); a selected tile: its mask bit (one atomic OR
//                                                           into words cleared on the same stream) and cwc_tile_facts of its
//                                                           bytes, any other the all-zero fact -- an empty tile to what follows
//   k_cwc_scan<true>, k_cwc_place<true>                   : the coalescer's, unchanged
//   k_rf_emit           (grid: tiles x streams, one wave) : k_cwc_emit with the tile loaded from the state again
//   k_state_clear_tiles (grid: tiles x streams, one wave) : zeroes the tiles whose mask bit is set: bytes up to the first 16-byte
//                                                           boundary, whole 16-byte stores, bytes behind the last
// The refresh record of a stream holds (x, state[x]) for the nonzero bytes of its selected tiles: applied to a state whose
// selected tiles are zero it makes them the sender's, whichever client applies it.
constexpr uint32_t kRfGolden = 0x9E3779B9u;

__device__ __forceinline__ uint32_t rf_mix(uint32_t v) {
    v ^= v >> 16;
    v *= 0x85EBCA6Bu;
    v ^= v >> 13;
    v *= 0xC2B2AE35u;
    v ^= v >> 16;
    return v;
}

// quad q of a tile (its words 4q .. 4q + 3) added to a lane's two sums
__device__ __forceinline__ void rf_fold(const cwa_u32x4 v, uint32_t q, uint32_t &sum, uint32_t &mix) {
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        sum += v[j];
        mix += rf_mix(v[j] ^ (kRfGolden * (4u * q + j + 1u)));
    }
}

// The digest of the kCwaTile bytes at s (LDS), in every lane.  One wave.
__device__ __forceinline__ uint2 rf_digest_lds(const uint8_t *s, int lane) {
    uint32_t sum = 0, mix = 0;
#pragma unroll
    for (uint32_t i = 0; i < kCwaTile / 1024; i++) rf_fold(((const cwa_u32x4 *)s)[64 * i + lane], 64 * i + lane, sum, mix);
    return make_uint2(cwa_wave_sum(sum), cwa_wave_sum(mix));
}

// len bytes at src -> s (LDS, kCwaTile bytes), the bytes past len zero: LDS holds whatever the previous workgroup left there.
// One wave; the tile is complete for every lane on return.
__device__ __forceinline__ void rf_tile_load(uint8_t *s, const uint8_t *src, uint32_t len, int lane) {
    if (len < kCwaTile) {
        for (uint32_t i = lane; i < kCwaTile / 16; i += 64) ((cwa_u32x4 *)s)[i] = cwa_u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
    }
    cwa_tile_load(s, src, len, lane);
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_state_digest(const uint8_t *states, size_t stride, uint32_t n, uint32_t ntiles,
                                                     uint32_t *digests) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = n - lo < kCwaTile ? n - lo : kCwaTile;
    const uint8_t *src = states + (size_t)st * stride + lo;
    uint2 d;
    if (len == kCwaTile && !((uintptr_t)src & 15u)) {   // (the same for every lane)
        cwa_u32x4 v[kCwaTile / 1024];
#pragma unroll
        for (uint32_t i = 0; i < kCwaTile / 1024; i++) v[i] = __builtin_nontemporal_load((const cwa_u32x4 *)src + 64 * i + lane);
        uint32_t sum = 0, mix = 0;
#pragma unroll
        for (uint32_t i = 0; i < kCwaTile / 1024; i++) rf_fold(v[i], 64 * i + lane, sum, mix);
        d = make_uint2(cwa_wave_sum(sum), cwa_wave_sum(mix));
    } else {
        rf_tile_load((uint8_t *)s_q, src, len, lane);
        d = rf_digest_lds((const uint8_t *)s_q, lane);
    }
    if (lane == 0) {
        uint32_t *out = digests + 2 * ((size_t)st * ntiles + tile);   // (4-byte aligned, no more)
        out[0] = d.x;
        out[1] = d.y;
    }
}

__global__ __launch_bounds__(64) void k_rf_facts(const CwaArgs a, const uint32_t *peer, uint32_t *mask, uint32_t mask_words) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    const size_t t = (size_t)st * a.ntiles + tile;
    rf_tile_load(s, a.state + (size_t)st * a.stride + lo, len, lane);
    bool selected = true;   // (the same for every lane)
    if (peer) {
        const uint2 d = rf_digest_lds(s, lane);
        selected = peer[2 * t] != d.x || peer[2 * t + 1] != d.y;
    }
    uint4 f = make_uint4(0u, 0u, 0u, 0u);
    if (selected) {
        f = cwc_tile_facts(s, lo, lane);
        if (lane == 0) atomicOr(mask + (size_t)st * mask_words + (tile >> 5), 1u << (tile & 31u));
    }
    if (lane == 0) a.chunk[t] = f;
}

__global__ __launch_bounds__(64) void k_rf_emit(const CwaArgs a, const CwcOut o) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16];
    __shared__ uint32_t s_code32[kCwaTile / 4 + 2], s_diff32[kCwaTile / 4 + 2];
    uint8_t *s = (uint8_t *)s_q;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint4 fact = a.chunk[(size_t)st * a.ntiles + tile];   // {nonzero bytes, entries before, escapes before, end before}
    if (fact.x == 0) return;   // not selected, or no nonzero byte
    const uint32_t seg = o.offsets[st], n = o.offsets[st + 1] - seg;
    const uint64_t fp0 = o.frame_pos[st], fp1 = o.frame_pos[st + 1];
    if (fp1 > o.capacity) return;   // the record does not fit: skipped whole, by every workgroup alike
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    rf_tile_load(s, a.state + (size_t)st * a.stride + lo, len, lane);
    cwc_emit_tile<true>(s, (uint8_t *)s_code32, (uint8_t *)s_diff32, fact, o, seg, n, fp0, cwire_record_escapes(fp1 - fp0, n), lo, lane);
}

__global__ __launch_bounds__(64) void k_state_clear_tiles(uint8_t *states, size_t stride, uint32_t n, uint32_t ntiles,
                                                          const uint32_t *mask, uint32_t mask_words) {
    const uint32_t lane = threadIdx.x;
    const uint32_t st = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    if (!((mask[(size_t)st * mask_words + (tile >> 5)] >> (tile & 31u)) & 1u)) return;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = n - lo < kCwaTile ? n - lo : kCwaTile;
    uint8_t *dst = states + (size_t)st * stride + lo;
    const uint32_t to16 = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
    const uint32_t head = to16 < len ? to16 : len;
    const uint32_t q = (len - head) / 16u, tail = head + 16u * q;   // len - tail < 16
    if (lane < head) dst[lane] = 0;
    for (uint32_t i = lane; i < q; i += 64) ((cwa_u32x4 *)(dst + head))[i] = cwa_u32x4{0u, 0u, 0u, 0u};
    if (lane < len - tail) dst[tail + lane] = 0;
}

// ---- mi355_wall_compose_batch, mi355_cwire_touched_tiles_batch: a wall of many cameras ------------------------------------------
// The thumbnail of a state at scale k (include/mi355diff.h is the definition): pixel (u, v), channel c is the rounded mean
// floor((sum + floor(a / 2)) / a) of the a <= k*k source bytes of its block, the blocks at the right and bottom edges smaller.
//   k_wall_compose (grid: (rows x column chunks, streams of the launch), 256 threads) : a workgroup owns up to wall_chunk_pixels(k)
//       pixels of ONE thumbnail row: a band of kh <= k source rows, each a contiguous range of at most kWallBytes bytes of the state.
//       With a mask it first asks whether a tile that one of those ranges meets is selected and returns if none is -- no state
//       byte moves for a still camera, and a selected tile repaints whole chunks, which the call is allowed to.  Thread j
//       then owns bytes [16j, 16j + 16) of every range: one 16-byte load per row where the row's address allows it (bytes
//       otherwise, and at the ragged end), added vertically as 16-bit sums packed two to a register (16 * 255 < 2^16), the
//       sums to LDS.  Output byte o = 3u + c of the chunk is then the sum of kw LDS entries at a 3-entry pitch; consecutive
//       threads take consecutive o, so the 16-bit LDS reads of a wave's step lie k entries apart on average (not 4k, as with
//       four bytes per thread) and its 64 one-byte stores are one 64-byte piece of the wall row.  One integer division per
//       output byte.
//   k_cw_touched   (grid: ceil(tiles / 64) x streams, one wave) : behind the directory; lane = tile, the touch test of
//       k_cwa_apply_multi_stream ORed over the stream's nframes records, a ballot, two mask words per wave stored by lane 0
//       (ORed onto what is there when accumulating: one wave owns the two words)
constexpr uint32_t kWallBytes = 4096;   // source bytes of one row per workgroup: 256 threads x 16

struct WallBand {
    const uint8_t *src;   // byte 0 of the band's first row inside the chunk
    uint32_t pitch;       // bytes between the band's rows (3 * width)
    uint32_t kh, cb;      // rows of the band, bytes per row of the chunk
};

// true: a selected tile of mask (the stream's row) meets one of the band's ranges; off: the band's first byte in the state
__device__ __forceinline__ bool wall_band_selected(const uint32_t *mask, uint32_t off, const WallBand &b) {
    bool any = false;
    for (uint32_t r = 0; r < b.kh; r++) {
        const uint32_t lo = off + r * b.pitch;
        for (uint32_t t = lo / kCwaTile; t <= (lo + b.cb - 1u) / kCwaTile; t++) any |= (mask[t >> 5] >> (t & 31u)) & 1u;
    }
    return any;
}

// The band sum, shared by k_wall_compose and the thumbnail records' kernels.  G column groups per thread, `step` bytes apart: bytes
// [c0 + g * step, + 16) of every row of the band added vertically, sixteen 16-bit sums in byte order per group, w0[g] those of bytes
// 0 .. 7 and w1[g] of bytes 8 .. 15; the bytes at or past b.cb count as zero.  One 16-byte load per row and group where the row's
// address allows it, bytes otherwise and at the ragged end.  The rows go R at a time: the R * G loads of a step are issued before
// the first of them is added (the wall: one group, row by row, its 256 threads and resident workgroups cover the latency; a
// thumbnail tile's single wave walks its chunks one after the other and needs the loads in flight itself).
template <int G, int R>
__device__ __forceinline__ void wall_band_sum16(const WallBand &b, uint32_t c0, uint32_t step, cwa_u32x4 (&w0)[G], cwa_u32x4 (&w1)[G]) {
    uint32_t ev[G][4], od[G][4], mine[G];   // ev[g][d]: bytes 0 and 2 of dword d, od[g][d]: bytes 1 and 3; mine: the group's bytes
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint32_t cg = c0 + (uint32_t)g * step;
        mine[g] = cg < b.cb ? (b.cb - cg < 16u ? b.cb - cg : 16u) : 0u;
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) ev[g][d] = od[g][d] = 0u;
    }
    if (mine[0]) {   // (the groups ascend: none behind an empty one)
        for (uint32_t r0 = 0; r0 < b.kh; r0 += R) {
            cwa_u32x4 q[R][G];
#pragma unroll
            for (int j = 0; j < R; j++) {
                const uint8_t *row = b.src + (size_t)(r0 + j) * b.pitch;
                const bool live = R == 1 || r0 + j < b.kh, quads = !((uintptr_t)row & 15u);
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const uint32_t cg = c0 + (uint32_t)g * step;
                    q[j][g] = cwa_u32x4{0u, 0u, 0u, 0u};
                    if (live && mine[g] == 16u && quads) {
                        q[j][g] = *(const cwa_u32x4 *)(row + cg);
                    } else if (live && mine[g]) {
#pragma unroll
                        for (uint32_t i = 0; i < 16u; i++)
                            if (i < mine[g]) q[j][g][i / 4u] |= (uint32_t)row[cg + i] << (8u * (i % 4u));
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < R; j++)
#pragma unroll
                for (int g = 0; g < G; g++)
#pragma unroll
                    for (uint32_t d = 0; d < 4u; d++) {
                        ev[g][d] += q[j][g][d] & 0x00FF00FFu;
                        od[g][d] += (q[j][g][d] >> 8) & 0x00FF00FFu;
                    }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (uint32_t d = 0; d < 2u; d++) {
            w0[g][2u * d] = (ev[g][d] & 0xFFFFu) | (od[g][d] << 16);
            w0[g][2u * d + 1u] = (ev[g][d] >> 16) | (od[g][d] & 0xFFFF0000u);
            w1[g][2u * d] = (ev[g][d + 2u] & 0xFFFFu) | (od[g][d + 2u] << 16);
            w1[g][2u * d + 1u] = (ev[g][d + 2u] >> 16) | (od[g][d + 2u] & 0xFFFF0000u);
        }
}

// Channel c of pixel u of the chunk whose column sums lie in s_sum: the sum of its kw entries at a 3-entry pitch
__device__ __forceinline__ uint32_t wall_box_sum(const uint16_t *s_sum, uint32_t u, uint32_t c, uint32_t k, uint32_t kw) {
    uint32_t sum = 0;
    for (uint32_t i = 0; i < kw; i++) sum += s_sum[3u * (u * k + i) + c];
    return sum;
}

__global__ __launch_bounds__(256) void k_wall_compose(const uint8_t *states, size_t stride, uint32_t width, uint32_t height,
                                                      const uint32_t *mask, uint32_t mask_words, uint8_t *wall, size_t wall_pitch,
                                                      const WallPlaceArgs h) {
    __shared__ cwa_u32x4 s_sum32[kWallBytes / 8];   // 16-bit column sums, eight to a quad
    const uint32_t j = blockIdx.y, tid = threadIdx.x;
    const uint32_t k = (uint32_t)h.k[j];
    if (k == 0) return;
    const uint32_t tw = (width + k - 1u) / k, th = (height + k - 1u) / k;
    const uint32_t cp = wall_chunk_pixels(tw, k), nch = (tw + cp - 1u) / cp;
    if (blockIdx.x >= th * nch) return;
    const uint32_t v = blockIdx.x / nch, u0 = (blockIdx.x % nch) * cp;
    const uint32_t cw = tw - u0 < cp ? tw - u0 : cp;                          // thumbnail pixels of the chunk
    const uint32_t x1 = (u0 + cw) * k < width ? (u0 + cw) * k : width;       // its source columns [u0 * k, x1)
    const uint32_t st = (uint32_t)h.first + j;
    WallBand b;
    b.pitch = 3u * width;
    b.kh = height - v * k < k ? height - v * k : k;
    b.cb = 3u * (x1 - u0 * k);
    const uint32_t off = v * k * b.pitch + 3u * u0 * k;
    b.src = states + (size_t)st * stride + off;
    if (mask && !wall_band_selected(mask + (size_t)st * mask_words, off, b)) return;   // (the same for every thread)

    cwa_u32x4 w0[1], w1[1];
    wall_band_sum16<1, 1>(b, 16u * tid, 0u, w0, w1);
    s_sum32[2u * tid] = w0[0];
    s_sum32[2u * tid + 1u] = w1[0];
    __syncthreads();

    const uint16_t *s_sum = (const uint16_t *)s_sum32;
    uint8_t *out = wall + (size_t)((uint32_t)h.y[j] + v) * wall_pitch + 3u * ((size_t)(uint32_t)h.x[j] + u0);
    for (uint32_t o = tid; o < 3u * cw; o += 256u) {
        const uint32_t u = o / 3u, c = o - 3u * u;
        const uint32_t left = width - (u0 + u) * k, kw = left < k ? left : k;
        const uint32_t a = kw * b.kh;
        const uint32_t sum = wall_box_sum(s_sum, u, c, k, kw);
        out[o] = (uint8_t)(a == 1u ? sum : (sum + a / 2u) / a);
    }
}

__global__ __launch_bounds__(64) void k_cw_touched(const CwaArgs a, int nframes, int accumulate, uint32_t *mask, uint32_t mask_words) {
    const uint32_t lane = threadIdx.x, waves = (a.ntiles + 63u) / 64u;   // workgroup w: stream w / waves, tiles 64 (w % waves) ..
    const uint32_t st = blockIdx.x / waves, wv = blockIdx.x % waves;
    const uint32_t tile = 64u * wv + lane;
    const size_t b0 = (size_t)st * nframes;   // the stream's first batch index
    bool touch = false;
    if (tile < a.ntiles) {
        for (int t = 0; t < nframes; t++) {
            const uint32_t fn = a.ftab[b0 + t].n;
            const uint4 *dir = a.dir + (b0 + t) * a.ntiles + tile;
            const uint32_t k0 = dir[0].x, kend = tile + 1 < a.ntiles ? dir[1].x : fn;
            touch |= k0 < kend && k0 < fn;
        }
    }
    const uint64_t set = __ballot(touch);
    if (lane == 0) {
        uint32_t *row = mask + (size_t)st * mask_words;
        const uint32_t w = 2u * wv;   // (< mask_words: the wave has a tile)
        row[w] = (accumulate ? row[w] : 0u) | (uint32_t)set;
        if (w + 1u < mask_words) row[w + 1u] = (accumulate ? row[w + 1u] : 0u) | (uint32_t)(set >> 32);
    }
}

// ---- mi355_thumb_cwire_batch: records of the thumbnails, from the states as a tick left them (include/mi355diff.h) -------------
// The tile grid runs over the THUMBNAIL (N' = 3 * tw * th bytes, cwa_tiles(N') tiles per stream): what is written -- the record
// and the held thumbnail -- is the thumbnail's, so a tile of it is the unit that owns its held bytes, its fact word and its place
// in the record, exactly as a tile of the state is in the refresh call.
//   k_thumb_facts (grid: thumbnail tiles x streams, one wave) : the tile is a run of (row, byte range) pieces, each cut along
//       the wall's chunks of its row (wall_chunk_pixels: a chunk's band is at most kWallBytes source bytes per row and keeps its
//       row's 16-byte alignment).  A chunk whose band meets no selected tile (wall_band_selected) is skipped before a state byte
//       moves; of a selected one the column sums go to LDS (wall_band_sum16: four 16-byte columns per lane, four rows at a
//       time, sixteen loads in flight) and the chunk's output bytes INSIDE the piece are made as k_wall_compose makes them
//       (wall_box_sum, then the rounding divide by act_div).
//       The held bytes of the tile lie in LDS (cwa_tile_load); where |new - held| > threshold the difference byte goes to the
//       tile of differences and `new` replaces the held byte in LDS, everywhere else the difference is zero.  cwc_tile_facts of
//       that tile; a tile with no selected chunk stores the all-zero fact.
//   k_cwc_scan<true>, k_cwc_place<true>                       : the coalescer's, on cwa_tiles(N') tiles per stream
//   k_thumb_emit  (grid: the same)                            : returns on a zero fact or a record that does not fit; builds the
//       same tile from the same bytes, stores the LDS copy of the held tile where a difference was set (whole dwords inside the
//       tile where the address allows, bytes otherwise) and writes the entries (cwc_emit_tile).  The only pass that writes the
//       held thumbnail and the last that reads it; a workgroup touches no thumbnail byte outside its own tile.
// LDS reads of the horizontal sum are 16-bit at a 3-entry pitch, k entries apart between neighbouring pixels, as in the wall.
__device__ __forceinline__ bool thumb_tile(uint8_t *s, uint8_t *s_held, cwa_u32x4 *s_sum32, const CwaArgs &a, const ThumbArgs &h,
                                           uint32_t st, uint32_t lo, uint32_t len, int lane) {
    const uint32_t k = h.k, rb = h.row.d, hi = lo + len;
    const uint32_t cp = wall_chunk_pixels(h.tw, k);
    const uint8_t *state = a.state + (size_t)st * a.stride;
    const uint32_t *mask = h.mask ? h.mask + (size_t)st * h.mask_words : nullptr;
    const uint16_t *s_sum = (const uint16_t *)s_sum32;
    for (uint32_t i = lane; i < kCwaTile / 16; i += 64) ((cwa_u32x4 *)s)[i] = cwa_u32x4{0u, 0u, 0u, 0u};
    cwa_tile_load(s_held, h.thumbs + (size_t)st * h.thumb_stride + lo, len, lane);
    __syncthreads();
    bool any = false;   // (the same for every lane, as is every branch around a barrier below)
    const uint32_t v1 = act_div(hi - 1u, h.row);
    for (uint32_t v = act_div(lo, h.row); v <= v1; v++) {
        const uint32_t r0 = v * rb;                                                      // the row's first thumbnail byte
        const uint32_t j0 = lo > r0 ? lo : r0, j1 = hi < r0 + rb ? hi : r0 + rb;         // the piece
        WallBand b;
        b.pitch = 3u * h.width;
        b.kh = h.height - v * k < k ? h.height - v * k : k;
        for (uint32_t cu0 = (j0 - r0) / 3u / cp * cp; 3u * cu0 < j1 - r0; cu0 += cp) {   // the row's chunks that the piece meets
            const uint32_t cw = h.tw - cu0 < cp ? h.tw - cu0 : cp;
            const uint32_t x1 = (cu0 + cw) * k < h.width ? (cu0 + cw) * k : h.width;
            b.cb = 3u * (x1 - cu0 * k);
            const uint32_t off = v * k * b.pitch + 3u * cu0 * k;
            b.src = state + off;
            if (mask && !wall_band_selected(mask, off, b)) continue;
            if (any) __syncthreads();   // the sums of the chunk before are read
            any = true;
            constexpr int kGroups = kWallBytes / 1024u;   // a lane's column groups, 1024 bytes apart: a wave's load is one piece
            cwa_u32x4 w0[kGroups], w1[kGroups];
            wall_band_sum16<kGroups, 4>(b, 16u * lane, 1024u, w0, w1);
#pragma unroll
            for (int g = 0; g < kGroups; g++) {
                const uint32_t q = 64u * g + lane;
                if (16u * q >= b.cb) continue;
                s_sum32[2u * q] = w0[g];
                s_sum32[2u * q + 1u] = w1[g];
            }
            __syncthreads();
            const uint32_t c0 = r0 + 3u * cu0, c1 = c0 + 3u * cw;   // the chunk's thumbnail bytes, cut to the piece
            const uint32_t o0 = j0 > c0 ? j0 : c0, o1 = j1 < c1 ? j1 : c1;
            for (uint32_t j = o0 + lane; j < o1; j += 64) {
                const uint32_t col = j - r0, u = col / 3u, c = col - 3u * u;
                const uint32_t left = h.width - u * k, kw = left < k ? left : k;
                const ActDiv area = h.area[(v + 1u == h.th ? 2u : 0u) + (u + 1u == h.tw ? 1u : 0u)];
                const uint32_t nw = act_div(wall_box_sum(s_sum, u - cu0, c, k, kw) + area.d / 2u, area);
                const uint32_t old = s_held[j - lo];
                const uint32_t mag = nw > old ? nw - old : old - nw;
                if (mag > h.threshold) {
                    s[j - lo] = (uint8_t)(nw - old);
                    s_held[j - lo] = (uint8_t)nw;
                }
            }
        }
    }
    __syncthreads();
    return any;
}

__global__ __launch_bounds__(64) void k_thumb_facts(const CwaArgs a, const ThumbArgs h) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16], s_h[kCwaTile / 16], s_sum32[kWallBytes / 8];
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    uint4 f = make_uint4(0u, 0u, 0u, 0u);
    if (thumb_tile((uint8_t *)s_q, (uint8_t *)s_h, s_sum32, a, h, st, lo, len, lane)) f = cwc_tile_facts((const uint8_t *)s_q, lo, lane);
    if (lane == 0) a.chunk[(size_t)st * a.ntiles + tile] = f;
}

__global__ __launch_bounds__(64) void k_thumb_emit(const CwaArgs a, const ThumbArgs h, const CwcOut o) {
    __shared__ cwa_u32x4 s_q[kCwaTile / 16], s_h[kCwaTile / 16], s_sum32[kWallBytes / 8];
    __shared__ uint32_t s_code32[kCwaTile / 4 + 2], s_diff32[kCwaTile / 4 + 2];
    const uint8_t *s = (const uint8_t *)s_q, *s_held = (const uint8_t *)s_h;
    const int lane = threadIdx.x;
    const uint32_t st = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const uint4 fact = a.chunk[(size_t)st * a.ntiles + tile];   // {nonzero bytes, entries before, escapes before, end before}
    if (fact.x == 0) return;   // no selected chunk, or no difference above the threshold
    const uint32_t seg = o.offsets[st], n = o.offsets[st + 1] - seg;
    const uint64_t fp0 = o.frame_pos[st], fp1 = o.frame_pos[st + 1];
    if (fp1 > o.capacity) return;   // the record does not fit: skipped whole, and the stream's held thumbnail stays as it is
    const uint32_t lo = tile * kCwaTile;
    const uint32_t len = a.n - lo < kCwaTile ? a.n - lo : kCwaTile;
    thumb_tile((uint8_t *)s_q, (uint8_t *)s_h, s_sum32, a, h, st, lo, len, lane);
    // the held thumbnail at the emitted bytes: a dword that holds one is stored whole (its other bytes are the held ones, read
    // by this workgroup alone), [0, len) only
    uint8_t *dst = h.thumbs + (size_t)st * h.thumb_stride + lo;
    const uint32_t q = ((uintptr_t)dst & 3u) ? 0u : len / 4u;
    for (uint32_t i = lane; i < q; i += 64)
        if (((const uint32_t *)s)[i]) ((uint32_t *)dst)[i] = ((const uint32_t *)s_held)[i];
    for (uint32_t i = 4u * q + lane; i < len; i += 64)
        if (s[i]) dst[i] = s_held[i];
    cwc_emit_tile<true>(s, (uint8_t *)s_code32, (uint8_t *)s_diff32, fact, o, seg, n, fp0, cwire_record_escapes(fp1 - fp0, n), lo, lane);
}

// ---- mi355_cwire_split_cwire_batch: every record cut into pieces of at most max_bytes bytes (include/mi355diff.h) -----------------
// The chunk table of the directory through its running sums (k_cwa_table, k_cwa_facts, k_cwa_scan 0, k_cwa_escsum, k_cwa_scan 1),
// then, over the blocks of kCwsBlock entries of all records (a block is kCwsBlock / kCwaChunk chunks, so the escape rank and the
// running index at its start are the words of its first chunk):
//   k_cws_table (grid: records)  : blk[b] = {record, block of the record, 0, 0}; the records' first blocks are kernel arguments
//   k_cws_count (grid: blocks)   : walks the block and leaves its pieces and their bytes in blk[b]
//   k_cws_scan  (one workgroup)  : exclusive scan of both in 64 bits -> base[b]; piece_first[r] at a record's first block,
//                                  piece_first[nrecords], piece_pos[0]
//   k_cws_emit  (grid: blocks)   : the same walk; every piece it closes is written, with piece_pos[p + 1], if it fits
// The walk (cws_walk): rounds of 4096 entries, a code dword per thread, the next round's dword loaded before this one is cut.  With r(d) the 255 codes of the block before dword d, a
// piece from dword a to dword q costs 8 + V(q) - V(a) - 4*[code[4a] == 255] + 4*F(a) with V(d) = 8d + 4r(d): the cost needs no
// scan of its own beside the escape rank and the running index of the decode step.  Wave 0 holds the open piece and finds the
// round's cuts one after the other -- the first dword the open piece cannot take, by a ballot over 64 of the round's V in LDS at
// a time -- and lists the pieces it closes; in the emit pass the sixteen waves then copy a listed piece each, whole dwords of the input's code and
// diff sections (the first code byte and the pad bytes of a record's last dword rewritten), the piece's own first escape and the
// input's escape words of its other 255 codes.  A cut needs two dwords before it (eight entries cost at most 56 bytes), so a round
// closes at most 512 pieces and the block's last.  No workgroup waits on another; every loop is bounded by the block's own entries;
// reads stay inside the record (code and diff dwords below pad4(n) / 4, escape words below e); a piece that does not fit is not
// begun.
constexpr int kCwsThreads = 1024, kCwsWaves = kCwsThreads / 64;   // a round: kCwsThreads dwords, one chunk of the table
constexpr int kCwsList = kCwsThreads / 2 + 4;

struct CwsPiece {
    uint32_t d, len, x, rank;       // first dword (of the block), entries, x_a, the input's escape rank of its first inner 255 code
    uint32_t F, bytes, off, idx;    // F(a), size, bytes and pieces of the block before it
};

__device__ __forceinline__ uint32_t cws_block_count(uint32_t n) { return n ? (n + kCwsBlock - 1) / kCwsBlock : 1u; }

__global__ __launch_bounds__(64) void k_cws_table(const CwaArgs a, uint4 *blk, const CwsTableArgs h) {
    const uint32_t rec = (uint32_t)h.first + blockIdx.x;
    const uint32_t nb = cws_block_count(a.ftab[rec].n);
    for (uint32_t j = threadIdx.x; j < nb; j += 64) blk[h.bbase[blockIdx.x] + j] = make_uint4(rec, j, 0u, 0u);
}

// One listed piece, by one wave; p0 / b0: pieces and bytes before the block
__device__ __forceinline__ void cws_write_piece(const CwaArgs &a, const CwaFrame &f, uint32_t d0, const CwsPiece &pc, uint64_t p0,
                                                uint64_t b0, const CwsOut &o, int lane) {
    const uint64_t p = p0 + pc.idx, pos = b0 + pc.off, end = pos + pc.bytes;
    if (lane == 0 && p + 1 <= o.piece_capacity) o.piece_pos[p + 1] = end;
    if (p >= o.piece_capacity || end > o.capacity) return;
    const CwireSections<const uint8_t> sec = cwa_sections(a, f);
    const uint32_t *code = sec.code32() + d0 + pc.d, *dif = sec.diff32() + d0 + pc.d, *esc = sec.esc32();
    const uint32_t ndw = cwire_dwords(pc.len), E = (pc.bytes - 8u - 8u * ndw) / 4u;
    const uint32_t last = (pc.len & 3u) ? 0xFFFFFFFFu >> (32u - 8u * (pc.len & 3u)) : 0xFFFFFFFFu;   // the last dword's entries
    uint32_t *out = (uint32_t *)(o.cwire + pos);
    if (lane == 0) {
        __builtin_nontemporal_store(pc.len, out);
        __builtin_nontemporal_store(E, out + 1);
    }
    uint32_t *oc = out + 2, *oe = oc + ndw, *od = oe + E;
    for (uint32_t i = lane; i < ndw; i += 64) {
        uint32_t w = code[i], v = dif[i];
        if (i == 0) w = (w & ~255u) | (pc.x < 255u ? pc.x : 255u);
        if (i + 1 == ndw) {
            w &= last;
            v &= last;
        }
        __builtin_nontemporal_store(w, oc + i);
        __builtin_nontemporal_store(v, od + i);
    }
    if (pc.F && lane == 0) __builtin_nontemporal_store(pc.x, oe);
    for (uint32_t i = lane; i < E - pc.F; i += 64) {
        const uint32_t r = pc.rank + i;
        __builtin_nontemporal_store(r < f.e ? esc[r] : 0u, oe + pc.F + i);   // (an escape ranked at or past e has no word)
    }
}

template <bool EMIT>
__device__ __forceinline__ void cws_walk(const CwaArgs &a, uint4 *blk, const ulonglong2 *base, uint32_t M, const CwsOut &o) {
    __shared__ uint32_t s_esc[2][kCwsWaves], s_sum[2][kCwsWaves];
    __shared__ uint32_t s_v[kCwsThreads], s_vn[kCwsThreads], s_xa[kCwsThreads], s_fl[kCwsThreads];
    __shared__ CwsPiece s_list[EMIT ? kCwsList : 1];
    __shared__ uint32_t s_nlist;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const uint4 bw = blk[b];
    const CwaFrame f = a.ftab[bw.x];
    const uint32_t k0 = bw.y * kCwsBlock;
    const uint32_t k1 = f.n - k0 < kCwsBlock ? f.n : k0 + kCwsBlock;
    const uint4 ch = a.chunk[f.cbase + bw.y * (kCwsBlock / kCwaChunk)];
    const CwireSections<const uint8_t> sec = cwa_sections(a, f);
    const uint32_t *code = sec.code32(), *esc = sec.esc32();
    const uint32_t d0 = k0 / 4, dend = k0 < k1 ? cwire_dwords(k1 - k0) : 0u;   // the block's dwords: d0 + [0, dend)
    uint64_t p0 = 0, b0 = 0;
    if (EMIT) {
        const ulonglong2 bs = base[b];
        p0 = bs.x;
        b0 = bs.y;
    }
    uint32_t carry_e = ch.y, carry_x = ch.z;   // escape rank and running index before the round
    // the open piece and the block's totals so far (wave 0, the same in every lane)
    uint32_t o_d = 0, o_base = 0, o_x = 0, o_rank = 0, o_F = 0, pieces = 0, bytes = 0;
    int buf = 0;
    uint32_t ahead = tid < dend ? code[d0 + tid] : 0u;   // the next round's code dword: in flight while this round is cut
    for (uint32_t r0 = 0; r0 < dend; r0 += kCwsThreads, buf ^= 1) {
        const uint32_t dl = r0 + tid, d = d0 + dl;
        const bool live = dl < dend;
        const uint32_t word = ahead;
        ahead = dl + kCwsThreads < dend ? code[d + kCwsThreads] : 0u;
        bool in[4], fl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) in[j] = live && 4 * d + j < k1;
        uint32_t wtot;
        const uint32_t before = cwire_escapes_before(word, in, fl, wtot);
        const uint32_t rank = block_waves_before<kCwsWaves>(wtot, 0, s_esc[buf], carry_e) + before;
        uint32_t inc[4], rk[4];
        bool bad[4];
        const uint32_t lsum = cwire_decode4(word, in, fl, rank, f.e, esc, inc, bad, rk);
        const uint32_t x = block_exclusive_scan<kCwsWaves>(lsum, s_sum[buf], carry_x);
        const uint32_t n255 = (uint32_t)fl[0] + fl[1] + fl[2] + fl[3];
        const uint32_t v = 8u * dl + 4u * (rank - ch.y), xa = x + inc[0] - 1u;
        s_v[tid] = v;
        s_vn[tid] = live ? v + 8u + 4u * n255 : v;
        s_xa[tid] = xa;
        s_fl[tid] = (fl[0] ? 1u : 0u) | (xa >= 255u ? 2u : 0u);
        __syncthreads();
        if (wave == 0) {
            const uint32_t nd = dend - r0 < (uint32_t)kCwsThreads ? dend - r0 : (uint32_t)kCwsThreads;
            uint32_t nlist = 0, lo = 0;   // lo: the first dword of the round not yet known to fit the open piece
            bool open = r0 != 0;          // (the block's first piece opens at its first dword)
            for (;;) {
                uint32_t q = open ? nd : 0u;   // the dword of the round the next piece opens at; nd: none
                for (; open && lo < nd; lo += 64) {   // 64 dwords a step: the cost grows with the dword, the first over the limit cuts
                    const uint32_t i = lo + lane;
                    const uint64_t m = __ballot(i < nd && s_vn[i] - o_base > M);
                    if (m) {
                        q = lo + (uint32_t)__ffsll((unsigned long long)m) - 1u;
                        break;
                    }
                }
                const bool fin = q == nd && r0 + nd == dend;   // the block's last piece ends with the block
                if (open && (q < nd || fin)) {                 // the open piece closes: dwords [o_d, r0 + q)
                    const uint32_t size = (q < nd ? s_v[q] : s_vn[nd - 1]) - o_base;
                    if (EMIT && lane == 0 && nlist < (uint32_t)kCwsList)
                        s_list[nlist] = CwsPiece{o_d, (fin ? k1 - k0 : 4u * (r0 + q)) - 4u * o_d, o_x, o_rank, o_F, size, bytes, pieces};
                    nlist++;
                    pieces++;
                    bytes += size;
                }
                if (q == nd) break;
                const uint32_t fw = s_fl[q];
                o_d = r0 + q;
                o_F = fw >> 1;
                o_x = s_xa[q];
                o_base = s_v[q] + 4u * (fw & 1u) - 4u * o_F - 8u;
                o_rank = ch.y + (s_v[q] - 8u * o_d) / 4u + (fw & 1u);
                open = true;
                lo = q + 1u;   // (its first dword always fits)
            }
            if (EMIT && lane == 0) s_nlist = nlist < (uint32_t)kCwsList ? nlist : (uint32_t)kCwsList;
        }
        if (EMIT) {
            __syncthreads();
            const uint32_t nlist = s_nlist;
            for (uint32_t i = wave; i < nlist; i += kCwsWaves) cws_write_piece(a, f, d0, s_list[i], p0, b0, o, lane);
        }
    }
    if (!EMIT && tid == 0) {
        blk[b].z = pieces;
        blk[b].w = bytes;
    }
}

__global__ __launch_bounds__(kCwsThreads) void k_cws_count(const CwaArgs a, uint4 *blk, uint32_t M) {
    cws_walk<false>(a, blk, nullptr, M, CwsOut{});
}

__global__ __launch_bounds__(kCwsThreads) void k_cws_emit(const CwaArgs a, uint4 *blk, const ulonglong2 *base, uint32_t M, const CwsOut o) {
    cws_walk<true>(a, blk, base, M, o);
}

__global__ __launch_bounds__(256) void k_cws_scan(const uint4 *blk, ulonglong2 *base, uint32_t nblocks, int nrecords, const CwsOut o) {
    __shared__ uint64_t s_p[2][4], s_b[2][4];
    uint64_t pieces = 0, bytes = 0;
    int buf = 0;
    for (uint32_t i0 = 0; i0 < nblocks; i0 += 256, buf ^= 1) {
        const uint32_t i = i0 + threadIdx.x;
        const uint4 w = i < nblocks ? blk[i] : make_uint4(0u, 1u, 0u, 0u);
        const uint64_t pb = block_exclusive_scan<4>((uint64_t)w.z, s_p[buf], pieces);
        const uint64_t bb = block_exclusive_scan<4>((uint64_t)w.w, s_b[buf], bytes);
        if (i < nblocks) {
            base[i] = make_ulonglong2(pb, bb);
            if (w.y == 0) o.piece_first[w.x] = (uint32_t)pb;
        }
    }
    if (threadIdx.x == 0) {
        o.piece_first[nrecords] = (uint32_t)pieces;
        o.piece_pos[0] = 0;
    }
}

// ---- mi355_cwire_fec_batch, mi355_cwire_fec_repair_batch: parity over groups of pieces (include/mi355diff.h, "Parity pieces") -----
//   k_fec_first  (one workgroup) : fec_first = the exclusive scan of ceil(pieces / group) per record.
//   k_fec_make   (a grid sized from the device, 256 threads) : the waves stride over items (group, chunk of kFecChunk dwords of its
//       parity block).  An item is wave-uniform: the group's record by binary search in fec_first, the void rule on the members'
//       positions a lane per member, then per dword of the chunk the members from the last slot down, four loads in flight: one
//       XOR into P, xtime and one XOR into Q.  No tables, no LDS, no atomics; the item of chunk 0 writes fec_len.
//   k_fec_repair (a workgroup per job) : the same walk over the survivors, the constant multiplies, the header and tail tests.
constexpr uint32_t kFecChunk = 64;

__global__ __launch_bounds__(256) void k_fec_first(const FecArgs a) {
    __shared__ uint32_t s_w[2][4];
    uint32_t groups = 0;
    int buf = 0;
    for (int r0 = 0; r0 < a.nrecords; r0 += 256, buf ^= 1) {
        const int r = r0 + (int)threadIdx.x;
        uint32_t v = 0;
        if (r < a.nrecords) {
            const uint32_t c = a.piece_first[r + 1] - a.piece_first[r];
            v = c / a.group + (c % a.group ? 1u : 0u);
        }
        const uint32_t before = block_exclusive_scan<4>(v, s_w[buf], groups);
        if (r < a.nrecords) a.fec_first[r] = before;
    }
    if (threadIdx.x == 0) a.fec_first[a.nrecords] = groups;
}

// shift: items of a group, a power of two not below the chunks of a pitch (an item past them has nothing to do)
__global__ __launch_bounds__(256) void k_fec_make(const FecArgs a, uint32_t shift) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t nwaves = (uint64_t)gridDim.x * 4u;
    const uint32_t total = a.fec_first[a.nrecords];
    const uint64_t ngroups = total < a.group_capacity ? total : a.group_capacity;
    const uint32_t cpp = (a.pitch / 4u + kFecChunk - 1u) / kFecChunk;
    const uint64_t nitems = ngroups << shift;
    for (uint64_t item = (uint64_t)blockIdx.x * 4u + wave; item < nitems; item += nwaves) {
        const uint32_t chunk = (uint32_t)item & ((1u << shift) - 1u);
        if (chunk >= cpp) continue;
        const uint32_t g = (uint32_t)(item >> shift);
        const FecGroup fg = fec_group(a.fec_first, a.piece_first, a.nrecords, a.group, g);
        // the void rule, before a piece byte moves: a lane per member
        uint32_t L = 0;
        bool bad = fg.m == 0;
        for (uint32_t i = lane; i < fg.m; i += 64u) {
            const uint32_t len = fec_member_len(a.piece_pos, a.piece_capacity, a.pieces_bytes, a.pitch, fg.p0 + i);
            bad |= len == 0;
            L = len > L ? len : L;
        }
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)L, k, 64);
            L = o > L ? o : L;
        }
        if (__ballot(bad)) L = 0;
        if (chunk == 0 && lane == 0) a.fec_len[g] = L;
        if ((uint64_t)chunk * kFecChunk * 4u >= L) continue;   // (a void group included)
        const uint64_t slot = (uint64_t)g * a.nparity * a.pitch;
        if (slot + (uint64_t)a.nparity * a.pitch > a.capacity) continue;   // no room: skipped whole
        const uint32_t w = chunk * kFecChunk + lane;
        uint32_t P = 0, Q = 0;
        for (uint32_t i = fg.m; i > 0;) {
            const uint32_t nb = i < 4u ? i : 4u;
            uint32_t v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                v[k] = 0;
                if (k < nb) {
                    const uint64_t p = fg.p0 + (i - 1u - k);
                    const uint64_t at = a.piece_pos[p];
                    const uint32_t len = (uint32_t)(a.piece_pos[p + 1] - at);
                    if (4u * w < len) v[k] = a.pieces[at / 4u + w];
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (k < nb) {
                    P ^= v[k];
                    Q = fec_xtime(Q) ^ v[k];
                }
            i -= nb;
        }
        if (4u * w < L) {
            a.out[slot / 4u + w] = P;
            if (a.nparity == 2u) a.out[(slot + a.pitch) / 4u + w] = Q;
        }
    }
}

__global__ __launch_bounds__(256) void k_fec_repair(const uint8_t *rx, const FecRepairArgs h, uint8_t *out, size_t pitch, uint32_t *verdict) {
    const FecRepairJob jb = h.job[blockIdx.x];
    const uint32_t nw = jb.fec_len / 4u;
    // the rebuilt dwords w of the lost slots (d1: the second of two)
    auto word = [&](uint32_t w, uint32_t &d0, uint32_t &d1) {
        uint32_t P = jb.p_off != kFecAbsent ? ((const uint32_t *)(rx + jb.p_off))[w] : 0u;
        uint32_t Q = jb.q_off != kFecAbsent ? ((const uint32_t *)(rx + jb.q_off))[w] : 0u;
        uint32_t qs = 0;
        for (uint32_t i = jb.members; i > 0; i--) {
            const uint64_t off = h.off[jb.slot0 + i - 1u];
            uint32_t v = 0;
            if (off != kFecAbsent && 4u * w < h.len[jb.slot0 + i - 1u]) v = ((const uint32_t *)(rx + off))[w];
            P ^= v;
            qs = fec_xtime(qs) ^ v;
        }
        Q ^= qs;
        d1 = 0;
        if (jb.mode == 1u) d0 = P;
        else if (jb.mode == 2u) d0 = fec_mul(Q, jb.c2);
        else {
            d1 = fec_mul(Q ^ fec_mul(P, jb.c1), jb.c2);
            d0 = P ^ d1;
        }
    };
    uint32_t vd[2] = {0u, 0u};
    if (jb.mode != 0u) {
        const int nblocks = jb.mode == 3u ? 2 : 1;
        uint32_t n[2] = {0u, 0u}, e[2] = {0u, 0u};
        uint64_t tail[2] = {0, 0};
        if (nw >= 2u) {   // every thread makes the headers for itself
            word(0, n[0], n[1]);
            word(1, e[0], e[1]);
            for (int k = 0; k < nblocks; k++) vd[k] = fec_header_verdict(n[k], e[k], jb.fec_len, &tail[k]);
        } else {
            vd[0] = vd[1] = 1u;
            tail[0] = tail[1] = jb.fec_len;
        }
        bool nz[2] = {false, false};
        uint32_t *o0 = (uint32_t *)(out + (size_t)(2u * jb.index) * pitch), *o1 = (uint32_t *)(out + (size_t)(2u * jb.index + 1u) * pitch);
        for (uint32_t w = threadIdx.x; w < nw; w += 256u) {
            uint32_t d[2];
            word(w, d[0], d[1]);
            o0[w] = d[0];
            if (nblocks == 2) o1[w] = d[1];
            for (int k = 0; k < nblocks; k++)   // (headers and tails are whole dwords)
                nz[k] |= 4ull * w >= tail[k] && d[k] != 0u;
        }
        for (int k = 0; k < 2; k++)
            if (__syncthreads_or(nz[k])) vd[k] |= 2u;
        if (nblocks == 1) vd[1] = 0u;
    }
    if (threadIdx.x == 0) {
        verdict[2u * jb.index] = vd[0];
        verdict[2u * jb.index + 1u] = vd[1];
    }
}

// ---- mi355_cwire_runs_encode_batch, mi355_cwire_runs_decode_batch: run-coded records for the link (include/mi355diff.h) -----------
// Encode, over the chunk table of the directory (k_cwa_table; a chunk is kCwaChunk codes of one record, and a multiple of 256
// entries, so every chunk boundary is a cut and a chunk's runs depend on the chunk alone):
//   k_cwr_count (grid: chunks)   : the chunk's run starts (k % 256 == 0 or a non-zero code), four entries per lane from one code
//                                  dword, ballot and popcount -> chunk.x
//   k_cwr_scan  (grid: records)  : exclusive scan over the record's chunks -> chunk.y, the first run rank; r, the size decision
//                                  and the form row
//   k_cwr_place (one workgroup)  : pos = the exclusive scan of the records' link bytes, in 64 bits
//   k_cwr_emit  (grid: chunks)   : the starts' codes and places compacted in LDS by rank, then gap[] and len[] (the distance to the
//                                  next start of the chunk) stored: whole dwords inside the chunk's runs, single bytes at its
//                                  ragged ends, the pads by the record's last chunk; esc and diff copied as dwords, each chunk its
//                                  share.  A record kept compact is copied, dword for dword.
// Decode, over workgroups of kCwrRuns runs (run form) or kCwaChunk entries (compact form, a copy):
//   k_cwr_table (grid: records)  : the host's places and headers -> rtab, frame_pos, workgroup -> record
//   k_cwr_sums  (grid: workgroups): sum of len + 1 over its runs -> chunk.y
//   k_cwr_dscan (grid: records)  : exclusive scan over the record's workgroups -> chunk.y, the entry its first run starts at
//   k_cwr_expand(grid: workgroups): scans its runs, then builds the code bytes of the entries they cover 4096 at a time in LDS --
//                                  zeros, the gaps at the run starts -- and stores them: whole dwords inside, single bytes at
//                                  the ragged ends; everything clamped to n, the record's last workgroup writes the pad.
// No workgroup waits on another and no two write the same byte; dwords that two workgroups share are written as bytes.
// Reads stay inside the spans the headers give, writes inside [pos[b], pos[b + 1]) of a record that fits.
__global__ __launch_bounds__(256) void k_cwr_count(const CwaArgs a) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t c = blockIdx.x;
    const CwaFrame f = a.ftab[a.chunk[c].w];
    const uint32_t k0 = (c - f.cbase) * kCwaChunk;
    const uint32_t k1 = f.n - k0 < kCwaChunk ? f.n : k0 + kCwaChunk;
    const uint32_t *code = cwa_sections(a, f).code32();
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < (int)(kCwaChunk / 1024); i++) {
        const uint32_t d = k0 / 4 + threadIdx.x + 256 * i;
        const uint32_t w = 4 * d < k1 ? code[d] : 0u;
        bool fl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) fl[j] = 4 * d + j < k1 && cwire_run_start(4 * d + j, (w >> (8 * j)) & 255u);
        uint32_t wtot;
        (void)cwire_rank4(fl, wtot);
        cnt += wtot;   // (the wave's, in every lane)
    }
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) a.chunk[c].x = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(256) void k_cwr_scan(const CwaArgs a, int policy, uint32_t *forms) {
    __shared__ uint32_t s_wave[2][4];
    const CwaFrame f = a.ftab[blockIdx.x];
    uint32_t carry = 0;
    int buf = 0;
    for (uint32_t i0 = 0; i0 < f.nc; i0 += 256, buf ^= 1) {
        const uint32_t i = i0 + threadIdx.x;
        uint4 *ch = a.chunk + f.cbase + i;
        const uint32_t before = block_exclusive_scan<4>(i < f.nc ? ch->x : 0u, s_wave[buf], carry);
        if (i < f.nc) ch->y = before;
    }
    if (threadIdx.x == 0) {
        uint32_t *row = forms + 4 * (size_t)blockIdx.x;
        row[0] = policy == 1 || cwire_runs_smaller(f.n, carry) ? 1u : 0u;
        row[1] = f.n;
        row[2] = f.e;
        row[3] = carry;
    }
}

__global__ __launch_bounds__(256) void k_cwr_place(const uint32_t *forms, int nrecords, uint64_t *pos) {
    __shared__ uint64_t s_wave[2][4];
    uint64_t carry = 0;
    int buf = 0;
    for (int b0 = 0; b0 < nrecords; b0 += 256, buf ^= 1) {
        const int b = b0 + (int)threadIdx.x;
        const uint32_t *row = forms + 4 * (size_t)b;
        const uint64_t bytes = b < nrecords ? cwire_link_bytes(row[0], row[1], row[2], row[3]) : 0;
        const uint64_t before = block_exclusive_scan<4>(bytes, s_wave[buf], carry);
        if (b < nrecords) pos[b] = before;
    }
    if (threadIdx.x == 0) pos[nrecords] = carry;
}

// dwords [lo, hi) of src to dst, by the workgroup's 256 threads
__device__ __forceinline__ void cwr_copy(const uint32_t *src, uint32_t *dst, uint32_t lo, uint32_t hi) {
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) __builtin_nontemporal_store(src[i], dst + i);
}
// ... of a diff section of n bytes: the pad bytes of its last dword leave as zeros
__device__ __forceinline__ void cwr_copy_diff(const uint32_t *src, uint32_t *dst, uint32_t lo, uint32_t hi, uint32_t n) {
    const uint32_t last = (n & 3u) ? 0xFFFFFFFFu >> (32u - 8u * (n & 3u)) : 0xFFFFFFFFu;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) __builtin_nontemporal_store(i + 1 == cwire_dwords(n) ? src[i] & last : src[i], dst + i);
}

// Bytes [lo, hi) of the byte array at dst (4-aligned) from the LDS bytes src[i - base], base a multiple of 4 relative to dst and
// base <= lo: the dwords that lie inside [lo, hi) whole, the bytes of the others one by one.  Dwords [q0, q1) are looked at.
__device__ __forceinline__ void cwr_store_bytes(uint8_t *dst, const uint8_t *src, uint64_t base, uint64_t lo, uint64_t hi, uint64_t q0, uint64_t q1) {
    for (uint64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        const uint64_t g = 4 * q;
        if (g >= lo && g + 4 <= hi) {
            __builtin_nontemporal_store(*(const uint32_t *)(src + (g - base)), (uint32_t *)(dst + g));
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (g + j >= lo && g + j < hi) dst[g + j] = src[g + j - base];
        }
    }
}

__global__ __launch_bounds__(256) void k_cwr_emit(const CwaArgs a, const CwrOut o) {
    __shared__ uint32_t s_wave[2][4];
    __shared__ uint16_t s_at[kCwaChunk + 4];
    __shared__ __attribute__((aligned(4))) uint8_t s_gap[kCwaChunk + 4], s_len[kCwaChunk + 4];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const uint4 ch = a.chunk[c];
    const uint32_t b = ch.w;
    const CwaFrame f = a.ftab[b];
    const uint32_t j = c - f.cbase;
    const uint32_t form = o.forms[4 * (size_t)b], r = o.forms[4 * (size_t)b + 3];
    const uint64_t pos = o.pos[b];
    if (o.pos[b + 1] > o.capacity) return;   // a record that does not fit is skipped whole
    const CwireSections<const uint8_t> sec = cwa_sections(a, f);
    const uint32_t k0 = j * kCwaChunk;
    const uint32_t k1 = f.n - k0 < kCwaChunk ? f.n : k0 + kCwaChunk;
    const uint32_t d0 = k0 / 4, nd = k0 < k1 ? cwire_dwords(k1 - k0) : 0u;   // the chunk's code and diff dwords: d0 + [0, nd)
    uint32_t e0, e1;
    cwire_share(f.e, j, f.nc, e0, e1);
    uint32_t *out = (uint32_t *)(o.out + pos);
    if (j == 0 && tid == 0) {
        __builtin_nontemporal_store(f.n, out);
        __builtin_nontemporal_store(f.e, out + 1);
        if (form) __builtin_nontemporal_store(r, out + 2);
    }
    if (!form) {   // the compact record, dword for dword
        const CwireSections<uint8_t> dst(o.out, pos, f.n, f.e);
        cwr_copy(sec.code32(), dst.code32(), d0, d0 + nd);
        cwr_copy(sec.esc32(), dst.esc32(), e0, e1);
        cwr_copy(sec.diff32(), dst.diff32(), d0, d0 + nd);
        return;
    }
    uint8_t *og = o.out + pos + 12, *ol = og + cwire_pad4(r);
    uint32_t *oe = (uint32_t *)(ol + cwire_pad4(r)), *od = oe + f.e;
    cwr_copy(sec.esc32(), oe, e0, e1);
    cwr_copy_diff(sec.diff32(), od, d0, d0 + nd, f.n);
    // Runs [lo, hi) of the record are the chunk's.  Its starts by rank: where (s_at) and their codes (s_gap); the LDS bytes of run
    // lo + i lie at sh + i, 4-aligned with gap[] and len[] of the record.
    const uint64_t lo = ch.y < r ? ch.y : r, base = lo & ~3ull;
    const uint32_t sh = (uint32_t)(lo - base);
    const uint32_t *code = sec.code32();
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < (int)(kCwaChunk / 1024); i++) {
        const uint32_t dl = tid + 256 * i;
        const uint32_t w = dl < nd ? code[d0 + dl] : 0u;
        bool fl[4];
#pragma unroll
        for (int q = 0; q < 4; q++) fl[q] = k0 + 4 * dl + q < k1 && cwire_run_start(4 * dl + q, (w >> (8 * q)) & 255u);
        uint32_t wtot;
        const uint32_t before = cwire_rank4(fl, wtot);
        uint32_t rank = block_waves_before<4>(wtot, 0, s_wave[i & 1], carry) + before;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (fl[q]) {
                s_at[rank] = (uint16_t)(4 * dl + q);   // (rank < kCwaChunk: a start per entry at the most)
                s_gap[sh + rank] = (uint8_t)(w >> (8 * q));
                rank++;
            }
    }
    const uint32_t x = carry < ch.x ? carry : ch.x;   // (they differ only when the input changed between the launches)
    if (tid == 0) s_at[carry] = (uint16_t)(k1 - k0);
    __syncthreads();
    for (uint32_t i = tid; i < x; i += 256) s_len[sh + i] = (uint8_t)(s_at[i + 1] - s_at[i] - 1u);
    __syncthreads();
    const uint64_t hi = r - lo < x ? r : lo + x;
    cwr_store_bytes(og, s_gap, base, lo, hi, base / 4, (hi + 3) / 4);
    cwr_store_bytes(ol, s_len, base, lo, hi, base / 4, (hi + 3) / 4);
    if (j + 1 == f.nc && tid == 0)
        for (uint64_t k = r; k < cwire_pad4(r); k++) og[k] = ol[k] = 0;
}

__global__ __launch_bounds__(256) void k_cwr_table(const CwrDecode d, const CwrTableArgs h) {
    const CwrRecord rec = h.rec[blockIdx.x];
    const uint32_t b = (uint32_t)h.first + blockIdx.x;
    if (threadIdx.x == 0) {
        d.rtab[b] = rec;
        d.frame_pos[b] = rec.out_pos;
        if (h.last && blockIdx.x + 1 == gridDim.x) d.frame_pos[b + 1] = h.total;
    }
    for (uint32_t j = threadIdx.x; j < rec.nc; j += 256) d.chunk[rec.cbase + j] = make_uint2(b, 0u);
}

// the sections of a record in the run form on the link
struct CwrSections {
    const uint8_t *gap, *len;
    const uint32_t *esc, *diff;
    __device__ CwrSections(const uint8_t *in, const CwrRecord &rec)
        : gap(in + rec.in_pos + 12), len(gap + cwire_pad4(rec.r)), esc((const uint32_t *)(len + cwire_pad4(rec.r))), diff(esc + rec.e) {}
};

__global__ __launch_bounds__(256) void k_cwr_sums(const CwrDecode d) {
    __shared__ uint32_t s_sum[4];
    const uint32_t c = blockIdx.x;
    const CwrRecord rec = d.rtab[d.chunk[c].x];
    if (!rec.form) return;
    const uint32_t q = (c - rec.cbase) * (kCwrRuns / 4) + threadIdx.x;   // the thread's dword of len[]: runs 4q .. 4q + 3
    uint32_t sum = 0;
    if (4 * (uint64_t)q < rec.r) {
        const uint32_t w = ((const uint32_t *)CwrSections(d.in, rec).len)[q];
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * (uint64_t)q + j < rec.r) sum += ((w >> (8 * j)) & 255u) + 1u;
    }
    sum = cwa_wave_sum(sum);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) d.chunk[c].y = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

__global__ __launch_bounds__(256) void k_cwr_dscan(const CwrDecode d) {
    __shared__ uint32_t s_wave[2][4];
    const CwrRecord rec = d.rtab[blockIdx.x];
    if (!rec.form) return;
    uint32_t carry = 0;
    int buf = 0;
    for (uint32_t i0 = 0; i0 < rec.nc; i0 += 256, buf ^= 1) {
        const uint32_t i = i0 + threadIdx.x;
        uint2 *ch = d.chunk + rec.cbase + i;
        const uint32_t before = block_exclusive_scan<4>(i < rec.nc ? ch->y : 0u, s_wave[buf], carry);
        if (i < rec.nc) ch->y = before;
    }
}

__global__ __launch_bounds__(256) void k_cwr_expand(const CwrDecode d) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_tile[kCwaChunk / 4];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const uint2 ch = d.chunk[c];
    const CwrRecord rec = d.rtab[ch.x];
    const uint32_t j = c - rec.cbase, n = rec.n;
    if (rec.out_pos + cwire_record_bytes(n, rec.e) > d.capacity) return;   // a record that does not fit is skipped whole
    const CwireSections<uint8_t> dst(d.out, rec.out_pos, n, rec.e);
    if (j == 0 && tid == 0) {
        uint32_t *head = (uint32_t *)(d.out + rec.out_pos);
        __builtin_nontemporal_store(n, head);
        __builtin_nontemporal_store(rec.e, head + 1);
    }
    uint32_t lo, hi;
    if (!rec.form) {   // the compact record, dword for dword
        const CwireSections<const uint8_t> src(d.in, rec.in_pos, n, rec.e);
        cwire_share(cwire_dwords(n), j, rec.nc, lo, hi);
        cwr_copy(src.code32(), dst.code32(), lo, hi);
        cwr_copy(src.diff32(), dst.diff32(), lo, hi);
        cwire_share(rec.e, j, rec.nc, lo, hi);
        cwr_copy(src.esc32(), dst.esc32(), lo, hi);
        return;
    }
    const CwrSections src(d.in, rec);
    cwire_share(cwire_dwords(n), j, rec.nc, lo, hi);
    cwr_copy_diff(src.diff, dst.diff32(), lo, hi, n);
    cwire_share(rec.e, j, rec.nc, lo, hi);
    cwr_copy(src.esc, dst.esc32(), lo, hi);
    // the thread's four runs: their gaps and the entries they start at
    const uint32_t q = j * (kCwrRuns / 4) + tid;
    uint32_t gw = 0, at[5];
    bool live[4] = {false, false, false, false};
    at[0] = 0;
    if (4 * (uint64_t)q < rec.r) {
        gw = ((const uint32_t *)src.gap)[q];
        const uint32_t lw = ((const uint32_t *)src.len)[q];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            live[i] = 4 * (uint64_t)q + i < rec.r;
            at[i + 1] = at[i] + (live[i] ? ((lw >> (8 * i)) & 255u) + 1u : 0u);
        }
    } else {
        at[1] = at[2] = at[3] = at[4] = 0;
    }
    uint32_t carry = 0;
    const uint32_t first = ch.y + block_exclusive_scan<4>(at[4], s_wave, carry);
    // The entries [E0, E1) are the workgroup's, clamped to n; the record's last workgroup goes on to pad4(n).  (Lengths that sum
    // past n, or past 2^32, only shorten or empty what is written.)
    const uint64_t E0 = ch.y < n ? ch.y : n, sumto = (uint64_t)ch.y + carry;
    const uint64_t E1 = j + 1 == rec.nc ? cwire_pad4(n) : (sumto < n ? sumto : n);
    for (uint64_t tile = E0 & ~3ull; tile < E1; tile += kCwaChunk) {
        __syncthreads();   // (the round before has stored its tile)
#pragma unroll
        for (int i = 0; i < (int)(kCwaChunk / 1024); i++) s_tile[tid + 256 * i] = 0u;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t x = (uint64_t)first + at[i];
            if (live[i] && x >= tile && x - tile < kCwaChunk && x >= E0 && x < n) ((uint8_t *)s_tile)[x - tile] = (uint8_t)(gw >> (8 * i));
        }
        __syncthreads();
        const uint64_t end = E1 - tile < kCwaChunk ? E1 : tile + kCwaChunk;
        cwr_store_bytes(dst.code, (const uint8_t *)s_tile, tile, E0 > tile ? E0 : tile, end, tile / 4, (end + 3) / 4);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
uint32_t cwa_chunks(uint32_t n) { return n ? (n + kCwaChunk - 1) / kCwaChunk : 1u; }
uint32_t cwa_tiles(uint32_t nbytes) { return (nbytes + kCwaTile - 1) / kCwaTile; }
uint32_t cwa_mask_words(uint32_t nbytes) { return (cwa_tiles(nbytes) + 31u) / 32u; }
uint32_t dsp_words(uint32_t nbytes) { return (nbytes / 3u + 31u) / 32u; }

// the n >= 1 records to the core's table (k_cwa_table, kCwaTableFrames per launch) -> their chunks (>= n: a record of no entries
// has one empty chunk)
static uint32_t launch_cwa_table(const CwaArgs &a, const CwaFrame *records, int n, hipStream_t s) {
    CwaTableArgs h{};
    for (int i0 = 0; i0 < n; i0 += kCwaTableFrames) {
        const int nf = n - i0 < kCwaTableFrames ? n - i0 : kCwaTableFrames;
        h.first = i0;
        for (int i = 0; i < nf; i++) h.frame[i] = records[i0 + i];
        hipLaunchKernelGGL(k_cwa_table, dim3(nf), dim3(256), 0, s, a, h);
    }
    return records[n - 1].cbase + records[n - 1].nc;
}

// mi355_cwire_check_batch: the chunk table and its first two passes are the directory's
hipError_t launch_cwire_check(const CwaArgs &a, const CwaFrame *records, int nrecords, uint32_t *verdicts, hipStream_t s) {
    if (nrecords <= 0) return hipSuccess;
    const uint32_t nchunks = launch_cwa_table(a, records, nrecords, s);
    hipLaunchKernelGGL(k_cwa_facts, dim3(nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cwa_scan, dim3(nrecords), dim3(256), 0, s, a, 0);
    hipLaunchKernelGGL(k_cwk_escsum, dim3(nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cwk_finish, dim3(nrecords), dim3(256), 0, s, a, verdicts);
    return hipGetLastError();
}

uint32_t cws_blocks(uint32_t n) { return n ? (n + kCwsBlock - 1) / kCwsBlock : 1u; }

// mi355_cwire_split_cwire_batch: the chunk table through its running sums, then the block table, count, scan and emit
hipError_t launch_cwire_split(const CwaArgs &a, const CwaFrame *records, int nrecords, uint32_t max_bytes, uint4 *blk, ulonglong2 *base,
                              const CwsOut &o, hipStream_t s) {
    if (nrecords <= 0) return hipSuccess;
    const uint32_t nchunks = launch_cwa_table(a, records, nrecords, s);
    hipLaunchKernelGGL(k_cwa_facts, dim3(nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cwa_scan, dim3(nrecords), dim3(256), 0, s, a, 0);
    hipLaunchKernelGGL(k_cwa_escsum, dim3(nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cwa_scan, dim3(nrecords), dim3(256), 0, s, a, 1);
    CwsTableArgs h{};
    uint32_t nblocks = 0;
    for (int i0 = 0; i0 < nrecords; i0 += kCwsTableRecords) {
        const int nr = nrecords - i0 < kCwsTableRecords ? nrecords - i0 : kCwsTableRecords;
        h.first = i0;
        for (int i = 0; i < nr; i++) {
            h.bbase[i] = nblocks;
            nblocks += cws_blocks(records[i0 + i].n);
        }
        hipLaunchKernelGGL(k_cws_table, dim3(nr), dim3(64), 0, s, a, blk, h);
    }
    hipLaunchKernelGGL(k_cws_count, dim3(nblocks), dim3(kCwsThreads), 0, s, a, blk, max_bytes);
    hipLaunchKernelGGL(k_cws_scan, dim3(1), dim3(256), 0, s, blk, base, nblocks, nrecords, o);
    hipLaunchKernelGGL(k_cws_emit, dim3(nblocks), dim3(kCwsThreads), 0, s, a, blk, base, max_bytes, o);
    return hipGetLastError();
}

// mi355_cwire_runs_encode_batch: the chunk table, then count, scan, place and emit
hipError_t launch_cwire_runs_encode(const CwaArgs &a, const CwaFrame *records, int nrecords, int policy, const CwrOut &o, hipStream_t s) {
    if (nrecords <= 0) return hipSuccess;
    const uint32_t nchunks = launch_cwa_table(a, records, nrecords, s);
    // (a workgroup per record, any count up to max_batch in one grid; the table's 128 headers a launch are crossed by the 130-record
    // call of tests/test_cwire_runs_gpu.py)
    const dim3 per_record((uint32_t)nrecords);
    hipLaunchKernelGGL(k_cwr_count, dim3(nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cwr_scan, per_record, dim3(256), 0, s, a, policy, o.forms);
    hipLaunchKernelGGL(k_cwr_place, dim3(1), dim3(256), 0, s, (const uint32_t *)o.forms, nrecords, o.pos);
    hipLaunchKernelGGL(k_cwr_emit, dim3(nchunks), dim3(256), 0, s, a, o);
    return hipGetLastError();
}

uint32_t cwr_chunks(uint32_t form, uint32_t n, uint32_t r) {
    if (!form) return cwa_chunks(n);
    return r ? (r + kCwrRuns - 1) / kCwrRuns : 1u;
}
uint32_t cwr_chunks_max(uint32_t nbytes) { return nbytes ? (nbytes + kCwrRuns - 1) / kCwrRuns : 1u; }

// mi355_cwire_runs_decode_batch: the record table, then sums, scan and expand
hipError_t launch_cwire_runs_decode(const CwrDecode &d, const CwrRecord *records, int nrecords, uint64_t total, hipStream_t s) {
    if (nrecords <= 0) return hipSuccess;
    CwrTableArgs h{};
    h.total = total;
    for (int i0 = 0; i0 < nrecords; i0 += kCwrTableRecords) {
        const int nr = nrecords - i0 < kCwrTableRecords ? nrecords - i0 : kCwrTableRecords;
        h.first = i0;
        h.last = i0 + nr == nrecords;
        for (int i = 0; i < nr; i++) h.rec[i] = records[i0 + i];
        hipLaunchKernelGGL(k_cwr_table, dim3(nr), dim3(256), 0, s, d, h);
    }
    const uint32_t nchunks = records[nrecords - 1].cbase + records[nrecords - 1].nc;
    hipLaunchKernelGGL(k_cwr_sums, dim3(nchunks), dim3(256), 0, s, d);
    const dim3 per_record((uint32_t)nrecords);   // (as in the encoder; the table's 64 records a launch are crossed by the same test)
    hipLaunchKernelGGL(k_cwr_dscan, per_record, dim3(256), 0, s, d);
    hipLaunchKernelGGL(k_cwr_expand, dim3(nchunks), dim3(256), 0, s, d);
    return hipGetLastError();
}

// mi355_cwire_fec_batch: the group scan, then the parity grid.  The host knows neither pieces nor groups: the grid comes from
// the device's size and strides over what the scan found.
hipError_t launch_cwire_fec(const FecArgs &a, uint32_t workgroups, hipStream_t s) {
    if (a.nrecords <= 0) return hipSuccess;
    const uint32_t cpp = (a.pitch / 4u + kFecChunk - 1u) / kFecChunk;
    uint32_t shift = 0;
    while ((1u << shift) < cpp) shift++;
    hipLaunchKernelGGL(k_fec_first, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_fec_make, dim3(workgroups), dim3(256), 0, s, a, shift);
    return hipGetLastError();
}

hipError_t launch_cwire_fec_repair(const uint8_t *rx, const FecRepairArgs &h, int njobs, uint8_t *out, size_t pitch, uint32_t *verdict,
                                   hipStream_t s) {
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fec_repair, dim3((uint32_t)njobs), dim3(256), 0, s, rx, h, out, pitch, verdict);
    return hipGetLastError();
}

// the directory of nframes >= 1 records (k_cwa_table .. k_cwa_dir)
static void launch_cwa_directory(const CwaArgs &a, const CwaFrame *frames, int nframes, hipStream_t s) {
    const uint32_t nchunks = launch_cwa_table(a, frames, nframes, s);
    hipLaunchKernelGGL(k_cwa_facts, dim3(nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cwa_scan, dim3(nframes), dim3(256), 0, s, a, 0);
    hipLaunchKernelGGL(k_cwa_escsum, dim3(nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cwa_scan, dim3(nframes), dim3(256), 0, s, a, 1);
    hipLaunchKernelGGL(k_cwa_dir, dim3(nchunks), dim3(256), 0, s, a);
}

hipError_t launch_cwire_apply(const CwaArgs &a, const CwaFrame *frames, int nframes, hipStream_t s) {
    if (nframes <= 0 || a.ntiles == 0) return hipSuccess;
    launch_cwa_directory(a, frames, nframes, s);
    hipLaunchKernelGGL(k_cwa_apply, dim3(a.ntiles), dim3(64), 0, s, a, nframes);
    return hipGetLastError();
}

hipError_t launch_cwire_apply_multi(const CwaArgs &a, const CwaFrame *records, int nstreams, hipStream_t s) {
    if (nstreams <= 0 || a.ntiles == 0) return hipSuccess;
    launch_cwa_directory(a, records, nstreams, s);
    hipLaunchKernelGGL(k_cwa_apply_multi, dim3(a.ntiles * (uint32_t)nstreams), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_cwire_apply_multi_stream(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, size_t out_stride,
                                           hipStream_t s) {
    if (nstreams <= 0 || nframes <= 0 || a.ntiles == 0) return hipSuccess;
    launch_cwa_directory(a, records, nstreams * nframes, s);
    hipLaunchKernelGGL(k_cwa_apply_multi_stream, dim3(a.ntiles * (uint32_t)nstreams), dim3(64), 0, s, a, nframes, out_stride);
    return hipGetLastError();
}

// The tail of every call that writes one segment / record per stream, once the facts of its tiles are made: the coalescer's scan
// over the facts of `a`, the places of the nsegments segments, then the call's own emit kernel, which emit(form) launches; form is
// std::integral_constant<bool, CWIRE>, the one place where the runtime cwire becomes the kernels' template argument.
template <class Emit>
static void launch_cwc_tail(const CwaArgs &a, const CwcOut &o, int nsegments, bool cwire, hipStream_t s, Emit emit) {
    const auto tail = [&](auto form) {
        hipLaunchKernelGGL(k_cwc_scan<decltype(form)::value>, dim3(nsegments), dim3(256), 0, s, a, o);
        hipLaunchKernelGGL(k_cwc_place<decltype(form)::value>, dim3(1), dim3(kCwcPlaceThreads), 0, s, o, nsegments);
        emit(form);
    };
    if (cwire) tail(std::true_type{});
    else tail(std::false_type{});
}

hipError_t launch_cwire_coalesce(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, const CwcOut &o, bool cwire,
                                 hipStream_t s) {
    if (nstreams <= 0 || nframes <= 0) return hipSuccess;
    const dim3 tiles(a.ntiles * (uint32_t)nstreams);
    if (a.ntiles) {
        launch_cwa_directory(a, records, nstreams * nframes, s);
        hipLaunchKernelGGL(k_cwc_sum, tiles, dim3(64), 0, s, a, nframes);
    }
    launch_cwc_tail(a, o, nstreams, cwire, s, [&](auto form) {
        if (a.ntiles) hipLaunchKernelGGL(k_cwc_emit<decltype(form)::value>, tiles, dim3(64), 0, s, a, o, nframes);
    });
    return hipGetLastError();
}

hipError_t launch_cwire_budget(const CwaArgs &a, const CwaFrame *records, int nstreams, const uint32_t *budget, uint32_t thr0,
                               uint32_t *hist, uint32_t *thresholds, const CwcOut &o, hipStream_t s) {
    if (nstreams <= 0) return hipSuccess;
    CwbInitArgs h{};
    h.thr0 = thr0;
    for (int s0 = 0; s0 < nstreams; s0 += kCwbInitStreams) {
        h.first = s0;
        const int ns = nstreams - s0 < kCwbInitStreams ? nstreams - s0 : kCwbInitStreams;
        for (int j = 0; j < ns; j++) h.budget[j] = budget[s0 + j];
        hipLaunchKernelGGL(k_cwb_init, dim3(ns), dim3(256), 0, s, hist, h);
    }
    const dim3 tiles(a.ntiles * (uint32_t)nstreams);
    if (a.ntiles) {
        launch_cwa_directory(a, records, nstreams, s);
        hipLaunchKernelGGL(k_cwb_hist, tiles, dim3(64), 0, s, a, hist);
    }
    hipLaunchKernelGGL(k_cwb_thr, dim3(nstreams), dim3(256), 0, s, hist, thr0, thresholds);
    if (a.ntiles) hipLaunchKernelGGL(k_cwb_facts, tiles, dim3(64), 0, s, a, (const uint32_t *)hist, thr0);
    launch_cwc_tail(a, o, nstreams, true, s, [&](auto) {
        if (a.ntiles) hipLaunchKernelGGL(k_cwb_emit, tiles, dim3(64), 0, s, a, o, (const uint32_t *)hist, thr0);
    });
    return hipGetLastError();
}

hipError_t launch_cwire_despeckle(const CwaArgs &a, const CwaFrame *records, int nstreams, const uint32_t *need, uint32_t width,
                                  uint32_t *words, uint32_t *changed, uint32_t *keep, uint32_t *dropped, const CwcOut &o,
                                  hipStream_t s) {
    if (nstreams <= 0) return hipSuccess;
    const uint32_t nwords = dsp_words(a.n);
    const uint32_t blocks = nwords / 4096u + 1u < 64u ? nwords / 4096u + 1u : 64u;   // 16 words or more a thread
    DspInitArgs h{};
    bool filter = false;
    for (int s0 = 0; s0 < nstreams; s0 += kDspInitStreams) {
        h.first = s0;
        const int part = nstreams - s0 < kDspInitStreams ? nstreams - s0 : kDspInitStreams;
        for (int j = 0; j < part; j++) {
            h.need[j] = need[s0 + j];
            filter = filter || need[s0 + j] != 0u;
        }
        hipLaunchKernelGGL(k_dsp_init, dim3(part, blocks), dim3(256), 0, s, words, dropped, changed, nwords, h);
    }
    const dim3 per_tile(a.ntiles * (uint32_t)nstreams), per_word((nwords + 255u) / 256u, (uint32_t)nstreams);
    if (a.ntiles) {
        launch_cwa_directory(a, records, nstreams, s);
        if (filter) {
            hipLaunchKernelGGL(k_dsp_mark, per_tile, dim3(64), 0, s, a, (const uint32_t *)words, changed, nwords);
            hipLaunchKernelGGL(k_dsp_keep, per_word, dim3(256), 0, s, (const uint32_t *)words,
                               (const uint32_t *)changed, keep, nwords, act_divisor(width));
        }
        hipLaunchKernelGGL(k_dsp_facts, per_tile, dim3(64), 0, s, a, (const uint32_t *)words, (const uint32_t *)keep, nwords, dropped);
    }
    launch_cwc_tail(a, o, nstreams, true, s, [&](auto) {
        if (a.ntiles) hipLaunchKernelGGL(k_dsp_emit, per_tile, dim3(64), 0, s, a, o, (const uint32_t *)words, (const uint32_t *)keep, nwords);
    });
    return hipGetLastError();
}

hipError_t launch_cwire_crop(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, const int32_t *rects, uint32_t width,
                             bool keep_index, uint32_t *words, const CwcOut &o, bool cwire, hipStream_t s) {
    if (nstreams <= 0 || nframes <= 0) return hipSuccess;
    const ActDiv row = act_divisor(a.ntiles ? 3u * width : 1u);
    if (a.ntiles) {
        launch_cwa_directory(a, records, nstreams * nframes, s);
        CropArgs h{};
        h.row_bytes = 3u * width;
        h.keep_index = keep_index ? 1 : 0;
        for (int s0 = 0; s0 < nstreams; s0 += kCropStreams) {
            h.first = s0;
            const int ns = nstreams - s0 < kCropStreams ? nstreams - s0 : kCropStreams;
            for (int j = 0; j < ns; j++)
                for (int k = 0; k < 4; k++) h.rect[j][k] = rects[4 * (size_t)(s0 + j) + k];
            hipLaunchKernelGGL(k_crop_facts, dim3(a.ntiles * (uint32_t)ns), dim3(64), 0, s, a, nframes, words, h, row);
        }
    }
    const dim3 tiles(a.ntiles * (uint32_t)nstreams);
    launch_cwc_tail(a, o, nstreams, cwire, s, [&](auto form) {
        if (a.ntiles) hipLaunchKernelGGL(k_crop_emit<decltype(form)::value>, tiles, dim3(64), 0, s, a, o, nframes, (const uint32_t *)words, row);
    });
    return hipGetLastError();
}

hipError_t launch_cwire_mosaic(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, const int32_t *place, uint32_t width,
                               uint32_t canvas_w, uint32_t canvas_bytes, uint32_t *words, const CwcOut &o, bool cwire, hipStream_t s) {
    if (nstreams <= 0 || nframes <= 0) return hipSuccess;
    const ActDiv rs = act_divisor(3u * width), rc = act_divisor(3u * canvas_w);
    const int ns = a.ntiles ? nstreams : 0;   // (frames of no bytes: nothing lands anywhere)
    if (ns) {
        launch_cwa_directory(a, records, nstreams * nframes, s);
        MosaicArgs h{};
        for (int s0 = 0; s0 < nstreams; s0 += kMosaicStreams) {
            h.first = s0;
            h.count = nstreams - s0 < kMosaicStreams ? nstreams - s0 : kMosaicStreams;
            for (int j = 0; j < h.count; j++)
                for (int k = 0; k < 6; k++) h.place[j][k] = place[6 * (size_t)(s0 + j) + k];
            hipLaunchKernelGGL(k_mosaic_table, dim3(1), dim3(kMosaicStreams), 0, s, words, h);
        }
    }
    CwaArgs ac = a;   // the coalescer's scan sees ONE stream of the canvas' tiles
    ac.n = canvas_bytes;
    ac.ntiles = cwa_tiles(canvas_bytes);
    const dim3 canvas_tiles(ac.ntiles);   // (the canvas' size alone: no count of frames, streams or records sizes this grid)
    hipLaunchKernelGGL(k_mosaic_facts, canvas_tiles, dim3(64), 0, s, a, ns, nframes, (const uint32_t *)words, rs, rc, canvas_bytes);
    launch_cwc_tail(ac, o, 1, cwire, s, [&](auto form) {   // (the facts and the emit see the streams' a)
        hipLaunchKernelGGL(k_mosaic_emit<decltype(form)::value>, canvas_tiles, dim3(64), 0, s, a, o, ns, nframes, (const uint32_t *)words, rs, rc,
                           canvas_bytes);
    });
    return hipGetLastError();
}

hipError_t launch_state_digest(const uint8_t *states, size_t stride, uint32_t n, int nstreams, uint32_t *digests, hipStream_t s) {
    const uint32_t ntiles = cwa_tiles(n);
    if (nstreams <= 0 || ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_state_digest, dim3(ntiles * (uint32_t)nstreams), dim3(64), 0, s, states, stride, n, ntiles, digests);
    return hipGetLastError();
}

hipError_t launch_refresh(const CwaArgs &a, int nstreams, const uint32_t *peer, uint32_t *mask, const CwcOut &o, hipStream_t s) {
    if (nstreams <= 0) return hipSuccess;
    const uint32_t mask_words = cwa_mask_words(a.n);
    const dim3 tiles(a.ntiles * (uint32_t)nstreams);
    if (a.ntiles) {
        const hipError_t e = hipMemsetAsync(mask, 0, (size_t)nstreams * mask_words * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rf_facts, tiles, dim3(64), 0, s, a, peer, mask, mask_words);
    }
    launch_cwc_tail(a, o, nstreams, true, s, [&](auto) {
        if (a.ntiles) hipLaunchKernelGGL(k_rf_emit, tiles, dim3(64), 0, s, a, o);
    });
    return hipGetLastError();
}

hipError_t launch_state_clear_tiles(uint8_t *states, size_t stride, uint32_t n, int nstreams, const uint32_t *mask, hipStream_t s) {
    const uint32_t ntiles = cwa_tiles(n);
    if (nstreams <= 0 || ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_state_clear_tiles, dim3(ntiles * (uint32_t)nstreams), dim3(64), 0, s, states, stride, n, ntiles, mask,
                       cwa_mask_words(n));
    return hipGetLastError();
}

hipError_t launch_wall_compose(const uint8_t *states, size_t stride, uint32_t width, uint32_t height, int nstreams,
                               const int32_t *place, const uint32_t *mask, uint8_t *wall, size_t wall_pitch, hipStream_t s) {
    const uint32_t mask_words = cwa_mask_words(3u * width * height);
    WallPlaceArgs h{};
    for (int s0 = 0; s0 < nstreams; s0 += kWallPlaceStreams) {
        h.first = s0;
        const int ns = nstreams - s0 < kWallPlaceStreams ? nstreams - s0 : kWallPlaceStreams;
        uint32_t blocks = 0;   // of the launch's stream that has the most
        for (int j = 0; j < ns; j++) {
            const int32_t *p = place + 3 * (size_t)(s0 + j);
            h.x[j] = p[0];
            h.y[j] = p[1];
            h.k[j] = p[2];
            if (p[2] < 1) continue;
            const uint32_t k = (uint32_t)p[2], tw = (width + k - 1u) / k, th = (height + k - 1u) / k;
            const uint32_t cp = wall_chunk_pixels(tw, k), b = th * ((tw + cp - 1u) / cp);
            blocks = b > blocks ? b : blocks;
        }
        if (blocks)
            hipLaunchKernelGGL(k_wall_compose, dim3(blocks, (uint32_t)ns), dim3(256), 0, s, states, stride, width, height, mask, mask_words,
                               wall, wall_pitch, h);
    }
    return hipGetLastError();
}

hipError_t launch_cwire_touched(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, bool accumulate, uint32_t *mask,
                                hipStream_t s) {
    if (nstreams <= 0 || nframes <= 0 || a.ntiles == 0) return hipSuccess;
    launch_cwa_directory(a, records, nstreams * nframes, s);
    hipLaunchKernelGGL(k_cw_touched, dim3((a.ntiles + 63u) / 64u * (uint32_t)nstreams), dim3(64), 0, s, a, nframes, accumulate ? 1 : 0, mask,
                       cwa_mask_words(a.n));
    return hipGetLastError();
}

hipError_t launch_thumb_cwire(const CwaArgs &a, int nstreams, uint32_t width, uint32_t height, uint32_t k, uint32_t threshold,
                              const uint32_t *mask, uint8_t *thumbs, size_t thumb_stride, const CwcOut &o, hipStream_t s) {
    if (nstreams <= 0) return hipSuccess;
    ThumbArgs h{};
    h.thumbs = thumbs;
    h.thumb_stride = thumb_stride;
    h.mask = mask;
    h.mask_words = cwa_mask_words(a.n);
    h.width = width;
    h.height = height;
    h.k = k;
    h.tw = (width + k - 1u) / k;
    h.th = (height + k - 1u) / k;
    h.threshold = threshold;
    CwaArgs at = a;   // the facts, the scan and the emit see the thumbnail's bytes and tiles; a.state / a.stride stay the states'
    at.n = 3u * h.tw * h.th;
    at.ntiles = cwa_tiles(at.n);
    if (at.ntiles) {   // (frames of no bytes have thumbnails of none: empty records)
        h.row = act_divisor(3u * h.tw);
        const uint32_t kw[2] = {k, width - (h.tw - 1u) * k}, kh[2] = {k, height - (h.th - 1u) * k};
        for (int i = 0; i < 4; i++) h.area[i] = act_divisor(kh[i >> 1] * kw[i & 1]);
    }
    const dim3 thumb_tiles(at.ntiles * (uint32_t)nstreams);   // (a wave per thumbnail tile and stream: one launch, no rounds)
    if (at.ntiles) hipLaunchKernelGGL(k_thumb_facts, thumb_tiles, dim3(64), 0, s, at, h);
    launch_cwc_tail(at, o, nstreams, true, s, [&](auto) {
        if (at.ntiles) hipLaunchKernelGGL(k_thumb_emit, thumb_tiles, dim3(64), 0, s, at, h, o);
    });
    return hipGetLastError();
}

ActDiv act_divisor(uint32_t d) { return ActDiv{d, d > 1u ? (uint32_t)(0x100000000ull / d) : ~0u}; }

static void launch_act_clear(const ActGeom &g, int nstreams, uint32_t *cells, uint32_t *summary, hipStream_t s) {
    const size_t ncells = (size_t)nstreams * g.cells;
    const size_t blocks = ((ncells > 8 * (size_t)nstreams ? ncells : 8 * (size_t)nstreams) + 255u) / 256u;
    hipLaunchKernelGGL(k_act_clear, dim3((uint32_t)(blocks > 2048u ? 2048u : blocks)), dim3(256), 0, s, cells, summary, ncells,
                       (uint32_t)nstreams);
}

hipError_t launch_cwire_activity(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, const ActGeom &g, bool accumulate,
                                 uint32_t *cells, uint32_t *summary, hipStream_t s) {
    if (nstreams <= 0 || nframes <= 0) return hipSuccess;
    if (a.ntiles) launch_cwa_directory(a, records, nstreams * nframes, s);
    if (!accumulate) launch_act_clear(g, nstreams, cells, summary, s);
    if (a.ntiles) hipLaunchKernelGGL(k_act_tile, dim3(a.ntiles * (uint32_t)nstreams), dim3(64), 0, s, a, nframes, g, cells, summary);
    hipLaunchKernelGGL(k_act_summary, dim3(nstreams), dim3(256), 0, s, (const uint32_t *)cells, summary, g.cells, g.min_count);
    return hipGetLastError();
}

hipError_t launch_activity(const uint32_t *d_offsets, const int32_t *xs, int nstreams, int nframes, const ActGeom &g, bool accumulate,
                           uint32_t *cells, uint32_t *summary, hipStream_t s) {
    if (nstreams <= 0 || nframes <= 0) return hipSuccess;
    if (!accumulate) launch_act_clear(g, nstreams, cells, summary, s);
    // device-side counts: a fixed grid strides over whatever the segments hold
    const size_t words = (size_t)nstreams * nframes + 1;
    const bool lds = words <= 8192;   // 32 KiB; more segments than that search the offsets where they are
    hipLaunchKernelGGL(k_act_entries, dim3(1024), dim3(256), lds ? words * sizeof(uint32_t) : 0, s, d_offsets, xs, (uint32_t)(words - 1),
                       act_divisor((uint32_t)nframes), g, cells, summary, lds ? 1 : 0);
    hipLaunchKernelGGL(k_act_summary, dim3(nstreams), dim3(256), 0, s, (const uint32_t *)cells, summary, g.cells, g.min_count);
    return hipGetLastError();
}

}  // namespace mi355

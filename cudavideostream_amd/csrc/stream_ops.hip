// stream_ops.hip -- the two small operators either side of the packed stream:
//
//   k_apply / k_apply_all : the client's reconstruction, client/opencv.cpp:64-66
//                           (`frame2.data[xs[i]] += buffer[i]` for the pos entries of a frame);
//   k_merge_parts         : concatenation of the streams of the row bands of ONE video stream that
//                           several cores (GPUs) packed independently into
//                           the single stream the sender would have produced;
//   k_cwire_*             : the compact wire format's encoder (packed stream -> gap-coded records) and decoder.
//
// The first two are index-driven byte scatter/copy: HBM-latency work with 5 bytes of traffic per entry, no
// arithmetic worth naming.
#include "internal.h"

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
// Record of frame t, 4-aligned, at frame_pos[t]:  u32 n | u32 e | u8 code[pad4(n)] | u32 esc[e] | u8 diff[pad4(n)]
// with g_0 = xs[0], g_k = xs[k] - xs[k-1] - 1, code[k] = min(g_k, 255) and esc[] the g_k of the codes 255, in order.
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
    uint32_t word = 0;
    const uint32_t i0 = 4 * d;
    uint32_t prev = i0 ? (uint32_t)xs[i0 - 1] : 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t i = i0 + j;
        g[j] = 0;
        esc[j] = false;
        if (i < n) {
            const uint32_t x = (uint32_t)xs[i];
            g[j] = i ? x - prev - 1u : x;
            prev = x;
            esc[j] = g[j] >= 255u;
            word |= (esc[j] ? 255u : g[j]) << (8 * j);
        }
    }
    return word;
}

__global__ __launch_bounds__(256) void k_cwire_count(const uint32_t *offsets, const int32_t *xs, uint64_t entries_capacity,
                                                     int nframes, uint32_t *cnt) {
    __shared__ uint32_t wsum[4];
    const int t = blockIdx.y, b = blockIdx.x, bpf = gridDim.x;
    const uint64_t total = offsets[nframes];
    uint32_t lo, n;
    if (total > entries_capacity || !cwire_frame_ok(offsets, t, total, &lo, &n)) return;
    const uint64_t D = (n + 3u) / 4u;
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
    __shared__ uint64_t s_wave[kCwScanThreads / 64];
    __shared__ uint64_t s_carry;
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    if (tid == 0) s_carry = 0;
    __syncthreads();
    if (s_bad) {
        if (tid == 0) frame_pos[nframes] = ~0ull;
        return;
    }
    for (int t0 = 0; t0 < nframes; t0 += kCwScanThreads) {
        const int t = t0 + tid;
        uint64_t rec = 0;
        if (t < nframes) {
            uint32_t e = 0;
            for (int b = 0; b < bpf; b++) {   // exclusive prefix of the frame's escapes per workgroup of the emit kernel
                const uint32_t c = s_cnt[t * bpf + b];
                cnt[(size_t)t * bpf + b] = e;
                e += c;
            }
            const uint64_t n = offsets[t + 1] - offsets[t];
            rec = 8 + 2 * ((n + 3) & ~3ull) + 4 * (uint64_t)e;
        }
        uint64_t incl = rec;   // inclusive scan of the record sizes over the wave, then over the waves
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const uint64_t v = __shfl_up(incl, k, 64);
            if (lane >= k) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t before = s_carry;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        if (t < nframes) frame_pos[t] = before + incl - rec;
        __syncthreads();
        if (tid == kCwScanThreads - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) frame_pos[nframes] = s_carry;
}

__global__ __launch_bounds__(256) void k_cwire_emit(const uint32_t *offsets, const int32_t *xs, const uint8_t *diff,
                                                    uint64_t entries_capacity, int nframes, const uint32_t *cnt,
                                                    const uint64_t *frame_pos, uint8_t *out, uint64_t capacity_bytes) {
    __shared__ uint32_t s_wave[2][4];
    const int t = blockIdx.y, b = blockIdx.x, bpf = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t total = offsets[nframes];
    uint32_t lo, n;
    if (total > entries_capacity || frame_pos[nframes] == ~0ull || !cwire_frame_ok(offsets, t, total, &lo, &n)) return;
    const uint64_t fp0 = frame_pos[t], fp1 = frame_pos[t + 1];
    if (fp1 > capacity_bytes) return;   // the frame does not fit: skipped whole
    const uint64_t D = (n + 3u) / 4u;
    const uint64_t ebytes = fp1 - fp0 - 8 - 8 * D;   // 4 e
    const uint32_t e = (uint32_t)(ebytes / 4);
    uint32_t *hdr = (uint32_t *)(out + fp0);
    uint32_t *code = hdr + 2, *esc = code + D, *dif = esc + e;
    if (b == 0 && threadIdx.x == 0) {
        hdr[0] = n;
        hdr[1] = e;
    }
    const int32_t *fx = xs + lo;
    const uint8_t *fd = diff + lo;
    const uint32_t d0 = (uint32_t)(D * b / bpf), d1 = (uint32_t)(D * (b + 1) / bpf);
    const uint64_t lt = (1ull << lane) - 1ull;
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
        uint32_t before = 0, wtot = 0;   // escapes of the lanes below this one in the wave, and of the whole wave
        uint64_t m[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            m[j] = __ballot(fl[j]);
            before += (uint32_t)__popcll(m[j] & lt);
            wtot += (uint32_t)__popcll(m[j]);
        }
        if (lane == 0) s_wave[buf][wave] = wtot;
        __syncthreads();
        uint32_t rank = carry + before;
        for (int w = 0; w < wave; w++) rank += s_wave[buf][w];
        carry += s_wave[buf][0] + s_wave[buf][1] + s_wave[buf][2] + s_wave[buf][3];
        if (live) {
            code[d] = word;
            dif[d] = dw;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (fl[j]) {
                    if (rank < e) esc[rank] = g[j];   // (only input that changed between the launches breaks rank < e)
                    rank++;
                }
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
// running sum of g + 1, minus 1.  Reads stay inside [pos, pos + 8 + 2 pad4(n) + 4 e); an escape ranked at or past e
// decodes to 0xFFFFFFFF (and adds nothing to the running sum); entries at or past `capacity` are not written.
__global__ __launch_bounds__(256) void k_cwire_decode(const CwireDecodeArgs a) {
    __shared__ uint32_t s_esc[2][4], s_sum[2][4];
    const CwireFrame f = a.frame[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        if (a.first_frame + blockIdx.x == 0) a.offsets[0] = 0;
        a.offsets[a.first_frame + blockIdx.x + 1] = f.out + f.n;
    }
    const uint32_t D = (f.n + 3u) / 4u;
    const uint32_t *code = (const uint32_t *)(a.cwire + f.pos + 8);
    const uint32_t *esc = code + D, *dif = esc + f.e;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t carry_e = 0, carry_x = 0;
    int buf = 0;
    for (uint32_t base = 0; base < D; base += 256, buf ^= 1) {
        const uint32_t d = base + threadIdx.x;
        const bool live = d < D;
        uint32_t word = live ? code[d] : 0u, dw = live ? dif[d] : 0u;
        bool fl[4];
        uint32_t before = 0, wtot = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            fl[j] = live && 4 * d + j < f.n && ((word >> (8 * j)) & 255u) == 255u;
            const uint64_t m = __ballot(fl[j]);
            before += (uint32_t)__popcll(m & lt);
            wtot += (uint32_t)__popcll(m);
        }
        if (lane == 0) s_esc[buf][wave] = wtot;
        __syncthreads();
        uint32_t rank = carry_e + before;
        for (int w = 0; w < wave; w++) rank += s_esc[buf][w];
        uint32_t inc[4], lsum = 0;
        bool bad[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            inc[j] = 0;
            bad[j] = false;
            if (live && 4 * d + j < f.n) {
                uint32_t g = (word >> (8 * j)) & 255u;
                if (fl[j]) {
                    if (rank < f.e) g = esc[rank];
                    else bad[j] = true;
                    rank++;
                }
                inc[j] = bad[j] ? 0u : g + 1u;
            }
            lsum += inc[j];
        }
        uint32_t incl = lsum;   // inclusive scan of the lanes' sums over the wave, then over the waves
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const uint32_t v = __shfl_up(incl, k, 64);
            if (lane >= k) incl += v;
        }
        if (lane == 63) s_sum[buf][wave] = incl;
        __syncthreads();
        uint32_t x = carry_x + incl - lsum;
        for (int w = 0; w < wave; w++) x += s_sum[buf][w];
        carry_e += s_esc[buf][0] + s_esc[buf][1] + s_esc[buf][2] + s_esc[buf][3];
        carry_x += s_sum[buf][0] + s_sum[buf][1] + s_sum[buf][2] + s_sum[buf][3];
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

}  // namespace mi355

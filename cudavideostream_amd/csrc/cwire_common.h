// cwire_common.h -- the compact wire format (include/mi355diff.h, "compact wire"), once, for host and device:
// the record's arithmetic and sections, the encode / decode step of a lane's four entries, and the workgroup scans
// of its kernels (stream_ops.hip: encoder, decoder, GPU client; diff_pack.hip: the log straight into records;
// core.hip: sizes, header walk, host client).
// Record of frame t, 4-aligned, at frame_pos[t]:  u32 n | u32 e | u8 code[pad4(n)] | u32 esc[e] | u8 diff[pad4(n)]
// with g_0 = xs[0], g_k = xs[k] - xs[k-1] - 1, code[k] = min(g_k, 255) and esc[] the g_k of the codes 255, in order.
#ifndef MI355_CWIRE_COMMON_H_
#define MI355_CWIRE_COMMON_H_

#include <type_traits>

#include "internal.h"

namespace mi355 {

__host__ __device__ inline uint64_t cwire_pad4(uint64_t x) { return (x + 3) & ~3ull; }
__host__ __device__ inline uint32_t cwire_dwords(uint32_t n) { return (n + 3u) / 4u; }   // code (or diff) dwords (32-bit, as the kernels always counted them)
__host__ __device__ inline uint64_t cwire_record_bytes(uint64_t n, uint64_t e) { return 8 + 2 * cwire_pad4(n) + 4 * e; }
// e of a record of `bytes` bytes with n entries
__host__ __device__ inline uint32_t cwire_record_escapes(uint64_t bytes, uint32_t n) {
    return (uint32_t)((bytes - 8 - 2 * cwire_pad4(n)) / 4);
}

// The run form of a record for the link (include/mi355diff.h, "Run-coded records"):
//   u32 n | u32 e | u32 r | u8 gap[pad4(r)] | u8 len[pad4(r)] | u32 esc[e] | u8 diff[pad4(n)]
// Entry k starts a run when k % 256 == 0 or code[k] != 0; gap = the start's code, len = the run's entries - 1.
__host__ __device__ inline uint64_t cwire_runs_bytes(uint64_t n, uint64_t e, uint64_t r) { return 12 + 2 * cwire_pad4(r) + 4 * e + cwire_pad4(n); }
__host__ __device__ inline bool cwire_run_start(uint32_t k, uint32_t code) { return (k & 255u) == 0 || code != 0; }
// the run form is strictly smaller than the compact record
__host__ __device__ inline bool cwire_runs_smaller(uint64_t n, uint64_t r) { return 4 + 2 * cwire_pad4(r) < cwire_pad4(n); }
// the bytes of record {n, e, r} on the link in either form (form != 0: the run form)
__host__ __device__ inline uint64_t cwire_link_bytes(uint32_t form, uint64_t n, uint64_t e, uint64_t r) {
    return form ? cwire_runs_bytes(n, e, r) : cwire_record_bytes(n, e);
}
// the dwords [lo, hi) of a section of `total` dwords that part j of nparts copies
__host__ __device__ inline void cwire_share(uint32_t total, uint32_t j, uint32_t nparts, uint32_t &lo, uint32_t &hi) {
    lo = (uint32_t)((uint64_t)total * j / nparts);
    hi = (uint32_t)((uint64_t)total * (j + 1) / nparts);
}

// Where the sections of the record {n, e} at base + pos are.  Byte = uint8_t or const uint8_t.
template <class Byte>
struct CwireSections {
    typedef typename std::conditional<std::is_const<Byte>::value, const uint32_t, uint32_t>::type Word;
    Byte *code, *esc, *diff;   // pad4(n) codes, e escapes of 4 bytes, pad4(n) differences
    __host__ __device__ CwireSections(Byte *base, uint64_t pos, uint32_t n, uint32_t e)
        : code(base + pos + 8), esc(code + cwire_pad4(n)), diff(esc + 4 * (uint64_t)e) {}
    // as dwords (the GPU entry points take a 4-aligned stream)
    __host__ __device__ Word *code32() const { return (Word *)code; }
    __host__ __device__ Word *esc32() const { return (Word *)esc; }
    __host__ __device__ Word *diff32() const { return (Word *)diff; }
};

// ---- a lane's four entries ------------------------------------------------------------------------------------------
// Encode: entry j (where ok[j]; they are the first of the four) has index x[j]; end = 1 + the index of the entry before
// the four (0: none).  Returns the code dword (0 in the bytes of the entries that are not there); fl[j]: entry j is
// there and escaped, g[j] its gap.
__device__ __forceinline__ uint32_t cwire_encode4(const uint32_t x[4], const bool ok[4], uint32_t end, uint32_t g[4], bool fl[4]) {
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        g[j] = x[j] - end;
        end = x[j] + 1u;
        fl[j] = ok[j] && g[j] >= 255u;
        word |= (ok[j] ? (g[j] < 255u ? g[j] : 255u) : 0u) << (8 * j);
    }
    return word;
}

// Flags -> how many the lanes below this one hold (ballot + popcount); wtot: how many the wave holds
__device__ __forceinline__ uint32_t cwire_rank4(const bool fl[4], uint32_t &wtot) {
    const uint64_t lt = (1ull << (threadIdx.x & 63u)) - 1ull;
    uint32_t before = 0;
    wtot = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t m = __ballot(fl[j]);
        before += (uint32_t)__popcll(m & lt);
        wtot += (uint32_t)__popcll(m);
    }
    return before;
}

// The escaped gaps of the four go to esc[rank], esc[rank + 1], ... (only input that changed between the launches of an
// encoder breaks rank < e)
template <bool NONTEMPORAL>
__device__ __forceinline__ void cwire_store_escapes(uint32_t *esc, uint32_t e, uint32_t rank, const uint32_t g[4], const bool fl[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (fl[j]) {
            if (rank < e) {
                if (NONTEMPORAL) __builtin_nontemporal_store(g[j], esc + rank);
                else esc[rank] = g[j];
            }
            rank++;
        }
}

// Decode, first half: the escape codes (fl[j]) among the live entries (in[j]) of a code dword -> those of the lanes
// below, and of the wave
__device__ __forceinline__ uint32_t cwire_escapes_before(uint32_t word, const bool in[4], bool fl[4], uint32_t &wtot) {
#pragma unroll
    for (int j = 0; j < 4; j++) fl[j] = in[j] && ((word >> (8 * j)) & 255u) == 255u;
    return cwire_rank4(fl, wtot);
}

// Decode, second half: rank = escapes of the frame before the lane's.  inc[j] = g + 1 of the live entries, the running
// index's increments; rk[j] the escape rank at entry j.  An escape ranked at or past e is BAD: it adds nothing (inc 0).
// Returns the sum of the four increments.
__device__ __forceinline__ uint32_t cwire_decode4(uint32_t word, const bool in[4], const bool fl[4], uint32_t rank, uint32_t e, const uint32_t *esc,
                                                  uint32_t inc[4], bool bad[4], uint32_t rk[4]) {
    uint32_t lsum = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        inc[j] = 0;
        bad[j] = false;
        rk[j] = rank;
        if (in[j]) {
            uint32_t g = (word >> (8 * j)) & 255u;
            if (fl[j]) {
                if (rank < e) g = esc[rank];
                else bad[j] = true;
                rank++;
            }
            inc[j] = bad[j] ? 0u : g + 1u;
        }
        lsum += inc[j];
    }
    return lsum;
}

// ---- workgroup scans (NW waves; T = uint32_t or uint64_t) -----------------------------------------------------------
template <class T>
__device__ __forceinline__ T wave_inclusive_scan_shfl(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const T u = __shfl_up(v, k, 64);
        if (lane >= k) v += u;
    }
    return v;
}

// carry + the totals of the waves below this one; carry += the totals of all waves.  Lane src_lane of a wave holds its
// total in v.  s_wave: NW words of LDS that the caller owns and does not hand in again before another barrier (it
// alternates two, or ends its round with one).  One barrier; a single wave needs neither the barrier nor s_wave.
template <int NW, class T>
__device__ __forceinline__ T block_waves_before(T v, int src_lane, T *s_wave, T &carry) {
    T before = carry;
    if (NW == 1) {
        carry += (T)__shfl(v, src_lane, 64);
        return before;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == src_lane) s_wave[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; w++) before += s_wave[w];
#pragma unroll NW <= 4 ? NW : 1   // (sixteen 64-bit totals in flight at once cost a 1024-thread kernel a wave of occupancy)
    for (int w = 0; w < NW; w++) carry += s_wave[w];
    return before;
}

// carry + the values of the threads below this one; carry += all values
template <int NW, class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *s_wave, T &carry) {
    const T incl = wave_inclusive_scan_shfl(v);
    return block_waves_before<NW>(incl, 63, s_wave, carry) + incl - v;
}

// frame_pos[0 .. nframes] = exclusive scan of the record sizes, by ONE workgroup of THREADS threads.  header(t, n, e)
// gives frame t's header, placed(t, pos, n, e) is told where it lies.  Each is called exactly once per frame, by one
// thread, header first, and may have side effects (k_cwire_scan's turns the emit kernel's escape counts into their
// prefix while it sums them); n and e enter header as 0.
template <int THREADS, class Header, class Placed>
__device__ __forceinline__ void cwire_scan_frame_pos(int nframes, uint64_t *frame_pos, Header header, Placed placed) {
    __shared__ uint64_t s_wave[THREADS / 64];
    const int tid = threadIdx.x;
    uint64_t carry = 0;
    for (int t0 = 0; t0 < nframes; t0 += THREADS) {
        const int t = t0 + tid;
        uint32_t n = 0, e = 0;
        if (t < nframes) header(t, n, e);
        const uint64_t rec = t < nframes ? cwire_record_bytes(n, e) : 0;
        const uint64_t pos = block_exclusive_scan<THREADS / 64>(rec, s_wave, carry);
        if (t < nframes) {
            frame_pos[t] = pos;
            placed(t, pos, n, e);
        }
        __syncthreads();   // s_wave is rewritten by the next round
    }
    if (tid == 0) frame_pos[nframes] = carry;
}

// ---- parity for the datagram path (include/mi355diff.h, "Parity pieces"): GF(2^8) modulo 0x11D on packed dwords ----------
// Every byte of v times 2
__host__ __device__ inline uint32_t fec_xtime(uint32_t v) { return ((v & 0x7f7f7f7fu) << 1) ^ (((v >> 7) & 0x01010101u) * 0x1du); }
// Every byte of v times the constant c: eight shift-and-XOR steps under a uniform constant
__host__ __device__ inline uint32_t fec_mul(uint32_t v, uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        r ^= (c >> k) & 1u ? v : 0u;
        v = fec_xtime(v);
    }
    return r;
}

// The record of global group g: the r with fec_first[r] <= g < fec_first[r + 1] (g below fec_first[nrecords])
__host__ __device__ inline int fec_group_record(const uint32_t *fec_first, int nrecords, uint32_t g) {
    int lo = 0, hi = nrecords;   // fec_first[lo] <= g < fec_first[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (fec_first[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Group g: its first piece p0 and its members m.  Returns its length L_g, 0 for a void group -- a member absent or malformed
// (include/mi355diff.h, "Void groups").  Members lane, lane + step, ... are tested: a host caller passes (0, 1), a wave (lane, 64)
// and combines the lanes' answers (any 0: void; else the largest).  Reads piece_first[r], [r + 1], and piece_pos[p], [p + 1]
// only for p < piece_capacity.
struct FecGroup {
    uint64_t p0;
    uint32_t m;
};
__host__ __device__ inline FecGroup fec_group(const uint32_t *fec_first, const uint32_t *piece_first, int nrecords, uint32_t group, uint32_t g) {
    const int r = fec_group_record(fec_first, nrecords, g);
    const uint32_t c = piece_first[r + 1] - piece_first[r];
    const uint64_t at = (uint64_t)(g - fec_first[r]) * group;
    FecGroup fg;
    fg.p0 = (uint64_t)piece_first[r] + at;
    fg.m = at < c ? (c - at < group ? (uint32_t)(c - at) : group) : 0u;
    return fg;
}
// One member: its length, 0 when absent or malformed
__host__ __device__ inline uint32_t fec_member_len(const uint64_t *piece_pos, uint64_t piece_capacity, uint64_t pieces_bytes, uint32_t pitch,
                                                   uint64_t p) {
    if (p >= piece_capacity) return 0;
    const uint64_t a = piece_pos[p], b = piece_pos[p + 1];
    if (b > pieces_bytes || b <= a || ((a | b) & 3u) || b - a > pitch) return 0;
    return (uint32_t)(b - a);
}
// The verdict of a rebuilt block's header {n, e} (bit 0: MI355_FEC_BAD_HEADER); *tail: the first byte that has to be zero
__host__ __device__ inline uint32_t fec_header_verdict(uint32_t n, uint32_t e, uint32_t fec_len, uint64_t *tail) {
    const uint64_t bytes = cwire_record_bytes(n, e);
    *tail = bytes < fec_len ? bytes : fec_len;
    return n == 0 || e > n || bytes > fec_len ? 1u : 0u;
}

}  // namespace mi355
#endif

// core.hip -- the C-ABI of libmi355diff.so (include/mi355diff.h): context, HBM layout, orchestration.
//
// Host-side counterpart of diff::cuda::CUDACore (reference server/src/kernels.cu:377-536).  HBM layout
// of one core (N = 3*width*height, W = ceil(N/1024) tiles, T = max_batch):
//   state     N            the client's reconstructed frame (d_current/d_previous pair of the
//                          reference collapsed into one persistent buffer)
//   in, aux, vis  N each   exec(): uploaded frame, filter scratch, visualisation frame
//   codes     ceil(T/4)*W*1024  code log written by k_diff_pack: 4 bytes per candidate lane (worst case: every lane
//                          of every frame), chunk-interleaved over tiles
//   rec       T*W*64*16    record log: 16 masked diff bytes per lane with two or more flagged bytes
//   meta      T*W*16       per (frame, tile): code position, record position, flagged bytes, candidates | multi << 16
//   groff     T*ceil(W/64)*16 (a prefix per range of 16 tiles);  totals T*8 {total, epoch} + the ticket;  offsets (T+1)*4
//   one_xs N*4, one_diff N exec(): packed output of a single frame before the D2H copies
//   cw_cnt    32 KiB       the compact-wire encoder's escape counts per workgroup
//   cw_rec    8 + 2*pad4(N) (rounded up to 16) + 16  mi355_exec_cwire / mi355_pipe_submit_cwire: the frame's record before its
//                          export and its frame_pos[2]; made by the first such call (or MI355_PREPARE_EXEC_CWIRE)
//   cw_items  T*ceil(W/16)*16 + T*4  mi355_diff_stream_cwire_batch: one word per item of the expansion, escapes per frame
//   cwa_*     T*24 + 2*T*ceil(N/4096)*16  mi355_apply_cwire_batch: frame table, chunk facts, tile directory
//   cws_*     2*T*max(1, ceil(N/65536))*16  mi355_cwire_split_cwire_batch: per block of 65536 entries its pieces and bytes, their bases
//   cwr_*     T*40 + T*max(1, ceil(N/1024))*8  mi355_cwire_runs_decode_batch: record table, one word per workgroup of 1024 runs
//   hist T*256*4, thr T*4 (per frame of a filter batch), k9 9*4, heat LUT 766*3, glyph atlas
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/mi355diff.h"
#include "cwire_common.h"

using namespace mi355;

// KiB chunks of one tile's code log: a frame appends at most 64 codes, a chunk holds 256
// (a frame's codes never straddle chunks: a chunk is left with fewer than 64 free places, i.e. more than 192 used)
static inline size_t code_chunks(size_t max_batch) { return (max_batch + 2) / 3 + 1; }

namespace {

thread_local std::string g_err;

int fail(int code, const char *what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s (%s)", what, hipGetErrorName(e), hipGetErrorString(e));
    else
        snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                             \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return fail(MI355_ERR_HIP, #expr, _e); \
    } while (0)

}  // namespace

struct mi355_core {
    mi355_config cfg{};
    int device = 0;
    uint32_t n = 0;        // bytes per frame
    uint32_t ntiles = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    uint8_t *state = nullptr, *in = nullptr, *aux = nullptr, *vis = nullptr;
    uint4 *rec = nullptr, *meta = nullptr;
    uint32_t *codes = nullptr;
    uint32_t *groff = nullptr, *totals = nullptr;   // totals: T tagged 64-bit words + the scan kernel's ticket (2T + 2 words)
    uint64_t scan_epoch = 0;      // tag of the last k_scan_groups launch, 1 .. kEpochWrap - 1 (internal.h, next_scan_epoch)
    uint32_t *offsets = nullptr;  // T+1, used by exec()
    int32_t *one_xs = nullptr;
    uint8_t *one_diff = nullptr;
    int32_t *hist = nullptr, *thr = nullptr;
    uint32_t *red_bounds = nullptr; // mi355_red_stream_batch (cleared form): entry ranges of the frame slices
    uint32_t *cw_cnt = nullptr;     // mi355_cwire_encode_batch: escapes per workgroup of the emit kernel (kCwireSlots words)
    // mi355_exec_cwire / mi355_pipe_submit_cwire (made on first use, need_exec_cwire): the frame's record on the device
    // (cw_rec_bytes = mi355_cwire_bytes_max(N, 1); the allocation is that rounded up to 16) and its frame_pos[2].  One buffer
    // serves every slot of the ring, as one_xs does: encode and export of a frame run back to back on the core's stream.
    uint8_t *cw_rec = nullptr;
    uint64_t *cw_rec_pos = nullptr;
    uint64_t cw_rec_bytes = 0;
    // ... and what k_export_record reports, pinned: kRecWords words {n, e, bytes low, bytes high} per slot of the ring, then
    // those of the blocking form, then 16 bytes of scratch (the warm pass's record; the pageable form's read-back)
    static constexpr int kRecWords = 4;
    uint32_t *h_rec = nullptr;
    bool cw_warm = false;             // the warm pass of the encode and export kernels has run and gave the empty record
    uint4 *cw_items = nullptr;      // mi355_diff_stream_cwire_batch: [T][ceil(W/16)] item words (diff_pack.hip, k_cwire_items)
    uint32_t *cw_esc = nullptr;     // ... and [T] escapes per frame
    CwaFrame *cwa_ftab = nullptr;   // mi355_apply_cwire_batch (stream_ops.hip): [T] frame headers of a slice,
    uint4 *cwa_chunk = nullptr;     // [T * cwa_chunks(N)] chunk facts,
    uint4 *cwa_dir = nullptr;       // [T][cwa_tiles(N)] directory words
    uint4 *cws_blk = nullptr;       // mi355_cwire_split_cwire_batch (stream_ops.hip): [T * cws_blocks(N)] block words
    ulonglong2 *cws_base = nullptr; // ... and the pieces and bytes before each block
    CwrRecord *cwr_rtab = nullptr;  // mi355_cwire_runs_decode_batch (stream_ops.hip): [T] records of a call,
    uint2 *cwr_chunk = nullptr;     // [T * cwr_chunks_max(N)] one word per workgroup
    uint32_t *cwb_hist = nullptr;   // mi355_cwire_budget_cwire_batch: [T][kCwbWords] bins of |cur - prev|, budget and threshold per stream
    // mi355_cwire_despeckle_cwire_batch (made on first use, need_despeckle): [2][T][dsp_words(N)] pixel bitmaps, changed then keep
    uint32_t *dsp_bits = nullptr;
    uint8_t *gray1 = nullptr;      // fused gray+binarize chain: one gray byte per pixel of a batch, made on first use
    size_t gray1_stride = 0;
    float *k9 = nullptr;
    float *kxk = nullptr;          // mi355_conv_kxk: up to 81 taps, made on first use
    uint8_t *lut = nullptr;
    uint8_t *glyphs = nullptr;
    int nglyphs = 0, glyph_h = 0, glyph_w = 0;
    std::string charset;
    bool have_k9 = false, k9_sym = false;   // k9_sym: corners equal and edges equal, bit for bit
    size_t workspace = 0;

    uint32_t *h_count = nullptr;  // pinned, 2 x u32 (offsets[0..1] of exec)

    // pipelined per-frame path (mi355_pipe_*): a ring of slots, uploads on their own stream
    static constexpr int kMaxSlots = 8;
    struct Slot {
        uint8_t *d_in = nullptr, *d_vis = nullptr;
        uint32_t *h_count = nullptr;                   // pinned, written by k_export
        hipEvent_t uploaded = nullptr, painted = nullptr, packed = nullptr, shown = nullptr;
        bool has_vis = false;
        bool compact = false;                          // submitted by mi355_pipe_submit_cwire: the results are in h_rec
        int64_t ticket = -1;                           // frame in flight in this slot, -1 = free
    };
    Slot slots[kMaxSlots];
    int nslots = 0;
    int64_t next_ticket = 0;
    hipStream_t up_stream = nullptr, down_stream = nullptr;

    // Pipelined batches (own stream only): the index and the expansion of batch k run on `side` beside the pack
    // kernel of batch k + 1 on the core's stream.  Two sets of logs, used alternately; set[0] is {rec, codes, meta,
    // groff, totals} above, set[1] is made when the mode is first used.
    struct LogSet {
        uint4 *rec = nullptr, *meta = nullptr;
        uint32_t *codes = nullptr, *groff = nullptr, *totals = nullptr;
        hipEvent_t packed = nullptr, expanded = nullptr;   // pack kernel done (main) / expansion done (side)
        bool in_use = false;                                // `expanded` has been recorded at least once
    };
    static constexpr int kSets = 2;   // (a third set was measured: no gain, profiles/archive/r04ay)
    LogSet set[kSets];
    int flip = 0;
    hipStream_t side = nullptr;
    hipEvent_t side_done = nullptr;   // == the `expanded` event of the last pipelined batch, or null: nothing pending
    bool pipeline_ok = true;          // false: MI355_PIPELINE=0 / MI355_OPT_PIPELINE 0, or the second set could not be allocated
    int median_rows = 0;              // MI355_OPT_MEDIAN_ROWS (0: chosen per launch)
    uint32_t cu_count = 0;            // compute units of the device (0: unknown)
    // pipelined batches of 64 tiles or more are packed by TWO launches (tiles [0, cut) on the core's stream, the rest on
    // `main2`): the two chains of pack kernels drift apart, each one's kernel boundary (L2 write-back, event packets:
    // 21-25 us) falls into the other's kernel.
    // (three or four launches were measured: much slower, profiles/archive/r04ah)
    hipStream_t main2 = nullptr;
    hipEvent_t packed2[kSets] = {};
    // Adaptive overlap: a batch whose expansion is longer than its pack kernel (dense input: a scene change, the synthetic
    // worst cases) loses by running beside the next batch's pack kernel (S0 pairs 0.313 ms one after the other, 0.35
    // overlapped).  The batch total (offsets[nframes]) of every own-stream batch is copied to pinned host memory behind its
    // expansion; the next calls look at the latest total that HAS ARRIVED (a word of pinned memory the index kernel stores, no
    // waiting) and run one batch after the other while more than kDensePct per cent of the bytes changed.  Results never
    // depend on it, only the schedule.
    static constexpr uint32_t kDensePct = 40;
    uint64_t *h_tot = nullptr;        // pinned: {entries of the latest own-stream batch whose index has run, its frames << 32},
                                      // stored by that batch's index kernel itself (k_scan_groups, `note`)
    bool dense = false;               // what the latest total that has arrived said
    bool filter_since_batch = false;  // a frame filter ran on this core since the last batch (use_device_filter)
    hipEvent_t fork[kSets] = {};          // recorded on the core's stream in front of a batch's first pack launch: the other parts wait for it
    int parts_pending = -1;           // log set of the last batch whose parts the core's stream has not waited for (-1: none)
    // Feedback pairs (mi355_diff_multi_*) write the CALLER's states, half of every state on `main2` when the pack is split.
    // Tick k + 1 on the same states needs no wait: a tile's bytes are read and written by the launches of one stream only,
    // tick after tick, as the core's own state is.  Any other batch that follows may read those states at other tile
    // positions (mi355_diff_pairs_batch with the states as an operand, other states that overlap these), so it first lets
    // the core's stream wait for the parts (run_batch).
    const void *fb_states = nullptr;  // states and stride of the last split feedback batch the core's stream has not
    size_t fb_stride = 0;             // waited for (nullptr: none)

    // timing: ring of event sets {before pack, after pack, before scan, after scan, after expand, after the second pack
    // launch of a split batch}, harvested lazily so that timed batches still queue back to back
    static constexpr int kEvRing = 32, kEvPer = 6;
    bool timing = false;
    hipEvent_t ev[kEvRing][kEvPer] = {};
    bool ev_split[kEvRing] = {};
    int ev_head = 0, ev_count = 0;  // oldest pending slot, number pending
    double ms_pack = 0, ms_scan = 0, ms_expand = 0, ms_total = 0;
    int launches = 0;
};

namespace mi355 {
int set_error(int code, const char *what) { return fail(code, what); }
hipStream_t core_stream(::mi355_core *c) {   // for work other translation units enqueue: after the last pipelined batch
    if (c->side_done && hipSetDevice(c->device) == hipSuccess && hipStreamWaitEvent(c->stream, c->side_done, 0) == hipSuccess)
        c->side_done = nullptr;
    return c->stream;
}
int core_device(const ::mi355_core *c) { return c->device; }
}  // namespace mi355

namespace {

// A stream of the core.  MI355_FLAG_OWN_QUEUES: in the least stream-priority class, whose hardware queues no framework's
// stream pool shares (include/mi355diff.h); else the default class.
hipError_t make_stream(const mi355_core *c, hipStream_t *s) {
    if (c->cfg.flags & MI355_FLAG_OWN_QUEUES) {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
            return hipStreamCreateWithPriority(s, hipStreamNonBlocking, least);
        (void)hipGetLastError();
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

template <class T>
int dev_alloc(mi355_core *c, T **p, size_t count) {
    const size_t bytes = count * sizeof(T);
    HIP_TRY(hipMalloc((void **)p, bytes ? bytes : 16));
    c->workspace += bytes;
    return MI355_OK;
}

// Every entry point starts here.  join: whatever the entry point enqueues on the core's stream (or waits for) comes
// after the expansion of the last pipelined batch, which runs on the side stream; only the pipelined batch path
// itself passes false (it orders its own kernels with events).
// parts: a pipelined batch is packed by launches on SEVERAL streams (run_batch); whatever follows on the core's stream must
// not overtake the parts that run elsewhere -- a frame filter that rewrites the buffer the batch is still reading, say.
// Only the next pipelined batch passes false here too (its own parts queue up behind the last batch's on their streams).
int use_device(mi355_core *c, bool join = true, bool parts = true) {
    HIP_TRY(hipSetDevice(c->device));
    if (join && c->side_done) {
        HIP_TRY(hipStreamWaitEvent(c->stream, c->side_done, 0));   // (the expansion waited for every part)
        c->side_done = nullptr;
        c->parts_pending = -1;
    }
    if (parts && c->parts_pending >= 0) {
        HIP_TRY(hipStreamWaitEvent(c->stream, c->packed2[c->parts_pending], 0));
        c->parts_pending = -1;
    }
    return MI355_OK;
}

// A frame filter takes frames, not packed streams: it does not wait for a pipelined batch that is still expanding on the
// side stream.  It leaves a hint, though: a caller that alternates filters and batches (the server's visualiser or noise
// filter in front of every diff: BASELINE configs 3 and 4) gains nothing from a batch's expansion running beside the next
// filter -- both are bound by the memory system -- and loses the pipelined batch's smaller pack grid and stream hops:
// 4.6 us per frame one after the other, 5.0-5.2 overlapped (config 3, profiles/archive/r04bd).  The next batch therefore runs one
// kernel after the other on the core's stream.
int use_device_filter(mi355_core *c) {
    c->filter_since_batch = true;
    return use_device(c, false);
}

// Fold pending event sets into the sums: all of them (blocking) or only until `keep` remain.
int harvest_timing(mi355_core *c, int keep = 0) {
    while (c->ev_count > keep) {
        hipEvent_t *e = c->ev[c->ev_head];
        HIP_TRY(hipEventSynchronize(e[4]));
        float a = 0, b = 0, d = 0, t = 0;
        HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
        if (c->ev_split[c->ev_head]) {   // two launches on two streams: the later end counts
            float a2 = 0;
            HIP_TRY(hipEventElapsedTime(&a2, e[0], e[5]));
            a = a2 > a ? a2 : a;
        }
        HIP_TRY(hipEventElapsedTime(&b, e[2], e[3]));
        HIP_TRY(hipEventElapsedTime(&d, e[3], e[4]));
        HIP_TRY(hipEventElapsedTime(&t, e[0], e[4]));   // the batch's way through the path (batches overlap when pipelined)
        c->ms_pack += a;
        c->ms_scan += b;
        c->ms_expand += d;
        c->ms_total += t;
        c->launches += 1;
        c->ev_head = (c->ev_head + 1) % mi355_core::kEvRing;
        c->ev_count -= 1;
    }
    return MI355_OK;
}

// tests/heat_map_benchmark/cpu.cu:19-27 for d = 0..765, stored B,G,R (cpu.cu:62-64).
void build_heat_lut(uint8_t *lut) {
    for (int diff = 0; diff <= 765; diff++) {
        float diff1 = diff / (255.0 * 2.0);
        double r = sin(M_PI * diff1 - M_PI / 2.0) * 255.0;
        double g = sin(M_PI * diff1) * 255.0;
        double b = sin(M_PI * diff1 + M_PI / 2.0) * 255.0;
        r = r > 0.0 ? r : 0.0; r = r < 255.0 ? r : 255.0;
        g = g > 0.0 ? g : 0.0; g = g < 255.0 ? g : 255.0;
        b = b > 0.0 ? b : 0.0; b = b < 255.0 ? b : 255.0;
        lut[diff * 3 + 0] = (uint8_t)(int)b;
        lut[diff * 3 + 1] = (uint8_t)(int)g;
        lut[diff * 3 + 2] = (uint8_t)(int)r;
    }
}

// Scratch of the fused gray+binarize chain (one byte per pixel, max_batch frames): made when first needed.
int need_gray1(mi355_core *c) {
    if (c->gray1 || c->n == 0) return MI355_OK;
    c->gray1_stride = ((size_t)c->n / 3 + 15) & ~(size_t)15;
    return dev_alloc(c, &c->gray1, c->gray1_stride * (size_t)c->cfg.max_batch);
}

// Every frame total of both log sets back to "never written" (the launch tags wrap, or a test moves them).  The caller has
// synchronised the core's streams.  The first version cleared with plain hipMemset calls -- served by the null stream / the
// runtime's own fill path, not by the core's streams -- and tests/soak_chain.py (round 6, the tag moved at random) then stopped
// in the index kernel's reader, waiting for a total that had been published: 3 runs of 3; with the clears enqueued on the core's
// stream and waited for, 5 of 5 ran to the end (tools/exp/r06s.sh).  What exactly let the published word be lost was not
// established (a core created while the null stream is busy behaves the same with either form: test_core_created_while_the_
// null_stream_is_busy); every clear of the core's own buffers goes the ordered way since.
int clear_totals(mi355_core *c) {
    const size_t bytes = 2 * (size_t)c->cfg.max_batch * sizeof(uint32_t);   // (the ticket behind them is 0 between launches)
    HIP_TRY(hipMemsetAsync(c->totals, 0, bytes, c->stream));
    if (c->set[1].totals) HIP_TRY(hipMemsetAsync(c->set[1].totals, 0, bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355_OK;
}

// Slice bounds of the cleared red map (mi355_red_stream_batch, clear != 0), max_batch frames: made when first needed.
int need_red_bounds(mi355_core *c) {
    if (c->red_bounds || c->n == 0) return MI355_OK;
    return dev_alloc(c, &c->red_bounds, (size_t)c->cfg.max_batch * red_bounds_per_frame(c->n));
}

// The second set of logs and the side stream of the pipelined mode, made when it is first used (or by mi355_prepare).
int setup_pipeline(mi355_core *c) {
    if (c->side || !c->pipeline_ok) return MI355_OK;
    // Pipelined batches: the pack kernel on 4 workgroups per CU (16 waves: half of them walk a second tile) instead of
    // one tile per wave (6 per CU).  It is bound by the memory system and does not need its occupancy (profiles/README.md,
    // round 1), while the expansion of the batch before, which shares the chip with it, lives on the wave slots and
    // registers that are left: 0.503-0.507 -> 0.487-0.497 ms per batch on the faster boxes, +-1 % on the slower ones
    // (profiles/archive/r04p, r04q, r04v).  run_batch sizes the grid from cu_count.
    const size_t T = (size_t)c->cfg.max_batch, W = c->ntiles;
    mi355_core::LogSet &s0 = c->set[0], &s1 = c->set[1];
    s0.rec = c->rec; s0.codes = c->codes; s0.meta = c->meta; s0.groff = c->groff; s0.totals = c->totals;
    bool ok = true;
    ok = ok && hipMalloc((void **)&s1.rec, T * W * 1024) == hipSuccess;
    ok = ok && hipMalloc((void **)&s1.codes, code_chunks(T) * W * 1024) == hipSuccess;
    ok = ok && hipMalloc((void **)&s1.meta, T * W * 16) == hipSuccess;
    ok = ok && hipMalloc((void **)&s1.groff, T * expand_groups(c->ntiles) * 16) == hipSuccess;
    ok = ok && hipMalloc((void **)&s1.totals, (2 * T + 2) * sizeof(uint32_t)) == hipSuccess;
    // (through the core's stream, and waited for -- clear_totals)
    ok = ok && hipMemsetAsync(s1.totals, 0, (2 * T + 2) * sizeof(uint32_t), c->stream) == hipSuccess &&   // tag 0 = never written; the ticket
         hipStreamSynchronize(c->stream) == hipSuccess;
    ok = ok && make_stream(c, &c->side) == hipSuccess;
    ok = ok && make_stream(c, &c->main2) == hipSuccess;
    for (int i = 0; i < mi355_core::kSets && ok; i++) {
        // device-scope release: these events only order kernels of this device against each other.  An event's default
        // is a SYSTEM-scope fence when it is recorded (caches written back and invalidated for the host's benefit),
        // which every batch paid twice on the core's stream between two pack kernels
        const unsigned flags = hipEventDisableTiming | hipEventReleaseToDevice;
        ok = hipEventCreateWithFlags(&c->set[i].packed, flags) == hipSuccess &&
             hipEventCreateWithFlags(&c->set[i].expanded, flags) == hipSuccess &&
             hipEventCreateWithFlags(&c->packed2[i], flags) == hipSuccess &&
             hipEventCreateWithFlags(&c->fork[i], flags) == hipSuccess;
    }
    if (!ok) {   // not an error: the batches then run one after the other, as with a caller's stream
        (void)hipGetLastError();
        void *ptrs[] = {s1.rec, s1.codes, s1.meta, s1.groff, s1.totals};
        for (void *p : ptrs) if (p) (void)hipFree(p);
        s1.rec = nullptr; s1.meta = nullptr; s1.codes = s1.groff = s1.totals = nullptr;
        if (c->side) { (void)hipStreamDestroy(c->side); c->side = nullptr; }
        if (c->main2) { (void)hipStreamDestroy(c->main2); c->main2 = nullptr; }
        // ... and what a later attempt (MI355_OPT_PIPELINE 1 switches the mode on again) would otherwise overwrite
        for (int i = 0; i < mi355_core::kSets; i++) {
            hipEvent_t *evs[] = {&c->set[i].packed, &c->set[i].expanded, &c->packed2[i], &c->fork[i]};
            for (hipEvent_t *e : evs) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
        }
        c->pipeline_ok = false;
        return MI355_OK;
    }
    c->workspace += T * W * 1024 + code_chunks(T) * W * 1024 + T * W * 16 + T * expand_groups(c->ntiles) * 16 + (2 * T + 2) * 4;
    return MI355_OK;
}

// Outputs of mi355_diff_stream_cwire_batch: compact records instead of (d_xs, d_diff)
struct CwireOut {
    uint64_t *frame_pos;
    uint8_t *cwire;
    uint64_t capacity;   // bytes
};

// What a batch asks of run_batch beyond its operands; the defaults are mi355_exec's: one stream against the core's state, the
// arrays out, everything on the core's stream.
struct BatchMode {
    // d_cur[i] against d_prev[i] (mi355_diff_pairs_batch); otherwise stream mode: frame 0 against the core's state, which takes
    // the last frame, and frame t against frame t - 1
    bool pair = false;
    // (pair mode) d_prev are the caller's states, one per batch index, and take the fed-back state of their frame
    // (mi355_diff_multi_*); the operands do not overlap (the entry points refuse that).
    bool feedback = false;
    // > 0 (stream mode, feedback): nframes / seg streams of seg frames each, batch index s * seg + t; d_prev are the caller's
    // states, one per STREAM (mi355_diff_multi_stream_*).  A tile of a state is read and written by the launches of one stream
    // only, exactly as with feedback pairs (the cut depends on the frame size alone), so the two forms share the fb_states
    // bookkeeping and may alternate on the same states.
    int seg = 0;
    // (stream mode, no feedback) d_prev is ONE frame, the predecessor of frame 0; frame t is compared with frame t - 1
    // (mi355_diff_consecutive_batch).  The core's state takes no part.  d_prev may be the core's state or a caller's states: like
    // a pair batch's operand it is read tile by tile by the launch that packs the tile, on the stream that wrote that tile.
    bool consecutive = false;
    // != nullptr: the expander writes the sender's byte stream (capacity in bytes) instead of d_xs / d_diff
    void *d_wire = nullptr;
    // != nullptr: the log is expanded into compact records (launch_expand_cwire) instead
    const CwireOut *cw = nullptr;
    // a public batch entry point on the core's OWN stream -- the index and the expansion run on the side stream beside the next
    // batch's pack kernel (which needs only the state, carried on the core's stream, and a free set of logs); completion is what
    // mi355_synchronize / any other entry point waits for (use_device joins).  With a caller's stream (mi355_set_stream)
    // everything stays on that stream, in order: a caller who enqueues its own consumers there must find the batch complete.
    bool pipelined = false;
};

CwireDirectArgs cwire_args(mi355_core *c, const CwireOut *cw, const uint32_t *d_offsets, uint32_t ntiles) {
    CwireDirectArgs x{};
    x.x.offsets = d_offsets;
    x.x.ntiles = ntiles;
    x.items = c->cw_items;
    x.esc = c->cw_esc;
    x.frame_pos = cw->frame_pos;
    x.cwire = cw->cwire;
    x.capacity = cw->capacity;
    return x;
}

int run_batch(mi355_core *c, const BatchMode &m, const void *d_cur, const void *d_prev, size_t stride,
              int nframes, void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0 || nframes > c->cfg.max_batch)
        return fail(MI355_ERR_INVALID, "nframes outside [0, max_batch]");
    if (!d_offsets) return fail(MI355_ERR_INVALID, "null d_offsets");
    if (nframes > 0 && c->n > 0 && (!d_cur || ((m.pair || m.consecutive) && !d_prev)))
        return fail(MI355_ERR_INVALID, "null frame pointer");
    if (nframes > 0 && stride < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if (capacity > 0 && !m.d_wire && !m.cw && (!d_xs || !d_diff)) return fail(MI355_ERR_INVALID, "null output pointer");
    bool pipelined = m.pipelined && c->stream == c->own_stream && c->pipeline_ok && nframes > 0 && c->n > 0;
    const bool own = pipelined;   // an own-stream batch (its total is recorded for the next decisions)
    if (c->filter_since_batch) pipelined = false;   // a filter / batch chain: one kernel after the other (use_device_filter)
    c->filter_since_batch = false;
    if (pipelined) {
        // the parts of the last batch: a tick on the states of the tick before may queue up behind them unseen (every tile
        // stays on its stream); any other tick must not write what a part elsewhere still reads, and no other batch may
        // read what a tick's part elsewhere still writes
        const bool same_states = m.feedback && c->fb_states == d_prev && c->fb_stride == stride;
        if (int rc = use_device(c, false, !same_states && (m.feedback || c->fb_states))) return rc;
        if (int rc = setup_pipeline(c)) return rc;
        pipelined = c->pipeline_ok;
    }
    if (pipelined && c->h_tot) {
        // the latest batch total that has arrived: dense input -> this batch runs after the expansion of the one before
        const uint64_t note = __atomic_load_n(c->h_tot, __ATOMIC_RELAXED);   // one 64-bit word: never torn
        if (note >> 32) c->dense = (note & 0xffffffffull) * 100u > (uint64_t)mi355_core::kDensePct * (note >> 32) * c->n;
        if (c->dense) pipelined = false;   // (no total has arrived yet: what the last one said still holds)
    }
    if (!pipelined)
        if (int rc = use_device(c)) return rc;
    c->fb_states = nullptr;   // (whatever was pending has been waited for above, or is these very states)
    if (nframes == 0 || c->n == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint32_t) * ((size_t)nframes + 1), c->stream));
        if (m.d_wire) {   // empty frames still have their headers {n = 0}
            const size_t head = 4 * (size_t)nframes < capacity ? 4 * (size_t)nframes : capacity & ~(size_t)3;
            if (head) HIP_TRY(hipMemsetAsync(m.d_wire, 0, head, c->stream));
        }
        if (m.cw) HIP_TRY(launch_expand_cwire(cwire_args(c, m.cw, (const uint32_t *)d_offsets, 0u), nframes, c->stream));
        return MI355_OK;
    }
    hipEvent_t *tev = nullptr;
    if (c->timing) {
        if (int rc = harvest_timing(c, mi355_core::kEvRing - 1)) return rc;
        tev = c->ev[(c->ev_head + c->ev_count) % mi355_core::kEvRing];
    }
    // the set of logs this batch writes; a pipelined batch may only start once the expansion that last read the
    // set (two batches ago) is done
    mi355_core::LogSet one;
    one.rec = c->rec; one.codes = c->codes; one.meta = c->meta; one.groff = c->groff; one.totals = c->totals;
    mi355_core::LogSet &ls = pipelined ? c->set[c->flip] : one;
    hipStream_t tail = pipelined ? c->side : c->stream;   // where the index and the expansion run
    if (pipelined && ls.in_use) HIP_TRY(hipStreamWaitEvent(c->stream, ls.expanded, 0));
    if (tev) HIP_TRY(hipEventRecord(tev[0], c->stream));
    PackArgs a{};
    a.cur = (const uint8_t *)d_cur;
    a.prev = m.seg ? nullptr : (const uint8_t *)d_prev;
    a.state = c->state;
    a.seg = m.seg;
    if (m.seg) a.states = (uint8_t *)const_cast<void *>(d_prev);
    a.stride = stride;
    a.n = c->n;
    a.nframes = nframes;
    a.thr = c->cfg.threshold;
    a.ntiles = c->ntiles;
    a.tile_begin = 0;
    a.tile_end = c->ntiles;
    a.rec = ls.rec;
    a.codes = ls.codes;
    a.codes_bytes = (uint32_t)(code_chunks((size_t)c->cfg.max_batch) * c->ntiles * 1024u);
    a.meta = ls.meta;
    a.rec_bytes = (uint32_t)((size_t)c->cfg.max_batch * c->ntiles * 1024u);
    a.meta_bytes = (uint32_t)((size_t)c->cfg.max_batch * c->ntiles * 16u);
    // the vector path of the pack kernel: 16-byte aligned operands, and a group of four frames within reach of one
    // buffer descriptor's 32-bit offsets (diff_pack.hip, Group::load_desc); d_prev: the pairs' second operand, or the one
    // predecessor of consecutive frames (nullptr otherwise)
    const bool aligned = (((uintptr_t)d_cur | (uintptr_t)d_prev | stride) & 15u) == 0 && 3 * (uint64_t)stride + c->n < (1ull << 32);
    // Pair mode: do the two operands share a frame (or part of one), i.e. does prev + j * stride come within a frame of
    // cur + i * stride for some i, j < T?  Pairs of consecutive frames do (cur of one pair is prev of the next: the second
    // read hits in the caches); the pairs of a round-robin shard do not, and are read with non-temporal loads like the
    // frames of a stream (diff_pack.hip, Group::load_desc).
    bool pair_once = false;
    if (m.pair) {
        const int64_t d = (int64_t)((intptr_t)d_prev - (intptr_t)d_cur), st = (int64_t)stride, T = nframes;
        bool shared = false;
        const int64_t k0 = d / st;
        for (int64_t k = k0 - 1; k <= k0 + 1; k++)
            if (k > -T && k < T && (d - k * st < 0 ? k * st - d : d - k * st) < (int64_t)c->n) shared = true;
        pair_once = !shared;
    }
    const uint32_t k1_blocks = 4u * c->cu_count;   // the pipelined pack grid (setup_pipeline; 0 = one tile per wave)
    const bool split = pipelined && c->main2 && c->ntiles >= 64;
    if (split) {
        // tiles [0, cut) on the core's stream, the rest on a stream of its own (which also has to see the log set free
        // and everything the core's stream holds so far: a filter that is still writing the frames this batch reads,
        // the upload of the state); each part takes its share of the pipelined grid
        const uint32_t cut = (c->ntiles / 2) & ~3u;
        uint32_t blocks0 = 0, blocks1 = 0;
        if (k1_blocks) {
            blocks0 = (uint32_t)((uint64_t)k1_blocks * cut / c->ntiles);
            if (blocks0 == 0) blocks0 = 1;
            blocks1 = k1_blocks > blocks0 ? k1_blocks - blocks0 : 1u;
        }
        HIP_TRY(hipEventRecord(c->fork[c->flip], c->stream));
        PackArgs a0 = a, a1 = a;
        a0.tile_end = cut;
        a1.tile_begin = cut;
        HIP_TRY(launch_diff_pack(a0, m.pair, aligned, pair_once, blocks0, c->stream, m.feedback, m.consecutive));
        HIP_TRY(hipStreamWaitEvent(c->main2, c->fork[c->flip], 0));
        if (ls.in_use) HIP_TRY(hipStreamWaitEvent(c->main2, ls.expanded, 0));
        HIP_TRY(launch_diff_pack(a1, m.pair, aligned, pair_once, blocks1, c->main2, m.feedback, m.consecutive));
        HIP_TRY(hipEventRecord(c->packed2[c->flip], c->main2));
        HIP_TRY(hipStreamWaitEvent(tail, c->packed2[c->flip], 0));
        if (tev) HIP_TRY(hipEventRecord(tev[5], c->main2));   // the pack "kernel" of a split batch ends when BOTH parts have
        c->parts_pending = c->flip;
        if (m.feedback) { c->fb_states = d_prev; c->fb_stride = stride; }
    } else {
        HIP_TRY(launch_diff_pack(a, m.pair, aligned, pair_once, pipelined ? k1_blocks : 0u, c->stream, m.feedback, m.consecutive));
    }
    if (tev) {
        HIP_TRY(hipEventRecord(tev[1], c->stream));
        c->ev_split[(c->ev_head + c->ev_count) % mi355_core::kEvRing] = split;
    }
    // The index kernel is short (12 us alone) and gates the expansion; it runs in front of it on the side stream (on the
    // core's stream, between two pack kernels, was measured: worse, profiles/archive/r04a).
    if (pipelined) {
        HIP_TRY(hipEventRecord(ls.packed, c->stream));
        HIP_TRY(hipStreamWaitEvent(tail, ls.packed, 0));
    }
    if (tev) HIP_TRY(hipEventRecord(tev[2], tail));
    if (next_scan_epoch(c->scan_epoch)) {
        // the launch tags have wrapped (2^33 launches): every total any launch of this core has written goes, behind a
        // synchronisation, before a tag is used a second time -- a slot can then never hold a stale word with a current tag
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->side) HIP_TRY(hipStreamSynchronize(c->side));
        if (c->main2) HIP_TRY(hipStreamSynchronize(c->main2));
        if (int rc = clear_totals(c)) return rc;
    }
    // (an own-stream batch leaves its total in pinned memory for the next calls' decisions -- stored by the index kernel
    // itself: a copy + an event behind every batch cost config 3's chain 4 %, the event's system-scope fence included)
    uint64_t *const note = own && c->h_tot && c->pipeline_ok ? c->h_tot : nullptr;
    HIP_TRY(launch_scan(ls.meta, ls.groff, (uint64_t *)ls.totals, c->ntiles, nframes, (uint32_t *)d_offsets,
                        ls.totals + 2 * (size_t)c->cfg.max_batch, c->scan_epoch, note, tail));
    if (tev) HIP_TRY(hipEventRecord(tev[3], tail));
    ExpandArgs g{};
    g.rec = ls.rec;
    g.codes = ls.codes;
    g.meta = ls.meta;
    g.roff = ls.groff;
    g.offsets = (const uint32_t *)d_offsets;
    g.ntiles = c->ntiles;
    g.codes_bytes = a.codes_bytes;
    g.rec_bytes = a.rec_bytes;
    g.out_xs = (int32_t *)d_xs;
    g.out_diff = (uint8_t *)d_diff;
    g.wire = (uint8_t *)m.d_wire;
    g.capacity = capacity;
    if (m.cw) {   // the same log into compact records (the kernels read only its fields and the offsets)
        CwireDirectArgs x = cwire_args(c, m.cw, g.offsets, c->ntiles);
        x.x = g;
        HIP_TRY(launch_expand_cwire(x, nframes, tail));
    } else {
        HIP_TRY(launch_expand(g, nframes, tail));
    }
    if (tev) {
        HIP_TRY(hipEventRecord(tev[4], tail));
        c->ev_count += 1;
    }
    if (pipelined) {
        HIP_TRY(hipEventRecord(ls.expanded, tail));
        ls.in_use = true;
        c->side_done = ls.expanded;
        c->flip ^= 1;
    }
    return MI355_OK;
}

}  // namespace

extern "C" {

const char *mi355_last_error(void) { return g_err.c_str(); }

int mi355_abi_version(void) { return MI355_ABI_VERSION; }

int mi355_create(const mi355_config *cfg, mi355_core **out) {
    if (!cfg || !out) return fail(MI355_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->width < 0 || cfg->height < 0) return fail(MI355_ERR_INVALID, "negative frame size");
    // |df| of two bytes is at most 255: a threshold of 255 flags nothing; larger or negative values are refused
    if (cfg->threshold < 0 || cfg->threshold > 255) return fail(MI355_ERR_INVALID, "threshold outside 0..255");
    if (cfg->max_batch < 1) return fail(MI355_ERR_INVALID, "max_batch < 1");
    if (cfg->visualizer < 0 || cfg->visualizer > 5) return fail(MI355_ERR_INVALID, "unknown visualizer");
    if (cfg->flags & ~MI355_FLAG_OWN_QUEUES) return fail(MI355_ERR_INVALID, "flags: unknown bit (MI355_FLAG_OWN_QUEUES is the only flag of this version of the library)");
    const uint64_t n64 = 3ull * (uint64_t)cfg->width * (uint64_t)cfg->height;
    if (n64 >= (1ull << 31)) return fail(MI355_ERR_INVALID, "frame larger than 2 GiB");
    // byte indices are int32 and batch offsets uint32 (the reference's h_xs / h_pos types)
    // (whole tiles: the record log, max_batch * ceil(N / 1024) KiB, is addressed with 32-bit byte offsets)
    // ... and so is the code log, code_chunks(max_batch) * ceil(N / 1024) KiB, which is the larger one for max_batch = 1
    // (two chunks per tile: a frame's codes never straddle a chunk)
    {
        const uint64_t tiles = (n64 + kTileBytes - 1) / kTileBytes, mb = (uint64_t)cfg->max_batch;
        const uint64_t chunks = mb > code_chunks((size_t)mb) ? mb : (uint64_t)code_chunks((size_t)mb);
        if (tiles * kTileBytes * chunks >= (1ull << 32))
            return fail(MI355_ERR_INVALID, "max_batch * frame bytes must stay below 2^32");
    }

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(MI355_ERR_HIP, "no HIP device available (libmi355diff has no CPU fallback)", e);
    mi355_core *c = new (std::nothrow) mi355_core;
    if (!c) return fail(MI355_ERR_INVALID, "out of host memory");
    c->cfg = *cfg;
    // the ONE environment variable the library reads (include/mi355diff.h, "Options")
    if (const char *v = getenv("MI355_PIPELINE")) c->pipeline_ok = v[0] != '0';
    if (cfg->device >= 0) c->device = cfg->device;
    else if ((e = hipGetDevice(&c->device)) != hipSuccess) { delete c; return fail(MI355_ERR_HIP, "hipGetDevice", e); }
    if (c->device >= ndev) { delete c; return fail(MI355_ERR_INVALID, "device ordinal out of range"); }

    c->n = (uint32_t)n64;
    c->ntiles = (c->n + kTileBytes - 1) / kTileBytes;
    {
        hipDeviceProp_t prop{};
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) c->cu_count = (uint32_t)prop.multiProcessorCount;
    }
    const size_t T = (size_t)cfg->max_batch, W = c->ntiles, N = c->n;

    int rc = use_device(c);
    if (!rc) { e = make_stream(c, &c->own_stream); if (e != hipSuccess) rc = fail(MI355_ERR_HIP, "hipStreamCreate", e); }
    c->stream = c->own_stream;
    for (int i = 0; i < mi355_core::kEvRing * mi355_core::kEvPer && !rc; i++) { e = hipEventCreateWithFlags(&c->ev[i / mi355_core::kEvPer][i % mi355_core::kEvPer], hipEventDisableSystemFence); if (e != hipSuccess) rc = fail(MI355_ERR_HIP, "hipEventCreate", e); }   // timing events: no system-scope fence (hip_runtime_api.h: "can improve the accuracy of timing measurements by avoiding the cost of cache writeback and invalidation")
    if (!rc && (e = init_gray_table()) != hipSuccess) rc = fail(MI355_ERR_HIP, "init_gray_table", e);
    if (!rc) rc = dev_alloc(c, &c->state, N + 16);
    if (!rc) rc = dev_alloc(c, &c->in, N + 16);
    if (!rc) rc = dev_alloc(c, &c->aux, N + 16);
    if (!rc) rc = dev_alloc(c, &c->vis, N + 16);
    if (!rc) rc = dev_alloc(c, &c->rec, T * W * 64);
    if (!rc) rc = dev_alloc(c, &c->codes, code_chunks(T) * W * 256);
    if (!rc) rc = dev_alloc(c, &c->meta, T * W);
    if (!rc) rc = dev_alloc(c, &c->groff, T * expand_groups(c->ntiles) * 4);   // one prefix per range of 16 tiles
    if (!rc) rc = dev_alloc(c, &c->totals, 2 * T + 2);   // T x {total, epoch} + the scan kernel's ticket counter
    if (!rc) { e = hipMemsetAsync(c->totals, 0, (2 * T + 2) * sizeof(uint32_t), c->own_stream); if (e != hipSuccess) rc = fail(MI355_ERR_HIP, "hipMemset", e); }
    if (!rc) rc = dev_alloc(c, &c->offsets, T + 1);
    if (!rc) rc = dev_alloc(c, &c->cw_cnt, (size_t)kCwireSlots);
    if (!rc) rc = dev_alloc(c, &c->cw_items, T * cwire_items_per_frame(c->ntiles));
    if (!rc) rc = dev_alloc(c, &c->cw_esc, T);
    if (!rc) rc = dev_alloc(c, &c->cwa_ftab, T);
    if (!rc) rc = dev_alloc(c, &c->cwa_chunk, T * cwa_chunks(c->n));
    if (!rc) rc = dev_alloc(c, &c->cwa_dir, T * cwa_tiles(c->n));
    if (!rc) rc = dev_alloc(c, &c->cwb_hist, T * kCwbWords);
    if (!rc) rc = dev_alloc(c, &c->cws_blk, T * cws_blocks(c->n));
    if (!rc) rc = dev_alloc(c, &c->cws_base, T * cws_blocks(c->n));
    if (!rc) rc = dev_alloc(c, &c->cwr_rtab, T);
    if (!rc) rc = dev_alloc(c, &c->cwr_chunk, T * cwr_chunks_max(c->n));
    if (!rc) rc = dev_alloc(c, &c->one_xs, N + 4);
    if (!rc) rc = dev_alloc(c, &c->one_diff, N + 16);
    if (!rc) rc = dev_alloc(c, &c->hist, 256 * T);
    if (!rc) rc = dev_alloc(c, &c->thr, T);
    if (!rc) rc = dev_alloc(c, &c->k9, 9);
    if (!rc) rc = dev_alloc(c, &c->lut, 768 * 3);
    if (!rc) { e = hipHostMalloc((void **)&c->h_count, 2 * sizeof(uint32_t), hipHostMallocDefault); if (e != hipSuccess) rc = fail(MI355_ERR_HIP, "hipHostMalloc", e); }
    if (!rc) { e = hipHostMalloc((void **)&c->h_tot, sizeof(uint64_t), hipHostMallocDefault); if (e != hipSuccess) rc = fail(MI355_ERR_HIP, "hipHostMalloc", e); else *c->h_tot = 0; }
    if (!rc) { e = hipMemsetAsync(c->state, 0, N + 16, c->own_stream); if (e != hipSuccess) rc = fail(MI355_ERR_HIP, "hipMemset", e); }
    // (the clears above went through the core's own stream -- clear_totals -- and are complete before the core is handed out)
    if (!rc) { e = hipStreamSynchronize(c->own_stream); if (e != hipSuccess) rc = fail(MI355_ERR_HIP, "hipStreamSynchronize", e); }
    if (!rc) {
        uint8_t lut[768 * 3] = {0};
        build_heat_lut(lut);
        e = hipMemcpy(c->lut, lut, sizeof lut, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(MI355_ERR_HIP, "hipMemcpy(lut)", e);
    }
    // what a per-frame server's first exec() would otherwise allocate (kernels.cu:493-498: visualiser 5)
    if (!rc && cfg->visualizer == MI355_VIS_BINARIZE) rc = need_gray1(c);
    if (rc) { mi355_destroy(c); return rc; }
    *out = c;
    return MI355_OK;
}

void mi355_destroy(mi355_core *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->nslots) (void)mi355_pipe_close(c);
    if (c->side) (void)hipStreamSynchronize(c->side);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    {
        mi355_core::LogSet &s1 = c->set[1];
        void *more[] = {s1.rec, s1.codes, s1.meta, s1.groff, s1.totals};
        for (void *p : more) if (p) (void)hipFree(p);
        for (auto &ls : c->set) {
            if (ls.packed) (void)hipEventDestroy(ls.packed);
            if (ls.expanded) (void)hipEventDestroy(ls.expanded);
        }
        if (c->side) (void)hipStreamDestroy(c->side);
        if (c->main2) { (void)hipStreamSynchronize(c->main2); (void)hipStreamDestroy(c->main2); }
        for (auto &e : c->packed2) if (e) (void)hipEventDestroy(e);
        for (auto &e : c->fork) if (e) (void)hipEventDestroy(e);
        if (c->h_tot) (void)hipHostFree(c->h_tot);
    }
    void *ptrs[] = {c->state, c->in, c->aux, c->vis, c->rec, c->codes, c->meta, c->groff, c->totals, c->offsets, c->one_xs, c->one_diff, c->hist, c->thr, c->k9,
                    c->lut, c->glyphs, c->kxk, c->gray1, c->red_bounds, c->cw_cnt, c->cw_items, c->cw_esc,
                    c->cwa_ftab, c->cwa_chunk, c->cwa_dir, c->cwb_hist, c->cws_blk, c->cws_base, c->cwr_rtab, c->cwr_chunk, c->cw_rec, c->cw_rec_pos, c->dsp_bits};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (c->h_count) (void)hipHostFree(c->h_count);
    if (c->h_rec) (void)hipHostFree(c->h_rec);
    for (auto &slot : c->ev) for (auto &ev : slot) if (ev) (void)hipEventDestroy(ev);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

static int warm_exec(mi355_core *c);   // below, beside mi355_exec
static int need_exec_cwire(mi355_core *c);   // below, beside mi355_exec_cwire
static int need_despeckle(mi355_core *c);    // below, beside mi355_cwire_despeckle_cwire_batch

int mi355_prepare(mi355_core *c, unsigned what) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (what & ~(MI355_PREPARE_ALL | MI355_PREPARE_EXEC_CWIRE | MI355_PREPARE_DESPECKLE)) return fail(MI355_ERR_INVALID, "mi355_prepare: unknown bit in `what`");
    if (int rc = use_device(c)) return rc;
    if ((what & MI355_PREPARE_BATCHES) && c->n > 0) {
        if (int rc = setup_pipeline(c)) return rc;   // (a core that cannot have its second set stays sequential: not an error)
    }
    if (what & MI355_PREPARE_GRAY_CHAIN)
        if (int rc = need_gray1(c)) return rc;
    if (what & MI355_PREPARE_RED_CLEAR)
        if (int rc = need_red_bounds(c)) return rc;
    if ((what & MI355_PREPARE_CONV_KXK) && !c->kxk)
        if (int rc = dev_alloc(c, &c->kxk, 81)) return rc;
    if ((what & MI355_PREPARE_EXEC) && c->n > 0 && c->nslots == 0)
        if (int rc = warm_exec(c)) return rc;
    if (what & MI355_PREPARE_EXEC_CWIRE)
        if (int rc = need_exec_cwire(c)) return rc;
    if (what & MI355_PREPARE_DESPECKLE)
        if (int rc = need_despeckle(c)) return rc;
    HIP_TRY(hipDeviceSynchronize());   // the memsets of the new buffers
    return MI355_OK;
}

size_t mi355_frame_bytes(const mi355_core *c) { return c ? c->n : 0; }
size_t mi355_workspace_bytes(const mi355_core *c) { return c ? c->workspace : 0; }

int mi355_set_stream(mi355_core *c, void *hip_stream) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    if (int rc = harvest_timing(c)) return rc;
    // every batch shares one workspace (log, meta, scans, state): work queued on the old stream must be done
    // before anything is enqueued on the new one
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t)hip_stream;  // NULL is the (legacy) default stream, a valid choice
    return MI355_OK;
}

int mi355_use_own_stream(mi355_core *c) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    if (int rc = harvest_timing(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));   // see mi355_set_stream
    c->stream = c->own_stream;
    return MI355_OK;
}

int mi355_synchronize(mi355_core *c) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355_OK;
}

// Options: the pipelined mode of the own-stream batches and two seams for tests, never a result.  Changing one first
// completes what is queued.
int mi355_set_option(mi355_core *c, int option, int value) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    switch (option) {
        case MI355_OPT_PIPELINE:
            if (value != 0 && value != 1) return fail(MI355_ERR_INVALID, "MI355_OPT_PIPELINE: 0 or 1");
            // (a core whose second log set could not be allocated stays sequential: setup_pipeline says so by itself)
            c->pipeline_ok = value == 1;
            return MI355_OK;
        case MI355_OPT_MEDIAN_ROWS:   // tests: the median filter's band length, instead of the one chosen per launch
            if (value < 0 || value > 60 || value % 5) return fail(MI355_ERR_INVALID, "MI355_OPT_MEDIAN_ROWS: 0 (default) or 5, 10, .. 60");
            c->median_rows = value;
            return MI355_OK;
        case MI355_OPT_SCAN_EPOCH_LEFT:   // tests: the index kernel's launch tag this many launches before its wrap
            if (value < 1 || value > (1 << 30)) return fail(MI355_ERR_INVALID, "MI355_OPT_SCAN_EPOCH_LEFT: 1..2^30");
            if (c->side) HIP_TRY(hipStreamSynchronize(c->side));
            if (c->main2) HIP_TRY(hipStreamSynchronize(c->main2));
            // every total goes with the jump: a tag set BACK (the option used twice before a wrap) would otherwise meet slots that
            // still carry that very tag from an earlier launch, and the index kernel would take their stale totals for this launch's
            // (found by tests/soak_chain.py in round 6: offsets of garbage, a red-map kernel walking 2^32 entries)
            if (int rc = clear_totals(c)) return rc;
            c->scan_epoch = kEpochWrap - 1 - (uint64_t)value;
            return MI355_OK;
        default: return fail(MI355_ERR_INVALID, "unknown option");
    }
}

int mi355_get_option(mi355_core *c, int option, int *value) {
    if (!c || !value) return fail(MI355_ERR_INVALID, "null argument");
    switch (option) {
        case MI355_OPT_PIPELINE: *value = c->pipeline_ok ? 1 : 0; return MI355_OK;
        case MI355_OPT_MEDIAN_ROWS: *value = c->median_rows; return MI355_OK;
        case MI355_OPT_SCAN_EPOCH_LEFT: {
            const uint64_t left = kEpochWrap - 1 - c->scan_epoch;
            *value = left > (1ull << 30) ? (1 << 30) : (int)left;
            return MI355_OK;
        }
        default: return fail(MI355_ERR_INVALID, "unknown option");
    }
}

int mi355_set_state(mi355_core *c, const uint8_t *host_frame) {
    if (!c || !host_frame) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipMemcpyAsync(c->state, host_frame, c->n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355_OK;
}

int mi355_get_state(mi355_core *c, uint8_t *host_frame) {
    if (!c || !host_frame) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipMemcpyAsync(host_frame, c->state, c->n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355_OK;
}

void *mi355_state_device_ptr(mi355_core *c) { return c ? c->state : nullptr; }

int mi355_set_conv_kernel(mi355_core *c, const float *k9) {
    if (!c || !k9) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipMemcpyAsync(c->k9, k9, 9 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_k9 = true;
    uint32_t b[9];
    memcpy(b, k9, sizeof b);
    c->k9_sym = b[0] == b[2] && b[0] == b[6] && b[0] == b[8] && b[1] == b[3] && b[1] == b[5] && b[1] == b[7];
    return MI355_OK;
}

int mi355_set_glyphs(mi355_core *c, const uint8_t *chars_px, int nglyphs, int glyph_h, int glyph_w,
                     const char *charset) {
    if (!c || !chars_px || !charset) return fail(MI355_ERR_INVALID, "null argument");
    if (nglyphs < 0 || glyph_h < 0 || glyph_w < 0 || (int)strlen(charset) != nglyphs)
        return fail(MI355_ERR_INVALID, "glyph atlas / charset mismatch");
    if (int rc = use_device(c)) return rc;
    const size_t bytes = (size_t)nglyphs * 3 * glyph_h * glyph_w;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->glyphs) { (void)hipFree(c->glyphs); c->glyphs = nullptr; }
    HIP_TRY(hipMalloc((void **)&c->glyphs, bytes ? bytes : 16));
    HIP_TRY(hipMemcpy(c->glyphs, chars_px, bytes, hipMemcpyHostToDevice));
    c->nglyphs = nglyphs; c->glyph_h = glyph_h; c->glyph_w = glyph_w;
    c->charset = charset;
    return MI355_OK;
}

int mi355_diff_stream_batch(mi355_core *c, const void *d_frames, size_t stride_bytes, int nframes,
                            void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    BatchMode m;
    m.pipelined = true;
    return run_batch(c, m, d_frames, nullptr, stride_bytes, nframes, d_offsets, d_xs, d_diff, capacity);
}

int mi355_diff_pairs_batch(mi355_core *c, const void *d_cur, const void *d_prev, size_t stride_bytes,
                           int nframes, void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    BatchMode m;
    m.pair = m.pipelined = true;
    return run_batch(c, m, d_cur, d_prev, stride_bytes, nframes, d_offsets, d_xs, d_diff, capacity);
}

int mi355_diff_stream_wire_batch(mi355_core *c, const void *d_frames, size_t stride_bytes, int nframes,
                                 void *d_offsets, void *d_wire, size_t capacity_bytes) {
    if (!d_wire) return fail(MI355_ERR_INVALID, "null d_wire");
    BatchMode m;
    m.d_wire = d_wire;
    m.pipelined = true;
    return run_batch(c, m, d_frames, nullptr, stride_bytes, nframes, d_offsets, nullptr, nullptr, capacity_bytes);
}

int mi355_diff_stream_cwire_batch(mi355_core *c, const void *d_frames, size_t stride_bytes, int nframes,
                                  void *d_offsets, void *d_frame_pos, void *d_cwire, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0 || nframes > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nframes outside [0, max_batch]");
    if (!d_offsets || !d_frame_pos) return fail(MI355_ERR_INVALID, "null d_offsets / d_frame_pos");
    if (capacity_bytes > 0 && !d_cwire) return fail(MI355_ERR_INVALID, "null d_cwire");
    if (((uintptr_t)d_cwire & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_frame_pos & 7u))
        return fail(MI355_ERR_INVALID, "d_cwire and d_offsets must be 4-byte aligned, d_frame_pos 8-byte aligned");
    const CwireOut cw{(uint64_t *)d_frame_pos, (uint8_t *)d_cwire, (uint64_t)capacity_bytes};
    BatchMode m;
    m.cw = &cw;
    m.pipelined = true;
    return run_batch(c, m, d_frames, nullptr, stride_bytes, nframes, d_offsets, nullptr, nullptr, 0);
}

// ---- the caller's regions of device memory, for the overlap tests of the entry points below ---------------------------------
namespace {
// [p, p + bytes) and its name in an error text
struct Region {
    const void *p;
    uint64_t bytes;
    const char *what;
};
// Plain intervals: an empty region that lies strictly inside another one overlaps it, {nullptr, 0} overlaps nothing (p = 0 and
// bytes = 0 never satisfy the second comparison).  The calls that let an empty region lie anywhere hand theirs through nowhere().
bool overlap(const Region &a, const Region &b) {
    const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
    return pa < pb + (uintptr_t)b.bytes && pb < pa + (uintptr_t)a.bytes;
}
int overlap_fail(const Region &a, const Region &b) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s and %s overlap", a.what, b.what);
    return fail(MI355_ERR_INVALID, msg);
}
Region nowhere(Region r) {
    if (r.bytes == 0) r.p = nullptr;
    return r;
}
// count >= 1 windows of the core's frame bytes, stride apart: from the first byte of the first to the end of the last
Region windows(const mi355_core *c, const void *p, int64_t count, size_t stride, const char *what) {
    return Region{p, (uint64_t)(count - 1) * stride + c->n, what};
}
Region states_region(const mi355_core *c, const void *d_states, size_t stride, int nstreams) {
    return windows(c, d_states, nstreams, stride, "the states");
}
Region out_frames_region(const mi355_core *c, const void *d_out, size_t out_stride, int64_t nframes) {
    return windows(c, d_out, nframes, out_stride, "the output frames");
}
Region input_region(const void *d_in, uint64_t bytes) { return Region{d_in, bytes, "the input stream"}; }
Region offsets_region(const void *d_offsets, int nstreams) { return Region{d_offsets, ((uint64_t)nstreams + 1) * sizeof(uint32_t), "d_offsets"}; }
Region frame_pos_region(const void *d_frame_pos, int nstreams) {
    return Region{d_frame_pos, ((uint64_t)nstreams + 1) * sizeof(uint64_t), "d_frame_pos"};
}
Region tile_mask_region(const mi355_core *c, const void *d_tile_mask, int nstreams) {
    return Region{d_tile_mask, 4 * (uint64_t)nstreams * cwa_mask_words(c->n), "d_tile_mask"};
}
// Refuses an output that overlaps an input, output by output in their order; among_outputs: and one that overlaps a later output
int check_regions(std::initializer_list<Region> in, std::initializer_list<Region> out, bool among_outputs = false) {
    for (const Region *o = out.begin(); o != out.end(); o++) {
        for (const Region &i : in)
            if (overlap(*o, i)) return overlap_fail(*o, i);
        for (const Region *later = o + 1; among_outputs && later != out.end(); later++)
            if (overlap(*o, *later)) return overlap_fail(*o, *later);
    }
    return MI355_OK;
}
}  // namespace

// mi355_diff_multi(_stream)_*: what the six forms refuse alike, before anything is launched (mi355_diff_multi_*: nframes = 1)
static int check_multi_stream(mi355_core *c, const void *d_frames, const void *d_states, size_t stride, int nstreams, int nframes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nframes < 0) return fail(MI355_ERR_INVALID, "negative nstreams / nframes");
    if ((int64_t)nstreams * nframes > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams * nframes above max_batch");
    if (nstreams == 0 || nframes == 0) return MI355_OK;
    if (!d_frames || !d_states) return fail(MI355_ERR_INVALID, "null d_frames / d_states");
    if (stride < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    const Region st = states_region(c, d_states, stride, nstreams);
    const Region fr = windows(c, d_frames, (int64_t)nstreams * nframes, stride, "the frames");
    if (overlap(st, fr)) return overlap_fail(st, fr);
    return MI355_OK;
}

int mi355_diff_consecutive_batch(mi355_core *c, const void *d_first_prev, const void *d_frames, size_t frame_step_bytes, int nframes,
                                 void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    BatchMode m;
    m.consecutive = m.pipelined = true;
    return run_batch(c, m, d_frames, d_first_prev, frame_step_bytes, nframes, d_offsets, d_xs, d_diff, capacity);
}

int mi355_diff_multi_batch(mi355_core *c, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                           void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    if (int rc = check_multi_stream(c, d_frames, d_states, stride_bytes, nstreams, 1)) return rc;
    BatchMode m;
    m.pair = m.feedback = m.pipelined = true;
    return run_batch(c, m, d_frames, d_states, stride_bytes, nstreams, d_offsets, d_xs, d_diff, capacity);
}

int mi355_diff_multi_wire_batch(mi355_core *c, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                                void *d_offsets, void *d_wire, size_t capacity_bytes) {
    if (int rc = check_multi_stream(c, d_frames, d_states, stride_bytes, nstreams, 1)) return rc;
    if (!d_wire) return fail(MI355_ERR_INVALID, "null d_wire");
    BatchMode m;
    m.pair = m.feedback = m.pipelined = true;
    m.d_wire = d_wire;
    return run_batch(c, m, d_frames, d_states, stride_bytes, nstreams, d_offsets, nullptr, nullptr, capacity_bytes);
}

int mi355_diff_multi_cwire_batch(mi355_core *c, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                                 void *d_offsets, void *d_frame_pos, void *d_cwire, size_t capacity_bytes) {
    if (int rc = check_multi_stream(c, d_frames, d_states, stride_bytes, nstreams, 1)) return rc;
    if (!d_offsets || !d_frame_pos) return fail(MI355_ERR_INVALID, "null d_offsets / d_frame_pos");
    if (capacity_bytes > 0 && !d_cwire) return fail(MI355_ERR_INVALID, "null d_cwire");
    if (((uintptr_t)d_cwire & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_frame_pos & 7u))
        return fail(MI355_ERR_INVALID, "d_cwire and d_offsets must be 4-byte aligned, d_frame_pos 8-byte aligned");
    const CwireOut cw{(uint64_t *)d_frame_pos, (uint8_t *)d_cwire, (uint64_t)capacity_bytes};
    BatchMode m;
    m.pair = m.feedback = m.pipelined = true;
    m.cw = &cw;
    return run_batch(c, m, d_frames, d_states, stride_bytes, nstreams, d_offsets, nullptr, nullptr, 0);
}

int mi355_diff_multi_stream_batch(mi355_core *c, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                                  int nframes, void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    if (int rc = check_multi_stream(c, d_frames, d_states, stride_bytes, nstreams, nframes)) return rc;
    BatchMode m;
    m.feedback = m.pipelined = true;
    m.seg = nframes;
    return run_batch(c, m, d_frames, d_states, stride_bytes, nstreams * nframes, d_offsets, d_xs, d_diff, capacity);
}

int mi355_diff_multi_stream_wire_batch(mi355_core *c, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                                       int nframes, void *d_offsets, void *d_wire, size_t capacity_bytes) {
    if (int rc = check_multi_stream(c, d_frames, d_states, stride_bytes, nstreams, nframes)) return rc;
    if (!d_wire) return fail(MI355_ERR_INVALID, "null d_wire");
    BatchMode m;
    m.feedback = m.pipelined = true;
    m.seg = nframes;
    m.d_wire = d_wire;
    return run_batch(c, m, d_frames, d_states, stride_bytes, nstreams * nframes, d_offsets, nullptr, nullptr, capacity_bytes);
}

int mi355_diff_multi_stream_cwire_batch(mi355_core *c, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                                        int nframes, void *d_offsets, void *d_frame_pos, void *d_cwire, size_t capacity_bytes) {
    if (int rc = check_multi_stream(c, d_frames, d_states, stride_bytes, nstreams, nframes)) return rc;
    if (!d_offsets || !d_frame_pos) return fail(MI355_ERR_INVALID, "null d_offsets / d_frame_pos");
    if (capacity_bytes > 0 && !d_cwire) return fail(MI355_ERR_INVALID, "null d_cwire");
    if (((uintptr_t)d_cwire & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_frame_pos & 7u))
        return fail(MI355_ERR_INVALID, "d_cwire and d_offsets must be 4-byte aligned, d_frame_pos 8-byte aligned");
    const CwireOut cw{(uint64_t *)d_frame_pos, (uint8_t *)d_cwire, (uint64_t)capacity_bytes};
    BatchMode m;
    m.feedback = m.pipelined = true;
    m.seg = nframes;
    m.cw = &cw;
    return run_batch(c, m, d_frames, d_states, stride_bytes, nstreams * nframes, d_offsets, nullptr, nullptr, 0);
}

size_t mi355_wire_bytes(int nframes, uint64_t entries) { return 4 * (size_t)nframes + 5 * (size_t)entries; }

int mi355_apply_batch(mi355_core *c, const void *d_offsets, const void *d_xs, const void *d_diff, int nframes,
                      void *d_frames_out, size_t stride_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0) return fail(MI355_ERR_INVALID, "nframes < 0");
    if (nframes == 0 || c->n == 0) return MI355_OK;
    if (!d_offsets || !d_xs || !d_diff) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (d_frames_out && stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if (int rc = use_device(c)) return rc;
    if (!d_frames_out) {
        HIP_TRY(launch_apply_all(c->state, c->n, (const int32_t *)d_xs, (const uint8_t *)d_diff,
                                 (const uint32_t *)d_offsets, nframes, c->stream));
        return MI355_OK;
    }
    for (int t = 0; t < nframes; t++) {
        HIP_TRY(launch_apply(c->state, c->n, d_xs, d_diff, (const uint32_t *)d_offsets, t, 0, c->stream));
        HIP_TRY(hipMemcpyAsync((uint8_t *)d_frames_out + (size_t)t * stride_bytes, c->state, c->n,
                               hipMemcpyDeviceToDevice, c->stream));
    }
    return MI355_OK;
}

int mi355_apply_wire_batch(mi355_core *c, const void *d_wire, const uint32_t *h_counts, int nframes,
                           void *d_frames_out, size_t stride_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0) return fail(MI355_ERR_INVALID, "nframes < 0");
    if (nframes == 0) return MI355_OK;
    if (!d_wire || !h_counts) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (d_frames_out && stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if (int rc = use_device(c)) return rc;
    const uint8_t *p = (const uint8_t *)d_wire;
    for (int t = 0; t < nframes; t++) {
        const uint32_t cnt = h_counts[t];
        if (cnt > c->n) return fail(MI355_ERR_INVALID, "frame count larger than the frame");
        const uint8_t *xs = p + 4, *df = xs + 4 * (size_t)cnt;   // opencv.cpp:52-62
        HIP_TRY(launch_apply(c->state, c->n, xs, df, nullptr, 0, cnt, c->stream));
        if (d_frames_out && c->n)
            HIP_TRY(hipMemcpyAsync((uint8_t *)d_frames_out + (size_t)t * stride_bytes, c->state, c->n,
                                   hipMemcpyDeviceToDevice, c->stream));
        p = df + cnt;
    }
    return MI355_OK;
}

int mi355_merge_parts(mi355_core *c, int nparts, int nframes, const void *d_part_offsets,
                      const uint32_t *h_part_base, const int32_t *h_xs_bias, const void *d_xs_all,
                      const void *d_diff_all, void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nparts < 1 || nparts > kMaxParts) return fail(MI355_ERR_INVALID, "nparts outside [1, 64]");
    if (nframes < 0) return fail(MI355_ERR_INVALID, "nframes < 0");
    if (!d_part_offsets || !h_part_base || !h_xs_bias || !d_offsets)
        return fail(MI355_ERR_INVALID, "null argument");
    if (capacity > 0 && (!d_xs_all || !d_diff_all || !d_xs || !d_diff))
        return fail(MI355_ERR_INVALID, "null stream pointer");
    if (int rc = use_device(c)) return rc;
    MergeArgs a{};
    a.part_off = (const uint32_t *)d_part_offsets;
    a.xs_all = (const int32_t *)d_xs_all;
    a.diff_all = (const uint8_t *)d_diff_all;
    a.out_xs = (int32_t *)d_xs;
    a.out_diff = (uint8_t *)d_diff;
    a.capacity = capacity;
    a.nparts = nparts;
    a.nframes = nframes;
    for (int p = 0; p < nparts; p++) {
        a.part_base[p] = h_part_base[p];
        a.xs_bias[p] = h_xs_bias[p];
    }
    HIP_TRY(launch_merge(a, (uint32_t *)d_offsets, c->stream));
    return MI355_OK;
}

// ---- compact wire (include/mi355diff.h) ----------------------------------------------------------------------------
size_t mi355_cwire_frame_bytes(uint32_t n, uint32_t e) { return (size_t)cwire_record_bytes(n, e); }

size_t mi355_cwire_bytes_max(size_t frame_bytes, int nframes) {
    return nframes > 0 ? (size_t)nframes * (size_t)cwire_record_bytes(frame_bytes, 0) : 0;
}

// The frame headers of a compact stream as the client read them (decode and GPU client): check() before anything is
// enqueued, then next() once per frame, in order, for the frame's place and header.
struct CwireHeaders {
    const uint32_t *counts, *escapes;
    int nframes;
    int t = 0;
    uint64_t pos = 0;
    // bounded: an entry count above frame_bytes is refused, too
    int check(bool bounded, uint32_t frame_bytes) const {
        for (int i = 0; i < nframes; i++) {
            if (escapes[i] > counts[i]) return fail(MI355_ERR_INVALID, "frame header: more escapes than entries");
            if (bounded && counts[i] > frame_bytes) return fail(MI355_ERR_INVALID, "frame header: more entries than frame bytes");
        }
        return MI355_OK;
    }
    struct Frame { uint64_t pos; uint32_t n, e; };
    Frame next() {
        const Frame f{pos, counts[t], escapes[t]};
        pos += cwire_record_bytes(f.n, f.e);
        t++;
        return f;
    }
};

// The record table of the GPU clients: the headers checked, then place, header and chunks of every record.  The chunk bases
// begin again every max_batch records: the scratch of the one-stream client holds one such slice (only mi355_apply_cwire_batch
// takes more records than that).
struct CwaTable {
    std::vector<CwaFrame> fr;
    uint64_t bytes = 0;   // of all the records
};
static int cwa_table(const mi355_core *c, const uint32_t *h_counts, const uint32_t *h_escapes, int nrecords, CwaTable *tab) {
    CwireHeaders hdr{h_counts, h_escapes, nrecords};
    if (int rc = hdr.check(true, c->n)) return rc;
    tab->fr.resize((size_t)nrecords);
    uint32_t cbase = 0;
    for (int k = 0; k < nrecords; k++) {
        if (k % c->cfg.max_batch == 0) cbase = 0;
        const CwireHeaders::Frame f = hdr.next();
        tab->fr[k] = CwaFrame{f.pos, f.n, f.e, cbase, cwa_chunks(f.n)};
        cbase += tab->fr[k].nc;
    }
    tab->bytes = hdr.pos;
    return MI355_OK;
}

// The core's scratch and frame size for a launch on the records at d_cwire; state / out / stride are the call's own.  Every
// field is filled for every call: the kernels of mi355_cwire_check_batch never read dir or ntiles, those of
// mi355_refresh_cwire_batch (d_cwire = nullptr) never read cwire, ftab or dir.
static CwaArgs cwa_args(const mi355_core *c, const void *d_cwire) {
    CwaArgs a{};
    a.cwire = (const uint8_t *)d_cwire;
    a.ftab = c->cwa_ftab;
    a.chunk = c->cwa_chunk;   // chunk facts for the directory, then one fact word per (stream, tile) where a call keeps such
    a.dir = c->cwa_dir;
    a.n = c->n;
    a.ntiles = cwa_tiles(c->n);
    return a;
}

// offsets[0] = 0 and frame_pos[0] = 0, where given, and nothing else: what an empty batch leaves
static int write_empty_heads(mi355_core *c, void *d_offsets, void *d_frame_pos) {
    if (!d_offsets && !d_frame_pos) return MI355_OK;
    if (int rc = use_device(c)) return rc;
    if (d_offsets) HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint32_t), c->stream));
    if (d_frame_pos) HIP_TRY(hipMemsetAsync(d_frame_pos, 0, sizeof(uint64_t), c->stream));
    return MI355_OK;
}

// *B = nstreams * nframes, the records or segments of a burst: refused below 0 and above max_batch
static int burst_count(const mi355_core *c, int nstreams, int nframes, int *B) {
    *B = 0;
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nframes < 0) return fail(MI355_ERR_INVALID, "nstreams or nframes < 0");
    if ((int64_t)nstreams * nframes > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams * nframes above max_batch");
    *B = nstreams * nframes;
    return MI355_OK;
}

int mi355_cwire_encode_batch(mi355_core *c, const void *d_offsets, const void *d_xs, const void *d_diff,
                             size_t entries_capacity, int nframes, void *d_frame_pos, void *d_cwire, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0) return fail(MI355_ERR_INVALID, "nframes < 0");
    if (nframes > kCwireSlots) return fail(MI355_ERR_INVALID, "nframes above 8192: encode the batch in parts");
    if (!d_offsets || !d_frame_pos) return fail(MI355_ERR_INVALID, "null d_offsets / d_frame_pos");
    if (entries_capacity > 0 && (!d_xs || !d_diff)) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (capacity_bytes > 0 && !d_cwire) return fail(MI355_ERR_INVALID, "null d_cwire");
    if (((uintptr_t)d_cwire & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_xs & 3u) || ((uintptr_t)d_frame_pos & 7u))
        return fail(MI355_ERR_INVALID, "d_cwire, d_offsets and d_xs must be 4-byte aligned, d_frame_pos 8-byte aligned");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(launch_cwire_encode((const uint32_t *)d_offsets, (const int32_t *)d_xs, (const uint8_t *)d_diff,
                                (uint64_t)entries_capacity, nframes, c->cw_cnt, (uint64_t *)d_frame_pos, (uint8_t *)d_cwire,
                                (uint64_t)capacity_bytes, c->stream));
    return MI355_OK;
}

int mi355_cwire_decode_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                             int nframes, void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0) return fail(MI355_ERR_INVALID, "nframes < 0");
    if (nframes == 0) return MI355_OK;
    if (!d_cwire || !h_counts || !h_escapes || !d_offsets) return fail(MI355_ERR_INVALID, "null argument");
    if (capacity > 0 && (!d_xs || !d_diff)) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (((uintptr_t)d_cwire & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_xs & 3u))
        return fail(MI355_ERR_INVALID, "d_cwire, d_offsets and d_xs must be 4-byte aligned");
    CwireHeaders hdr{h_counts, h_escapes, nframes};
    if (int rc = hdr.check(false, 0)) return rc;
    if (int rc = use_device(c)) return rc;
    CwireDecodeArgs a{};
    a.cwire = (const uint8_t *)d_cwire;
    a.offsets = (uint32_t *)d_offsets;
    a.xs = (int32_t *)d_xs;
    a.diff = (uint8_t *)d_diff;
    a.capacity = capacity;
    uint32_t out = 0;   // uint32, like every offsets array of the library
    for (int t0 = 0; t0 < nframes; t0 += kCwireDecodeFrames) {
        const int nf = nframes - t0 < kCwireDecodeFrames ? nframes - t0 : kCwireDecodeFrames;
        a.first_frame = t0;
        for (int k = 0; k < nf; k++) {
            const CwireHeaders::Frame f = hdr.next();
            a.frame[k] = CwireFrame{f.pos, f.n, f.e, out, 0};
            out += f.n;
        }
        HIP_TRY(launch_cwire_decode(a, nf, c->stream));
    }
    return MI355_OK;
}

int mi355_apply_cwire_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                            int nframes, void *d_frames_out, size_t stride_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0) return fail(MI355_ERR_INVALID, "nframes < 0");
    if (nframes == 0) return MI355_OK;
    if (!d_cwire || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null argument");
    if ((uintptr_t)d_cwire & 3u) return fail(MI355_ERR_INVALID, "d_cwire must be 4-byte aligned");
    if (d_frames_out && stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, nframes, &tab)) return rc;
    if (c->n == 0) return MI355_OK;   // (every count is 0)
    if (int rc = use_device(c)) return rc;
    CwaArgs a = cwa_args(c, d_cwire);
    a.state = c->state;
    a.stride = stride_bytes;
    const int T = c->cfg.max_batch;
    for (int t0 = 0; t0 < nframes; t0 += T) {   // slices of at most max_batch frames: the scratch holds one
        a.out = d_frames_out ? (uint8_t *)d_frames_out + (size_t)t0 * stride_bytes : nullptr;
        HIP_TRY(launch_cwire_apply(a, tab.fr.data() + t0, nframes - t0 < T ? nframes - t0 : T, c->stream));
    }
    return MI355_OK;
}

// ---- mi355_apply_multi(_stream)_*: nframes segments / records of each of nstreams streams onto the caller's states, batch index
// b = s*nframes + t (mi355_apply_multi_*: nframes = 1, no output frames) ---------------------------------------------------------
// What the six forms refuse alike, before anything is launched; *run = there is something to do
static int check_apply_multi_stream(mi355_core *c, bool inputs, int nstreams, int nframes, const void *d_states, size_t stride,
                                    const void *d_out, size_t out_stride, bool *run) {
    *run = false;
    int B;
    if (int rc = burst_count(c, nstreams, nframes, &B)) return rc;
    if (B == 0) return MI355_OK;
    if (!inputs) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!d_states) return fail(MI355_ERR_INVALID, "null d_states");
    if (stride < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if (d_out) {
        if (out_stride < c->n) return fail(MI355_ERR_INVALID, "out_stride_bytes < frame bytes");
        if (int rc = check_regions({out_frames_region(c, d_out, out_stride, B)}, {states_region(c, d_states, stride, nstreams)})) return rc;
    }
    *run = c->n > 0;
    return MI355_OK;
}

// An input of `bytes` bytes (known from the host's headers) against the states and, where there are any, the output frames
static int check_apply_multi_input(const mi355_core *c, const void *d_in, uint64_t bytes, int nstreams, int nframes, const void *d_states,
                                   size_t stride, const void *d_out, size_t out_stride) {
    return check_regions({input_region(d_in, bytes)},
                         {states_region(c, d_states, stride, nstreams),
                          d_out ? out_frames_region(c, d_out, out_stride, (int64_t)nstreams * nframes) : Region{}});
}

// One launch's streams [s0, s0 + h->count) of a wire stream, record t of each: batch index b = s*nframes + t, pos[b] its place
static void fill_apply_multi_wire(ApplyMultiWireArgs *h, int s0, int nstreams, int nframes, int t, const uint64_t *pos,
                                  const uint32_t *h_counts) {
    h->first = s0;
    h->count = nstreams - s0 < kApplyMultiWireStreams ? nstreams - s0 : kApplyMultiWireStreams;
    h->cum[0] = 0;
    for (int j = 0; j < h->count; j++) {
        const size_t b = (size_t)(s0 + j) * nframes + t;
        h->pos[j] = pos[b];
        h->cum[j + 1] = h->cum[j] + h_counts[b];
    }
}

// pos[b]: byte position of {n, xs, diff} of batch index b of a wire stream, pos[B] its length; refuses a count above the frame
static int wire_positions(const mi355_core *c, const uint32_t *h_counts, int B, std::vector<uint64_t> *pos) {
    pos->assign((size_t)B + 1, 0);
    for (int b = 0; b < B; b++) {
        if (h_counts[b] > c->n) return fail(MI355_ERR_INVALID, "frame count larger than the frame");
        (*pos)[b + 1] = (*pos)[b] + mi355_wire_bytes(1, h_counts[b]);
    }
    return MI355_OK;
}

int mi355_apply_multi_batch(mi355_core *c, const void *d_offsets, const void *d_xs, const void *d_diff, int nstreams,
                            void *d_states, size_t stride_bytes) {
    bool run;
    if (int rc = check_apply_multi_stream(c, d_offsets && d_xs && d_diff, nstreams, 1, d_states, stride_bytes, nullptr, 0, &run)) return rc;
    if (nstreams > 0 && (((uintptr_t)d_offsets | (uintptr_t)d_xs) & 3u))
        return fail(MI355_ERR_INVALID, "d_offsets and d_xs must be 4-byte aligned");
    if (!run) return MI355_OK;
    if (int rc = use_device(c)) return rc;
    HIP_TRY(launch_apply_multi((uint8_t *)d_states, stride_bytes, c->n, (const uint32_t *)d_offsets, (const int32_t *)d_xs,
                               (const uint8_t *)d_diff, nstreams, c->stream));
    return MI355_OK;
}

int mi355_apply_multi_wire_batch(mi355_core *c, const void *d_wire, const uint32_t *h_counts, int nstreams, void *d_states,
                                 size_t stride_bytes) {
    bool run;
    if (int rc = check_apply_multi_stream(c, d_wire && h_counts, nstreams, 1, d_states, stride_bytes, nullptr, 0, &run)) return rc;
    if (nstreams == 0) return MI355_OK;
    std::vector<uint64_t> pos;
    if (int rc = wire_positions(c, h_counts, nstreams, &pos)) return rc;
    if (int rc = check_apply_multi_input(c, d_wire, pos[nstreams], nstreams, 1, d_states, stride_bytes, nullptr, 0)) return rc;
    if (!run) return MI355_OK;
    if (int rc = use_device(c)) return rc;
    ApplyMultiWireArgs h{};
    for (int s0 = 0; s0 < nstreams; s0 += kApplyMultiWireStreams) {
        fill_apply_multi_wire(&h, s0, nstreams, 1, 0, pos.data(), h_counts);
        HIP_TRY(launch_apply_multi_wire((uint8_t *)d_states, stride_bytes, c->n, (const uint8_t *)d_wire, h, c->stream));
    }
    return MI355_OK;
}

int mi355_apply_multi_cwire_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                                  int nstreams, void *d_states, size_t stride_bytes) {
    bool run;
    if (int rc = check_apply_multi_stream(c, d_cwire && h_counts && h_escapes, nstreams, 1, d_states, stride_bytes, nullptr, 0, &run))
        return rc;
    if (nstreams == 0) return MI355_OK;
    if ((uintptr_t)d_cwire & 3u) return fail(MI355_ERR_INVALID, "d_cwire must be 4-byte aligned");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, nstreams, &tab)) return rc;
    if (int rc = check_apply_multi_input(c, d_cwire, tab.bytes, nstreams, 1, d_states, stride_bytes, nullptr, 0)) return rc;
    if (!run) return MI355_OK;
    if (int rc = use_device(c)) return rc;
    CwaArgs a = cwa_args(c, d_cwire);
    a.state = (uint8_t *)d_states;
    a.stride = stride_bytes;
    HIP_TRY(launch_cwire_apply_multi(a, tab.fr.data(), nstreams, c->stream));
    return MI355_OK;
}

int mi355_apply_multi_stream_batch(mi355_core *c, const void *d_offsets, const void *d_xs, const void *d_diff, int nstreams,
                                   int nframes, void *d_states, size_t stride_bytes, void *d_frames_out, size_t out_stride_bytes) {
    bool run;
    if (int rc = check_apply_multi_stream(c, d_offsets && d_xs && d_diff, nstreams, nframes, d_states, stride_bytes, d_frames_out,
                                          out_stride_bytes, &run))
        return rc;
    if (nstreams > 0 && nframes > 0 && (((uintptr_t)d_offsets | (uintptr_t)d_xs) & 3u))
        return fail(MI355_ERR_INVALID, "d_offsets and d_xs must be 4-byte aligned");
    if (!run) return MI355_OK;
    if (int rc = use_device(c)) return rc;
    for (int t = 0; t < nframes; t++) {   // records of one stream may hit the same byte: one launch per t (stream_ops.hip)
        HIP_TRY(launch_apply_multi_strided((uint8_t *)d_states, stride_bytes, c->n, (const uint32_t *)d_offsets,
                                           (const int32_t *)d_xs, (const uint8_t *)d_diff, nstreams, nframes, t, c->stream));
        if (d_frames_out)
            HIP_TRY(launch_apply_multi_show((const uint8_t *)d_states, stride_bytes, c->n, (uint8_t *)d_frames_out, out_stride_bytes,
                                            nstreams, nframes, t, c->stream));
    }
    return MI355_OK;
}

int mi355_apply_multi_stream_wire_batch(mi355_core *c, const void *d_wire, const uint32_t *h_counts, int nstreams, int nframes,
                                        void *d_states, size_t stride_bytes, void *d_frames_out, size_t out_stride_bytes) {
    bool run;
    if (int rc = check_apply_multi_stream(c, d_wire && h_counts, nstreams, nframes, d_states, stride_bytes, d_frames_out,
                                          out_stride_bytes, &run))
        return rc;
    const int B = nstreams > 0 && nframes > 0 ? nstreams * nframes : 0;   // (<= max_batch)
    if (B == 0) return MI355_OK;
    std::vector<uint64_t> pos;
    if (int rc = wire_positions(c, h_counts, B, &pos)) return rc;
    if (int rc = check_apply_multi_input(c, d_wire, pos[B], nstreams, nframes, d_states, stride_bytes, d_frames_out, out_stride_bytes))
        return rc;
    if (!run) return MI355_OK;
    if (int rc = use_device(c)) return rc;
    ApplyMultiWireArgs h{};
    for (int t = 0; t < nframes; t++) {   // launch t: record s*nframes + t of every stream s, 128 streams per launch
        for (int s0 = 0; s0 < nstreams; s0 += kApplyMultiWireStreams) {
            fill_apply_multi_wire(&h, s0, nstreams, nframes, t, pos.data(), h_counts);
            HIP_TRY(launch_apply_multi_wire((uint8_t *)d_states, stride_bytes, c->n, (const uint8_t *)d_wire, h, c->stream));
        }
        if (d_frames_out)
            HIP_TRY(launch_apply_multi_show((const uint8_t *)d_states, stride_bytes, c->n, (uint8_t *)d_frames_out, out_stride_bytes,
                                            nstreams, nframes, t, c->stream));
    }
    return MI355_OK;
}

int mi355_apply_multi_stream_cwire_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                                         int nstreams, int nframes, void *d_states, size_t stride_bytes, void *d_frames_out,
                                         size_t out_stride_bytes) {
    bool run;
    if (int rc = check_apply_multi_stream(c, d_cwire && h_counts && h_escapes, nstreams, nframes, d_states, stride_bytes,
                                          d_frames_out, out_stride_bytes, &run))
        return rc;
    const int B = nstreams > 0 && nframes > 0 ? nstreams * nframes : 0;   // (<= max_batch)
    if (B == 0) return MI355_OK;
    if ((uintptr_t)d_cwire & 3u) return fail(MI355_ERR_INVALID, "d_cwire must be 4-byte aligned");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, B, &tab)) return rc;
    if (int rc = check_apply_multi_input(c, d_cwire, tab.bytes, nstreams, nframes, d_states, stride_bytes, d_frames_out, out_stride_bytes))
        return rc;
    if (!run) return MI355_OK;
    if (int rc = use_device(c)) return rc;
    CwaArgs a = cwa_args(c, d_cwire);
    a.state = (uint8_t *)d_states;
    a.out = (uint8_t *)d_frames_out;
    a.stride = stride_bytes;
    HIP_TRY(launch_cwire_apply_multi_stream(a, tab.fr.data(), nstreams, nframes, out_stride_bytes, c->stream));
    return MI355_OK;
}

// ---- the calls that take a burst of compact records and write ONE segment or ONE compact record per stream ---------------------
// Their outputs, as the kernels take them, with what the calls refuse about them: offsets and either the arrays (xs, diff,
// capacity in entries) or, compact, the records (frame_pos, cwire, capacity in bytes); the pointers of the other form are null.
struct Produced : CwcOut {
    bool compact;
    static Produced arrays(void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
        return Produced{{(uint32_t *)d_offsets, nullptr, nullptr, (int32_t *)d_xs, (uint8_t *)d_diff, capacity}, false};
    }
    static Produced records(void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes) {
        return Produced{{(uint32_t *)d_offsets, (uint64_t *)d_frame_pos, (uint8_t *)d_cwire_out, nullptr, nullptr, capacity_bytes}, true};
    }
    // (d_cwire: the call's input, which the text names among the outputs)
    int check_aligned(const void *d_cwire) const {
        if (((uintptr_t)d_cwire & 3u) || ((uintptr_t)offsets & 3u) || ((uintptr_t)cwire & 3u) || ((uintptr_t)xs & 3u))
            return fail(MI355_ERR_INVALID, "d_cwire, d_cwire_out, d_offsets and d_xs must be 4-byte aligned");
        if ((uintptr_t)frame_pos & 7u) return fail(MI355_ERR_INVALID, "d_frame_pos must be 8-byte aligned");
        return MI355_OK;
    }
    int check_given() const {
        if (!offsets || (compact ? !frame_pos || !cwire : !xs || !diff)) return fail(MI355_ERR_INVALID, "null output pointer");
        return MI355_OK;
    }
    // Refuses an output that overlaps the input, output by output; nsegments: the segments / records written (nstreams, or the
    // mosaic's one)
    int check_apart(const Region &in, int nsegments) const {
        if (compact)
            return check_regions({in}, {offsets_region(offsets, nsegments), frame_pos_region(frame_pos, nsegments),
                                        Region{cwire, capacity, "d_cwire_out"}});
        return check_regions({in}, {offsets_region(offsets, nsegments), Region{xs, 4 * capacity, "d_xs"}, Region{diff, capacity, "d_diff"}});
    }
};

// The last rungs of coalesce, crop and mosaic alike: the record table (its header refusals), the overlap refusals, the device
static int producer_table(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int B, const Produced &o,
                          int nsegments, CwaTable *tab) {
    if (int rc = cwa_table(c, h_counts, h_escapes, B, tab)) return rc;
    if (int rc = o.check_apart(input_region(d_cwire, tab->bytes), nsegments)) return rc;
    return use_device(c);
}

// ---- mi355_cwire_coalesce_(cwire_)batch: nframes records of each of nstreams streams -> ONE segment / record per stream -------
// Both forms: everything is refused here, before anything is launched; the core's state is not touched.
static int coalesce(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams,
                    int nframes, const Produced &o) {
    int B;
    if (int rc = burst_count(c, nstreams, nframes, &B)) return rc;
    if (int rc = o.check_aligned(d_cwire)) return rc;
    if (B == 0) return write_empty_heads(c, o.offsets, o.frame_pos);
    if (!d_cwire || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (int rc = o.check_given()) return rc;
    CwaTable tab;
    if (int rc = producer_table(c, d_cwire, h_counts, h_escapes, B, o, nstreams, &tab)) return rc;
    HIP_TRY(launch_cwire_coalesce(cwa_args(c, d_cwire), tab.fr.data(), nstreams, nframes, o, o.compact, c->stream));
    return MI355_OK;
}

int mi355_cwire_coalesce_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                               int nstreams, int nframes, void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    return coalesce(c, d_cwire, h_counts, h_escapes, nstreams, nframes, Produced::arrays(d_offsets, d_xs, d_diff, capacity));
}

int mi355_cwire_coalesce_cwire_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                                     int nstreams, int nframes, void *d_offsets, void *d_frame_pos, void *d_cwire_out,
                                     size_t capacity_bytes) {
    return coalesce(c, d_cwire, h_counts, h_escapes, nstreams, nframes, Produced::records(d_offsets, d_frame_pos, d_cwire_out, capacity_bytes));
}

// ---- mi355_cwire_crop_(cwire_)batch: coalesce(...) with every stream's sums cut to its rectangle -----------------------------
// Both forms: everything is refused here, before anything is launched; the core's state is not touched.  The per-stream words
// are the budget call's (c->cwb_hist, max_batch rows): both calls are ordered on the core's stream.
static int crop(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams, int nframes,
                const int32_t *h_rects, unsigned flags, const Produced &o) {
    int B;
    if (int rc = burst_count(c, nstreams, nframes, &B)) return rc;
    if (flags & ~MI355_CROP_KEEP_INDEX) return fail(MI355_ERR_INVALID, "unknown flag bit (MI355_CROP_KEEP_INDEX is the only one)");
    if (int rc = o.check_aligned(d_cwire)) return rc;
    if (B == 0) return write_empty_heads(c, o.offsets, o.frame_pos);
    if (!d_cwire || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!h_rects) return fail(MI355_ERR_INVALID, "null h_rects");
    if (int rc = o.check_given()) return rc;
    for (int s = 0; s < nstreams; s++) {
        const int32_t *r = h_rects + 4 * (size_t)s;
        if (r[0] < 0 || r[1] < 0 || r[2] < 0 || r[3] < 0) return fail(MI355_ERR_INVALID, "rectangle with a negative member");
        if ((int64_t)r[0] + r[2] > c->cfg.width || (int64_t)r[1] + r[3] > c->cfg.height)
            return fail(MI355_ERR_INVALID, "rectangle outside the frame");
    }
    CwaTable tab;
    if (int rc = producer_table(c, d_cwire, h_counts, h_escapes, B, o, nstreams, &tab)) return rc;
    HIP_TRY(launch_cwire_crop(cwa_args(c, d_cwire), tab.fr.data(), nstreams, nframes, h_rects, (uint32_t)c->cfg.width,
                              (flags & MI355_CROP_KEEP_INDEX) != 0, c->cwb_hist, o, o.compact, c->stream));
    return MI355_OK;
}

int mi355_cwire_crop_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams,
                           int nframes, const int32_t *h_rects, unsigned flags, void *d_offsets, void *d_xs, void *d_diff,
                           size_t capacity) {
    return crop(c, d_cwire, h_counts, h_escapes, nstreams, nframes, h_rects, flags, Produced::arrays(d_offsets, d_xs, d_diff, capacity));
}

int mi355_cwire_crop_cwire_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams,
                                 int nframes, const int32_t *h_rects, unsigned flags, void *d_offsets, void *d_frame_pos,
                                 void *d_cwire_out, size_t capacity_bytes) {
    return crop(c, d_cwire, h_counts, h_escapes, nstreams, nframes, h_rects, flags,
                Produced::records(d_offsets, d_frame_pos, d_cwire_out, capacity_bytes));
}

// ---- mi355_cwire_mosaic_(cwire_)batch: the streams' coalesced records placed on a canvas, ONE segment / record out --------------
// Both forms: everything is refused here, before anything is launched; the core's state is not touched.  The per-stream words
// are the budget call's, as for the crop; the facts of the canvas' tiles take the chunk scratch, which holds max_batch *
// cwa_chunks(N) words and is not grown here.
static int mosaic(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams, int nframes,
                  const int32_t *h_place, int canvas_w, int canvas_h, const Produced &o) {
    int B;
    if (int rc = burst_count(c, nstreams, nframes, &B)) return rc;
    if (canvas_w < 1 || canvas_h < 1) return fail(MI355_ERR_INVALID, "canvas_w or canvas_h < 1");
    const uint64_t nc = 3ull * (uint64_t)canvas_w * (uint64_t)canvas_h;
    if (nc >= (1ull << 31)) return fail(MI355_ERR_INVALID, "canvas of 2^31 bytes or more");
    if ((uint64_t)mi355_state_tiles((size_t)nc) > (uint64_t)c->cfg.max_batch * mi355_state_tiles(c->n))
        return fail(MI355_ERR_INVALID, "canvas of more 4096-byte tiles than max_batch frames hold: create the core with a larger max_batch");
    if (int rc = o.check_aligned(d_cwire)) return rc;
    if (B == 0) return write_empty_heads(c, o.offsets, o.frame_pos);
    if (!d_cwire || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!h_place) return fail(MI355_ERR_INVALID, "null h_place");
    if (int rc = o.check_given()) return rc;
    for (int s = 0; s < nstreams; s++) {
        const int32_t *p = h_place + 6 * (size_t)s;
        for (int k = 0; k < 6; k++)
            if (p[k] < 0) return fail(MI355_ERR_INVALID, "placement with a negative member");
        if ((int64_t)p[0] + p[2] > c->cfg.width || (int64_t)p[1] + p[3] > c->cfg.height)
            return fail(MI355_ERR_INVALID, "source rectangle outside the frame");
        if ((int64_t)p[4] + p[2] > canvas_w || (int64_t)p[5] + p[3] > canvas_h)
            return fail(MI355_ERR_INVALID, "destination rectangle outside the canvas");
    }
    CwaTable tab;
    if (int rc = producer_table(c, d_cwire, h_counts, h_escapes, B, o, 1, &tab)) return rc;
    HIP_TRY(launch_cwire_mosaic(cwa_args(c, d_cwire), tab.fr.data(), nstreams, nframes, h_place, (uint32_t)c->cfg.width, (uint32_t)canvas_w,
                                (uint32_t)nc, c->cwb_hist, o, o.compact, c->stream));
    return MI355_OK;
}

int mi355_cwire_mosaic_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams,
                             int nframes, const int32_t *h_place, int canvas_w, int canvas_h, void *d_offsets, void *d_xs, void *d_diff,
                             size_t capacity) {
    return mosaic(c, d_cwire, h_counts, h_escapes, nstreams, nframes, h_place, canvas_w, canvas_h,
                  Produced::arrays(d_offsets, d_xs, d_diff, capacity));
}

int mi355_cwire_mosaic_cwire_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams,
                                   int nframes, const int32_t *h_place, int canvas_w, int canvas_h, void *d_offsets, void *d_frame_pos,
                                   void *d_cwire_out, size_t capacity_bytes) {
    return mosaic(c, d_cwire, h_counts, h_escapes, nstreams, nframes, h_place, canvas_w, canvas_h,
                  Produced::records(d_offsets, d_frame_pos, d_cwire_out, capacity_bytes));
}

// ---- mi355_cwire_budget_cwire_batch: the records of one tick held to an entry budget each ------------------------------------
size_t mi355_cwire_budget_entries(size_t frame_bytes, size_t record_bytes) {
    // the largest n <= frame_bytes whose worst record (e = min(n, frame_bytes / 256) escapes) fits; the size rises with n
    const uint64_t most_e = frame_bytes / 256;
    uint64_t lo = 0, hi = frame_bytes;   // lo fits (or nothing does), hi + 1 does not
    if (record_bytes < 8) return 0;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (cwire_record_bytes(mid, mid < most_e ? mid : most_e) <= (uint64_t)record_bytes) lo = mid;
        else hi = mid - 1;
    }
    return (size_t)lo;
}

int mi355_cwire_budget_cwire_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                                   void *d_states, size_t stride_bytes, int nstreams, const uint32_t *h_budget, void *d_thresholds,
                                   void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nstreams > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams outside [0, max_batch]");
    if (((uintptr_t)d_cwire & 3u) || ((uintptr_t)d_cwire_out & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_thresholds & 3u))
        return fail(MI355_ERR_INVALID, "d_cwire, d_cwire_out, d_offsets and d_thresholds must be 4-byte aligned");
    if ((uintptr_t)d_frame_pos & 7u) return fail(MI355_ERR_INVALID, "d_frame_pos must be 8-byte aligned");
    if (nstreams == 0) return write_empty_heads(c, d_offsets, d_frame_pos);
    if (!d_cwire || !h_counts || !h_escapes || !d_states || !h_budget) return fail(MI355_ERR_INVALID, "null input pointer");
    if (!d_thresholds || !d_offsets || !d_frame_pos || !d_cwire_out) return fail(MI355_ERR_INVALID, "null output pointer");
    if (stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, nstreams, &tab)) return rc;
    const Region in = input_region(d_cwire, tab.bytes), st = states_region(c, d_states, stride_bytes, nstreams);
    if (overlap(st, in)) return overlap_fail(st, in);
    if (int rc = check_regions({in, st}, {offsets_region(d_offsets, nstreams), Region{d_thresholds, (uint64_t)nstreams * sizeof(uint32_t), "d_thresholds"},
                                          frame_pos_region(d_frame_pos, nstreams), Region{d_cwire_out, capacity_bytes, "d_cwire_out"}}))
        return rc;
    if (int rc = use_device(c)) return rc;
    CwaArgs a = cwa_args(c, d_cwire);
    a.state = (uint8_t *)d_states;
    a.stride = stride_bytes;
    HIP_TRY(launch_cwire_budget(a, tab.fr.data(), nstreams, h_budget, (uint32_t)c->cfg.threshold, c->cwb_hist, (uint32_t *)d_thresholds,
                                Produced::records(d_offsets, d_frame_pos, d_cwire_out, capacity_bytes), c->stream));
    return MI355_OK;
}

// ---- mi355_cwire_despeckle_host / _cwire_batch: the records of one tick without their isolated changes ------------------------
// The definition.  Everything is validated and decoded before anything is written.
int mi355_cwire_despeckle_host(int width, int height, const void *cwire, size_t cwire_bytes, const uint32_t *h_counts,
                               const uint32_t *h_escapes, uint8_t *states, size_t spacing_bytes, int nstreams, const uint32_t *h_need,
                               uint32_t *dropped, uint32_t *offsets, uint64_t *frame_pos, void *cwire_out, size_t capacity_bytes) {
    if (nstreams < 0) return fail(MI355_ERR_INVALID, "nstreams < 0");
    if (width < 1 || height < 1) return fail(MI355_ERR_INVALID, "width or height < 1");
    const uint64_t P = (uint64_t)width * (uint64_t)height, N = 3 * P;
    if (N >= (1ull << 31)) return fail(MI355_ERR_INVALID, "frame of 2^31 bytes or more");
    if (spacing_bytes < N) return fail(MI355_ERR_INVALID, "spacing_bytes (the stride of the states) < frame bytes");
    if (nstreams > 0 && (!cwire || !h_counts || !h_escapes || !states || !h_need)) return fail(MI355_ERR_INVALID, "null input pointer");
    if (nstreams > 0 && (!dropped || !offsets || !frame_pos || !cwire_out)) return fail(MI355_ERR_INVALID, "null output pointer");
    const uint8_t *p = (const uint8_t *)cwire;
    std::vector<std::vector<uint32_t>> xs((size_t)nstreams);
    std::vector<std::vector<uint8_t>> ds((size_t)nstreams);
    char msg[160];
    uint64_t at = 0;
    for (int s = 0; s < nstreams; s++) {
        const uint32_t n = h_counts[s], e = h_escapes[s];
        if (h_need[s] > 8) {
            snprintf(msg, sizeof msg, "stream %d: need %u > 8", s, h_need[s]);
            return fail(MI355_ERR_INVALID, msg);
        }
        if (n > N) {
            snprintf(msg, sizeof msg, "compact stream: record %d: %u entries > frame bytes", s, n);
            return fail(MI355_ERR_INVALID, msg);
        }
        if (e > n) {
            snprintf(msg, sizeof msg, "compact stream: record %d: %u escapes > %u entries", s, e, n);
            return fail(MI355_ERR_INVALID, msg);
        }
        const uint64_t rec = cwire_record_bytes(n, e);
        if (at > cwire_bytes || cwire_bytes - at < rec) {
            snprintf(msg, sizeof msg, "compact stream: record %d: truncated record", s);
            return fail(MI355_ERR_INVALID, msg);
        }
        const CwireSections<const uint8_t> sec(p, at, n, e);
        uint32_t n255 = 0;
        for (uint32_t k = 0; k < n; k++) n255 += sec.code[k] == 255;
        if (n255 != e) {
            snprintf(msg, sizeof msg, "compact stream: record %d: %u escape codes, header says %u", s, n255, e);
            return fail(MI355_ERR_INVALID, msg);
        }
        uint64_t x = 0;   // running index + 1 (64-bit: escape values cannot wrap it)
        for (uint32_t k = 0, r = 0; k < n; k++) {
            uint32_t g = sec.code[k];
            if (g == 255) memcpy(&g, sec.esc + 4 * (size_t)r++, 4);
            x += (uint64_t)g + 1;
            if (x > N) {
                snprintf(msg, sizeof msg, "compact stream: record %d: entry %u decodes to an index >= frame bytes", s, k);
                return fail(MI355_ERR_INVALID, msg);
            }
            if (sec.diff[k]) {   // (a zero difference is no entry)
                xs[s].push_back((uint32_t)(x - 1));
                ds[s].push_back(sec.diff[k]);
            }
        }
        at += rec;
    }
    // which entries stay: the changed pixels around the entry's pixel, counted on a map with a border of one pixel
    const size_t bw = (size_t)width + 2;
    std::vector<uint8_t> changed;
    uint8_t *out = (uint8_t *)cwire_out;
    uint32_t first = 0;
    uint64_t pos = 0;
    for (int s = 0; s < nstreams; s++) {
        const uint32_t need = h_need[s];
        std::vector<uint32_t> &x = xs[s];
        std::vector<uint8_t> &d = ds[s];
        size_t kept = x.size();
        if (need) {
            changed.assign(bw * ((size_t)height + 2), 0);
            const auto cell = [&](uint32_t xi) { return ((size_t)(xi / 3) / width + 1) * bw + (xi / 3) % width + 1; };
            for (uint32_t xi : x) changed[cell(xi)] = 1;
            uint8_t *state = states + (size_t)s * spacing_bytes;
            kept = 0;
            for (size_t k = 0; k < x.size(); k++) {
                const uint8_t *m = &changed[cell(x[k])], *up = m - bw, *down = m + bw;
                const uint32_t c = up[-1] + up[0] + up[1] + m[-1] + m[1] + down[-1] + down[0] + down[1];
                if (c >= need) {
                    x[kept] = x[k];
                    d[kept++] = d[k];
                } else {
                    state[x[k]] = (uint8_t)(state[x[k]] - d[k]);   // the value before the tick
                }
            }
        }
        dropped[s] = (uint32_t)(x.size() - kept);
        uint32_t e = 0, end = 0;
        for (size_t k = 0; k < kept; k++) {
            e += x[k] - end >= 255u;
            end = x[k] + 1u;
        }
        const uint32_t n = (uint32_t)kept;
        const uint64_t rec = cwire_record_bytes(n, e);
        offsets[s] = first;
        frame_pos[s] = pos;
        if (pos + rec <= capacity_bytes) {   // (a record that does not fit is skipped whole)
            memset(out + pos, 0, rec);
            memcpy(out + pos, &n, 4);
            memcpy(out + pos + 4, &e, 4);
            const CwireSections<uint8_t> sec(out, pos, n, e);
            end = 0;
            for (uint32_t k = 0, r = 0; k < n; k++) {
                const uint32_t g = x[k] - end;
                sec.code[k] = (uint8_t)(g < 255u ? g : 255u);
                if (g >= 255u) memcpy(sec.esc + 4 * (size_t)r++, &g, 4);
                sec.diff[k] = d[k];
                end = x[k] + 1u;
            }
        }
        first += n;
        pos += rec;
    }
    if (offsets) offsets[nstreams] = first;
    if (frame_pos) frame_pos[nstreams] = pos;
    return MI355_OK;
}

// The pixel bitmaps (changed, keep; max_batch streams each) of the despeckle call: made when first needed, or by
// mi355_prepare(MI355_PREPARE_DESPECKLE) -- 133 MB at 1080p with max_batch 256, so not every core carries them.
static int need_despeckle(mi355_core *c) {
    if (c->dsp_bits || c->n == 0) return MI355_OK;
    const size_t words = 2 * (size_t)c->cfg.max_batch * dsp_words(c->n);
    if (int rc = dev_alloc(c, &c->dsp_bits, words)) return rc;
    HIP_TRY(hipMemsetAsync(c->dsp_bits, 0, words * sizeof(uint32_t), c->stream));
    return MI355_OK;
}

int mi355_cwire_despeckle_cwire_batch(mi355_core *c, const void *d_cwire_in, const uint32_t *h_counts, const uint32_t *h_escapes,
                                      void *d_states, size_t spacing_bytes, int nstreams, const uint32_t *h_need, void *d_dropped,
                                      void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nstreams > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams outside [0, max_batch]");
    if (((uintptr_t)d_cwire_in & 3u) || ((uintptr_t)d_cwire_out & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_dropped & 3u))
        return fail(MI355_ERR_INVALID, "d_cwire_in, d_cwire_out, d_offsets and d_dropped must be 4-byte aligned");
    if ((uintptr_t)d_frame_pos & 7u) return fail(MI355_ERR_INVALID, "d_frame_pos must be 8-byte aligned");
    if (nstreams == 0) return write_empty_heads(c, d_offsets, d_frame_pos);
    if (!d_cwire_in || !h_counts || !h_escapes || !d_states || !h_need) return fail(MI355_ERR_INVALID, "null input pointer");
    if (!d_dropped || !d_offsets || !d_frame_pos || !d_cwire_out) return fail(MI355_ERR_INVALID, "null output pointer");
    if (spacing_bytes < c->n) return fail(MI355_ERR_INVALID, "spacing_bytes (the stride of the states) < frame bytes");
    for (int s = 0; s < nstreams; s++)
        if (h_need[s] > 8) return fail(MI355_ERR_INVALID, "h_need above 8");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, nstreams, &tab)) return rc;
    const Region in = input_region(d_cwire_in, tab.bytes), st = states_region(c, d_states, spacing_bytes, nstreams);
    if (overlap(st, in)) return overlap_fail(st, in);
    if (int rc = check_regions({in, st}, {offsets_region(d_offsets, nstreams), Region{d_dropped, (uint64_t)nstreams * sizeof(uint32_t), "d_dropped"},
                                          frame_pos_region(d_frame_pos, nstreams), Region{d_cwire_out, capacity_bytes, "d_cwire_out"}}))
        return rc;
    if (int rc = use_device(c)) return rc;
    if (int rc = need_despeckle(c)) return rc;
    CwaArgs a = cwa_args(c, d_cwire_in);
    a.state = (uint8_t *)d_states;
    a.stride = spacing_bytes;
    uint32_t *changed = c->dsp_bits, *keep = changed + (size_t)c->cfg.max_batch * dsp_words(c->n);
    HIP_TRY(launch_cwire_despeckle(a, tab.fr.data(), nstreams, h_need, (uint32_t)c->cfg.width, c->cwb_hist, changed, keep, (uint32_t *)d_dropped,
                                   Produced::records(d_offsets, d_frame_pos, d_cwire_out, capacity_bytes), c->stream));
    return MI355_OK;
}

// ---- mi355_(cwire_)activity_batch: per stream, where the entries of its records land (stream_ops.hip, k_act_*) ----------------
size_t mi355_activity_cells(int width, int height, int cell_w, int cell_h, int *grid_w, int *grid_h) {
    const bool ok = width >= 1 && height >= 1 && cell_w >= 1 && cell_h >= 1;
    const int gw = ok ? (int)(((int64_t)width + cell_w - 1) / cell_w) : 0, gh = ok ? (int)(((int64_t)height + cell_h - 1) / cell_h) : 0;
    if (grid_w) *grid_w = gw;
    if (grid_h) *grid_h = gh;
    return (size_t)gw * (size_t)gh;
}

// What both forms refuse alike, before anything is launched; *B = nstreams * nframes (0: nothing to do).  in0 / in1: the form's
// two device inputs, in_ok: none of its inputs is null.
static int check_activity(mi355_core *c, const void *in0, const void *in1, bool in_ok, int nstreams, int nframes, int cell_w, int cell_h,
                          uint32_t min_count, const void *d_cells, const void *d_summary, int *B, ActGeom *g) {
    if (int rc = burst_count(c, nstreams, nframes, B)) return rc;
    if (cell_w < 1 || cell_h < 1) return fail(MI355_ERR_INVALID, "cell_w or cell_h < 1");
    if (min_count < 1) return fail(MI355_ERR_INVALID, "min_count < 1");
    if (((uintptr_t)in0 | (uintptr_t)in1 | (uintptr_t)d_cells | (uintptr_t)d_summary) & 3u)
        return fail(MI355_ERR_INVALID, "the device pointers must be 4-byte aligned");
    if (*B == 0) return MI355_OK;
    if (!in_ok) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!d_cells || !d_summary) return fail(MI355_ERR_INVALID, "null output pointer");
    int gw = 0;
    g->n = c->n;
    g->width = act_divisor((uint32_t)c->cfg.width);
    g->cell_w = act_divisor((uint32_t)cell_w);
    g->cell_h = act_divisor((uint32_t)cell_h);
    g->cells = (uint32_t)mi355_activity_cells(c->cfg.width, c->cfg.height, cell_w, cell_h, &gw, nullptr);
    g->grid_w = (uint32_t)gw;
    g->min_count = min_count;
    return MI355_OK;
}

int mi355_activity_batch(mi355_core *c, const void *d_offsets, const void *d_xs, int nstreams, int nframes, int cell_w, int cell_h,
                         uint32_t min_count, int accumulate, void *d_cells, void *d_summary) {
    int B;
    ActGeom g{};
    if (int rc = check_activity(c, d_offsets, d_xs, d_offsets && d_xs, nstreams, nframes, cell_w, cell_h, min_count, d_cells, d_summary, &B, &g))
        return rc;
    if (B == 0) return MI355_OK;
    if (int rc = use_device(c)) return rc;
    HIP_TRY(launch_activity((const uint32_t *)d_offsets, (const int32_t *)d_xs, nstreams, nframes, g, accumulate != 0, (uint32_t *)d_cells,
                            (uint32_t *)d_summary, c->stream));
    return MI355_OK;
}

int mi355_cwire_activity_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams,
                               int nframes, int cell_w, int cell_h, uint32_t min_count, int accumulate, void *d_cells, void *d_summary) {
    int B;
    ActGeom g{};
    if (int rc = check_activity(c, d_cwire, nullptr, d_cwire && h_counts && h_escapes, nstreams, nframes, cell_w, cell_h, min_count, d_cells,
                                d_summary, &B, &g))
        return rc;
    if (B == 0) return MI355_OK;
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, B, &tab)) return rc;
    if (int rc = check_regions({input_region(d_cwire, tab.bytes)}, {Region{d_cells, 4 * (uint64_t)nstreams * g.cells, "d_cells"},
                                                                    Region{d_summary, 32 * (uint64_t)nstreams, "d_summary"}}))
        return rc;
    if (int rc = use_device(c)) return rc;
    const CwaArgs a = cwa_args(c, d_cwire);
    HIP_TRY(launch_cwire_activity(a, tab.fr.data(), nstreams, nframes, g, accumulate != 0, (uint32_t *)d_cells, (uint32_t *)d_summary, c->stream));
    return MI355_OK;
}

// client/opencv.cpp:50-66 on the compact stream, on the host.  A frame is validated whole before any byte of the state
// changes, so a malformed frame leaves the state as the frames before it made it.
int mi355_cwire_apply_host(uint8_t *state, size_t frame_bytes, const void *cwire, size_t cwire_bytes, int nframes,
                           size_t *consumed) {
    if (consumed) *consumed = 0;
    if (!state || !cwire || !consumed) return fail(MI355_ERR_INVALID, "null argument");
    if (nframes < 0) return fail(MI355_ERR_INVALID, "nframes < 0");
    const uint8_t *p = (const uint8_t *)cwire;
    size_t at = 0;
    char msg[160];
    for (int t = 0; t < nframes; t++) {
        if (cwire_bytes - at < 8) {
            snprintf(msg, sizeof msg, "compact stream: frame %d: truncated header", t);
            return fail(MI355_ERR_INVALID, msg);
        }
        uint32_t n, e;
        memcpy(&n, p + at, 4);
        memcpy(&e, p + at + 4, 4);
        if (n > frame_bytes) {
            snprintf(msg, sizeof msg, "compact stream: frame %d: %u entries > frame bytes", t, n);
            return fail(MI355_ERR_INVALID, msg);
        }
        if (e > n) {
            snprintf(msg, sizeof msg, "compact stream: frame %d: %u escapes > %u entries", t, e, n);
            return fail(MI355_ERR_INVALID, msg);
        }
        const size_t rec = mi355_cwire_frame_bytes(n, e);
        if (cwire_bytes - at < rec) {
            snprintf(msg, sizeof msg, "compact stream: frame %d: truncated record", t);
            return fail(MI355_ERR_INVALID, msg);
        }
        const CwireSections<const uint8_t> sec(p, at, n, e);
        const uint8_t *code = sec.code, *escb = sec.esc, *diff = sec.diff;
        uint32_t n255 = 0;
        for (uint32_t k = 0; k < n; k++) n255 += code[k] == 255;
        if (n255 != e) {
            snprintf(msg, sizeof msg, "compact stream: frame %d: %u escape codes, header says %u", t, n255, e);
            return fail(MI355_ERR_INVALID, msg);
        }
        uint64_t x = 0;   // running index + 1 (64-bit: escape values cannot wrap it)
        for (uint32_t k = 0, r = 0; k < n; k++) {
            uint32_t g = code[k];
            if (g == 255) memcpy(&g, escb + 4 * (size_t)r++, 4);
            x += (uint64_t)g + 1;
            if (x > frame_bytes) {
                snprintf(msg, sizeof msg, "compact stream: frame %d: entry %u decodes to an index >= frame bytes", t, k);
                return fail(MI355_ERR_INVALID, msg);
            }
        }
        x = 0;
        for (uint32_t k = 0, r = 0; k < n; k++) {
            uint32_t g = code[k];
            if (g == 255) memcpy(&g, escb + 4 * (size_t)r++, 4);
            x += (uint64_t)g + 1;
            state[x - 1] = (uint8_t)(state[x - 1] + diff[k]);   // opencv.cpp:65
        }
        at += rec;
        *consumed = at;
    }
    return MI355_OK;
}

// ---- mi355_cwire_check_host / _batch: one verdict of four words per record (include/mi355diff.h) ---------------------------
// The definition: the decode rule of the GPU clients with a running total that cannot wrap (frame_bytes < 2^32 - 1 and every
// step adds at most 2^32, so a total that has passed 2^33 is frozen: it stays above frame_bytes and above the saturation point).
int mi355_cwire_check_host(size_t frame_bytes, const void *cwire, size_t cwire_bytes, const uint32_t *h_counts,
                           const uint32_t *h_escapes, int nrecords, uint32_t *verdicts) {
    if (nrecords < 0) return fail(MI355_ERR_INVALID, "nrecords < 0");
    if (frame_bytes >= 0xFFFFFFFFull) return fail(MI355_ERR_INVALID, "frame_bytes must be below 2^32 - 1");
    if (nrecords == 0) return MI355_OK;
    if (!cwire || !h_counts || !h_escapes || !verdicts) return fail(MI355_ERR_INVALID, "null argument");
    uint64_t end = 0;
    for (int b = 0; b < nrecords; b++) {
        if (h_escapes[b] > h_counts[b]) return fail(MI355_ERR_INVALID, "frame header: more escapes than entries");
        if (h_counts[b] > frame_bytes) return fail(MI355_ERR_INVALID, "frame header: more entries than frame bytes");
        end += cwire_record_bytes(h_counts[b], h_escapes[b]);
        if (end > cwire_bytes) return fail(MI355_ERR_INVALID, "the records end past cwire_bytes");
    }
    const uint8_t *p = (const uint8_t *)cwire;
    uint64_t pos = 0;
    for (int b = 0; b < nrecords; b++) {
        const uint32_t n = h_counts[b], e = h_escapes[b];
        const CwireSections<const uint8_t> sec(p, pos, n, e);
        uint32_t hn, he, flags = 0, r = 0, first = n;
        memcpy(&hn, p + pos, 4);
        memcpy(&he, p + pos + 4, 4);
        if (hn != n || he != e) flags |= MI355_CWIRE_BAD_HEADER;
        uint64_t x = 0;
        for (uint32_t k = 0; k < n; k++) {
            uint64_t g = sec.code[k];
            if (g == 255) {
                if (r++ >= e) continue;   // a bad escape: the total stays
                uint32_t v;
                memcpy(&v, sec.esc + 4 * (size_t)(r - 1), 4);
                if (v < 255) flags |= MI355_CWIRE_BAD_ESCAPE;
                g = v;
            }
            if (x < (1ull << 33)) x += g + 1;
            if (x > frame_bytes && first == n) first = k;
        }
        for (uint64_t k = n; k < cwire_pad4(n); k++)
            if (sec.code[k] | sec.diff[k]) flags |= MI355_CWIRE_BAD_PAD;
        if (r != e) flags |= MI355_CWIRE_BAD_CODES;
        if (first < n) flags |= MI355_CWIRE_BAD_RANGE;
        uint32_t *v = verdicts + 4 * (size_t)b;
        v[0] = flags;
        v[1] = r;
        v[2] = first;
        v[3] = x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x;
        pos += cwire_record_bytes(n, e);
    }
    return MI355_OK;
}

int mi355_cwire_check_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nrecords,
                            void *d_verdicts) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nrecords < 0 || nrecords > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nrecords outside [0, max_batch]");
    if (nrecords == 0) return MI355_OK;
    if (!d_cwire || !h_counts || !h_escapes || !d_verdicts) return fail(MI355_ERR_INVALID, "null argument");
    if (((uintptr_t)d_cwire | (uintptr_t)d_verdicts) & 3u) return fail(MI355_ERR_INVALID, "d_cwire and d_verdicts must be 4-byte aligned");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, nrecords, &tab)) return rc;
    if (int rc = check_regions({input_region(d_cwire, tab.bytes)}, {Region{d_verdicts, 16 * (uint64_t)nrecords, "d_verdicts"}})) return rc;
    if (int rc = use_device(c)) return rc;
    const CwaArgs a = cwa_args(c, d_cwire);
    HIP_TRY(launch_cwire_check(a, tab.fr.data(), nrecords, (uint32_t *)d_verdicts, c->stream));
    return MI355_OK;
}

// ---- mi355_cwire_split_host / _cwire_batch: records cut into pieces of at most max_bytes (include/mi355diff.h, "the piece rule") ----
static uint64_t split_content_pieces(uint64_t n, uint64_t e, uint64_t M) { return (2 * cwire_pad4(n) + 4 * e) / (M - 35); }

size_t mi355_cwire_split_pieces_max(uint32_t n, uint32_t e, size_t max_bytes) {
    if (max_bytes < 64 || max_bytes > kCwsBlock) return 0;
    return (size_t)(((uint64_t)n + kCwsBlock - 1) / kCwsBlock + split_content_pieces(n, e, max_bytes));
}

size_t mi355_cwire_split_bytes_max(uint32_t n, uint32_t e, size_t max_bytes) {
    if (max_bytes < 64 || max_bytes > kCwsBlock) return 0;
    return (size_t)cwire_record_bytes(n, e) + 12 * mi355_cwire_split_pieces_max(n, e, max_bytes);
}

static int split_check_limit(size_t max_bytes) {
    if (max_bytes < 64 || max_bytes > kCwsBlock || (max_bytes & 3u))
        return fail(MI355_ERR_INVALID, "max_bytes must be a multiple of 4 in [64, 65536]");
    return MI355_OK;
}

// The definition.  The decode rule of the GPU clients (an escape ranked at or past e adds nothing, the running index wraps at
// 2^32), so that the piece sizes of malformed content are the device form's, too.
int mi355_cwire_split_host(size_t frame_bytes, const void *cwire, size_t cwire_bytes, const uint32_t *h_counts,
                           const uint32_t *h_escapes, int nrecords, size_t max_bytes, uint32_t *piece_first, uint64_t *piece_pos,
                           size_t piece_capacity, void *out, size_t capacity_bytes) {
    if (nrecords < 0) return fail(MI355_ERR_INVALID, "nrecords < 0");
    if (frame_bytes >= 0xFFFFFFFFull) return fail(MI355_ERR_INVALID, "frame_bytes must be below 2^32 - 1");
    if (int rc = split_check_limit(max_bytes)) return rc;
    if (nrecords == 0) {
        if (piece_first) piece_first[0] = 0;
        if (piece_pos) piece_pos[0] = 0;
        return MI355_OK;
    }
    if (!cwire || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!piece_first || !piece_pos || !out) return fail(MI355_ERR_INVALID, "null output pointer");
    uint64_t span = 0;
    for (int r = 0; r < nrecords; r++) {
        if (h_escapes[r] > h_counts[r]) return fail(MI355_ERR_INVALID, "frame header: more escapes than entries");
        if (h_counts[r] > frame_bytes) return fail(MI355_ERR_INVALID, "frame header: more entries than frame bytes");
        span += cwire_record_bytes(h_counts[r], h_escapes[r]);
        if (span > cwire_bytes) return fail(MI355_ERR_INVALID, "the records end past cwire_bytes");
    }
    if (int rc = check_regions({input_region(cwire, span)},
                               {Region{piece_first, 4 * ((uint64_t)nrecords + 1), "piece_first"},
                                Region{piece_pos, 8 * ((uint64_t)piece_capacity + 1), "piece_pos"}, Region{out, capacity_bytes, "out"}}))
        return rc;
    const uint8_t *p = (const uint8_t *)cwire;
    uint8_t *dst = (uint8_t *)out;
    const uint32_t M = (uint32_t)max_bytes;
    std::vector<uint32_t> xs, rk;   // per entry: its index, and the 255 codes before it
    uint64_t pos = 0, pieces = 0, at = 0;
    piece_pos[0] = 0;
    for (int r = 0; r < nrecords; r++) {
        const uint32_t n = h_counts[r], e = h_escapes[r];
        const CwireSections<const uint8_t> sec(p, pos, n, e);
        piece_first[r] = (uint32_t)pieces;
        xs.resize(n);
        rk.resize((size_t)n + 1);
        uint32_t X = 0, rank = 0;
        for (uint32_t k = 0; k < n; k++) {
            rk[k] = rank;
            uint32_t g = sec.code[k];
            bool bad = false;
            if (g == 255) {
                if (rank < e) memcpy(&g, sec.esc + 4 * (size_t)rank, 4);
                else bad = true;
                rank++;
            }
            if (!bad) X += g + 1u;
            xs[k] = X - 1u;
        }
        rk[n] = rank;
        for (uint32_t k0 = 0; k0 < n; k0 += kCwsBlock) {
            const uint32_t B = n - k0 < kCwsBlock ? n : k0 + kCwsBlock;
            for (uint32_t a = k0; a < B;) {
                const uint32_t F = xs[a] >= 255u ? 1u : 0u;
                uint32_t cost = 8 + 4 * F, b = a;
                while (b < B) {   // four more entries, or the block's rest
                    const uint32_t nb = B - b < 4 ? B : b + 4, from = b == a ? a + 1 : b;
                    const uint32_t c = 8 + 4 * (rk[nb] - rk[from]);
                    if (cost + c > M) break;
                    cost += c;
                    b = nb;
                }
                const uint32_t len = b - a, E = (cost - 8 - 2 * (uint32_t)cwire_pad4(len)) / 4;
                if (pieces + 1 <= piece_capacity) piece_pos[pieces + 1] = at + cost;
                if (pieces < piece_capacity && at + cost <= capacity_bytes) {
                    uint8_t *q = dst + at;
                    memset(q, 0, cost);
                    memcpy(q, &len, 4);
                    memcpy(q + 4, &E, 4);
                    const CwireSections<uint8_t> o(dst, at, len, E);
                    memcpy(o.code, sec.code + a, len);
                    o.code[0] = (uint8_t)(xs[a] < 255u ? xs[a] : 255u);
                    if (F) memcpy(o.esc, &xs[a], 4);
                    for (uint32_t i = 0; i < E - F; i++) {
                        const uint32_t rr = rk[a + 1] + i;
                        if (rr < e) memcpy(o.esc + 4 * (size_t)(F + i), sec.esc + 4 * (size_t)rr, 4);
                    }
                    memcpy(o.diff, sec.diff + a, len);
                }
                pieces++;
                at += cost;
                a = b;
            }
        }
        pos += cwire_record_bytes(n, e);
    }
    piece_first[nrecords] = (uint32_t)pieces;
    return MI355_OK;
}

int mi355_cwire_split_cwire_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nrecords,
                                  size_t max_bytes, void *d_piece_first, void *d_piece_pos, size_t piece_capacity, void *d_cwire_out,
                                  size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nrecords < 0 || nrecords > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nrecords outside [0, max_batch]");
    if (int rc = split_check_limit(max_bytes)) return rc;
    if (((uintptr_t)d_cwire | (uintptr_t)d_cwire_out | (uintptr_t)d_piece_first) & 3u)
        return fail(MI355_ERR_INVALID, "d_cwire, d_cwire_out and d_piece_first must be 4-byte aligned");
    if ((uintptr_t)d_piece_pos & 7u) return fail(MI355_ERR_INVALID, "d_piece_pos must be 8-byte aligned");
    if (nrecords == 0) return write_empty_heads(c, d_piece_first, d_piece_pos);
    if (!d_cwire || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!d_piece_first || !d_piece_pos || !d_cwire_out) return fail(MI355_ERR_INVALID, "null output pointer");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, nrecords, &tab)) return rc;
    if (int rc = check_regions({input_region(d_cwire, tab.bytes)},
                               {Region{d_piece_first, 4 * ((uint64_t)nrecords + 1), "d_piece_first"},
                                Region{d_piece_pos, 8 * ((uint64_t)piece_capacity + 1), "d_piece_pos"},
                                Region{d_cwire_out, capacity_bytes, "d_cwire_out"}}))
        return rc;
    if (int rc = use_device(c)) return rc;
    const CwaArgs a = cwa_args(c, d_cwire);
    const CwsOut o{(uint32_t *)d_piece_first, (uint64_t *)d_piece_pos, (uint64_t)piece_capacity, (uint8_t *)d_cwire_out,
                   (uint64_t)capacity_bytes};
    HIP_TRY(launch_cwire_split(a, tab.fr.data(), nrecords, (uint32_t)max_bytes, c->cws_blk, c->cws_base, o, c->stream));
    return MI355_OK;
}

// ---- mi355_cwire_runs_*: run-coded records for the link (include/mi355diff.h, "Run-coded records") ---------------------------------
size_t mi355_cwire_runs_frame_bytes(uint32_t n, uint32_t e, uint32_t r) { return (size_t)cwire_runs_bytes(n, e, r); }

size_t mi355_cwire_runs_bytes_max(size_t frame_bytes, int nrecords, int policy) {
    if (nrecords <= 0) return 0;
    if (policy == MI355_RUNS_WHERE_SMALLER) return mi355_cwire_bytes_max(frame_bytes, nrecords);
    if (policy == MI355_RUNS_ALWAYS) return (size_t)nrecords * (size_t)(12 + 3 * cwire_pad4(frame_bytes));
    return 0;
}

static int runs_check_policy(int policy) {
    if (policy != MI355_RUNS_WHERE_SMALLER && policy != MI355_RUNS_ALWAYS) return fail(MI355_ERR_INVALID, "unknown policy");
    return MI355_OK;
}

// The definition of the encoder: a walk over the codes, run by run.
int mi355_cwire_runs_encode_host(size_t frame_bytes, const void *cwire, size_t cwire_bytes, const uint32_t *h_counts,
                                 const uint32_t *h_escapes, int nrecords, int policy, uint32_t *forms, uint64_t *pos, void *out,
                                 size_t capacity_bytes) {
    if (nrecords < 0) return fail(MI355_ERR_INVALID, "nrecords < 0");
    if (frame_bytes >= 0xFFFFFFFFull) return fail(MI355_ERR_INVALID, "frame_bytes must be below 2^32 - 1");
    if (int rc = runs_check_policy(policy)) return rc;
    if (nrecords == 0) {
        if (pos) pos[0] = 0;
        return MI355_OK;
    }
    if (!cwire || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!forms || !pos || !out) return fail(MI355_ERR_INVALID, "null output pointer");
    uint64_t span = 0;
    for (int b = 0; b < nrecords; b++) {
        if (h_escapes[b] > h_counts[b]) return fail(MI355_ERR_INVALID, "frame header: more escapes than entries");
        if (h_counts[b] > frame_bytes) return fail(MI355_ERR_INVALID, "frame header: more entries than frame bytes");
        span += cwire_record_bytes(h_counts[b], h_escapes[b]);
        if (span > cwire_bytes) return fail(MI355_ERR_INVALID, "the records end past cwire_bytes");
    }
    if (int rc = check_regions({input_region(cwire, span)},
                               {Region{forms, 16 * (uint64_t)nrecords, "forms"}, Region{pos, 8 * ((uint64_t)nrecords + 1), "pos"},
                                Region{out, capacity_bytes, "out"}}))
        return rc;
    const uint8_t *p = (const uint8_t *)cwire;
    uint8_t *dst = (uint8_t *)out;
    std::vector<uint8_t> gap, len;
    uint64_t in_pos = 0, at = 0;
    for (int b = 0; b < nrecords; b++) {
        const uint32_t n = h_counts[b], e = h_escapes[b];
        const CwireSections<const uint8_t> sec(p, in_pos, n, e);
        gap.clear();
        len.clear();
        for (uint32_t k = 0; k < n; k++) {
            if (cwire_run_start(k, sec.code[k])) {
                gap.push_back(sec.code[k]);
                len.push_back(0);
            } else {
                len.back()++;
            }
        }
        const uint32_t r = (uint32_t)gap.size();
        const uint32_t form = policy == MI355_RUNS_ALWAYS || cwire_runs_smaller(n, r) ? MI355_RUNS_FORM_RUNS : MI355_RUNS_FORM_COMPACT;
        const uint64_t bytes = cwire_link_bytes(form, n, e, r);
        const uint32_t row[4] = {form, n, e, r};
        memcpy(forms + 4 * (size_t)b, row, sizeof row);
        pos[b] = at;
        if (at + bytes <= capacity_bytes) {   // (a record that does not fit is skipped whole)
            uint8_t *q = dst + at;
            if (form == MI355_RUNS_FORM_COMPACT) {
                memcpy(q, p + in_pos, bytes);
                memcpy(q, row + 1, 8);
            } else {
                memset(q, 0, bytes);
                memcpy(q, row + 1, 12);
                uint8_t *og = q + 12, *ol = og + cwire_pad4(r), *oe = ol + cwire_pad4(r), *od = oe + 4 * (size_t)e;
                if (r) {
                    memcpy(og, gap.data(), r);
                    memcpy(ol, len.data(), r);
                }
                memcpy(oe, sec.esc, 4 * (size_t)e);
                memcpy(od, sec.diff, n);
            }
        }
        at += bytes;
        in_pos += cwire_record_bytes(n, e);
    }
    pos[nrecords] = at;
    return MI355_OK;
}

int mi355_cwire_runs_encode_batch(mi355_core *c, const void *d_cwire_in, const uint32_t *h_counts, const uint32_t *h_escapes, int nrecords,
                                  int policy, void *d_forms, void *d_pos, void *d_out, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nrecords < 0 || nrecords > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nrecords outside [0, max_batch]");
    if (int rc = runs_check_policy(policy)) return rc;
    if (((uintptr_t)d_cwire_in | (uintptr_t)d_out | (uintptr_t)d_forms) & 3u)
        return fail(MI355_ERR_INVALID, "d_cwire_in, d_out and d_forms must be 4-byte aligned");
    if ((uintptr_t)d_pos & 7u) return fail(MI355_ERR_INVALID, "d_pos must be 8-byte aligned");
    if (nrecords == 0) return write_empty_heads(c, nullptr, d_pos);
    if (!d_cwire_in || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!d_forms || !d_pos || !d_out) return fail(MI355_ERR_INVALID, "null output pointer");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, nrecords, &tab)) return rc;
    if (int rc = check_regions({input_region(d_cwire_in, tab.bytes)},
                               {Region{d_forms, 16 * (uint64_t)nrecords, "d_forms"}, Region{d_pos, 8 * ((uint64_t)nrecords + 1), "d_pos"},
                                Region{d_out, capacity_bytes, "d_out"}}))
        return rc;
    if (int rc = use_device(c)) return rc;
    const CwaArgs a = cwa_args(c, d_cwire_in);
    const CwrOut o{(uint32_t *)d_forms, (uint64_t *)d_pos, (uint8_t *)d_out, (uint64_t)capacity_bytes};
    HIP_TRY(launch_cwire_runs_encode(a, tab.fr.data(), nrecords, policy, o, c->stream));
    return MI355_OK;
}

// What both decoders refuse in a row of the forms table
static int runs_check_row(const uint32_t *row, uint64_t frame_bytes) {
    if (row[0] != MI355_RUNS_FORM_COMPACT && row[0] != MI355_RUNS_FORM_RUNS) return fail(MI355_ERR_INVALID, "forms: a form other than 0 or 1");
    if (row[1] > frame_bytes) return fail(MI355_ERR_INVALID, "forms: more entries than frame bytes");
    if (row[2] > row[1]) return fail(MI355_ERR_INVALID, "forms: more escapes than entries");
    if (row[3] > row[1]) return fail(MI355_ERR_INVALID, "forms: more runs than entries");
    return MI355_OK;
}

// The definition of the decoder.  Records before a refused one stay written, with their frame_pos.
int mi355_cwire_runs_decode_host(size_t frame_bytes, const void *in, size_t in_bytes, const uint32_t *h_forms, int nrecords,
                                 uint64_t *frame_pos, void *cwire_out, size_t capacity_bytes) {
    if (nrecords < 0) return fail(MI355_ERR_INVALID, "nrecords < 0");
    if (frame_bytes >= 0xFFFFFFFFull) return fail(MI355_ERR_INVALID, "frame_bytes must be below 2^32 - 1");
    if (nrecords == 0) {
        if (frame_pos) frame_pos[0] = 0;
        return MI355_OK;
    }
    if (!in || !h_forms) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!frame_pos || !cwire_out) return fail(MI355_ERR_INVALID, "null output pointer");
    if (int rc = check_regions({input_region(in, in_bytes), Region{h_forms, 16 * (uint64_t)nrecords, "h_forms"}},
                               {Region{frame_pos, 8 * ((uint64_t)nrecords + 1), "frame_pos"}, Region{cwire_out, capacity_bytes, "cwire_out"}}))
        return rc;
    const uint8_t *p = (const uint8_t *)in;
    uint8_t *dst = (uint8_t *)cwire_out;
    uint64_t in_pos = 0, at = 0;
    frame_pos[0] = 0;
    for (int b = 0; b < nrecords; b++) {
        const uint32_t *row = h_forms + 4 * (size_t)b;
        if (int rc = runs_check_row(row, frame_bytes)) return rc;
        const uint32_t form = row[0], n = row[1], e = row[2], r = row[3];
        const uint64_t in_rec = cwire_link_bytes(form, n, e, r), bytes = cwire_record_bytes(n, e);
        if (in_pos + in_rec > in_bytes) return fail(MI355_ERR_INVALID, "the records end past in_bytes (truncated input)");
        const uint8_t *q = p + in_pos;
        const uint8_t *ig = q + 12, *il = ig + cwire_pad4(r), *ie = il + cwire_pad4(r), *id = ie + 4 * (size_t)e;
        if (form == MI355_RUNS_FORM_RUNS) {
            uint64_t k = 0, n255 = 0;
            for (uint32_t i = 0; i < r; i++) {
                const uint32_t L = il[i] + 1u;
                if ((k & 255u) + L > 256u) return fail(MI355_ERR_INVALID, "a run crosses a multiple of 256 entries");
                k += L;
                n255 += ig[i] == 255;
            }
            if (k != n) return fail(MI355_ERR_INVALID, "the run lengths do not sum to n");
            if (n255 != e) return fail(MI355_ERR_INVALID, "the 255 gaps are not e");
        }
        if (at + bytes <= capacity_bytes) {   // (a record that does not fit is skipped whole)
            uint8_t *o = dst + at;
            if (form == MI355_RUNS_FORM_COMPACT) {
                memcpy(o, q, bytes);
                memcpy(o, row + 1, 8);
            } else {
                memset(o, 0, bytes);
                memcpy(o, row + 1, 8);
                const CwireSections<uint8_t> sec(dst, at, n, e);
                uint64_t k = 0;
                for (uint32_t i = 0; i < r; i++) {
                    sec.code[k] = ig[i];
                    k += il[i] + 1u;
                }
                memcpy(sec.esc, ie, 4 * (size_t)e);
                memcpy(sec.diff, id, n);
            }
        }
        at += bytes;
        in_pos += in_rec;
        frame_pos[b + 1] = at;
    }
    return MI355_OK;
}

int mi355_cwire_runs_decode_batch(mi355_core *c, const void *d_in, const uint32_t *h_forms, int nrecords, void *d_frame_pos,
                                  void *d_cwire_out, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nrecords < 0 || nrecords > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nrecords outside [0, max_batch]");
    if (((uintptr_t)d_in | (uintptr_t)d_cwire_out) & 3u) return fail(MI355_ERR_INVALID, "d_in and d_cwire_out must be 4-byte aligned");
    if ((uintptr_t)d_frame_pos & 7u) return fail(MI355_ERR_INVALID, "d_frame_pos must be 8-byte aligned");
    if (nrecords == 0) return write_empty_heads(c, nullptr, d_frame_pos);
    if (!d_in || !h_forms) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!d_frame_pos || !d_cwire_out) return fail(MI355_ERR_INVALID, "null output pointer");
    std::vector<CwrRecord> recs((size_t)nrecords);
    uint64_t in_pos = 0, at = 0;
    uint32_t cbase = 0;
    for (int b = 0; b < nrecords; b++) {
        const uint32_t *row = h_forms + 4 * (size_t)b;
        if (int rc = runs_check_row(row, c->n)) return rc;
        recs[b] = CwrRecord{in_pos, at, row[0], row[1], row[2], row[3], cbase, cwr_chunks(row[0], row[1], row[3])};
        cbase += recs[b].nc;
        in_pos += cwire_link_bytes(row[0], row[1], row[2], row[3]);
        at += cwire_record_bytes(row[1], row[2]);
    }
    if (int rc = check_regions({input_region(d_in, in_pos)},
                               {frame_pos_region(d_frame_pos, nrecords), Region{d_cwire_out, capacity_bytes, "d_cwire_out"}}))
        return rc;
    if (int rc = use_device(c)) return rc;
    const CwrDecode d{(const uint8_t *)d_in, c->cwr_rtab, c->cwr_chunk, (uint64_t *)d_frame_pos, (uint8_t *)d_cwire_out,
                      (uint64_t)capacity_bytes};
    HIP_TRY(launch_cwire_runs_decode(d, recs.data(), nrecords, at, c->stream));
    return MI355_OK;
}

// ---- mi355_cwire_fec_*: parity blocks over groups of pieces, and their repair (include/mi355diff.h, "Parity pieces") ----------
size_t mi355_cwire_fec_groups_max(size_t piece_capacity, int nrecords, int group) {
    if (group < 1 || group > 255 || nrecords < 0) return 0;
    return piece_capacity / (size_t)group + (size_t)nrecords;
}

static int fec_check_shape(int group, int nparity, size_t pitch) {
    if (group < 1 || group > 255) return fail(MI355_ERR_INVALID, "group outside [1, 255]");
    if (nparity < 1 || nparity > 2) return fail(MI355_ERR_INVALID, "nparity must be 1 or 2");
    if (pitch < 64 || pitch > 65536 || (pitch & 3u)) return fail(MI355_ERR_INVALID, "pitch must be a multiple of 4 in [64, 65536]");
    return MI355_OK;
}

// inputs and outputs of the two forms alike
static int fec_check_regions(const void *pieces, size_t pieces_bytes, const void *piece_first, const void *piece_pos, size_t piece_capacity,
                             int nrecords, int nparity, const void *fec_first, const void *fec_len, size_t group_capacity, const void *out,
                             size_t capacity_bytes) {
    (void)nparity;
    return check_regions({Region{pieces, pieces_bytes, "the pieces"}, Region{piece_first, 4 * ((uint64_t)nrecords + 1), "piece_first"},
                          Region{piece_pos, 8 * ((uint64_t)piece_capacity + 1), "piece_pos"}},
                         {Region{fec_first, 4 * ((uint64_t)nrecords + 1), "fec_first"}, nowhere(Region{fec_len, 4 * (uint64_t)group_capacity, "fec_len"}),
                          nowhere(Region{out, capacity_bytes, "the parity blocks"})},
                         true);
}

// The definition.  The group and member arithmetic is cwire_common.h's, shared with the kernel.
int mi355_cwire_fec_host(const void *pieces, size_t pieces_bytes, const uint32_t *piece_first, const uint64_t *piece_pos,
                         size_t piece_capacity, int nrecords, int group, int nparity, size_t pitch, uint32_t *fec_first, uint32_t *fec_len,
                         size_t group_capacity, void *out, size_t capacity_bytes) {
    if (nrecords < 0) return fail(MI355_ERR_INVALID, "nrecords < 0");
    if (int rc = fec_check_shape(group, nparity, pitch)) return rc;
    if (nrecords == 0) {
        if (fec_first) fec_first[0] = 0;
        return MI355_OK;
    }
    if (!pieces || !piece_first || !piece_pos || !fec_first || !fec_len || !out) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = fec_check_regions(pieces, pieces_bytes, piece_first, piece_pos, piece_capacity, nrecords, nparity, fec_first, fec_len,
                                   group_capacity, out, capacity_bytes))
        return rc;
    const uint32_t G = (uint32_t)group, K = (uint32_t)nparity;
    uint32_t groups = 0;
    for (int r = 0; r < nrecords; r++) {
        const uint32_t c = piece_first[r + 1] - piece_first[r];
        fec_first[r] = groups;
        groups += c / G + (c % G ? 1u : 0u);
    }
    fec_first[nrecords] = groups;
    const uint8_t *src = (const uint8_t *)pieces;
    std::vector<uint32_t> P, Q;
    for (uint32_t g = 0; g < groups && g < group_capacity; g++) {
        const FecGroup fg = fec_group(fec_first, piece_first, nrecords, G, g);
        uint32_t L = 0;
        bool bad = fg.m == 0;
        for (uint32_t i = 0; i < fg.m; i++) {
            const uint32_t len = fec_member_len(piece_pos, piece_capacity, pieces_bytes, (uint32_t)pitch, fg.p0 + i);
            bad |= len == 0;
            L = len > L ? len : L;
        }
        if (bad) L = 0;
        fec_len[g] = L;
        const uint64_t slot = (uint64_t)g * K * pitch;
        if (L == 0 || slot + (uint64_t)K * pitch > capacity_bytes) continue;
        P.assign(L / 4, 0u);
        Q.assign(L / 4, 0u);
        for (uint32_t i = fg.m; i > 0; i--) {   // Horner, from the last slot down
            const uint64_t at = piece_pos[fg.p0 + i - 1];
            const uint32_t len = (uint32_t)(piece_pos[fg.p0 + i] - at);
            for (uint32_t w = 0; w < L / 4; w++) {
                uint32_t v = 0;
                if (4 * w < len) memcpy(&v, src + at + 4 * (size_t)w, 4);
                P[w] ^= v;
                Q[w] = fec_xtime(Q[w]) ^ v;
            }
        }
        memcpy((uint8_t *)out + slot, P.data(), L);
        if (K == 2) memcpy((uint8_t *)out + slot + pitch, Q.data(), L);
    }
    return MI355_OK;
}

int mi355_cwire_fec_batch(mi355_core *c, const void *d_pieces, size_t pieces_bytes, const void *d_piece_first, const void *d_piece_pos,
                          size_t piece_capacity, int nrecords, int group, int nparity, size_t pitch, void *d_fec_first, void *d_fec_len,
                          size_t group_capacity, void *d_out, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nrecords < 0 || nrecords > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nrecords outside [0, max_batch]");
    if (int rc = fec_check_shape(group, nparity, pitch)) return rc;
    if (((uintptr_t)d_pieces | (uintptr_t)d_piece_first | (uintptr_t)d_fec_first | (uintptr_t)d_fec_len | (uintptr_t)d_out) & 3u)
        return fail(MI355_ERR_INVALID, "d_pieces, d_piece_first, d_fec_first, d_fec_len and d_out must be 4-byte aligned");
    if ((uintptr_t)d_piece_pos & 7u) return fail(MI355_ERR_INVALID, "d_piece_pos must be 8-byte aligned");
    if (nrecords == 0) return write_empty_heads(c, d_fec_first, nullptr);
    if (!d_pieces || !d_piece_first || !d_piece_pos || !d_fec_first || !d_fec_len || !d_out) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = fec_check_regions(d_pieces, pieces_bytes, d_piece_first, d_piece_pos, piece_capacity, nrecords, nparity, d_fec_first,
                                   d_fec_len, group_capacity, d_out, capacity_bytes))
        return rc;
    if (int rc = use_device(c)) return rc;
    const FecArgs a{(const uint32_t *)d_pieces, (uint64_t)pieces_bytes, (const uint32_t *)d_piece_first, (const uint64_t *)d_piece_pos,
                    (uint64_t)piece_capacity, nrecords, (uint32_t)group, (uint32_t)nparity, (uint32_t)pitch, (uint32_t *)d_fec_first,
                    (uint32_t *)d_fec_len, (uint64_t)group_capacity, (uint32_t *)d_out, (uint64_t)capacity_bytes};
    HIP_TRY(launch_cwire_fec(a, c->cu_count * 8u, c->stream));   // eight waves per SIMD
    return MI355_OK;
}

namespace {
// GF(2^8) modulo 0x11D on one byte, through the packed forms of cwire_common.h
uint32_t gf_pow2(uint32_t i) {
    uint32_t v = 1;
    while (i--) v = fec_xtime(v) & 255u;
    return v;
}
uint32_t gf_inv(uint32_t c) {
    for (uint32_t x = 1; x < 256; x++)
        if ((fec_mul(x, c) & 255u) == 1u) return x;
    return 0;
}

// What one job asks for, refused or turned into the kernel's mode and constants (FecRepairJob).  present(i, from): slot i survives.
struct FecPlan {
    uint32_t mode, c1, c2, a, b, lost;
};
typedef bool (*FecPresent)(int i, const void *from);
int fec_plan(int members, FecPresent present_fn, const void *from, const uint32_t *slot_len, bool have_p, bool have_q, uint32_t fec_len, FecPlan *pl) {
    if (members < 1 || members > 255) return fail(MI355_ERR_INVALID, "members outside [1, 255]");
    if (fec_len == 0 || (fec_len & 3u)) return fail(MI355_ERR_INVALID, "fec_len must be a positive multiple of 4");
    if (!slot_len) return fail(MI355_ERR_INVALID, "null argument");
    uint32_t lost[2] = {0, 0}, u = 0;
    for (int i = 0; i < members; i++) {
        if (!present_fn(i, from)) {
            if (u < 2) lost[u] = (uint32_t)i;
            u++;
        } else if (slot_len[i] == 0 || (slot_len[i] & 3u) || slot_len[i] > fec_len)
            return fail(MI355_ERR_INVALID, "a surviving length must be a positive multiple of 4 and at most fec_len");
    }
    if (u > (have_p ? 1u : 0u) + (have_q ? 1u : 0u)) return fail(MI355_ERR_INVALID, "more slots lost than parity blocks present");
    pl->lost = u;
    pl->a = lost[0];
    pl->b = lost[1];
    pl->c1 = pl->c2 = 0;
    if (u == 0) pl->mode = 0;
    else if (u == 1 && have_p) pl->mode = 1;
    else if (u == 1) {
        pl->mode = 2;
        pl->c2 = gf_inv(gf_pow2(lost[0]));
    } else {
        pl->mode = 3;
        pl->c1 = gf_pow2(lost[0]);
        pl->c2 = gf_inv(gf_pow2(lost[0]) ^ gf_pow2(lost[1]));
    }
    return MI355_OK;
}
}  // namespace

// The definition of the repair: the formulas of the header, word by word.
int mi355_cwire_fec_repair_host(int members, const void *const *slot, const uint32_t *slot_len, const void *p, const void *q,
                                uint32_t fec_len, void *out0, void *out1, uint32_t verdict[2]) {
    if (!slot) return fail(MI355_ERR_INVALID, "null argument");
    FecPlan pl;
    if (int rc = fec_plan(members, [](int i, const void *from) { return ((const void *const *)from)[i] != nullptr; }, slot, slot_len, p != nullptr, q != nullptr, fec_len, &pl)) return rc;
    if (pl.lost >= 1 && (!out0 || !verdict)) return fail(MI355_ERR_INVALID, "null output");
    if (pl.lost == 2 && !out1) return fail(MI355_ERR_INVALID, "null output");
    if (verdict) verdict[0] = verdict[1] = 0;
    if (pl.lost == 0) return MI355_OK;
    const uint32_t nw = fec_len / 4;
    std::vector<uint32_t> d[2];
    d[0].assign(nw, 0u);
    d[1].assign(nw, 0u);
    for (uint32_t w = 0; w < nw; w++) {
        uint32_t P = 0, Q = 0, qs = 0;
        if (p) memcpy(&P, (const uint8_t *)p + 4 * (size_t)w, 4);
        if (q) memcpy(&Q, (const uint8_t *)q + 4 * (size_t)w, 4);
        for (int i = members; i > 0; i--) {
            uint32_t v = 0;
            if (slot[i - 1] && 4 * w < slot_len[i - 1]) memcpy(&v, (const uint8_t *)slot[i - 1] + 4 * (size_t)w, 4);
            P ^= v;
            qs = fec_xtime(qs) ^ v;
        }
        Q ^= qs;   // P, Q: Pxy and Qxy of the header
        if (pl.mode == 1) d[0][w] = P;
        else if (pl.mode == 2) d[0][w] = fec_mul(Q, pl.c2);
        else {
            d[1][w] = fec_mul(Q ^ fec_mul(P, pl.c1), pl.c2);
            d[0][w] = P ^ d[1][w];
        }
    }
    for (uint32_t k = 0; k < pl.lost; k++) {
        memcpy(k ? out1 : out0, d[k].data(), fec_len);
        uint64_t tail = fec_len;
        verdict[k] = nw >= 2 ? fec_header_verdict(d[k][0], d[k][1], fec_len, &tail) : (uint32_t)MI355_FEC_BAD_HEADER;
        for (uint32_t w = (uint32_t)(tail / 4); w < nw; w++)
            if (d[k][w]) verdict[k] |= MI355_FEC_BAD_TAIL;
    }
    return MI355_OK;
}

int mi355_cwire_fec_repair_batch(mi355_core *c, const void *d_rx, size_t rx_bytes, int njobs, const uint32_t *h_job_first,
                                 const uint64_t *h_slot_off, const uint32_t *h_slot_len, const uint64_t *h_parity_off,
                                 const uint32_t *h_fec_len, void *d_out, size_t pitch, void *d_verdict) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (njobs < 0 || njobs > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "njobs outside [0, max_batch]");
    if (njobs == 0) return MI355_OK;
    if (!d_rx || !h_job_first || !h_slot_off || !h_slot_len || !h_parity_off || !h_fec_len || !d_out || !d_verdict)
        return fail(MI355_ERR_INVALID, "null argument");
    if (((uintptr_t)d_rx | (uintptr_t)d_out | (uintptr_t)d_verdict | pitch) & 3u)
        return fail(MI355_ERR_INVALID, "d_rx, d_out, d_verdict and pitch must be multiples of 4");
    if (int rc = check_regions({Region{d_rx, rx_bytes, "d_rx"}},
                               {Region{d_out, 2 * (uint64_t)njobs * pitch, "d_out"}, Region{d_verdict, 8 * (uint64_t)njobs, "d_verdict"}}, true))
        return rc;
    auto block_ok = [&](uint64_t off, uint64_t len) { return !(off & 3u) && off <= rx_bytes && len <= rx_bytes - off; };
    std::vector<FecPlan> plan((size_t)njobs);
    for (int j = 0; j < njobs; j++) {   // everything is refused before anything is launched
        if (h_job_first[j + 1] < h_job_first[j]) return fail(MI355_ERR_INVALID, "h_job_first must not decrease");
        const uint32_t s0 = h_job_first[j];
        const int64_t members = (int64_t)h_job_first[j + 1] - s0;
        const uint64_t po = h_parity_off[2 * (size_t)j], qo = h_parity_off[2 * (size_t)j + 1];
        if (int rc = fec_plan(members > 255 ? 256 : (int)members, [](int i, const void *from) { return ((const uint64_t *)from)[i] != MI355_FEC_ABSENT; },
                              h_slot_off + s0, h_slot_len + s0,
                              po != MI355_FEC_ABSENT, qo != MI355_FEC_ABSENT, h_fec_len[j], &plan[(size_t)j]))
            return rc;
        if (h_fec_len[j] > pitch) return fail(MI355_ERR_INVALID, "h_fec_len above pitch");
        for (int i = 0; i < (int)members; i++)
            if (h_slot_off[s0 + i] != MI355_FEC_ABSENT && !block_ok(h_slot_off[s0 + i], h_slot_len[s0 + i]))
                return fail(MI355_ERR_INVALID, "a slot misaligned or past rx_bytes");
        if ((po != MI355_FEC_ABSENT && !block_ok(po, h_fec_len[j])) || (qo != MI355_FEC_ABSENT && !block_ok(qo, h_fec_len[j])))
            return fail(MI355_ERR_INVALID, "a parity block misaligned or past rx_bytes");
    }
    if (int rc = use_device(c)) return rc;
    FecRepairArgs h{};
    int nj = 0;
    uint32_t ns = 0;
    auto flush = [&]() -> hipError_t {
        const hipError_t e = launch_cwire_fec_repair((const uint8_t *)d_rx, h, nj, (uint8_t *)d_out, pitch, (uint32_t *)d_verdict, c->stream);
        nj = 0;
        ns = 0;
        return e;
    };
    for (int j = 0; j < njobs; j++) {
        const uint32_t s0 = h_job_first[j], members = h_job_first[j + 1] - s0;
        if (nj == kFecRepairJobs || ns + members > (uint32_t)kFecRepairSlots) HIP_TRY(flush());
        const FecPlan &pl = plan[(size_t)j];
        h.job[nj] = FecRepairJob{h_parity_off[2 * (size_t)j], h_parity_off[2 * (size_t)j + 1], ns, members, h_fec_len[j], pl.mode, pl.c1, pl.c2,
                                 (uint32_t)j};
        for (uint32_t i = 0; i < members; i++) {
            h.off[ns + i] = h_slot_off[s0 + i];
            h.len[ns + i] = h_slot_len[s0 + i];
        }
        ns += members;
        nj++;
    }
    HIP_TRY(flush());
    return MI355_OK;
}

// ---- resynchronising a receiver: tile digests, refresh records, tile clears (stream_ops.hip, k_state_digest, k_rf_*) ----------
size_t mi355_state_tiles(size_t frame_bytes) { return frame_bytes / kCwaTile + (frame_bytes % kCwaTile ? 1 : 0); }

// The definition of the digest; the device forms compute the same two words per tile.
int mi355_state_digest_host(const uint8_t *state, size_t frame_bytes, uint32_t *digests) {
    if (frame_bytes && (!state || !digests)) return fail(MI355_ERR_INVALID, "null argument");
    const size_t tiles = mi355_state_tiles(frame_bytes);
    for (size_t t = 0; t < tiles; t++) {
        const size_t lo = t * kCwaTile, len = frame_bytes - lo < kCwaTile ? frame_bytes - lo : kCwaTile;
        uint32_t sum = 0, mix = 0;
        for (uint32_t i = 0; i < kCwaTile / 4; i++) {
            uint32_t w = 0;   // little-endian, the bytes past the tile's end zero
            for (uint32_t j = 0; j < 4 && 4 * (size_t)i + j < len; j++) w |= (uint32_t)state[lo + 4 * i + j] << (8 * j);
            uint32_t v = w ^ (0x9E3779B9u * (i + 1u));
            v ^= v >> 16;
            v *= 0x85EBCA6Bu;
            v ^= v >> 13;
            v *= 0xC2B2AE35u;
            v ^= v >> 16;
            sum += w;
            mix += v;
        }
        const uint32_t d[2] = {sum, mix};
        memcpy((uint8_t *)digests + 8 * t, d, 8);   // (no alignment asked of digests)
    }
    return MI355_OK;
}

// In these calls and in the wall's an empty region overlaps nothing, wherever it lies: every region goes through nowhere().
// The states of zero-byte frames are empty whatever the stride.
static Region resync_states(const mi355_core *c, const void *d_states, size_t stride, int nstreams) {
    return c->n ? states_region(c, d_states, stride, nstreams) : Region{nullptr, 0, "the states"};
}

int mi355_state_digest_batch(mi355_core *c, const void *d_states, size_t stride_bytes, int nstreams, void *d_digests) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nstreams > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams outside [0, max_batch]");
    if (nstreams == 0) return MI355_OK;
    if (!d_states || !d_digests) return fail(MI355_ERR_INVALID, "null argument");
    if (stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if ((uintptr_t)d_digests & 3u) return fail(MI355_ERR_INVALID, "d_digests must be 4-byte aligned");
    if (int rc = check_regions({resync_states(c, d_states, stride_bytes, nstreams)},
                               {nowhere(Region{d_digests, 8 * (uint64_t)nstreams * cwa_tiles(c->n), "d_digests"})}))
        return rc;
    if (int rc = use_device(c)) return rc;
    HIP_TRY(launch_state_digest((const uint8_t *)d_states, stride_bytes, c->n, nstreams, (uint32_t *)d_digests, c->stream));
    return MI355_OK;
}

int mi355_refresh_cwire_batch(mi355_core *c, const void *d_states, size_t stride_bytes, int nstreams, const void *d_peer_digests,
                              void *d_tile_mask, void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nstreams > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams outside [0, max_batch]");
    if (((uintptr_t)d_peer_digests & 3u) || ((uintptr_t)d_tile_mask & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_cwire_out & 3u))
        return fail(MI355_ERR_INVALID, "d_peer_digests, d_tile_mask, d_offsets and d_cwire_out must be 4-byte aligned");
    if ((uintptr_t)d_frame_pos & 7u) return fail(MI355_ERR_INVALID, "d_frame_pos must be 8-byte aligned");
    if (nstreams == 0) return write_empty_heads(c, d_offsets, d_frame_pos);
    if (!d_states) return fail(MI355_ERR_INVALID, "null d_states");
    if (!d_tile_mask || !d_offsets || !d_frame_pos || !d_cwire_out) return fail(MI355_ERR_INVALID, "null output pointer");
    if (stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if (int rc = check_regions({resync_states(c, d_states, stride_bytes, nstreams),
                                d_peer_digests ? nowhere(Region{d_peer_digests, 8 * (uint64_t)nstreams * cwa_tiles(c->n), "the peer digests"}) : Region{}},
                               {nowhere(tile_mask_region(c, d_tile_mask, nstreams)), offsets_region(d_offsets, nstreams),
                                frame_pos_region(d_frame_pos, nstreams), nowhere(Region{d_cwire_out, capacity_bytes, "d_cwire_out"})},
                               true))
        return rc;
    if (int rc = use_device(c)) return rc;
    CwaArgs a = cwa_args(c, nullptr);   // (chunk: one fact word per (stream, tile), nstreams <= max_batch)
    a.state = (uint8_t *)d_states;      // (only read)
    a.stride = stride_bytes;
    HIP_TRY(launch_refresh(a, nstreams, (const uint32_t *)d_peer_digests, (uint32_t *)d_tile_mask,
                           Produced::records(d_offsets, d_frame_pos, d_cwire_out, capacity_bytes), c->stream));
    return MI355_OK;
}

int mi355_state_clear_tiles_batch(mi355_core *c, void *d_states, size_t stride_bytes, int nstreams, const void *d_tile_mask) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nstreams > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams outside [0, max_batch]");
    if (nstreams == 0) return MI355_OK;
    if (!d_states || !d_tile_mask) return fail(MI355_ERR_INVALID, "null argument");
    if (stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if ((uintptr_t)d_tile_mask & 3u) return fail(MI355_ERR_INVALID, "d_tile_mask must be 4-byte aligned");
    if (int rc = check_regions({resync_states(c, d_states, stride_bytes, nstreams)}, {nowhere(tile_mask_region(c, d_tile_mask, nstreams))}))
        return rc;
    if (int rc = use_device(c)) return rc;
    HIP_TRY(launch_state_clear_tiles((uint8_t *)d_states, stride_bytes, c->n, nstreams, (const uint32_t *)d_tile_mask, c->stream));
    return MI355_OK;
}

// ---- a wall of many cameras: thumbnails of the states in one frame, touched-tile masks (stream_ops.hip, k_wall_compose) -------
size_t mi355_wall_thumb_size(int width, int height, int k, int *tw, int *th) {
    const bool ok = width >= 1 && height >= 1 && k >= 1 && k <= 16;
    const int w = ok ? (int)(((int64_t)width + k - 1) / k) : 0, h = ok ? (int)(((int64_t)height + k - 1) / k) : 0;
    if (tw) *tw = w;
    if (th) *th = h;
    return (size_t)w * (size_t)h;
}

int mi355_wall_compose_batch(mi355_core *c, const void *d_states, size_t stride_bytes, int nstreams, const int32_t *h_place,
                             const void *d_tile_mask, void *d_wall, int wall_w, int wall_h, size_t wall_pitch) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nstreams > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams outside [0, max_batch]");
    if (nstreams == 0) return MI355_OK;
    if (!d_states || !h_place || !d_wall) return fail(MI355_ERR_INVALID, "null argument");
    if (stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if (wall_w < 1 || wall_h < 1) return fail(MI355_ERR_INVALID, "wall_w or wall_h < 1");
    if (wall_pitch < 3 * (size_t)wall_w) return fail(MI355_ERR_INVALID, "wall_pitch < 3 * wall_w");
    if ((uintptr_t)d_tile_mask & 3u) return fail(MI355_ERR_INVALID, "d_tile_mask must be 4-byte aligned");
    for (int s = 0; s < nstreams; s++) {
        const int32_t x = h_place[3 * s], y = h_place[3 * s + 1], k = h_place[3 * s + 2];
        if (k < 0 || k > 16) return fail(MI355_ERR_INVALID, "h_place: a scale outside [0, 16]");
        if (k == 0) continue;
        int tw, th;
        mi355_wall_thumb_size(c->cfg.width, c->cfg.height, k, &tw, &th);
        if (x < 0 || y < 0 || (int64_t)x + tw > wall_w || (int64_t)y + th > wall_h)
            return fail(MI355_ERR_INVALID, "h_place: a thumbnail does not lie inside the wall");
    }
    const Region st = resync_states(c, d_states, stride_bytes, nstreams);
    const Region wl{d_wall, (uint64_t)(wall_h - 1) * wall_pitch + 3 * (uint64_t)wall_w, "the wall"};
    const Region mk = d_tile_mask ? nowhere(tile_mask_region(c, d_tile_mask, nstreams)) : Region{nullptr, 0, "d_tile_mask"};
    if (overlap(wl, st)) return overlap_fail(wl, st);
    if (overlap(mk, st)) return overlap_fail(mk, st);
    if (overlap(wl, mk)) return overlap_fail(wl, mk);
    if (int rc = use_device(c)) return rc;
    HIP_TRY(launch_wall_compose((const uint8_t *)d_states, stride_bytes, (uint32_t)c->cfg.width, (uint32_t)c->cfg.height, nstreams, h_place,
                                (const uint32_t *)d_tile_mask, (uint8_t *)d_wall, wall_pitch, c->stream));
    return MI355_OK;
}

int mi355_cwire_touched_tiles_batch(mi355_core *c, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams,
                                    int nframes, int accumulate, void *d_tile_mask) {
    int B;
    if (int rc = burst_count(c, nstreams, nframes, &B)) return rc;
    if (((uintptr_t)d_cwire | (uintptr_t)d_tile_mask) & 3u) return fail(MI355_ERR_INVALID, "the device pointers must be 4-byte aligned");
    if (B == 0) return MI355_OK;
    if (!d_cwire || !h_counts || !h_escapes) return fail(MI355_ERR_INVALID, "null stream pointer");
    if (!d_tile_mask) return fail(MI355_ERR_INVALID, "null output pointer");
    CwaTable tab;
    if (int rc = cwa_table(c, h_counts, h_escapes, B, &tab)) return rc;
    if (int rc = check_regions({input_region(d_cwire, tab.bytes)}, {nowhere(tile_mask_region(c, d_tile_mask, nstreams))})) return rc;
    if (int rc = use_device(c)) return rc;
    const CwaArgs a = cwa_args(c, d_cwire);
    HIP_TRY(launch_cwire_touched(a, tab.fr.data(), nstreams, nframes, accumulate != 0, (uint32_t *)d_tile_mask, c->stream));
    return MI355_OK;
}

// ---- records of the thumbnails: a low-resolution viewer served from full-size states (stream_ops.hip, k_thumb_facts) ----------
// The host form is the definition: exactly the required pixels, two passes over them (the sizes, then the record), the box
// average recomputed in the second.
extern "C++" {
namespace {
struct ThumbHost {
    const uint8_t *state;
    const uint32_t *mask;
    int64_t w, h, k, tw, th;
    bool required(int64_t u, int64_t v) const {
        if (!mask) return true;
        const int64_t x0 = u * k, x1 = std::min(w, x0 + k);
        for (int64_t y = v * k; y < std::min(h, (v + 1) * k); y++)
            for (int64_t t = 3 * (y * w + x0) / kCwaTile; t <= (3 * (y * w + x1) - 1) / kCwaTile; t++) {
                uint32_t word;
                memcpy(&word, (const uint8_t *)mask + 4 * (t >> 5), 4);   // (no alignment asked of the mask)
                if ((word >> (t & 31)) & 1u) return true;
            }
        return false;
    }
    void pixel(int64_t u, int64_t v, uint8_t bgr[3]) const {
        const int64_t x0 = u * k, x1 = std::min(w, x0 + k), y0 = v * k, y1 = std::min(h, y0 + k), a = (x1 - x0) * (y1 - y0);
        int64_t sum[3] = {0, 0, 0};
        for (int64_t y = y0; y < y1; y++)
            for (int64_t x = x0; x < x1; x++)
                for (int c = 0; c < 3; c++) sum[c] += state[3 * (y * w + x) + c];
        for (int c = 0; c < 3; c++) bgr[c] = (uint8_t)((sum[c] + a / 2) / a);
    }
    // op(j, new byte, held byte) for every byte of a required pixel whose difference is above the threshold, j ascending
    template <class Op>
    void walk(const uint8_t *thumb, int threshold, Op op) const {
        for (int64_t v = 0; v < th; v++)
            for (int64_t u = 0; u < tw; u++) {
                if (!required(u, v)) continue;
                uint8_t bgr[3];
                pixel(u, v, bgr);
                for (int c = 0; c < 3; c++) {
                    const int64_t j = 3 * (v * tw + u) + c;
                    if (std::abs((int)bgr[c] - (int)thumb[j]) > threshold) op((uint32_t)j, bgr[c], thumb[j]);
                }
            }
    }
};
}  // namespace
}  // extern "C++"

int mi355_thumb_cwire_host(const uint8_t *state, int width, int height, int k, int threshold, const uint32_t *tile_mask, uint8_t *thumb,
                           void *out, size_t capacity_bytes, uint32_t *n, uint32_t *e, size_t *bytes) {
    if (width < 1 || height < 1) return fail(MI355_ERR_INVALID, "width or height < 1");
    if (3 * (int64_t)width * height >= (int64_t)1 << 31) return fail(MI355_ERR_INVALID, "3 * width * height >= 2^31");
    if (k < 1 || k > 16) return fail(MI355_ERR_INVALID, "k outside 1 .. 16");
    if (threshold < 0 || threshold > 255) return fail(MI355_ERR_INVALID, "threshold outside 0 .. 255");
    if (!state || !thumb || !n || !e || !bytes) return fail(MI355_ERR_INVALID, "null argument");
    if (!out && capacity_bytes) return fail(MI355_ERR_INVALID, "null out with capacity_bytes > 0");
    ThumbHost t{state, tile_mask, width, height, k, (width + k - 1) / k, (height + k - 1) / k};
    uint32_t cn = 0, ce = 0, end = 0;
    t.walk(thumb, threshold, [&](uint32_t j, uint8_t, uint8_t) {
        ce += j - end >= 255u;
        end = j + 1u;
        cn++;
    });
    const size_t need = (size_t)cwire_record_bytes(cn, ce);
    *n = cn;
    *e = ce;
    *bytes = need;
    if (need > capacity_bytes) return MI355_OK;   // exact sizes, nothing written: the caller repeats with more room
    const uint32_t head[2] = {cn, ce};
    memcpy(out, head, 8);   // (no alignment asked of out)
    const CwireSections<uint8_t> sec((uint8_t *)out, 0, cn, ce);
    for (uint32_t i = cn; i < (uint32_t)cwire_pad4(cn); i++) sec.code[i] = sec.diff[i] = 0;
    uint32_t i = 0, r = 0;
    end = 0;
    t.walk(thumb, threshold, [&](uint32_t j, uint8_t nw, uint8_t held) {
        const uint32_t g = j - end;
        sec.code[i] = (uint8_t)(g < 255u ? g : 255u);
        if (g >= 255u) {
            memcpy(sec.esc + 4 * (size_t)r++, &g, 4);
        }
        sec.diff[i++] = (uint8_t)(nw - held);
        thumb[j] = nw;   // (behind the walk's read of this byte; no later byte depends on it)
        end = j + 1u;
    });
    return MI355_OK;
}

int mi355_thumb_cwire_batch(mi355_core *c, const void *d_states, size_t state_spacing_bytes, int nstreams, int k, int threshold,
                            const void *d_tile_mask, void *d_thumbs, size_t thumb_spacing_bytes, void *d_offsets, void *d_frame_pos,
                            void *d_cwire_out, size_t capacity_bytes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nstreams < 0 || nstreams > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nstreams outside [0, max_batch]");
    if (k < 1 || k > 16) return fail(MI355_ERR_INVALID, "k outside 1 .. 16");
    if (threshold < 0 || threshold > 255) return fail(MI355_ERR_INVALID, "threshold outside 0 .. 255");
    if (((uintptr_t)d_tile_mask & 3u) || ((uintptr_t)d_offsets & 3u) || ((uintptr_t)d_cwire_out & 3u))
        return fail(MI355_ERR_INVALID, "d_tile_mask, d_offsets and d_cwire_out must be 4-byte aligned");
    if ((uintptr_t)d_frame_pos & 7u) return fail(MI355_ERR_INVALID, "d_frame_pos must be 8-byte aligned");
    if (nstreams == 0) return write_empty_heads(c, d_offsets, d_frame_pos);
    if (!d_states || !d_thumbs) return fail(MI355_ERR_INVALID, "null d_states or d_thumbs");
    if (!d_offsets || !d_frame_pos || !d_cwire_out) return fail(MI355_ERR_INVALID, "null output pointer");
    int tw, th;
    const uint64_t thumb_bytes = 3 * (uint64_t)mi355_wall_thumb_size(c->cfg.width, c->cfg.height, k, &tw, &th);
    if (state_spacing_bytes < c->n) return fail(MI355_ERR_INVALID, "state_spacing_bytes < frame bytes");
    if (thumb_spacing_bytes < thumb_bytes) return fail(MI355_ERR_INVALID, "thumb_spacing_bytes < thumbnail bytes");
    const Region st = resync_states(c, d_states, state_spacing_bytes, nstreams);
    const Region mk = d_tile_mask ? nowhere(tile_mask_region(c, d_tile_mask, nstreams)) : Region{nullptr, 0, "d_tile_mask"};
    if (overlap(mk, st)) return overlap_fail(mk, st);
    if (int rc = check_regions({st, mk},
                               {nowhere(Region{d_thumbs, thumb_bytes ? (uint64_t)(nstreams - 1) * thumb_spacing_bytes + thumb_bytes : 0,
                                               "the thumbnails"}),
                                offsets_region(d_offsets, nstreams), frame_pos_region(d_frame_pos, nstreams),
                                nowhere(Region{d_cwire_out, capacity_bytes, "d_cwire_out"})},
                               true))
        return rc;
    if (int rc = use_device(c)) return rc;
    CwaArgs a = cwa_args(c, nullptr);   // (chunk: one fact word per (stream, thumbnail tile), no more than the states' tiles)
    a.state = (uint8_t *)d_states;      // (only read)
    a.stride = state_spacing_bytes;
    HIP_TRY(launch_thumb_cwire(a, nstreams, (uint32_t)c->cfg.width, (uint32_t)c->cfg.height, (uint32_t)k, (uint32_t)threshold,
                               (const uint32_t *)d_tile_mask, (uint8_t *)d_thumbs, thumb_spacing_bytes,
                               Produced::records(d_offsets, d_frame_pos, d_cwire_out, capacity_bytes), c->stream));
    return MI355_OK;
}

int mi355_int_diff(mi355_core *c, const void *d_cur, const void *d_prev, void *d_out, size_t n) {
    if (!c || (n && (!d_cur || !d_prev || !d_out))) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device_filter(c)) return rc;
    HIP_TRY(launch_int_diff((const int32_t *)d_cur, (const int32_t *)d_prev, (int32_t *)d_out, n, c->stream));
    return MI355_OK;
}

int mi355_gray_avg(mi355_core *c, const void *d_in, void *d_out) {
    if (!c || (c->n && (!d_in || !d_out))) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device_filter(c)) return rc;
    HIP_TRY(launch_gray((const uint8_t *)d_in, (uint8_t *)d_out, c->n / 3, false, FrameBatch{c->n, 1}, c->stream));
    return MI355_OK;
}

int mi355_gray_weighted(mi355_core *c, const void *d_in, void *d_out) {
    if (!c || (c->n && (!d_in || !d_out))) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device_filter(c)) return rc;
    HIP_TRY(launch_gray((const uint8_t *)d_in, (uint8_t *)d_out, c->n / 3, true, FrameBatch{c->n, 1}, c->stream));
    return MI355_OK;
}

int mi355_binarize_chain(mi355_core *c, const void *d_gray, void *d_out, void *d_hist, void *d_thr) {
    if (!c || (c->n && (!d_gray || !d_out))) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device_filter(c)) return rc;
    int32_t *hist = d_hist ? (int32_t *)d_hist : c->hist;
    int32_t *thr = d_thr ? (int32_t *)d_thr : c->thr;
    HIP_TRY(launch_binarize_chain((const uint8_t *)d_gray, (uint8_t *)d_out, c->n, hist, thr, FrameBatch{c->n, 1}, c->stream));
    return MI355_OK;
}

int mi355_heat_map(mi355_core *c, const void *d_cur, const void *d_prev, void *d_out) {
    if (!c || (c->n && (!d_cur || !d_prev || !d_out))) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device_filter(c)) return rc;
    HIP_TRY(launch_heat_map((const uint8_t *)d_cur, (const uint8_t *)d_prev, (uint8_t *)d_out, c->n / 3,
                            c->lut, FrameBatch{c->n, 1}, c->stream));
    return MI355_OK;
}

int mi355_red_dense(mi355_core *c, const void *d_cur, const void *d_prev, void *d_out) {
    if (!c || (c->n && (!d_cur || !d_prev || !d_out))) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device_filter(c)) return rc;
    HIP_TRY(launch_red_dense((const uint8_t *)d_cur, (const uint8_t *)d_prev, (uint8_t *)d_out, c->n / 3,
                             c->cfg.threshold, FrameBatch{c->n, 1}, c->stream));
    return MI355_OK;
}

int mi355_red_overlap(mi355_core *c, void *d_img, const void *d_xs, const void *d_count, uint32_t count) {
    if (!c || !d_img || ((d_count || count) && !d_xs)) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(launch_red_overlap((uint8_t *)d_img, (const int32_t *)d_xs, (const uint32_t *)d_count, count,
                               c->n, c->stream));
    return MI355_OK;
}

int mi355_red_stream_batch(mi355_core *c, const void *d_offsets, const void *d_xs, int nframes, void *d_frames,
                           size_t stride_bytes, int clear) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0) return fail(MI355_ERR_INVALID, "nframes < 0");
    if (nframes == 0 || c->n == 0) return MI355_OK;
    if (!d_offsets || !d_xs || !d_frames) return fail(MI355_ERR_INVALID, "null argument");
    if (stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    if (int rc = use_device(c)) return rc;
    // only the cleared form needs per-frame scratch (slice bounds), which is sized for max_batch frames
    if (clear && nframes > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nframes outside [0, max_batch]");
    if (clear)
        if (int rc = need_red_bounds(c)) return rc;
    HIP_TRY(launch_red_stream((uint8_t *)d_frames, (const uint32_t *)d_offsets, (const int32_t *)d_xs, c->n, clear != 0,
                              FrameBatch{stride_bytes, nframes}, c->stream, c->red_bounds));
    return MI355_OK;
}

int mi355_conv3x3(mi355_core *c, const void *d_in, void *d_out) {
    if (!c || (c->n && (!d_in || !d_out))) return fail(MI355_ERR_INVALID, "null argument");
    if (d_in == d_out && c->n) return fail(MI355_ERR_INVALID, "conv3x3 cannot run in place");
    if (!c->have_k9) return fail(MI355_ERR_STATE, "mi355_set_conv_kernel not called");
    if (int rc = use_device_filter(c)) return rc;
    HIP_TRY(launch_conv3x3((const uint8_t *)d_in, (uint8_t *)d_out, c->cfg.width, c->cfg.height, c->k9,
                           c->k9_sym, FrameBatch{c->n, 1}, c->stream));
    return MI355_OK;
}

int mi355_conv_kxk(mi355_core *c, const void *d_in, void *d_out, const float *k, int K) {
    if (!c || !k || (c->n && (!d_in || !d_out))) return fail(MI355_ERR_INVALID, "null argument");
    if (K < 1 || K > 9) return fail(MI355_ERR_INVALID, "K outside [1, 9]");
    if (d_in == d_out && c->n) return fail(MI355_ERR_INVALID, "conv_kxk cannot run in place");
    if (int rc = use_device_filter(c)) return rc;
    if (!c->kxk)
        if (int rc = dev_alloc(c, &c->kxk, 81)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));    // a filter of an earlier call may still be reading the taps
    HIP_TRY(hipMemcpyAsync(c->kxk, k, sizeof(float) * K * K, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));    // k is the caller's (pageable) memory
    HIP_TRY(launch_conv_kxk((const uint8_t *)d_in, (uint8_t *)d_out, c->cfg.width, c->cfg.height, c->kxk, K,
                            FrameBatch{c->n, 1}, c->stream));
    return MI355_OK;
}

int mi355_median5x5(mi355_core *c, const void *d_in, void *d_out) {
    if (!c || !d_in || !d_out) return fail(MI355_ERR_INVALID, "null argument");
    if (d_in == d_out) return fail(MI355_ERR_INVALID, "median is not in-place");
    if (int rc = use_device_filter(c)) return rc;
    HIP_TRY(launch_median5x5((const uint8_t *)d_in, (uint8_t *)d_out, c->cfg.width, c->cfg.height, c->median_rows,
                             FrameBatch{c->n, 1}, c->stream));
    return MI355_OK;
}

int mi355_filter_batch(mi355_core *c, int op, const void *d_in, const void *d_in2, void *d_out,
                       size_t stride_bytes, int nframes) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (nframes < 0 || nframes > c->cfg.max_batch) return fail(MI355_ERR_INVALID, "nframes outside [0, max_batch]");
    if (nframes == 0 || c->n == 0) return MI355_OK;
    if (!d_in || !d_out) return fail(MI355_ERR_INVALID, "null frame pointer");
    if (stride_bytes < c->n) return fail(MI355_ERR_INVALID, "stride_bytes < frame bytes");
    const bool two = op == MI355_OP_HEAT_MAP || op == MI355_OP_RED_DENSE;
    if (two && !d_in2) return fail(MI355_ERR_INVALID, "this filter needs the previous frames (d_in2)");
    if (op == MI355_OP_CONV3X3 && !c->have_k9) return fail(MI355_ERR_STATE, "mi355_set_conv_kernel not called");
    if ((op == MI355_OP_CONV3X3 || op == MI355_OP_MEDIAN5X5) && d_in == d_out)
        return fail(MI355_ERR_INVALID, "neighbourhood filters cannot run in place");
    if (int rc = use_device_filter(c)) return rc;
    const uint8_t *in = (const uint8_t *)d_in, *in2 = (const uint8_t *)d_in2;
    uint8_t *out = (uint8_t *)d_out;
    const FrameBatch fb{stride_bytes, nframes};
    const uint32_t npix = c->n / 3;
    switch (op) {
        case MI355_OP_GRAY_AVG: HIP_TRY(launch_gray(in, out, npix, false, fb, c->stream)); break;
        case MI355_OP_GRAY_WEIGHTED: HIP_TRY(launch_gray(in, out, npix, true, fb, c->stream)); break;
        case MI355_OP_BINARIZE: HIP_TRY(launch_binarize_chain(in, out, c->n, c->hist, c->thr, fb, c->stream)); break;
        case MI355_OP_GRAY_AVG_BINARIZE:
            if (int rc = need_gray1(c)) return rc;
            HIP_TRY(launch_gray_binarize_fused(in, out, npix, false, c->hist, c->thr, fb, c->stream, c->gray1, c->gray1_stride)); break;
        case MI355_OP_GRAY_WEIGHTED_BINARIZE:
            if (int rc = need_gray1(c)) return rc;
            HIP_TRY(launch_gray_binarize_fused(in, out, npix, true, c->hist, c->thr, fb, c->stream, c->gray1, c->gray1_stride)); break;
        case MI355_OP_HEAT_MAP: HIP_TRY(launch_heat_map(in, in2, out, npix, c->lut, fb, c->stream)); break;
        case MI355_OP_RED_DENSE: HIP_TRY(launch_red_dense(in, in2, out, npix, c->cfg.threshold, fb, c->stream)); break;
        case MI355_OP_CONV3X3: HIP_TRY(launch_conv3x3(in, out, c->cfg.width, c->cfg.height, c->k9, c->k9_sym, fb, c->stream)); break;
        case MI355_OP_MEDIAN5X5: HIP_TRY(launch_median5x5(in, out, c->cfg.width, c->cfg.height, c->median_rows, fb, c->stream)); break;
        default: return fail(MI355_ERR_INVALID, "unknown filter op");
    }
    return MI355_OK;
}

// CUDACore::exec_core, kernels.cu:430-525.
namespace {

// kernels.cu:466-502: text overlay on the frame, then the visualisers that look at the frame before the
// diff (heat / gray / binarize), or the canvas the red maps are painted on afterwards.
int prepare_frame(mi355_core *c, uint8_t *frame, uint8_t *vis_out, const char *text, hipStream_t s) {
    const int vis = c->cfg.visualizer;
    const uint32_t N = c->n, npix = N / 3;
    const FrameBatch one{N, 1};
    if (text && c->glyphs) {
        const size_t full_area = (size_t)3 * c->glyph_h * c->glyph_w;
        int offset = 0;
        for (const char *p = text; *p; ++p, offset += c->glyph_w * 3) {
            const size_t idx = c->charset.find(*p);
            if (idx == std::string::npos) continue;
            HIP_TRY(launch_blit_glyph(frame, c->glyphs + idx * full_area, c->glyph_h, 3 * c->glyph_w, offset,
                                      3 * c->cfg.width, c->cfg.height, s));
        }
    }
    if (vis == MI355_VIS_HEAT) {
        HIP_TRY(launch_heat_map(frame, c->state, vis_out, npix, c->lut, one, s));
    } else if (vis == MI355_VIS_GRAY) {
        HIP_TRY(launch_gray(frame, vis_out, npix, true, one, s));
    } else if (vis == MI355_VIS_BINARIZE) {
        // grayscale_kernel_v3 + histogram + compute_max + binarize (kernels.cu:493-498), fused: the
        // gray frame is never materialised
        if (int rc = need_gray1(c)) return rc;
        HIP_TRY(launch_gray_binarize_fused(frame, vis_out, npix, true, c->hist, c->thr, one, s, c->gray1, c->gray1_stride));
    } else if (vis == MI355_VIS_RED_OVERLAP) {
        // kernels.cu:517 paints onto d_previous, i.e. the state *before* this frame's feedback
        HIP_TRY(hipMemcpyAsync(vis_out, c->state, N, hipMemcpyDeviceToDevice, s));
    } else if (vis == MI355_VIS_RED) {
        HIP_TRY(hipMemsetAsync(vis_out, 0, N, s));                      // kernels.cu:513
    }
    return MI355_OK;
}

int check_exec_args(mi355_core *c, const void *frame_data, const void *show_ready, const void *h_xs) {
    if (!c || !frame_data || !h_xs) return fail(MI355_ERR_INVALID, "null argument");
    if (c->cfg.visualizer != MI355_VIS_NONE && !show_ready)
        return fail(MI355_ERR_INVALID, "visualizer set but show_ready is null");
    if (c->cfg.noise_filter && !c->have_k9) return fail(MI355_ERR_STATE, "noise filter on but no conv kernel set");
    return MI355_OK;
}

bool is_pinned(const void *p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

}  // namespace

// MI355_PREPARE_EXEC: the kernels of one mi355_exec over a copy of the current state.  Nothing differs from the state, so no
// byte is flagged, the state is rewritten with itself and the export stores a count of 0 into the core's own pinned word.
static int warm_exec(mi355_core *c) {
    hipStream_t s = c->stream;
    const uint32_t N = c->n;
    const int vis = c->cfg.visualizer;
    HIP_TRY(hipMemcpyAsync(c->in, c->state, N, hipMemcpyDeviceToDevice, s));
    if (c->cfg.noise_filter && c->have_k9)   // (its output is not used: a filtered frame would differ from the state)
        HIP_TRY(launch_conv3x3(c->in, c->aux, c->cfg.width, c->cfg.height, c->k9, c->k9_sym, FrameBatch{N, 1}, s));
    if (int rc = prepare_frame(c, c->in, c->vis, nullptr, s)) return rc;
    if (int rc = run_batch(c, BatchMode{}, c->in, nullptr, N, 1, c->offsets, c->one_xs, c->one_diff, N)) return rc;
    if (vis == MI355_VIS_RED || vis == MI355_VIS_RED_OVERLAP)
        HIP_TRY(launch_red_overlap(c->vis, c->one_xs, c->offsets + 1, 0, N, s));
    HIP_TRY(launch_export(c->offsets, c->one_xs, c->one_diff, (int32_t *)c->h_count, (uint8_t *)c->h_count, c->h_count, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (c->h_count[0] != 0) return fail(MI355_ERR_STATE, "mi355_prepare(EXEC): the warm pass found a difference");
    return MI355_OK;
}

// A frame of mi355_exec / mi355_exec_cwire up to its packed entries in one_xs / one_diff (the caller has made the device
// current): upload, noise filter, overlay, the visualisers that look at the frame before the diff, the diff with feedback.
static int exec_frame(mi355_core *c, const uint8_t *frame_data, uint8_t *show_ready, const char *text) {
    const int vis = c->cfg.visualizer;
    hipStream_t s = c->stream;
    const uint32_t N = c->n;
    const FrameBatch one{N, 1};

    // kernels.cu:457-462  H2D (+ convolution when NOISE_FILTER)
    if (c->cfg.noise_filter) {
        HIP_TRY(hipMemcpyAsync(c->aux, frame_data, N, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_conv3x3(c->aux, c->in, c->cfg.width, c->cfg.height, c->k9, c->k9_sym, one, s));
    } else {
        HIP_TRY(hipMemcpyAsync(c->in, frame_data, N, hipMemcpyHostToDevice, s));
    }
    if (int rc = prepare_frame(c, c->in, c->vis, text, s)) return rc;
    if (vis == MI355_VIS_HEAT || vis == MI355_VIS_GRAY || vis == MI355_VIS_BINARIZE)
        HIP_TRY(hipMemcpyAsync(show_ready, c->vis, N, hipMemcpyDeviceToHost, s));

    // kernels.cu:505  kernel2
    return run_batch(c, BatchMode{}, c->in, nullptr, N, 1, c->offsets, c->one_xs, c->one_diff, N);
}

int mi355_exec(mi355_core *c, uint8_t *frame_data, uint8_t *show_ready, const char *text,
               uint32_t *h_pos, int32_t *h_xs) {
    if (!h_pos) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = check_exec_args(c, frame_data, show_ready, h_xs)) return rc;
    if (c->nslots) return fail(MI355_ERR_STATE, "pipe open: use mi355_pipe_submit");
    const int vis = c->cfg.visualizer;
    if (int rc = use_device(c)) return rc;
    hipStream_t s = c->stream;
    const uint32_t N = c->n;
    if (int rc = exec_frame(c, frame_data, show_ready, text)) return rc;
    if (is_pinned(frame_data) && is_pinned(h_xs)) {
        // Pinned buffers (alloc_arrays): the count stays on the device, the red maps take it from there and
        // k_export stores count/diff/xs through the mapped pointers -- one synchronisation instead of the
        // reference's two (kernels.cu:508,524); what the caller sees on return is the same.
        if (vis == MI355_VIS_RED || vis == MI355_VIS_RED_OVERLAP) {
            HIP_TRY(launch_red_overlap(c->vis, c->one_xs, c->offsets + 1, 0, N, s));
            HIP_TRY(hipMemcpyAsync(show_ready, c->vis, N, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(launch_export(c->offsets, c->one_xs, c->one_diff, h_xs, frame_data, c->h_count, s));
        HIP_TRY(hipStreamSynchronize(s));
        *h_pos = c->h_count[0];
        return MI355_OK;
    }
    // pageable buffers: the reference's sequence, kernels.cu:507-508 count back + first synchronisation
    HIP_TRY(hipMemcpyAsync(c->h_count, c->offsets, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t pos = c->h_count[1];
    *h_pos = pos;
    // kernels.cu:511-520  red maps from the packed indices
    if (vis == MI355_VIS_RED || vis == MI355_VIS_RED_OVERLAP) {
        HIP_TRY(launch_red_overlap(c->vis, c->one_xs, nullptr, pos, N, s));
        HIP_TRY(hipMemcpyAsync(show_ready, c->vis, N, hipMemcpyDeviceToHost, s));
    }
    // kernels.cu:522-524
    if (pos) {
        HIP_TRY(hipMemcpyAsync(frame_data, c->one_diff, pos, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_xs, c->one_xs, (size_t)pos * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return MI355_OK;
}

// ---- pipelined per-frame path --------------------------------------------------------------------------
int mi355_pipe_close(mi355_core *c) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
    if (c->down_stream) (void)hipStreamSynchronize(c->down_stream);
    (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < c->nslots; i++) {
        mi355_core::Slot &sl = c->slots[i];
        if (sl.d_in) { (void)hipFree(sl.d_in); c->workspace -= c->n + 16; }
        if (sl.d_vis) { (void)hipFree(sl.d_vis); c->workspace -= c->n + 16; }
        if (sl.h_count) (void)hipHostFree(sl.h_count);
        for (hipEvent_t e : {sl.uploaded, sl.painted, sl.packed, sl.shown}) if (e) (void)hipEventDestroy(e);
        sl = mi355_core::Slot{};
    }
    c->nslots = 0;
    if (c->up_stream) { (void)hipStreamDestroy(c->up_stream); c->up_stream = nullptr; }
    if (c->down_stream) { (void)hipStreamDestroy(c->down_stream); c->down_stream = nullptr; }
    return MI355_OK;
}

int mi355_pipe_open(mi355_core *c, int depth) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (depth < 1 || depth > mi355_core::kMaxSlots) return fail(MI355_ERR_INVALID, "depth outside [1, 8]");
    if (c->nslots) return fail(MI355_ERR_STATE, "pipe already open");
    if (int rc = use_device(c)) return rc;
    int rc = MI355_OK;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking)) != hipSuccess) rc = fail(MI355_ERR_HIP, "hipStreamCreate", e);
    if (!rc && (e = hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking)) != hipSuccess) rc = fail(MI355_ERR_HIP, "hipStreamCreate", e);
    c->nslots = depth;   // so that a failed open is undone by pipe_close
    const bool vis = c->cfg.visualizer != MI355_VIS_NONE;
    for (int i = 0; i < depth && !rc; i++) {
        mi355_core::Slot &sl = c->slots[i];
        rc = dev_alloc(c, &sl.d_in, (size_t)c->n + 16);
        if (!rc && vis) rc = dev_alloc(c, &sl.d_vis, (size_t)c->n + 16);
        if (!rc && (e = hipHostMalloc((void **)&sl.h_count, sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess) rc = fail(MI355_ERR_HIP, "hipHostMalloc", e);
        for (hipEvent_t *ev : {&sl.uploaded, &sl.painted, &sl.packed, &sl.shown})
            if (!rc && (e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) rc = fail(MI355_ERR_HIP, "hipEventCreate", e);
    }
    if (rc) {
        const std::string keep = g_err;
        (void)mi355_pipe_close(c);
        g_err = keep;
        return rc;
    }
    c->next_ticket = 0;
    return MI355_OK;
}

// A frame of mi355_pipe_submit / mi355_pipe_submit_cwire up to its export, into the ring's next slot: upload, noise filter,
// overlay, visualiser, diff with feedback into one_xs / one_diff, red maps, the visualisation frame's way back.
static int pipe_frame(mi355_core *c, const uint8_t *frame_data, uint8_t *show_ready, const char *text, mi355_core::Slot &sl) {
    const int vis = c->cfg.visualizer;
    const uint32_t N = c->n;
    const FrameBatch one{N, 1};
    hipStream_t s = c->stream;
    if (sl.ticket >= 0) {   // ring full: the slot's previous frame was never waited for; finish it first
        HIP_TRY(hipEventSynchronize(sl.packed));
        if (sl.has_vis) HIP_TRY(hipEventSynchronize(sl.shown));
        sl.ticket = -1;
    }
    // upload on its own stream: frame k+1 crosses PCIe while frame k is packed (threads.cpp's capture and
    // elaboration threads overlap the same way, threads.cpp:59-106,134-147)
    HIP_TRY(hipMemcpyAsync(sl.d_in, frame_data, N, hipMemcpyHostToDevice, c->up_stream));
    HIP_TRY(hipEventRecord(sl.uploaded, c->up_stream));
    HIP_TRY(hipStreamWaitEvent(s, sl.uploaded, 0));
    uint8_t *frame = sl.d_in;
    if (c->cfg.noise_filter) {
        HIP_TRY(launch_conv3x3(sl.d_in, c->in, c->cfg.width, c->cfg.height, c->k9, c->k9_sym, one, s));
        frame = c->in;
    }
    if (int rc = prepare_frame(c, frame, sl.d_vis, text, s)) return rc;
    if (int rc = run_batch(c, BatchMode{}, frame, nullptr, N, 1, c->offsets, c->one_xs, c->one_diff, N)) return rc;
    if (vis == MI355_VIS_RED || vis == MI355_VIS_RED_OVERLAP)
        HIP_TRY(launch_red_overlap(sl.d_vis, c->one_xs, c->offsets + 1, 0, N, s));
    sl.has_vis = vis != MI355_VIS_NONE;
    if (sl.has_vis) {   // the visualisation frame goes back on a third stream, beside the next frame's kernels
        HIP_TRY(hipEventRecord(sl.painted, s));
        HIP_TRY(hipStreamWaitEvent(c->down_stream, sl.painted, 0));
        HIP_TRY(hipMemcpyAsync(show_ready, sl.d_vis, N, hipMemcpyDeviceToHost, c->down_stream));
        HIP_TRY(hipEventRecord(sl.shown, c->down_stream));
    }
    return MI355_OK;
}

int mi355_pipe_submit(mi355_core *c, uint8_t *frame_data, uint8_t *show_ready, const char *text, int32_t *h_xs,
                      int64_t *ticket) {
    if (!ticket) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = check_exec_args(c, frame_data, show_ready, h_xs)) return rc;
    if (!c->nslots) return fail(MI355_ERR_STATE, "pipe not open");
    if (int rc = use_device(c)) return rc;
    // the kernels store through these pointers: pageable memory would fault on the device
    if (!is_pinned(frame_data) || !is_pinned(h_xs) || (show_ready && !is_pinned(show_ready)))
        return fail(MI355_ERR_INVALID, "pipe buffers must be pinned host memory (mi355_host_alloc)");
    mi355_core::Slot &sl = c->slots[c->next_ticket % c->nslots];
    if (int rc = pipe_frame(c, frame_data, show_ready, text, sl)) return rc;
    // count, indices and differences leave through the mapped pointers: no host round trip for the count
    HIP_TRY(launch_export(c->offsets, c->one_xs, c->one_diff, h_xs, frame_data, sl.h_count, c->stream));
    HIP_TRY(hipEventRecord(sl.packed, c->stream));
    sl.compact = false;
    sl.ticket = c->next_ticket;
    *ticket = c->next_ticket++;
    return MI355_OK;
}

// Finds the frame of `ticket` complete in its slot, or says why not.
static int pipe_wait_slot(mi355_core *c, int64_t ticket, bool compact_only, mi355_core::Slot **out) {
    if (!c->nslots) return fail(MI355_ERR_STATE, "pipe not open");
    if (ticket < 0 || ticket >= c->next_ticket) return fail(MI355_ERR_INVALID, "unknown ticket");
    mi355_core::Slot &sl = c->slots[ticket % c->nslots];
    if (sl.ticket != ticket) return fail(MI355_ERR_STATE, "ticket already waited for or overwritten");
    if (compact_only && !sl.compact)   // (the ticket stays waitable)
        return fail(MI355_ERR_STATE, "ticket of mi355_pipe_submit: it has no compact record, use mi355_pipe_wait");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipEventSynchronize(sl.packed));
    if (sl.has_vis) HIP_TRY(hipEventSynchronize(sl.shown));
    *out = &sl;
    return MI355_OK;
}

int mi355_pipe_wait(mi355_core *c, int64_t ticket, uint32_t *h_pos) {
    if (!c || !h_pos) return fail(MI355_ERR_INVALID, "null argument");
    mi355_core::Slot *sl = nullptr;
    if (int rc = pipe_wait_slot(c, ticket, false, &sl)) return rc;
    *h_pos = sl->compact ? c->h_rec[(sl - c->slots) * mi355_core::kRecWords] : *sl->h_count;
    sl->ticket = -1;
    return MI355_OK;
}

// ---- the per-frame path into ONE compact record (include/mi355diff.h, "compact form of the per-frame entry points") ----
namespace {

constexpr int kRecBlocking = mi355_core::kMaxSlots;        // h_rec: the words of mi355_exec_cwire
constexpr int kRecScratch = mi355_core::kMaxSlots + 1;     // ... and the 16 bytes of scratch

// one_xs / one_diff of the frame run_batch has just packed -> its record in cw_rec, the record's size in cw_rec_pos[1]
int encode_record(mi355_core *c) {
    HIP_TRY(launch_cwire_encode(c->offsets, c->one_xs, c->one_diff, c->n, 1, c->cw_cnt, c->cw_rec_pos, c->cw_rec, c->cw_rec_bytes,
                                c->stream));
    return MI355_OK;
}

int check_exec_cwire_args(mi355_core *c, const void *frame_data, const void *show_ready, const void *h_record, size_t record_capacity) {
    if (int rc = check_exec_args(c, frame_data, show_ready, h_record)) return rc;
    if ((uintptr_t)h_record & 3u) return fail(MI355_ERR_INVALID, "h_record must be 4-byte aligned");
    // a record that did not fit would lose a frame whose state has already advanced: the worst case is demanded up front
    if (record_capacity < mi355_cwire_bytes_max(c->n, 1))
        return fail(MI355_ERR_INVALID, "record_capacity below mi355_cwire_bytes_max(frame bytes, 1)");
    return MI355_OK;
}

// h_record is pinned up to the last byte the export kernel could ever store (the worst-case record)
bool record_is_pinned(const mi355_core *c, const void *h_record) {
    return is_pinned(h_record) && is_pinned((const uint8_t *)h_record + mi355_cwire_bytes_max(c->n, 1) - 1);
}

void read_rec_words(const uint32_t *w, uint32_t *h_pos, uint32_t *h_escapes, size_t *h_bytes) {
    *h_pos = w[0];
    *h_escapes = w[1];
    *h_bytes = (size_t)(w[2] | (uint64_t)w[3] << 32);
}

}  // namespace

// The record buffer, its frame_pos and the pinned result words; then the encode and export kernels once, on an empty frame
// (the offsets of a frame without entries), so that the first real frame does not pay for their first use.
static int need_exec_cwire(mi355_core *c) {
    if (c->cw_warm) return MI355_OK;   // (a warm pass that failed is run again, on the buffers that exist)
    c->cw_rec_bytes = (uint64_t)mi355_cwire_bytes_max(c->n, 1);
    if (!c->cw_rec)
        if (int rc = dev_alloc(c, &c->cw_rec, (size_t)((c->cw_rec_bytes + 15) & ~15ull))) return rc;
    if (!c->cw_rec_pos)
        if (int rc = dev_alloc(c, &c->cw_rec_pos, 2)) return rc;
    if (!c->h_rec) {
        HIP_TRY(hipHostMalloc((void **)&c->h_rec, (size_t)(kRecScratch + 1) * mi355_core::kRecWords * sizeof(uint32_t), hipHostMallocDefault));
        memset(c->h_rec, 0xff, (size_t)(kRecScratch + 1) * mi355_core::kRecWords * sizeof(uint32_t));
    }
    // (c->offsets: every frame queued so far has read its own, in stream order; the next frame writes them again)
    HIP_TRY(hipMemsetAsync(c->offsets, 0, 2 * sizeof(uint32_t), c->stream));
    if (int rc = encode_record(c)) return rc;
    uint32_t *const words = c->h_rec + kRecBlocking * mi355_core::kRecWords, *const scratch = c->h_rec + kRecScratch * mi355_core::kRecWords;
    HIP_TRY(launch_export_record(c->cw_rec_pos, c->cw_rec, c->cw_rec_bytes, scratch, words, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (words[0] != 0 || words[1] != 0 || words[2] != 8 || words[3] != 0 || scratch[0] != 0 || scratch[1] != 0)
        return fail(MI355_ERR_STATE, "MI355_PREPARE_EXEC_CWIRE: the warm pass did not give the empty record");
    c->cw_warm = true;
    return MI355_OK;
}

int mi355_exec_cwire(mi355_core *c, const uint8_t *frame_data, uint8_t *show_ready, const char *text, void *h_record,
                     size_t record_capacity, uint32_t *h_pos, uint32_t *h_escapes, size_t *h_bytes) {
    if (!h_pos || !h_escapes || !h_bytes) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = check_exec_cwire_args(c, frame_data, show_ready, h_record, record_capacity)) return rc;
    if (c->nslots) return fail(MI355_ERR_STATE, "pipe open: use mi355_pipe_submit_cwire");
    const int vis = c->cfg.visualizer;
    if (int rc = use_device(c)) return rc;
    if (int rc = need_exec_cwire(c)) return rc;
    hipStream_t s = c->stream;
    const uint32_t N = c->n;
    if (int rc = exec_frame(c, frame_data, show_ready, text)) return rc;
    // the red maps take the count from the device in either form (the indices stay in one_xs)
    if (vis == MI355_VIS_RED || vis == MI355_VIS_RED_OVERLAP) {
        HIP_TRY(launch_red_overlap(c->vis, c->one_xs, c->offsets + 1, 0, N, s));
        HIP_TRY(hipMemcpyAsync(show_ready, c->vis, N, hipMemcpyDeviceToHost, s));
    }
    if (int rc = encode_record(c)) return rc;
    if (record_is_pinned(c, h_record)) {
        // pinned: the record's size stays on the device, k_export_record stores exactly that many bytes through the mapped
        // pointer -- one synchronisation
        uint32_t *const words = c->h_rec + kRecBlocking * mi355_core::kRecWords;
        HIP_TRY(launch_export_record(c->cw_rec_pos, c->cw_rec, c->cw_rec_bytes, (uint32_t *)h_record, words, s));
        HIP_TRY(hipStreamSynchronize(s));
        read_rec_words(words, h_pos, h_escapes, h_bytes);
        return MI355_OK;
    }
    // pageable: the header and the size come back first, then a copy of exactly that many bytes
    uint32_t *const scratch = c->h_rec + kRecScratch * mi355_core::kRecWords;
    HIP_TRY(hipMemcpyAsync(scratch, c->cw_rec, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(scratch + 2, c->cw_rec_pos + 1, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t bytes = scratch[2] | (uint64_t)scratch[3] << 32;
    if (bytes > c->cw_rec_bytes || scratch[0] > N || scratch[1] > scratch[0] || bytes != cwire_record_bytes(scratch[0], scratch[1]))
        return fail(MI355_ERR_STATE, "mi355_exec_cwire: the encoder left an inconsistent record");
    HIP_TRY(hipMemcpyAsync(h_record, c->cw_rec, (size_t)bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *h_pos = scratch[0];
    *h_escapes = scratch[1];
    *h_bytes = (size_t)bytes;
    return MI355_OK;
}

int mi355_pipe_submit_cwire(mi355_core *c, const uint8_t *frame_data, uint8_t *show_ready, const char *text, void *h_record,
                            size_t record_capacity, int64_t *ticket) {
    if (!ticket) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = check_exec_cwire_args(c, frame_data, show_ready, h_record, record_capacity)) return rc;
    if (!c->nslots) return fail(MI355_ERR_STATE, "pipe not open");
    if (int rc = use_device(c)) return rc;
    // the export kernel stores through h_record, and only a pinned frame crosses PCIe beside the frame before it
    if (!is_pinned(frame_data) || !record_is_pinned(c, h_record) || (show_ready && !is_pinned(show_ready)))
        return fail(MI355_ERR_INVALID, "pipe buffers must be pinned host memory (mi355_host_alloc)");
    if (int rc = need_exec_cwire(c)) return rc;
    mi355_core::Slot &sl = c->slots[c->next_ticket % c->nslots];
    if (int rc = pipe_frame(c, frame_data, show_ready, text, sl)) return rc;
    if (int rc = encode_record(c)) return rc;
    HIP_TRY(launch_export_record(c->cw_rec_pos, c->cw_rec, c->cw_rec_bytes, (uint32_t *)h_record,
                                 c->h_rec + (&sl - c->slots) * mi355_core::kRecWords, c->stream));
    HIP_TRY(hipEventRecord(sl.packed, c->stream));
    sl.compact = true;
    sl.ticket = c->next_ticket;
    *ticket = c->next_ticket++;
    return MI355_OK;
}

int mi355_pipe_wait_cwire(mi355_core *c, int64_t ticket, uint32_t *h_pos, uint32_t *h_escapes, size_t *h_bytes) {
    if (!c || !h_pos || !h_escapes || !h_bytes) return fail(MI355_ERR_INVALID, "null argument");
    mi355_core::Slot *sl = nullptr;
    if (int rc = pipe_wait_slot(c, ticket, true, &sl)) return rc;
    read_rec_words(c->h_rec + (sl - c->slots) * mi355_core::kRecWords, h_pos, h_escapes, h_bytes);
    sl->ticket = -1;
    return MI355_OK;
}

int mi355_host_alloc(void **out, size_t bytes) {
    if (!out) return fail(MI355_ERR_INVALID, "null argument");
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault));
    return MI355_OK;
}

int mi355_host_free(void *p) {
    if (!p) return MI355_OK;
    HIP_TRY(hipHostFree(p));
    return MI355_OK;
}

int mi355_dev_alloc(mi355_core *c, void **out, size_t bytes) {
    if (!c || !out) return fail(MI355_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipMalloc(out, bytes ? bytes : 16));
    return MI355_OK;
}

// ---- output arrays whose PLACEMENT lets the dense expansion run at its fast speed ---------------------------------------
// What round 6 found (profiles/README.md, r06a-r06e): when most bytes of a frame change (the synthetic S0 / P = N regimes, a
// scene cut), k_expand is bound by its stores, and writes the index array and the value array at 5.1 TB/s together when the
// two streams overlap in the memory system -- or at 4.0 TB/s (265 instead of 205 us per 32 S0 pairs) when they do not.
// Which of the two a pair of arrays gets is a property of the PAIR's physical memory (it stays with the arrays for their
// life; another value array beside the same index array re-draws it; between one pair in six and two in three are of the
// fast kind, box to box; physically contiguous memory is the slowest; the L2's tag stalls and the DRAM-credit stalls of
// its write requests differ, the request counts do not) -- nothing a caller can see in an address, nothing an offset
// inside an allocation changes, and a synthetic store kernel of another grid shape mis-predicts it (r06d).  What a caller
// CAN do is measure with the expansion itself: this call packs a batch of noise frames (P = 0.85 N, the S0 regime) once per
// candidate value array and keeps the first pair on which k_expand moves its bytes at the fast rate.
namespace {
__global__ __launch_bounds__(256) void k_noise_frames(uint32_t *out, size_t nwords, uint32_t seed) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += stride) {
        uint32_t x = (uint32_t)i * 2654435761u + seed;
        x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
        out[i] = x;
    }
}
}  // namespace

int mi355_alloc_outputs(mi355_core *c, size_t capacity, void **d_xs, void **d_diff, int *draws_out) {
    if (!c || !d_xs || !d_diff) return fail(MI355_ERR_INVALID, "null argument");
    *d_xs = *d_diff = nullptr;
    if (draws_out) *draws_out = 0;
    if (c->nslots) return fail(MI355_ERR_STATE, "pipe open");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t xs_bytes = (capacity ? capacity : 4) * sizeof(int32_t), df_bytes = capacity ? capacity : 16;
    int32_t *xs = nullptr;
    HIP_TRY(hipMalloc((void **)&xs, xs_bytes));
    // the probe: T frames of noise against T other frames of noise, as many as the arrays hold; only worth its while where the
    // placement matters (a pair of a few hundred MB written by a few thousand expander waves at a time)
    const size_t N = c->n;
    int T = c->cfg.max_batch;
    if (N && (size_t)T * N > capacity) T = (int)(capacity / N);
    constexpr int kMaxDraws = 32;
    uint8_t *cand[kMaxDraws] = {};
    int ndraw = 0, keep = -1;
    int rc = MI355_OK;
    if (T >= 8 && (size_t)T * N >= ((size_t)48 << 20) && N % 16 == 0 && 3 * (uint64_t)N + N < (1ull << 32)) {
        uint8_t *frames = nullptr;
        uint32_t *off = nullptr;
        const size_t fbytes = 2 * (size_t)T * N;
        if (hipMalloc((void **)&frames, fbytes) != hipSuccess || hipMalloc((void **)&off, ((size_t)T + 1) * 4) != hipSuccess) {
            (void)hipGetLastError();   // no room for the probe: plain allocations
        } else {
            hipLaunchKernelGGL(k_noise_frames, dim3(4096), dim3(256), 0, c->stream, (uint32_t *)frames, fbytes / 4, 0x9e3779b9u);
            const bool was_timing = c->timing;
            if ((rc = harvest_timing(c)) == MI355_OK) {
                const double s_pack = c->ms_pack, s_scan = c->ms_scan, s_exp = c->ms_expand, s_tot = c->ms_total;
                const int s_l = c->launches;
                double best_rate = 0;
                BatchMode pairs;
                pairs.pair = true;
                while (ndraw < kMaxDraws && rc == MI355_OK) {
                    if (hipMalloc((void **)&cand[ndraw], df_bytes) != hipSuccess) { (void)hipGetLastError(); break; }
                    uint8_t *df = cand[ndraw++];
                    // untimed first: ~15 ms of this load on the first candidate (a chip that has been idle needs them to reach
                    // its clocks), one batch on the others
                    c->timing = false;
                    for (int rep = 0; rep < (ndraw == 1 ? 48 : 1) && rc == MI355_OK; rep++)
                        rc = run_batch(c, pairs, frames, frames + (size_t)T * N, N, T, off, xs, df, capacity);
                    c->timing = true;
                    c->ms_expand = 0; c->launches = 0;
                    for (int rep = 0; rep < 3 && rc == MI355_OK; rep++)
                        rc = run_batch(c, pairs, frames, frames + (size_t)T * N, N, T, off, xs, df, capacity);
                    if (rc == MI355_OK) rc = harvest_timing(c);
                    if (rc != MI355_OK) break;
                    uint32_t total = 0;
                    if (hipMemcpy(&total, off + T, 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(MI355_ERR_HIP, "hipMemcpy(total)"); break; }
                    // bytes the expansion moves: the records it reads (16 per lane: T x N) + 5 per entry it writes
                    const double ms = c->ms_expand / (c->launches ? c->launches : 1);
                    const double rate = ((double)T * N + 5.0 * total) / (ms * 1e-3);   // bytes per second
                    if (rate > best_rate) { best_rate = rate; keep = ndraw - 1; }
                    if (rate >= 4.5e12) break;   // fast pairs: 5.0-5.2 TB/s; slow ones: 3.9-4.1 (profiles/r06*)
                }
                c->timing = was_timing;
                c->ms_pack = s_pack; c->ms_scan = s_scan; c->ms_expand = s_exp; c->ms_total = s_tot; c->launches = s_l;
            }
            (void)hipStreamSynchronize(c->stream);
        }
        if (frames) (void)hipFree(frames);
        if (off) (void)hipFree(off);
    }
    if (rc == MI355_OK && keep < 0) {   // small arrays, or no room for the probe
        if (ndraw == 0 && hipMalloc((void **)&cand[0], df_bytes) == hipSuccess) ndraw = 1;
        keep = ndraw > 0 ? 0 : -1;
        if (keep < 0) rc = fail(MI355_ERR_HIP, "hipMalloc(value array)");
    }
    for (int i = 0; i < ndraw; i++)
        if (i != keep || rc != MI355_OK) (void)hipFree(cand[i]);
    if (rc != MI355_OK) { (void)hipFree(xs); return rc; }
    *d_xs = xs;
    *d_diff = cand[keep];
    if (draws_out) *draws_out = ndraw;
    return MI355_OK;
}

int mi355_dev_free(mi355_core *c, void *d_ptr) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));   // nothing of this core may still be using it
    HIP_TRY(hipFree(d_ptr));
    return MI355_OK;
}

int mi355_upload(mi355_core *c, void *d_dst, const void *host_src, size_t bytes) {
    if (!c || (bytes && (!d_dst || !host_src))) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device(c)) return rc;
    if (!bytes) return MI355_OK;
    HIP_TRY(hipMemcpyAsync(d_dst, host_src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355_OK;
}

int mi355_download(mi355_core *c, void *host_dst, const void *d_src, size_t bytes) {
    if (!c || (bytes && (!host_dst || !d_src))) return fail(MI355_ERR_INVALID, "null argument");
    if (int rc = use_device(c)) return rc;
    if (!bytes) return MI355_OK;
    HIP_TRY(hipMemcpyAsync(host_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355_OK;
}

int mi355_set_timing(mi355_core *c, int enabled) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    if (int rc = harvest_timing(c)) return rc;
    c->timing = enabled != 0;
    return MI355_OK;
}

int mi355_get_timing(mi355_core *c, double *ms_pack, double *ms_total, int *launches) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    if (int rc = harvest_timing(c)) return rc;
    if (ms_pack) *ms_pack = c->ms_pack;
    if (ms_total) *ms_total = c->ms_total;
    if (launches) *launches = c->launches;
    return MI355_OK;
}

int mi355_get_kernel_timing(mi355_core *c, double *ms_pack, double *ms_scan, double *ms_expand, int *launches) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    if (int rc = harvest_timing(c)) return rc;
    if (ms_pack) *ms_pack = c->ms_pack;
    if (ms_scan) *ms_scan = c->ms_scan;
    if (ms_expand) *ms_expand = c->ms_expand;
    if (launches) *launches = c->launches;
    return MI355_OK;
}

int mi355_reset_timing(mi355_core *c) {
    if (!c) return fail(MI355_ERR_INVALID, "null core");
    if (int rc = use_device(c)) return rc;
    if (int rc = harvest_timing(c)) return rc;
    c->ms_pack = c->ms_scan = c->ms_expand = c->ms_total = 0;
    c->launches = 0;
    return MI355_OK;
}

}  // extern "C"

// compat/src/cudacore.cpp -- diff::cuda::CUDACore over the C-ABI of libmi355diff.so.
//
// Host code stays C++ (as in the reference) and reaches the GPU only through include/mi355diff.h.
// Error behaviour follows the reference's CUDA_CHECK (server/src/kernels.cu:11-22): message on stderr,
// then exit with a non-zero status; nothing is thrown and nothing is returned.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../../include/mi355diff.h"
#include "../include/common.h"
#include "../include/kernels.cuh"

using namespace diff::cuda;
using namespace diff::utils;

#define MI355_CHECK(call)                                                                         \
    do {                                                                                          \
        const int rc_ = (call);                                                                   \
        if (rc_ != MI355_OK) {                                                                    \
            fprintf(stderr, "MI355_CHECK() error %d (%s) @ %s:%d [%s]\n", rc_, mi355_last_error(), \
                    __FILE__, __LINE__, __func__);                                                \
            exit(rc_ < 0 ? -rc_ : rc_);                                                           \
        }                                                                                         \
    } while (0)

static int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

CUDACore::CUDACore(uint8_t *charsPx, matsz &charsSz, float *k, int total, uint8_t *sampleMatData,
                   matsz &frameSz) {
    memset(reserved_, 0, sizeof reserved_);
    reserved_int_ = 0;
    core_ = nullptr;
    total_ = total;
    if (total != 3 * frameSz.area()) {
        fprintf(stderr, "CUDACore: total (%d) != 3 * %d * %d\n", total, frameSz.height, frameSz.width);
        exit(1);
    }
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = frameSz.width;
    cfg.height = frameSz.height;
    cfg.threshold = LR_THRESHOLDS;
    cfg.max_batch = env_int("MI355_MAX_BATCH", 1);   // exec_multi: the most cameras per tick (the logs grow with it)
    if (cfg.max_batch < 1) cfg.max_batch = 1;
    cfg.device = 0;  // kernels.cu:385 uses device 0
#ifdef NOISE_FILTER
    cfg.noise_filter = 1;
#endif
#ifdef NOISE_VISUALIZER
    cfg.visualizer = NOISE_VISUALIZER;
#endif
    cfg.noise_filter = env_int("MI355_NOISE_FILTER", cfg.noise_filter);
    cfg.visualizer = env_int("MI355_VISUALIZER", cfg.visualizer);
    MI355_CHECK(mi355_create(&cfg, &core_));
    if (k) MI355_CHECK(mi355_set_conv_kernel(core_, k));                         // kernels.cu:394
    if (charsPx && charsSz.area() > 0)                                            // kernels.cu:379-382
        MI355_CHECK(mi355_set_glyphs(core_, charsPx, (int)(sizeof(CHARS_STR) - 1), charsSz.height,
                                     charsSz.width, CHARS_STR));
    if (sampleMatData) MI355_CHECK(mi355_set_state(core_, sampleMatData));        // kernels.cu:406
    // nothing is left to be made, loaded or first-used inside exec_core (the reference allocates everything here too,
    // kernels.cu:395-402)
    MI355_CHECK(mi355_prepare(core_, MI355_PREPARE_EXEC | MI355_PREPARE_GRAY_CHAIN));
}

void CUDACore::exec_core(uint8_t *frameData, uint8_t *showReadyNData, std::string &text,
                         unsigned int *h_pos, int *h_xs) {
    uint32_t pos = 0;
    MI355_CHECK(mi355_exec(core_, frameData, showReadyNData, text.empty() ? nullptr : text.c_str(), &pos,
                           reinterpret_cast<int32_t *>(h_xs)));
    *h_pos = pos;
}

void CUDACore::pipe_open(int depth) { MI355_CHECK(mi355_pipe_open(core_, depth)); }

void CUDACore::pipe_close() { MI355_CHECK(mi355_pipe_close(core_)); }

long long CUDACore::exec_submit(uint8_t *frameData, uint8_t *showReadyNData, std::string &text, int *h_xs) {
    int64_t ticket = -1;
    MI355_CHECK(mi355_pipe_submit(core_, frameData, showReadyNData, text.empty() ? nullptr : text.c_str(),
                                  reinterpret_cast<int32_t *>(h_xs), &ticket));
    return ticket;
}

void CUDACore::exec_wait(long long ticket, unsigned int *h_pos) {
    uint32_t pos = 0;
    MI355_CHECK(mi355_pipe_wait(core_, ticket, &pos));
    *h_pos = pos;
}

void CUDACore::alloc_record(void **h_record, size_t *record_capacity, int r, int c) {
    *record_capacity = mi355_cwire_bytes_max((size_t)3 * r * c, 1);
    MI355_CHECK(mi355_host_alloc(h_record, *record_capacity));
}

void CUDACore::exec_core_compact(const uint8_t *frameData, uint8_t *showReadyNData, std::string &text, void *h_record,
                                 size_t record_capacity, unsigned int *h_pos, unsigned int *h_escapes, size_t *h_bytes) {
    uint32_t pos = 0, esc = 0;
    MI355_CHECK(mi355_exec_cwire(core_, frameData, showReadyNData, text.empty() ? nullptr : text.c_str(), h_record,
                                 record_capacity, &pos, &esc, h_bytes));
    *h_pos = pos;
    *h_escapes = esc;
}

long long CUDACore::exec_submit_compact(const uint8_t *frameData, uint8_t *showReadyNData, std::string &text, void *h_record,
                                        size_t record_capacity) {
    int64_t ticket = -1;
    MI355_CHECK(mi355_pipe_submit_cwire(core_, frameData, showReadyNData, text.empty() ? nullptr : text.c_str(), h_record,
                                        record_capacity, &ticket));
    return ticket;
}

void CUDACore::exec_wait_compact(long long ticket, unsigned int *h_pos, unsigned int *h_escapes, size_t *h_bytes) {
    uint32_t pos = 0, esc = 0;
    MI355_CHECK(mi355_pipe_wait_cwire(core_, ticket, &pos, &esc, h_bytes));
    *h_pos = pos;
    *h_escapes = esc;
}

void CUDACore::exec_multi(const void *d_frames, void *d_states, size_t stride, int nstreams, void *d_offsets, void *d_xs,
                          void *d_diff, size_t capacity) {
    MI355_CHECK(mi355_diff_multi_batch(core_, d_frames, d_states, stride, nstreams, d_offsets, d_xs, d_diff, capacity));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::exec_multi_stream(const void *d_frames, void *d_states, size_t stride, int nstreams, int nframes,
                                 void *d_offsets, void *d_xs, void *d_diff, size_t capacity) {
    MI355_CHECK(mi355_diff_multi_stream_batch(core_, d_frames, d_states, stride, nstreams, nframes, d_offsets, d_xs, d_diff,
                                              capacity));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::apply_multi(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, void *d_states,
                           size_t stride) {
    MI355_CHECK(mi355_apply_multi_cwire_batch(core_, d_cwire, counts, escapes, nstreams, d_states, stride));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::apply_multi_stream(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                                  void *d_states, size_t stride, void *d_frames_out, size_t out_stride) {
    MI355_CHECK(mi355_apply_multi_stream_cwire_batch(core_, d_cwire, counts, escapes, nstreams, nframes, d_states, stride,
                                                     d_frames_out, out_stride));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::coalesce_multi_stream(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                                     void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes) {
    MI355_CHECK(mi355_cwire_coalesce_cwire_batch(core_, d_cwire, counts, escapes, nstreams, nframes, d_offsets, d_frame_pos,
                                                 d_cwire_out, capacity_bytes));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::crop_multi_stream(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                                 const int32_t *h_rects, unsigned flags, void *d_offsets, void *d_frame_pos, void *d_cwire_out,
                                 size_t capacity_bytes) {
    MI355_CHECK(mi355_cwire_crop_cwire_batch(core_, d_cwire, counts, escapes, nstreams, nframes, h_rects, flags, d_offsets,
                                             d_frame_pos, d_cwire_out, capacity_bytes));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::mosaic_multi_stream(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                                   const int32_t *h_place, int canvas_w, int canvas_h, void *d_offsets, void *d_frame_pos,
                                   void *d_cwire_out, size_t capacity_bytes) {
    MI355_CHECK(mi355_cwire_mosaic_cwire_batch(core_, d_cwire, counts, escapes, nstreams, nframes, h_place, canvas_w, canvas_h,
                                               d_offsets, d_frame_pos, d_cwire_out, capacity_bytes));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::despeckle_multi(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, void *d_states, size_t stride,
                               int nstreams, const uint32_t *need, void *d_dropped, void *d_offsets, void *d_frame_pos,
                               void *d_cwire_out, size_t capacity_bytes) {
    MI355_CHECK(mi355_cwire_despeckle_cwire_batch(core_, d_cwire, counts, escapes, d_states, stride, nstreams, need, d_dropped, d_offsets,
                                                  d_frame_pos, d_cwire_out, capacity_bytes));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::budget_multi(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, void *d_states, size_t stride,
                            int nstreams, const uint32_t *budgets, void *d_thresholds, void *d_offsets, void *d_frame_pos,
                            void *d_cwire_out, size_t capacity_bytes) {
    MI355_CHECK(mi355_cwire_budget_cwire_batch(core_, d_cwire, counts, escapes, d_states, stride, nstreams, budgets, d_thresholds,
                                               d_offsets, d_frame_pos, d_cwire_out, capacity_bytes));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::activity_multi(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                              int cell_w, int cell_h, uint32_t min_count, int accumulate, void *d_cells, void *d_summary) {
    MI355_CHECK(mi355_cwire_activity_batch(core_, d_cwire, counts, escapes, nstreams, nframes, cell_w, cell_h, min_count, accumulate,
                                           d_cells, d_summary));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::check_multi(const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nrecords, void *d_verdicts) {
    MI355_CHECK(mi355_cwire_check_batch(core_, d_cwire, h_counts, h_escapes, nrecords, d_verdicts));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::digest_multi(const void *d_states, size_t stride, int nstreams, void *d_digests) {
    MI355_CHECK(mi355_state_digest_batch(core_, d_states, stride, nstreams, d_digests));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::refresh_multi(const void *d_states, size_t stride, int nstreams, const void *d_peer_digests, void *d_tile_mask,
                             void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes) {
    MI355_CHECK(mi355_refresh_cwire_batch(core_, d_states, stride, nstreams, d_peer_digests, d_tile_mask, d_offsets, d_frame_pos,
                                          d_cwire_out, capacity_bytes));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::clear_tiles_multi(void *d_states, size_t stride, int nstreams, const void *d_tile_mask) {
    MI355_CHECK(mi355_state_clear_tiles_batch(core_, d_states, stride, nstreams, d_tile_mask));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::wall_compose_multi(const void *d_states, size_t stride, int nstreams, const int32_t *h_place, const void *d_tile_mask,
                                  void *d_wall, int wall_w, int wall_h, size_t wall_pitch) {
    MI355_CHECK(mi355_wall_compose_batch(core_, d_states, stride, nstreams, h_place, d_tile_mask, d_wall, wall_w, wall_h, wall_pitch));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::touched_tiles_multi(const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams, int nframes,
                                   bool accumulate, void *d_tile_mask) {
    MI355_CHECK(mi355_cwire_touched_tiles_batch(core_, d_cwire, h_counts, h_escapes, nstreams, nframes, accumulate ? 1 : 0, d_tile_mask));
    MI355_CHECK(mi355_synchronize(core_));
}

void CUDACore::thumb_cwire_multi(const void *d_states, size_t stride, int nstreams, int k, int threshold, const void *d_tile_mask,
                                 void *d_thumbs, size_t thumb_stride, void *d_offsets, void *d_frame_pos, void *d_cwire_out,
                                 size_t capacity_bytes) {
    MI355_CHECK(mi355_thumb_cwire_batch(core_, d_states, stride, nstreams, k, threshold, d_tile_mask, d_thumbs, thumb_stride, d_offsets,
                                        d_frame_pos, d_cwire_out, capacity_bytes));
    MI355_CHECK(mi355_synchronize(core_));
}

size_t CUDACore::chunkt_size() { return 32; }  // sizeof(long4), kernels.cu:27,527-529

void CUDACore::alloc_arrays(uint8_t **h_frame, uint8_t **n_frame, uint8_t **o_frame, int **h_xs, int r,
                            int c) {
    const size_t n = (size_t)3 * r * c, slack = 32;
    MI355_CHECK(mi355_host_alloc((void **)h_frame, n + slack));
    MI355_CHECK(mi355_host_alloc((void **)n_frame, n + slack));
    MI355_CHECK(mi355_host_alloc((void **)o_frame, n + slack));
    MI355_CHECK(mi355_host_alloc((void **)h_xs, n * sizeof(int) + slack));
}

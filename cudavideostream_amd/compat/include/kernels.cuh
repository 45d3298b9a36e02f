// compat/include/kernels.cuh -- diff::cuda::CUDACore, the MI355X drop-in.
//
// Same class name, namespace and public member functions as the reference's
// server/include/kernels.cuh:13-43, so the reference's server.cpp / threads.cpp link against it
// unchanged (same mangled names).  The reference constructs the object BY VALUE on the caller's stack
// (server/src/server.cpp:53) using its own header, so the object size here must not exceed the
// reference's: the private part is one handle plus padding up to the reference's 160 bytes (LP64)
// instead of the reference's device pointers.  The test harness's layout check
// verifies the size against the reference header whenever the reference tree is present.
#ifndef MI355_COMPAT_KERNELS_CUH_
#define MI355_COMPAT_KERNELS_CUH_

#include <stddef.h>
#include <stdint.h>
#include <string>

#include "utils.hpp"

struct mi355_core;

namespace diff {
namespace cuda {

class CUDACore {
private:
    mi355_core *core_;          // the C-ABI handle (include/mi355diff.h)
    int total_;
    int reserved_int_;
    unsigned char reserved_[144];

public:
    // kernels.cu:377-428: uploads the glyph atlas, the convolution kernel and the base frame.
    CUDACore(uint8_t *charsPx, diff::utils::matsz &charsSz, float *k, int total, uint8_t *sampleMatData,
             diff::utils::matsz &frameSz);
    // kernels.cu:531-536: pinned host buffers (three frames of 3rc bytes + slack, one int[3rc] + slack).
    static void alloc_arrays(uint8_t **h_frame, uint8_t **n_frame, uint8_t **o_frame, int **h_xs, int r, int c);
    // kernels.cu:430-525: one frame in (frameData), diff/xs/count (+ visualisation frame) out.
    void exec_core(uint8_t *frameData, uint8_t *showReadyNData, std::string &text, unsigned int *h_pos,
                   int *h_xs);
    // kernels.cu:527-529
    size_t chunkt_size();

    // ---- additions (not in the reference; non-virtual, the object layout is unchanged) -----------------
    // exec_core split in two so that several frames are in flight (include/mi355diff.h, mi355_pipe_*):
    // the elaboration thread of threads.cpp:134-147 submits frame k, then waits for frame k-1 and hands
    // it to the sender, instead of blocking twice inside exec_core for every frame.
    void pipe_open(int depth);
    long long exec_submit(uint8_t *frameData, uint8_t *showReadyNData, std::string &text, int *h_xs);
    void exec_wait(long long ticket, unsigned int *h_pos);
    void pipe_close();
    // The same three with the frame's changes as ONE compact record in host memory, ready for one write() (include/
    // mi355diff.h, mi355_exec_cwire / mi355_pipe_submit_cwire / mi355_pipe_wait_cwire): frameData is only read, h_record
    // (alloc_record: pinned, record_capacity bytes) takes the record, *h_bytes its length, *h_pos / *h_escapes its header.
    // Plain and compact calls may alternate on one object.
    static void alloc_record(void **h_record, size_t *record_capacity, int r, int c);
    void exec_core_compact(const uint8_t *frameData, uint8_t *showReadyNData, std::string &text, void *h_record,
                           size_t record_capacity, unsigned int *h_pos, unsigned int *h_escapes, size_t *h_bytes);
    long long exec_submit_compact(const uint8_t *frameData, uint8_t *showReadyNData, std::string &text, void *h_record,
                                  size_t record_capacity);
    void exec_wait_compact(long long ticket, unsigned int *h_pos, unsigned int *h_escapes, size_t *h_bytes);
    // One tick of nstreams cameras in one call (include/mi355diff.h, mi355_diff_multi_batch): camera s has its new frame at
    // d_frames + s*stride and its reconstructed-frame state at d_states + s*stride, both in DEVICE memory of the caller
    // (mi355_dev_alloc / hipMalloc); segment s of (d_offsets, d_xs, d_diff) is its packed frame.  Blocking, like exec_core.
    // nstreams <= MI355_MAX_BATCH of the environment when the object was made (default 1: the reference's one stream).
    void exec_multi(const void *d_frames, void *d_states, size_t stride, int nstreams, void *d_offsets, void *d_xs,
                    void *d_diff, size_t capacity);
    // nframes frames of each of nstreams cameras in one call (include/mi355diff.h, mi355_diff_multi_stream_batch): frame t of
    // camera s at d_frames + (s*nframes + t)*stride, its state at d_states + s*stride; segments s*nframes .. (s+1)*nframes - 1
    // of (d_offsets, d_xs, d_diff) are its packed frames.  Blocking, like exec_multi; nstreams*nframes <= MI355_MAX_BATCH.
    void exec_multi_stream(const void *d_frames, void *d_states, size_t stride, int nstreams, int nframes, void *d_offsets,
                           void *d_xs, void *d_diff, size_t capacity);
    // The receiving end of such a tick (include/mi355diff.h, mi355_apply_multi_cwire_batch): the compact record of camera s
    // -- records back to back in DEVICE memory, headers counts[s] / escapes[s] as read from the sockets -- is applied to the
    // frame at d_states + s*stride, which is then the frame to show.  Blocking, like exec_multi; the same nstreams bound.
    void apply_multi(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, void *d_states,
                     size_t stride);
    // The receiving end of a burst (include/mi355diff.h, mi355_apply_multi_stream_cwire_batch): the nframes records of camera s
    // -- records back to back in DEVICE memory, camera-major as exec_multi_stream's sender made them, headers counts[s*nframes
    // + t] / escapes[...] as read from the sockets -- are applied in order to the frame at d_states + s*stride; d_frames_out !=
    // nullptr: the frame after record t also goes to d_frames_out + (s*nframes + t)*out_stride.  Blocking, like apply_multi;
    // nstreams*nframes <= MI355_MAX_BATCH.
    void apply_multi_stream(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                            void *d_states, size_t stride, void *d_frames_out, size_t out_stride);
    // A relay between the two (include/mi355diff.h, mi355_cwire_coalesce_cwire_batch): the nframes records of camera s, laid
    // out and described as for apply_multi_stream, become ONE record per camera -- the sum of the burst's differences per byte,
    // bytes that went back to where they were dropped -- at d_cwire_out + d_frame_pos[s] (uint64[nstreams + 1]), entry counts
    // scanned in d_offsets (uint32[nstreams + 1]); all in DEVICE memory.  No state is involved.  Blocking, like
    // apply_multi_stream; nstreams*nframes <= MI355_MAX_BATCH.
    void coalesce_multi_stream(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                               void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes);
    // The same relay for a viewer that zooms into a camera (include/mi355diff.h, mi355_cwire_crop_cwire_batch): the burst of
    // camera s cut to the rectangle h_rects[s] = {x0, y0, w, h} in pixels and written with the byte indices of the rectangle's own
    // w x h frame (flags = MI355_CROP_KEEP_INDEX: of the full frame), so the viewer holds a w x h frame.  Outputs as
    // coalesce_multi_stream's.  Blocking; nstreams*nframes <= MI355_MAX_BATCH.
    void crop_multi_stream(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                           const int32_t *h_rects, unsigned flags, void *d_offsets, void *d_frame_pos, void *d_cwire_out,
                           size_t capacity_bytes);
    // A multiview relay (include/mi355diff.h, mi355_cwire_mosaic_cwire_batch): the bursts of all the cameras placed side by side
    // into ONE record of a canvas_w x canvas_h canvas, h_place[s] = {sx, sy, w, h, dx, dy} in pixels; the client holds one canvas
    // state and reads one socket.  d_offsets uint32[2], d_frame_pos uint64[2].  Blocking; nstreams*nframes <= MI355_MAX_BATCH, and
    // the canvas may have at most MI355_MAX_BATCH frames' worth of 4096-byte tiles.
    void mosaic_multi_stream(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes,
                             const int32_t *h_place, int canvas_w, int canvas_h, void *d_offsets, void *d_frame_pos,
                             void *d_cwire_out, size_t capacity_bytes);
    // The sender's rate control behind exec_multi's compact form (include/mi355diff.h, mi355_cwire_budget_cwire_batch): record s
    // of the tick just diffed keeps at most budgets[s] entries (mi355_cwire_budget_entries turns a byte budget into one;
    // UINT32_MAX: no limit), the largest changes first: the thinned records go to d_cwire_out + d_frame_pos[s], the threshold that
    // was needed to d_thresholds[s] (uint32[nstreams]), and d_states + s*stride is taken back to the previous value where an entry
    // was dropped, so the change stays pending for a later tick.  All but counts / escapes / budgets in DEVICE memory.  Blocking.
    void budget_multi(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, void *d_states, size_t stride,
                      int nstreams, const uint32_t *budgets, void *d_thresholds, void *d_offsets, void *d_frame_pos,
                      void *d_cwire_out, size_t capacity_bytes);
    // The second lever, keyed on the neighbourhood (include/mi355diff.h, mi355_cwire_despeckle_cwire_batch): an entry of record s
    // stays when at least need[s] (0 .. 8; 0: the record passes through) of the 8 pixels around its pixel changed too.  The kept
    // entries go to d_cwire_out + d_frame_pos[s], the entries dropped per camera to d_dropped (uint32[nstreams]), and d_states +
    // s*stride is taken back to the previous value where an entry was dropped.  Run it before budget_multi when both are wanted.
    // All but counts / escapes / need in DEVICE memory.  Blocking.
    void despeckle_multi(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, void *d_states, size_t stride,
                         int nstreams, const uint32_t *need, void *d_dropped, void *d_offsets, void *d_frame_pos,
                         void *d_cwire_out, size_t capacity_bytes);
    // Where the cameras move (include/mi355diff.h, mi355_cwire_activity_batch): from the nframes records of camera s, laid out
    // and described as for apply_multi_stream, a grid of changed bytes per cell of cell_w x cell_h pixels at d_cells
    // (uint32[nstreams][mi355_activity_cells(...)]) and eight words at d_summary (uint32[nstreams][8]): entries, box x0, y0, x1,
    // y1, cells of at least min_count, peak count, peak cell.  accumulate != 0 adds onto what the two hold.  Both in DEVICE
    // memory; no state is involved.  Blocking, like budget_multi; nstreams*nframes <= MI355_MAX_BATCH.
    void activity_multi(const void *d_cwire, const uint32_t *counts, const uint32_t *escapes, int nstreams, int nframes, int cell_w,
                        int cell_h, uint32_t min_count, int accumulate, void *d_cells, void *d_summary);
    // Before any of the calls above trusts what arrived (include/mi355diff.h, mi355_cwire_check_batch): one verdict of four words
    // per record at d_verdicts (uint32[nrecords][4], DEVICE memory) -- {MI355_CWIRE_BAD_* flags, 0: well-formed and canonical;
    // 255 codes; first entry at or past the frame's end, n: none; 1 + the last index, saturated} -- from the records alone, laid
    // out and described as for apply_multi.  No state is involved.  Blocking; nrecords <= MI355_MAX_BATCH.
    void check_multi(const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nrecords, void *d_verdicts);
    // Resynchronising a receiver (include/mi355diff.h, "Resynchronising a receiver"), all on DEVICE memory, states laid out as for
    // apply_multi.  digest_multi: the receiver's two words per tile of 4096 bytes, uint32[nstreams][tiles][2] (mi355_state_tiles).
    // refresh_multi, the sender: the tiles whose digest differs from d_peer_digests (NULL: every tile) as a mask
    // (uint32[nstreams][ceil(tiles / 32)]) and one ordinary compact record per stream that holds their nonzero bytes, laid out
    // and bounded as coalesce_multi_stream's.  clear_tiles_multi, the receiver again: zeroes the masked tiles; apply_multi of
    // the refresh records then makes them the sender's.  Blocking; nstreams <= MI355_MAX_BATCH.
    void digest_multi(const void *d_states, size_t stride, int nstreams, void *d_digests);
    void refresh_multi(const void *d_states, size_t stride, int nstreams, const void *d_peer_digests, void *d_tile_mask,
                       void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes);
    void clear_tiles_multi(void *d_states, size_t stride, int nstreams, const void *d_tile_mask);
    // A wall of many cameras (include/mi355diff.h, "A wall of many cameras"), all on DEVICE memory but h_place.
    // wall_compose_multi: the box-downscaled thumbnail of each state (laid out as for apply_multi) at scale h_place[s][2]
    // (1 .. 16; 0: not shown) to (h_place[s][0], h_place[s][1]) of the BGR24 wall; d_tile_mask (refresh_multi's or
    // touched_tiles_multi's) limits the repaint to where a selected tile lands, NULL repaints all.  touched_tiles_multi: that mask
    // from the records of a tick or burst, described as for apply_multi_stream; accumulate ORs onto what the mask holds.
    // Blocking; nstreams (* nframes) <= MI355_MAX_BATCH.
    void wall_compose_multi(const void *d_states, size_t stride, int nstreams, const int32_t *h_place, const void *d_tile_mask,
                            void *d_wall, int wall_w, int wall_h, size_t wall_pitch);
    void touched_tiles_multi(const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes, int nstreams, int nframes,
                             bool accumulate, void *d_tile_mask);
    // thumb_cwire_multi: ONE compact record per stream of the thumbnail at scale k (1 .. 16) of each state against the held
    // thumbnail at d_thumbs + s*thumb_stride (3 * ceil(w / k) * ceil(h / k) bytes), which moves where an entry is written; the
    // mask as above, over the full-size states; outputs as for the refresh call.  Blocking; nstreams <= MI355_MAX_BATCH.
    void thumb_cwire_multi(const void *d_states, size_t stride, int nstreams, int k, int threshold, const void *d_tile_mask,
                           void *d_thumbs, size_t thumb_stride, void *d_offsets, void *d_frame_pos, void *d_cwire_out,
                           size_t capacity_bytes);
};

static_assert(sizeof(CUDACore) == 160, "must match the reference's object size (LP64)");

}  // namespace cuda
}  // namespace diff
#endif

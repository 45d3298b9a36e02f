/*
 * mi355diff.h -- C-ABI of libmi355diff.so: the MI355X (gfx950) frame-differencing + filter core.
 *
 * This is the drop-in boundary for the hot path of MatteoBattilana/CUDAVideoStream: everything the
 * reference's `diff::cuda::CUDACore` (server/include/kernels.cuh:13-43, server/src/kernels.cu:377-536)
 * does on the GPU, behind plain C entry points (no C++/STL/torch types).  The C++ class of the same
 * name that the reference's server.cpp links against lives in cudavideostream_amd/compat/ and only
 * forwards to these functions; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - A frame is width*height BGR24 pixels, row-major, N = 3*width*height bytes
 *     (server/src/server.cpp:46).  All arithmetic is per byte, as in the reference.
 *   - "d_" arguments are device (HBM) pointers of the core's device; everything else is host memory.
 *   - One core = one device = one stream = one caller thread at a time (the reference calls exec_core
 *     from a single thread, server/src/server.cpp:139).  Several cores (one per GPU) are independent.
 *   - Every function returns MI355_OK (0) or a negative error; mi355_last_error() gives the text for
 *     the calling thread.  Device-resident entry points are asynchronous on the core's stream and
 *     never synchronise; host-buffer entry points return after the results are in the host buffers.
 *   - There is no CPU fallback: without a usable HIP device mi355_create() fails.
 */
#ifndef MI355DIFF_H_
#define MI355DIFF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_OK 0
#define MI355_ERR_INVALID (-1)  /* bad argument / configuration */
#define MI355_ERR_HIP (-2)      /* a HIP runtime call failed */
#define MI355_ERR_STATE (-3)    /* call not valid in the core's current state */

/* Visualiser selection of exec(): the values of NOISE_VISUALIZER in server/include/common.h:11. */
#define MI355_VIS_NONE 0
#define MI355_VIS_HEAT 1         /* kernels.cu:480  heat_map                      */
#define MI355_VIS_RED 2          /* kernels.cu:513  memset + red_black_map_overlap */
#define MI355_VIS_RED_OVERLAP 3  /* kernels.cu:517  red on the previous frame      */
#define MI355_VIS_GRAY 4         /* kernels.cu:487  grayscale_kernel_v3 (weighted) */
#define MI355_VIS_BINARIZE 5     /* kernels.cu:493-498 gray + histogram + max + binarize */

typedef struct mi355_core mi355_core;

typedef struct mi355_config {
    int32_t width;      /* pixels */
    int32_t height;     /* pixels */
    int32_t threshold;  /* LR_THRESHOLDS, server/include/common.h:14 (20); strict >, 0..255 (255 flags nothing) */
    int32_t max_batch;  /* largest nframes of a *_batch call; sizes the workspace (>= 1) */
    int32_t device;     /* HIP device ordinal, or -1 for the current device */
    int32_t noise_filter; /* != 0: exec() runs the 3x3 convolution first (NOISE_FILTER, common.h:5) */
    int32_t visualizer; /* MI355_VIS_* used by exec() (NOISE_VISUALIZER, common.h:11) */
    int32_t flags;      /* MI355_FLAG_* (below), or 0; unknown bits are refused */
} mi355_config;
/* MI355_FLAG_OWN_QUEUES: the core's streams (its own stream and the two side streams of pipelined batches) are created in the
 * LEAST stream-priority class.  HIP serves the streams of one priority class of a process with at most GPU_MAX_HW_QUEUES (4)
 * hardware queues; a process that also holds a framework's stream pools in the default class -- PyTorch creates 32 per class
 * the moment torch.distributed / RCCL asks for one -- leaves the core's three streams sharing queues, and kernels that are
 * meant to run BESIDE each other (the expansion of batch k and the pack kernel of batch k + 1) run one after the other:
 * 462 k instead of 560-620 k frames/s at 1080p (round 6, profiles/README.md r06k / r06l).  No framework uses the least class,
 * so there the three streams get hardware queues of their own (545-551 k with or without torch.distributed in the
 * process; in a process WITHOUT other streams the default class is 1-2 % faster, hence a flag).  Set it in any process that
 * also runs PyTorch collectives / RCCL / other HIP streams (bench.py does under a launcher). */
#define MI355_FLAG_OWN_QUEUES 1

/* ABI version of this header: bumped whenever an existing entry point changes its argument list (round 3 did that to
 * mi355_group_gather without a marker: a caller built against the older header still linked and passed shifted
 * arguments).  A binding checks mi355_abi_version() == MI355_ABI_VERSION when it loads the library
 * (cudavideostream_amd/lib.py, compat/include/group.hpp do).
 *   3  round 3: mi355_group_gather gained member_capacity (6th argument)
 *   4  round 4: + mi355_abi_version, mi355_probe_clock, mi355_probe_hbm_read (additions only)
 *   5  round 5: + mi355_set_option / mi355_get_option; MI355_FLAG_FUSED / MI355_FLAG_CHAIN (two opt-in experiments) are
 *      gone and cfg.flags must be 0; the environment variables MI355_SPLIT, MI355_DENSE_PCT, MI355_CHAIN_HINT and the
 *      undocumented tuning variables are no longer read (options below); + MI355_OPT_MEDIAN_ROWS, mi355_probe_hbm_write
 *      (additions)
 *   6  round 6: + mi355_prepare, mi355_alloc_outputs, MI355_OPT_SCAN_EPOCH_LEFT, cfg.flags bit MI355_FLAG_OWN_QUEUES (additions only)
 *   7  + the compact wire format: mi355_cwire_frame_bytes, mi355_cwire_bytes_max, mi355_cwire_encode_batch,
 *      mi355_cwire_decode_batch, mi355_cwire_apply_host (additions only)
 *   8  the schedule options 2..5 (split share, dense threshold, filter/batch chain hint, pack grid) are gone: their ids
 *      are refused (MI355_ERR_INVALID) and will not be reused; their defaults are the library's fixed schedule, unchanged
 *      (mi355_diff_stream_batch)
 *   9  + mi355_diff_stream_cwire_batch (additions only)
 *   10 + mi355_apply_cwire_batch (additions only); + mi355_diff_multi_batch, mi355_diff_multi_wire_batch,
 *      mi355_diff_multi_cwire_batch (additions only: no existing argument list changed, so the number stays);
 *      + mi355_apply_multi_batch, mi355_apply_multi_wire_batch, mi355_apply_multi_cwire_batch (additions only);
 *      + mi355_diff_multi_stream_batch, mi355_diff_multi_stream_wire_batch, mi355_diff_multi_stream_cwire_batch (additions
 *      only); + mi355_apply_multi_stream_batch, mi355_apply_multi_stream_wire_batch, mi355_apply_multi_stream_cwire_batch
 *      (additions only); + mi355_cwire_coalesce_batch, mi355_cwire_coalesce_cwire_batch (additions only);
 *      + mi355_exec_cwire, mi355_pipe_submit_cwire, mi355_pipe_wait_cwire, MI355_PREPARE_EXEC_CWIRE (additions only);
 *      + mi355_cwire_budget_cwire_batch, mi355_cwire_budget_entries (additions only);
 *      + mi355_activity_batch, mi355_cwire_activity_batch, mi355_activity_cells (additions only);
 *      + mi355_cwire_check_host, mi355_cwire_check_batch, MI355_CWIRE_BAD_* (additions only);
 *      + mi355_state_tiles, mi355_state_digest_host, mi355_state_digest_batch, mi355_refresh_cwire_batch,
 *      mi355_state_clear_tiles_batch (additions only);
 *      + mi355_wall_thumb_size, mi355_wall_compose_batch, mi355_cwire_touched_tiles_batch (additions only);
 *      + mi355_cwire_crop_batch, mi355_cwire_crop_cwire_batch, MI355_CROP_KEEP_INDEX (additions only);
 *      + mi355_cwire_mosaic_batch, mi355_cwire_mosaic_cwire_batch (additions only);
 *      + mi355_diff_consecutive_batch (additions only);
 *      + mi355_cwire_split_host, mi355_cwire_split_cwire_batch, mi355_cwire_split_pieces_max, mi355_cwire_split_bytes_max,
 *      MI355_CWIRE_SPLIT_BLOCK (additions only);
 *      + mi355_thumb_cwire_host, mi355_thumb_cwire_batch (additions only);
 *      + mi355_cwire_fec_* (additions only);
 *      + mi355_cwire_runs_frame_bytes, mi355_cwire_runs_bytes_max, mi355_cwire_runs_encode_host, mi355_cwire_runs_encode_batch,
 *      mi355_cwire_runs_decode_host, mi355_cwire_runs_decode_batch, MI355_RUNS_* (additions only);
 *      + mi355_cwire_despeckle_host, mi355_cwire_despeckle_cwire_batch, MI355_PREPARE_DESPECKLE (additions only) */
#define MI355_ABI_VERSION 10
int mi355_abi_version(void);

/* ---- life cycle: CUDACore::CUDACore (kernels.cu:377-428) without the uploads ------------------ */
int mi355_create(const mi355_config *cfg, mi355_core **out);
void mi355_destroy(mi355_core *core);
const char *mi355_last_error(void);
/* Size in bytes of one frame (3*width*height). */
size_t mi355_frame_bytes(const mi355_core *core);
/* Bytes of HBM workspace held by the core (state, logs, counters).  The logs are sized for the worst case (every byte
 * of every frame of a batch changed): about (1 + 1/3) * max_batch * N bytes, 2.07 GB for 1080p and max_batch 256.  The
 * first asynchronous batch call on the core's own stream allocates a second set (hipMalloc + hipMemset inside that
 * call: it is not asynchronous) for the pipelined mode below; scratch buffers of the fused gray+binarize chain and of
 * the cleared red map are likewise allocated by the first call that needs them -- unless mi355_prepare has made them. */
size_t mi355_workspace_bytes(const mi355_core *core);
/* Makes NOW what the entry points would otherwise make on first use -- so that no hipMalloc / hipMemset / stream or event
 * creation happens inside an asynchronous entry point and a server's first frames do not stall.  `what` is a mask:
 *   MI355_PREPARE_BATCHES      second set of logs, side streams and events of pipelined own-stream batches
 *                              (mi355_diff_stream_batch / _pairs_batch / _wire_batch on the core's own stream);
 *   MI355_PREPARE_GRAY_CHAIN   one gray byte per pixel for max_batch frames (MI355_OP_GRAY_*_BINARIZE, MI355_VIS_BINARIZE);
 *   MI355_PREPARE_RED_CLEAR    slice bounds of mi355_red_stream_batch(clear != 0);
 *   MI355_PREPARE_CONV_KXK     the tap buffer of mi355_conv_kxk;
 *   MI355_PREPARE_EXEC         one pass of mi355_exec's own kernels (noise filter if its kernel is set, visualiser, pack,
 *                              index, expansion, red map, export) over a copy of the CURRENT state -- nothing differs, so
 *                              the state and the caller's buffers stay as they are -- so that the first real frame does
 *                              not pay for the first use of each kernel (measured: the first exec_core of a fresh core
 *                              1.4 ms, the later ones 0.16).  The C++ drop-in's constructor calls it.
 *   MI355_PREPARE_EXEC_CWIRE   the record buffer (mi355_cwire_bytes_max(N, 1) bytes) and the pinned result words of
 *                              mi355_exec_cwire / mi355_pipe_submit_cwire, and one pass of their encode and export kernels on
 *                              an empty frame.  Not part of MI355_PREPARE_ALL: only a caller of the compact per-frame form
 *                              wants it, and asks for it by name.
 *   MI355_PREPARE_DESPECKLE    the pixel bitmaps of mi355_cwire_despeckle_cwire_batch: 2 * max_batch * 4 * ceil(width*height / 32)
 *                              bytes (133 MB at 1080p with max_batch 256).  Not part of MI355_PREPARE_ALL for that size: only
 *                              a caller of that call wants them, and asks by name (or lets its first call make them).
 * mi355_create already makes the one a per-frame server needs (MI355_VIS_BINARIZE's gray bytes).  Blocking; idempotent;
 * mi355_workspace_bytes grows by what was made.  After mi355_prepare(core, MI355_PREPARE_ALL) no entry point of the core
 * allocates (mi355_pipe_open and mi355_set_glyphs, which say so, excepted -- and the first mi355_exec_cwire /
 * mi355_pipe_submit_cwire, unless MI355_PREPARE_EXEC_CWIRE, which MI355_PREPARE_ALL does not contain, was asked for too). */
#define MI355_PREPARE_BATCHES 1u
#define MI355_PREPARE_GRAY_CHAIN 2u
#define MI355_PREPARE_RED_CLEAR 4u
#define MI355_PREPARE_CONV_KXK 8u
#define MI355_PREPARE_EXEC 16u
#define MI355_PREPARE_ALL 31u
#define MI355_PREPARE_EXEC_CWIRE 32u
#define MI355_PREPARE_DESPECKLE 64u
int mi355_prepare(mi355_core *core, unsigned what);

/* Streams.  A core starts on a stream of its own, created hipStreamNonBlocking: it is NOT ordered against the
 * legacy default stream nor against any other stream of the caller.  Buffers the caller fills asynchronously on
 * another stream (hipMemcpyAsync, a framework's kernels) must be complete -- hipStreamSynchronize / an event the
 * caller waits for -- before an asynchronous entry point of the core reads them, and the caller must
 * mi355_synchronize (or use the blocking entry points) before it reads the outputs on another stream.
 * mi355_set_stream makes the core enqueue on an existing hipStream_t instead (e.g. PyTorch's current stream; NULL is
 * the default stream), so that the caller's own work on that stream is ordered with the core's; mi355_use_own_stream
 * goes back.  Both wait for the work already queued on the stream being left (all batches of a core share one
 * workspace). */
int mi355_set_stream(mi355_core *core, void *hip_stream);
int mi355_use_own_stream(mi355_core *core);
int mi355_synchronize(mi355_core *core);
/* Lifetime of the caller's buffers.  The device-resident entry points are asynchronous: every d_ buffer handed to one
 * (inputs AND outputs) must stay allocated, and the inputs unmodified, until the work has completed -- mi355_synchronize,
 * or, with mi355_set_stream, the caller's own synchronisation of that stream.  A framework whose allocator recycles a
 * freed tensor for other kernels on ITS stream (PyTorch's caching allocator) must keep the tensors referenced until
 * then: on the core's own stream the library's kernels are not ordered against the framework's stream.
 * (cudavideostream_amd/core.py holds such references itself until synchronize().) */

/* Options.  The pipelining of the batches on the core's own stream can be switched off per core; two more options are
 * seams for the tests.  RESULTS never depend on any of them.  Changing an option first waits for the work the core has
 * queued; an unknown id (2..5 included: options of ABI version 7 and earlier) is refused with MI355_ERR_INVALID.
 * Of the environment the library reads two variables and nothing else: MI355_PIPELINE=0 makes MI355_OPT_PIPELINE default to 0 for every core of the process (a switch for
 * the operator of an unmodified server binary); and, in the multi-GPU entry points only, MI355_RCCL_LIB=path names
 * another library with the ten RCCL entry points they bind instead of librccl.so.1 (the tests' stand-ins, which let
 * several ranks share the one GPU of a test box). */
#define MI355_OPT_PIPELINE 1     /* 1 (default): own-stream batches are pipelined (below); 0: one kernel after the other */
#define MI355_OPT_MEDIAN_ROWS 6  /* tests only: 0 (default): the 5x5 median's column-strip kernel walks bands of 5..60
                                  * rows, chosen per launch (from 20 rows up the length that wastes least of the frame's last pair of bands; shorter
                                  * when that makes fewer than a few thousand waves); 5, 10, .. 60: this many */
#define MI355_OPT_SCAN_EPOCH_LEFT 7 /* tests only: launches of the index kernel left before its 33-bit launch tag wraps (the
                                  * totals are then cleared behind a synchronisation and the tag restarts at 1); set: 1..2^30 */
int mi355_set_option(mi355_core *core, int option, int value);
int mi355_get_option(mi355_core *core, int option, int *value);

/* ---- state: the reconstructed client frame ("previous" with negative feedback) ------------------
 * kernels.cu:406 uploads the base frame into d_current; after each frame the surviving buffer is
 * cur where |df| > threshold and prev elsewhere (kernels.cu:312-331, tests/cuda_streaming/test.cu:571).
 * The core keeps ONE persistent state buffer with exactly those contents. */
int mi355_set_state(mi355_core *core, const uint8_t *host_frame);
int mi355_get_state(mi355_core *core, uint8_t *host_frame);
void *mi355_state_device_ptr(mi355_core *core);

/* ---- constants: cudaMemcpyToSymbol(dev_k) kernels.cu:394, glyph upload kernels.cu:381-382 ------ */
int mi355_set_conv_kernel(mi355_core *core, const float *k9);
int mi355_set_glyphs(mi355_core *core, const uint8_t *chars_px, int nglyphs, int glyph_h, int glyph_w,
                     const char *charset);

/* ---- the hot path, device resident ---------------------------------------------------------------
 * kernel2 (kernels.cu:289-334) over a batch.  For every frame t (in order) and every byte i
 * (ascending): df = frame[t][i] - state[i]; if |df| > threshold emit (xs = i, diff = (uint8)df) and
 * state[i] = frame[t][i].  Output is the CPU path's order (tests/cuda_streaming/test.cu:563-573),
 * not the reference kernel's atomicInc order.
 *   d_frames : nframes frames, frame t at d_frames + t*stride_bytes (stride_bytes >= N; the fast
 *              path needs d_frames and stride_bytes to be multiples of 16)
 *              Strides and pitches -- every stride_bytes, out_stride_bytes and wall_pitch of this
 *              header -- are bounded from below only (>= N; the wall pitch >= 3*wall_w); from above
 *              only the address space bounds them: every index * stride is a 64-bit product, and
 *              tests/test_far_strides_gpu.py runs every strided entry point (the mi355_group_diff_*
 *              calls excepted: the same kernels) on windows 4 GiB and more apart, one slab per
 *              camera.  One speed cliff: the pack kernel's vector path reads a group of frames
 *              through one 32-bit window and needs 3*stride_bytes + N < 2^32; a larger stride takes
 *              the byte path (the one unaligned operands take), with identical results and slower.
 *              By how much has not been measured.
 *              The top of the range mi355_create accepts is tested in tests/test_top_of_range_gpu.py:
 *              diff batches of 65535, 65536, 65537 and 131073 frames or streams (the expansion kernels
 *              take the whole batch as one grid dimension, above 65535 too); log offsets from 2^31
 *              to 9216 bytes below 2^32 (1000x700 at max_batch 1100 and 2045, the largest accepted);
 *              batch totals of 2^31 entries and more with d_xs past 8 GiB, plain-wire positions and
 *              RECORD positions (d_frame_pos) past 2^32 -- 4.6 GB of records written by
 *              mi355_diff_stream_cwire_batch and read by the apply, check, decode, multi-stream apply,
 *              coalesce, crop, activity and touched-tiles calls.
 *   d_offsets: uint32[nframes+1], exclusive scan of the per-frame counts (offsets[0] = 0)
 *   d_xs     : int32[capacity]  byte indices, frame t's entries at [offsets[t], offsets[t+1])
 *   d_diff   : uint8[capacity]  (uint8)df of the same entries
 * Entries beyond `capacity` are dropped (offsets stay exact), so check offsets[nframes] <= capacity.
 * Asynchronous.  On the core's OWN stream consecutive batches are pipelined: the index and the expansion of a
 * batch run on a side stream beside the next batch's pack kernel.  A batch's outputs (d_offsets, d_xs, d_diff,
 * d_wire) are complete after mi355_synchronize and for every later call on this core that can consume them
 * (mi355_apply_*, mi355_red_stream_batch / _red_overlap, mi355_merge_parts, mi355_cwire_encode_batch /
 * mi355_cwire_decode_batch / mi355_apply_cwire_batch, mi355_download, mi355_exec / mi355_pipe_*, the group gather) -- these first wait for the last
 * expansion.  The frame filters (mi355_filter_batch,
 * mi355_gray_*, mi355_binarize_chain, mi355_heat_map, mi355_red_dense, mi355_conv*, mi355_median5x5,
 * mi355_int_diff) take frames, not packed streams, and are ordered on the core's stream only: they may run beside
 * the expansion of the batch before (visualiser of frame k + 1 beside the expansion of frame k).  With a caller's
 * stream (mi355_set_stream) nothing is pipelined: every kernel runs on that stream, in call order.
 * MI355_OPT_PIPELINE 0 (or MI355_PIPELINE=0 in the environment) switches the pipelining off.  A pipelined batch is packed
 * on 4 workgroups per CU; a frame of 64 tiles (64 KiB) or more is packed by two kernel launches on two streams of the
 * core, the first half of the tiles (rounded down to a multiple of 4) and the rest, each with its share of that grid.
 * A batch that follows a frame filter on this core (the server's visualiser or noise filter in front of every diff) is not
 * overlapped: one kernel after the other measured faster for such chains.
 * The overlap is adaptive: a batch in which more than 40 % of the bytes changed (a scene change) has an expansion longer
 * than its pack kernel and loses by running beside the next batch.  The index kernel of every own-stream
 * batch leaves the batch's total in a word of pinned host memory; the library, without ever waiting for it, runs batches
 * one after the other while the latest total that has arrived says "dense".  Only the schedule depends on it, never a result.
 * Cache policy: the frames of a stream are read, and every output (d_xs, d_diff, d_wire; the visualiser frames of the
 * filters) is written, with non-temporal instructions -- each is touched once.  A consumer that reads the packed stream
 * right behind the batch (mi355_apply_*, the red map, the gather) reads it from memory, not from the caches. */
int mi355_diff_stream_batch(mi355_core *core, const void *d_frames, size_t stride_bytes, int nframes,
                            void *d_offsets, void *d_xs, void *d_diff, size_t capacity);

/* Stateless form (tests/algorithms_benchmarks.cu style frame pairs): frame t is compared with
 * d_prev + t*stride_bytes instead of the state; the core's state is neither read nor written.
 * The two operands may overlap in any way (pairs of consecutive frames of one buffer: d_prev = frames,
 * d_cur = frames + stride).  The library looks at the addresses: operands that share a frame are read through the
 * caches (the second read of a frame hits), operands that share none -- separate buffers, or the pairs (f - 1, f) of
 * every 8th f that a round-robin shard diffs -- with non-temporal loads. */
int mi355_diff_pairs_batch(mi355_core *core, const void *d_cur, const void *d_prev,
                           size_t stride_bytes, int nframes, void *d_offsets, void *d_xs,
                           void *d_diff, size_t capacity);

/* Consecutive frames, stateless, every frame read ONCE: frame 0 is compared with the one frame at d_first_prev,
 * frame t >= 1 with frame t-1 of d_frames (d_frames + (t-1)*frame_step_bytes; frame_step_bytes is the distance between two
 * frames in bytes, with the rules of every stride_bytes of this header: >= the frame's bytes, bounded above by the address
 * space alone, a multiple of 16 for the fast path).  No feedback: the comparand of frame t+1 is
 * frame t itself, not a reconstructed state (the reference's stateless benchmark, tests/algorithms_benchmarks.cu:24-40,
 * run over a recorded sequence; the reference keeps the previous frame resident and swaps, server/src/kernels.cu:451 --
 * here a wave keeps the previous frame of its tile in registers, as the stream kernel keeps the state).  For every t in
 * order and every byte i ascending: df = frame[t][i] - prev[t][i]; |df| > threshold emits (i, (uint8)df).
 * The output is bit for bit that of mi355_diff_pairs_batch(d_cur = d_frames, prev = {d_first_prev, d_frames,
 * d_frames + frame_step_bytes, ...}) if such a prev could be expressed; with d_first_prev == d_frames - frame_step_bytes it IS
 * mi355_diff_pairs_batch(core, d_frames, d_frames - frame_step_bytes, ...), d_offsets included, with every frame loaded
 * once instead of twice (measured 14 to 19 % faster per pair at 4K and 1080p, profiles/pair_consecutive.json; the bytes
 * fetched from memory drop by 4 % only, the pair form's second load of a frame hits in the L2).
 * The core's state is neither read nor written, and nothing at d_first_prev or in d_frames is written.  d_first_prev may
 * lie anywhere readable: inside the frames' buffer (a ring), in another buffer (the last frame of the block before, for a
 * rank that takes frames [rB, (r+1)B) of a sequence plus one predecessor), or be mi355_state_device_ptr(core).
 * Capacity, drop, alignment (d_first_prev counts as an operand: off 16 bytes it sends the batch down the byte path) and
 * d_offsets rules, the ordering and pipelining on the core's own stream (the two launches at 64 tiles and more included)
 * and the behaviour on a caller's stream are those of mi355_diff_pairs_batch.  MI355_ERR_INVALID, before anything is
 * launched or written: a null d_first_prev or d_frames with nframes > 0 and a frame of more than 0 bytes; nframes outside
 * [0, max_batch]; frame_step_bytes < frame bytes; null outputs where mi355_diff_pairs_batch refuses them.  nframes == 0
 * writes offsets[0] = 0.  mi355_diff_pairs_batch does not route itself here, whatever its operands. */
int mi355_diff_consecutive_batch(mi355_core *core, const void *d_first_prev, const void *d_frames,
                                 size_t frame_step_bytes, int nframes,
                                 void *d_offsets, void *d_xs, void *d_diff, size_t capacity);

/* ---- the stream either side of the path ---------------------------------------
 * Wire form of mi355_diff_stream_batch: instead of separate (xs, diff) arrays the batch leaves as the exact
 * byte stream the reference's sender thread writes per frame (server/src/threads.cpp:227-229):
 *     u32 n (= h_pos) | i32 xs[n] | u8 diff[n]
 * frames back to back, frame t at byte 4*t + 5*offsets[t] of d_wire; mi355_wire_bytes(nframes,
 * offsets[nframes]) bytes in all, ready for one write() to the socket after the base frame
 * (threads.cpp:224, mi355_get_state before the first batch).  A frame that does not fit in capacity_bytes
 * is dropped whole (its header is still written when it fits); d_offsets is exact regardless. */
int mi355_diff_stream_wire_batch(mi355_core *core, const void *d_frames, size_t stride_bytes, int nframes,
                                 void *d_offsets, void *d_wire, size_t capacity_bytes);
size_t mi355_wire_bytes(int nframes, uint64_t entries);
/* Compact form of the same batch (the record layout is under "compact wire format" below): the batch leaves as the records
 * mi355_cwire_encode_batch would write from mi355_diff_stream_batch's (d_offsets, d_xs, d_diff), byte for byte, without those
 * arrays.  Threshold, negative feedback and the state are those of mi355_diff_stream_batch on the same frames, and d_offsets
 * (uint32[nframes + 1]) is the same.  Frame t's record is at byte d_frame_pos[t] (uint64[nframes + 1], exclusive scan of the
 * record sizes, always exact); it is written only if d_frame_pos[t + 1] <= capacity_bytes, a frame that does not fit is
 * skipped whole, header included.  mi355_cwire_bytes_max(N, nframes) always suffices.  nframes <= max_batch; d_cwire and
 * d_offsets 4-byte aligned, d_frame_pos 8-byte aligned; anything else is refused (MI355_ERR_INVALID) before anything is
 * written.  Ordering and pipelining are those of mi355_diff_stream_batch: outputs complete after mi355_synchronize and for
 * every later consumer on this core.  The expansion runs four kernels on the batch's log (the stores are non-temporal); it
 * adds max_batch * (16 * ceil(N / 16384) + 4) bytes of workspace, allocated with the core (about 1.6 MB at 1080p with
 * max_batch 256). */
int mi355_diff_stream_cwire_batch(mi355_core *core, const void *d_frames, size_t stride_bytes, int nframes,
                                  void *d_offsets, void *d_frame_pos, void *d_cwire, size_t capacity_bytes);

/* ---- many streams, one frame each ("many cameras per GPU") ---------------------------
 * One tick of nstreams independent streams in ONE call: stream s (0 <= s < nstreams <= max_batch) has its new frame at
 * d_frames + s*stride_bytes and its state -- the frame its clients have reconstructed, kept in the CALLER's memory -- at
 * d_states + s*stride_bytes.  For every s and every byte i (ascending) exactly what mi355_diff_stream_batch(nframes = 1)
 * does on a core whose state is states[s]: df = frame[s][i] - state[s][i]; if |df| > threshold emit (i, (uint8)df) into
 * segment s and set state[s][i] = frame[s][i].  The core's own state is neither read nor written.
 * The outputs are those of the single-stream forms with "frame t" read as "stream s": d_offsets is uint32[nstreams + 1];
 * the wire form holds {u32 n, i32 xs[n], u8 diff[n]} per stream, stream s at byte 4*s + 5*offsets[s]; the compact form one
 * record per stream at d_frame_pos[s].  Capacity, drop and alignment rules and mi355_cwire_bytes_max(N, nstreams) are
 * unchanged; when the outputs overflow the states still advance completely.  A per-stream consumer slices segment s out
 * for that camera's socket; a late joiner is served with mi355_download of states[s] as its base frame.
 * Refused (MI355_ERR_INVALID) before anything is launched or written: a null d_frames or d_states with nstreams > 0,
 * nstreams outside [0, max_batch], stride_bytes < N, states [d_states, d_states + (nstreams-1)*stride_bytes + N) that overlap
 * the frames' region of the same shape, and whatever the single-stream form refuses.  nstreams == 0 writes offsets[0] = 0
 * (and frame_pos[0] = 0).  The fast path needs d_frames, d_states and stride_bytes to be multiples of 16; anything else
 * goes the byte path.  Bytes of the states' region outside the N bytes of each state are never written.
 * The pack kernel is the pair form with a write-back: a lane stores its 16 state bytes only if one of them changed, so
 * the write traffic follows the changes, not N.  The frames are read with non-temporal loads, the states with plain loads
 * (they are read again one tick later) and written with non-temporal stores.
 * Ordering is that of mi355_diff_stream_batch with the caller's states in the place of the core's: asynchronous; on the
 * core's own stream ticks are pipelined and the next tick on the same (d_states, stride_bytes) sees every state byte the
 * tick before wrote, split launches included; every later entry point of this core that reads the states (mi355_download,
 * a frame filter, mi355_diff_pairs_batch, a tick on other states) finds them complete; with a caller's stream everything
 * runs on it in call order.  Work of the CALLER on another stream (the upload of the next frames, a copy of a state) is
 * ordered by the caller: mi355_synchronize first. */
int mi355_diff_multi_batch(mi355_core *core, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                           void *d_offsets, void *d_xs, void *d_diff, size_t capacity);
int mi355_diff_multi_wire_batch(mi355_core *core, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                                void *d_offsets, void *d_wire, size_t capacity_bytes);
int mi355_diff_multi_cwire_batch(mi355_core *core, const void *d_frames, void *d_states, size_t stride_bytes, int nstreams,
                                 void *d_offsets, void *d_frame_pos, void *d_cwire, size_t capacity_bytes);
/* ---- many streams, many frames each (recorded streams, buffered ticks, a camera that catches up) ----------------------
 * nframes frames of each of nstreams independent streams in ONE call: frame t of stream s is at
 * d_frames + (s*nframes + t)*stride_bytes (stream-major), stream s's state -- in the CALLER's memory -- at
 * d_states + s*stride_bytes.  For every s the frames t = 0 .. nframes - 1 are processed in order, and the result is exactly
 * what mi355_diff_stream_batch(nframes) leaves on a core whose state is states[s]: threshold, negative feedback, ascending
 * indices; afterwards states[s] is that core's state.  The core's own state is neither read nor written.  With
 * nstreams == 1 this is the stream form on a caller-held state, with nframes == 1 it is mi355_diff_multi_*.
 * The outputs are those of the single-stream forms with batch index b = s*nframes + t in the place of "frame t":
 * d_offsets is uint32[nstreams*nframes + 1]; the wire form holds {u32 n, i32 xs[n], u8 diff[n]} of batch index b at byte
 * 4*b + 5*offsets[b]; the compact form its record at d_frame_pos[b] (uint64[nstreams*nframes + 1]).  The nframes frames of
 * a stream are therefore ONE contiguous slice of every output: one write() per socket.  Capacity, drop and alignment rules
 * are unchanged and mi355_cwire_bytes_max(N, nstreams*nframes) always suffices; when the outputs overflow the states still
 * advance completely.
 * Refused (MI355_ERR_INVALID) before anything is launched or written: a null core, a negative nstreams or nframes,
 * nstreams*nframes > max_batch, a null d_frames or d_states with nstreams*nframes > 0, stride_bytes < N, states
 * [d_states, d_states + (nstreams-1)*stride_bytes + N) that overlap the frames
 * [d_frames, d_frames + (nstreams*nframes-1)*stride_bytes + N), and whatever the single-stream form of the same output
 * refuses.  nstreams*nframes == 0 writes offsets[0] = 0 (and frame_pos[0] = 0) and nothing else.  Bytes of the states'
 * region outside the N bytes of each state are never written, the gap of the stride included; the frames are only read.
 * The fast path needs d_frames, d_states and stride_bytes to be multiples of 16; anything else goes the byte path with
 * identical results.
 * The pack kernel is the STREAM form (one wave keeps its tile's state in registers and reads N bytes per frame, not 2N) with
 * the register-held state exchanged every nframes frames: states[s] is read once (plain loads, prefetched with the frames
 * of the register group the exchange falls into) and written once per call (non-temporal stores, only by lanes whose 16
 * bytes changed during the stream's frames).  Per frame it reads N + N/nframes bytes where nframes calls of
 * mi355_diff_multi_* read 2N, and it is one launch sequence instead of nframes.  No workspace beyond the core's; nothing
 * is allocated inside the call.
 * Ordering is that of mi355_diff_multi_batch: asynchronous; pipelined on the core's own stream, split launches included; the
 * next call on the same (d_states, stride_bytes) -- of this form or of mi355_diff_multi_*, the two may alternate without a
 * synchronisation -- sees every state byte this one wrote; every later entry point of the core that reads the states finds
 * them complete; with a caller's stream everything runs on it in call order.
 * Measured (profiles/multi_stream.json: 1080p, webcam-like input, compact form, microseconds per frame, median of five
 * rounds; T calls of mi355_diff_multi_cwire_batch on the same frames / S cores with mi355_diff_stream_cwire_batch(T) in
 * brackets): S = 4: T = 4 5.50 (25.4 / 12.8), T = 16 3.79 (25.4 / 4.12), T = 64 3.41 (25.5 / 3.00); S = 16: T = 4 3.99
 * (8.82 / 12.8), T = 16 3.33 (8.83 / 4.84), T = 64 3.51 in two calls (8.93 / 3.04).  DESIGN.md section 4, "K1, segmented
 * stream form". */
int mi355_diff_multi_stream_batch(mi355_core *core, const void *d_frames, void *d_states, size_t stride_bytes,
                                  int nstreams, int nframes, void *d_offsets, void *d_xs, void *d_diff, size_t capacity);
int mi355_diff_multi_stream_wire_batch(mi355_core *core, const void *d_frames, void *d_states, size_t stride_bytes,
                                       int nstreams, int nframes, void *d_offsets, void *d_wire, size_t capacity_bytes);
int mi355_diff_multi_stream_cwire_batch(mi355_core *core, const void *d_frames, void *d_states, size_t stride_bytes,
                                        int nstreams, int nframes, void *d_offsets, void *d_frame_pos, void *d_cwire,
                                        size_t capacity_bytes);
/* The receiving end of such a tick, client/opencv.cpp:50-66 for nstreams cameras in ONE call: segment or record s
 * (0 <= s < nstreams <= max_batch) is applied to the N bytes at d_states + s*stride_bytes -- for each of its entries
 * state[s][x] += diff (uint8 wrap-around) -- exactly what mi355_apply_batch / _wire_batch / _cwire_batch with nframes = 1 does
 * on a client core whose state is states[s].  The core's own state is neither read nor written, and there is no
 * d_frames_out: the caller's state is the frame to show.
 * The inputs have the layout of the outputs of mi355_diff_multi_*: d_offsets is uint32[nstreams + 1] over (d_xs, d_diff); the
 * wire form holds stream s at byte 4*s + 5*sum(h_counts[0..s)); the compact records lie back to back where h_counts[s] = n
 * and h_escapes[s] = e put them.  The headers come from the host, as the client read them from the sockets; the header
 * words in the buffer are skipped, not trusted.  A receiver that reads nstreams sockets stages the records back to back
 * itself; a camera that sent nothing this tick is an n = 0 record (8 bytes compact, 4 bytes wire) whose contents are
 * never read.
 *   Written bytes: bytes of the states' region outside the N bytes of each state are never written, the stride gap
 *   included, and record s never changes a byte of states[r], r != s -- also with stride_bytes == N and N no multiple of
 *   4: every read-modify-write is of single bytes, or of a tile that lies within its state.
 *   d_states and stride_bytes may have any alignment; the compact form moves whole 16-byte words when both are multiples
 *   of 16, bytes otherwise.
 *   Well-formed records: every state is bit-identical to mi355_cwire_apply_host on that stream's record, and to the
 *   one-stream GPU forms on a core that holds that state.
 *   Malformed compact content under consistent headers: the guarantees of mi355_apply_cwire_batch -- nothing is read
 *   outside the records' span, nothing is written outside the nstreams states, an escape ranked at or past e and an index
 *   >= N change nothing; beyond that only the malformed stream's own state is unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: a null core; nstreams outside [0, max_batch];
 *   with nstreams > 0 a null input pointer, a null d_states or stride_bytes < N; h_escapes[s] > h_counts[s]; h_counts[s]
 *   > N; d_cwire (arrays form: d_offsets or d_xs) not 4-byte aligned; wire and compact forms: an input span, known from
 *   the host's headers, that overlaps the states' region [d_states, d_states + (nstreams-1)*stride_bytes + N).
 *   nstreams == 0 does nothing and returns MI355_OK.
 * Asynchronous on the core's stream.  Like every other consumer of a packed stream the call first waits for the last
 * expansion of this core: mi355_diff_multi_cwire_batch followed by mi355_apply_multi_cwire_batch on the same core (a relay
 * that checks what it forwards) needs no synchronisation in between.  Every later entry point of this core that reads
 * the states finds them complete; with a caller's stream everything runs on it in call order.
 * The compact form runs the directory kernels of mi355_apply_cwire_batch on the nstreams records and then ONE kernel on a
 * grid of 4096-byte tiles x streams: a tile that no entry of its record lands in -- the directory says so before a state
 * byte is touched -- is neither read nor written, the others are loaded, updated and stored back with non-temporal
 * stores.  Traffic on the states is 2 * 4096 bytes per touched tile, not 2N per stream.  Six launches and one more per
 * 128 streams, whatever nstreams; the arrays form is one launch (a lane finds its segment by binary search in the
 * offsets), the wire form one per 128 streams.  No workspace beyond the scratch of mi355_apply_cwire_batch, which is sized
 * for max_batch records.
 * Measured (profiles/multi_client.json: 1080p, webcam-like input, microseconds per stream and tick, S = 4 / 16 / 64): the
 * compact form 7.537 / 3.544 / 2.972 against 22.841 / 22.355 / 22.863 for S client cores calling
 * mi355_apply_cwire_batch(nframes = 1) each.  That input touches all 1519 tiles of every state (its changes are sensor noise
 * over the whole picture), so there the states still move 2N per stream; the tile skip pays on local changes. */
int mi355_apply_multi_batch(mi355_core *core, const void *d_offsets, const void *d_xs, const void *d_diff,
                            int nstreams, void *d_states, size_t stride_bytes);
int mi355_apply_multi_wire_batch(mi355_core *core, const void *d_wire, const uint32_t *h_counts,
                                 int nstreams, void *d_states, size_t stride_bytes);
int mi355_apply_multi_cwire_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts,
                                  const uint32_t *h_escapes, int nstreams, void *d_states,
                                  size_t stride_bytes);
/* The receiving end of a burst, the counterpart of mi355_diff_multi_stream_*: nframes segments or records of each of nstreams
 * streams are applied to nstreams states in the CALLER's memory in ONE call, straight from the stream-major layout the
 * sockets delivered.  The batch index is b = s*nframes + t and the inputs have exactly the layout of the outputs of
 * mi355_diff_multi_stream_*: d_offsets is uint32[nstreams*nframes + 1] over (d_xs, d_diff); the wire form holds
 * {u32 n, i32 xs[n], u8 diff[n]} of index b at byte 4*b + 5*sum(h_counts[0..b)); the compact records lie back to back in b
 * order where h_counts[b] = n and h_escapes[b] = e put them.  The headers come from the host; the header words in the buffer
 * are skipped, not trusted, as in mi355_apply_multi_*.
 * For every s the records t = 0 .. nframes - 1 are applied in order to the N bytes at d_states + s*stride_bytes (state[x] +=
 * diff, uint8 wrap-around): bit-identical to mi355_apply_batch / _wire_batch / _cwire_batch(nframes) on a client core whose
 * state is states[s], to mi355_cwire_apply_host on that stream's slice, and to nframes ticks of mi355_apply_multi_* on
 * re-staged records.  With nframes == 1 it is mi355_apply_multi_*, with nstreams == 1 the one-stream client on a caller-held
 * state.  The core's own state is neither read nor written.
 * d_frames_out != NULL: the frame of stream s after record t is also written to d_frames_out + b*out_stride_bytes (N bytes
 * each, the gap of the stride is never written; any alignment works, whole 16-byte stores when the pointer and the stride
 * are multiples of 16) -- what a video wall or a recorder shows between the ends of a burst.  NULL: only the states advance
 * and out_stride_bytes is ignored.
 *   Written bytes: nothing outside the N bytes of each state and of each output frame; record (s, t) never changes a byte
 *   of states[r], r != s -- also with stride_bytes == N and N no multiple of 4 or 16.
 *   Malformed compact content under consistent headers: the guarantees of mi355_apply_multi_cwire_batch -- nothing is read
 *   outside the records' span, nothing is written outside the states and the output frames, an escape ranked at or past e
 *   and an index >= N change nothing; beyond that only the malformed stream's own state and frames are unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: a null core; a negative nstreams or nframes;
 *   nstreams*nframes > max_batch (the directory scratch of mi355_apply_cwire_batch holds max_batch records); with
 *   nstreams*nframes > 0 a null input pointer, a null d_states or stride_bytes < N; out_stride_bytes < N with d_frames_out
 *   set; h_escapes[b] > h_counts[b]; h_counts[b] > N; d_cwire (arrays form: d_offsets or d_xs) not 4-byte aligned; any
 *   overlap between two of the states' region [d_states, d_states + (nstreams-1)*stride_bytes + N), the output frames
 *   [d_frames_out, d_frames_out + (nstreams*nframes-1)*out_stride_bytes + N) and -- wire and compact forms -- the input span
 *   known from the host's headers.  nstreams*nframes == 0 does nothing and returns MI355_OK.
 * Ordering is that of mi355_apply_multi_*: asynchronous on the core's stream, behind the last expansion of this core, so
 * mi355_diff_multi_stream_cwire_batch followed by this call on one core needs no synchronisation; every later entry point
 * of the core that reads the states or the output frames finds them complete; with a caller's stream everything runs on it
 * in call order.  Nothing is allocated inside the call.
 * The compact form runs the directory kernels of mi355_apply_cwire_batch on the nstreams*nframes records and then ONE
 * kernel on a grid of 4096-byte tiles x streams: a wave finds the records of its stream that have an entry in its tile
 * (one lane per record, one ballot per 64 records) before a state byte is touched; with no output frames a tile that no
 * record lands in is neither read nor written; the others are loaded once, the records that touch them are applied in
 * order in LDS, and the tile is stored back once, non-temporal.  State traffic per touched tile is 2 * 4096 bytes per
 * CALL, not per tick, plus nframes * 4096 written when frames go out.  Six launches and one more per 128 records.
 * The arrays and wire forms are not tuned: records of one stream may hit the same byte, so they issue one launch per t
 * (the wire form one per 128 streams and t), each followed by a copy kernel when frames go out.
 * Measured once on one MI355X (profiles/multi_stream_client.json: 1080p, compact form, microseconds per record, median of five
 * rounds whose spread -- max minus min over the median -- is at most 4.0 % for this call, 1.3 % for the ticks and 7.6 % for the
 * cores; without / with output frames, and in brackets T calls of mi355_apply_multi_cwire_batch on records re-staged
 * beforehand / S client cores with mi355_apply_cwire_batch(T) each, both without frames, same run, same board).
 * Webcam-like input, every tile touched by every record: S = 4: T = 4 2.628 / 3.212 (7.299 / 5.339), T = 16 1.28 / 1.841
 * (7.344 / 1.891), T = 64 0.989 / 1.582 (7.529 / 1.37); S = 16: T = 4 1.549 / 2.309 (3.521 / 5.056), T = 16 1.021 / 1.737
 * (3.573 / 1.494), T = 64 0.987 / 1.965 (3.688 / 1.205).
 * Local input (a block moving on a still background, 367 of 1519 tiles touched): S = 4: T = 4 3.118 / 3.935 (10.55 / 6.081),
 * T = 16 1.127 / 2.068 (10.612 / 2.316), T = 64 0.703 / 1.643 (10.757 / 1.391); S = 16: T = 4 1.083 / 2.001 (3.108 / 5.055),
 * T = 16 0.427 / 1.473 (3.127 / 1.631), T = 64 0.453 / 1.423 (3.174 / 1.06).
 * Without frames the call is ahead of the pre-staged ticks and of the S cores by more than the spread at every point on both
 * inputs; with frames it is still ahead of the ticks everywhere, but behind S cores that write none at T = 64 (and at S = 16,
 * T = 16 on the webcam-like input).  The time does not fall T-fold as the state traffic does: the records are still read
 * twice and decoded once each.  DESIGN.md section 4, "The receiving end of a burst". */
int mi355_apply_multi_stream_batch(mi355_core *core, const void *d_offsets, const void *d_xs, const void *d_diff,
                                   int nstreams, int nframes, void *d_states, size_t stride_bytes,
                                   void *d_frames_out, size_t out_stride_bytes);
int mi355_apply_multi_stream_wire_batch(mi355_core *core, const void *d_wire, const uint32_t *h_counts,
                                        int nstreams, int nframes, void *d_states, size_t stride_bytes,
                                        void *d_frames_out, size_t out_stride_bytes);
int mi355_apply_multi_stream_cwire_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts,
                                         const uint32_t *h_escapes, int nstreams, int nframes, void *d_states,
                                         size_t stride_bytes, void *d_frames_out, size_t out_stride_bytes);

/* A burst coalesced: nframes compact records of each of nstreams streams (batch index b = s*nframes + t, the layout of
 * mi355_diff_multi_stream_cwire_batch's output; the headers h_counts[b] / h_escapes[b] from the host as in
 * mi355_apply_multi_stream_cwire_batch) -> ONE segment / record per stream, the one that takes a client from the frame
 * before the burst to the frame after it.  For a relay that is nframes ticks behind, a recorder that keeps every
 * nframes-th picture, a wall that shows its cameras at a fraction of their rate: none of them holds a state.
 *   Result: for stream s, sum[x] = the sum over t of the difference record (s, t) holds at index x, in uint8 wrap-around
 *   (0 where no record has an entry).  Segment s holds the entries (x, sum[x]) with sum[x] != 0 in ascending x -- an index
 *   whose differences cancel drops out.  d_offsets: uint32[nstreams + 1], the exclusive scan of the segments' counts.
 *   Compact form: record s is the canonical encoding of segment s -- the bytes mi355_cwire_encode_batch would write from it,
 *   pad bytes zero, headers {n, e} written -- at d_cwire_out + d_frame_pos[s]; d_frame_pos: uint64[nstreams + 1], always
 *   exact.  Record s is written only if d_frame_pos[s + 1] <= capacity_bytes; one that does not fit is skipped whole and the
 *   records behind it that fit are still written.  mi355_cwire_bytes_max(N, nstreams) always suffices.
 *   Arrays form: entries at or past `capacity` are dropped, the offsets stay exact.
 *   Applying output record s to any N-byte state equals applying the stream's nframes records in order (mi355_cwire_apply_host,
 *   mi355_apply_multi_cwire_batch, and mi355_apply_multi_batch for the arrays form).  With nframes == 1 a record this library
 *   made comes back byte for byte.  A stream whose records cancel completely yields an n = 0 record of 8 bytes.
 *   Malformed compact content under consistent headers: nothing is read outside the input span, nothing is written outside the
 *   outputs; an escape ranked at or past e and an index >= N contribute nothing (the guarantees of
 *   mi355_apply_multi_stream_cwire_batch).  The output is still one well-formed canonical record per stream -- it is encoded
 *   from the accumulated sums -- and d_offsets / d_frame_pos agree with it; only the malformed stream's own record is
 *   otherwise unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: a null core; a negative nstreams or nframes;
 *   nstreams*nframes > max_batch; with nstreams*nframes > 0 a null input or output pointer; h_escapes[b] > h_counts[b];
 *   h_counts[b] > N; d_cwire, d_cwire_out, d_offsets or d_xs not 4-byte aligned; d_frame_pos not 8-byte aligned; the input
 *   span (known from the host's headers) overlapping an output region: [d_cwire_out, + capacity_bytes), d_xs / d_diff over
 *   `capacity` entries, the offsets or frame_pos array.  nstreams*nframes == 0 writes offsets[0] = 0 (and frame_pos[0] = 0)
 *   and nothing else.
 * Asynchronous on the core's stream, behind the last expansion of this core as every consumer of a packed stream is, so
 * mi355_diff_multi_stream_cwire_batch followed by this call on one core needs no synchronisation; with a caller's stream
 * everything runs on it in call order.  Nothing is allocated inside the call; the core's state is neither read nor written
 * (the call uses the directory scratch of mi355_apply_cwire_batch and nothing else of the core).
 * The directory kernels of mi355_apply_cwire_batch on the nstreams*nframes records, then four launches: a grid of 4096-byte
 * tiles x streams sums the records that land in a tile into a ZEROED tile in LDS and leaves four facts of it (nonzero bytes,
 * first, last, gaps >= 255 inside); one workgroup per stream scans the tiles; one workgroup places the streams and writes
 * headers and pad bytes; the tile grid runs again, a tile without a nonzero byte returns on its fact word, the others rebuild
 * their sums from the records and store their entries.  The records are read about three times; no N-byte buffer exists.
 * Not measured yet: tools/bench_multi.py --legs coalesce writes profiles/multi_coalesce.json (microseconds per input record
 * against mi355_apply_multi_stream_cwire_batch onto relay-held states + mi355_diff_multi_cwire_batch of a threshold-0 core, same
 * run, same board).  The expectation to test -- no slower than that route at S = 16, T = 16 on either input, by more than
 * the rounds' spread -- is neither met nor missed until that file exists.  DESIGN.md section 4, "Coalescing a burst". */
int mi355_cwire_coalesce_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                               int nstreams, int nframes, void *d_offsets, void *d_xs, void *d_diff, size_t capacity);
int mi355_cwire_coalesce_cwire_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts,
                                     const uint32_t *h_escapes, int nstreams, int nframes, void *d_offsets,
                                     void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes);

/* A camera cropped: the records of mi355_cwire_coalesce_* (same input, same batch index b = s*nframes + t, the headers
 * h_counts[b] / h_escapes[b] from the host, the header words in the buffer not trusted) cut to one rectangle per stream,
 * h_rects[s] = {x0, y0, w, h} in pixels of the core's W x H frame, and re-indexed to the rectangle's own w x h frame.  For a
 * viewer that zooms into a part of one camera of a wall and a relay that thins a camera's traffic to the region somebody looks
 * at: the client holds a w x h state, not a full one.  Cropping commutes with the client's state[x] += diff, so it is exact and
 * needs no state.
 *   Sums and selection: sum_s[x] = the uint8 wrap-around sum of stream s's differences at byte index x < N, as in the coalescer.
 *   An entry (x, sum_s[x]) with sum_s[x] != 0 is kept if its pixel lies inside the rectangle: row = x / (3*W) in [y0, y0 + h) and
 *   column byte = x % (3*W) in [3*x0, 3*(x0 + w)).
 *   Index map: a kept entry is written with index (row - y0)*3*w + column byte - 3*x0, its byte index in the w x h BGR24 frame of
 *   the rectangle (N'_s = 3*w*h bytes).  The map is monotone: the kept entries stay in ascending order.  With flags =
 *   MI355_CROP_KEEP_INDEX the entry is written with x unchanged instead: the record then updates only the rectangle of a
 *   full-size state.  w == 0 or h == 0 selects nothing and yields an n = 0 record of 8 bytes.  With nframes > 1 the result is
 *   the crop of the coalesced burst; with nframes == 1, the full-frame rectangle and a record this library made, the input
 *   comes back byte for byte.
 *   Outputs: those of the coalescer -- d_offsets, uint32[nstreams + 1]; compact form: record s, the canonical encoding of
 *   segment s (pad bytes zero, headers written), at d_cwire_out + d_frame_pos[s], d_frame_pos uint64[nstreams + 1] and always
 *   exact; a record is written only if it fits, one that does not is skipped whole and the ones behind it that fit are still
 *   written; arrays form: entries at or past `capacity` are dropped, the offsets stay exact.  mi355_cwire_bytes_max(N, nstreams)
 *   always suffices as capacity, and without MI355_CROP_KEEP_INDEX so does the sum over s of mi355_cwire_bytes_max(3*w_s*h_s, 1).
 *   Law: for any N-byte state A let crop(A) be the rectangle of A as a w x h frame.  Applying output record s to crop(A) equals
 *   the crop of applying the stream's nframes records to A.  With MI355_CROP_KEEP_INDEX, applying it to A changes exactly the
 *   rectangle, in the same way.
 *   Malformed content under consistent headers: the coalescer's guarantees -- nothing is read outside the input span, nothing is
 *   written outside the outputs, an escape ranked at or past e and an index >= N contribute nothing.  Output record s is still
 *   well-formed and canonical: mi355_cwire_check_host(N'_s, ...) gives verdict 0 (against N with MI355_CROP_KEEP_INDEX).
 *   Refused with MI355_ERR_INVALID before anything is launched or written: whatever mi355_cwire_coalesce_* refuses; a null
 *   h_rects when nstreams*nframes > 0; a flag bit other than MI355_CROP_KEEP_INDEX; a rectangle with a negative member; a
 *   rectangle with x0 + w > W or y0 + h > H (computed in 64 bits).  nstreams*nframes == 0 writes offsets[0] = 0 (and
 *   frame_pos[0] = 0) and nothing else.
 * Asynchronous on the core's stream, behind the last expansion of this core as every consumer of a packed stream is; with a
 * caller's stream everything runs on it in call order.  Nothing is allocated inside the call and nothing is copied to the
 * device: the rectangles travel as kernel arguments of the first tile pass, which leaves six words per stream in the per-stream
 * words of mi355_cwire_budget_cwire_batch for the second (the two calls are ordered on one stream).  The core's state is neither
 * read nor written.
 * The directory kernels on the nstreams*nframes records, then the coalescer's four launches with a filter on the tile: a
 * 4096-byte tile whose byte range misses the rectangle's rows [3W*y0, 3W*(y0 + h)) stores the all-zero fact and reads no record
 * byte; the others sum their records in LDS, zero the bytes outside the rectangle (a lane's 64 bytes may span several rows when
 * 3W < 64; a tile may sit inside one row when 3W > 4096) and take the four facts in mapped indices; the coalescer's scan and
 * placement follow unchanged; the tile grid runs again and writes the entries with mapped indices.  The row of a byte comes from
 * an exact multiply-and-correct division by 3W, once per lane and again only where a lane's bytes reach a later row.
 * Measured (profiles/multi_crop.json: tools/bench_multi.py --legs crop; the compact form at 1080p, T = 1, median of five rounds,
 * spread of the rounds 0.1 - 1.0 %, against mi355_cwire_coalesce_cwire_batch on the same records in the same run), us per stream
 * at S = 4 / 16 / 64: webcam-like input (137 k entries per stream, 37 k in the quarter picture) coalesce 15.9 / 8.1 / 6.2, the
 * quarter-picture crop 15.5 / 6.8 / 4.6, the full-frame crop 16.6 / 8.6 / 6.7; local input (a block moving over a still
 * background, 4.8 k entries) coalesce 16.6 / 5.4 / 2.4, quarter 17.8 / 5.7 / 2.6, full 16.9 / 5.5 / 2.5.  The expectation --
 * the quarter-picture crop no slower than that coalesce call by more than the rounds' spread -- is met on the webcam-like input
 * (0.97 / 0.83 / 0.74 of it) and MISSED on the local input (1.07 / 1.06 / 1.10: there nearly every tile is empty in both calls
 * and the kept ones pay the mask and the map); the full-frame crop is 2 - 8 % slower than the coalesce call (1 to 30 us per call),
 * more than the spread, with no table launch left to blame.  An earlier attempt at this call was
 * not merged; this one rests on the budget call's filtered tile and on the one record table and region test of core.hip.
 * DESIGN.md section 4, "Cropping records". */
#define MI355_CROP_KEEP_INDEX 1u
int mi355_cwire_crop_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                           int nstreams, int nframes, const int32_t *h_rects, unsigned flags, void *d_offsets, void *d_xs,
                           void *d_diff, size_t capacity);
int mi355_cwire_crop_cwire_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                                 int nstreams, int nframes, const int32_t *h_rects, unsigned flags, void *d_offsets,
                                 void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes);

/* Many cameras on one canvas: the opposite direction of the crop.  The records of mi355_cwire_coalesce_* / mi355_cwire_crop_*
 * (same input, same batch index b = s*nframes + t, the headers h_counts[b] / h_escapes[b] from the host, the header words in the
 * buffer not trusted, frames of the core's W x H, N bytes) -> ONE segment / record for a BGR24 canvas of canvas_w x canvas_h
 * pixels, Nc = 3*canvas_w*canvas_h bytes, that shows the cameras side by side at full resolution.  For a multiview relay (four
 * 1080p cameras in a 4K canvas, one record per tick for a client that holds one canvas state and reads one socket), a recorder
 * that keeps one stream per wall, and row-band sharding: the compact records of several cores that each own a band of one
 * picture merged into the whole picture's record (mi355_merge_parts does that for the arrays form only).  Placing commutes with
 * the client's state[x] += diff, exactly as cropping does, so it is exact and needs no state.
 *   Placement: h_place[s] = {sx, sy, w, h, dx, dy} in pixels: the rectangle [sx, sx + w) x [sy, sy + h) of camera s goes to
 *   [dx, dx + w) x [dy, dy + h) of the canvas.  w == 0 or h == 0 places nothing.
 *   Sums: sum_s[x] = the uint8 wrap-around sum of stream s's differences at byte index x < N, as in the coalescer.  Canvas byte
 *   y lies in row R = y / (3*canvas_w) at column byte q = y % (3*canvas_w); stream s covers y when dy <= R < dy + h and
 *   3*dx <= q < 3*(dx + w), and its source byte is then (sy + R - dy)*3*W + 3*sx + (q - 3*dx).  C[y] = the uint8 sum of
 *   sum_s[source byte] over the streams that cover y.  Destination rectangles that overlap are not refused: their differences
 *   add, which is well defined and spares an S^2 host check.
 *   Outputs: the ONE segment holds the entries (y, C[y]) with C[y] != 0 in ascending y; d_offsets = {0, n} (uint32[2]).  The
 *   compact form writes its canonical record (headers written, pad bytes zero, byte for byte what mi355_cwire_encode_batch would
 *   write) at d_cwire_out, d_frame_pos = {0, record bytes} (uint64[2]), both always exact; the record is written only if it
 *   fits, otherwise nothing of it is written.  Arrays form: entries at or past `capacity` are dropped.
 *   mi355_cwire_bytes_max(Nc, 1) always suffices.  A canvas no camera lands on yields the 8-byte n = 0 record.
 *   Laws: (a) apply -- applying the output to an Nc-byte canvas state K changes exactly the covered bytes; with disjoint
 *   destinations the rectangle of K at (dx, dy, w, h) becomes what stream s's records make of it through the crop law.
 *   (b) inverse of the crop -- with disjoint destinations, mi355_cwire_crop_cwire_batch of the output, on a core of the canvas'
 *   geometry with rectangle (dx, dy, w, h), equals mi355_cwire_crop_cwire_batch of stream s's input with (sx, sy, w, h), byte
 *   for byte.  (c) special cases -- one stream with {0, 0, W, H, 0, 0} on a W x H canvas is the coalescer's output byte for
 *   byte; one stream with {x0, y0, w, h, 0, 0} on a w x h canvas is the crop call's.  (d) bands -- {0, 0, W, H, 0, s*H} on a
 *   W x S*H canvas is the bands' coalesced records concatenated with index bias s*N.
 *   Malformed content under consistent headers: the family's memory safety -- nothing is read outside the input span, nothing
 *   is written outside the outputs; an index >= N and an escape ranked at or past e contribute nothing.  The output is still
 *   one canonical record: mi355_cwire_check_host(Nc, ...) gives word 0 == 0.  Only canvas bytes inside the malformed stream's
 *   destination are otherwise unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: whatever mi355_cwire_coalesce_* refuses; a null
 *   h_place when nstreams*nframes > 0; a negative member of a placement; sx + w > W or sy + h > H; dx + w > canvas_w or
 *   dy + h > canvas_h (all computed in 64 bits); canvas_w or canvas_h < 1; Nc >= 2^31, the bound mi355_create puts on a frame;
 *   the input span overlapping an output region; and a canvas of more 4096-byte tiles than the fact scratch holds, that is
 *   mi355_state_tiles(Nc) > max_batch * mi355_state_tiles(N).  Nothing is allocated inside the call: the per-tile facts take
 *   the scratch the core made for max_batch records, so a canvas needs a core whose max_batch covers it -- four 1080p
 *   cameras in a 3840 x 2160 canvas: mi355_state_tiles(N) = 1519, max_batch 4 gives 6076 words for the canvas' 6075 tiles.
 *   nstreams*nframes == 0 writes offsets[0] = 0 (and frame_pos[0] = 0) and nothing else.
 * Asynchronous on the core's stream, behind the last expansion of this core as every consumer of a packed stream is; with a
 * caller's stream everything runs on it in call order.  Nothing is copied to the device: the placements travel as kernel
 * arguments of a small table kernel (128 streams per launch), which leaves six words per stream in the per-stream words of
 * mi355_cwire_budget_cwire_batch (the two calls are ordered on one stream).  The core's state is neither read nor written.
 * The directory kernels on the nstreams*nframes records, the table kernel, then a tile grid over the CANVAS: a 4096-byte canvas
 * tile tests 64 streams a round (do its rows meet the destination's, does it hold a byte of its columns), per hit 64 records a
 * round on the directory words of the source tiles its bytes come from, and per record with an entry there walks the record
 * once from the first of those tiles, adding the entries of the source rectangle at their canvas byte into a zeroed tile in
 * LDS.  The coalescer's scan and placement follow unchanged, for one stream of mi355_state_tiles(Nc) tiles; the tile grid runs
 * again and writes the entries.  The row of a source byte comes from an exact multiply-and-correct division by 3W, once per
 * kept entry; while a record is walked, the header, directory word and first block of the next are in flight.  A first form:
 * a walk begins at the first source tile's edge, not at the first byte the canvas tile needs, and a canvas narrower than the
 * source frames walks over source rows it then drops.
 * Measured (profiles/multi_mosaic.json: tools/bench_multi.py --legs mosaic --streams 4,16; the compact form at 1080p, whole
 * frames in a 2x2 grid of a 3840 x 2160 canvas and a 4x4 grid of a 7680 x 4320 canvas, median of five rounds, spread of the rounds
 * 0.2 - 9 %), us per input record, the call / the route a caller has without it in the same run
 * (mi355_apply_multi_stream_cwire_batch onto relay-held states, mi355_wall_compose_batch at k = 1 into a canvas, a synchronize,
 * mi355_diff_stream_cwire_batch(nframes = 1) on a threshold-0 core of the canvas' geometry; its record equals the call's byte
 * for byte at every point).  Webcam-like input (137 k entries per record): S = 4, T = 1 26.09 / 36.33, T = 16 4.96 / 3.22; S = 16,
 * T = 1 19.16 / 17.18, T = 16 4.08 / 2.23.  Local input (a block moving over a still background, 4.8 k entries): S = 4, T = 1
 * 25.43 / 35.81, T = 16 3.19 / 2.84; S = 16, T = 1 14.12 / 15.92, T = 16 1.73 / 1.45.  The expectation -- no slower than that route at
 * any point, by more than the rounds' spread -- is met at T = 1 for S = 4 on both inputs and for S = 16 on the local input (0.71 -
 * 0.89 of the route) and MISSED at T = 1 for S = 16 webcam-like cameras (1.12) and at T = 16 everywhere (1.12 - 1.83): the route
 * pays per state and canvas byte once per call whatever T is, the call per record entry, in both tile passes.  Not profiled per
 * kernel, not tuned in this change.  DESIGN.md section 4, "Placing cameras on a canvas". */
int mi355_cwire_mosaic_batch(mi355_core *core, const void *d_cwire_in, const uint32_t *h_counts, const uint32_t *h_escapes,
                             int nstreams, int nframes, const int32_t *h_place /* [nstreams][6] */, int canvas_w, int canvas_h,
                             void *d_offsets /* uint32[2] */, void *d_xs, void *d_diff, size_t capacity);
int mi355_cwire_mosaic_cwire_batch(mi355_core *core, const void *d_cwire_in, const uint32_t *h_counts, const uint32_t *h_escapes,
                                   int nstreams, int nframes, const int32_t *h_place, int canvas_w, int canvas_h,
                                   void *d_offsets /* uint32[2] */, void *d_frame_pos /* uint64[2] */, void *d_cwire_out,
                                   size_t capacity_bytes);

/* Records for a datagram socket: every compact record (back to back where h_counts[r] / h_escapes[r] put them, as in
 * mi355_cwire_check_batch; the header words in the buffer are not trusted) cut into pieces of at most max_bytes bytes each.  A
 * record is additive over ascending, disjoint indices, so any run of its entries is a record of the same frame: a piece IS a
 * record, the receiver needs nothing new, pieces may be applied in any order and a lost piece costs its own entries only (which
 * the resync calls -- mi355_state_digest_batch, mi355_refresh_cwire_batch, mi355_state_clear_tiles_batch -- then repair).
 *   The piece rule (mi355_cwire_split_host is the definition; entry k of a record has index x_k by the decode rule of
 *   mi355_cwire_check_*):  the entries are cut at every multiple of MI355_CWIRE_SPLIT_BLOCK and no piece crosses such a cut.  A
 *   piece [a, b) costs bytes(a, b) = 8 + 2*pad4(b - a) + 4*(F(a) + #{k in (a, b): code[k] == 255}) with F(a) = 1 if x_a >= 255, else
 *   0.  From a (always a multiple of 4) with B = min(n, the end of a's block) the piece ends at the largest b <= B with
 *   bytes(a, b) <= max_bytes where b == B or (b - a) % 4 == 0; the next piece starts at b.  max_bytes is a multiple of 4 in
 *   [64, 65536]: four escaped entries cost 32 bytes, so a piece always exists.  A record with n == 0 yields no piece.
 *   Piece contents: header {b - a, its escapes}; code[a .. b) and diff[a .. b) copied, pad bytes zero; the first code is
 *   min(x_a, 255); escape section: x_a first if F(a), then the input's escape values of the 255 codes in (a, b), in order.  Every
 *   piece's code and diff sections are whole dwords of the input.
 *   Laws: a piece of a canonical record is canonical (mi355_cwire_check_host gives word 0 == 0 against N); decoding a record's
 *   pieces back to back gives the record's (xs, diff); applying any permutation of the pieces gives the state the record gives;
 *   applying any subset changes exactly that subset's indices; a record that fits max_bytes comes back as one piece, byte for byte
 *   the input when x_0 < 255 or code[0] was already 255 (both always hold for canonical input).
 *   Outputs: piece_first, uint32[nrecords + 1], the exclusive scan of the pieces per record, always exact.  piece_pos,
 *   uint64[piece_capacity + 1], the exclusive scan of the piece sizes: entries 0 .. min(total, piece_capacity) are written and
 *   exact.  Piece p is written whole, at out + piece_pos[p], iff p < piece_capacity and piece_pos[p + 1] <= capacity_bytes; one
 *   that does not fit is skipped whole and later ones that fit are still written.  Pieces lie in record order, then entry order.
 *   Capacity helpers (host only, never below what the rule produces): mi355_cwire_split_pieces_max(n, e, M) = ceil(n / 65536) +
 *   floor((2*pad4(n) + 4e) / (M - 35)).  Derivation: a piece that is not the last of its block could not take four more entries,
 *   which cost at most 24 bytes, so it is larger than M - 24; of its bytes at most 8 (header) + 4 (its own first escape) are not
 *   bytes of the input's sections, so it holds at least M - 35 of the record's 2*pad4(n) + 4e section bytes; and every block adds
 *   one last piece.  mi355_cwire_split_bytes_max(n, e, M) = record bytes + 12 * pieces_max (a piece adds a header and at most one
 *   escape word, and pads at most the record's own pad).  Both return 0 for a max_bytes outside [64, 65536].  Sum them over the
 *   records of a call.
 *   Malformed content under consistent headers: the family's guarantees -- nothing is read outside the input span, nothing is
 *   written outside the outputs; piece sizes follow the codes and the wrapped running index (an escape ranked at or past e adds
 *   nothing); the contents of that record's pieces are otherwise unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: whatever mi355_cwire_check_batch refuses; max_bytes
 *   below 64, above 65536 or not a multiple of 4; with nrecords > 0 a null output pointer; d_cwire_out or d_piece_first not 4-byte
 *   aligned; d_piece_pos not 8-byte aligned; the input span overlapping an output region.  nrecords == 0 writes piece_first[0] =
 *   0 and piece_pos[0] = 0 and nothing else.
 * Asynchronous on the core's stream, behind the last expansion of this core as every consumer of a packed stream is; with a
 * caller's stream everything runs on it in call order.  Nothing is allocated inside the call (two words per block of 65536
 * entries are made with the core and counted by mi355_workspace_bytes) and the core's state is neither read nor written.
 * The chunk table of the GPU clients through its running sums, then a count pass over the blocks of all records (a workgroup
 * walks its block four entries per lane, scans escape rank and running index, and finds each cut), one scan (piece_first, the
 * pieces and bytes before each block in 64 bits, piece_pos[0]) and an emit pass that walks the blocks again and writes headers,
 * codes, escapes, differences and zero pads with non-temporal stores, whole dwords copied.  No workgroup waits on another and
 * no walk is longer than one block.
 * Measured (profiles/multi_split.json: tools/bench_multi.py --legs split; 1080p, T = 1, median of five rounds, spread of the
 * rounds 0.1 - 3.7 %, against mi355_cwire_coalesce_cwire_batch with T = 1 on the same records in the same run; the pieces equal
 * the host form's at every point), us per input record at S = 4 / 16 / 64: webcam-like input (137 k entries per record, 201
 * pieces at M = 1400, 32 at M = 8972) coalesce 15.99 / 8.20 / 6.30, split at 1400 51.99 / 13.22 / 3.44, at 8972 50.18 / 12.77 /
 * 3.50; local input (a block moving over a still background, 4.8 k entries, 9 and 2 pieces) coalesce 16.64 / 5.41 / 2.41, split
 * at 1400 10.20 / 2.71 / 0.73, at 8972 10.00 / 2.64 / 0.73.  The expectation -- no slower than that coalesce call by more than
 * the rounds' spread -- is met on the local input at every S (0.30 - 0.61 of it) and for 64 webcam-like cameras (0.55) and MISSED
 * for 4 and 16 webcam-like cameras (3.2 and 1.6 times its time): such a record is three blocks, four cameras are twelve
 * workgroups that each walk sixteen rounds twice, and the call is bound by the latency of a round, not by bytes.  An earlier
 * attempt at this call was not merged; this one fixes the piece rule so that blocks are independent.  The input is named
 * d_cwire_in, as the mosaic call's is.  DESIGN.md section 4, "Splitting records into datagrams". */
#define MI355_CWIRE_SPLIT_BLOCK 65536u
int mi355_cwire_split_host(size_t frame_bytes, const void *cwire, size_t cwire_bytes, const uint32_t *h_counts,
                           const uint32_t *h_escapes, int nrecords, size_t max_bytes, uint32_t *piece_first,
                           uint64_t *piece_pos, size_t piece_capacity, void *out, size_t capacity_bytes);
int mi355_cwire_split_cwire_batch(mi355_core *core, const void *d_cwire_in, const uint32_t *h_counts, const uint32_t *h_escapes,
                                  int nrecords, size_t max_bytes, void *d_piece_first, void *d_piece_pos,
                                  size_t piece_capacity, void *d_cwire_out, size_t capacity_bytes);
size_t mi355_cwire_split_pieces_max(uint32_t n, uint32_t e, size_t max_bytes);
size_t mi355_cwire_split_bytes_max(uint32_t n, uint32_t e, size_t max_bytes);

/* Parity pieces for the datagram path: K parity datagrams per group of G pieces, so that any K losses inside a group are rebuilt
 * by the receiver itself -- no digests up, no refresh records down, and a one-way or multicast link needs no back channel.  What
 * is lost beyond K of a group stays the resync calls' business.
 *   Input: what mi355_cwire_split_cwire_batch wrote -- the piece buffer of pieces_bytes bytes, piece_first (uint32[nrecords + 1])
 *   and piece_pos (uint64[piece_capacity + 1]); piece p is the bytes [piece_pos[p], piece_pos[p + 1]).
 *   Groups: record r has c_r = piece_first[r + 1] - piece_first[r] pieces and ceil(c_r / G) groups; group j of record r has the
 *   members at slots i = 0 .. m - 1, m = min(G, c_r - j*G), the member at slot i being piece piece_first[r] + j*G + i.  G (group) is
 *   in 1 .. 255, K (nparity) is 1 or 2; groups never span records.  fec_first, uint32[nrecords + 1], is the exclusive scan of the
 *   groups per record and always exact; global group g = fec_first[r] + j.
 *   Parity: L_g is the largest member length of the group.  Every member is read as little-endian dwords, zero-extended to L_g.
 *   P[w] is the XOR of the members' words w.  Q[w] is the XOR over the slots i of 2^i * D_i[w], byte by byte in GF(2^8) modulo
 *   x^8 + x^4 + x^3 + x^2 + 1 (0x11D) -- equally Horner's rule from the last slot down, Q = xtime(Q) ^ D_i, with xtime(v) =
 *   ((v & 0x7f7f7f7f) << 1) ^ (((v >> 7) & 0x01010101) * 0x1d) on a packed dword.  The powers 2^0 .. 2^254 are distinct, hence
 *   G <= 255.
 *   Outputs, at a fixed pitch (the prototypes' spacing_bytes): fec_len, uint32[group_capacity]: entries g < min(total groups, group_capacity) are written and
 *   exact, later entries are untouched.  Parity block q of group g (0: P, 1: Q) is the L_g bytes at out + (g*K + q)*pitch; bytes
 *   [L_g, pitch) of a slot are never written.  pitch is a multiple of 4 in [64, 65536], normally the split call's max_bytes.  A
 *   group with g >= group_capacity or (g + 1)*K*pitch > capacity_bytes is skipped whole and groups behind it that fit are written.
 *   mi355_cwire_fec_groups_max(piece_capacity, nrecords, group) = floor(piece_capacity / group) + nrecords is never below the
 *   groups of piece_capacity pieces in nrecords records (0 for a group outside 1 .. 255).
 *   Void groups: a group is void when a member is absent (p >= piece_capacity, or piece_pos[p + 1] > pieces_bytes) or malformed
 *   (piece_pos[p + 1] < piece_pos[p]; position or length not a multiple of 4; length 0; length > pitch).  It has fec_len[g] = 0
 *   and none of its parity bytes is written.  This is the memory-safety rule: nothing is read outside the three input extents as
 *   stated, nothing is written outside the outputs.  Tables that the split call wrote are always consistent; for any other table
 *   only that guarantee holds.
 *   Laws: a group of one member has P == Q == that member; fec_first depends on piece_first alone; parity of the pieces of
 *   canonical records, then any loss of at most K of a group's m + K datagrams, then repair gives back the lost pieces byte for
 *   byte; every rebuilt piece is canonical (mi355_cwire_check_host word 0 == 0); applying survivors and rebuilt pieces in any
 *   order gives the state the record gives.
 *   mi355_cwire_fec_host is the definition: plain C++, no core, no HIP call.  mi355_cwire_fec_batch is bit-identical to it in
 *   fec_first, fec_len (as far as written) and every written parity byte; asynchronous on the core's stream, in call order behind
 *   the split call with no synchronisation in between; nothing is allocated and the core's state is untouched.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: a null core; nrecords outside [0, max_batch]; group,
 *   nparity or pitch out of range; with nrecords > 0 a null pointer; the 4-byte tables, d_pieces or d_out not 4-byte aligned;
 *   d_piece_pos not 8-byte aligned; any output region overlapping an input region or another output.  nrecords == 0 writes
 *   fec_first[0] = 0 and nothing else.
 * Repair of one group, mi355_cwire_fec_repair_host (the definition): slot[i] is the surviving member at slot i (slot_len[i]
 * bytes) or NULL for a lost one; p and q are the group's parity blocks or NULL; fec_len is the group's L_g.  u is the number of
 * NULL slots, a < b the lost slots.  u == 0 writes nothing; u >= 1 writes fec_len bytes per lost slot, out0 for a, out1 for b.
 * With Pxy = P ^ (XOR of the survivors) and Qxy = Q ^ (XOR of 2^i * survivor i): one lost and P present, D_a = Pxy; one lost and
 * only Q present, D_a = inv(2^a) * Qxy; two lost, D_b = inv(2^a ^ 2^b) * (Qxy ^ 2^a * Pxy) and D_a = Pxy ^ D_b.
 *   verdict[k] of rebuilt block k: bit 0 (MI355_FEC_BAD_HEADER): its header {n, e} has n == 0, e > n or
 *   mi355_cwire_frame_bytes(n, e) > fec_len (a block shorter than a header has it set, too); bit 1 (MI355_FEC_BAD_TAIL): a nonzero
 *   byte at or past mi355_cwire_frame_bytes(n, e).  Zero for what the sender made, and zero for a block that is not rebuilt.  A
 *   clean verdict is no replacement for mi355_cwire_check_* before applying.
 *   Refused, with the outputs untouched: members outside 1 .. 255; fec_len 0 or not a multiple of 4; a surviving length 0, not a
 *   multiple of 4 or > fec_len; u > (p != NULL) + (q != NULL); a needed output NULL (verdict is needed when u >= 1).
 *   Everything is wordwise, so the form also works on a common prefix of all blocks: from the first 8 bytes of each datagram
 *   (fec_len = 8, every length 8) a receiver gets a lost piece's {n, e} without touching the payload; the verdict of a prefix
 *   says nothing.
 * Repair of many groups on a core, mi355_cwire_fec_repair_batch: job j has the slots h_job_first[j] .. h_job_first[j + 1] of
 * h_slot_off (byte offsets into d_rx, MI355_FEC_ABSENT: lost) and h_slot_len, the parity blocks at h_parity_off[2j] (P) and
 * [2j + 1] (Q) (MI355_FEC_ABSENT: not there) and h_fec_len[j].  Rebuilt block k of job j is the h_fec_len[j] bytes at d_out +
 * (2j + k)*pitch, a job with one loss writes block 0 only; d_verdict, uint32[njobs][2], is written for every job, the words of
 * blocks not rebuilt 0.  Byte for byte the host form's output.  All descriptors are host arrays and may be reused when the call
 * returns: they travel as kernel arguments, 8 jobs and 256 slots per launch at the most, as h_place of the wall does (losses are
 * rare: a launch per job or two is fine).  Asynchronous on the core's stream; nothing is allocated and nothing synchronises; the
 * GF constants of a job are computed on the host.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: whatever the host form refuses, per job; an offset not
 *   4-byte aligned or a block reaching past rx_bytes; h_fec_len[j] > pitch; njobs outside [0, max_batch]; d_rx, d_out, d_verdict
 *   or pitch not a multiple of 4; d_out or d_verdict overlapping d_rx or each other; with njobs > 0 a null pointer.  A job with
 *   nothing lost is legal and writes only its two verdict words.
 * The parity call: one workgroup scans the groups per record, then a grid sized from the device (the host does not know the
 * piece count and does not wait for it) whose waves stride over (group, 256 bytes of its parity block): the group's record by
 * binary search in fec_first, the void rule on the members' positions before a piece byte moves, then per dword the members
 * from the last slot down, one coalesced dword load bounded by the member's length, one XOR into P, xtime and one XOR into Q.
 * No tables, no LDS, no atomics, no workgroup waits on another; pieces are 4-byte aligned only, so every load is one dword.
 * The repair call: a workgroup per job does the same walk over the survivors, then the constant multiplies (eight shift-and-XOR
 * steps on packed dwords under a wave-uniform constant), the header and tail tests and one verdict store per block.
 * Measured (profiles/multi_fec.json: tools/bench_multi.py --legs fec; 1080p, T = 1, M = 1400, G = 8, median of five rounds, against
 * mi355_cwire_split_cwire_batch on the same records in the same run; the parity equals the host form's at every point and the
 * rebuilt pieces the pieces), us per input record at S = 4 / 16 / 64: webcam-like input (137 k entries per record, 201 pieces, 26
 * groups, 71 kB of parity at K = 2) split 52.29 / 13.22 / 3.46, parity at K = 1 2.49 / 0.59 / 0.24, at K = 2 2.62 / 0.53 / 0.24; local
 * input (a block moving over a still background, 4.8 k entries, 9 pieces, 2 groups) split 10.36 / 2.59 / 0.72, parity at K = 1 2.45 /
 * 0.55 / 0.20, at K = 2 2.46 / 0.55 / 0.15.  The spread of the rounds is 0.1 - 10 % for the split call and 4 - 47 % for the parity
 * call (126 % at one K = 1 point): at a few microseconds a call it is the host's enqueue rate that is timed.  The expectation -- the
 * parity call at K = 2 no slower than the split call that feeds it, at any S, by more than the rounds' spread -- is met at every
 * point (0.04 - 0.07 of the split call on webcam-like input, 0.21 - 0.24 on the local input): it reads once what split wrote and
 * writes a quarter of it, in two launches where split takes nine.  The repair call, one job per stream, reported and not judged:
 * 2.6 / 1.0 / 1.1 us per job for one lost piece and 2.7 / 1.1 / 1.1 for two, on either input.  Not profiled per kernel.  DESIGN.md
 * section 4, "Parity for the datagram path". */
#define MI355_FEC_BAD_HEADER 1u
#define MI355_FEC_BAD_TAIL 2u
#define MI355_FEC_ABSENT UINT64_MAX
size_t mi355_cwire_fec_groups_max(size_t piece_capacity, int nrecords, int group);
int mi355_cwire_fec_host(const void *pieces, size_t pieces_bytes, const uint32_t *piece_first, const uint64_t *piece_pos,
                         size_t piece_capacity, int nrecords, int group, int nparity, size_t spacing_bytes, uint32_t *fec_first,
                         uint32_t *fec_len, size_t group_capacity, void *out, size_t capacity_bytes);
int mi355_cwire_fec_batch(mi355_core *core, const void *d_pieces, size_t pieces_bytes, const void *d_piece_first,
                          const void *d_piece_pos, size_t piece_capacity, int nrecords, int group, int nparity, size_t spacing_bytes,
                          void *d_fec_first, void *d_fec_len, size_t group_capacity, void *d_out, size_t capacity_bytes);
int mi355_cwire_fec_repair_host(int members, const void *const *slot /* [members], NULL: lost */, const uint32_t *slot_len,
                                const void *p /* or NULL */, const void *q /* or NULL */, uint32_t fec_len, void *out0, void *out1,
                                uint32_t verdict[2]);
int mi355_cwire_fec_repair_batch(mi355_core *core, const void *d_rx, size_t rx_bytes, int njobs,
                                 const uint32_t *h_job_first /* [njobs + 1] */, const uint64_t *h_slot_off, const uint32_t *h_slot_len,
                                 const uint64_t *h_parity_off /* [njobs][2] */, const uint32_t *h_fec_len /* [njobs] */, void *d_out,
                                 size_t spacing_bytes, void *d_verdict /* uint32[njobs][2] */);

/* Run-coded records for the link: a transcoder at the link's edge, the sender's last call before a stream socket and the
 * receiver's first call behind it.  A compact record spends a code byte on every entry, also where the entry's index is the one
 * before plus one (code 0); key frames (mi355_refresh_cwire_batch without digests), moving objects, threshold 0, a camera's first
 * thumbnail record and mosaic canvases are almost only such codes.  The run form keeps one code per RUN of consecutive indices and
 * halves those records; scattered noise it would enlarge, so the encoder packs a record only where the policy says so and tells
 * the receiver in a table.  Everything between the two calls keeps working on compact records; decode(encode(x)) is x byte for
 * byte.
 *   The run form of a compact record {n, e, code[n], esc[e], diff[n]}: entry k STARTS A RUN when k % 256 == 0 or code[k] != 0; a
 *   run is a start and the entries behind it up to the next start.  Runs never cross a multiple of 256 entries, a run holds 1 ..
 *   256 entries (its length fits a byte, no second escape list), every 255 code is a start (the escape section carries over word
 *   for word), and the runs of entries [4096c, 4096c + 4096) depend on those entries alone.  The cut costs at most 2 bytes per 256
 *   entries.  4-byte aligned, little-endian:
 *     u32 n | u32 e | u32 r
 *     u8  gap[r]            code[k] of each run's first entry, in order (255: escaped, as in the compact record)
 *     u8  0[pad4(r) - r]
 *     u8  len[r]            entries of the run - 1
 *     u8  0[pad4(r) - r]
 *     u32 esc[e]            the compact record's escape section
 *     u8  diff[n]           the compact record's diff section
 *     u8  0[pad4(n) - n]
 *   mi355_cwire_runs_frame_bytes(n, e, r) = 12 + 2*pad4(r) + 4*e + pad4(n): smaller than the compact record exactly when
 *   4 + 2*pad4(r) < pad4(n).  xs = {3, 4, 5, 300, 301, 1000}: codes {3, 0, 0, 255, 0, 255}, esc {294, 698}; runs gap {3, 255, 255},
 *   len {2, 1, 0}, r = 3; 36 bytes against 32, so not packed.  Canonical: one byte string per compact record -- runs are maximal
 *   under the rule, pad bytes zero; n == 0 has r == 0 and 12 bytes.
 *   Capacity: r <= n, and an escape spans at least 256 indices that hold one entry, so n + 255*e <= N and a record in the run form
 *   never needs more than 12 + 3*pad4(n) + 4*e <= 12 + 3*pad4(N) bytes; under MI355_RUNS_WHERE_SMALLER a record leaves in the
 *   smaller of its forms, never above the compact record's 8 + 2*pad4(N).  mi355_cwire_runs_bytes_max(frame_bytes, nrecords, policy)
 *   = nrecords * (12 + 3*pad4(N)) under MI355_RUNS_ALWAYS, mi355_cwire_bytes_max(N, nrecords) under MI355_RUNS_WHERE_SMALLER, 0 for
 *   an unknown policy.
 *   Encoder.  Input: compact records back to back where h_counts[b] / h_escapes[b] put them, as in mi355_cwire_check_batch.
 *   forms, uint32[nrecords][4]: forms[b] = {form, n, e, r}, form MI355_RUNS_FORM_COMPACT (the output bytes of record b are the
 *   compact record) or MI355_RUNS_FORM_RUNS (they are the run form); r is the run count in either case.  The table is what the
 *   sender puts on the socket ahead of the bytes and what the receiver hands to the decoder -- as every call of the family takes
 *   h_counts / h_escapes from the host.  The header words inside the buffers are written by the encoder; the decoder skips them
 *   and never follows them.  Policy: MI355_RUNS_WHERE_SMALLER uses the run form exactly when it is strictly smaller,
 *   MI355_RUNS_ALWAYS always (tests, measurements).  pos, uint64[nrecords + 1]: the exclusive scan of the output sizes, always
 *   exact; record b is written whole at out + pos[b] iff pos[b + 1] <= capacity_bytes, one that does not fit is skipped whole and
 *   later ones that fit are still written.  A record kept compact is copied as it is (its pad bytes too); in the run form the
 *   pad bytes are zero.
 *   Decoder.  Input: the encoder's bytes and h_forms.  Output: the compact records back to back, frame_pos (uint64[nrecords + 1],
 *   always exact -- it follows from h_forms alone) and the capacity rule above.  Decoding what the encoder wrote returns the
 *   encoder's input bytes and frame positions, under either policy.
 *   The host forms are the definition: plain C++, no core, no HIP call, no alignment requirement.  The GPU forms are bit-identical
 *   to them in every output.
 *   mi355_cwire_runs_decode_host refuses with MI355_ERR_INVALID (the reason in mi355_last_error): a truncated input; a form other
 *   than 0 or 1; n > frame_bytes, e > n or r > n; a run that crosses a multiple of 256 entries; run lengths that do not sum to n;
 *   a count of 255 gaps other than e.  Records before the refused one stay written, with their frame_pos.
 *   mi355_cwire_runs_decode_batch under malformed content with consistent headers promises what the family promises: nothing is
 *   read outside the span the headers give, nothing is written outside [frame_pos[b], frame_pos[b + 1]) and the position table,
 *   entries past n are dropped; the contents of that one record are otherwise unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched or written (batch forms): a null core; nrecords outside
 *   [0, max_batch]; with nrecords > 0 a null pointer; h_escapes[b] > h_counts[b], h_counts[b] > N (decoder: a row of h_forms the
 *   host decoder refuses by itself); an unknown policy; buffers, forms or input not 4-byte aligned, positions not 8-byte aligned;
 *   the input span overlapping an output.  nrecords == 0 writes pos[0] = 0 (frame_pos[0] = 0) and nothing else.
 * Asynchronous on the core's stream, behind the last expansion of this core; with a caller's stream everything runs on it in call
 * order.  Nothing is allocated inside a call (the decoder's record table and one word per 1024 runs are made with the core and
 * counted by mi355_workspace_bytes; the encoder uses the chunk table of the GPU clients) and the core's state is not touched.
 * Encoder: the chunk table, a count pass (a workgroup per 4096 codes, four entries per lane from one code dword, run starts by
 * ballot and popcount), a scan per record (first run rank per chunk, r, the size decision, the form row), one workgroup for pos in
 * 64 bits, and an emit pass per chunk: the starts' codes and places compacted in LDS, len as the distance to the chunk's next
 * start, gap[] and len[] stored as whole dwords inside the chunk's runs and single bytes at its ragged ends (no dword has two
 * writers, the pads have one), esc and diff copied as whole dwords, non-temporal stores.  Decoder: the sum of len + 1 per
 * workgroup of 1024 runs, a scan per record, then each workgroup builds the code bytes its runs cover 4096 at a time in LDS and
 * stores them under the same single-writer rule, clamped to n.  No workgroup waits on another.
 * Measured (profiles/multi_runs.json: tools/bench_multi.py --legs runs; 1080p, T = 1, MI355_RUNS_WHERE_SMALLER, median of five
 * rounds, spread of the rounds 0.1 - 7.3 %, against mi355_cwire_coalesce_cwire_batch with T = 1 on the same records in the same
 * run; both outputs equal the host forms' at every point), us per record at S = 4 / 16 / 64: key frames (mi355_refresh_cwire_batch
 * of every tile; 6.22 M entries, 24.6 k runs, 12.44 MB in, 6.27 MB out: 0.504) coalesce 48.32 / 37.26 / 36.41, encode
 * 11.79 / 8.43 / 9.81, decode 25.80 / 8.58 / 6.12; local input (a block moving over a still background, 4.8 k entries, 630 runs,
 * 11.7 kB in, 8.2 kB out: 0.70) coalesce 16.64 / 5.37 / 2.39, encode 4.55 / 1.12 / 0.34, decode 3.62 / 0.94 / 0.26;
 * webcam-like input (137 k entries, 122 k runs: kept compact, a dword copy) coalesce 16.18 / 8.14 / 6.23, encode 4.59 / 1.13 / 0.36,
 * decode 3.62 / 0.95 / 0.26.  The expectation -- each call no slower than that coalesce call by more than the rounds' spread -- is
 * met at every point (encode 0.06 - 0.28 of it, decode 0.04 - 0.53): both read the record about twice and write less than the
 * coalescer does.  Not profiled per kernel.  DESIGN.md section 4, "Run-coded records for the
 * link". */
#define MI355_RUNS_WHERE_SMALLER 0
#define MI355_RUNS_ALWAYS 1
#define MI355_RUNS_FORM_COMPACT 0u
#define MI355_RUNS_FORM_RUNS 1u
size_t mi355_cwire_runs_frame_bytes(uint32_t n, uint32_t e, uint32_t r);
size_t mi355_cwire_runs_bytes_max(size_t frame_bytes, int nrecords, int policy);
int mi355_cwire_runs_encode_host(size_t frame_bytes, const void *cwire, size_t cwire_bytes, const uint32_t *h_counts,
                                 const uint32_t *h_escapes, int nrecords, int policy, uint32_t *forms /* [nrecords][4] */,
                                 uint64_t *pos /* [nrecords + 1] */, void *out, size_t capacity_bytes);
int mi355_cwire_runs_encode_batch(mi355_core *core, const void *d_cwire_in, const uint32_t *h_counts, const uint32_t *h_escapes,
                                  int nrecords, int policy, void *d_forms, void *d_pos, void *d_out, size_t capacity_bytes);
int mi355_cwire_runs_decode_host(size_t frame_bytes, const void *in, size_t in_bytes, const uint32_t *h_forms, int nrecords,
                                 uint64_t *frame_pos /* [nrecords + 1] */, void *cwire_out, size_t capacity_bytes);
int mi355_cwire_runs_decode_batch(mi355_core *core, const void *d_in, const uint32_t *h_forms, int nrecords, void *d_frame_pos,
                                  void *d_cwire_out, size_t capacity_bytes);

/* A tick held to a budget: the sender's rate control.  The nstreams compact records mi355_diff_multi_cwire_batch just wrote
 * (back to back where h_counts[s] / h_escapes[s] put them; the headers come from the host and are not trusted in the buffer, as
 * in mi355_apply_multi_cwire_batch) and the caller's states as that tick left them (stream s at d_states + s*stride_bytes) ->
 * records of at most h_budget[s] entries each (UINT32_MAX: no limit), the largest changes kept.  What is not sent is not lost:
 * the state goes back to the previous value there, so the change stays pending and is sent on a later tick if it persists --
 * the negative feedback of the diff itself, with the threshold raised for one camera for one tick.
 *   Semantics: T0 = the core's threshold.  For an entry (x, d) of stream s let cur = state[s][x], prev = (uint8)(cur - d) and
 *   a = |cur - prev| as integers, 1 .. 255 -- taken from the STATE: (uint8)df is the same byte for df and df +- 256, the diff
 *   byte alone does not give the magnitude.  T_s = the least T in [T0, 255] such that at most h_budget[s] entries have a > T
 *   (T = 255 keeps nothing, so T_s exists).  Entries of equal magnitude cannot be told apart: when more than h_budget[s] of them
 *   share the largest magnitude, T_s passes all of them and this tick sends none of them (they stay pending).
 *   Outputs: d_thresholds, uint32[nstreams], receives T_s.  Record s at d_cwire_out + d_frame_pos[s] is the canonical encoding
 *   (ascending indices, pad bytes zero, headers written) of the entries with a > T_s; d_offsets, uint32[nstreams + 1], is the
 *   exclusive scan of the kept counts; d_frame_pos, uint64[nstreams + 1], is always exact.  state[s][x] = prev at every dropped
 *   entry.
 *   Guarantees: records, offsets, frame positions and states are byte for byte what mi355_diff_multi_cwire_batch of a core with
 *   threshold T_s would have left from the same frames and the same states before the tick (the entries of a tick at T' >= T
 *   are a subset of those at T, and the states differ exactly at the dropped ones).  A stream within its budget comes back
 *   byte for byte and its state is not written (not even read).  Capacity rule of the family: a record with d_frame_pos[s + 1]
 *   > capacity_bytes is skipped whole and the ones behind it that fit are written; the states are thinned completely
 *   regardless; mi355_cwire_bytes_max(N, nstreams) always suffices.  Bytes of the states' region outside the N bytes of each
 *   state are never written, the stride gap included (every state store is a single byte).
 *   Malformed content under consistent headers: the guarantees of mi355_cwire_coalesce_cwire_batch -- nothing is read outside
 *   the input span or the states, nothing is written outside the outputs and the N bytes of each state, an index >= N and an
 *   escape ranked at or past e contribute nothing; that stream's own result is otherwise unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: a null core; nstreams outside [0, max_batch]; with
 *   nstreams > 0 a null pointer among the arguments; h_escapes[s] > h_counts[s]; h_counts[s] > N; stride_bytes < N; d_cwire,
 *   d_cwire_out, d_offsets or d_thresholds not 4-byte aligned; d_frame_pos not 8-byte aligned; the input span (known from the
 *   host's headers) overlapping an output region or the states' region [d_states, d_states + (nstreams-1)*stride_bytes + N); an
 *   output region (offsets, thresholds, frame_pos, [d_cwire_out, + capacity_bytes)) overlapping the states' region.
 *   nstreams == 0 writes offsets[0] = 0 and frame_pos[0] = 0 and nothing else.
 * Asynchronous on the core's stream, behind the last expansion of this core as every consumer of a packed stream is, so it may
 * follow mi355_diff_multi_cwire_batch on one core without a synchronisation of the device work (the host still needs the
 * headers); a later tick on the same states sees every byte this call wrote; with a caller's stream everything runs on it in
 * call order.  Nothing is allocated inside the call: the 258 words per stream it needs beyond the directory scratch of
 * mi355_apply_cwire_batch (256 bins, budget, threshold) are made with the core, max_batch of them, and counted by
 * mi355_workspace_bytes.
 * The directory kernels of mi355_apply_cwire_batch on the nstreams records, then a grid of 4096-byte tiles x streams three
 * times, one wave per tile, a tile no entry lands in returning on its directory word: (1) streams over their budget only: the
 * tile of differences rebuilt in LDS, the same tile of the state beside it, a per entry into a 256-bin histogram in LDS, one
 * global atomic per nonzero bin; one workgroup per stream then sums the bins from the top for T_s; (2) the tile again with the
 * entries of a <= T_s zeroed -> the coalescer's facts, its scan and its placement; (3) the same filtered tile from the same
 * bytes, the dropped entries' state bytes stored (the only pass that writes the state is the last that reads it; a tile of a
 * record that is skipped for lack of room still reverts), the kept entries written as the coalescer writes them.  A stream
 * with T_s == T0 skips the state in every pass.  The cost follows the entries and their tiles, not N.
 * Out of scope: the stream forms (nframes frames chained through one state: frame t + 1 depends on how frame t was thinned);
 * the per-frame host path (mi355_exec_cwire, mi355_pipe_submit_cwire); an arrays or plain-wire output form.
 * Not measured yet: tools/bench_multi.py --legs budget writes profiles/multi_budget.json (microseconds per stream of this call
 * with budgets at half of each stream's count, against a second mi355_diff_multi_cwire_batch over the same frames -- the
 * cheapest re-diff a caller has without it, and one that still lacks the threshold choice; 1080p, webcam-like input, S = 4, 16,
 * 64, median of five rounds, same run, same board).  The expectation to test -- cheaper than that second diff at every S -- is
 * neither met nor missed until that file exists.  DESIGN.md section 4, "Holding a tick to a budget". */
int mi355_cwire_budget_cwire_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                                   void *d_states, size_t stride_bytes, int nstreams, const uint32_t *h_budget,
                                   void *d_thresholds, void *d_offsets, void *d_frame_pos, void *d_cwire_out,
                                   size_t capacity_bytes);
/* Host only, no core: the largest n such that EVERY record of n entries of a frame of frame_bytes bytes fits in record_bytes --
 * the largest n <= frame_bytes with 8 + 2*pad4(n) + 4*min(n, frame_bytes/256) <= record_bytes (an escape spans at least 256
 * bytes of the frame), 0 when record_bytes < 8.  A sender turns its per-socket byte budget into h_budget[s] with it. */
size_t mi355_cwire_budget_entries(size_t frame_bytes, size_t record_bytes);

/* A tick without its speckle: the sender's second lever, keyed on the neighbourhood instead of the magnitude.  The nstreams compact
 * records mi355_diff_multi_cwire_batch just wrote (placed by h_counts[s] / h_escapes[s]; the headers come from the host, as in
 * mi355_cwire_budget_cwire_batch) and the caller's states as that tick left them -> records without the entries of isolated
 * pixels (state s at states + s*spacing_bytes, the stride of the states as in the budget call).  What is not sent is not lost: the
 * state goes back to the previous value there, so the change stays pending.  A
 * sender that wants both runs this call first and the budget call on what is left.
 *   Semantics, for stream s, frame width x height, P = width*height, N = 3P:
 *   Changed pixel: pixel p is changed if record s holds an entry with index x < N, a nonzero diff byte and x / 3 == p (a zero
 *   diff byte is no entry, as in the coalescer; records of this library hold none).
 *   Neighbour count: c(p) = the changed pixels among (px + dx, py + dy), dx, dy in {-1, 0, 1} and not both 0, inside the frame,
 *   with px = p % width and py = p / width.  Pixels outside the frame count 0; the other channels of p itself do not count.
 *   Keep or drop: need = h_need[s], 0 .. 8.  0: the stream passes through byte for byte, its state is neither read nor written.
 *   Otherwise an entry (x, d) is kept iff c(x / 3) >= need: all entries of a pixel share its fate.
 *   Revert: for a dropped entry state[s][x] = (uint8)(state[s][x] - d), the value before the tick (the budget call's revert).
 *   Outputs: record s at d_cwire_out + d_frame_pos[s] is the canonical encoding (ascending indices, pad bytes zero, header
 *   written) of the kept entries; d_offsets, uint32[nstreams + 1], is the exclusive scan of the kept counts; d_frame_pos,
 *   uint64[nstreams + 1], is always exact; d_dropped, uint32[nstreams], receives the entries dropped per stream.  Capacity rule
 *   of the family: a record with d_frame_pos[s + 1] > capacity_bytes is skipped whole and later ones that fit are still written;
 *   the states are reverted completely regardless; mi355_cwire_bytes_max(N, nstreams) always suffices.
 *   Guarantees: (1) Equals a diff on blanked frames: with frames' = the tick's frames with every byte of every dropped pixel
 *   replaced by the state byte before the tick, the records, offsets, frame positions and states are byte for byte what
 *   mi355_diff_multi_cwire_batch leaves from frames' and the states before the tick: sender and receiver stay equal.  (2) A stream
 *   with nothing to drop comes back byte for byte and its state is not written.  (3) Bytes of the states' region outside the N
 *   bytes of each state are never written; state stores are single bytes.  (4) Malformed content under consistent headers gets
 *   the budget call's promise: nothing is read outside the input span and the states, nothing is written outside the outputs
 *   and the N bytes of each state, an index >= N and an escape ranked at or past e contribute nothing; only that stream's own
 *   result is otherwise unspecified.  (5) No stale scratch: consecutive calls on one core are independent, whatever the earlier
 *   call's nstreams, h_need or records were.
 * mi355_cwire_despeckle_host is the definition: plain C++ on host memory, no core, no HIP call, no alignment requirement.  It
 * validates every record as mi355_cwire_apply_host does and refuses with MI355_ERR_INVALID and a reason, before anything is
 * written: a truncated record, n > N, e > n, a count of 255 codes that is not e, an index >= N; h_need[s] > 8; a null pointer
 * with nstreams > 0; nstreams < 0; width < 1; height < 1; spacing_bytes < N.
 * The batch form refuses with MI355_ERR_INVALID before anything is launched or written: a null core; nstreams outside
 * [0, max_batch]; with nstreams > 0 a null pointer among the arguments; h_escapes[s] > h_counts[s]; h_counts[s] > N;
 * h_need[s] > 8; spacing_bytes < N; d_cwire_in, d_cwire_out, d_offsets or d_dropped not 4-byte aligned; d_frame_pos not 8-byte
 * aligned; the input span overlapping an output region or the states' region; an output region (offsets, dropped, frame_pos,
 * [d_cwire_out, + capacity_bytes)) overlapping the states' region.  nstreams == 0 writes offsets[0] = 0 and frame_pos[0] = 0
 * and nothing else.  Asynchronous on the core's stream, behind the last expansion of this core, so it may follow
 * mi355_diff_multi_cwire_batch on one core without a synchronisation of the device work; a later tick on the same states sees
 * every byte this call wrote.
 * Scratch: two bitmaps of one bit per pixel and stream (changed, keep), 2 * max_batch * 4 * ceil(P / 32) bytes, made by the
 * first call that needs them or by mi355_prepare(core, MI355_PREPARE_DESPECKLE) and counted by mi355_workspace_bytes from then
 * on; after the prepare nothing is allocated inside the call.
 * The directory kernels of mi355_apply_cwire_batch on the nstreams records, then, one wave per 4096-byte tile x stream and a
 * tile no entry lands in returning on its directory word: the changed bitmap of the filtered streams zeroed; (1) the tile of
 * differences rebuilt in LDS, its changed pixels OR-ed into the bitmap, one atomic per nonzero word; (2) a lane per 32 pixels
 * on the bitmap alone: the eight neighbour bitmaps by bit shifts (distance 1 and width - 1, width, width + 1, the first and last
 * column masked), added bit-parallel and compared with need -> the keep bitmap.  This pass reads and writes N/24 bytes per
 * filtered stream and is the only cost of the call that follows N and not the entries; (3) the tile again with the entries of
 * the pixels not kept zeroed -> the coalescer's facts, its scan and its placement, the dropped entries counted; (4) the same
 * filtered tile from the same bytes, the dropped entries' state bytes reverted by single-byte loads and stores (the state is
 * touched nowhere else; a tile of a record that is skipped for lack of room still reverts), the kept entries written as the
 * coalescer writes them.
 * Out of scope: the burst forms (frame t + 1 depends on how frame t was filtered); the per-frame host path; an arrays or
 * plain-wire output; another neighbourhood than the 8 surrounding pixels; despeckle and budget in one call.
 * Measured (profiles/multi_despeckle.json: tools/bench_multi.py --legs despeckle; microseconds per stream of this call at need = 3
 * against mi355_cwire_budget_cwire_batch on the same records with budgets at half the counts; 1080p, S = 4, 16, 64, median of
 * five rounds, spread 0.4 to 2.2 %, same run, same board): webcam-like input 52.9 / 38.5 / 28.5 against the budget call's 45.6 /
 * 25.0 / 20.5, with 547 235 entries in and 56 455 out at S = 4 (bytes 1 105 716 -> 135 348), equal to the host form's; local input
 * (nothing to drop) 22.2 / 7.7 / 4.0 against 23.7 / 9.0 / 5.1.  The expectation -- no slower than the budget call at any S by
 * more than the rounds' spread plus the N/24 bitmap pass -- is MISSED on the webcam-like input (1.16x to 1.54x, where nine of ten
 * entries are dropped and each costs a byte load and store to the state) and met on the local input.  DESIGN.md section 4,
 * "Dropping isolated changes". */
int mi355_cwire_despeckle_host(int width, int height, const void *cwire, size_t cwire_bytes, const uint32_t *h_counts,
                               const uint32_t *h_escapes, uint8_t *states, size_t spacing_bytes, int nstreams,
                               const uint32_t *h_need, uint32_t *dropped, uint32_t *offsets, uint64_t *frame_pos,
                               void *cwire_out, size_t capacity_bytes);
int mi355_cwire_despeckle_cwire_batch(mi355_core *core, const void *d_cwire_in, const uint32_t *h_counts, const uint32_t *h_escapes,
                                      void *d_states, size_t spacing_bytes, int nstreams, const uint32_t *h_need, void *d_dropped,
                                      void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes);

/* Where a camera moves: per stream, a grid of counts of its records' entries and a bounding box, made on the GPU from the records
 * a node already holds -- a recorder that keeps footage only while something moves, a wall that frames the active cameras, a
 * sender that hands its socket budget to the cameras with motion download 32 bytes per camera instead of 4n bytes of indices.
 * Inputs, batch index b = s*nframes + t (nframes == 1: one tick of nstreams cameras; nstreams == 1: one stream's batch):
 *   mi355_activity_batch        d_offsets, uint32[nstreams*nframes + 1], over d_xs -- what mi355_diff_multi_batch /
 *                               mi355_diff_multi_stream_batch wrote (d_diff is not needed); d_xs is read as uint32
 *   mi355_cwire_activity_batch  compact records back to back where h_counts[b] / h_escapes[b] put them; the header words in the
 *                               buffer are skipped, not trusted, as in mi355_apply_multi_stream_cwire_batch
 *   Semantics: an entry with byte index x < N is a changed byte of pixel p = x / 3, column px = p % width, row py = p / width, and
 *   counts 1 in cell (py / cell_h) * grid_w + px / cell_w (mi355_activity_cells gives grid_w and the cells per stream).  An index
 *   >= N contributes nothing.  Counts are of changed BYTES, the unit of h_pos and n: a pixel whose three channels changed counts
 *   3, an index present in two records of a burst counts twice.
 *   Outputs, per stream s: d_cells, uint32[nstreams][grid_w*grid_h], the entries of the stream's nframes records per cell;
 *   d_summary, uint32[nstreams][8]:
 *     0     entries counted (x < N)
 *     1, 2  x0, y0: least column and row of a counted entry, in pixels; UINT32_MAX when word 0 is 0
 *     3, 4  x1, y1: greatest column and row, inclusive; 0 when word 0 is 0
 *     5     active cells: cells whose count is >= min_count
 *     6     peak: the largest cell count
 *     7     index of the peak cell, the lowest among equals; 0 when word 6 is 0
 *   accumulate == 0: the nstreams grids are cleared and the summaries set to the empty values first.  accumulate != 0: the call
 *   adds onto what d_cells and d_summary hold -- from an earlier call with the same geometry and nstreams, or the empty values:
 *   counts and word 0 add (uint32 wrap-around), the box widens, words 5 to 7 are recomputed from the accumulated grids.  A burst
 *   in one call equals its records fed one tick at a time with accumulate set; a running motion picture over a time window is a
 *   sequence of accumulating calls.
 *   Guarantees: nothing is written outside d_cells (4 * nstreams * cells bytes) and d_summary (32 * nstreams bytes); the core's
 *   state is neither read nor written.  Malformed compact content under consistent headers: the guarantees of
 *   mi355_apply_multi_stream_cwire_batch -- nothing is read outside the input span, an escape ranked at or past e and an index
 *   >= N contribute nothing; only that stream's own grid and summary are otherwise unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: a null core; nstreams or nframes < 0; nstreams*nframes
 *   > max_batch; cell_w < 1, cell_h < 1 or min_count < 1; d_cwire, d_offsets, d_xs, d_cells or d_summary not 4-byte aligned; with
 *   nstreams*nframes > 0 a null pointer among the arguments, h_escapes[b] > h_counts[b], h_counts[b] > N, or (compact form) the
 *   input span known from the host's headers overlapping either output region.  nstreams*nframes == 0 does nothing.  A cell larger
 *   than the frame is valid: a grid of one cell.
 * Asynchronous on the core's stream, behind the last expansion of this core as every consumer of a packed stream is:
 * mi355_diff_multi_batch followed by mi355_activity_batch on one core needs no synchronisation in between; with a caller's stream
 * everything runs on it in call order.  Nothing is allocated inside the call; the compact form uses the directory scratch of
 * mi355_apply_cwire_batch and nothing else of the core.
 * Compact form: the directory kernels of mi355_apply_cwire_batch on the nstreams*nframes records, a clear launch (skipped when
 * accumulating), then a grid of 4096-byte tiles x streams, one wave per tile: the wave finds the records of its stream that have
 * an entry in the tile (a lane per record, a ballot per 64) and returns if there are none -- no state byte moves, the cost follows
 * the changes; else it walks those entries with the decode loop of the apply calls, counts them per pixel in LDS (a tile holds at
 * most 1366 pixels; no global atomic per entry), folds the pixels to cells 64 at a time -- indices ascend, so the cells along a row
 * form runs, and a scan sums each run -- with one global atomic per run, and reduces entries and box in the wave to one atomic per
 * word.  One workgroup per stream then reduces the finished grid to words 5 to 7.  Row, column and cell come from exact divisions
 * by multipliers the host prepares, for every width and cell size.
 * Arrays form: the clear and summary launches around ONE launch in which a lane takes an entry, finds its segment by binary search
 * in the offsets (as mi355_apply_multi_batch does) and a wave merges equal neighbouring cells before its atomics.  This form is
 * not tuned further.
 * Not measured yet: tools/bench_multi.py --legs activity --streams 4,16,64 writes profiles/multi_activity.json (microseconds per
 * record of the compact form, 16x16 cells, 1080p, median of five rounds with the spread, webcam-like input and a block moving on
 * a still background, S = 4, 16, 64 with T = 1 and S = 16 with T = 16, against mi355_apply_multi_stream_cwire_batch without output
 * frames on the same records in the same run on the same board -- the same directory kernels and entry walk, plus the state
 * tiles it moves).  The expectation to test -- no slower than that apply at any point by more than the rounds' spread -- is
 * neither met nor missed until that file exists.
 * DESIGN.md section 4, "Where a record lands: motion grids". */
int mi355_activity_batch(mi355_core *core, const void *d_offsets, const void *d_xs, int nstreams, int nframes, int cell_w,
                         int cell_h, uint32_t min_count, int accumulate, void *d_cells, void *d_summary);
int mi355_cwire_activity_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                               int nstreams, int nframes, int cell_w, int cell_h, uint32_t min_count, int accumulate,
                               void *d_cells, void *d_summary);
/* Host only, no core: cells of the grid; *grid_w = ceil(width / cell_w), *grid_h = ceil(height / cell_h) (either may be NULL);
 * returns grid_w * grid_h, 0 (and 0 in both) for width, height, cell_w or cell_h < 1. */
size_t mi355_activity_cells(int width, int height, int cell_w, int cell_h, int *grid_w, int *grid_h);

/* The client's side, client/opencv.cpp:50-66: for every frame in order, state[xs[i]] += diff[i] (uint8
 * wrap-around) on the core's state (a client core is a core whose state was set to the received base frame,
 * opencv.cpp:38-46).  d_frames_out != NULL: the reconstructed frame t is also copied to d_frames_out +
 * t*stride_bytes (what the client shows, opencv.cpp:68); NULL: only the state advances, all frames in one
 * launch.  Indices >= N are ignored.  Asynchronous on the core's stream. */
int mi355_apply_batch(mi355_core *core, const void *d_offsets, const void *d_xs, const void *d_diff,
                      int nframes, void *d_frames_out, size_t stride_bytes);
/* Same from the wire bytes; h_counts[t] (host) are the headers the client has read from the socket
 * (opencv.cpp:52), the header words inside d_wire are skipped, not trusted. */
int mi355_apply_wire_batch(mi355_core *core, const void *d_wire, const uint32_t *h_counts, int nframes,
                           void *d_frames_out, size_t stride_bytes);

/* Several cores may each own a row band of ONE stream (bands are contiguous byte ranges of the frame, so a
 * band is a core of the band's height fed with d_frames + band_start).  After the
 * bands' streams have been gathered back to back (part p's entries at h_part_base[p], its own index
 * d_part_offsets[p][0..nframes]), this merges them into the single stream of the whole frame: frame t =
 * the parts' frame-t segments in part order, xs + h_xs_bias[p] (the band's first byte). */
int mi355_merge_parts(mi355_core *core, int nparts, int nframes, const void *d_part_offsets,
                      const uint32_t *h_part_base, const int32_t *h_xs_bias, const void *d_xs_all,
                      const void *d_diff_all, void *d_offsets, void *d_xs, void *d_diff, size_t capacity);

/* ---- compact wire format: the same stream as the wire form above in about 2/5 of the bytes ----------------------------
 * Each index is coded as its gap from the previous one, which nearly always fits one byte.  One record per frame, records
 * back to back, each 4-byte aligned from the start of the buffer; all integers little-endian; pad4(x) = x rounded up to a
 * multiple of 4:
 *     u32 n                 entries of the frame (h_pos; the same entries, in the same ascending order, as the packed stream)
 *     u32 e                 escaped gaps
 *     u8  code[n]           g_0 = xs[0], g_k = xs[k] - xs[k-1] - 1;  code[k] = g_k if g_k < 255, else 255 (escape)
 *     u8  0[pad4(n) - n]
 *     u32 esc[e]            g_k of every k with code[k] == 255, in k order
 *     u8  diff[n]           (uint8)df, as diff[] of the wire form
 *     u8  0[pad4(n) - n]
 * A record is mi355_cwire_frame_bytes(n, e) = 8 + 2*pad4(n) + 4*e bytes.  An escape spans at least 256 indices, so e <= N/256
 * and a frame never needs more than 8 + 2*pad4(N) bytes (mi355_cwire_bytes_max: nframes times that).  The encoding is
 * canonical: one byte string per (xs, diff), pad bytes zero.  The reference's client cannot read it. */
size_t mi355_cwire_frame_bytes(uint32_t n, uint32_t e);
size_t mi355_cwire_bytes_max(size_t frame_bytes, int nframes);
/* Encodes a packed stream of nframes frames -- of mi355_diff_stream_batch / _pairs_batch, mi355_merge_parts or a rank's
 * segment of the group gather -- into records: frame t at byte d_frame_pos[t] (uint64[nframes + 1], exclusive scan of the
 * record sizes; d_frame_pos[nframes] = the bytes of the whole batch).
 *   Precondition: entries strictly ascending within each frame, as every entry point of this library emits them.
 *   Frame t is written only if d_frame_pos[t + 1] <= capacity_bytes; a frame that does not fit is skipped whole (nothing of
 *   it is written); d_frame_pos is exact regardless.
 *   offsets[nframes] > entries_capacity (the diff batch dropped entries), or offsets that run backwards: nothing is read
 *   from d_xs / d_diff, nothing is written but d_frame_pos[nframes] = UINT64_MAX.
 *   d_cwire, d_offsets and d_xs 4-byte aligned, d_frame_pos 8-byte aligned; nframes <= 8192.  Asynchronous on the core's
 *   stream; three kernel launches, the stores are dwords. */
int mi355_cwire_encode_batch(mi355_core *core, const void *d_offsets, const void *d_xs, const void *d_diff,
                             size_t entries_capacity, int nframes, void *d_frame_pos, void *d_cwire, size_t capacity_bytes);
/* The inverse, into a packed stream (d_offsets uint32[nframes + 1], d_xs int32, d_diff uint8), for mi355_apply_batch.  The
 * headers come from the host as the client read them from the socket: h_counts[t] = n, h_escapes[t] = e (the header words
 * inside d_cwire are skipped, not trusted); the records are where those headers put them.  Entries beyond `capacity` are
 * dropped, d_offsets stays exact.  Malformed content never makes it read outside a frame's record or write outside its
 * outputs: an escape code ranked at or past e decodes to index 0xFFFFFFFF (mi355_apply_batch ignores it).  h_escapes[t] >
 * h_counts[t] is refused.  Same alignment as the encoder.  Asynchronous on the core's stream. */
int mi355_cwire_decode_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                             int nframes, void *d_offsets, void *d_xs, void *d_diff, size_t capacity);
/* A GPU client in one call: client/opencv.cpp:50-66 straight from the records.  For each record t in order, state[x] += diff
 * (uint8 wrap-around) on the core's state; d_frames_out != NULL: the reconstructed frame t is also written to
 * d_frames_out + t*stride_bytes (whole 16-byte stores when d_frames_out and stride_bytes are multiples of 16, any
 * alignment works); NULL: only the state advances.  The headers come from the host, as for mi355_cwire_decode_batch:
 * h_counts[t] = n, h_escapes[t] = e; the records lie back to back where those headers put them and the header words inside
 * d_cwire are skipped, not trusted.
 *   Well-formed records: the state and every output frame are bit-identical to mi355_cwire_apply_host, and to
 *   mi355_cwire_decode_batch followed by mi355_apply_batch (in both modes).
 *   Malformed content (with consistent headers) stays memory-safe: nothing is read outside the records' span, nothing is
 *   written outside the state and the nframes output frames (not into the stride gap either).  An escape ranked at or past
 *   e and an index >= N change nothing; beyond that the bytes of a malformed frame's result are unspecified.
 *   Refused with MI355_ERR_INVALID before anything is launched: nframes < 0; a null d_cwire, h_counts or h_escapes when
 *   nframes > 0; h_escapes[t] > h_counts[t]; h_counts[t] > N; d_cwire not 4-byte aligned; stride_bytes < N with
 *   d_frames_out set.
 * nframes has no upper bound: longer batches are applied in slices of max_batch frames.  Scratch of the core, allocated with
 * it and counted by mi355_workspace_bytes: max_batch * (24 + 32 * ceil(N / 4096)) bytes (12.5 MB at 1080p with max_batch
 * 256).  Asynchronous on the core's stream; per slice six kernel launches and one more per 128 frames, no copies. */
int mi355_apply_cwire_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                            int nframes, void *d_frames_out, size_t stride_bytes);
/* A client without a GPU: client/opencv.cpp:50-66 on the compact stream, state[xs] += diff for nframes records of host
 * memory `cwire` (cwire_bytes bytes) on a host frame of frame_bytes bytes.  No core, no HIP call.  Every frame is validated
 * before it is applied; MI355_ERR_INVALID (with the reason in mi355_last_error) for a truncated record, n > frame_bytes,
 * e > n, a count of 255 codes other than e, a decoded index >= frame_bytes, a null pointer or nframes < 0.  The frames
 * before a bad one stay applied and *consumed = their bytes (on success: all bytes of the nframes records). */
int mi355_cwire_apply_host(uint8_t *state, size_t frame_bytes, const void *cwire, size_t cwire_bytes, int nframes,
                           size_t *consumed);

/* Checking records before they are used: one verdict of four words per record, from the record's bytes alone -- no state, so a
 * relay that coalesces bursts, a recorder that keeps every T-th picture or a wall that asks for motion grids can tell a good
 * record from a damaged one before it forwards, counts or applies it.  The GPU consumers of compact records promise memory
 * safety under malformed content and nothing more; the directory kernels of mi355_apply_cwire_batch keep the running index in
 * 32 bits, so a record whose escape values sum past 2^32 wraps to a small index and is applied somewhere inside the frame.  The
 * check cannot wrap.
 * The records lie back to back where h_counts[b] = n and h_escapes[b] = e put them, as in every other call of the family; the
 * header words in the buffer are compared (BAD_HEADER) and never used to find anything.
 *   Decode rule (that of the GPU clients), with unbounded integers: walk k = 0 .. n-1 with escape rank r = 0 and running total
 *   X = 0; c = code[k]; c < 255: X += c + 1; else if r < e: X += esc[r] + 1, r++; else r++ and X stays (a bad escape).  X_k is X
 *   after step k; entry k has index X_k - 1.
 *   Verdict of record b, uint32[4]:
 *     0  the flags below, or'ed; 0: well-formed and canonical
 *     1  the number of 255 codes among the n codes (the final r)
 *     2  the least k with X_k > N; n when there is none
 *     3  min(X_{n-1}, 0xFFFFFFFF): 1 + the last decoded index, saturated; 0 for n = 0
 *   BAD_CODES: word 1 != e.  BAD_RANGE: word 2 < n.  BAD_ESCAPE: some esc[r] < 255 with r < min(e, word 1).  BAD_PAD: one of the
 *   2 * (pad4(n) - n) pad bytes is not zero.  BAD_HEADER: the {n, e} words in the buffer differ from h_counts[b] / h_escapes[b].
 *   Properties: a record whose BAD_HEADER bit is clear is accepted by mi355_cwire_apply_host on a frame of N bytes exactly when
 *   BAD_CODES and BAD_RANGE are clear.  Word 0 == 0 exactly when the record's bytes equal the canonical encoding of what it
 *   decodes to -- what mi355_cwire_encode_batch would write.  No sum wraps: a total of 2^32 or more is BAD_RANGE, whatever it
 *   is modulo 2^32 (N < 2^32 - 1).
 * mi355_cwire_check_host is the definition: host memory, no alignment, no core, no HIP call.  Refused with MI355_ERR_INVALID,
 * the verdicts untouched: a null pointer with nrecords > 0; nrecords < 0; h_escapes[b] > h_counts[b]; h_counts[b] > frame_bytes;
 * frame_bytes >= 2^32 - 1; records that, by the headers, end past cwire_bytes.
 * mi355_cwire_check_batch is the same on the GPU, N the core's frame bytes, d_verdicts uint32[nrecords][4], bit-identical to the
 * host form.  Refused with MI355_ERR_INVALID before anything is launched or written: a null core; nrecords outside
 * [0, max_batch]; with nrecords > 0 a null pointer among the arguments, h_escapes[b] > h_counts[b], h_counts[b] > N, d_cwire
 * or d_verdicts not 4-byte aligned, or the input span known from the headers overlapping the 16 * nrecords verdict bytes.
 * nrecords == 0 does nothing.
 *   Guarantees: nothing is read outside the span that the host's headers give, nothing is written outside the verdicts, the
 *   core's state is neither read nor written, nothing is allocated inside the call (the chunk table of mi355_apply_cwire_batch's
 *   directory scratch is reused, sized for max_batch records).  Asynchronous on the core's stream, behind the last expansion of
 *   this core: mi355_diff_multi_cwire_batch followed by the check on one core needs no synchronisation in between.
 *   Kernels: the chunk table and the first two passes of the directory (per chunk of 4096 codes: its 255 codes and the sum of
 *   the other codes' g + 1; per record: each chunk's first escape rank), then per chunk the escaped gaps of its ranks below e
 *   added in 64 bits and clamped to 0xFFFFFFFF (clamped addition is associative: exact below 2^32, stuck at the top above),
 *   with the escape values < 255 and the last chunk's pad bytes noted; then one workgroup per record scans the chunk sums, walks
 *   the one chunk whose prefix is the first above N for word 2 with the decode step of the GPU clients, compares the header and
 *   stores the verdict.  Four launches and one more per 128 records; the records are read about twice, no state tile moves.
 * Not measured yet: tools/bench_multi.py --legs check --streams 4,16,64 writes profiles/multi_check.json (microseconds per record,
 * 1080p, median of five rounds with the spread, webcam-like input and a block moving on a still background, S = 4, 16, 64 with
 * T = 1 and S = 16 with T = 16, against mi355_apply_multi_stream_cwire_batch without output frames on the same records in the
 * same run on the same board).  The expectation to test -- no slower than that apply at any point by more than the rounds'
 * spread -- is neither met nor missed until that file exists.
 * DESIGN.md section 4, "Checking records before they are used". */
#define MI355_CWIRE_BAD_CODES   1u  /* the number of 255 codes among the n codes is not e                 */
#define MI355_CWIRE_BAD_RANGE   2u  /* an entry decodes to an index >= N                                  */
#define MI355_CWIRE_BAD_PAD     4u  /* a pad byte behind code[n) or diff[n) is not zero                   */
#define MI355_CWIRE_BAD_ESCAPE  8u  /* a used escape value is < 255 (it should have been a code)          */
#define MI355_CWIRE_BAD_HEADER 16u  /* the {n, e} words in the buffer differ from h_counts / h_escapes    */
int mi355_cwire_check_host(size_t frame_bytes, const void *cwire, size_t cwire_bytes, const uint32_t *h_counts,
                           const uint32_t *h_escapes, int nrecords, uint32_t *verdicts /* [nrecords][4] */);
int mi355_cwire_check_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                            int nrecords, void *d_verdicts /* uint32[nrecords][4] */);

/* ---- Resynchronising a receiver: tile digests, refresh records, tile clears ------------------------------------------------
 * Compact records are additive (state[x] += diff, mod 256): a receiver is right only while it applies every record of a camera
 * exactly once.  After a record it refused (mi355_cwire_check_batch), lost, or never saw because it joined late, every later
 * record lands on a wrong state and the error never decays.  These calls let it find out and let the sender repair it with
 * ordinary records, tile by tile.
 *   tiles = ceil(N / 4096); tile t of a state is its bytes [4096 t, min(N, 4096 (t + 1))) -- the grid of the apply kernels;
 *   mask_words = ceil(tiles / 32).
 * The protocol, in the order of the socket:
 *   up    the receiver's digests, uint32[S][tiles][2] (mi355_state_digest_batch on its states; 8 bytes per 4096 of a state);
 *   down  behind the sender's latest tick: the tile mask, uint32[S][mask_words], and one refresh record per camera
 *         (mi355_refresh_cwire_batch on the sender's states and the receiver's digests);
 *   then  the receiver clears the masked tiles (mi355_state_clear_tiles_batch) and applies the refresh records
 *         (mi355_apply_multi_cwire_batch) on one stream with no synchronisation in between, after every tick that came before
 *         them on the socket.  A host client clears the tiles itself and calls mi355_cwire_apply_host.
 * The digests describe the receiver's state of some earlier tick: the tiles that the ticks in flight since then changed differ
 * from the sender's too and are selected as well.  That is wasteful, never wrong: a selected tile is cleared and rewritten whole.
 *
 * The digest of a tile: extend it with zero bytes to 4096 bytes, read them as little-endian words w_i, i = 0 .. 1023;
 *   word 0 = sum of w_i                                       mod 2^32
 *   word 1 = sum of h(w_i ^ (0x9E3779B9 * (i + 1) mod 2^32))  mod 2^32
 *   h(v): v ^= v >> 16; v *= 0x85EBCA6B; v ^= v >> 13; v *= 0xC2B2AE35; v ^= v >> 16   (mod 2^32; a bijection)
 * Properties: a change confined to one 4-byte word always changes word 0.  Word 1 depends on position: words that moved or were
 * swapped show there (for nearly every pair of unequal words), where word 0 stays.  The digest is NOT cryptographic: it guards
 * against loss and damage, not against an adversary.
 * mi355_state_tiles(frame_bytes) is tiles (0 for 0).  mi355_state_digest_host is the definition: host memory, no alignment, no
 * core, no HIP call; digests[tiles][2].  Refused with MI355_ERR_INVALID, the output untouched: a null pointer with
 * frame_bytes > 0.
 * mi355_state_digest_batch: stream s is the N bytes at d_states + s*stride_bytes (any alignment of base and stride, as for the
 * apply calls; stride_bytes == N with N odd included), d_digests uint32[nstreams][tiles][2], bit-identical to the host form.
 * Asynchronous on the core's stream, ordered like every other consumer of the states; nothing is allocated; the core's own state
 * is untouched.  Refused before anything is launched or written: a null core; nstreams outside [0, max_batch]; with
 * nstreams > 0 a null pointer, stride_bytes < N, d_digests not 4-byte aligned, or the digests overlapping the states' region
 * [d_states, + (nstreams - 1)*stride_bytes + N).  nstreams == 0 does nothing.
 *   Kernel: tiles x streams single-wave workgroups.  A whole tile at a 16-byte aligned address is four 16-byte loads per lane,
 *   each load of the wave 1 KiB in one piece; any other tile goes through LDS with the unaligned tile load of the apply kernels,
 *   the bytes past N zeroed there.  Both sums are folded per lane and added across the wave; lane 0 stores the 8 bytes.
 * mi355_refresh_cwire_batch, the sender's answer: tile t of stream s is SELECTED when either word of d_peer_digests[s][t] differs
 * from the digest of the sender's tile, computed inside the call; d_peer_digests == NULL selects every tile (a key frame, for a
 * receiver that joins late).  d_tile_mask[s][t >> 5] has bit t & 31 set exactly for the selected tiles (bits at or past tiles
 * are zero).  Record s, at d_cwire_out + d_frame_pos[s], is the canonical compact encoding of the entries (x, state[s][x]) for
 * every x in a selected tile with state[s][x] != 0, ascending: headers {n, e} written, pad bytes zero, byte for byte what
 * mi355_cwire_encode_batch would write from those entries.  d_offsets uint32[nstreams + 1] is the exclusive scan of the counts,
 * d_frame_pos uint64[nstreams + 1] is always exact.
 *   The guarantee: let R be any N-byte state whose selected tiles are zero.  Record s applied to R -- by mi355_cwire_apply_host,
 *   mi355_apply_multi_cwire_batch, or the coalescer in front of either -- makes the selected tiles equal to the sender's and
 *   leaves the others as they were.  A selected tile that the sender holds all zero has no entry but its mask bit is set: the
 *   receiver clears it.  A stream with no selected tile yields the 8-byte n = 0 record.  The records are ordinary records:
 *   mi355_cwire_check_batch gives word 0 == 0 for each, and activity, coalesce and budget take them.
 *   Capacity, as in the family: a record with d_frame_pos[s + 1] > capacity_bytes is skipped whole, the records behind it that
 *   fit are written; mask, offsets and frame positions are exact regardless.  mi355_cwire_bytes_max(N, nstreams) always suffices.
 *   Refused before anything is launched or written: a null core; nstreams outside [0, max_batch]; with nstreams > 0 a null
 *   pointer other than d_peer_digests, stride_bytes < N; d_peer_digests, d_tile_mask, d_offsets or d_cwire_out not 4-byte
 *   aligned; d_frame_pos not 8-byte aligned; an output region overlapping the states' region, the peer digests or another output
 *   region.  nstreams == 0 writes offsets[0] = 0 and frame_pos[0] = 0 and nothing else; as in the coalescer, either of the
 *   two may be null there and is then skipped, the alignment rules still hold, and no other argument is looked at.  The states
 *   are only read; nothing is
 *   allocated (one fact word per (stream, tile) lives in the directory scratch of mi355_apply_cwire_batch, as in the coalescer).
 *   Kernels: the mask words are cleared on the core's stream; k_rf_facts (tiles x streams, one wave) loads the tile into LDS,
 *   digests it there, compares, and stores the coalescer's tile facts for a selected tile (and ORs its mask bit in, one atomic)
 *   or the all-zero fact; the coalescer's scan and place kernels follow unchanged; k_rf_emit loads the selected tiles that hold
 *   a nonzero byte again and encodes them from LDS with the coalescer's emit step.  The states are read about twice.
 * mi355_state_clear_tiles_batch, the receiver's first step: zeroes the tiles of state s whose bit of d_tile_mask[s] is set, inside
 * the N bytes of the state only -- never the stride gap, never a byte of an unselected tile; byte stores at the ragged ends of an
 * unaligned tile, 16-byte stores inside.  Mask bits at or past tiles are ignored.  Refused as for the digest call, and for a mask
 * that is not 4-byte aligned or overlaps the states.
 * Not measured: tools/bench_multi.py --legs refresh --streams 4,16,64 writes profiles/multi_refresh.json (microseconds per stream,
 * 1080p, webcam-like input, median of five rounds with the spread: the digest call, the refresh with 1 %, 10 % and all tiles
 * selected, the clear, against mi355_diff_multi_cwire_batch on the same streams in the same run on the same board -- the call the
 * sender pays every tick, which reads 2N per stream where the digest reads N).  The expectation to test -- the digest call no
 * slower than that diff at any S by more than the rounds' spread -- is neither met nor missed until that file exists; the other
 * figures are reported, not judged.  The expectation is about streams at 16-byte aligned addresses: a stream at any other
 * address (stride_bytes == N with N no multiple of 16: every stream but the first) sends every tile through the byte loads of
 * the unaligned tile load, as in the apply calls, and is expected to be several times slower; the leg reports that layout too
 * (digest_skewed: base + 1, stride N) without judging it.
 * DESIGN.md section 4, "Resynchronising a receiver". */
size_t mi355_state_tiles(size_t frame_bytes);
int mi355_state_digest_host(const uint8_t *state, size_t frame_bytes, uint32_t *digests /* [tiles][2] */);
int mi355_state_digest_batch(mi355_core *core, const void *d_states, size_t stride_bytes, int nstreams,
                             void *d_digests /* uint32[nstreams][tiles][2] */);
int mi355_refresh_cwire_batch(mi355_core *core, const void *d_states, size_t stride_bytes, int nstreams,
                              const void *d_peer_digests /* uint32[nstreams][tiles][2], or NULL: every tile */,
                              void *d_tile_mask /* uint32[nstreams][mask_words] */, void *d_offsets /* uint32[nstreams + 1] */,
                              void *d_frame_pos /* uint64[nstreams + 1] */, void *d_cwire_out, size_t capacity_bytes);
int mi355_state_clear_tiles_batch(mi355_core *core, void *d_states, size_t stride_bytes, int nstreams, const void *d_tile_mask);

/* ---- A wall of many cameras: thumbnails of many states in one frame, repainted where records landed ---------------------------
 * The third node of the compact wire, next to the relay and the recorder: a receiver that holds S camera states
 * (mi355_apply_multi_stream_cwire_batch) and shows them side by side.  mi355_wall_compose_batch box-downscales the states into
 * thumbnails placed in ONE wall frame; mi355_cwire_touched_tiles_batch says which tiles the records of a tick or burst land in, as
 * the tile mask of mi355_refresh_cwire_batch (uint32[S][mask_words], tiles and mask_words as defined there), and with that mask
 * the compose moves state bytes only where something changed.  All integers, every comparison exact.
 *   The thumbnail of a state (width x height BGR24, N = 3*width*height) at scale k in 1 .. 16 is tw x th pixels,
 *   tw = ceil(width / k), th = ceil(height / k) (mi355_wall_thumb_size: host only, returns tw*th and the two through the pointers
 *   that are not null; 0 and zeros for width or height < 1 or k outside 1 .. 16).  Pixel (u, v), channel c: its block is the
 *   source pixels x in [u*k, min(width, (u + 1)*k)), y in [v*k, min(height, (v + 1)*k)), a their number (the blocks at the right
 *   and bottom edges are smaller when k does not divide the frame), and
 *     value = floor((sum of the block's channel-c bytes + floor(a / 2)) / a).
 *   k = 1 is a copy; a k above the width or the height gives a thumbnail one pixel wide or high.
 *   The wall is BGR24, wall_w x wall_h pixels, pixel (X, Y) at d_wall + Y*wall_pitch + 3*X, wall_pitch >= 3*wall_w; d_wall and
 *   the pitch may have any alignment.  h_place is a HOST array int32[nstreams][3] = {x, y, k}: the thumbnail of stream s (the N
 *   bytes at d_states + s*stride_bytes, any alignment, as for the apply calls) occupies [x, x + tw) x [y, y + th) of the wall;
 *   k == 0: the stream is not shown and nothing of it is read or written.
 * mi355_wall_compose_batch with d_tile_mask == NULL writes every pixel of every shown thumbnail from the current states.  With a
 * mask, a thumbnail pixel of stream s is REQUIRED when its block contains a source pixel p whose bytes [3p, 3p + 3) meet a tile
 * whose bit of d_tile_mask[s] is set (a pixel that straddles a tile edge belongs to both tiles).  Every required pixel is
 * rewritten from the current states; the call may also rewrite any other pixel of the same stream's thumbnail, with that pixel's
 * correct value; a stream with no selected tile has no pixel written; mask bits at or past tiles are ignored.
 *   Both forms: nothing is ever written outside the shown thumbnails' rectangles -- the pitch gap, the wall between the
 *   rectangles and the memory around the wall stay untouched.  The states are only read, the core's own state is untouched,
 *   nothing is allocated.  Asynchronous on the core's stream, in call order behind an apply or a clear on the same core with no
 *   synchronisation in between.  h_place may be reused as soon as the call returns: it travels as kernel arguments, 128 streams
 *   per launch.  Rectangles that overlap each other are not checked: their shared pixels are unspecified among the overlapping
 *   thumbnails' values.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: a null core; nstreams outside [0, max_batch]; with
 *   nstreams > 0 a null d_states, h_place or d_wall, stride_bytes < N, wall_w or wall_h < 1, wall_pitch < 3*wall_w, a k outside
 *   [0, 16], a shown rectangle not inside the wall, a mask that is not 4-byte aligned, the wall's region
 *   [d_wall, + (wall_h - 1)*wall_pitch + 3*wall_w) or the mask overlapping the states' region, or overlapping each other.
 *   nstreams == 0 does nothing.
 *   The property that ties the calls together: if the wall equals the full composition of the states before a tick, then
 *   apply (mi355_apply_multi_stream_cwire_batch), mi355_cwire_touched_tiles_batch of the same records and the masked compose,
 *   with no wait between the three, make it the full composition of the states after the tick.  The same holds for a resync:
 *   mi355_state_clear_tiles_batch, the apply of the refresh records, and the masked compose with the refresh call's own mask.
 *   The masks are one object: a tick's mask and a refresh's mask OR together (accumulate below).
 *   Kernel: k_wall_compose, one for both forms.  A workgroup of 256 threads owns a chunk of one thumbnail row of one stream: a
 *   band of up to k source rows, each a contiguous range of at most 4096 bytes of the state (chunks are multiples of 16 pixels,
 *   so a chunk starts at the alignment of its row).  With a mask it first tests the bits of the tiles those ranges meet and
 *   returns if none is set, before a state byte moves -- which is why correct rewrites beyond the required set are allowed.
 *   Otherwise thread j loads bytes [16j, 16j + 16) of every row of the band (one 16-byte load where the row's address allows
 *   it, bytes otherwise and at the ragged end), adds them vertically in registers as 16-bit sums and puts the sums into LDS; the
 *   threads then produce the chunk's output bytes, consecutive threads consecutive bytes: the sum of up to k LDS entries at a
 *   3-entry pitch, the rounding term, one integer division, one byte store.
 * mi355_cwire_touched_tiles_batch: the records lie back to back where the host's headers put them, batch index
 * b = s*nframes + t, described as for mi355_cwire_activity_batch (the header words in the buffer are skipped, not trusted).  Bit
 * t & 31 of d_tile_mask[s][t >> 5] is set exactly when some record of stream s has an entry whose decoded index x lies in tile t,
 * 4096 t <= x < min(N, 4096 (t + 1)); bits at or past tiles are zero.  accumulate == 0 overwrites the nstreams rows;
 * accumulate != 0 ORs onto what they hold (a refresh mask, the mask of earlier ticks).  It uses the directory kernels of
 * mi355_apply_cwire_batch and nothing else of the core; no state is touched, nothing is allocated; asynchronous on the core's
 * stream.  Malformed content under consistent headers gets the memory-safety guarantees of mi355_cwire_activity_batch: only that
 * stream's own mask words below tiles are unspecified.  Refused before anything is launched or written: a null core; negative
 * counts; nstreams*nframes > max_batch; d_cwire or the mask not 4-byte aligned; with nstreams*nframes > 0 a null pointer,
 * h_escapes[b] > h_counts[b], h_counts[b] > N, or the input span overlapping the mask.  nstreams*nframes == 0 does nothing (no
 * row is written).
 *   Kernel: k_cw_touched behind the directory, a lane per tile (a wave per 64 tiles of a stream).  Each lane walks the stream's
 *   nframes records reading dir[b][tile] and dir[b][tile + 1] -- the touch test of the multi-stream apply; neighbouring lanes read
 *   neighbouring words -- and ORs over t; a ballot gives the wave's two mask words and lane 0 stores them, after a plain load and
 *   OR when accumulating (one wave owns those words).  No atomics.
 * Measured: profiles/multi_wall.json (tools/bench_multi.py --legs wall --streams 4,16,64; microseconds per stream, 1080p,
 * k = 2, 4, 8, median of five rounds, spreads below 3 %, one run on one board).  Both expectations were MISSED.  The full compose
 * at k = 8 takes 2.13 / 1.40 / 1.42 us per stream at S = 4 / 16 / 64 against 1.60 / 1.10 / 1.04 for mi355_state_digest_batch
 * on the same aligned states (1.28 to 1.37 times slower; k = 4: 2.58 / 1.71 / 1.77, k = 2: 4.47 / 3.46 / 3.38).  Touched tiles
 * plus the masked compose on the moving-block tick (367 of 1519 tiles touched) take 12.2 / 3.8 / 1.6 us per stream at k = 8:
 * cheaper than the full compose only at S = 64 with k = 2 (0.80 times), dearer everywhere else (1.08 to 5.7 times), because the
 * touched-tiles call pays the directory's six launches again, 40 to 75 us per call whatever S is; a mask that comes for free (the
 * refresh's) was not measured alone.  The skewed layout (base + 1, stride N: byte loads) takes 8.4 / 6.8 / 7.1 at k = 4, reported
 * and not judged.  DESIGN.md says what bounds both.
 * DESIGN.md section 4, "A wall of many cameras". */
size_t mi355_wall_thumb_size(int width, int height, int k, int *tw, int *th);
int mi355_wall_compose_batch(mi355_core *core, const void *d_states, size_t stride_bytes, int nstreams,
                             const int32_t *h_place /* [nstreams][3] */, const void *d_tile_mask /* or NULL: every tile */,
                             void *d_wall, int wall_w, int wall_h, size_t wall_pitch);
int mi355_cwire_touched_tiles_batch(mi355_core *core, const void *d_cwire, const uint32_t *h_counts, const uint32_t *h_escapes,
                                    int nstreams, int nframes, int accumulate, void *d_tile_mask /* uint32[nstreams][mask_words] */);

/* ---- Thumbnail records: a low-resolution viewer served from full-size states ------------------------------------------------------
 * The node that the wall is not: a REMOTE receiver that wants a camera at 1/k size.  Box averaging with rounding does not commute
 * with state[x] += diff (mod 256), so records cannot be downscaled without state the way they are cropped or placed; this call
 * keeps that state where mi355_diff_multi_* keeps its states -- in the caller's memory -- and does work only where the tick's tile
 * mask says something changed.  Its output is one ordinary compact record per stream of a tw x th frame: mi355_cwire_apply_host,
 * mi355_apply_multi_cwire_batch, mi355_cwire_mosaic_* (sixteen thumbnails as ONE canvas record), mi355_cwire_split_*,
 * mi355_cwire_check_* and the coalescer take it unchanged.  All integers, every comparison exact.
 *   Geometry and value are the wall's: tw = ceil(width / k), th = ceil(height / k), N' = 3*tw*th, k in 1 .. 16
 *   (mi355_wall_thumb_size), value = floor((sum of the block's channel-c bytes + floor(a / 2)) / a).  thumbnail(A) is the N'-byte
 *   BGR24 thumbnail of an N-byte state A.
 *   state_spacing_bytes and thumb_spacing_bytes are the bytes from one stream's state, or held thumbnail, to the next stream's:
 *   what the other calls name stride_bytes, with its rules ("Strides and pitches" above: any value >= the window's bytes, the
 *   products in 64 bits), and any alignment.
 *   Inputs of stream s: the state at d_states + s*state_spacing_bytes (only read); the HELD THUMBNAIL at d_thumbs +
 *   s*thumb_spacing_bytes, N' bytes, any alignment, read and written -- the frame this stream's low-resolution viewer has
 *   reconstructed; d_tile_mask, NULL for every tile or uint32[nstreams][mask_words] over the FULL-SIZE state's 4096-byte tiles,
 *   the object mi355_cwire_touched_tiles_batch and mi355_refresh_cwire_batch write (bits at or past tiles are ignored);
 *   threshold in 0 .. 255.
 *   A thumbnail pixel is REQUIRED by the wall's rule: its block contains a source pixel p whose bytes [3p, 3p + 3) meet a
 *   selected tile (a pixel that straddles a tile edge belongs to both tiles).  The call processes every required pixel and MAY
 *   process any other byte of the same stream's thumbnail (whole chunks, as the masked compose).  For every processed byte j:
 *   new = thumbnail(state_s)[j], old = thumbs_s[j], df = new - old as integers; if |df| > threshold the entry (j, (uint8)df)
 *   belongs to record s and thumbs_s[j] = new; otherwise nothing happens at j and the difference stays pending, as in the diff's
 *   negative feedback.  threshold == 0 makes the held thumbnail an exact mirror (the relay's setting).
 *   Outputs are those of mi355_refresh_cwire_batch: d_offsets uint32[nstreams + 1], d_frame_pos uint64[nstreams + 1] (always
 *   exact), record s at d_cwire_out + d_frame_pos[s], the canonical encoding of its entries in ascending j (headers written, pad
 *   bytes zero, byte for byte what mi355_cwire_encode_batch writes).  A record with d_frame_pos[s + 1] > capacity_bytes is skipped
 *   whole AND ITS STREAM'S HELD THUMBNAIL IS NOT WRITTEN AT ALL: the viewer did not get the record, so the caller's model of the
 *   viewer does not move; the caller repeats the call with more room and the same mask.  Records behind a skipped one that fit
 *   are written.  mi355_cwire_bytes_max(N', nstreams) always suffices.
 *   Laws:
 *   1. Always: applying output record s to a copy of the held thumbnail as it was before the call gives the held thumbnail as it
 *      is after the call -- any input, any mask, whichever extra bytes were processed.
 *   2. Always: after the call every byte of a required pixel has thumbs[j] == thumbnail(state)[j], or |thumbnail(state)[j] - old|
 *      <= threshold and thumbs[j] == old; any other byte is untouched or satisfies the same.
 *   3. Under the invariant "outside the required pixels |thumbnail(state) - thumbs| <= threshold everywhere" (it holds when this
 *      call has maintained the thumbnails with one threshold and the masks covered every change of the states) the output is
 *      unique: byte for byte the host form's, and byte for byte what mi355_diff_multi_cwire_batch of a core of geometry tw x th
 *      with that threshold writes from the frames thumbnail(state_s) and the states thumbs_s; held thumbnails and frame
 *      positions match too.
 *   4. The chain property, next to the wall's: if thumbs == thumbnail(states) before a tick and threshold == 0, then the tick
 *      (mi355_diff_multi_cwire_batch on a sender, mi355_apply_multi_stream_cwire_batch on a relay),
 *      mi355_cwire_touched_tiles_batch of the same records and this call, with no wait between the three, leave
 *      thumbs == thumbnail(states); a viewer that applies the records holds the same bytes.
 *   5. Key record: a NULL mask with a zeroed held thumbnail and threshold == 0 yields (j, thumbnail[j]) for every nonzero byte,
 *      the refresh record of the thumbnail: a late joiner's first record and the repair after a lost one (the viewer clears its
 *      state, the caller zeroes thumbs_s, one call with a NULL mask follows).
 *   6. k == 1: the thumbnail is the state; with a zeroed held thumbnail, a NULL mask and threshold == 0 the records equal those of
 *      mi355_refresh_cwire_batch(d_peer_digests = NULL) byte for byte.
 *   Refused with MI355_ERR_INVALID before anything is launched or written: a null core; nstreams outside [0, max_batch]; k outside
 *   1 .. 16; threshold outside 0 .. 255; with nstreams > 0 a null pointer other than d_tile_mask, state_spacing_bytes < N,
 *   thumb_spacing_bytes < N'; d_tile_mask, d_offsets or d_cwire_out not 4-byte aligned; d_frame_pos not 8-byte aligned; any two of
 *   these regions overlapping: the states' region, the thumbnails' region [d_thumbs, + (nstreams - 1)*thumb_spacing_bytes + N'),
 *   the mask, the offsets, the frame positions, [d_cwire_out, + capacity_bytes).  nstreams == 0 writes offsets[0] = 0 and
 *   frame_pos[0] = 0 and nothing else.  Bytes of the thumbnails' region outside each stream's N' bytes are never written, the
 *   stride gap included; the states and the core's own state are never written; nothing is allocated.  Asynchronous on the core's
 *   stream, in call order behind a tick, an apply, a clear or a touched-tiles call on the same core, with no synchronisation.
 *   One k and one threshold per call: a ladder (full, 1/2, 1/4) is one call per rung, each rung with its own held thumbnails.
 * mi355_thumb_cwire_host is the definition: plain C++, no core, no HIP call, no alignment demands.  It processes EXACTLY the
 * required pixels of one state; *n, *e and *bytes (the record's entries, escapes and size) are always exact; the record and the
 * thumbnail are written only if the record fits capacity_bytes.  Refused, with outputs untouched: a null state, thumb, n, e or
 * bytes; a null out when capacity_bytes > 0; width or height < 1; 3*width*height >= 2^31; k or threshold out of range.
 *   Kernels: k_thumb_facts and k_thumb_emit around the coalescer's scan and place, the shape of the refresh call.  The grid runs
 *   over the tiles of the THUMBNAIL (4096 consecutive thumbnail bytes: several short rows, or part of a long one), one wave per
 *   tile and stream.  A tile's rows are cut along the wall's chunks; a chunk whose source band meets no selected tile is skipped
 *   before a state byte moves, a selected one is box-averaged with the wall's band sum (16-byte loads where the row's address
 *   allows, 16-bit vertical sums, the horizontal sum through LDS at a 3-entry pitch, the rounding divide by multiply-and-correct).
 *   The emit pass rebuilds the same tile from the same bytes; it is the only pass that writes the held thumbnail (at the emitted
 *   bytes) and the last that reads it, and no workgroup touches another tile's thumbnail bytes.
 * Measured: profiles/multi_thumb.json (tools/bench_multi.py --legs thumb --streams 4,16,64; microseconds per stream, 1080p,
 * k = 2, 4, 8, threshold 0, median of five rounds, spreads up to 10 % at S = 4 and below 5 % above, one run on one board; every
 * pass finds the held thumbnails one tick behind).  The route a caller had before -- touched tiles, the masked
 * mi355_wall_compose_batch into a scratch wall, a synchronise, mi355_diff_multi_cwire_batch on a threshold-0 core of the
 * thumbnail's geometry -- wrote the same records at all 18 points.  Both expectations were MISSED.  Touched tiles plus this call
 * take 30.7 / 34.8 / 59.0 us per stream at S = 4 (k = 2 / 4 / 8, webcam-like tick), 21.2 / 10.4 / 15.7 at S = 16 and
 * 19.8 / 8.53 / 5.71 at S = 64 against 41.5 / 41.7 / 35.7, 17.1 / 15.1 / 13.0 and 11.0 / 8.50 / 7.75 for the route; on the moving
 * block 29.7 / 36.4 / 60.7, 9.88 / 10.2 / 15.8 and 6.63 / 4.33 / 4.37 against 41.2 / 41.3 / 40.9, 15.5 / 14.4 / 13.9 and
 * 8.37 / 7.01 / 6.42: no slower than the route at 12 of 18 points (0.62 to 1.00 times), slower at k = 8 for S = 4 and 16 (1.14
 * to 1.65 times: 24 tiles per stream, the call lasts as long as one tile's single wave) and on the webcam-like tick at k = 2 for
 * S = 16 and 64 (1.24 and 1.80: a record as long as the thumbnail, bounded by the byte-serial emit).  The call alone with the
 * moving block's mask (367 of 1519 tiles) against no mask: cheaper at k = 2 for every S (0.95, 0.68, 0.61 times) and at k = 4 for
 * S = 64 (0.76), not cheaper at k = 4 for S = 4 and 16 and at k = 8 (1.01 to 1.15 times).  DESIGN.md says what bounds both.
 * DESIGN.md section 4, "Records of the thumbnails". */
int mi355_thumb_cwire_host(const uint8_t *state, int width, int height, int k, int threshold,
                           const uint32_t *tile_mask /* or NULL: every tile */, uint8_t *thumb /* N' bytes, in and out */,
                           void *out, size_t capacity_bytes, uint32_t *n, uint32_t *e, size_t *bytes);
int mi355_thumb_cwire_batch(mi355_core *core, const void *d_states, size_t state_spacing_bytes, int nstreams, int k, int threshold,
                            const void *d_tile_mask /* or NULL: every tile */, void *d_thumbs, size_t thumb_spacing_bytes,
                            void *d_offsets, void *d_frame_pos, void *d_cwire_out, size_t capacity_bytes);

/* Integer difference of tests/algorithms_benchmarks.cu:24-30 (kernel1): d[i] = cur[i] - prev[i] on
 * int32 arrays of n elements, no threshold, no pack. */
int mi355_int_diff(mi355_core *core, const void *d_cur, const void *d_prev, void *d_out, size_t n);

/* ---- filters, device resident (all N-byte BGR24 frames; in-place allowed unless noted) --------- */
/* kernels.cu:31-43 / server.cpp:96-101: s = (B+G+R)/3 into the 3 channels. */
int mi355_gray_avg(mi355_core *core, const void *d_in, void *d_out);
/* kernels.cu:67-95 / tests/grayscale-weighted/cpu.cu:40: (uint8)(0.114*B + 0.587*G + 0.299*R). */
int mi355_gray_weighted(mi355_core *core, const void *d_in, void *d_out);
/* kernels.cu:138-241 / server.cpp:103-135: histogram of every 3rd byte, two-max threshold clamped
 * to [50,200] (CPU semantics), binarize.  d_hist (int32[256]) and d_thr (int32[1]) may be NULL. */
int mi355_binarize_chain(mi355_core *core, const void *d_gray, void *d_out, void *d_hist, void *d_thr);
/* kernels.cu:243-270 / tests/heat_map_benchmark/cpu.cu:19-27,54-66. */
int mi355_heat_map(mi355_core *core, const void *d_cur, const void *d_prev, void *d_out);
/* tests/heat_map_red_benchmark/cpu.cu:38-55 (dense red/black map). */
int mi355_red_dense(mi355_core *core, const void *d_cur, const void *d_prev, void *d_out);
/* kernels.cu:273-281: img[x + (2 - x%3)] = 255 for the n indices in d_xs; n is read from d_count
 * (uint32 on the device) when d_count != NULL, else `count` is used. */
int mi355_red_overlap(mi355_core *core, void *d_img, const void *d_xs, const void *d_count,
                      uint32_t count);
/* The same from a packed stream, for a batch: frame t (at d_frames + t*stride_bytes) gets R = 255 for every
 * pixel owning one of its entries xs[offsets[t] .. offsets[t+1]).  clear != 0 zeroes the frames first
 * (NOISE_VISUALIZER 2, kernels.cu:513); clear == 0 paints onto what they hold (NOISE_VISUALIZER 3, :517).
 * clear != 0 builds every frame from its entries in ONE write-only pass and needs them ASCENDING within the
 * frame -- as every diff entry point of this library produces them (the pass finds a slice's entries by
 * binary search; entries out of order would be dropped without an error) -- and nframes <= max_batch.
 * clear == 0 is a plain scatter: any order, any nframes.
 * Either form takes frame counts beyond 65535 (the frame is a grid dimension of its kernels): such a batch is issued
 * as several grids of at most 65535 frames each, with the same result as one. */
int mi355_red_stream_batch(mi355_core *core, const void *d_offsets, const void *d_xs, int nframes,
                           void *d_frames, size_t stride_bytes, int clear);
/* kernels.cu:97-136: 3x3 convolution with the kernel of mi355_set_conv_kernel; not in-place.  fp32, taps in
 * i-major / j-minor order, one multiply then one add per tap; the float result is truncated toward zero and
 * saturated to [0, 255] (any nine floats are accepted: negative taps and sums above 255 clamp). */
int mi355_conv3x3(mi355_core *core, const void *d_in, void *d_out);
/* The K x K form of the same filter as the reference's filter study runs it, K = 1..9, even K included
 * (tests/noise_filter_benchmark/v2.cu:36-80: taps at rows / columns -K/2 .. K-1-K/2, zero outside the image); k =
 * K*K floats in host memory, row-major (v2.cu:116-124 mean, :139-160 Gaussian).  Same arithmetic and conversion as
 * mi355_conv3x3 (for K = 3 the two agree bit for bit); not in-place; not tuned -- the server's path is K = 3. */
int mi355_conv_kxk(mi355_core *core, const void *d_in, void *d_out, const float *k, int K);

/* tests/noise_filter_benchmark/v3.cu:32-90 (the K = 5 median the reference evaluated and left out of its
 * server for speed): per channel the median of the 5x5 neighbourhood, zeros outside the image; not in-place. */
int mi355_median5x5(mi355_core *core, const void *d_in, void *d_out);

/* Batched form of the per-frame filters: nframes frames at d_in + t*stride_bytes (and d_in2 + t*stride_bytes
 * for the two-input filters) -> d_out + t*stride_bytes, one launch per kernel for the whole batch.
 * The *_BINARIZE ops compute one histogram and one two-max threshold per frame; the fused forms read the colour
 * frame ONCE: pass 1 converts it and keeps one gray byte per pixel in a scratch of the core (max_batch * N/3 bytes,
 * allocated at the first such call) beside the histogram, pass 2 binarizes from that scratch (BASELINE config 3).
 * Every nframes in [0, max_batch] is accepted, whatever max_batch mi355_create allowed: up to 65535 frames are one launch
 * per kernel; a longer batch is issued as several grids of at most 65535 frames each (the frame is a grid dimension),
 * every slice with its own frames, histograms and thresholds, and computes what one launch would.  An argument the call
 * refuses (MI355_ERR_INVALID) is refused before anything is written; any other error (MI355_ERR_HIP from an allocation or a
 * launch, MI355_ERR_STATE) may leave the output frames, and the core's histograms and thresholds, partly written. */
#define MI355_OP_GRAY_AVG 1                /* kernels.cu:31-43                         */
#define MI355_OP_GRAY_WEIGHTED 2           /* kernels.cu:67-95                         */
#define MI355_OP_BINARIZE 3                /* gray3 in: kernels.cu:138-241             */
#define MI355_OP_GRAY_AVG_BINARIZE 4       /* colour in: server.cpp:96-135 in one call */
#define MI355_OP_GRAY_WEIGHTED_BINARIZE 5  /* colour in: kernels.cu:493-498 (visualizer 5) */
#define MI355_OP_HEAT_MAP 6                /* d_in = cur, d_in2 = prev: kernels.cu:243-270 */
#define MI355_OP_RED_DENSE 7               /* d_in = cur, d_in2 = prev: test.cu:142-168 */
#define MI355_OP_CONV3X3 8                 /* kernels.cu:97-136, not in place          */
#define MI355_OP_MEDIAN5X5 9               /* noise_filter_benchmark/v3.cu:32-90, not in place */
int mi355_filter_batch(mi355_core *core, int op, const void *d_in, const void *d_in2, void *d_out,
                       size_t stride_bytes, int nframes);

/* ---- the per-frame host entry point: CUDACore::exec_core (kernels.cu:430-525) -------------------
 * frame_data: in = the captured frame (N bytes), out = diff[0..*h_pos)      (kernels.cu:461,522)
 * show_ready: out = the visualisation frame when cfg.visualizer != 0        (kernels.cu:481-518)
 * text      : overlay string (characters of the glyph charset) or NULL      (kernels.cu:466-476)
 * h_pos     : out = number of changed bytes                                 (kernels.cu:507)
 * h_xs      : out = their byte indices, ascending                           (kernels.cu:523)
 * Returns after both device synchronisations of the reference (kernels.cu:508,524). */
int mi355_exec(mi355_core *core, uint8_t *frame_data, uint8_t *show_ready, const char *text,
               uint32_t *h_pos, int32_t *h_xs);

/* ---- the same entry point, pipelined ----------------------------------------------
 * The reference overlaps capture, elaboration and sending with three threads around a ring of six pinned
 * slots (server/src/threads.cpp:59-106,134-147,166-179) but exec_core itself blocks the host twice per
 * frame (kernels.cu:508,524).  Here the overlap moves below the boundary: mi355_pipe_submit enqueues the
 * upload of frame k on a copy stream, its kernels on the core's stream and its results' way back, and
 * returns; while frame k is packed, frame k+1 crosses PCIe.  The changed-byte count never visits the host
 * in between: a device kernel stores exactly count indices/differences, and the count, through the mapped
 * pinned pointers.  mi355_pipe_wait(ticket) blocks until that frame's outputs are in the caller's
 * buffers and returns h_pos.  Frames are processed in submission order (the state carries over).
 *   - every host buffer must be pinned memory of mi355_host_alloc (alloc_arrays, kernels.cu:531-536) and
 *     stay untouched between submit and wait; argument meaning as mi355_exec;
 *   - depth (1..8) frames may be in flight; submitting into a full ring first completes the oldest frame;
 *   - mi355_exec is refused while the pipe is open. */
int mi355_pipe_open(mi355_core *core, int depth);
int mi355_pipe_submit(mi355_core *core, uint8_t *frame_data, uint8_t *show_ready, const char *text,
                      int32_t *h_xs, int64_t *ticket);
int mi355_pipe_wait(mi355_core *core, int64_t ticket, uint32_t *h_pos);
int mi355_pipe_close(mi355_core *core);

/* ---- compact form of the per-frame entry points: the frame's changes as ONE compact record in host memory -----------
 * Each frame gets exactly what mi355_exec / mi355_pipe_submit do to it, in the same order, on the same state: upload, noise
 * filter when configured, text overlay, visualiser into show_ready (the red maps included), diff with negative feedback.
 * The packed entries do not go to h_xs / frame_data: h_record receives the frame's compact record, byte for byte what
 * mi355_cwire_encode_batch writes for those entries (header {n, e} included, pad bytes zero), *h_bytes =
 * mi355_cwire_frame_bytes(n, e) bytes long, ready for one write(); *h_pos = n, *h_escapes = e.
 *   - frame_data is only read (the one difference from mi355_exec); no byte of h_record at or past *h_bytes is written;
 *     nothing but h_record and show_ready is written on the host.
 *   - Refused before anything is launched (MI355_ERR_INVALID, or MI355_ERR_STATE for the open / closed pipe): whatever
 *     mi355_exec refuses; a null h_record, h_pos, h_escapes, h_bytes or ticket; an h_record that is not 4-byte aligned;
 *     record_capacity < mi355_cwire_bytes_max(N, 1) -- a record that did not fit would lose a frame whose state has already
 *     advanced, so the worst case is demanded up front; mi355_exec_cwire while a pipe is open, the submit / wait forms while
 *     none is; pageable buffers handed to mi355_pipe_submit_cwire.
 *   - mi355_exec_cwire takes pinned or pageable buffers, as mi355_exec does.  A pinned h_record is written by a device
 *     kernel through the mapped pointer (the size never visits the host; whole 16-byte stores when h_record is 16-byte
 *     aligned); for a pageable one the size is read back and exactly that many bytes are copied.
 *   - Plain and compact submits may alternate on one open pipe, mi355_exec and mi355_exec_cwire on one core: they share the
 *     state and the ticket counter.  mi355_pipe_wait on a compact ticket is valid and returns n; mi355_pipe_wait_cwire on a
 *     plain ticket is MI355_ERR_STATE and leaves the ticket waitable.  Ring overrun and "already waited" as above.
 *   - The first compact call of a core allocates (a device record buffer of mi355_cwire_bytes_max(N, 1) bytes, counted by
 *     mi355_workspace_bytes, and a few pinned words) and synchronises once, unless
 *     mi355_prepare(core, MI355_PREPARE_EXEC_CWIRE) did.  mi355_pipe_open allocates nothing for it.
 * On the device the frame is packed as for mi355_exec, then encoded (three launches) and exported (one).  Speed of
 * mi355_pipe_submit_cwire against mi355_pipe_submit on the same frames: not yet measured (tools/bench_cwire.py host
 * is the run, and writes profiles/host_cwire.json). */
int mi355_exec_cwire(mi355_core *core, const uint8_t *frame_data, uint8_t *show_ready, const char *text, void *h_record,
                     size_t record_capacity, uint32_t *h_pos, uint32_t *h_escapes, size_t *h_bytes);
int mi355_pipe_submit_cwire(mi355_core *core, const uint8_t *frame_data, uint8_t *show_ready, const char *text, void *h_record,
                            size_t record_capacity, int64_t *ticket);
int mi355_pipe_wait_cwire(mi355_core *core, int64_t ticket, uint32_t *h_pos, uint32_t *h_escapes, size_t *h_bytes);

/* ---- pinned host memory: CUDACore::alloc_arrays (kernels.cu:531-536) ---------------------------- */
int mi355_host_alloc(void **out, size_t bytes);
int mi355_host_free(void *p);

/* ---- device memory for hosts without a HIP binding ---------------------------------------------------
 * The device-resident entry points take device pointers.  A caller that links the HIP runtime (or PyTorch)
 * brings its own; a host language that reaches this library only through the C-ABI (cgo, JNI, ctypes ...)
 * uses these: plain hipMalloc/hipFree on the core's device, and copies ordered on the core's stream
 * (mi355_upload returns once the host buffer may be reused, mi355_download once the bytes are there). */
int mi355_dev_alloc(mi355_core *core, void **out, size_t bytes);
int mi355_dev_free(mi355_core *core, void *d_ptr);
/* The two output arrays of the batch entry points -- d_xs (capacity x int32) and d_diff (capacity x uint8) -- as a PAIR whose
 * placement in memory lets the DENSE expansion run at its fast speed.  When most bytes of a frame change (a scene cut, the
 * synthetic worst cases S0 / P = N), the expansion is bound by its stores to these two arrays, and their two streams either
 * overlap in the memory system (205 us per 32 dense 1080p frames) or do not (265): a property of the pair's physical memory
 * that no address shows, the same for the life of the arrays; about one pair in six of plain allocations is the fast kind
 * (round 6, profiles/README.md).  This call allocates the index array, then draws value arrays (at most 32), runs for each
 * a batch of noise frames (max_batch pairs, P = 0.85 N: ~1 ms) through the core's own kernels into the pair, and keeps the
 * first pair on which the expansion moves its bytes at the fast rate; the others are freed; *draws (may be NULL) = value
 * arrays drawn.  Blocking; the core's state and results are untouched (the probe batches are stateless pairs).  Arrays that
 * hold fewer than 8 frames' worth of entries, and callers of sparse streams (a webcam's: the expansion is then bound
 * elsewhere), need none of this: plain allocations.  Free both with mi355_dev_free. */
int mi355_alloc_outputs(mi355_core *core, size_t capacity, void **d_xs, void **d_diff, int *draws);
int mi355_upload(mi355_core *core, void *d_dst, const void *host_src, size_t bytes);
int mi355_download(mi355_core *core, void *host_dst, const void *d_src, size_t bytes);

/* ---- multi-GPU: several devices of one node, RCCL over xGMI only for the final changed-pixel gather ------------
 * The reference runs on one GPU (server/src/kernels.cu:385); this is the sharding BASELINE.json asks of the path
 * (SURVEY.md section 8e).  The data path has no collective: every member runs an independent stream (E1), its
 * share of round-robin frame pairs (E1, BASELINE config 5) or a row band of one stream (E2; merge with
 * mi355_merge_parts on the root's core) through the single-device entry points, side by side.  The one exchange
 * step is mi355_group_gather.
 *
 * A group is either all in this process -- mi355_group_create makes one core per device and an RCCL communicator
 * over them (a C++ server linked against libmi355compat.a) -- or one member per process: every process creates
 * its core as usual and calls mi355_group_adopt_rank with the same 128-byte id (made once by
 * mi355_group_unique_id and handed around by the launcher, e.g. torch.distributed broadcast).  RCCL is bound at
 * the first group call (dlopen of librccl.so.1); single-GPU users never load it.  The same "one caller thread
 * at a time" rule as for a core applies to a group. */
#define MI355_GROUP_ID_BYTES 128
typedef struct mi355_group mi355_group;
int mi355_group_create(const mi355_config *cfg, int ndev, const int *devices /* NULL: 0..ndev-1 */,
                       mi355_group **out);
int mi355_group_unique_id(void *id128);
int mi355_group_adopt_rank(mi355_core *core, int nranks, int rank, const void *id128, mi355_group **out);
void mi355_group_destroy(mi355_group *group);   /* destroys the cores mi355_group_create made, not adopted ones */
int mi355_group_ranks(const mi355_group *group);           /* members in all processes */
int mi355_group_local_members(const mi355_group *group);   /* members in this process: 0 <= i < this */
mi355_core *mi355_group_core(mi355_group *group, int i);   /* member i's core: mi355_set_state etc. */
int mi355_group_rank_of(const mi355_group *group, int i);  /* member i's rank in the group */
/* mi355_diff_stream_batch / mi355_diff_pairs_batch on every local member, pointer arrays indexed by local member;
 * asynchronous on each member's stream. */
int mi355_group_diff_stream_batch(mi355_group *group, const void *const *d_frames, size_t stride_bytes, int nframes,
                                  void *const *d_offsets, void *const *d_xs, void *const *d_diff, size_t capacity);
int mi355_group_diff_pairs_batch(mi355_group *group, const void *const *d_cur, const void *const *d_prev,
                                 size_t stride_bytes, int nframes, void *const *d_offsets, void *const *d_xs,
                                 void *const *d_diff, size_t capacity);
/* Gather-v of the members' batch outputs to rank `root`: collective over ALL ranks of the group (every process
 * calls it with its local members' arrays).  On the root's device: d_root_offsets[rank][0..nframes] = that
 * rank's own exclusive scan, d_root_xs / d_root_diff = the ranks' entries back to back in rank order (rank r at
 * the sum of the counts before it; root_capacity entries).  member_capacity = the entries every local member's
 * d_xs / d_diff hold (the `capacity` its batch ran with).  h_counts[rank] receives every rank's total in every
 * process (one host synchronisation, kernels.cu:507-508 reads its count back the same way); the transfers
 * themselves are asynchronous on the members' streams.  d_root_* / root_capacity are ignored where the root is
 * not local.
 * Failures that concern the whole exchange are decided collectively, BEFORE anything is sent, and reported on
 * every rank alike (MI355_ERR_INVALID): a member whose batch overflowed its buffers (offsets[nframes] >
 * member_capacity: the entries beyond were dropped, there is nothing to send), a gathered total above the root's
 * capacity, missing root buffers.  No rank is left waiting for another. */
int mi355_group_gather(mi355_group *group, int root, int nframes, const void *const *d_offsets,
                       const void *const *d_xs, const void *const *d_diff, size_t member_capacity,
                       void *d_root_offsets, void *d_root_xs, void *d_root_diff, size_t root_capacity,
                       uint64_t *h_counts);
int mi355_group_synchronize(mi355_group *group);

/* ---- measurement ---------------------------------------------------------------------------------
 * With timing on, every *_batch call brackets its kernels with HIP events on the stream they are
 * launched on.  mi355_get_timing synchronises the stream and returns the sums since the last reset:
 * ms_pack = the diff/threshold/pack kernel alone, ms_total = pack + scan + gather. */
int mi355_set_timing(mi355_core *core, int enabled);
int mi355_get_timing(mi355_core *core, double *ms_pack, double *ms_total, int *launches);
/* The same sums per kernel: pack (k_diff_pack; both launches of a split pipelined batch, from the start of the first to
 * the end of whichever ends later), scan (k_scan_groups), expand (k_expand).  One batch after the other their sum is
 * ms_total; pipelined batches wait between their pack kernel and their index (for the stream hop), so ms_total is larger. */
int mi355_get_kernel_timing(mi355_core *core, double *ms_pack, double *ms_scan, double *ms_expand, int *launches);
int mi355_reset_timing(mi355_core *core);
/* Diagnostics: the shader clock (MHz) the device holds under an integer-VALU load of about `milliseconds` ms
 * (1..2000), measured inside a kernel as d(s_memtime) / d(s_memrealtime) x 100 MHz, median over all waves
 * (csrc/diag.hip).  The diff path is bound by instruction issue, so its frames/s follow this clock; boards differ.
 * Runs on the core's stream and returns after it has finished; not part of any data path. */
int mi355_probe_clock(mi355_core *core, int milliseconds, double *shader_mhz);
/* Diagnostics: GB/s of a plain streaming read of a temporary `megabytes` MB buffer (64..16384; best of three passes):
 * what this board's memory system gives a read-only kernel.  The pack kernel is bound by it; boards differ by ~7 %. */
int mi355_probe_hbm_read(mi355_core *core, size_t megabytes, double *gbps);
/* Diagnostics: GB/s of plain streaming WRITES into a temporary buffer (non-temporal, best of three passes): narrow = 0:
 * 16 bytes per lane (whole lines, the filters' outputs); narrow = 1: what a dense expansion emits, a 4-byte index and a
 * 1-byte value per lane to two arrays.  Boards with the same read rate differ by a quarter in this one. */
int mi355_probe_hbm_write(mi355_core *core, size_t megabytes, int narrow, double *gbps);

#ifdef __cplusplus
}
#endif
#endif /* MI355DIFF_H_ */

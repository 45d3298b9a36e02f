// internal.h -- shared declarations of libmi355diff (not part of the C-ABI).
#ifndef MI355_INTERNAL_H_
#define MI355_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mi355 {

// Geometry of the diff/threshold/pack kernel: one wave64 owns one 1 KiB *tile* of the frame
// (64 lanes x 16 B, a single global_load_dwordx4 per frame) for the whole batch.
constexpr uint32_t kTileBytes = 1024;
constexpr uint32_t kWavesPerBlock = 4;

struct PackArgs {
    const uint8_t *cur;    // frame t at cur + t*stride
    const uint8_t *prev;   // pair mode: prev frame t at prev + t*stride; consecutive frames: frame 0's predecessor; stream mode: unused
    union {
        uint8_t *state;    // stream mode: N bytes, read at start and written back at the end
        uint8_t *states;   // segmented stream mode (seg > 0): stream s's state at states + s*stride, read when its segment
    };                     // begins and written back when it ends
    size_t stride;         // bytes between frames
    uint32_t n;            // bytes per frame
    int32_t nframes;       // T
    int32_t thr;           // threshold
    uint32_t ntiles;       // W = ceil(n / 1024)
    uint32_t tile_begin;   // this launch packs tiles [tile_begin, tile_end): the whole frame, or one part of it when a
    uint32_t tile_end;     // pipelined batch is packed by two staggered launches (core.hip, run_batch)
    uint32_t *codes;       // code log: T/4 chunks x W tiles x 256 codes (one per candidate lane)
    uint4 *rec;            // record log: T chunks x W tiles x 64 records of 16 masked diff bytes (multi-byte lanes)
    uint4 *meta;           // [T][W]: {code position, record position, flagged bytes, candidates | multi-byte lanes << 16}
    uint32_t codes_bytes;  // sizes of the logs (buffer descriptors; all < 2^32)
    uint32_t rec_bytes;
    uint32_t meta_bytes;
    // segmented stream mode (mi355_diff_multi_stream_*): batch index b = s * seg + t is frame t of stream s
    int32_t seg;           // frames per stream (0: not segmented); nframes = streams * seg
};
// (seg fills the struct's tail padding and states shares state's place: the kernel arguments keep their size, and with it the
// existing instantiations of k_diff_pack their code down to the offset of the implicit arguments)
static_assert(sizeof(PackArgs) == 96, "see above");

struct ExpandArgs {
    const uint32_t *codes;
    const uint4 *rec;
    const uint4 *meta;        // [T][W]
    const uint32_t *roff;     // [T][4G] flagged bytes of the frame before each range of 16 tiles (G = ceil(W/64) groups)
    const uint32_t *offsets;  // [T+1]   exclusive scan of the frame totals
    uint32_t ntiles;
    uint32_t codes_bytes;     // sizes of the two logs (the expander's buffer descriptors; both < 2^32)
    uint32_t rec_bytes;
    int32_t *out_xs;
    uint8_t *out_diff;
    uint8_t *wire;            // != nullptr: write the sender's byte stream here instead of out_xs/out_diff
    size_t capacity;          // entries of out_xs/out_diff, or bytes of wire
};

// core.hip, for the other translation units of the library (group.hip)
}  // namespace mi355
struct mi355_core;
namespace mi355 {
int set_error(int code, const char *what);        // sets the calling thread's mi355_last_error text, returns code
hipStream_t core_stream(::mi355_core *c);   // the stream the core currently enqueues on (joins a pipelined batch's side stream first)
int core_device(const ::mi355_core *c);

// diff_pack.hip
// a.seg > 0 (stream mode only): the segmented form, a.states instead of a.state
hipError_t launch_diff_pack(const PackArgs &a, bool pair, bool aligned, bool pair_once /* pair mode: no frame is an operand twice */,
                            uint32_t max_blocks /* 0: one tile per wave */, hipStream_t s,
                            bool feedback = false /* pair mode: prev + t * stride is writable and takes frame t's fed-back state */,
                            bool consecutive = false /* stream mode without feedback: frame t against frame t - 1, frame 0
                                                        against the one frame at a.prev; a.state unused */);
uint32_t expand_groups(uint32_t ntiles);
// A frame total travels as ONE 64-bit word {total: 31 bits (a frame is below 2 GiB), tag of the launch: 33 bits}
// (diff_pack.hip, publish_total).  The tag counts the launches of a core and is never 0 (0 = never written); when it
// would wrap the host clears every total behind a synchronisation (core.hip, next_scan_epoch), so a slot can never
// carry a stale word with the current tag, whatever the number of launches.
constexpr int kTotalBits = 31;
constexpr uint64_t kEpochWrap = 1ull << (64 - kTotalBits);   // tags are 1 .. kEpochWrap - 1
// the tag of the next launch; true: the tags have wrapped, the caller must clear the totals before that launch
inline bool next_scan_epoch(uint64_t &epoch) {
    if (++epoch < kEpochWrap) return false;
    epoch = 1;
    return true;
}
hipError_t launch_scan(const uint4 *meta, uint32_t *roff, uint64_t *totals /* [T] {total, tag} */, uint32_t ntiles,
                       int nframes, uint32_t *offsets, uint32_t *ticket /* zero between launches */,
                       uint64_t epoch /* 1 .. kEpochWrap - 1, different from every tag `totals` still holds */,
                       uint64_t *note /* pinned host word for {batch total, frames << 32}, or nullptr */, hipStream_t s);
hipError_t launch_expand(const ExpandArgs &a, int nframes, hipStream_t s);
// The log straight into compact records (mi355_diff_stream_cwire_batch; diff_pack.hip, "compact-wire expansion").
__host__ __device__ uint32_t cwire_items_per_frame(uint32_t ntiles);   // = items of k_expand: ceil(W / 16)
struct CwireDirectArgs {
    ExpandArgs x;             // the log and the batch's offsets (out_xs / out_diff / wire / capacity unused)
    uint4 *items;             // [T][cwire_items_per_frame(W)] scratch of the core
    uint32_t *esc;            // [T] escapes per frame, scratch of the core
    uint64_t *frame_pos;      // [T+1] the caller's
    uint8_t *cwire;           // the caller's records
    uint64_t capacity;        // bytes of cwire
};
// nframes == 0 or ntiles == 0 (offsets already zero): only frame_pos and the empty records' headers are written
hipError_t launch_expand_cwire(const CwireDirectArgs &a, int nframes, hipStream_t s);

// stream_ops.hip
constexpr int kMaxParts = 64;
struct MergeArgs {
    const uint32_t *part_off;   // [nparts][T+1] device: each part's own exclusive scan
    const int32_t *xs_all;      // parts' entries back to back, part p at part_base[p]
    const uint8_t *diff_all;
    int32_t *out_xs;
    uint8_t *out_diff;
    size_t capacity;
    int32_t nparts, nframes;
    uint32_t part_base[kMaxParts];
    int32_t xs_bias[kMaxParts];
};
hipError_t launch_apply(uint8_t *frame, uint32_t nbytes, const void *xs, const void *diff,
                        const uint32_t *d_offsets, int t, uint32_t host_count, hipStream_t s);
hipError_t launch_apply_all(uint8_t *frame, uint32_t nbytes, const int32_t *xs, const uint8_t *diff,
                            const uint32_t *d_offsets, int nframes, hipStream_t s);
// mi355_apply_multi_*: segment s of a packed stream onto states + s*stride
hipError_t launch_apply_multi(uint8_t *states, size_t stride, uint32_t nbytes, const uint32_t *d_offsets, const int32_t *xs,
                              const uint8_t *diff, int nstreams, hipStream_t s);
constexpr int kApplyMultiWireStreams = 128;   // streams per k_apply_multi_wire launch (their places travel as kernel arguments)
struct ApplyMultiWireArgs {
    int32_t first, count;                       // streams [first, first + count)
    uint64_t pos[kApplyMultiWireStreams];       // byte position of stream first + j's {n, xs, diff} in the wire stream
    uint64_t cum[kApplyMultiWireStreams + 1];   // entries of this launch's streams before j (cum[count]: all of them)
};
hipError_t launch_apply_multi_wire(uint8_t *states, size_t stride, uint32_t nbytes, const uint8_t *wire,
                                   const ApplyMultiWireArgs &h, hipStream_t s);
// mi355_apply_multi_stream_*: launch t of a burst takes segment s*nframes + t of every stream s; ..._show copies the states
// to the output frames s*nframes + t (out + b*out_stride) afterwards
hipError_t launch_apply_multi_strided(uint8_t *states, size_t stride, uint32_t nbytes, const uint32_t *d_offsets, const int32_t *xs,
                                      const uint8_t *diff, int nstreams, int nframes, int t, hipStream_t s);
hipError_t launch_apply_multi_show(const uint8_t *states, size_t stride, uint32_t nbytes, uint8_t *out, size_t out_stride,
                                   int nstreams, int nframes, int t, hipStream_t s);
hipError_t launch_export(const uint32_t *offsets, const int32_t *xs, const uint8_t *diff, int32_t *h_xs,
                         uint8_t *h_diff, uint32_t *h_count, hipStream_t s);
// one compact record (rec[0 .. frame_pos[1]), at most rec_bytes) to the mapped h_record, {n, e, bytes low, bytes high} to h_words
hipError_t launch_export_record(const uint64_t *frame_pos, const uint8_t *rec, uint64_t rec_bytes, uint32_t *h_record,
                                uint32_t *h_words, hipStream_t s);
hipError_t launch_merge(const MergeArgs &a, uint32_t *out_offsets, hipStream_t s);
// compact wire (include/mi355diff.h): the encoder's per-workgroup escape counts live in kCwireSlots words of the core
// (nframes * cwire_blocks_per_frame(nframes) <= kCwireSlots), so one encode takes at most kCwireSlots frames
constexpr int kCwireSlots = 8192;
int cwire_blocks_per_frame(int nframes);
hipError_t launch_cwire_encode(const uint32_t *offsets, const int32_t *xs, const uint8_t *diff, uint64_t entries_capacity,
                               int nframes, uint32_t *cnt /* kCwireSlots words */, uint64_t *frame_pos, uint8_t *out,
                               uint64_t capacity_bytes, hipStream_t s);
constexpr int kCwireDecodeFrames = 64;   // frames per decode launch (their descriptors travel as kernel arguments)
struct CwireFrame {
    uint64_t pos;   // byte position of the record in the compact stream
    uint32_t n, e;  // its header, as the client read it
    uint32_t out;   // entries of the frames before it (its first entry in xs / diff)
    uint32_t pad;
};
struct CwireDecodeArgs {
    const uint8_t *cwire;
    uint32_t *offsets;
    int32_t *xs;
    uint8_t *diff;
    uint64_t capacity;
    int32_t first_frame;
    CwireFrame frame[kCwireDecodeFrames];
};
hipError_t launch_cwire_decode(const CwireDecodeArgs &a, int nframes, hipStream_t s);
// stream_ops.hip -- mi355_apply_cwire_batch: records straight onto the state, tile-major (one wave per kCwaTile bytes)
constexpr uint32_t kCwaChunk = 4096;    // codes per workgroup of the directory kernels
constexpr uint32_t kCwaTile = 4096;     // bytes of the state per workgroup of the apply kernel
constexpr int kCwaTableFrames = 128;    // frame headers per k_cwa_table launch (kernel arguments)
struct CwaFrame {
    uint64_t pos;         // byte position of the record in the compact stream
    uint32_t n, e;        // its header, as the client read it
    uint32_t cbase, nc;   // its chunks: [cbase, cbase + nc) of the slice, nc = cwa_chunks(n)
};
struct CwaArgs {
    const uint8_t *cwire;
    CwaFrame *ftab;       // [T] scratch of the core
    uint4 *chunk;         // [T * cwa_chunks(N)] scratch: {escape codes, first escape rank, running index, frame}
    uint4 *dir;           // [T][ntiles] scratch: {first entry, its escape rank, running index before it, 0}
    uint8_t *state;
    uint8_t *out;         // frame t at out + t*stride, or nullptr
    size_t stride;
    uint32_t n;           // bytes per frame
    uint32_t ntiles;      // cwa_tiles(n)
};
struct CwaTableArgs {
    int32_t first;
    CwaFrame frame[kCwaTableFrames];
};
uint32_t cwa_chunks(uint32_t n);        // chunks of a frame of n entries (1 for n = 0)
uint32_t cwa_tiles(uint32_t nbytes);
uint32_t cwa_mask_words(uint32_t nbytes);   // 32-bit words of a stream's tile mask
// frames[i].cbase / nc filled by the caller; nframes <= the scratch's T
hipError_t launch_cwire_apply(const CwaArgs &a, const CwaFrame *frames, int nframes, hipStream_t s);
// mi355_apply_multi_cwire_batch: record s onto a.state + s*a.stride (the caller's states; a.out unused), tiles x streams
hipError_t launch_cwire_apply_multi(const CwaArgs &a, const CwaFrame *records, int nstreams, hipStream_t s);
// mi355_apply_multi_stream_cwire_batch: records s*nframes + t, t in order, onto a.state + s*a.stride; a.out != nullptr: the frame
// after record b = s*nframes + t also to a.out + b*out_stride (a.stride is the states')
hipError_t launch_cwire_apply_multi_stream(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, size_t out_stride,
                                           hipStream_t s);
// mi355_cwire_coalesce_(cwire_)batch: records s*nframes + t of each stream summed (mod 256) into ONE record / segment per stream;
// a.state / a.out / a.stride unused, a.chunk doubles as the per-(stream, tile) facts once the directory is made
struct CwcOut {
    uint32_t *offsets;     // [nstreams + 1]
    uint64_t *frame_pos;   // [nstreams + 1], compact form
    uint8_t *cwire;        // compact form: the records
    int32_t *xs;           // arrays form
    uint8_t *diff;
    uint64_t capacity;     // bytes of cwire, or entries of xs / diff
};
hipError_t launch_cwire_coalesce(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, const CwcOut &o, bool cwire,
                                 hipStream_t s);
// mi355_cwire_budget_cwire_batch: record s thinned to budget[s] entries (host array) at the least threshold >= thr0 that allows it,
// a.state + s*a.stride reverted at the dropped entries; hist: kCwbWords words per stream (scratch of the core), thresholds and o:
// the caller's.  a.out unused, a.chunk doubles as the facts as above.
constexpr int kCwbInitStreams = 128;                         // budgets per k_cwb_init launch (kernel arguments)
constexpr uint32_t kCwbBudget = 256, kCwbThr = 257, kCwbWords = 258;   // a stream's row: 256 bins of |cur - prev|, its budget, its T
struct CwbInitArgs {
    int32_t first;
    uint32_t thr0;
    uint32_t budget[kCwbInitStreams];
};
hipError_t launch_cwire_budget(const CwaArgs &a, const CwaFrame *records, int nstreams, const uint32_t *budget, uint32_t thr0,
                               uint32_t *hist, uint32_t *thresholds, const CwcOut &o, hipStream_t s);
// mi355_cwire_despeckle_cwire_batch: record s without the entries of the pixels that have fewer than need[s] (host array, 0 .. 8; 0:
// not filtered) changed pixels among the 8 around them, a.state + s*a.stride reverted at the dropped entries.  words: the budget
// call's per-stream rows, of which a stream's first is written (need); changed / keep: dsp_words(a.n) words per stream each (scratch
// of the core, one bit per pixel); dropped (uint32 per stream) and o: the caller's.  a.out unused, a.chunk doubles as the facts.
constexpr int kDspInitStreams = 128;   // needs per k_dsp_init launch (kernel arguments)
struct DspInitArgs {
    int32_t first;
    uint32_t need[kDspInitStreams];
};
uint32_t dsp_words(uint32_t nbytes);   // 32-bit words of a stream's pixel bitmap
hipError_t launch_cwire_despeckle(const CwaArgs &a, const CwaFrame *records, int nstreams, const uint32_t *need, uint32_t width,
                                  uint32_t *words, uint32_t *changed, uint32_t *keep, uint32_t *dropped, const CwcOut &o,
                                  hipStream_t s);
// mi355_(cwire_)activity_batch: per stream, a grid of counts of the entries of its nframes records (batch index s*nframes + t)
// per cell of cell_w x cell_h pixels, and 8 summary words (include/mi355diff.h).  Divisors travel with floor(2^32 / d).
struct ActDiv {
    uint32_t d, m;   // m = floor(2^32 / d), 2^32 - 1 for d = 1
};
ActDiv act_divisor(uint32_t d);   // d >= 1
struct ActGeom {
    uint32_t n;                      // bytes per frame
    ActDiv width, cell_w, cell_h;    // pixels
    uint32_t grid_w, cells;          // cells per row of the grid, cells per stream
    uint32_t min_count;
};
// compact form: a.state / a.out / a.stride unused; accumulate == false: grids and summaries are cleared first
hipError_t launch_cwire_activity(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, const ActGeom &g, bool accumulate,
                                 uint32_t *cells, uint32_t *summary, hipStream_t s);
hipError_t launch_activity(const uint32_t *d_offsets, const int32_t *xs, int nstreams, int nframes, const ActGeom &g, bool accumulate,
                           uint32_t *cells, uint32_t *summary, hipStream_t s);
// mi355_cwire_crop_(cwire_)batch: the coalescer with every stream's sums cut to its rectangle rects[s] = {x0, y0, w, h} (host array,
// checked by the caller against width x height) and, unless keep_index, re-indexed to the rectangle's w x h frame.  words: the budget
// call's per-stream rows (kCwbWords words apart), of which a stream's first six are written (its rows, its column bytes and the
// map's two constants: CropWords); a and o as for the coalescer.
constexpr int kCropStreams = 128;   // rectangles per k_crop_facts launch (kernel arguments)
struct CropArgs {
    int32_t first;        // the launch's first stream
    uint32_t row_bytes;   // 3W
    int32_t keep_index;
    int32_t rect[kCropStreams][4];
};
hipError_t launch_cwire_crop(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, const int32_t *rects, uint32_t width,
                             bool keep_index, uint32_t *words, const CwcOut &o, bool cwire, hipStream_t s);
// mi355_cwire_mosaic_(cwire_)batch: the coalesced records of the streams placed on a BGR24 canvas of canvas_bytes = 3 * canvas_w *
// canvas_h bytes, place[s] = {sx, sy, w, h, dx, dy} (host array, checked by the caller against the frame and the canvas), ONE
// segment / record out (o.offsets uint32[2], o.frame_pos uint64[2]).  words: the budget call's per-stream rows, of which a stream's
// first six are written (MosaicWords); a.chunk holds one fact word per CANVAS tile, so cwa_tiles(canvas_bytes) must not exceed the
// scratch (the caller refuses a larger canvas); a as for the coalescer, of the source frames.
constexpr int kMosaicStreams = 128;   // placements per k_mosaic_table launch (kernel arguments)
struct MosaicArgs {
    int32_t first, count;   // the launch's first stream and its streams
    int32_t place[kMosaicStreams][6];
};
hipError_t launch_cwire_mosaic(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, const int32_t *place, uint32_t width,
                               uint32_t canvas_w, uint32_t canvas_bytes, uint32_t *words, const CwcOut &o, bool cwire, hipStream_t s);
// mi355_cwire_check_batch: verdicts[b][0 .. 4) of record b (include/mi355diff.h); a.ftab and a.chunk are the scratch it uses, a.n the
// frame bytes; a.dir / a.state / a.out / a.stride / a.ntiles unused
hipError_t launch_cwire_check(const CwaArgs &a, const CwaFrame *records, int nrecords, uint32_t *verdicts, hipStream_t s);
// Resynchronising a receiver (include/mi355diff.h).  mi355_state_digest_batch: digests[s][tile][0 .. 2) of the n bytes at
// states + s*stride
hipError_t launch_state_digest(const uint8_t *states, size_t stride, uint32_t n, int nstreams, uint32_t *digests, hipStream_t s);
// mi355_refresh_cwire_batch: a.state / a.stride / a.n / a.ntiles the sender's states (only read), a.chunk the per-(stream, tile)
// facts; peer: the receiver's digests or nullptr (every tile); mask: [nstreams][ceil(ntiles / 32)]; o as for the coalescer
hipError_t launch_refresh(const CwaArgs &a, int nstreams, const uint32_t *peer, uint32_t *mask, const CwcOut &o, hipStream_t s);
// mi355_state_clear_tiles_batch: the tiles of states + s*stride whose bit of mask[s] is set -> 0
hipError_t launch_state_clear_tiles(uint8_t *states, size_t stride, uint32_t n, int nstreams, const uint32_t *mask, hipStream_t s);
// A wall of many cameras (include/mi355diff.h).  mi355_wall_compose_batch: the thumbnail of the width x height state at
// states + s*stride, scale place[s][2] (0: not shown), to (place[s][0], place[s][1]) of the wall; mask: the tile mask above or
// nullptr (every tile).  The placements travel as kernel arguments, kWallPlaceStreams streams per launch.
constexpr int kWallPlaceStreams = 128;
struct WallPlaceArgs {
    int32_t first;
    int32_t x[kWallPlaceStreams], y[kWallPlaceStreams], k[kWallPlaceStreams];
};
// Thumbnail pixels per workgroup of k_wall_compose: a row's tw pixels in even chunks of a multiple of 16 pixels (a chunk's
// first source byte, 3*k*u0, keeps its row's 16-byte alignment) whose 3*k*pixels source bytes per row fit the workgroup's 4096
__host__ __device__ inline uint32_t wall_chunk_pixels(uint32_t tw, uint32_t k) {
    const uint32_t most = (4096u / (3u * k)) & ~15u;   // 1360 (k = 1) .. 80 (k = 16)
    const uint32_t nch = (tw + most - 1u) / most;
    return ((tw + nch - 1u) / nch + 15u) & ~15u;       // <= most
}
hipError_t launch_wall_compose(const uint8_t *states, size_t stride, uint32_t width, uint32_t height, int nstreams,
                               const int32_t *place /* host, [nstreams][3] */, const uint32_t *mask, uint8_t *wall, size_t wall_pitch,
                               hipStream_t s);
// mi355_cwire_touched_tiles_batch: behind the directory of the nstreams*nframes records, mask[s] (ceil(a.ntiles / 32) words) = or
// |= the tiles that a record of stream s has an entry in; a.state / a.out / a.stride unused
hipError_t launch_cwire_touched(const CwaArgs &a, const CwaFrame *records, int nstreams, int nframes, bool accumulate, uint32_t *mask,
                                hipStream_t s);
// mi355_thumb_cwire_batch: ONE record per stream of the thumbnail at scale k of the width x height state at a.state + s*a.stride
// (only read) against the held thumbnail at thumbs + s*thumb_stride, which moves where an entry is written.  mask: the states'
// tile mask or nullptr (every tile).  a.n / a.ntiles: the states'; the kernels get a copy with the thumbnail's, and a.chunk holds
// one fact word per (stream, thumbnail tile) -- never more than the states' tiles.  o as for the coalescer, compact form.
struct ThumbArgs {
    uint8_t *thumbs;
    size_t thumb_stride;
    const uint32_t *mask;
    uint32_t mask_words;
    uint32_t width, height, k, tw, th, threshold;
    ActDiv row;       // bytes of a thumbnail row, 3 * tw
    ActDiv area[4];   // pixels of a block: [2 * (the last row) + (the last column)]
};
hipError_t launch_thumb_cwire(const CwaArgs &a, int nstreams, uint32_t width, uint32_t height, uint32_t k, uint32_t threshold,
                              const uint32_t *mask, uint8_t *thumbs, size_t thumb_stride, const CwcOut &o, hipStream_t s);
// mi355_cwire_split_cwire_batch: every record cut into pieces of at most max_bytes bytes (include/mi355diff.h, "the piece rule").
// A block is kCwsBlock entries of one record, kCwsBlock / kCwaChunk chunks of the chunk table; a record of no entries has one
// empty block, as it has one empty chunk.  blk / base: one word each per block of the call (scratch of the core, cws_blocks(N) per
// record of max_batch): blk = {record, block of the record, pieces, bytes}, base = {pieces, bytes} of the blocks before it.
constexpr uint32_t kCwsBlock = 65536;
constexpr int kCwsTableRecords = 128;   // first blocks per k_cws_table launch (kernel arguments)
struct CwsTableArgs {
    int32_t first;
    uint32_t bbase[kCwsTableRecords];
};
struct CwsOut {
    uint32_t *piece_first;   // [nrecords + 1]
    uint64_t *piece_pos;     // [piece_capacity + 1]
    uint64_t piece_capacity;
    uint8_t *cwire;
    uint64_t capacity;       // bytes of cwire
};
uint32_t cws_blocks(uint32_t n);   // blocks of a record of n entries (1 for n = 0)
// a.ftab and a.chunk are the scratch it shares with the other calls; a.dir / a.state / a.out / a.stride / a.ntiles unused
hipError_t launch_cwire_split(const CwaArgs &a, const CwaFrame *records, int nrecords, uint32_t max_bytes, uint4 *blk, ulonglong2 *base,
                              const CwsOut &o, hipStream_t s);
// mi355_cwire_runs_encode_batch: every record into the run form or copied, as the policy says (include/mi355diff.h, "Run-coded
// records").  a.ftab and a.chunk are the scratch it shares with the other calls (chunk = {runs, first run rank, 0, record});
// forms / pos / out: the caller's.  a.dir / a.state / a.out / a.stride / a.ntiles unused.
struct CwrOut {
    uint32_t *forms;     // [nrecords][4] {form, n, e, r}
    uint64_t *pos;       // [nrecords + 1]
    uint8_t *out;
    uint64_t capacity;   // bytes of out
};
hipError_t launch_cwire_runs_encode(const CwaArgs &a, const CwaFrame *records, int nrecords, int policy, const CwrOut &o, hipStream_t s);
// mi355_cwire_runs_decode_batch: the records' places and headers are the host's (h_forms) and travel as kernel arguments,
// kCwrTableRecords per launch.  A record in the run form is kCwrRuns runs per workgroup, one in the compact form kCwaChunk entries.
constexpr uint32_t kCwrRuns = 1024;
constexpr int kCwrTableRecords = 64;
struct CwrRecord {
    uint64_t in_pos, out_pos;   // byte positions on the link and in the compact stream
    uint32_t form, n, e, r;
    uint32_t cbase, nc;         // its workgroups: [cbase, cbase + nc) of the call, nc = cwr_chunks(form, n, r)
};
struct CwrTableArgs {
    int32_t first, last;        // the launch's first record; last != 0: the launch holds the call's last record
    uint64_t total;             // frame_pos[nrecords]
    CwrRecord rec[kCwrTableRecords];
};
struct CwrDecode {
    const uint8_t *in;
    CwrRecord *rtab;       // [T] scratch of the core
    uint2 *chunk;          // [T * cwr_chunks_max(N)] scratch: {record, entries of the record before the workgroup's runs}
    uint64_t *frame_pos;   // [nrecords + 1], the caller's
    uint8_t *out;
    uint64_t capacity;     // bytes of out
};
uint32_t cwr_chunks(uint32_t form, uint32_t n, uint32_t r);   // workgroups of a record (never 0)
uint32_t cwr_chunks_max(uint32_t nbytes);                     // ... of any record of a frame of nbytes bytes
hipError_t launch_cwire_runs_decode(const CwrDecode &d, const CwrRecord *records, int nrecords, uint64_t total, hipStream_t s);
// mi355_cwire_fec_batch: parity blocks over groups of the pieces the split call wrote (include/mi355diff.h, "Parity pieces").
// Everything the kernels read lies on the device; waves: how many waves the parity kernel's grid holds (sized from the device).
struct FecArgs {
    const uint32_t *pieces;       // pieces_bytes bytes
    uint64_t pieces_bytes;
    const uint32_t *piece_first;  // [nrecords + 1]
    const uint64_t *piece_pos;    // [piece_capacity + 1]
    uint64_t piece_capacity;
    int nrecords;
    uint32_t group, nparity, pitch;
    uint32_t *fec_first;          // [nrecords + 1]
    uint32_t *fec_len;            // [group_capacity]
    uint64_t group_capacity;
    uint32_t *out;
    uint64_t capacity;            // bytes of out
};
hipError_t launch_cwire_fec(const FecArgs &a, uint32_t workgroups, hipStream_t s);
// mi355_cwire_fec_repair_batch: the jobs' descriptors travel as kernel arguments, at most kFecRepairJobs jobs and kFecRepairSlots
// slots per launch (a job of 255 members fits one launch).  mode: 0 nothing lost; 1 out0 = Pxy; 2 out0 = c2 * Qxy (P absent);
// 3 two lost: out1 = c2 * (Qxy ^ c1 * Pxy), out0 = Pxy ^ out1.  Offsets are bytes into rx, kFecAbsent: not there.
constexpr int kFecRepairJobs = 8, kFecRepairSlots = 256;
constexpr uint64_t kFecAbsent = ~0ull;
struct FecRepairJob {
    uint64_t p_off, q_off;
    uint32_t slot0, members, fec_len, mode, c1, c2, index;   // slot0: its first slot of the launch; index: the job of the call
};
struct FecRepairArgs {
    FecRepairJob job[kFecRepairJobs];
    uint64_t off[kFecRepairSlots];
    uint32_t len[kFecRepairSlots];
};
// One launch: njobs jobs of h; block k of job j to out + (2j + k)*pitch, verdict[2j + k]
hipError_t launch_cwire_fec_repair(const uint8_t *rx, const FecRepairArgs &h, int njobs, uint8_t *out, size_t pitch, uint32_t *verdict,
                                   hipStream_t s);

// filters.hip -- every per-frame kernel takes a FrameBatch: frame f lives at base + f*stride
struct FrameBatch {
    size_t stride;
    int nframes;
};
hipError_t launch_int_diff(const int32_t *cur, const int32_t *prev, int32_t *out, size_t n,
                           hipStream_t s);
hipError_t init_gray_table();   // the weighted gray's exception table on the current device
hipError_t launch_gray(const uint8_t *in, uint8_t *out, uint32_t npix, bool weighted, FrameBatch fb,
                       hipStream_t s);
hipError_t launch_binarize_chain(const uint8_t *gray, uint8_t *out, uint32_t nbytes, int32_t *hist,
                                 int32_t *thr, FrameBatch fb, hipStream_t s);
hipError_t launch_gray_binarize_fused(const uint8_t *color, uint8_t *out, uint32_t npix, bool weighted,
                                      int32_t *hist, int32_t *thr, FrameBatch fb, hipStream_t s,
                                      uint8_t *gray1 /* scratch: nframes x gray1_stride bytes, or nullptr */,
                                      size_t gray1_stride /* >= npix, a multiple of 16 */);
hipError_t launch_heat_map(const uint8_t *cur, const uint8_t *prev, uint8_t *out, uint32_t npix,
                           const uint8_t *lut, FrameBatch fb, hipStream_t s);
hipError_t launch_red_dense(const uint8_t *cur, const uint8_t *prev, uint8_t *out, uint32_t npix,
                            int thr, FrameBatch fb, hipStream_t s);
hipError_t launch_red_overlap(uint8_t *img, const int32_t *xs, const uint32_t *d_count,
                              uint32_t count, uint32_t nbytes, hipStream_t s);
uint32_t red_bounds_per_frame(uint32_t nbytes);
hipError_t launch_red_stream(uint8_t *out, const uint32_t *offsets, const int32_t *xs, uint32_t nbytes, bool clear,
                             FrameBatch fb, hipStream_t s,
                             uint32_t *bounds_scratch /* nframes x red_bounds_per_frame(nbytes) words, or nullptr */);
hipError_t launch_conv3x3(const uint8_t *in, uint8_t *out, int w, int h, const float *k9, bool k9_symmetric,
                          FrameBatch fb, hipStream_t s);
hipError_t launch_conv_kxk(const uint8_t *in, uint8_t *out, int w, int h, const float *kk /* device, K*K */, int K,
                           FrameBatch fb, hipStream_t s);
hipError_t launch_median5x5(const uint8_t *in, uint8_t *out, int w, int h, int rows_per_band /* 0: chosen here */, FrameBatch fb,
                            hipStream_t s);
hipError_t launch_blit_glyph(uint8_t *frame, const uint8_t *glyph, int glyph_h, int glyph_wbytes,
                             int x_off_bytes, int frame_wbytes, int frame_h, hipStream_t s);

}  // namespace mi355
#endif

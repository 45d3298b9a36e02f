// tools/roundtrip.cpp -- server -> socket bytes -> client, in plain C++ over the C-ABI only.
//
// Compiled with g++ (no HIP header, no HIP runtime call here): what a host written in any language with
// a C FFI does.  A "server" core packs a stream of frames into the byte stream the reference's sender
// thread writes (server/src/threads.cpp:220-233: base frame, then per frame u32 n | i32 xs[n] | u8 diff[n]);
// the bytes go through a pipe to a "client" that parses them exactly as client/opencv.cpp:38-66 does
// (read the base frame, then pos, pos indices, pos differences per frame) and rebuilds the frames on a
// second core.  The program checks that the client's frame equals the server's reconstructed state
// after every batch and that every rebuilt byte is within the threshold of the frame that was sent.
//
// --compact: the same over the compact wire format (include/mi355diff.h): the server packs a batch and encodes it on the
// GPU (mi355_diff_stream_batch, mi355_cwire_encode_batch), the records cross the same pipe, and the client -- with no
// core and no GPU -- rebuilds every frame on the host with mi355_cwire_apply_host; each rebuilt frame is checked against
// the frame that was sent, and the client's frame against the server's state after every batch.
// --compact --direct: the server makes the records in one call (mi355_diff_stream_cwire_batch), without the xs / diff arrays.
// --compact --gpu-client: the client core also uploads the received records and applies them in one call
// (mi355_apply_cwire_batch) into its shown frames; every shown frame must equal the host client's frame after that record,
// and the client core's state the server's state after every batch.
// --compact --multi S: many cameras per GPU, both ends.  A server core runs T ticks of S synthetic cameras through
// mi355_diff_multi_cwire_batch; each tick's records (headers included) cross the pipe; a client core uploads them and applies
// them in one call (mi355_apply_multi_cwire_batch) onto S states of its own.  After every tick the client's states must equal
// the server's, byte for byte, and after the last tick the frames a host client (mi355_cwire_apply_host) rebuilt per camera.
// --compact --multi S --budget BYTES: the sender holds every camera's record of a tick to BYTES bytes (a socket's share of the
// link): the records larger than that are thinned to mi355_cwire_budget_entries(N, BYTES) entries by
// mi355_cwire_budget_cwire_batch, which takes the sender's states back where it drops an entry.  Checked: every record written is
// at most BYTES; each client's frame equals the sender's state after every tick; and once the input has stood still for enough
// ticks every client's frame is within the threshold of the camera's frame at every byte -- what was postponed arrives.
// --compact --multi S --burst K: the sender buffers K ticks per camera (a recorder, a camera that catches up) and makes their
// S * K records in ONE call, mi355_diff_multi_stream_cwire_batch: camera s's K records are one contiguous slice, one write()
// per socket.  The receiver stages record (s, t) of every s back to back for tick t and applies the ticks with the same
// mi355_apply_multi_cwire_batch; after every burst the states at both ends must be equal.
// --compact --multi S --burst K --burst-client: the receiver uploads every camera's slice as it came off its socket, stream-major
// and not re-staged, and applies the whole burst with ONE mi355_apply_multi_stream_cwire_batch into output frames.  After every
// burst the states at both ends must be equal, and every output frame the frame a host client (mi355_cwire_apply_host) rebuilt
// for that camera and tick.
// --compact --multi S --burst K --coalesce: a relay between the two ends that forwards at 1/K of the rate (a slow link, a
// time-lapse recorder, a video wall).  It holds no frame: it uploads every camera's slice as it came off its socket, makes
// ONE record per camera of the burst with mi355_cwire_coalesce_cwire_batch, and forwards those S records; the receiver applies
// them with one mi355_apply_multi_cwire_batch.  After every burst each camera's state at the receiver must equal the frame of
// a host client (mi355_cwire_apply_host) that applied all K original records, and the sender's state.  The line also says how
// many bytes the relay received and how many it forwarded.
// --compact --multi S --activity CELL [--burst K --burst-client]: after every tick (or burst) the receiver also asks where its
// cameras move: mi355_cwire_activity_batch on the records it is about to apply, square cells of CELL pixels -> a grid of changed
// bytes per cell and eight summary words per camera.  Checked against a plain C++ count over records decoded here; the box and the
// active cells of every camera's last tick (or burst) are printed.
// --compact --multi S --check [--burst K --burst-client]: the receiver trusts nothing it has not checked: before it applies a tick
// (or burst) it asks mi355_cwire_check_batch for a verdict per record and requires every record well-formed and canonical (word
// 0 == 0), the verdicts equal to mi355_cwire_check_host's on the received bytes, and word 3 of every record equal to 1 + the
// last byte index that the apply then changes.  Once per run it also checks a damaged copy of the first non-empty record -- one
// code byte set to 255 -- and requires MI355_CWIRE_BAD_CODES.
// --compact --multi S --resync K [--burst B]: a receiver that lost a record finds its way back.  At tick K the receiver drops one
// camera's record (it applies an empty record in its place), so that camera's frame is wrong from then on.  After tick K + 1 it
// digests its states (mi355_state_digest_batch, checked against mi355_state_digest_host) and sends the digests up; the sender
// answers behind its latest tick -- with --burst B the end of the burst it has already made -- with a tile mask and one refresh
// record per camera (mi355_refresh_cwire_batch); the receiver applies the ticks that were in flight, clears the masked tiles
// (mi355_state_clear_tiles_batch) and applies the refresh records like any others.  Checked: the dropped camera's frame differs
// from the sender's at every tick between the loss and the refresh, and every other frame of every tick -- all of them from the
// refresh on -- equals the sender's; the dropped camera has mask bits and, unless ticks were in flight, only that camera (the
// others get the 8-byte record); a host client that
// clears the tiles itself and calls mi355_cwire_apply_host ends at the same frames.
// --compact --multi S --wall K [--burst B --burst-client | --resync R [--burst B]]: the receiver is a wall that shows its cameras.  It
// keeps ONE wall frame of ceil(sqrt(S)) columns of thumbnails at scale K, composed fully once (mi355_wall_compose_batch without
// a mask).  After every tick's apply -- with --burst B --burst-client after every burst's -- it asks which tiles the records it just
// applied land in (mi355_cwire_touched_tiles_batch) and repaints the wall there (mi355_wall_compose_batch with that mask), the
// three calls with no wait in between.  With --resync R the refresh's own mask goes through the same masked compose behind the
// clear and the apply.  After every tick or burst, and after the refresh, the wall must equal a plain C++ box average of the
// receiver's states, and the wall's bytes outside the thumbnails the pattern they started as.
// --compact --per-frame: the per-frame server, one host frame per call and no device pointer in sight.  The sender feeds
// host frames through mi355_pipe_submit_cwire, four in flight, and writes each frame's record to the pipe with ONE write()
// from the pinned buffer it arrived in; the receiver -- a thread with no core -- reads header and body, applies the record
// with mi355_cwire_apply_host and compares its frame, frame by frame, with that of a host client of the plain path
// (mi355_exec on a second core: frame[xs[i]] += diff[i], client/opencv.cpp:64-66).
//
//   tools/roundtrip [--width W] [--height H] [--frames T] [--batch B]
//                   [--compact [--direct] [--gpu-client] [--per-frame] [--multi S [--budget BYTES | --burst K [--burst-client | --coalesce]] [--activity CELL] [--check] | --resync K [--burst B]] [--wall K]]
//   exit status 0 = all checks passed
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <csignal>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../include/mi355diff.h"

#define OK(call)                                                                              \
    do {                                                                                      \
        if ((call) != MI355_OK) {                                                             \
            fprintf(stderr, "%s failed: %s\n", #call, mi355_last_error());                    \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

// a frame sequence with sub-threshold noise everywhere and a block that moves
static void make_frame(std::vector<uint8_t> &f, const std::vector<uint8_t> &base, int w, int h, int t) {
    for (size_t i = 0; i < f.size(); i++) f[i] = (uint8_t)(base[i] + (rnd() >> 24) % 9);
    const int bw = w / 4 + 1, bh = h / 4 + 1, x0 = (t * 3) % (w - bw + 1), y0 = h / 3;
    for (int y = y0; y < y0 + bh && y < h; y++)
        for (int x = x0; x < x0 + bw; x++)
            for (int c = 0; c < 3; c++) f[((size_t)y * w + x) * 3 + c] = (uint8_t)(200 + 10 * c);
}

static bool read_all(int fd, void *p, size_t n) {   // the client's read loops, opencv.cpp:40-62
    uint8_t *b = (uint8_t *)p;
    while (n) {
        const ssize_t k = read(fd, b, n);
        if (k <= 0) return false;
        b += k;
        n -= (size_t)k;
    }
    return true;
}

// "send" n bytes and "receive" them: written in pieces that fit the pipe buffer, read back in between
static bool through_pipe(int wfd, int rfd, const uint8_t *src, uint8_t *dst, size_t n) {
    for (size_t at = 0; at < n;) {
        const size_t piece = n - at < 32768 ? n - at : 32768;
        if (write(wfd, src + at, piece) != (ssize_t)piece) return false;
        if (!read_all(rfd, dst + at, piece)) return false;
        at += piece;
    }
    return true;
}

// --activity CELL (see the head of the file): the receiver's motion grids of the records in rx, against a count made here
struct ActivityCheck {
    mi355_core *core = nullptr;
    int w = 0, h = 0, cell = 0, S = 0, gw = 0, gh = 0, calls = 0;
    size_t cells = 0;
    void *d_cells = nullptr, *d_summary = nullptr;
    std::vector<uint32_t> got_cells, got_sum, want_cells, want_sum;

    int open(mi355_core *c, int w_, int h_, int cell_, int S_) {
        core = c; w = w_; h = h_; cell = cell_; S = S_;
        cells = mi355_activity_cells(w, h, cell, cell, &gw, &gh);
        if (!cells) { fprintf(stderr, "--activity CELL needs CELL >= 1\n"); return 2; }
        OK(mi355_dev_alloc(core, &d_cells, sizeof(uint32_t) * cells * S));
        OK(mi355_dev_alloc(core, &d_summary, sizeof(uint32_t) * 8 * S));
        got_cells.resize(cells * S); want_cells.resize(cells * S);
        got_sum.resize((size_t)8 * S); want_sum.resize((size_t)8 * S);
        return 0;
    }
    // the nb records of each of the S cameras: back to back in rx (and uploaded to d_rx), headers counts / escapes
    int run(const void *d_rx, const uint8_t *rx, const uint32_t *counts, const uint32_t *escapes, int nb, int t) {
        if (!cell) return 0;
        OK(mi355_cwire_activity_batch(core, d_rx, counts, escapes, S, nb, cell, cell, 1, 0, d_cells, d_summary));
        OK(mi355_download(core, got_cells.data(), d_cells, sizeof(uint32_t) * got_cells.size()));
        OK(mi355_download(core, got_sum.data(), d_summary, sizeof(uint32_t) * got_sum.size()));
        calls++;
        const uint64_t n = (uint64_t)3 * w * h;
        std::fill(want_cells.begin(), want_cells.end(), 0u);
        size_t p = 0;
        for (int s = 0; s < S; s++) {
            uint32_t *grid = &want_cells[cells * s], *sum = &want_sum[(size_t)8 * s];
            uint32_t total = 0, x0 = UINT32_MAX, y0 = UINT32_MAX, x1 = 0, y1 = 0;
            for (int k = 0; k < nb; k++) {
                const uint32_t cnt = counts[s * nb + k], esc = escapes[s * nb + k];
                const uint8_t *code = rx + p + 8, *escb = code + ((cnt + 3u) & ~3u);
                uint64_t x = 0;   // running index + 1
                for (uint32_t i = 0, r = 0; i < cnt; i++) {
                    uint32_t g = code[i];
                    if (g == 255) memcpy(&g, escb + 4 * (size_t)r++, 4);
                    x += (uint64_t)g + 1;
                    if (x > n) continue;
                    const uint32_t px = (uint32_t)(((x - 1) / 3) % w), py = (uint32_t)(((x - 1) / 3) / w);
                    grid[(size_t)(py / cell) * gw + px / cell]++;
                    total++;
                    if (px < x0) x0 = px;
                    if (py < y0) y0 = py;
                    if (px > x1) x1 = px;
                    if (py > y1) y1 = py;
                }
                p += mi355_cwire_frame_bytes(cnt, esc);
            }
            uint32_t active = 0, peak = 0, at = 0;
            for (size_t i = 0; i < cells; i++) {
                if (grid[i] >= 1) active++;
                if (grid[i] > peak) { peak = grid[i]; at = (uint32_t)i; }
            }
            const uint32_t want[8] = {total, x0, y0, x1, y1, active, peak, at};
            memcpy(sum, want, sizeof want);
        }
        if (got_cells != want_cells) { fprintf(stderr, "tick %d: motion grids != the count over the decoded records\n", t); return 1; }
        if (got_sum != want_sum) { fprintf(stderr, "tick %d: motion summaries != the count over the decoded records\n", t); return 1; }
        return 0;
    }
    // ", "activity": {...}" for the result line: box and active cells of every camera's last tick (or burst)
    std::string json() const {
        if (!cell) return "";
        std::string o = ", \"activity\": {\"cell\": " + std::to_string(cell) + ", \"grid\": [" + std::to_string(gw) + ", " + std::to_string(gh) +
                        "], \"checked_calls\": " + std::to_string(calls) + ", \"cameras\": [";
        for (int s = 0; s < S; s++) {
            const uint32_t *m = &got_sum[(size_t)8 * s];
            o += std::string(s ? ", " : "") + "{\"entries\": " + std::to_string(m[0]) + ", \"box\": ";
            if (m[0]) o += "[" + std::to_string(m[1]) + ", " + std::to_string(m[2]) + ", " + std::to_string(m[3]) + ", " + std::to_string(m[4]) + "]";
            else o += "null";
            o += ", \"active_cells\": " + std::to_string(m[5]) + "}";
        }
        return o + "]}";
    }
    int close() {
        if (!cell) return 0;
        OK(mi355_dev_free(core, d_cells));
        OK(mi355_dev_free(core, d_summary));
        return 0;
    }
};

// --check (see the head of the file): the verdicts of the records in rx before they are applied, and what the apply then changed
struct RecordCheck {
    mi355_core *core = nullptr;
    bool on = false, damaged_done = false;
    size_t n = 0;
    int records = 0;
    void *d_verdicts = nullptr, *d_damaged = nullptr;
    std::vector<uint32_t> got, want;

    int open(mi355_core *c, size_t n_, int most) {
        core = c; n = n_; on = true;
        OK(mi355_dev_alloc(core, &d_verdicts, sizeof(uint32_t) * 4 * most));
        OK(mi355_dev_alloc(core, &d_damaged, mi355_cwire_bytes_max(n, 1)));
        got.resize((size_t)4 * most); want.resize((size_t)4 * most);
        return 0;
    }
    // the nrec records back to back in rx (cb bytes, uploaded to d_rx), headers counts / escapes
    int run(const void *d_rx, const uint8_t *rx, size_t cb, const uint32_t *counts, const uint32_t *escapes, int nrec, int t) {
        if (!on) return 0;
        OK(mi355_cwire_check_batch(core, d_rx, counts, escapes, nrec, d_verdicts));
        OK(mi355_download(core, got.data(), d_verdicts, sizeof(uint32_t) * 4 * nrec));
        OK(mi355_cwire_check_host(n, rx, cb, counts, escapes, nrec, want.data()));
        if (memcmp(got.data(), want.data(), sizeof(uint32_t) * 4 * nrec) != 0) { fprintf(stderr, "tick %d: device verdicts != host verdicts\n", t); return 1; }
        size_t p = 0;
        for (int r = 0; r < nrec; r++) {
            if (got[(size_t)4 * r] != 0) { fprintf(stderr, "tick %d: record %d: verdict flags %u\n", t, r, got[(size_t)4 * r]); return 1; }
            const size_t size = mi355_cwire_frame_bytes(counts[r], escapes[r]);
            if (!damaged_done && counts[r] > 0) {   // a copy of this record with its first plain code turned into an escape code
                std::vector<uint8_t> copy(rx + p, rx + p + size);
                uint32_t k = 0;
                while (k < counts[r] && copy[8 + k] == 255) k++;
                if (k < counts[r]) {
                    copy[8 + k] = 255;
                    uint32_t v[4] = {0, 0, 0, 0};
                    OK(mi355_upload(core, d_damaged, copy.data(), size));
                    OK(mi355_cwire_check_batch(core, d_damaged, counts + r, escapes + r, 1, d_verdicts));
                    OK(mi355_download(core, v, d_verdicts, sizeof v));
                    if (!(v[0] & MI355_CWIRE_BAD_CODES) || v[1] != escapes[r] + 1) {
                        fprintf(stderr, "tick %d: the damaged copy of record %d got verdict {%u, %u, %u, %u}\n", t, r, v[0], v[1], v[2], v[3]);
                        return 1;
                    }
                    damaged_done = true;
                }
            }
            p += size;
        }
        records += nrec;
        return 0;
    }
    // after the apply: record r (of the last run) turned frame `before` into `after`
    int applied(int r, const uint8_t *before, const uint8_t *after, int t) const {
        if (!on) return 0;
        size_t last = n;
        while (last > 0 && before[last - 1] == after[last - 1]) last--;
        if (got[(size_t)4 * r + 3] != last) {
            fprintf(stderr, "tick %d: record %d: verdict word 3 is %u, the last byte applied is %zu - 1\n", t, r, got[(size_t)4 * r + 3], last);
            return 1;
        }
        return 0;
    }
    std::string json() const {
        if (!on) return "";
        return ", \"check\": {\"records\": " + std::to_string(records) + ", \"damaged_copy\": " + (damaged_done ? "\"bad_codes\"" : "null") + "}";
    }
    int close() {
        if (!on) return 0;
        if (!damaged_done) { fprintf(stderr, "--check: no record had an entry to damage\n"); return 1; }
        OK(mi355_dev_free(core, d_verdicts));
        OK(mi355_dev_free(core, d_damaged));
        return 0;
    }
};

// --wall K (see the head of the file): the receiver's wall of thumbnails, kept current where records land, against a box average
// made here
struct WallCheck {
    mi355_core *core = nullptr;
    int w = 0, h = 0, k = 0, S = 0, tw = 0, th = 0, cols = 0, wall_w = 0, wall_h = 0, composes = 0, compared = 0;
    size_t pitch = 0, mask_bytes = 0;
    void *d_wall = nullptr, *d_mask = nullptr;
    std::vector<int32_t> place;
    std::vector<uint8_t> got, want;
    enum : uint8_t { kPattern = 0x5C };     // what the wall holds outside the thumbnails (and in its pitch gap), from start to end

    int open(mi355_core *c, int w_, int h_, int k_, int S_) {
        if (!mi355_wall_thumb_size(w_, h_, k_, &tw, &th)) { fprintf(stderr, "--wall K needs 1 <= K <= 16\n"); return 2; }
        core = c; w = w_; h = h_; k = k_; S = S_;
        while (cols * cols < S) cols++;
        const int rows = (S + cols - 1) / cols;
        wall_w = cols * (tw + 1) + 1;   // a pixel of the pattern around every thumbnail
        wall_h = rows * (th + 1) + 1;
        pitch = (size_t)3 * wall_w + 5;
        place.resize((size_t)3 * S);
        for (int s = 0; s < S; s++) {
            place[3 * s] = 1 + (s % cols) * (tw + 1);
            place[3 * s + 1] = 1 + (s / cols) * (th + 1);
            place[3 * s + 2] = k;
        }
        mask_bytes = 4 * (size_t)S * ((mi355_state_tiles((size_t)3 * w * h) + 31) / 32);
        got.assign(pitch * wall_h, kPattern);
        want = got;
        OK(mi355_dev_alloc(core, &d_wall, got.size()));
        OK(mi355_dev_alloc(core, &d_mask, mask_bytes));
        OK(mi355_upload(core, d_wall, got.data(), got.size()));
        return 0;
    }
    // every thumbnail from the states as they are
    int full(const void *d_states) {
        if (!k) return 0;
        OK(mi355_wall_compose_batch(core, d_states, (size_t)3 * w * h, S, place.data(), nullptr, d_wall, wall_w, wall_h, pitch));
        composes++;
        return 0;
    }
    // behind the apply of the nb records of each camera at d_rx (headers counts / escapes): their tiles, repainted
    int update(const void *d_rx, const uint32_t *counts, const uint32_t *escapes, int nb, const void *d_states) {
        if (!k) return 0;
        OK(mi355_cwire_touched_tiles_batch(core, d_rx, counts, escapes, S, nb, 0, d_mask));
        return masked(d_mask, d_states);
    }
    int masked(const void *d_tile_mask, const void *d_states) {
        if (!k) return 0;
        OK(mi355_wall_compose_batch(core, d_states, (size_t)3 * w * h, S, place.data(), d_tile_mask, d_wall, wall_w, wall_h, pitch));
        composes++;
        return 0;
    }
    // the wall against the box average of `states` (the receiver's, S frames back to back)
    int compare(const uint8_t *states, int t) {
        if (!k) return 0;
        OK(mi355_download(core, got.data(), d_wall, got.size()));
        for (int s = 0; s < S; s++) {
            const uint8_t *st = states + (size_t)s * 3 * w * h;
            for (int v = 0; v < th; v++)
                for (int u = 0; u < tw; u++) {
                    const int x0 = u * k, x1 = std::min(w, x0 + k), y0 = v * k, y1 = std::min(h, y0 + k);
                    const uint32_t a = (uint32_t)((x1 - x0) * (y1 - y0));
                    uint32_t sum[3] = {0, 0, 0};
                    for (int y = y0; y < y1; y++)
                        for (int x = x0; x < x1; x++)
                            for (int c = 0; c < 3; c++) sum[c] += st[3 * ((size_t)y * w + x) + c];
                    uint8_t *o = &want[(size_t)(place[3 * s + 1] + v) * pitch + 3 * (size_t)(place[3 * s] + u)];
                    for (int c = 0; c < 3; c++) o[c] = (uint8_t)((sum[c] + a / 2) / a);
                }
        }
        if (got != want) { fprintf(stderr, "tick %d: the wall != the box average of the receiver's states\n", t); return 1; }
        compared++;
        return 0;
    }
    std::string json() const {
        if (!k) return "";
        return ", \"wall\": {\"scale\": " + std::to_string(k) + ", \"size\": [" + std::to_string(wall_w) + ", " + std::to_string(wall_h) +
               "], \"thumb\": [" + std::to_string(tw) + ", " + std::to_string(th) + "], \"composes\": " + std::to_string(composes) +
               ", \"walls_equal\": " + std::to_string(compared) + "}";
    }
    int close() {
        if (!k) return 0;
        if (!compared) { fprintf(stderr, "--wall: no wall was compared\n"); return 1; }
        OK(mi355_dev_free(core, d_wall));
        OK(mi355_dev_free(core, d_mask));
        return 0;
    }
};

// --compact --multi S (see the head of the file)
static int run_multi(int w, int h, int T, int S, int activity, bool check, int wall_k) {
    const size_t n = (size_t)3 * w * h;
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = S; cfg.device = -1;
    mi355_core *server = nullptr, *client = nullptr;
    OK(mi355_create(&cfg, &server));
    OK(mi355_create(&cfg, &client));
    const size_t cw_cap = mi355_cwire_bytes_max(n, S);
    void *d_frames = nullptr, *d_sstates = nullptr, *d_off = nullptr, *d_pos = nullptr, *d_cw = nullptr;   // server
    void *d_rx = nullptr, *d_cstates = nullptr;                                                              // client
    OK(mi355_dev_alloc(server, &d_frames, (size_t)S * n));
    OK(mi355_dev_alloc(server, &d_sstates, (size_t)S * n));
    OK(mi355_dev_alloc(server, &d_off, sizeof(uint32_t) * (S + 1)));
    OK(mi355_dev_alloc(server, &d_pos, sizeof(uint64_t) * (S + 1)));
    OK(mi355_dev_alloc(server, &d_cw, cw_cap));
    OK(mi355_dev_alloc(client, &d_rx, cw_cap));
    OK(mi355_dev_alloc(client, &d_cstates, (size_t)S * n));
    ActivityCheck act;
    if (activity)
        if (int rc = act.open(client, w, h, activity, S)) return rc;
    RecordCheck chk;
    if (check)
        if (int rc = chk.open(client, n, S)) return rc;
    WallCheck wall;
    if (wall_k)
        if (int rc = wall.open(client, w, h, wall_k, S)) return rc;
    int fds[2];
    if (pipe(fds) != 0) return 1;
    // every camera's base frame: the server's states, and through the pipe the client's (opencv.cpp:38-46 per camera)
    std::vector<uint8_t> bases((size_t)S * n), host_frames((size_t)S * n), frames((size_t)S * n), s_states((size_t)S * n),
        c_states((size_t)S * n), cw_host(cw_cap), rx(cw_cap);
    for (int s = 0; s < S; s++)
        for (size_t i = 0; i < n; i++) bases[(size_t)s * n + i] = (uint8_t)(40 + (i * 7 + (size_t)s * 31) % 150);
    OK(mi355_upload(server, d_sstates, bases.data(), bases.size()));
    if (!through_pipe(fds[1], fds[0], bases.data(), host_frames.data(), bases.size())) return 1;
    OK(mi355_upload(client, d_cstates, host_frames.data(), host_frames.size()));
    if (int rc = wall.full(d_cstates)) return rc;
    std::vector<uint8_t> base(n), frame(n), before(check ? host_frames : std::vector<uint8_t>());   // (before: the states a tick finds)
    std::vector<uint32_t> off(S + 1), counts(S), escapes(S);
    std::vector<uint64_t> pos(S + 1);
    size_t sent_bytes = 0, changed = 0;
    int max_err = 0;
    for (int t = 0; t < T; t++) {
        for (int s = 0; s < S; s++) {   // camera s: its own base, its block a few steps ahead of its neighbour's
            memcpy(base.data(), &bases[(size_t)s * n], n);
            make_frame(frame, base, w, h, t + 5 * s);
            memcpy(&frames[(size_t)s * n], frame.data(), n);
        }
        // ---- server: one tick -> S records
        OK(mi355_upload(server, d_frames, frames.data(), frames.size()));
        OK(mi355_diff_multi_cwire_batch(server, d_frames, d_sstates, n, S, d_off, d_pos, d_cw, cw_cap));
        OK(mi355_download(server, off.data(), d_off, sizeof(uint32_t) * (S + 1)));
        OK(mi355_download(server, pos.data(), d_pos, sizeof(uint64_t) * (S + 1)));
        if (pos[S] > cw_cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
        const size_t cb = (size_t)pos[S];
        OK(mi355_download(server, cw_host.data(), d_cw, cb));
        changed += off[S];
        // ---- the sockets (one pipe here: the receiver stages the cameras' records back to back)
        if (!through_pipe(fds[1], fds[0], cw_host.data(), rx.data(), cb)) return 1;
        sent_bytes += cb;
        // ---- client: the headers as read from the stream, one upload, one call
        size_t p = 0;
        for (int s = 0; s < S; s++) {
            if (p + 8 > cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
            memcpy(&counts[s], rx.data() + p, 4);
            memcpy(&escapes[s], rx.data() + p + 4, 4);
            size_t used = 0;   // ... and the host client of camera s beside it
            OK(mi355_cwire_apply_host(&host_frames[(size_t)s * n], n, rx.data() + p, cb - p, 1, &used));
            if (used != mi355_cwire_frame_bytes(counts[s], escapes[s])) { fprintf(stderr, "stream framing broken\n"); return 1; }
            p += used;
        }
        if (p != cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
        OK(mi355_upload(client, d_rx, rx.data(), cb));
        if (int rc = act.run(d_rx, rx.data(), counts.data(), escapes.data(), 1, t)) return rc;
        if (int rc = chk.run(d_rx, rx.data(), cb, counts.data(), escapes.data(), S, t)) return rc;
        OK(mi355_apply_multi_cwire_batch(client, d_rx, counts.data(), escapes.data(), S, d_cstates, n));
        if (int rc = wall.update(d_rx, counts.data(), escapes.data(), 1, d_cstates)) return rc;
        // ---- checks
        OK(mi355_download(client, c_states.data(), d_cstates, c_states.size()));
        if (int rc = wall.compare(c_states.data(), t)) return rc;
        for (int s = 0; s < S && check; s++)
            if (int rc = chk.applied(s, &before[(size_t)s * n], &c_states[(size_t)s * n], t)) return rc;
        if (check) before = c_states;
        OK(mi355_download(server, s_states.data(), d_sstates, s_states.size()));
        if (memcmp(s_states.data(), c_states.data(), s_states.size()) != 0) {
            fprintf(stderr, "tick %d: client states != server states\n", t);
            return 1;
        }
        for (size_t i = 0; i < c_states.size(); i++) {
            const int e = abs((int)c_states[i] - (int)frames[i]);
            if (e > max_err) max_err = e;
        }
    }
    if (memcmp(host_frames.data(), c_states.data(), c_states.size()) != 0) { fprintf(stderr, "client states != host client frames\n"); return 1; }
    if (max_err > cfg.threshold) { fprintf(stderr, "rebuilt frame off by %d > threshold\n", max_err); return 1; }
    void *srv[] = {d_frames, d_sstates, d_off, d_pos, d_cw};
    for (void *q : srv) OK(mi355_dev_free(server, q));
    OK(mi355_dev_free(client, d_rx));
    OK(mi355_dev_free(client, d_cstates));
    if (int rc = act.close()) return rc;
    if (int rc = chk.close()) return rc;
    if (int rc = wall.close()) return rc;
    mi355_destroy(server);
    mi355_destroy(client);
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"width\": %d, \"height\": %d, \"ticks\": %d, "
           "\"changed_bytes\": %zu, \"wire_bytes\": %zu, \"reference_wire_bytes\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d%s%s%s}\n",
           S, w, h, T, changed, sent_bytes, mi355_wire_bytes(T * S, changed), (size_t)T * S * n, max_err, act.json().c_str(),
           chk.json().c_str(), wall.json().c_str());
    return 0;
}

// --compact --multi S --budget BYTES (see the head of the file)
static int run_multi_budget(int w, int h, int T, int S, long bytes) {
    const size_t n = (size_t)3 * w * h;
    const size_t most = bytes >= 0 ? mi355_cwire_budget_entries(n, (size_t)bytes) : 0;
    if (most == 0) { fprintf(stderr, "--budget %ld holds no entry of a %dx%d frame\n", bytes, w, h); return 2; }
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = S; cfg.device = -1;
    mi355_core *server = nullptr, *client = nullptr;
    OK(mi355_create(&cfg, &server));
    OK(mi355_create(&cfg, &client));
    const size_t cw_cap = mi355_cwire_bytes_max(n, S);
    void *d_frames = nullptr, *d_sstates = nullptr, *d_off = nullptr, *d_pos = nullptr, *d_cw = nullptr;   // server
    void *d_thr = nullptr, *d_ooff = nullptr, *d_opos = nullptr, *d_out = nullptr;
    void *d_rx = nullptr, *d_cstates = nullptr;                                                              // client
    OK(mi355_dev_alloc(server, &d_frames, (size_t)S * n));
    OK(mi355_dev_alloc(server, &d_sstates, (size_t)S * n));
    OK(mi355_dev_alloc(server, &d_off, sizeof(uint32_t) * (S + 1)));
    OK(mi355_dev_alloc(server, &d_pos, sizeof(uint64_t) * (S + 1)));
    OK(mi355_dev_alloc(server, &d_cw, cw_cap));
    OK(mi355_dev_alloc(server, &d_thr, sizeof(uint32_t) * S));
    OK(mi355_dev_alloc(server, &d_ooff, sizeof(uint32_t) * (S + 1)));
    OK(mi355_dev_alloc(server, &d_opos, sizeof(uint64_t) * (S + 1)));
    OK(mi355_dev_alloc(server, &d_out, cw_cap));
    OK(mi355_dev_alloc(client, &d_rx, cw_cap));
    OK(mi355_dev_alloc(client, &d_cstates, (size_t)S * n));
    int fds[2];
    if (pipe(fds) != 0) return 1;
    std::vector<uint8_t> bases((size_t)S * n), frames((size_t)S * n), s_states((size_t)S * n), c_states((size_t)S * n), cw_host(cw_cap),
        rx(cw_cap);
    for (int s = 0; s < S; s++)
        for (size_t i = 0; i < n; i++) bases[(size_t)s * n + i] = (uint8_t)(40 + (i * 7 + (size_t)s * 31) % 150);
    OK(mi355_upload(server, d_sstates, bases.data(), bases.size()));
    if (!through_pipe(fds[1], fds[0], bases.data(), c_states.data(), bases.size())) return 1;
    OK(mi355_upload(client, d_cstates, c_states.data(), c_states.size()));
    std::vector<uint8_t> base(n), frame(n);
    std::vector<uint32_t> counts(S), escapes(S), budget(S), thr(S);
    std::vector<uint64_t> pos(S + 1);
    size_t sent_bytes = 0, largest = 0;
    int thinned = 0, max_thr = cfg.threshold, max_err = 0, still = 0;
    // T ticks of moving input, then the last frames again and again until nothing is held back any more: what a budget
    // postponed must arrive.  A tick sends up to `most` of a camera's pending entries, so N / most still ticks suffice -- unless
    // more than `most` of them share one magnitude (then no threshold separates them; the synthetic input has no such group).
    const int still_limit = (int)(2 * ((n + most - 1) / most)) + 2;
    for (int t = 0;; t++) {
        if (t < T) {
            for (int s = 0; s < S; s++) {   // camera s: its own base, its block a few steps ahead of its neighbour's
                memcpy(base.data(), &bases[(size_t)s * n], n);
                make_frame(frame, base, w, h, t + 5 * s);
                memcpy(&frames[(size_t)s * n], frame.data(), n);
            }
            OK(mi355_upload(server, d_frames, frames.data(), frames.size()));
        }
        // ---- server: one tick -> S records, their headers, the records above the budget thinned
        OK(mi355_diff_multi_cwire_batch(server, d_frames, d_sstates, n, S, d_off, d_pos, d_cw, cw_cap));
        OK(mi355_download(server, pos.data(), d_pos, sizeof(uint64_t) * (S + 1)));
        if (pos[S] > cw_cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
        bool over = false;
        for (int s = 0; s < S; s++) {
            uint32_t hdr[2];
            OK(mi355_download(server, hdr, (const uint8_t *)d_cw + pos[s], sizeof hdr));
            counts[s] = hdr[0];
            escapes[s] = hdr[1];
            budget[s] = pos[s + 1] - pos[s] > (uint64_t)bytes ? (uint32_t)most : UINT32_MAX;
            if (budget[s] != UINT32_MAX) { over = true; thinned++; }
        }
        OK(mi355_cwire_budget_cwire_batch(server, d_cw, counts.data(), escapes.data(), d_sstates, n, S, budget.data(), d_thr, d_ooff,
                                          d_opos, d_out, cw_cap));
        OK(mi355_download(server, pos.data(), d_opos, sizeof(uint64_t) * (S + 1)));
        OK(mi355_download(server, thr.data(), d_thr, sizeof(uint32_t) * S));
        if (pos[S] > cw_cap) { fprintf(stderr, "thinned stream larger than its bound\n"); return 1; }
        for (int s = 0; s < S; s++) {   // check 1: every record that is written fits the socket's budget
            const size_t rb = (size_t)(pos[s + 1] - pos[s]);
            if (rb > (size_t)bytes) { fprintf(stderr, "tick %d: camera %d's record has %zu bytes > %ld\n", t, s, rb, bytes); return 1; }
            if (rb > largest) largest = rb;
            if ((int)thr[s] > max_thr) max_thr = (int)thr[s];
            if ((budget[s] == UINT32_MAX) != ((int)thr[s] == cfg.threshold)) { fprintf(stderr, "tick %d: camera %d: threshold %u\n", t, s, thr[s]); return 1; }
        }
        const size_t cb = (size_t)pos[S];
        OK(mi355_download(server, cw_host.data(), d_out, cb));
        if (!through_pipe(fds[1], fds[0], cw_host.data(), rx.data(), cb)) return 1;
        sent_bytes += cb;
        // ---- client: the headers as read from the stream, one upload, one call
        size_t p = 0;
        for (int s = 0; s < S; s++) {
            if (p + 8 > cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
            memcpy(&counts[s], rx.data() + p, 4);
            memcpy(&escapes[s], rx.data() + p + 4, 4);
            p += mi355_cwire_frame_bytes(counts[s], escapes[s]);
        }
        if (p != cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
        OK(mi355_upload(client, d_rx, rx.data(), cb));
        OK(mi355_apply_multi_cwire_batch(client, d_rx, counts.data(), escapes.data(), S, d_cstates, n));
        // ---- check 2: each client's frame equals the sender's state after every tick
        OK(mi355_download(client, c_states.data(), d_cstates, c_states.size()));
        OK(mi355_download(server, s_states.data(), d_sstates, s_states.size()));
        if (memcmp(s_states.data(), c_states.data(), s_states.size()) != 0) {
            fprintf(stderr, "tick %d: client states != server states\n", t);
            return 1;
        }
        if (t + 1 < T) continue;
        // ---- check 3, once the input stands still: every client's frame within the threshold of the camera's, at every byte
        max_err = 0;
        for (size_t i = 0; i < c_states.size(); i++) {
            const int e = abs((int)c_states[i] - (int)frames[i]);
            if (e > max_err) max_err = e;
        }
        if (t >= T && !over && max_err <= cfg.threshold) break;
        if (t >= T) still++;
        if (still > still_limit) { fprintf(stderr, "held still for %d ticks and still off by %d > threshold\n", still, max_err); return 1; }
    }
    void *srv[] = {d_frames, d_sstates, d_off, d_pos, d_cw, d_thr, d_ooff, d_opos, d_out};
    for (void *q : srv) OK(mi355_dev_free(server, q));
    OK(mi355_dev_free(client, d_rx));
    OK(mi355_dev_free(client, d_cstates));
    mi355_destroy(server);
    mi355_destroy(client);
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"budget_bytes\": %ld, \"budget_entries\": %zu, \"width\": %d, "
           "\"height\": %d, \"ticks\": %d, \"still_ticks\": %d, \"thinned_records\": %d, \"largest_record_bytes\": %zu, "
           "\"largest_threshold\": %d, \"records_within_budget\": true, \"states_equal_every_tick\": true, "
           "\"max_abs_error_when_still\": %d, \"wire_bytes\": %zu}\n",
           S, bytes, most, w, h, T, still + 1, thinned, largest, max_thr, max_err, sent_bytes);
    return 0;
}

// --compact --multi S --burst K (see the head of the file)
static int run_multi_burst(int w, int h, int T, int S, int K) {
    const size_t n = (size_t)3 * w * h;
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = S * K; cfg.device = -1;
    mi355_core *server = nullptr, *client = nullptr;
    OK(mi355_create(&cfg, &server));
    cfg.max_batch = S;
    OK(mi355_create(&cfg, &client));
    const int B = S * K;
    const size_t cw_cap = mi355_cwire_bytes_max(n, B), tick_cap = mi355_cwire_bytes_max(n, S);
    void *d_frames = nullptr, *d_sstates = nullptr, *d_off = nullptr, *d_pos = nullptr, *d_cw = nullptr;   // server
    void *d_rx = nullptr, *d_cstates = nullptr;                                                              // client
    OK(mi355_dev_alloc(server, &d_frames, (size_t)B * n));
    OK(mi355_dev_alloc(server, &d_sstates, (size_t)S * n));
    OK(mi355_dev_alloc(server, &d_off, sizeof(uint32_t) * (B + 1)));
    OK(mi355_dev_alloc(server, &d_pos, sizeof(uint64_t) * (B + 1)));
    OK(mi355_dev_alloc(server, &d_cw, cw_cap));
    OK(mi355_dev_alloc(client, &d_rx, tick_cap));
    OK(mi355_dev_alloc(client, &d_cstates, (size_t)S * n));
    int fds[2];
    if (pipe(fds) != 0) return 1;
    std::vector<uint8_t> bases((size_t)S * n), host_frames((size_t)S * n), frames((size_t)B * n), s_states((size_t)S * n),
        c_states((size_t)S * n), cw_host(cw_cap), rx(cw_cap), stage(tick_cap);
    for (int s = 0; s < S; s++)
        for (size_t i = 0; i < n; i++) bases[(size_t)s * n + i] = (uint8_t)(40 + (i * 7 + (size_t)s * 31) % 150);
    OK(mi355_upload(server, d_sstates, bases.data(), bases.size()));
    if (!through_pipe(fds[1], fds[0], bases.data(), host_frames.data(), bases.size())) return 1;
    OK(mi355_upload(client, d_cstates, host_frames.data(), host_frames.size()));
    std::vector<uint8_t> base(n), frame(n);
    std::vector<uint32_t> off(B + 1), counts(S), escapes(S);
    std::vector<uint64_t> pos(B + 1);
    std::vector<size_t> at(B), len(B);   // where record (s, t) lies in the received bytes, as the receiver found it
    size_t sent_bytes = 0, changed = 0;
    int max_err = 0, calls = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K, nrec = S * nb;
        for (int s = 0; s < S; s++) {   // camera s's nb frames, one behind the other
            memcpy(base.data(), &bases[(size_t)s * n], n);
            for (int k = 0; k < nb; k++) {
                make_frame(frame, base, w, h, t0 + k + 5 * s);
                memcpy(&frames[((size_t)s * nb + k) * n], frame.data(), n);
            }
        }
        // ---- server: nb ticks of S cameras -> S * nb records in one call
        OK(mi355_upload(server, d_frames, frames.data(), (size_t)nrec * n));
        OK(mi355_diff_multi_stream_cwire_batch(server, d_frames, d_sstates, n, S, nb, d_off, d_pos, d_cw, cw_cap));
        calls++;
        OK(mi355_download(server, off.data(), d_off, sizeof(uint32_t) * (nrec + 1)));
        OK(mi355_download(server, pos.data(), d_pos, sizeof(uint64_t) * (nrec + 1)));
        if (pos[nrec] > cw_cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
        const size_t cb = (size_t)pos[nrec];
        OK(mi355_download(server, cw_host.data(), d_cw, cb));
        changed += off[nrec];
        // ---- the sockets: camera s's slice [pos[s * nb], pos[(s + 1) * nb]) is one write
        for (int s = 0; s < S; s++) {
            const size_t a = (size_t)pos[(size_t)s * nb], b = (size_t)pos[(size_t)(s + 1) * nb];
            if (!through_pipe(fds[1], fds[0], cw_host.data() + a, rx.data() + a, b - a)) return 1;
        }
        sent_bytes += cb;
        // ---- receiver: the records of every socket, found from their headers
        size_t p = 0;
        for (int r = 0; r < nrec; r++) {
            if (p + 8 > cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
            uint32_t c, e;
            memcpy(&c, rx.data() + p, 4);
            memcpy(&e, rx.data() + p + 4, 4);
            at[r] = p;
            len[r] = mi355_cwire_frame_bytes(c, e);
            p += len[r];
        }
        if (p != cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
        // ---- client: tick k = record (s, k) of every s back to back, one upload, one call
        for (int k = 0; k < nb; k++) {
            size_t q = 0;
            for (int s = 0; s < S; s++) {
                const int r = s * nb + k;
                memcpy(stage.data() + q, rx.data() + at[r], len[r]);
                memcpy(&counts[s], stage.data() + q, 4);
                memcpy(&escapes[s], stage.data() + q + 4, 4);
                size_t used = 0;   // ... and the host client of camera s beside it
                OK(mi355_cwire_apply_host(&host_frames[(size_t)s * n], n, stage.data() + q, len[r], 1, &used));
                if (used != len[r]) { fprintf(stderr, "stream framing broken\n"); return 1; }
                q += len[r];
            }
            OK(mi355_upload(client, d_rx, stage.data(), q));
            OK(mi355_apply_multi_cwire_batch(client, d_rx, counts.data(), escapes.data(), S, d_cstates, n));
            OK(mi355_download(client, c_states.data(), d_cstates, c_states.size()));
            if (memcmp(host_frames.data(), c_states.data(), c_states.size()) != 0) {
                fprintf(stderr, "tick %d: client states != host client frames\n", t0 + k);
                return 1;
            }
            for (int s = 0; s < S; s++)
                for (size_t i = 0; i < n; i++) {
                    const int e = abs((int)c_states[(size_t)s * n + i] - (int)frames[((size_t)s * nb + k) * n + i]);
                    if (e > max_err) max_err = e;
                }
        }
        // ---- the states at both ends
        OK(mi355_download(server, s_states.data(), d_sstates, s_states.size()));
        if (memcmp(s_states.data(), c_states.data(), s_states.size()) != 0) {
            fprintf(stderr, "burst at tick %d: client states != server states\n", t0);
            return 1;
        }
    }
    if (max_err > cfg.threshold) { fprintf(stderr, "rebuilt frame off by %d > threshold\n", max_err); return 1; }
    void *srv[] = {d_frames, d_sstates, d_off, d_pos, d_cw};
    for (void *q : srv) OK(mi355_dev_free(server, q));
    OK(mi355_dev_free(client, d_rx));
    OK(mi355_dev_free(client, d_cstates));
    mi355_destroy(server);
    mi355_destroy(client);
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"sender_calls\": %d, \"width\": %d, \"height\": %d, "
           "\"ticks\": %d, \"changed_bytes\": %zu, \"wire_bytes\": %zu, \"reference_wire_bytes\": %zu, \"raw_bytes\": %zu, "
           "\"max_abs_error\": %d}\n",
           S, K, calls, w, h, T, changed, sent_bytes, mi355_wire_bytes(T * S, changed), (size_t)T * S * n, max_err);
    return 0;
}

// --compact --multi S --burst K --burst-client (see the head of the file)
static int run_multi_burst_client(int w, int h, int T, int S, int K, int activity, bool check, int wall_k) {
    const size_t n = (size_t)3 * w * h;
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = S * K; cfg.device = -1;
    mi355_core *server = nullptr, *client = nullptr;
    OK(mi355_create(&cfg, &server));
    OK(mi355_create(&cfg, &client));
    const int B = S * K;
    const size_t cw_cap = mi355_cwire_bytes_max(n, B);
    void *d_frames = nullptr, *d_sstates = nullptr, *d_off = nullptr, *d_pos = nullptr, *d_cw = nullptr;   // server
    void *d_rx = nullptr, *d_cstates = nullptr, *d_shown = nullptr;                                         // client
    OK(mi355_dev_alloc(server, &d_frames, (size_t)B * n));
    OK(mi355_dev_alloc(server, &d_sstates, (size_t)S * n));
    OK(mi355_dev_alloc(server, &d_off, sizeof(uint32_t) * (B + 1)));
    OK(mi355_dev_alloc(server, &d_pos, sizeof(uint64_t) * (B + 1)));
    OK(mi355_dev_alloc(server, &d_cw, cw_cap));
    OK(mi355_dev_alloc(client, &d_rx, cw_cap));
    OK(mi355_dev_alloc(client, &d_cstates, (size_t)S * n));
    OK(mi355_dev_alloc(client, &d_shown, (size_t)B * n));
    ActivityCheck act;
    if (activity)
        if (int rc = act.open(client, w, h, activity, S)) return rc;
    RecordCheck chk;
    if (check)
        if (int rc = chk.open(client, n, B)) return rc;
    WallCheck wall;
    if (wall_k)
        if (int rc = wall.open(client, w, h, wall_k, S)) return rc;
    int fds[2];
    if (pipe(fds) != 0) return 1;
    std::vector<uint8_t> bases((size_t)S * n), host_frames((size_t)S * n), frames((size_t)B * n), s_states((size_t)S * n),
        c_states((size_t)S * n), shown((size_t)B * n), host_shown((size_t)B * n), cw_host(cw_cap), rx(cw_cap);
    for (int s = 0; s < S; s++)
        for (size_t i = 0; i < n; i++) bases[(size_t)s * n + i] = (uint8_t)(40 + (i * 7 + (size_t)s * 31) % 150);
    OK(mi355_upload(server, d_sstates, bases.data(), bases.size()));
    if (!through_pipe(fds[1], fds[0], bases.data(), host_frames.data(), bases.size())) return 1;
    OK(mi355_upload(client, d_cstates, host_frames.data(), host_frames.size()));
    if (int rc = wall.full(d_cstates)) return rc;
    std::vector<uint8_t> base(n), frame(n), before(check ? host_frames : std::vector<uint8_t>());   // (before: the states a burst finds)
    std::vector<uint32_t> off(B + 1), counts(B), escapes(B);
    std::vector<uint64_t> pos(B + 1);
    size_t sent_bytes = 0, changed = 0;
    int max_err = 0, calls = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K, nrec = S * nb;
        for (int s = 0; s < S; s++) {   // camera s's nb frames, one behind the other
            memcpy(base.data(), &bases[(size_t)s * n], n);
            for (int k = 0; k < nb; k++) {
                make_frame(frame, base, w, h, t0 + k + 5 * s);
                memcpy(&frames[((size_t)s * nb + k) * n], frame.data(), n);
            }
        }
        // ---- server: nb ticks of S cameras -> S * nb records in one call
        OK(mi355_upload(server, d_frames, frames.data(), (size_t)nrec * n));
        OK(mi355_diff_multi_stream_cwire_batch(server, d_frames, d_sstates, n, S, nb, d_off, d_pos, d_cw, cw_cap));
        calls++;
        OK(mi355_download(server, off.data(), d_off, sizeof(uint32_t) * (nrec + 1)));
        OK(mi355_download(server, pos.data(), d_pos, sizeof(uint64_t) * (nrec + 1)));
        if (pos[nrec] > cw_cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
        const size_t cb = (size_t)pos[nrec];
        OK(mi355_download(server, cw_host.data(), d_cw, cb));
        changed += off[nrec];
        // ---- the sockets: camera s's slice is one write; the receiver reads its nb records (header, then the rest) behind
        // the slice of camera s - 1 and uploads the slice as it came, stream-major, nothing re-staged
        size_t p = 0;
        for (int s = 0; s < S; s++) {
            const size_t a = (size_t)pos[(size_t)s * nb], b = (size_t)pos[(size_t)(s + 1) * nb];
            if (a != p) { fprintf(stderr, "stream framing broken\n"); return 1; }
            if (!through_pipe(fds[1], fds[0], cw_host.data() + a, rx.data() + a, b - a)) return 1;
            for (int k = 0; k < nb; k++) {
                const int r = s * nb + k;
                if (p + 8 > b) { fprintf(stderr, "stream framing broken\n"); return 1; }
                memcpy(&counts[r], rx.data() + p, 4);
                memcpy(&escapes[r], rx.data() + p + 4, 4);
                size_t used = 0;   // the host client of camera s beside it: the frame it shows after tick k
                OK(mi355_cwire_apply_host(&host_frames[(size_t)s * n], n, rx.data() + p, b - p, 1, &used));
                if (used != mi355_cwire_frame_bytes(counts[r], escapes[r])) { fprintf(stderr, "stream framing broken\n"); return 1; }
                memcpy(&host_shown[(size_t)r * n], &host_frames[(size_t)s * n], n);
                p += used;
            }
            if (p != b) { fprintf(stderr, "stream framing broken\n"); return 1; }
            if (b > a) OK(mi355_upload(client, (uint8_t *)d_rx + a, rx.data() + a, b - a));
        }
        sent_bytes += cb;
        if (int rc = act.run(d_rx, rx.data(), counts.data(), escapes.data(), nb, t0)) return rc;
        if (int rc = chk.run(d_rx, rx.data(), cb, counts.data(), escapes.data(), nrec, t0)) return rc;
        // ---- client: the whole burst in one call, every frame in between into d_shown
        OK(mi355_apply_multi_stream_cwire_batch(client, d_rx, counts.data(), escapes.data(), S, nb, d_cstates, n, d_shown, n));
        if (int rc = wall.update(d_rx, counts.data(), escapes.data(), nb, d_cstates)) return rc;
        OK(mi355_download(client, c_states.data(), d_cstates, c_states.size()));
        if (int rc = wall.compare(c_states.data(), t0 + nb - 1)) return rc;
        OK(mi355_download(client, shown.data(), d_shown, (size_t)nrec * n));
        for (int r = 0; r < nrec && check; r++)   // record (s, k) turned the frame after record (s, k - 1) into its own
            if (int rc = chk.applied(r, r % nb ? &shown[(size_t)(r - 1) * n] : &before[(size_t)(r / nb) * n], &shown[(size_t)r * n], t0)) return rc;
        if (check) before = c_states;
        OK(mi355_download(server, s_states.data(), d_sstates, s_states.size()));
        if (memcmp(s_states.data(), c_states.data(), s_states.size()) != 0) {
            fprintf(stderr, "burst at tick %d: client states != server states\n", t0);
            return 1;
        }
        for (int r = 0; r < nrec; r++)
            if (memcmp(&shown[(size_t)r * n], &host_shown[(size_t)r * n], n) != 0) {
                fprintf(stderr, "burst at tick %d: camera %d, tick %d: GPU client frame != host client frame\n", t0, r / nb, t0 + r % nb);
                return 1;
            }
        for (size_t i = 0; i < (size_t)nrec * n; i++) {
            const int e = abs((int)shown[i] - (int)frames[i]);
            if (e > max_err) max_err = e;
        }
    }
    if (max_err > cfg.threshold) { fprintf(stderr, "rebuilt frame off by %d > threshold\n", max_err); return 1; }
    void *srv[] = {d_frames, d_sstates, d_off, d_pos, d_cw};
    for (void *q : srv) OK(mi355_dev_free(server, q));
    void *cli[] = {d_rx, d_cstates, d_shown};
    for (void *q : cli) OK(mi355_dev_free(client, q));
    if (int rc = act.close()) return rc;
    if (int rc = chk.close()) return rc;
    if (int rc = wall.close()) return rc;
    mi355_destroy(server);
    mi355_destroy(client);
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"burst_client\": true, \"sender_calls\": %d, "
           "\"receiver_calls\": %d, \"width\": %d, \"height\": %d, \"ticks\": %d, \"changed_bytes\": %zu, \"wire_bytes\": %zu, "
           "\"reference_wire_bytes\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d%s%s%s}\n",
           S, K, calls, calls, w, h, T, changed, sent_bytes, mi355_wire_bytes(T * S, changed), (size_t)T * S * n, max_err,
           act.json().c_str(), chk.json().c_str(), wall.json().c_str());
    return 0;
}

// --compact --multi S --burst K --coalesce (see the head of the file)
static int run_multi_burst_coalesce(int w, int h, int T, int S, int K) {
    const size_t n = (size_t)3 * w * h;
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = S * K; cfg.device = -1;
    mi355_core *server = nullptr, *relay = nullptr, *client = nullptr;
    OK(mi355_create(&cfg, &server));
    OK(mi355_create(&cfg, &relay));
    cfg.max_batch = S;
    OK(mi355_create(&cfg, &client));
    const int B = S * K;
    const size_t cw_cap = mi355_cwire_bytes_max(n, B), one_cap = mi355_cwire_bytes_max(n, S);
    void *d_frames = nullptr, *d_sstates = nullptr, *d_off = nullptr, *d_pos = nullptr, *d_cw = nullptr;   // server
    void *d_in = nullptr, *d_roff = nullptr, *d_rpos = nullptr, *d_fwd = nullptr;                           // relay
    void *d_rx = nullptr, *d_cstates = nullptr;                                                              // client
    OK(mi355_dev_alloc(server, &d_frames, (size_t)B * n));
    OK(mi355_dev_alloc(server, &d_sstates, (size_t)S * n));
    OK(mi355_dev_alloc(server, &d_off, sizeof(uint32_t) * (B + 1)));
    OK(mi355_dev_alloc(server, &d_pos, sizeof(uint64_t) * (B + 1)));
    OK(mi355_dev_alloc(server, &d_cw, cw_cap));
    OK(mi355_dev_alloc(relay, &d_in, cw_cap));
    OK(mi355_dev_alloc(relay, &d_roff, sizeof(uint32_t) * (S + 1)));
    OK(mi355_dev_alloc(relay, &d_rpos, sizeof(uint64_t) * (S + 1)));
    OK(mi355_dev_alloc(relay, &d_fwd, one_cap));
    OK(mi355_dev_alloc(client, &d_rx, one_cap));
    OK(mi355_dev_alloc(client, &d_cstates, (size_t)S * n));
    int fds[2];
    if (pipe(fds) != 0) return 1;
    std::vector<uint8_t> bases((size_t)S * n), host_frames((size_t)S * n), frames((size_t)B * n), s_states((size_t)S * n),
        c_states((size_t)S * n), cw_host(cw_cap), relay_rx(cw_cap), fwd(one_cap), rx(one_cap);
    for (int s = 0; s < S; s++)
        for (size_t i = 0; i < n; i++) bases[(size_t)s * n + i] = (uint8_t)(40 + (i * 7 + (size_t)s * 31) % 150);
    OK(mi355_upload(server, d_sstates, bases.data(), bases.size()));
    if (!through_pipe(fds[1], fds[0], bases.data(), host_frames.data(), bases.size())) return 1;
    OK(mi355_upload(client, d_cstates, host_frames.data(), host_frames.size()));
    std::vector<uint8_t> base(n), frame(n);
    std::vector<uint32_t> off(B + 1), counts(B), escapes(B), roff(S + 1), ocounts(S), oescapes(S);
    std::vector<uint64_t> pos(B + 1), rpos(S + 1);
    size_t received = 0, forwarded = 0, changed = 0, kept = 0;
    int max_err = 0, calls = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K, nrec = S * nb;
        for (int s = 0; s < S; s++) {   // camera s's nb frames, one behind the other
            memcpy(base.data(), &bases[(size_t)s * n], n);
            for (int k = 0; k < nb; k++) {
                make_frame(frame, base, w, h, t0 + k + 5 * s);
                memcpy(&frames[((size_t)s * nb + k) * n], frame.data(), n);
            }
        }
        // ---- server: nb ticks of S cameras -> S * nb records in one call
        OK(mi355_upload(server, d_frames, frames.data(), (size_t)nrec * n));
        OK(mi355_diff_multi_stream_cwire_batch(server, d_frames, d_sstates, n, S, nb, d_off, d_pos, d_cw, cw_cap));
        OK(mi355_download(server, off.data(), d_off, sizeof(uint32_t) * (nrec + 1)));
        OK(mi355_download(server, pos.data(), d_pos, sizeof(uint64_t) * (nrec + 1)));
        if (pos[nrec] > cw_cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
        const size_t cb = (size_t)pos[nrec];
        OK(mi355_download(server, cw_host.data(), d_cw, cb));
        changed += off[nrec];
        // ---- the sockets into the relay: camera s's slice is one write; the relay reads the headers, uploads the slice as it
        // came; a host client beside it applies all nb original records of the camera
        size_t p = 0;
        for (int s = 0; s < S; s++) {
            const size_t a = (size_t)pos[(size_t)s * nb], b = (size_t)pos[(size_t)(s + 1) * nb];
            if (a != p) { fprintf(stderr, "stream framing broken\n"); return 1; }
            if (!through_pipe(fds[1], fds[0], cw_host.data() + a, relay_rx.data() + a, b - a)) return 1;
            for (int k = 0; k < nb; k++) {
                const int r = s * nb + k;
                if (p + 8 > b) { fprintf(stderr, "stream framing broken\n"); return 1; }
                memcpy(&counts[r], relay_rx.data() + p, 4);
                memcpy(&escapes[r], relay_rx.data() + p + 4, 4);
                size_t used = 0;
                OK(mi355_cwire_apply_host(&host_frames[(size_t)s * n], n, relay_rx.data() + p, b - p, 1, &used));
                if (used != mi355_cwire_frame_bytes(counts[r], escapes[r])) { fprintf(stderr, "stream framing broken\n"); return 1; }
                p += used;
            }
            if (p != b) { fprintf(stderr, "stream framing broken\n"); return 1; }
            if (b > a) OK(mi355_upload(relay, (uint8_t *)d_in + a, relay_rx.data() + a, b - a));
        }
        received += cb;
        // ---- relay: the burst -> one record per camera, in one call; no frame exists here
        OK(mi355_cwire_coalesce_cwire_batch(relay, d_in, counts.data(), escapes.data(), S, nb, d_roff, d_rpos, d_fwd, one_cap));
        calls++;
        OK(mi355_download(relay, roff.data(), d_roff, sizeof(uint32_t) * (S + 1)));
        OK(mi355_download(relay, rpos.data(), d_rpos, sizeof(uint64_t) * (S + 1)));
        if (rpos[S] > one_cap) { fprintf(stderr, "coalesced stream larger than its bound\n"); return 1; }
        const size_t fb = (size_t)rpos[S];
        OK(mi355_download(relay, fwd.data(), d_fwd, fb));
        kept += roff[S];
        // ---- the sockets out of the relay, one record per camera; the receiver finds them from their headers
        if (!through_pipe(fds[1], fds[0], fwd.data(), rx.data(), fb)) return 1;
        forwarded += fb;
        p = 0;
        for (int s = 0; s < S; s++) {
            if (p + 8 > fb) { fprintf(stderr, "forwarded framing broken\n"); return 1; }
            memcpy(&ocounts[s], rx.data() + p, 4);
            memcpy(&oescapes[s], rx.data() + p + 4, 4);
            p += mi355_cwire_frame_bytes(ocounts[s], oescapes[s]);
        }
        if (p != fb) { fprintf(stderr, "forwarded framing broken\n"); return 1; }
        // ---- receiver: one call per burst
        OK(mi355_upload(client, d_rx, rx.data(), fb));
        OK(mi355_apply_multi_cwire_batch(client, d_rx, ocounts.data(), oescapes.data(), S, d_cstates, n));
        OK(mi355_download(client, c_states.data(), d_cstates, c_states.size()));
        OK(mi355_download(server, s_states.data(), d_sstates, s_states.size()));
        for (int s = 0; s < S; s++)
            if (memcmp(&host_frames[(size_t)s * n], &c_states[(size_t)s * n], n) != 0) {
                fprintf(stderr, "burst at tick %d: camera %d: receiver state != host client that applied all %d records\n", t0, s, nb);
                return 1;
            }
        if (memcmp(s_states.data(), c_states.data(), s_states.size()) != 0) {
            fprintf(stderr, "burst at tick %d: receiver states != server states\n", t0);
            return 1;
        }
        for (int s = 0; s < S; s++)
            for (size_t i = 0; i < n; i++) {
                const int e = abs((int)c_states[(size_t)s * n + i] - (int)frames[((size_t)s * nb + nb - 1) * n + i]);
                if (e > max_err) max_err = e;
            }
    }
    if (max_err > cfg.threshold) { fprintf(stderr, "rebuilt frame off by %d > threshold\n", max_err); return 1; }
    void *srv[] = {d_frames, d_sstates, d_off, d_pos, d_cw};
    for (void *q : srv) OK(mi355_dev_free(server, q));
    void *rel[] = {d_in, d_roff, d_rpos, d_fwd};
    for (void *q : rel) OK(mi355_dev_free(relay, q));
    OK(mi355_dev_free(client, d_rx));
    OK(mi355_dev_free(client, d_cstates));
    mi355_destroy(server);
    mi355_destroy(relay);
    mi355_destroy(client);
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"coalesce\": true, \"relay_calls\": %d, "
           "\"width\": %d, \"height\": %d, \"ticks\": %d, \"changed_bytes\": %zu, \"coalesced_entries\": %zu, "
           "\"relay_received_bytes\": %zu, \"relay_forwarded_bytes\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d}\n",
           S, K, calls, w, h, T, changed, kept, received, forwarded, (size_t)T * S * n, max_err);
    return 0;
}

// --compact --per-frame (see the head of the file)
namespace {
struct Expected {   // the plain path's client frames, in order, from the sender to the receiver thread
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::vector<uint8_t> > q;
    void push(const std::vector<uint8_t> &f) {
        { std::lock_guard<std::mutex> l(m); q.push_back(f); }
        cv.notify_one();
    }
    std::vector<uint8_t> pop() {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [this] { return !q.empty(); });
        std::vector<uint8_t> f = std::move(q.front());
        q.pop_front();
        return f;
    }
};
struct Receiver {
    int fd, frames;
    size_t n;
    Expected *expected;
    int equal = 0;
    size_t bytes = 0;
    std::string error;
    void run() {
        receive();
        if (!error.empty()) close(fd);   // the sender's next write then fails instead of waiting for a reader that has left
    }
    void receive() {   // opencv.cpp:38-66 over the compact stream: the base frame, then header + body per frame
        std::vector<uint8_t> frame(n), rec;
        if (!read_all(fd, frame.data(), n)) { error = "base frame: short read"; return; }
        for (int t = 0; t < frames; t++) {
            uint32_t hdr[2];
            if (!read_all(fd, hdr, 8)) { error = "record header: short read"; return; }
            const size_t len = mi355_cwire_frame_bytes(hdr[0], hdr[1]);
            rec.resize(len);
            memcpy(rec.data(), hdr, 8);
            if (!read_all(fd, rec.data() + 8, len - 8)) { error = "record body: short read"; return; }
            size_t used = 0;
            if (mi355_cwire_apply_host(frame.data(), n, rec.data(), len, 1, &used) != MI355_OK || used != len) {
                error = std::string("mi355_cwire_apply_host: ") + mi355_last_error();
                return;
            }
            bytes += len;
            const std::vector<uint8_t> want = expected->pop();
            if (want.size() != n || memcmp(want.data(), frame.data(), n) != 0) {
                error = "frame " + std::to_string(t) + ": compact client frame != plain client frame";
                return;
            }
            equal++;
        }
    }
};
}  // namespace

static int run_per_frame(int w, int h, int T) {
    const size_t n = (size_t)3 * w * h;
    const int depth = 4;
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = 1; cfg.device = -1;
    mi355_core *server = nullptr, *plain = nullptr;
    OK(mi355_create(&cfg, &server));
    OK(mi355_create(&cfg, &plain));
    std::vector<uint8_t> base(n), frame(n), p_frame(n), s_state(n);
    for (size_t i = 0; i < n; i++) base[i] = (uint8_t)(40 + (i * 7) % 150);
    OK(mi355_set_state(server, base.data()));
    OK(mi355_set_state(plain, base.data()));
    OK(mi355_prepare(server, MI355_PREPARE_EXEC_CWIRE));
    p_frame = base;
    const size_t cap = mi355_cwire_bytes_max(n, 1);
    void *h_frame[depth], *h_rec[depth], *p_in = nullptr, *p_xs = nullptr;
    for (int i = 0; i < depth; i++) {
        OK(mi355_host_alloc(&h_frame[i], n));
        OK(mi355_host_alloc(&h_rec[i], cap));
    }
    OK(mi355_host_alloc(&p_in, n));
    OK(mi355_host_alloc(&p_xs, n * sizeof(int32_t)));
    int fds[2];
    if (pipe(fds) != 0) return 1;
    OK(mi355_pipe_open(server, depth));
    // (from here to receiver.join() an error ends the loop, not the function: the thread is joined first)
    Expected expected;
    Receiver rx;
    rx.fd = fds[0]; rx.frames = T; rx.n = n; rx.expected = &expected;
    signal(SIGPIPE, SIG_IGN);   // (a write to a pipe the receiver has closed returns an error)
    std::thread receiver(&Receiver::run, &rx);
    bool ok = true;
    auto send = [&](const void *p, size_t len) {   // ONE write per record; the loop only serves a short write
        const uint8_t *b = (const uint8_t *)p;
        while (len) {
            const ssize_t k = write(fds[1], b, len);
            if (k <= 0) return false;
            b += k;
            len -= (size_t)k;
        }
        return true;
    };
    ok = send(base.data(), n);   // threads.cpp:220
    int64_t tickets[depth];
    size_t changed = 0, sent_bytes = 0;
    int rc = 0;
    auto finish = [&](int t) -> int {   // the sender thread's part: wait for frame t, one write
        uint32_t pos = 0, esc = 0;
        size_t len = 0;
        OK(mi355_pipe_wait_cwire(server, tickets[t % depth], &pos, &esc, &len));
        if (len != mi355_cwire_frame_bytes(pos, esc) || len > cap) { fprintf(stderr, "frame %d: record size\n", t); return 1; }
        changed += pos;
        sent_bytes += len;
        if (!send(h_rec[t % depth], len)) { fprintf(stderr, "write failed\n"); return 1; }
        return 0;
    };
    for (int t = 0; t < T && ok && !rc; t++) {
        if (t >= depth) rc = finish(t - depth);
        if (rc) break;
        make_frame(frame, base, w, h, t);
        // the plain path beside it: mi355_exec on its own core, and its host client
        memcpy(p_in, frame.data(), n);
        uint32_t pos = 0;
        if (mi355_exec(plain, (uint8_t *)p_in, nullptr, nullptr, &pos, (int32_t *)p_xs) != MI355_OK) {
            fprintf(stderr, "mi355_exec failed: %s\n", mi355_last_error());
            rc = 1;
            break;
        }
        for (uint32_t i = 0; i < pos; i++) p_frame[((const int32_t *)p_xs)[i]] += ((const uint8_t *)p_in)[i];
        expected.push(p_frame);
        // the elaboration loop: one host frame in, a ticket out
        memcpy(h_frame[t % depth], frame.data(), n);
        if (mi355_pipe_submit_cwire(server, (const uint8_t *)h_frame[t % depth], nullptr, nullptr, h_rec[t % depth], cap,
                                    &tickets[t % depth]) != MI355_OK) {
            fprintf(stderr, "mi355_pipe_submit_cwire failed: %s\n", mi355_last_error());
            rc = 1;
            break;
        }
    }
    for (int t = T > depth ? T - depth : 0; t < T && ok && !rc; t++) rc = finish(t);
    close(fds[1]);   // (a receiver that still waits for bytes sees the end of the stream)
    if (rc || !ok)
        for (int t = 0; t < T; t++) expected.push(std::vector<uint8_t>());   // ... and one that waits for a frame gets a wrong one
    receiver.join();
    if (rc || !ok) return 1;
    if (!rx.error.empty()) { fprintf(stderr, "%s\n", rx.error.c_str()); return 1; }
    OK(mi355_pipe_close(server));
    OK(mi355_get_state(server, s_state.data()));
    if (memcmp(s_state.data(), p_frame.data(), n) != 0) { fprintf(stderr, "server state != plain client frame\n"); return 1; }
    for (int i = 0; i < depth; i++) {
        OK(mi355_host_free(h_frame[i]));
        OK(mi355_host_free(h_rec[i]));
    }
    OK(mi355_host_free(p_in));
    OK(mi355_host_free(p_xs));
    mi355_destroy(server);
    mi355_destroy(plain);
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"per_frame\": true, \"depth\": %d, \"width\": %d, \"height\": %d, "
           "\"frames\": %d, \"frames_equal\": %d, \"changed_bytes\": %zu, \"wire_bytes\": %zu, \"reference_wire_bytes\": %zu, "
           "\"raw_bytes\": %zu}\n",
           depth, w, h, T, rx.equal, changed, sent_bytes, mi355_wire_bytes(T, changed), (size_t)T * n);
    return rx.equal == T ? 0 : 1;
}

// --compact --multi S --resync R [--burst K] (see the head of the file)
static int run_multi_resync(int w, int h, int T, int S, int R, int K, int wall_k) {
    const size_t n = (size_t)3 * w * h;
    if (R < 0 || R + 1 >= T) { fprintf(stderr, "--resync K needs 0 <= K and K + 1 < --frames\n"); return 2; }
    if (K < 1) K = 1;
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = S * K; cfg.device = -1;
    mi355_core *server = nullptr, *client = nullptr;
    OK(mi355_create(&cfg, &server));
    cfg.max_batch = S;
    OK(mi355_create(&cfg, &client));
    const int B = S * K, victim = R % S;
    const size_t cw_cap = mi355_cwire_bytes_max(n, B), tick_cap = mi355_cwire_bytes_max(n, S);
    const size_t tiles = mi355_state_tiles(n), mask_words = (tiles + 31) / 32;
    const size_t dig_bytes = 8 * (size_t)S * tiles, mask_bytes = 4 * (size_t)S * mask_words;
    void *d_frames = nullptr, *d_sstates = nullptr, *d_off = nullptr, *d_pos = nullptr, *d_cw = nullptr;   // server
    void *d_peer = nullptr, *d_smask = nullptr, *d_roff = nullptr, *d_rpos = nullptr, *d_rcw = nullptr;    // ... its refresh
    void *d_rx = nullptr, *d_cstates = nullptr, *d_dig = nullptr, *d_cmask = nullptr;                      // client
    OK(mi355_dev_alloc(server, &d_frames, (size_t)B * n));
    OK(mi355_dev_alloc(server, &d_sstates, (size_t)S * n));
    OK(mi355_dev_alloc(server, &d_off, sizeof(uint32_t) * (B + 1)));
    OK(mi355_dev_alloc(server, &d_pos, sizeof(uint64_t) * (B + 1)));
    OK(mi355_dev_alloc(server, &d_cw, cw_cap));
    OK(mi355_dev_alloc(server, &d_peer, dig_bytes));
    OK(mi355_dev_alloc(server, &d_smask, mask_bytes));
    OK(mi355_dev_alloc(server, &d_roff, sizeof(uint32_t) * (S + 1)));
    OK(mi355_dev_alloc(server, &d_rpos, sizeof(uint64_t) * (S + 1)));
    OK(mi355_dev_alloc(server, &d_rcw, tick_cap));
    OK(mi355_dev_alloc(client, &d_rx, tick_cap));
    OK(mi355_dev_alloc(client, &d_cstates, (size_t)S * n));
    OK(mi355_dev_alloc(client, &d_dig, dig_bytes));
    OK(mi355_dev_alloc(client, &d_cmask, mask_bytes));
    WallCheck wall;
    if (wall_k)
        if (int rc = wall.open(client, w, h, wall_k, S)) return rc;
    int fds[2];
    if (pipe(fds) != 0) return 1;
    // truth: a host client per camera that applies EVERY record -- the sender's state after every tick
    std::vector<uint8_t> bases((size_t)S * n), truth((size_t)S * n), frames((size_t)B * n), s_states((size_t)S * n),
        c_states((size_t)S * n), cw_host(cw_cap), rx(cw_cap), stage(tick_cap), host_client;
    for (int s = 0; s < S; s++)
        for (size_t i = 0; i < n; i++) bases[(size_t)s * n + i] = (uint8_t)(40 + (i * 7 + (size_t)s * 31) % 150);
    OK(mi355_upload(server, d_sstates, bases.data(), bases.size()));
    if (!through_pipe(fds[1], fds[0], bases.data(), truth.data(), bases.size())) return 1;
    OK(mi355_upload(client, d_cstates, truth.data(), truth.size()));
    if (int rc = wall.full(d_cstates)) return rc;
    std::vector<uint8_t> base(n), frame(n);
    std::vector<uint32_t> off(B + 1), counts(S), escapes(S), dig(2 * (size_t)S * tiles), dig_up(dig.size()), dig_host(2 * tiles),
        mask(S * mask_words), mask_rx(mask.size());
    std::vector<uint64_t> pos(B + 1), rpos(S + 1);
    std::vector<size_t> at(B), len(B);
    size_t sent_bytes = 0, refresh_bytes = 0, lost_entries = 0, tiles_selected = 0;
    int wrong_ticks = 0, right_ticks_after = 0;
    bool lost = false, refreshed = false;
    // the receiver's frames of tick t against the truth: while the record is lost the victim's differs and only the victim's
    auto compare = [&](int t) -> int {
        for (int s = 0; s < S; s++) {
            const bool same = memcmp(&truth[(size_t)s * n], &c_states[(size_t)s * n], n) == 0;
            const bool wrong = lost && !refreshed && s == victim;
            if (same == wrong) {
                fprintf(stderr, "tick %d: camera %d: the receiver's frame %s the sender's\n", t, s, same ? "equals" : "differs from");
                return 1;
            }
        }
        if (lost && !refreshed) wrong_ticks++;
        if (refreshed) right_ticks_after++;
        return 0;
    };
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K, nrec = S * nb;
        for (int s = 0; s < S; s++) {   // camera s's nb frames, one behind the other
            memcpy(base.data(), &bases[(size_t)s * n], n);
            for (int k = 0; k < nb; k++) {
                make_frame(frame, base, w, h, t0 + k + 5 * s);
                memcpy(&frames[((size_t)s * nb + k) * n], frame.data(), n);
            }
        }
        // ---- server: nb ticks of S cameras
        OK(mi355_upload(server, d_frames, frames.data(), (size_t)nrec * n));
        if (K == 1) OK(mi355_diff_multi_cwire_batch(server, d_frames, d_sstates, n, S, d_off, d_pos, d_cw, cw_cap));
        else OK(mi355_diff_multi_stream_cwire_batch(server, d_frames, d_sstates, n, S, nb, d_off, d_pos, d_cw, cw_cap));
        OK(mi355_download(server, pos.data(), d_pos, sizeof(uint64_t) * (nrec + 1)));
        if (pos[nrec] > cw_cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
        const size_t cb = (size_t)pos[nrec];
        OK(mi355_download(server, cw_host.data(), d_cw, cb));
        if (!through_pipe(fds[1], fds[0], cw_host.data(), rx.data(), cb)) return 1;
        sent_bytes += cb;
        size_t p = 0;
        for (int r = 0; r < nrec; r++) {   // the records of every socket, found from their headers
            if (p + 8 > cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
            uint32_t c, e;
            memcpy(&c, rx.data() + p, 4);
            memcpy(&e, rx.data() + p + 4, 4);
            at[r] = p;
            len[r] = mi355_cwire_frame_bytes(c, e);
            p += len[r];
        }
        if (p != cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
        // ---- client: tick k = record (s, k) of every s back to back, one upload, one call
        bool asked = false;
        for (int k = 0; k < nb; k++) {
            const int t = t0 + k;
            size_t q = 0;
            for (int s = 0; s < S; s++) {
                const int r = s * nb + k;
                size_t used = 0;
                OK(mi355_cwire_apply_host(&truth[(size_t)s * n], n, rx.data() + at[r], len[r], 1, &used));
                if (used != len[r]) { fprintf(stderr, "stream framing broken\n"); return 1; }
                if (t == R && s == victim) {   // the loss: the receiver has nothing to apply for this camera
                    memcpy(&lost_entries, rx.data() + at[r], 4);
                    if (lost_entries == 0) { fprintf(stderr, "--resync: the record to drop holds no entry\n"); return 1; }
                    memset(stage.data() + q, 0, 8);
                    counts[s] = escapes[s] = 0;
                    q += 8;
                    lost = true;
                    continue;
                }
                memcpy(stage.data() + q, rx.data() + at[r], len[r]);
                memcpy(&counts[s], stage.data() + q, 4);
                memcpy(&escapes[s], stage.data() + q + 4, 4);
                q += len[r];
            }
            OK(mi355_upload(client, d_rx, stage.data(), q));
            OK(mi355_apply_multi_cwire_batch(client, d_rx, counts.data(), escapes.data(), S, d_cstates, n));
            if (int rc = wall.update(d_rx, counts.data(), escapes.data(), 1, d_cstates)) return rc;   // (the wall shows what it holds)
            if (t == R + 1) {   // the receiver asks: its digests go up
                OK(mi355_state_digest_batch(client, d_cstates, n, S, d_dig));
                OK(mi355_download(client, dig.data(), d_dig, dig_bytes));
                asked = true;
            }
            OK(mi355_download(client, c_states.data(), d_cstates, c_states.size()));
            if (asked && t == R + 1)
                for (int s = 0; s < S; s++) {
                    OK(mi355_state_digest_host(&c_states[(size_t)s * n], n, dig_host.data()));
                    if (memcmp(dig_host.data(), &dig[2 * (size_t)s * tiles], 8 * tiles) != 0) {
                        fprintf(stderr, "tick %d: camera %d: device digests != host digests\n", t, s);
                        return 1;
                    }
                }
            if (int rc = compare(t)) return rc;
            if (int rc = wall.compare(c_states.data(), t)) return rc;
        }
        // ---- the states at both ends of the burst: the truth is the sender's
        OK(mi355_download(server, s_states.data(), d_sstates, s_states.size()));
        if (memcmp(s_states.data(), truth.data(), s_states.size()) != 0) { fprintf(stderr, "tick %d: host frames != server states\n", t0); return 1; }
        if (!asked) continue;
        const bool in_flight = t0 + nb - 1 > R + 1;
        // ---- server: the answer, behind its latest tick
        if (!through_pipe(fds[1], fds[0], (const uint8_t *)dig.data(), (uint8_t *)dig_up.data(), dig_bytes)) return 1;
        OK(mi355_upload(server, d_peer, dig_up.data(), dig_bytes));
        OK(mi355_refresh_cwire_batch(server, d_sstates, n, S, d_peer, d_smask, d_roff, d_rpos, d_rcw, tick_cap));
        OK(mi355_download(server, rpos.data(), d_rpos, sizeof(uint64_t) * (S + 1)));
        OK(mi355_download(server, mask.data(), d_smask, mask_bytes));
        refresh_bytes = (size_t)rpos[S];
        if (refresh_bytes > tick_cap) { fprintf(stderr, "refresh records larger than their bound\n"); return 1; }
        OK(mi355_download(server, cw_host.data(), d_rcw, refresh_bytes));
        if (!through_pipe(fds[1], fds[0], (const uint8_t *)mask.data(), (uint8_t *)mask_rx.data(), mask_bytes)) return 1;
        if (!through_pipe(fds[1], fds[0], cw_host.data(), stage.data(), refresh_bytes)) return 1;
        // ---- client: clear, then apply like any other records; a host client does the same beside it
        host_client = c_states;
        p = 0;
        for (int s = 0; s < S; s++) {
            if (p + 8 > refresh_bytes) { fprintf(stderr, "refresh framing broken\n"); return 1; }
            memcpy(&counts[s], stage.data() + p, 4);
            memcpy(&escapes[s], stage.data() + p + 4, 4);
            size_t bits = 0;
            for (size_t tl = 0; tl < tiles; tl++)
                if (mask_rx[s * mask_words + (tl >> 5)] >> (tl & 31) & 1u) {
                    bits++;
                    const size_t lo = tl * 4096, hi = lo + 4096 < n ? lo + 4096 : n;
                    memset(&host_client[(size_t)s * n + lo], 0, hi - lo);
                }
            // (ticks in flight behind the digests changed tiles of every camera: those are selected too, wasteful and never wrong)
            if (s == victim ? bits == 0 : !in_flight && (bits != 0 || counts[s] != 0)) {
                fprintf(stderr, "refresh: camera %d: %zu tiles selected, %u entries\n", s, bits, counts[s]);
                return 1;
            }
            tiles_selected += bits;
            size_t used = 0;
            OK(mi355_cwire_apply_host(&host_client[(size_t)s * n], n, stage.data() + p, refresh_bytes - p, 1, &used));
            p += used;
        }
        if (p != refresh_bytes) { fprintf(stderr, "refresh framing broken\n"); return 1; }
        OK(mi355_upload(client, d_cmask, mask_rx.data(), mask_bytes));
        OK(mi355_upload(client, d_rx, stage.data(), refresh_bytes));
        OK(mi355_state_clear_tiles_batch(client, d_cstates, n, S, d_cmask));
        OK(mi355_apply_multi_cwire_batch(client, d_rx, counts.data(), escapes.data(), S, d_cstates, n));
        if (int rc = wall.masked(d_cmask, d_cstates)) return rc;   // the refresh's own mask: what was cleared and refilled is repainted
        OK(mi355_download(client, c_states.data(), d_cstates, c_states.size()));
        if (int rc = wall.compare(c_states.data(), t0 + nb - 1)) return rc;
        refreshed = true;
        if (memcmp(c_states.data(), host_client.data(), c_states.size()) != 0) { fprintf(stderr, "refresh: client states != host client frames\n"); return 1; }
        if (memcmp(c_states.data(), s_states.data(), c_states.size()) != 0) { fprintf(stderr, "refresh: client states != server states\n"); return 1; }
    }
    if (!refreshed || wrong_ticks < 1) { fprintf(stderr, "--resync: no refresh happened\n"); return 1; }
    void *srv[] = {d_frames, d_sstates, d_off, d_pos, d_cw, d_peer, d_smask, d_roff, d_rpos, d_rcw};
    for (void *q : srv) OK(mi355_dev_free(server, q));
    void *cli[] = {d_rx, d_cstates, d_dig, d_cmask};
    for (void *q : cli) OK(mi355_dev_free(client, q));
    if (int rc = wall.close()) return rc;
    mi355_destroy(server);
    mi355_destroy(client);
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"resync\": %d, \"width\": %d, \"height\": %d, "
           "\"ticks\": %d, \"dropped_camera\": %d, \"dropped_entries\": %zu, \"wrong_ticks\": %d, \"ticks_equal_after_refresh\": %d, "
           "\"tiles\": %zu, \"tiles_selected\": %zu, \"digest_bytes\": %zu, \"mask_bytes\": %zu, \"refresh_bytes\": %zu, "
           "\"key_frame_bytes\": %zu, \"wire_bytes\": %zu%s}\n",
           S, K, R, w, h, T, victim, lost_entries, wrong_ticks, right_ticks_after, tiles, tiles_selected, dig_bytes, mask_bytes,
           refresh_bytes, (size_t)S * n, sent_bytes, wall.json().c_str());
    return 0;
}

int main(int argc, char **argv) {
    int w = 320, h = 180, T = 24, B = 8, multi = 0, burst = 0, activity = -1, resync = -1, wall = 0;
    long budget = -1;
    bool compact = false, direct = false, gpu_client = false, burst_client = false, coalesce = false, per_frame = false, check = false;
    for (int i = 1; i < argc; i++) {
        if (std::string(argv[i]) == "--compact") compact = true;
        if (std::string(argv[i]) == "--direct") direct = true;
        if (std::string(argv[i]) == "--gpu-client") gpu_client = true;
        if (std::string(argv[i]) == "--burst-client") burst_client = true;
        if (std::string(argv[i]) == "--coalesce") coalesce = true;
        if (std::string(argv[i]) == "--per-frame") per_frame = true;
        if (std::string(argv[i]) == "--check") check = true;
    }
    if (direct && !compact) { fprintf(stderr, "--direct needs --compact\n"); return 2; }
    if (gpu_client && !compact) { fprintf(stderr, "--gpu-client needs --compact\n"); return 2; }
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--compact" || k == "--direct" || k == "--gpu-client" || k == "--burst-client" || k == "--coalesce" || k == "--per-frame" || k == "--check") { i--; continue; }
        const int v = atoi(argv[i + 1]);
        if (k == "--width") w = v; else if (k == "--height") h = v;
        else if (k == "--frames") T = v; else if (k == "--batch") B = v;
        else if (k == "--multi") multi = v;
        else if (k == "--burst") burst = v;
        else if (k == "--activity") activity = v < 0 ? 0 : v;
        else if (k == "--resync") resync = v < 0 ? 0 : v;
        else if (k == "--wall") wall = v < 1 ? -1 : v;
        else if (k == "--budget") budget = atol(argv[i + 1]) < 0 ? 0 : atol(argv[i + 1]);
    }
    if (burst && (!multi || burst < 0)) { fprintf(stderr, "--burst K needs --multi S and K >= 1\n"); return 2; }
    if (burst_client && (!compact || !multi || !burst)) { fprintf(stderr, "--burst-client needs --compact --multi S --burst K\n"); return 2; }
    if (coalesce && (!compact || !multi || !burst || burst_client)) {
        fprintf(stderr, "--coalesce needs --compact --multi S --burst K, without --burst-client\n");
        return 2;
    }
    if (budget >= 0 && (!compact || !multi || burst || direct || gpu_client || per_frame)) {
        fprintf(stderr, "--budget BYTES needs --compact --multi S alone\n");
        return 2;
    }
    if (activity >= 0 && (activity == 0 || !compact || !multi || budget >= 0 || coalesce || (burst && !burst_client))) {
        fprintf(stderr, "--activity CELL needs CELL >= 1 and --compact --multi S, alone or with --burst K --burst-client\n");
        return 2;
    }
    if (activity < 0) activity = 0;
    if (check && (!compact || !multi || budget >= 0 || coalesce || per_frame || (burst && !burst_client))) {
        fprintf(stderr, "--check needs --compact --multi S, alone or with --burst K --burst-client\n");
        return 2;
    }
    if (resync >= 0 && (!compact || !multi || budget >= 0 || coalesce || per_frame || burst_client || activity || check)) {
        fprintf(stderr, "--resync K needs --compact --multi S, alone or with --burst B\n");
        return 2;
    }
    if (wall && (wall < 0 || wall > 16 || !compact || !multi || budget >= 0 || coalesce || per_frame || (burst && !burst_client && resync < 0))) {
        fprintf(stderr, "--wall K needs 1 <= K <= 16 and --compact --multi S, alone, with --burst B --burst-client or with --resync R\n");
        return 2;
    }
    if (per_frame) {
        if (!compact || direct || gpu_client || multi) { fprintf(stderr, "--per-frame needs --compact alone\n"); return 2; }
        return run_per_frame(w, h, T);
    }
    if (multi) {
        if (!compact || direct || gpu_client || multi < 0) { fprintf(stderr, "--multi S needs --compact alone and S >= 1\n"); return 2; }
        if (resync >= 0) return run_multi_resync(w, h, T, multi, resync, burst, wall);
        if (burst_client) return run_multi_burst_client(w, h, T, multi, burst, activity, check, wall);
        if (coalesce) return run_multi_burst_coalesce(w, h, T, multi, burst);
        if (budget >= 0) return run_multi_budget(w, h, T, multi, budget);
        return burst ? run_multi_burst(w, h, T, multi, burst) : run_multi(w, h, T, multi, activity, check, wall);
    }
    const size_t n = (size_t)3 * w * h;
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = B; cfg.device = -1;
    mi355_core *server = nullptr, *client = nullptr;
    OK(mi355_create(&cfg, &server));
    OK(mi355_create(&cfg, &client));

    std::vector<uint8_t> base(n), frame(n), frames((size_t)B * n), shown((size_t)B * n), s_state(n), c_state(n);
    for (size_t i = 0; i < n; i++) base[i] = (uint8_t)(40 + (i * 7) % 150);
    OK(mi355_set_state(server, base.data()));                  // kernels.cu:406

    int fds[2];
    if (pipe(fds) != 0) return 1;
    // ---- sender side: the base frame first (threads.cpp:220)
    std::vector<uint8_t> wire_host(mi355_wire_bytes(B, (uint64_t)B * n));
    void *d_frames = nullptr, *d_wire = nullptr, *d_off = nullptr, *d_cwire = nullptr, *d_shown = nullptr;
    OK(mi355_dev_alloc(server, &d_frames, (size_t)B * n));
    OK(mi355_dev_alloc(server, &d_wire, wire_host.size()));
    OK(mi355_dev_alloc(server, &d_off, sizeof(uint32_t) * (B + 1)));
    OK(mi355_dev_alloc(client, &d_cwire, wire_host.size()));
    OK(mi355_dev_alloc(client, &d_shown, (size_t)B * n));

    // ---- client start-up: read the base frame (opencv.cpp:38-46)
    std::vector<uint8_t> got_base(n);
    if (!through_pipe(fds[1], fds[0], base.data(), got_base.data(), n)) return 1;
    OK(mi355_set_state(client, got_base.data()));

    size_t sent_bytes = 0, changed = 0;
    int max_err = 0;
    if (compact) {
        // ---- sender: pack + encode on the GPU; client: the host decoder on a host frame (no core)
        void *d_xs = nullptr, *d_df = nullptr, *d_pos = nullptr, *d_cw = nullptr;
        const size_t cap = (size_t)B * n, cw_cap = mi355_cwire_bytes_max(n, B);
        if (!direct) {   // (the one-call form needs no arrays of 5 bytes per entry)
            OK(mi355_dev_alloc(server, &d_xs, cap * 4));
            OK(mi355_dev_alloc(server, &d_df, cap));
        }
        OK(mi355_dev_alloc(server, &d_pos, sizeof(uint64_t) * (B + 1)));
        OK(mi355_dev_alloc(server, &d_cw, cw_cap));
        std::vector<uint8_t> cw_host(cw_cap), rx(cw_cap), c_frame(got_base);
        for (int t0 = 0; t0 < T; t0 += B) {
            const int nb = T - t0 < B ? T - t0 : B;
            for (int k = 0; k < nb; k++) {
                make_frame(frame, base, w, h, t0 + k);
                memcpy(&frames[(size_t)k * n], frame.data(), n);
            }
            std::vector<uint32_t> off(nb + 1);
            std::vector<uint64_t> pos(nb + 1);
            OK(mi355_upload(server, d_frames, frames.data(), (size_t)nb * n));
            if (direct) {
                OK(mi355_diff_stream_cwire_batch(server, d_frames, n, nb, d_off, d_pos, d_cw, cw_cap));
            } else {
                OK(mi355_diff_stream_batch(server, d_frames, n, nb, d_off, d_xs, d_df, cap));
                OK(mi355_cwire_encode_batch(server, d_off, d_xs, d_df, cap, nb, d_pos, d_cw, cw_cap));
            }
            OK(mi355_download(server, off.data(), d_off, sizeof(uint32_t) * (nb + 1)));
            OK(mi355_download(server, pos.data(), d_pos, sizeof(uint64_t) * (nb + 1)));
            if (pos[nb] > cw_cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
            const size_t cb = (size_t)pos[nb];
            OK(mi355_download(server, cw_host.data(), d_cw, cb));
            changed += off[nb];
            if (!through_pipe(fds[1], fds[0], cw_host.data(), rx.data(), cb)) return 1;
            sent_bytes += cb;
            std::vector<uint32_t> counts(nb), escapes(nb);
            if (gpu_client) {   // the headers as the client reads them from the stream, then one call for the batch
                size_t p = 0;
                for (int k = 0; k < nb; k++) {
                    memcpy(&counts[k], rx.data() + p, 4);
                    memcpy(&escapes[k], rx.data() + p + 4, 4);
                    p += mi355_cwire_frame_bytes(counts[k], escapes[k]);
                }
                if (p != cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
                OK(mi355_upload(client, d_cwire, rx.data(), cb));
                OK(mi355_apply_cwire_batch(client, d_cwire, counts.data(), escapes.data(), nb, d_shown, n));
                OK(mi355_download(client, shown.data(), d_shown, (size_t)nb * n));
            }
            size_t at = 0;
            for (int k = 0; k < nb; k++) {   // one frame at a time: what the client shows after each
                size_t used = 0;
                OK(mi355_cwire_apply_host(c_frame.data(), n, rx.data() + at, cb - at, 1, &used));
                at += used;
                if (gpu_client && memcmp(&shown[(size_t)k * n], c_frame.data(), n) != 0) {
                    fprintf(stderr, "GPU client frame %d != host client frame\n", t0 + k);
                    return 1;
                }
                for (size_t i = 0; i < n; i++) {
                    const int e = abs((int)c_frame[i] - (int)frames[(size_t)k * n + i]);
                    if (e > max_err) max_err = e;
                }
            }
            if (at != cb) { fprintf(stderr, "stream framing broken\n"); return 1; }
            OK(mi355_get_state(server, s_state.data()));
            if (memcmp(s_state.data(), c_frame.data(), n) != 0) { fprintf(stderr, "client frame != server state\n"); return 1; }
            if (gpu_client) {
                OK(mi355_get_state(client, c_state.data()));
                if (memcmp(s_state.data(), c_state.data(), n) != 0) { fprintf(stderr, "GPU client state != server state\n"); return 1; }
            }
        }
        if (max_err > cfg.threshold) { fprintf(stderr, "rebuilt frame off by %d > threshold\n", max_err); return 1; }
        if (!direct) {
            OK(mi355_dev_free(server, d_xs));
            OK(mi355_dev_free(server, d_df));
        }
        OK(mi355_dev_free(server, d_pos));
        OK(mi355_dev_free(server, d_cw));
        OK(mi355_dev_free(server, d_frames));
        OK(mi355_dev_free(server, d_wire));
        OK(mi355_dev_free(server, d_off));
        OK(mi355_dev_free(client, d_cwire));
        OK(mi355_dev_free(client, d_shown));
        mi355_destroy(server);
        mi355_destroy(client);
        printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"direct\": %s, \"gpu_client\": %s, \"width\": %d, \"height\": %d, \"frames\": %d, \"batch\": %d, "
               "\"changed_bytes\": %zu, \"wire_bytes\": %zu, \"reference_wire_bytes\": %zu, \"raw_bytes\": %zu, "
               "\"max_abs_error\": %d}\n",
               direct ? "true" : "false", gpu_client ? "true" : "false", w, h, T, B, changed, sent_bytes, mi355_wire_bytes(T, changed), (size_t)T * n, max_err);
        return 0;
    }
    for (int t0 = 0; t0 < T; t0 += B) {
        const int nb = T - t0 < B ? T - t0 : B;
        for (int k = 0; k < nb; k++) {
            make_frame(frame, base, w, h, t0 + k);
            memcpy(&frames[(size_t)k * n], frame.data(), n);
        }
        // ---- server: one batch -> the socket bytes of nb frames
        std::vector<uint32_t> off(nb + 1);
        OK(mi355_upload(server, d_frames, frames.data(), (size_t)nb * n));
        OK(mi355_diff_stream_wire_batch(server, d_frames, n, nb, d_off, d_wire, wire_host.size()));
        OK(mi355_download(server, off.data(), d_off, sizeof(uint32_t) * (nb + 1)));
        const size_t wb = mi355_wire_bytes(nb, off[nb]);
        OK(mi355_download(server, wire_host.data(), d_wire, wb));
        changed += off[nb];
        // ---- the socket (a pipe here)
        std::vector<uint8_t> rx(wb);
        if (!through_pipe(fds[1], fds[0], wire_host.data(), rx.data(), wb)) return 1;
        sent_bytes += wb;
        // ---- client: parse the headers as opencv.cpp:52 does, hand the bytes to the device
        std::vector<uint32_t> counts(nb);
        size_t at = 0;
        for (int k = 0; k < nb; k++) {
            uint32_t pos;
            memcpy(&pos, &rx[at], 4);
            counts[k] = pos;
            at += 4 + (size_t)5 * pos;
        }
        if (at != wb) { fprintf(stderr, "stream framing broken\n"); return 1; }
        OK(mi355_upload(client, d_cwire, rx.data(), wb));
        OK(mi355_apply_wire_batch(client, d_cwire, counts.data(), nb, d_shown, n));
        OK(mi355_download(client, shown.data(), d_shown, (size_t)nb * n));
        // ---- checks
        OK(mi355_get_state(server, s_state.data()));
        OK(mi355_get_state(client, c_state.data()));
        if (memcmp(s_state.data(), c_state.data(), n) != 0) { fprintf(stderr, "client state != server state\n"); return 1; }
        if (memcmp(&shown[(size_t)(nb - 1) * n], c_state.data(), n) != 0) { fprintf(stderr, "last shown frame != state\n"); return 1; }
        for (size_t i = 0; i < (size_t)nb * n; i++) {
            const int e = abs((int)shown[i] - (int)frames[i]);
            if (e > max_err) max_err = e;
        }
    }
    if (max_err > cfg.threshold) { fprintf(stderr, "rebuilt frame off by %d > threshold\n", max_err); return 1; }
    OK(mi355_dev_free(server, d_frames));
    OK(mi355_dev_free(server, d_wire));
    OK(mi355_dev_free(server, d_off));
    OK(mi355_dev_free(client, d_cwire));
    OK(mi355_dev_free(client, d_shown));
    mi355_destroy(server);
    mi355_destroy(client);
    printf("{\"roundtrip\": \"ok\", \"width\": %d, \"height\": %d, \"frames\": %d, \"batch\": %d, "
           "\"changed_bytes\": %zu, \"wire_bytes\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d}\n",
           w, h, T, B, changed, sent_bytes, (size_t)T * n, max_err);
    return 0;
}

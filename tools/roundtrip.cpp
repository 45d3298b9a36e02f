// tools/roundtrip.cpp -- server -> socket bytes -> client, in plain C++ over the C-ABI only.
//
// Compiled with g++ (no HIP header, no HIP runtime call here): what a host written in any language with
// a C FFI does.  A "server" core packs a stream of frames into the byte stream the reference's sender
// thread writes (server/src/threads.cpp:220-233: base frame, then per frame u32 n | i32 xs[n] | u8 diff[n]);
// the bytes go through a pipe to a "client" that parses them exactly as client/opencv.cpp:38-66 does
// (read the base frame, then pos, pos indices, pos differences per frame) and rebuilds the frames on a
// second core.  The program checks that the client's frame equals the server's reconstructed state
// after every batch and that every rebuilt byte is within the threshold of the frame that was sent.
// Every other mode is described at the head of the run_* function, or of the check a mode hands its records to
// (ActivityCheck, RecordCheck, WallCheck, ThumbViewer), that is that mode.
//
//   tools/roundtrip [--width W] [--height H] [--frames T] [--batch B]
//                   [--compact [--direct] [--gpu-client] [--per-frame] [--multi S [--budget BYTES | --despeckle NEED | --burst K [--burst-client | --coalesce]] [--activity CELL] [--check] | --resync K [--burst B] | --crop X,Y,W,H [--burst K] | --mosaic CxR [--burst K] | [--burst K --coalesce] --datagram BYTES [--fec G[,K]] | --thumb K [--burst T] [--thumb-drop TICK]] [--wall K] [--runs]]
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

static mi355_config make_config(int w, int h, int max_batch) {
    mi355_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = w; cfg.height = h; cfg.threshold = 20; cfg.max_batch = max_batch; cfg.device = -1;
    return cfg;
}

// --compact --multi S ... --runs: the link's edge.  Behind whatever relay steps were asked for, the node that writes records to a
// stream socket run-codes them first (mi355_cwire_runs_encode_batch, MI355_RUNS_WHERE_SMALLER) and writes the forms table and
// then the bytes; the node that reads them decodes them (mi355_cwire_runs_decode_batch) and goes on as it did before, on the
// compact records it would have read without the flag -- which the tool checks byte for byte.  The two calls run on cores of
// their own, of the size of the frames whose records cross (a canvas for --mosaic).  Session::send_records is that socket.
static bool g_runs = false;
struct Session;
struct RunsLink {
    mi355_core *enc, *dec;
    int w, h, most;
    size_t cap;
    void *e_in, *e_forms, *e_pos, *e_out, *d_in, *d_pos, *d_out;
    std::vector<uint32_t> counts, escapes, forms, forms_rx;
    std::vector<uint64_t> pos;
    std::vector<uint8_t> link, link_rx;
    size_t compact_bytes, link_bytes, table_bytes, records, packed;
    RunsLink() : enc(nullptr), dec(nullptr), w(0), h(0), most(0), cap(0), compact_bytes(0), link_bytes(0), table_bytes(0), records(0), packed(0) {}
    int ensure(Session &ss, int nrec);
    int send(Session &ss, const uint8_t *src, uint8_t *dst, size_t bytes, int nrec);
};

// What one run holds: its cores, its pipe and every allocation it handed out.  A failure is printed where it happens and
// remembered: everything after it hands out nullptr, so a mode asks ok() once behind its set-up.  close() is for the success
// path; after an error the function returns and the process ends.
struct Session {
    int w, h, threshold, fds[2];
    size_t n;   // bytes of a frame
    bool failed = false;
    std::vector<mi355_core *> cores;
    struct Dev { mi355_core *core; void *p; };
    std::vector<Dev> devs;
    std::vector<void *> pins;
    RunsLink runs;   // --runs: what crosses the stream socket

    Session(int w_, int h_) : w(w_), h(h_), threshold(make_config(w_, h_, 1).threshold), n((size_t)3 * w_ * h_) {
        if (pipe(fds) != 0) failed = true;
    }
    bool ok() const { return !failed; }
    void *fail(const char *what) {
        if (!failed) fprintf(stderr, "%s failed: %s\n", what, mi355_last_error());
        failed = true;
        return nullptr;
    }
    mi355_core *core(int max_batch) { return core_of(w, h, max_batch); }
    mi355_core *core_of(int cw, int ch, int max_batch) {   // (a core of another frame size: the link of a canvas)
        const mi355_config cfg = make_config(cw, ch, max_batch);
        mi355_core *c = nullptr;
        if (failed || mi355_create(&cfg, &c) != MI355_OK) return (mi355_core *)fail("mi355_create");
        cores.push_back(c);
        return c;
    }
    void *dev(mi355_core *c, size_t bytes) {
        void *p = nullptr;
        if (failed || mi355_dev_alloc(c, &p, bytes) != MI355_OK) return fail("mi355_dev_alloc");
        devs.push_back(Dev{c, p});
        return p;
    }
    void *pinned(size_t bytes) {
        void *p = nullptr;
        if (failed || mi355_host_alloc(&p, bytes) != MI355_OK) return fail("mi355_host_alloc");
        pins.push_back(p);
        return p;
    }
    // "send" bytes and "receive" them: written in pieces that fit the pipe buffer, read back in between
    bool send(const void *src, void *dst, size_t bytes) { return through(fds, src, dst, bytes); }
    // nrec compact records to the stream socket and off it again; with --runs they cross it run-coded where that is smaller
    bool send_records(const uint8_t *src, uint8_t *dst, size_t bytes, int nrec) {
        if (!g_runs || nrec == 0) return send(src, dst, bytes);
        return runs.send(*this, src, dst, bytes, nrec) == 0;
    }
    static bool through(const int pipe_fds[2], const void *src, void *dst, size_t bytes) {   // (any pipe: a mode may open more)
        for (size_t at = 0; at < bytes;) {
            const size_t piece = bytes - at < 32768 ? bytes - at : 32768;
            if (write(pipe_fds[1], (const uint8_t *)src + at, piece) != (ssize_t)piece) return false;
            if (!read_all(pipe_fds[0], (uint8_t *)dst + at, piece)) return false;
            at += piece;
        }
        return true;
    }
    int close() {
        for (size_t i = 0; i < devs.size(); i++) OK(mi355_dev_free(devs[i].core, devs[i].p));
        for (size_t i = 0; i < pins.size(); i++) OK(mi355_host_free(pins[i]));
        for (size_t i = 0; i < cores.size(); i++) mi355_destroy(cores[i]);
        if (g_runs)
            printf("{\"runs\": true, \"records\": %zu, \"records_packed\": %zu, \"compact_bytes\": %zu, \"link_bytes\": %zu, "
                   "\"forms_table_bytes\": %zu}\n", runs.records, runs.packed, runs.compact_bytes, runs.link_bytes, runs.table_bytes);
        return 0;
    }
};

// ---- checks every mode makes
static int max_abs_error(const uint8_t *a, const uint8_t *b, size_t bytes) {
    int max_err = 0;
    for (size_t i = 0; i < bytes; i++) {
        const int e = abs((int)a[i] - (int)b[i]);
        if (e > max_err) max_err = e;
    }
    return max_err;
}

static int within_threshold(int max_err, const Session &ss) {
    if (max_err > ss.threshold) { fprintf(stderr, "rebuilt frame off by %d > threshold\n", max_err); return 1; }
    return 0;
}

// the two buffers are equal, or: "tick t: what" (t < 0: no tick to name)
static int same(const void *a, const void *b, size_t bytes, const char *what, int t = -1) {
    if (memcmp(a, b, bytes) == 0) return 0;
    if (t >= 0) fprintf(stderr, "tick %d: ", t);
    fprintf(stderr, "%s\n", what);
    return 1;
}

// The receiver's header walk: nrec records back to back in rx[p, end), found from their headers as they are read from a
// socket -> counts[r], escapes[r] and, if asked for, where each lies: at[r] .. at[r + 1]
static int walk_records(const uint8_t *rx, size_t p, size_t end, int nrec, uint32_t *counts, uint32_t *escapes, size_t *at) {
    int r = 0;
    for (; r < nrec && p + 8 <= end; r++) {
        memcpy(&counts[r], rx + p, 4);
        memcpy(&escapes[r], rx + p + 4, 4);
        if (at) at[r] = p;
        p += mi355_cwire_frame_bytes(counts[r], escapes[r]);
    }
    if (at) at[r] = p;
    if (r == nrec && p == end) return 0;
    fprintf(stderr, "stream framing broken\n");
    return 1;
}

int RunsLink::ensure(Session &ss, int nrec) {
    if (w == 0) { w = ss.w; h = ss.h; }
    if (nrec <= most) return 0;
    most = nrec;   // (a mode that sends more records later gets a larger pair of cores; the old ones go with the session)
    const size_t n = (size_t)3 * w * h;
    cap = mi355_cwire_runs_bytes_max(n, most, MI355_RUNS_WHERE_SMALLER);
    enc = ss.core_of(w, h, most);
    dec = ss.core_of(w, h, most);
    e_in = ss.dev(enc, cap); e_forms = ss.dev(enc, 16 * (size_t)most); e_pos = ss.dev(enc, 8 * ((size_t)most + 1)); e_out = ss.dev(enc, cap);
    d_in = ss.dev(dec, cap); d_pos = ss.dev(dec, 8 * ((size_t)most + 1)); d_out = ss.dev(dec, cap);
    counts.resize(most); escapes.resize(most); forms.resize(4 * (size_t)most); forms_rx.resize(4 * (size_t)most); pos.resize((size_t)most + 1);
    link.resize(cap); link_rx.resize(cap);
    return ss.ok() ? 0 : 1;
}

int RunsLink::send(Session &ss, const uint8_t *src, uint8_t *dst, size_t bytes, int nrec) {
    if (ensure(ss, nrec)) return 1;
    // ---- the sender's last call: its records (their headers are its own) -> the forms table and the link bytes
    if (bytes > cap || walk_records(src, 0, bytes, nrec, counts.data(), escapes.data(), nullptr)) return 1;
    OK(mi355_upload(enc, e_in, src, bytes));
    OK(mi355_cwire_runs_encode_batch(enc, e_in, counts.data(), escapes.data(), nrec, MI355_RUNS_WHERE_SMALLER, e_forms, e_pos, e_out, cap));
    OK(mi355_download(enc, forms.data(), e_forms, 16 * (size_t)nrec));
    OK(mi355_download(enc, pos.data(), e_pos, 8 * ((size_t)nrec + 1)));
    const size_t lb = (size_t)pos[nrec];
    if (lb > bytes) { fprintf(stderr, "--runs: the link bytes exceed the compact bytes\n"); return 1; }
    OK(mi355_download(enc, link.data(), e_out, lb));
    // ---- the socket: the table, then the bytes
    if (!ss.send(forms.data(), forms_rx.data(), 16 * (size_t)nrec) || !ss.send(link.data(), link_rx.data(), lb)) return 1;
    // ---- the receiver's first call: compact records again, where it would have read them
    OK(mi355_upload(dec, d_in, link_rx.data(), lb));
    OK(mi355_cwire_runs_decode_batch(dec, d_in, forms_rx.data(), nrec, d_pos, d_out, cap));
    OK(mi355_download(dec, pos.data(), d_pos, 8 * ((size_t)nrec + 1)));
    if (pos[nrec] != bytes) { fprintf(stderr, "--runs: the decoded records are %llu bytes, the sender's %zu\n", (unsigned long long)pos[nrec], bytes); return 1; }
    OK(mi355_download(dec, dst, d_out, bytes));
    if (memcmp(dst, src, bytes) != 0) { fprintf(stderr, "--runs: the decoded records differ from the sender's\n"); return 1; }
    for (int b = 0; b < nrec; b++) packed += forms[4 * (size_t)b] == MI355_RUNS_FORM_RUNS;
    records += nrec; compact_bytes += bytes; link_bytes += lb; table_bytes += 16 * (size_t)nrec;
    return 0;
}

// a host client beside a receiver: record r of a walk (rx, at) onto its frame; it must use the bytes the header said it has
static int host_apply(uint8_t *frame, size_t n, const uint8_t *rx, const size_t *at, int r) {
    size_t used = 0;
    OK(mi355_cwire_apply_host(frame, n, rx + at[r], at[r + 1] - at[r], 1, &used));
    if (used != at[r + 1] - at[r]) { fprintf(stderr, "stream framing broken\n"); return 1; }
    return 0;
}

// ---- the two ends of the many-camera modes
// The sender: S camera states on a core of its own, and one step of the loop -- upload the frames of nb ticks, diff them
// into records (one call), download offsets and positions, refuse a stream larger than its bound, download the bytes.
struct Sender {
    mi355_core *core = nullptr;
    int S = 0;
    size_t n = 0, cap = 0, cb = 0, changed = 0;   // cb: the bytes of the last step; changed: entries so far
    void *d_frames = nullptr, *d_states = nullptr, *d_off = nullptr, *d_pos = nullptr, *d_cw = nullptr;
    std::vector<uint8_t> frames, bytes, states;   // stream-major frames of a step, its records, the states (get_states)
    std::vector<uint32_t> off;
    std::vector<uint64_t> pos;

    int open(Session &ss, int S_, int K) {   // K: the most ticks in one step
        const int B = S_ * K;
        S = S_; n = ss.n; cap = mi355_cwire_bytes_max(n, B);
        core = ss.core(B);
        d_frames = ss.dev(core, (size_t)B * n);
        d_states = ss.dev(core, (size_t)S * n);
        d_off = ss.dev(core, sizeof(uint32_t) * (B + 1));
        d_pos = ss.dev(core, sizeof(uint64_t) * (B + 1));
        d_cw = ss.dev(core, cap);
        frames.resize((size_t)B * n); bytes.resize(cap); states.resize((size_t)S * n);
        off.resize(B + 1); pos.resize(B + 1);
        return ss.ok() ? 0 : 1;
    }
    // one tick (mi355_diff_multi_cwire_batch), or a burst of nb ticks, camera s's nb records one contiguous slice
    int step(int nb, bool burst) {
        const int nrec = S * nb;
        OK(mi355_upload(core, d_frames, frames.data(), (size_t)nrec * n));
        if (!burst) OK(mi355_diff_multi_cwire_batch(core, d_frames, d_states, n, S, d_off, d_pos, d_cw, cap));
        else OK(mi355_diff_multi_stream_cwire_batch(core, d_frames, d_states, n, S, nb, d_off, d_pos, d_cw, cap));
        OK(mi355_download(core, off.data(), d_off, sizeof(uint32_t) * (nrec + 1)));
        OK(mi355_download(core, pos.data(), d_pos, sizeof(uint64_t) * (nrec + 1)));
        if (pos[nrec] > cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
        cb = (size_t)pos[nrec];
        OK(mi355_download(core, bytes.data(), d_cw, cb));
        changed += off[nrec];
        return 0;
    }
    int get_states() {
        OK(mi355_download(core, states.data(), d_states, states.size()));
        return 0;
    }
};

// A node that receives records: a core, the bytes as they came (rx, and d_rx for their upload), the headers its walk found
// and, unless it is a relay that holds no frame, S camera states.
struct Receiver {
    mi355_core *core = nullptr;
    int S = 0;
    size_t n = 0, cap = 0;
    void *d_rx = nullptr, *d_states = nullptr;
    std::vector<uint8_t> rx, states;
    std::vector<uint32_t> counts, escapes;
    std::vector<size_t> at;

    int open(Session &ss, int S_, int max_batch, int most, bool holds_states = true) {   // most: records in one upload
        S = S_; n = ss.n; cap = mi355_cwire_bytes_max(n, most);
        core = ss.core(max_batch);
        d_rx = ss.dev(core, cap);
        if (holds_states) d_states = ss.dev(core, (size_t)S * n);
        rx.resize(cap); states.resize(holds_states ? (size_t)S * n : 0);
        counts.resize(most); escapes.resize(most); at.resize(most + 1);
        return ss.ok() ? 0 : 1;
    }
    // records first .. first + nrec - 1 lie in rx[from, to)
    int walk(size_t from, size_t to, int first, int nrec) {
        return walk_records(rx.data(), from, to, nrec, &counts[first], &escapes[first], &at[first]);
    }
    // Tick k of a burst of nb that was received stream-major (burst, b_at): record (s, k) of every camera s back to back in rx,
    // walked.  drop >= 0: that camera's record is lost, an empty record stands in its place.  Returns the bytes staged.
    size_t stage(const uint8_t *burst, const size_t *b_at, int nb, int k, int drop) {
        size_t q = 0;
        for (int s = 0; s < S; s++) {
            const int r = s * nb + k;
            const size_t len = s == drop ? 8 : b_at[r + 1] - b_at[r];
            if (s == drop) memset(rx.data() + q, 0, 8);
            else memcpy(rx.data() + q, burst + b_at[r], len);
            memcpy(&counts[s], rx.data() + q, 4);
            memcpy(&escapes[s], rx.data() + q + 4, 4);
            at[s] = q;
            q += len;
        }
        at[S] = q;
        return q;
    }
    // one tick's S records, uploaded to d_rx, onto the states: one call
    int apply_tick() {
        OK(mi355_apply_multi_cwire_batch(core, d_rx, counts.data(), escapes.data(), S, d_states, n));
        return 0;
    }
    int get_states() {
        OK(mi355_download(core, states.data(), d_states, states.size()));
        return 0;
    }
};

// the states at both ends (the receiver's as get_states() left them) are equal
static int states_equal(Sender &tx, const Receiver &rcv, int t) {
    if (tx.get_states()) return 1;
    return same(tx.states.data(), rcv.states.data(), tx.states.size(), "receiver states != sender states", t);
}

// S synthetic cameras: their base frames and, tick by tick, their frames
struct Cameras {
    int S, w, h;
    size_t n;
    std::vector<uint8_t> bases, base, frame;

    Cameras(int S_, int w_, int h_) : S(S_), w(w_), h(h_), n((size_t)3 * w_ * h_), bases((size_t)S_ * n), base(n), frame(n) {
        for (int s = 0; s < S; s++)
            for (size_t i = 0; i < n; i++) bases[(size_t)s * n + i] = (uint8_t)(40 + (i * 7 + (size_t)s * 31) % 150);
    }
    // the frames of ticks t0 .. t0 + nb - 1, stream-major: camera s's nb frames one behind the other, its own base, its block a
    // few steps ahead of its neighbour's
    void fill(uint8_t *frames, int t0, int nb) {
        for (int s = 0; s < S; s++) {
            memcpy(base.data(), &bases[(size_t)s * n], n);
            for (int k = 0; k < nb; k++) {
                make_frame(frame, base, w, h, t0 + k + 5 * s);
                memcpy(frames + ((size_t)s * nb + k) * n, frame.data(), n);
            }
        }
    }
    // every camera's base frame: the sender's states, and through the pipe the receiver's (opencv.cpp:38-46 per camera)
    int start(Session &ss, Sender &tx, Receiver &rcv, uint8_t *host_copy) {
        OK(mi355_upload(tx.core, tx.d_states, bases.data(), bases.size()));
        if (!ss.send(bases.data(), host_copy, bases.size())) return 1;
        OK(mi355_upload(rcv.core, rcv.d_states, host_copy, bases.size()));
        return 0;
    }
};

// The sockets of a burst into a node that keeps the slices as they came (a burst client, a relay): camera s's nb records,
// [pos[s * nb], pos[(s + 1) * nb]), are one write; the node reads their headers behind those of camera s - 1 and uploads the
// slice where it lies, stream-major, nothing re-staged.  A host client of camera s beside it applies the records one by one
// (host_shown, if given: the frame it shows after each).
static int slices_to_node(Session &ss, const Sender &tx, Receiver &node, int nb, uint8_t *host_frames, uint8_t *host_shown,
                          bool last_hop = false /* the node is the receiver: with --runs this socket is the link */) {
    const size_t n = tx.n;
    for (int s = 0; s < tx.S; s++) {
        const size_t a = (size_t)tx.pos[(size_t)s * nb], b = (size_t)tx.pos[(size_t)(s + 1) * nb];
        if (!(last_hop ? ss.send_records(tx.bytes.data() + a, node.rx.data() + a, b - a, nb) : ss.send(tx.bytes.data() + a, node.rx.data() + a, b - a)))
            return 1;
        if (node.walk(a, b, s * nb, nb)) return 1;
        for (int r = s * nb; r < (s + 1) * nb; r++) {
            if (host_apply(host_frames + (size_t)s * n, n, node.rx.data(), node.at.data(), r)) return 1;
            if (host_shown) memcpy(host_shown + (size_t)r * n, host_frames + (size_t)s * n, n);
        }
        if (b > a) OK(mi355_upload(node.core, (uint8_t *)node.d_rx + a, node.rx.data() + a, b - a));
    }
    return 0;
}

// --compact --multi S --activity CELL [--burst K --burst-client]: after every tick (or burst) the receiver also asks where its
// cameras move: mi355_cwire_activity_batch on the records it is about to apply, square cells of CELL pixels -> a grid of changed
// bytes per cell and eight summary words per camera.  Checked against a plain C++ count over records decoded here; the box and the
// active cells of every camera's last tick (or burst) are printed.
struct ActivityCheck {
    mi355_core *core = nullptr;
    int w = 0, h = 0, cell = 0, S = 0, gw = 0, gh = 0, calls = 0;
    size_t cells = 0;
    void *d_cells = nullptr, *d_summary = nullptr;
    std::vector<uint32_t> got_cells, got_sum, want_cells, want_sum;

    int open(Session &ss, mi355_core *c, int cell_, int S_) {   // cell_ == 0: not asked for
        if (!cell_) return 0;
        core = c; w = ss.w; h = ss.h; cell = cell_; S = S_;
        cells = mi355_activity_cells(w, h, cell, cell, &gw, &gh);
        if (!cells) { fprintf(stderr, "--activity CELL needs CELL >= 1\n"); return 2; }
        d_cells = ss.dev(core, sizeof(uint32_t) * cells * S);
        d_summary = ss.dev(core, sizeof(uint32_t) * 8 * S);
        if (!ss.ok()) return 1;
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
};

// --compact --multi S --check [--burst K --burst-client]: the receiver trusts nothing it has not checked: before it applies a tick
// (or burst) it asks mi355_cwire_check_batch for a verdict per record and requires every record well-formed and canonical (word
// 0 == 0), the verdicts equal to mi355_cwire_check_host's on the received bytes, and word 3 of every record equal to 1 + the
// last byte index that the apply then changes.  Once per run it also checks a damaged copy of the first non-empty record -- one
// code byte set to 255 -- and requires MI355_CWIRE_BAD_CODES.
struct RecordCheck {
    mi355_core *core = nullptr;
    bool on = false, damaged_done = false;
    size_t n = 0;
    int records = 0;
    void *d_verdicts = nullptr, *d_damaged = nullptr;
    std::vector<uint32_t> got, want;

    int open(Session &ss, mi355_core *c, bool on_, int most) {
        if (!on_) return 0;
        core = c; n = ss.n; on = true;
        d_verdicts = ss.dev(core, sizeof(uint32_t) * 4 * most);
        d_damaged = ss.dev(core, mi355_cwire_bytes_max(n, 1));
        if (!ss.ok()) return 1;
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
        return 0;
    }
};

// pixel (u, v) of the thumbnail at scale k of the w x h BGR24 frame st: the rounded mean of its block, in plain C++
static void box_average(const uint8_t *st, int w, int h, int k, int u, int v, uint8_t *bgr) {
    const int x0 = u * k, x1 = std::min(w, x0 + k), y0 = v * k, y1 = std::min(h, y0 + k);
    const uint32_t a = (uint32_t)((x1 - x0) * (y1 - y0));
    uint32_t sum[3] = {0, 0, 0};
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++)
            for (int c = 0; c < 3; c++) sum[c] += st[3 * ((size_t)y * w + x) + c];
    for (int c = 0; c < 3; c++) bgr[c] = (uint8_t)((sum[c] + a / 2) / a);
}

// --compact --multi S --wall K [--burst B --burst-client | --resync R [--burst B]]: the receiver is a wall that shows its cameras.  It
// keeps ONE wall frame of ceil(sqrt(S)) columns of thumbnails at scale K, composed fully once (mi355_wall_compose_batch without
// a mask).  After every tick's apply -- with --burst B --burst-client after every burst's -- it asks which tiles the records it just
// applied land in (mi355_cwire_touched_tiles_batch) and repaints the wall there (mi355_wall_compose_batch with that mask), the
// three calls with no wait in between.  With --resync R the refresh's own mask goes through the same masked compose behind the
// clear and the apply.  After every tick or burst, and after the refresh, the wall must equal a plain C++ box average of the
// receiver's states, and the wall's bytes outside the thumbnails the pattern they started as.
struct WallCheck {
    mi355_core *core = nullptr;
    int w = 0, h = 0, k = 0, S = 0, tw = 0, th = 0, cols = 0, wall_w = 0, wall_h = 0, composes = 0, compared = 0;
    size_t pitch = 0, mask_bytes = 0;
    void *d_wall = nullptr, *d_mask = nullptr;
    std::vector<int32_t> place;
    std::vector<uint8_t> got, want;
    enum : uint8_t { kPattern = 0x5C };     // what the wall holds outside the thumbnails (and in its pitch gap), from start to end

    int open(Session &ss, mi355_core *c, int k_, int S_) {   // k_ == 0: not asked for
        if (!k_) return 0;
        if (!mi355_wall_thumb_size(ss.w, ss.h, k_, &tw, &th)) { fprintf(stderr, "--wall K needs 1 <= K <= 16\n"); return 2; }
        core = c; w = ss.w; h = ss.h; k = k_; S = S_;
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
        d_wall = ss.dev(core, got.size());
        d_mask = ss.dev(core, mask_bytes);
        if (!ss.ok()) return 1;
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
                for (int u = 0; u < tw; u++)
                    box_average(st, w, h, k, u, v, &want[(size_t)(place[3 * s + 1] + v) * pitch + 3 * (size_t)(place[3 * s] + u)]);
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
        return 0;
    }
};

// --compact --multi S: many cameras per GPU, both ends.  A server core runs T ticks of S synthetic cameras through
// mi355_diff_multi_cwire_batch; each tick's records (headers included) cross the pipe; a client core uploads them and applies
// them in one call (mi355_apply_multi_cwire_batch) onto S states of its own.  After every tick the client's states must equal
// the server's, byte for byte, and the frames a host client (mi355_cwire_apply_host) rebuilt per camera.
// --compact --multi S --burst K --burst-client (K > 0 here): the sender makes the S * K records of K ticks in ONE call
// (run_multi_burst says how); the receiver uploads every camera's slice as it came off its socket, stream-major and not
// re-staged, and applies the whole burst with ONE mi355_apply_multi_stream_cwire_batch into output frames.  After every burst
// the states at both ends must be equal, and every output frame the frame a host client rebuilt for that camera and tick.
static int run_multi(int w, int h, int T, int S, int K, int activity, bool check, int wall_k) {
    const bool burst = K > 0;
    if (!burst) K = 1;
    Session ss(w, h);
    const size_t n = ss.n;
    const int B = S * K;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver rcv;
    ActivityCheck act;
    RecordCheck chk;
    WallCheck wall;
    if (tx.open(ss, S, K) || rcv.open(ss, S, B, B)) return 1;
    void *d_shown = burst ? ss.dev(rcv.core, (size_t)B * n) : nullptr;
    if (!ss.ok()) return 1;
    if (int rc = act.open(ss, rcv.core, activity, S)) return rc;
    if (int rc = chk.open(ss, rcv.core, check, B)) return rc;
    if (int rc = wall.open(ss, rcv.core, wall_k, S)) return rc;
    // a host client per camera beside the receiver, and what it shows after every record of a burst
    std::vector<uint8_t> host_frames((size_t)S * n), host_shown((size_t)B * n), shown(burst ? (size_t)B * n : 0);
    if (cams.start(ss, tx, rcv, host_frames.data())) return 1;
    if (int rc = wall.full(rcv.d_states)) return rc;
    std::vector<uint8_t> before(check ? host_frames : std::vector<uint8_t>());   // (the states a tick or burst finds)
    const uint32_t *counts = rcv.counts.data(), *escapes = rcv.escapes.data();
    size_t sent_bytes = 0;
    int max_err = 0, calls = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K, nrec = S * nb, t = t0 + nb - 1;
        cams.fill(tx.frames.data(), t0, nb);
        // ---- server: one tick -> S records, or nb ticks -> S * nb records, in one call
        if (tx.step(nb, burst)) return 1;
        calls++;
        // ---- the sockets, the headers as read from the stream, the upload; the host clients beside it.  A tick: one pipe here,
        // the receiver stages the cameras' records back to back.  A burst: a slice per camera.
        if (burst) {
            if (slices_to_node(ss, tx, rcv, nb, host_frames.data(), host_shown.data(), true)) return 1;
        } else {
            if (!ss.send_records(tx.bytes.data(), rcv.rx.data(), tx.cb, S) || rcv.walk(0, tx.cb, 0, S)) return 1;
            for (int s = 0; s < S; s++)
                if (host_apply(&host_frames[(size_t)s * n], n, rcv.rx.data(), rcv.at.data(), s)) return 1;
            host_shown = host_frames;
            OK(mi355_upload(rcv.core, rcv.d_rx, rcv.rx.data(), tx.cb));
        }
        sent_bytes += tx.cb;
        if (int rc = act.run(rcv.d_rx, rcv.rx.data(), counts, escapes, nb, t0)) return rc;
        if (int rc = chk.run(rcv.d_rx, rcv.rx.data(), tx.cb, counts, escapes, nrec, t0)) return rc;
        // ---- client: one call; of a burst, every frame in between into d_shown
        if (burst) OK(mi355_apply_multi_stream_cwire_batch(rcv.core, rcv.d_rx, counts, escapes, S, nb, rcv.d_states, n, d_shown, n));
        else if (rcv.apply_tick()) return 1;
        if (int rc = wall.update(rcv.d_rx, counts, escapes, nb, rcv.d_states)) return rc;
        // ---- checks; `after`: the frame behind every record (of a tick, the states themselves)
        if (rcv.get_states()) return 1;
        if (int rc = wall.compare(rcv.states.data(), t)) return rc;
        if (burst) OK(mi355_download(rcv.core, shown.data(), d_shown, (size_t)nrec * n));
        const uint8_t *after = burst ? shown.data() : rcv.states.data();
        for (int r = 0; r < nrec && check; r++)   // record (s, k) turned the frame after record (s, k - 1) into its own
            if (int rc = chk.applied(r, r % nb ? after + (size_t)(r - 1) * n : &before[(size_t)(r / nb) * n], after + (size_t)r * n, t0)) return rc;
        if (check) before = rcv.states;
        if (states_equal(tx, rcv, t0)) return 1;
        for (int r = 0; r < nrec; r++)
            if (memcmp(after + (size_t)r * n, &host_shown[(size_t)r * n], n) != 0) {
                fprintf(stderr, "tick %d: camera %d: GPU client frame != host client frame\n", t0 + r % nb, r / nb);
                return 1;
            }
        max_err = std::max(max_err, max_abs_error(after, tx.frames.data(), (size_t)nrec * n));
    }
    if (within_threshold(max_err, ss)) return 1;
    if (int rc = chk.close()) return rc;
    if (int rc = wall.close()) return rc;
    if (ss.close()) return 1;
    const size_t changed = tx.changed, ref_bytes = mi355_wire_bytes(T * S, changed), raw = (size_t)T * S * n;
    const std::string checks = act.json() + chk.json() + wall.json();
    if (burst)
        printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"burst_client\": true, \"sender_calls\": %d, "
               "\"receiver_calls\": %d, \"width\": %d, \"height\": %d, \"ticks\": %d, \"changed_bytes\": %zu, \"wire_bytes\": %zu, "
               "\"reference_wire_bytes\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d%s}\n",
               S, K, calls, calls, w, h, T, changed, sent_bytes, ref_bytes, raw, max_err, checks.c_str());
    else
        printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"width\": %d, \"height\": %d, \"ticks\": %d, "
               "\"changed_bytes\": %zu, \"wire_bytes\": %zu, \"reference_wire_bytes\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d%s}\n",
               S, w, h, T, changed, sent_bytes, ref_bytes, raw, max_err, checks.c_str());
    return 0;
}

// --compact --multi S --budget BYTES: the sender holds every camera's record of a tick to BYTES bytes (a socket's share of the
// link): the records larger than that are thinned to mi355_cwire_budget_entries(N, BYTES) entries by
// mi355_cwire_budget_cwire_batch, which takes the sender's states back where it drops an entry.  Checked: every record written is
// at most BYTES; each client's frame equals the sender's state after every tick; and once the input has stood still for enough
// ticks every client's frame is within the threshold of the camera's frame at every byte -- what was postponed arrives.
static int run_multi_budget(int w, int h, int T, int S, long bytes) {
    const size_t n = (size_t)3 * w * h;
    const size_t most = bytes >= 0 ? mi355_cwire_budget_entries(n, (size_t)bytes) : 0;
    if (most == 0) { fprintf(stderr, "--budget %ld holds no entry of a %dx%d frame\n", bytes, w, h); return 2; }
    Session ss(w, h);
    Cameras cams(S, w, h);
    Sender tx;
    Receiver rcv;
    if (tx.open(ss, S, 1) || rcv.open(ss, S, S, S)) return 1;
    void *d_thr = ss.dev(tx.core, sizeof(uint32_t) * S), *d_ooff = ss.dev(tx.core, sizeof(uint32_t) * (S + 1));
    void *d_opos = ss.dev(tx.core, sizeof(uint64_t) * (S + 1)), *d_out = ss.dev(tx.core, tx.cap);
    if (!ss.ok()) return 1;
    if (cams.start(ss, tx, rcv, rcv.states.data())) return 1;
    std::vector<uint32_t> counts(S), escapes(S), budget(S), thr(S);
    std::vector<uint64_t> pos(S + 1);
    size_t sent_bytes = 0, largest = 0;
    int thinned = 0, max_thr = ss.threshold, max_err = 0, still = 0;
    // T ticks of moving input, then the last frames again and again until nothing is held back any more: what a budget
    // postponed must arrive.  A tick sends up to `most` of a camera's pending entries, so N / most still ticks suffice -- unless
    // more than `most` of them share one magnitude (then no threshold separates them; the synthetic input has no such group).
    const int still_limit = (int)(2 * ((n + most - 1) / most)) + 2;
    for (int t = 0;; t++) {
        if (t < T) cams.fill(tx.frames.data(), t, 1);
        // ---- server: one tick -> S records, their headers, the records above the budget thinned
        if (tx.step(1, false)) return 1;
        bool over = false;
        for (int s = 0; s < S; s++) {
            memcpy(&counts[s], &tx.bytes[tx.pos[s]], 4);
            memcpy(&escapes[s], &tx.bytes[tx.pos[s] + 4], 4);
            budget[s] = tx.pos[s + 1] - tx.pos[s] > (uint64_t)bytes ? (uint32_t)most : UINT32_MAX;
            if (budget[s] != UINT32_MAX) { over = true; thinned++; }
        }
        OK(mi355_cwire_budget_cwire_batch(tx.core, tx.d_cw, counts.data(), escapes.data(), tx.d_states, n, S, budget.data(), d_thr, d_ooff,
                                          d_opos, d_out, tx.cap));
        OK(mi355_download(tx.core, pos.data(), d_opos, sizeof(uint64_t) * (S + 1)));
        OK(mi355_download(tx.core, thr.data(), d_thr, sizeof(uint32_t) * S));
        if (pos[S] > tx.cap) { fprintf(stderr, "thinned stream larger than its bound\n"); return 1; }
        for (int s = 0; s < S; s++) {   // check 1: every record that is written fits the socket's budget
            const size_t rb = (size_t)(pos[s + 1] - pos[s]);
            if (rb > (size_t)bytes) { fprintf(stderr, "tick %d: camera %d's record has %zu bytes > %ld\n", t, s, rb, bytes); return 1; }
            if (rb > largest) largest = rb;
            if ((int)thr[s] > max_thr) max_thr = (int)thr[s];
            if ((budget[s] == UINT32_MAX) != ((int)thr[s] == ss.threshold)) { fprintf(stderr, "tick %d: camera %d: threshold %u\n", t, s, thr[s]); return 1; }
        }
        const size_t cb = (size_t)pos[S];
        OK(mi355_download(tx.core, tx.bytes.data(), d_out, cb));
        if (!ss.send(tx.bytes.data(), rcv.rx.data(), cb)) return 1;
        sent_bytes += cb;
        // ---- client: the headers as read from the stream, one upload, one call
        if (rcv.walk(0, cb, 0, S)) return 1;
        OK(mi355_upload(rcv.core, rcv.d_rx, rcv.rx.data(), cb));
        if (rcv.apply_tick()) return 1;
        // ---- check 2: each client's frame equals the sender's state after every tick
        if (rcv.get_states() || states_equal(tx, rcv, t)) return 1;
        if (t + 1 < T) continue;
        // ---- check 3, once the input stands still: every client's frame within the threshold of the camera's, at every byte
        max_err = max_abs_error(rcv.states.data(), tx.frames.data(), (size_t)S * n);
        if (t >= T && !over && max_err <= ss.threshold) break;
        if (t >= T) still++;
        if (still > still_limit) { fprintf(stderr, "held still for %d ticks and still off by %d > threshold\n", still, max_err); return 1; }
    }
    if (ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"budget_bytes\": %ld, \"budget_entries\": %zu, \"width\": %d, "
           "\"height\": %d, \"ticks\": %d, \"still_ticks\": %d, \"thinned_records\": %d, \"largest_record_bytes\": %zu, "
           "\"largest_threshold\": %d, \"records_within_budget\": true, \"states_equal_every_tick\": true, "
           "\"max_abs_error_when_still\": %d, \"wire_bytes\": %zu}\n",
           S, bytes, most, w, h, T, still + 1, thinned, largest, max_thr, max_err, sent_bytes);
    return 0;
}

// the byte indices of the entries with a nonzero difference of the well-formed record {n, e} at rec
static void record_indices(const uint8_t *rec, uint32_t n, uint32_t e, std::vector<uint32_t> *xs) {
    const size_t pad = ((size_t)n + 3) & ~(size_t)3;
    const uint8_t *code = rec + 8, *esc = code + pad, *diff = esc + 4 * (size_t)e;
    uint64_t x = 0;
    xs->clear();
    for (uint32_t k = 0, r = 0; k < n; k++) {
        uint32_t g = code[k];
        if (g == 255) memcpy(&g, esc + 4 * (size_t)r++, 4);
        x += (uint64_t)g + 1;
        if (diff[k]) xs->push_back((uint32_t)(x - 1));
    }
}

// --compact --multi S --despeckle NEED: the sender drops every camera's isolated changes before it sends a tick
// (mi355_cwire_despeckle_cwire_batch, need = NEED for every camera), which takes its states back where it drops an entry; a host
// client per camera applies what arrives.  Checked every tick: each client's frame equals the sender's state; records, counts and
// states equal mi355_cwire_despeckle_host on a host copy of the tick; every sent entry's pixel has at least NEED changed pixels
// among the 8 around it, by a plain count over the tick's own record.  After the moving input the last frames are repeated: what
// was dropped is found again and dropped again, nothing is sent and the states stand still.
static int run_multi_despeckle(int w, int h, int T, int S, long need_arg) {
    Session ss(w, h);
    const size_t n = ss.n;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver rcv;
    if (tx.open(ss, S, 1) || rcv.open(ss, S, S, S)) return 1;
    void *d_drop = ss.dev(tx.core, sizeof(uint32_t) * S), *d_ooff = ss.dev(tx.core, sizeof(uint32_t) * (S + 1));
    void *d_opos = ss.dev(tx.core, sizeof(uint64_t) * (S + 1)), *d_out = ss.dev(tx.core, tx.cap);
    if (!ss.ok()) return 1;
    OK(mi355_prepare(tx.core, MI355_PREPARE_DESPECKLE));
    if (cams.start(ss, tx, rcv, rcv.states.data())) return 1;
    std::vector<uint32_t> counts(S), escapes(S), need(S, (uint32_t)need_arg), dropped(S), h_dropped(S), h_off(S + 1), xs_in, xs_out;
    std::vector<uint64_t> pos(S + 1), h_pos(S + 1);
    std::vector<uint8_t> out(tx.cap), h_out(tx.cap), h_states, changed((size_t)w * h), before;
    size_t entries_in = 0, entries_out = 0, bytes_in = 0, bytes_out = 0, still_entries_out = 0;
    const int still_ticks = 2;
    for (int t = 0; t < T + still_ticks; t++) {
        if (t < T) cams.fill(tx.frames.data(), t, 1);
        // ---- server: one tick -> S records and their headers, then the records without their isolated changes
        if (tx.step(1, false)) return 1;
        for (int s = 0; s < S; s++) {
            memcpy(&counts[s], &tx.bytes[tx.pos[s]], 4);
            memcpy(&escapes[s], &tx.bytes[tx.pos[s] + 4], 4);
            entries_in += counts[s];
        }
        bytes_in += tx.cb;
        if (tx.get_states()) return 1;
        h_states = tx.states;   // (the host form's copy: the states as the diff left them)
        OK(mi355_cwire_despeckle_cwire_batch(tx.core, tx.d_cw, counts.data(), escapes.data(), tx.d_states, n, S, need.data(), d_drop, d_ooff,
                                             d_opos, d_out, tx.cap));
        OK(mi355_download(tx.core, pos.data(), d_opos, sizeof(uint64_t) * (S + 1)));
        OK(mi355_download(tx.core, dropped.data(), d_drop, sizeof(uint32_t) * S));
        if (pos[S] > tx.cap) { fprintf(stderr, "despeckled stream larger than its bound\n"); return 1; }
        const size_t cb = (size_t)pos[S];
        OK(mi355_download(tx.core, out.data(), d_out, cb));
        // ---- check 1: the host form on a host copy gives the same records, counts and states
        OK(mi355_cwire_despeckle_host(w, h, tx.bytes.data(), tx.cb, counts.data(), escapes.data(), h_states.data(), n, S, need.data(),
                                      h_dropped.data(), h_off.data(), h_pos.data(), h_out.data(), tx.cap));
        if (h_pos != pos || h_dropped != dropped || memcmp(h_out.data(), out.data(), cb) != 0) {
            fprintf(stderr, "tick %d: the records differ from mi355_cwire_despeckle_host's\n", t);
            return 1;
        }
        if (tx.get_states()) return 1;
        if (same(tx.states.data(), h_states.data(), h_states.size(), "sender states != mi355_cwire_despeckle_host's", t)) return 1;
        // ---- the pipe, the headers as read from the stream, a host client per camera
        if (!ss.send(out.data(), rcv.rx.data(), cb) || rcv.walk(0, cb, 0, S)) return 1;
        for (int s = 0; s < S; s++) {
            if (host_apply(&rcv.states[(size_t)s * n], n, rcv.rx.data(), rcv.at.data(), s)) return 1;
            // ---- check 2: every sent entry has at least NEED changed pixels around its pixel, by a plain count
            record_indices(&tx.bytes[tx.pos[s]], counts[s], escapes[s], &xs_in);
            record_indices(rcv.rx.data() + rcv.at[s], rcv.counts[s], rcv.escapes[s], &xs_out);
            std::fill(changed.begin(), changed.end(), 0);
            for (uint32_t x : xs_in) changed[x / 3] = 1;
            for (uint32_t x : xs_out) {
                const int p = (int)(x / 3), px = p % w, py = p / w;
                long c = 0;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++)
                        if ((dx || dy) && px + dx >= 0 && px + dx < w && py + dy >= 0 && py + dy < h) c += changed[(size_t)(py + dy) * w + px + dx];
                if (c < need_arg) { fprintf(stderr, "tick %d: camera %d: byte %u was sent with %ld changed neighbours\n", t, s, x, c); return 1; }
            }
            if (xs_in.size() != xs_out.size() + dropped[s]) { fprintf(stderr, "tick %d: camera %d: kept + dropped != entries\n", t, s); return 1; }
            (t < T ? entries_out : still_entries_out) += xs_out.size();
        }
        if (t < T) bytes_out += cb;
        // ---- check 3: each client's frame equals the sender's state after every tick
        if (same(tx.states.data(), rcv.states.data(), tx.states.size(), "receiver states != sender states", t)) return 1;
        // ---- check 4, once the input stands still: so do the states
        if (t >= T && same(tx.states.data(), before.data(), before.size(), "the states moved while the input stood still", t)) return 1;
        before = tx.states;
    }
    if (still_entries_out) { fprintf(stderr, "%zu entries were sent while the input stood still\n", still_entries_out); return 1; }
    if (ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"despeckle\": %ld, \"width\": %d, \"height\": %d, \"ticks\": %d, "
           "\"still_ticks\": %d, \"entries_in\": %zu, \"entries_out\": %zu, \"bytes_in\": %zu, \"bytes_out\": %zu, "
           "\"equals_host_form\": true, \"sent_entries_have_neighbours\": true, \"states_equal_every_tick\": true, "
           "\"states_stand_still\": true}\n",
           S, need_arg, w, h, T, still_ticks, entries_in, entries_out, bytes_in, bytes_out);
    return 0;
}

// --compact --multi S --burst K: the sender buffers K ticks per camera (a recorder, a camera that catches up) and makes their
// S * K records in ONE call, mi355_diff_multi_stream_cwire_batch: camera s's K records are one contiguous slice, one write()
// per socket.  The receiver stages record (s, t) of every s back to back for tick t and applies the ticks with the same
// mi355_apply_multi_cwire_batch; after every burst the states at both ends must be equal.
static int run_multi_burst(int w, int h, int T, int S, int K) {
    Session ss(w, h);
    const size_t n = ss.n;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver rcv;
    if (tx.open(ss, S, K) || rcv.open(ss, S, S, S)) return 1;
    std::vector<uint8_t> host_frames((size_t)S * n), burst(tx.cap);   // a host client per camera; the bytes as the sockets gave them
    std::vector<uint32_t> b_counts(S * K), b_escapes(S * K);
    std::vector<size_t> b_at(S * K + 1);   // where record (s, t) lies in them, as the receiver found it
    if (cams.start(ss, tx, rcv, host_frames.data())) return 1;
    size_t sent_bytes = 0;
    int max_err = 0, calls = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K;
        cams.fill(tx.frames.data(), t0, nb);
        // ---- server: nb ticks of S cameras -> S * nb records in one call
        if (tx.step(nb, true)) return 1;
        calls++;
        // ---- the sockets: camera s's slice [pos[s * nb], pos[(s + 1) * nb]) is one write
        for (int s = 0; s < S; s++) {
            const size_t a = (size_t)tx.pos[(size_t)s * nb], b = (size_t)tx.pos[(size_t)(s + 1) * nb];
            if (!ss.send_records(tx.bytes.data() + a, burst.data() + a, b - a, nb)) return 1;
        }
        sent_bytes += tx.cb;
        // ---- receiver: the records of every socket, found from their headers
        if (walk_records(burst.data(), 0, tx.cb, S * nb, b_counts.data(), b_escapes.data(), b_at.data())) return 1;
        // ---- client: tick k = record (s, k) of every s back to back (the host client of camera s beside it), one upload, one call
        for (int k = 0; k < nb; k++) {
            const size_t q = rcv.stage(burst.data(), b_at.data(), nb, k, -1);
            for (int s = 0; s < S; s++)
                if (host_apply(&host_frames[(size_t)s * n], n, rcv.rx.data(), rcv.at.data(), s)) return 1;
            OK(mi355_upload(rcv.core, rcv.d_rx, rcv.rx.data(), q));
            if (rcv.apply_tick() || rcv.get_states()) return 1;
            if (same(host_frames.data(), rcv.states.data(), rcv.states.size(), "receiver states != host client frames", t0 + k)) return 1;
            for (int s = 0; s < S; s++)
                max_err = std::max(max_err, max_abs_error(&rcv.states[(size_t)s * n], &tx.frames[((size_t)s * nb + k) * n], n));
        }
        // ---- the states at both ends
        if (states_equal(tx, rcv, t0)) return 1;
    }
    if (within_threshold(max_err, ss) || ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"sender_calls\": %d, \"width\": %d, \"height\": %d, "
           "\"ticks\": %d, \"changed_bytes\": %zu, \"wire_bytes\": %zu, \"reference_wire_bytes\": %zu, \"raw_bytes\": %zu, "
           "\"max_abs_error\": %d}\n",
           S, K, calls, w, h, T, tx.changed, sent_bytes, mi355_wire_bytes(T * S, tx.changed), (size_t)T * S * n, max_err);
    return 0;
}

// --compact --multi S --thumb K [--burst T] [--thumb-drop TICK]: the sender also serves a low-resolution viewer.  It holds, next
// to its S states, the S thumbnails at scale K that the viewer has reconstructed.  Behind every tick -- with --burst T behind every
// burst -- it asks which tiles its own records landed in (mi355_cwire_touched_tiles_batch) and makes ONE record per camera of the
// thumbnail's frame there (mi355_thumb_cwire_batch, threshold 0), the calls with no wait in between; camera s's thumbnail record
// goes through a second pipe of its own.  The viewer is host-only: S frames of tw x th pixels, mi355_cwire_apply_host.  It joins
// late: before the first tick the sender's held thumbnails and the viewer's frames are zero and one call without a mask makes
// the key records.  After every tick or burst the viewer must equal a plain C++ box average of the sender's downloaded states.
// The full-size receiver runs beside it as in --burst (tick by tick with T = 1).
// --thumb-drop TICK: the viewer discards camera TICK % S's thumbnail record of the step that holds that tick; its picture must
// then be wrong; the repair is the key-record procedure (the viewer clears that frame, the sender zeroes that held thumbnail, one
// call without a mask) and the pictures must be equal from then on.
struct ThumbViewer {
    mi355_core *core = nullptr;   // the sender's
    int w = 0, h = 0, k = 0, S = 0, tw = 0, th = 0, calls = 0, compared = 0;
    size_t nt = 0, cap = 0, sent = 0;
    void *d_thumbs = nullptr, *d_mask = nullptr, *d_off = nullptr, *d_pos = nullptr, *d_cw = nullptr;
    std::vector<int> fds;           // a pipe per camera
    std::vector<uint8_t> bytes, rx, frames, want;
    std::vector<uint32_t> counts, escapes;
    std::vector<uint64_t> pos;

    int open(Session &ss, const Sender &tx, int k_, int most) {   // most: the records of the sender's largest step
        if (!mi355_wall_thumb_size(ss.w, ss.h, k_, &tw, &th)) { fprintf(stderr, "--thumb K needs 1 <= K <= 16\n"); return 2; }
        core = tx.core; w = ss.w; h = ss.h; k = k_; S = tx.S;
        nt = (size_t)3 * tw * th;
        cap = mi355_cwire_bytes_max(nt, S);
        d_thumbs = ss.dev(core, (size_t)S * nt);
        d_mask = ss.dev(core, 4 * (size_t)S * ((mi355_state_tiles(ss.n) + 31) / 32));
        d_off = ss.dev(core, sizeof(uint32_t) * (S + 1));
        d_pos = ss.dev(core, sizeof(uint64_t) * (S + 1));
        d_cw = ss.dev(core, cap);
        if (!ss.ok()) return 1;
        fds.resize((size_t)2 * S);
        for (int s = 0; s < S; s++)
            if (pipe(&fds[(size_t)2 * s]) != 0) { fprintf(stderr, "pipe failed\n"); return 1; }
        bytes.resize(cap); rx.resize(cap); frames.assign((size_t)S * nt, 0); want.resize((size_t)S * nt);
        counts.resize(most); escapes.resize(most); pos.resize(S + 1);
        OK(mi355_upload(core, d_thumbs, frames.data(), frames.size()));   // nobody has seen anything yet
        return 0;
    }
    // the thumbnail records of the states as they are: where the nb records per camera of the sender's last step landed, or
    // (nb == 0) everywhere; every camera's record through its pipe and onto the viewer's frame, but camera `drop`'s, which is lost.
    // *lost: the entries of the lost record
    int serve(const Sender &tx, int nb, int drop, uint32_t *lost) {
        const void *mask = nullptr;
        if (nb) {
            if (walk_records(tx.bytes.data(), 0, tx.cb, S * nb, counts.data(), escapes.data(), nullptr)) return 1;
            OK(mi355_cwire_touched_tiles_batch(core, tx.d_cw, counts.data(), escapes.data(), S, nb, 0, d_mask));
            mask = d_mask;
        }
        OK(mi355_thumb_cwire_batch(core, tx.d_states, tx.n, S, k, 0, mask, d_thumbs, nt, d_off, d_pos, d_cw, cap));
        calls++;
        OK(mi355_download(core, pos.data(), d_pos, sizeof(uint64_t) * (S + 1)));
        if (pos[S] > cap) { fprintf(stderr, "thumbnail records larger than their bound\n"); return 1; }
        OK(mi355_download(core, bytes.data(), d_cw, (size_t)pos[S]));
        for (int s = 0; s < S; s++) {
            const size_t a = (size_t)pos[s], len = (size_t)pos[s + 1] - a;
            if (!Session::through(&fds[(size_t)2 * s], bytes.data() + a, rx.data() + a, len)) return 1;
            sent += len;
            if (s == drop) {
                memcpy(lost, rx.data() + a, 4);
                continue;
            }
            size_t used = 0;
            OK(mi355_cwire_apply_host(&frames[(size_t)s * nt], nt, rx.data() + a, len, 1, &used));
            if (used != len) { fprintf(stderr, "thumbnail stream framing broken\n"); return 1; }
        }
        return 0;
    }
    // the key-record procedure for camera s
    int rejoin(const Sender &tx, int s) {
        std::fill(frames.begin() + (size_t)s * nt, frames.begin() + (size_t)(s + 1) * nt, 0);
        OK(mi355_upload(core, (uint8_t *)d_thumbs + (size_t)s * nt, &frames[(size_t)s * nt], nt));
        return serve(tx, 0, -1, nullptr);
    }
    // the box average of the sender's states (S frames back to back) -> want; true: the viewer's camera s shows it
    void average(const uint8_t *states) {
        for (int s = 0; s < S; s++)
            for (int v = 0; v < th; v++)
                for (int u = 0; u < tw; u++)
                    box_average(states + (size_t)s * 3 * w * h, w, h, k, u, v, &want[(size_t)s * nt + 3 * ((size_t)v * tw + u)]);
    }
    bool shows(int s) const { return memcmp(&frames[(size_t)s * nt], &want[(size_t)s * nt], nt) == 0; }
    int compare(const uint8_t *states, int t) {
        average(states);
        for (int s = 0; s < S; s++)
            if (!shows(s)) { fprintf(stderr, "tick %d: camera %d: the viewer != the box average of the sender's state\n", t, s); return 1; }
        compared++;
        return 0;
    }
};

static int run_multi_thumb(int w, int h, int T, int S, int K, int k, int drop_tick) {
    const bool burst = K > 0;
    if (!burst) K = 1;
    Session ss(w, h);
    const size_t n = ss.n;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver rcv;
    ThumbViewer view;
    if (tx.open(ss, S, K) || rcv.open(ss, S, S, S)) return 1;
    if (int rc = view.open(ss, tx, k, S * K)) return rc;
    std::vector<uint8_t> host_frames((size_t)S * n), sock(tx.cap);   // a host client per camera; the bytes as the sockets gave them
    std::vector<uint32_t> b_counts(S * K), b_escapes(S * K);
    std::vector<size_t> b_at(S * K + 1);
    if (cams.start(ss, tx, rcv, host_frames.data())) return 1;
    // ---- the viewer joins: key records of the thumbnails of the base frames
    if (view.serve(tx, 0, -1, nullptr) || tx.get_states() || view.compare(tx.states.data(), -1)) return 1;
    size_t sent_bytes = 0;
    int max_err = 0, repaired = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K;
        cams.fill(tx.frames.data(), t0, nb);
        if (tx.step(nb, burst)) return 1;
        // ---- the low-resolution viewer: touched tiles of the step's records, the thumbnails' records, a pipe per camera
        const bool dropping = drop_tick >= t0 && drop_tick < t0 + nb;
        const int drop = dropping ? drop_tick % S : -1;
        uint32_t lost = 0;
        if (view.serve(tx, nb, drop, &lost) || tx.get_states()) return 1;
        if (dropping) {
            if (!lost) { fprintf(stderr, "--thumb-drop: the record to drop holds no entry\n"); return 1; }
            view.average(tx.states.data());
            if (view.shows(drop)) { fprintf(stderr, "--thumb-drop: the picture is right without its record\n"); return 1; }
            if (view.rejoin(tx, drop)) return 1;
            repaired++;
        }
        if (view.compare(tx.states.data(), t0 + nb - 1)) return 1;
        // ---- the full-size receiver beside it: every socket's records, staged and applied tick by tick
        for (int s = 0; s < S; s++) {
            const size_t a = (size_t)tx.pos[(size_t)s * nb], b = (size_t)tx.pos[(size_t)(s + 1) * nb];
            if (!ss.send(tx.bytes.data() + a, sock.data() + a, b - a)) return 1;
        }
        sent_bytes += tx.cb;
        if (walk_records(sock.data(), 0, tx.cb, S * nb, b_counts.data(), b_escapes.data(), b_at.data())) return 1;
        for (int j = 0; j < nb; j++) {
            const size_t q = rcv.stage(sock.data(), b_at.data(), nb, j, -1);
            for (int s = 0; s < S; s++)
                if (host_apply(&host_frames[(size_t)s * n], n, rcv.rx.data(), rcv.at.data(), s)) return 1;
            OK(mi355_upload(rcv.core, rcv.d_rx, rcv.rx.data(), q));
            if (rcv.apply_tick() || rcv.get_states()) return 1;
            if (same(host_frames.data(), rcv.states.data(), rcv.states.size(), "receiver states != host client frames", t0 + j)) return 1;
            for (int s = 0; s < S; s++)
                max_err = std::max(max_err, max_abs_error(&rcv.states[(size_t)s * n], &tx.frames[((size_t)s * nb + j) * n], n));
        }
        if (states_equal(tx, rcv, t0)) return 1;
    }
    if (drop_tick >= 0 && !repaired) { fprintf(stderr, "--thumb-drop TICK needs 0 <= TICK < --frames\n"); return 2; }
    if (within_threshold(max_err, ss) || ss.close()) return 1;
    for (int fd : view.fds) close(fd);
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"width\": %d, \"height\": %d, \"ticks\": %d, "
           "\"changed_bytes\": %zu, \"wire_bytes\": %zu, \"max_abs_error\": %d, \"thumb\": {\"scale\": %d, \"size\": [%d, %d], "
           "\"calls\": %d, \"wire_bytes\": %zu, \"viewers_equal\": %d, \"repaired\": %d}}\n",
           S, burst ? K : 0, w, h, T, tx.changed, sent_bytes, max_err, k, view.tw, view.th, view.calls, view.sent, view.compared, repaired);
    return 0;
}

// --compact --multi S --burst K --coalesce: a relay between the two ends that forwards at 1/K of the rate (a slow link, a
// time-lapse recorder, a video wall).  It holds no frame: it uploads every camera's slice as it came off its socket, makes
// ONE record per camera of the burst with mi355_cwire_coalesce_cwire_batch, and forwards those S records; the receiver applies
// them with one mi355_apply_multi_cwire_batch.  After every burst each camera's state at the receiver must equal the frame of
// a host client (mi355_cwire_apply_host) that applied all K original records, and the sender's state.  The line also says how
// many bytes the relay received and how many it forwarded.
static int run_multi_burst_coalesce(int w, int h, int T, int S, int K) {
    Session ss(w, h);
    const size_t n = ss.n;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver relay, rcv;
    if (tx.open(ss, S, K) || relay.open(ss, S, S * K, S * K, false) || rcv.open(ss, S, S, S)) return 1;
    void *d_roff = ss.dev(relay.core, sizeof(uint32_t) * (S + 1)), *d_rpos = ss.dev(relay.core, sizeof(uint64_t) * (S + 1));
    void *d_fwd = ss.dev(relay.core, rcv.cap);
    if (!ss.ok()) return 1;
    std::vector<uint8_t> host_frames((size_t)S * n), fwd(rcv.cap);
    std::vector<uint32_t> roff(S + 1);
    std::vector<uint64_t> rpos(S + 1);
    if (cams.start(ss, tx, rcv, host_frames.data())) return 1;
    size_t received = 0, forwarded = 0, kept = 0;
    int max_err = 0, calls = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K;
        cams.fill(tx.frames.data(), t0, nb);
        // ---- server: nb ticks of S cameras -> S * nb records in one call
        if (tx.step(nb, true)) return 1;
        // ---- the sockets into the relay; a host client beside it applies all nb original records of every camera
        if (slices_to_node(ss, tx, relay, nb, host_frames.data(), nullptr)) return 1;
        received += tx.cb;
        // ---- relay: the burst -> one record per camera, in one call; no frame exists here
        OK(mi355_cwire_coalesce_cwire_batch(relay.core, relay.d_rx, relay.counts.data(), relay.escapes.data(), S, nb, d_roff, d_rpos,
                                            d_fwd, rcv.cap));
        calls++;
        OK(mi355_download(relay.core, roff.data(), d_roff, sizeof(uint32_t) * (S + 1)));
        OK(mi355_download(relay.core, rpos.data(), d_rpos, sizeof(uint64_t) * (S + 1)));
        if (rpos[S] > rcv.cap) { fprintf(stderr, "coalesced stream larger than its bound\n"); return 1; }
        const size_t fb = (size_t)rpos[S];
        OK(mi355_download(relay.core, fwd.data(), d_fwd, fb));
        kept += roff[S];
        // ---- the sockets out of the relay, one record per camera; the receiver finds them from their headers
        if (!ss.send_records(fwd.data(), rcv.rx.data(), fb, S)) return 1;
        forwarded += fb;
        if (rcv.walk(0, fb, 0, S)) return 1;
        // ---- receiver: one call per burst
        OK(mi355_upload(rcv.core, rcv.d_rx, rcv.rx.data(), fb));
        if (rcv.apply_tick() || rcv.get_states()) return 1;
        // ---- checks
        for (int s = 0; s < S; s++)
            if (memcmp(&host_frames[(size_t)s * n], &rcv.states[(size_t)s * n], n) != 0) {
                fprintf(stderr, "tick %d: camera %d: receiver state != host client that applied all %d records\n", t0, s, nb);
                return 1;
            }
        if (states_equal(tx, rcv, t0)) return 1;
        for (int s = 0; s < S; s++)
            max_err = std::max(max_err, max_abs_error(&rcv.states[(size_t)s * n], &tx.frames[((size_t)s * nb + nb - 1) * n], n));
    }
    if (within_threshold(max_err, ss) || ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"coalesce\": true, \"relay_calls\": %d, "
           "\"width\": %d, \"height\": %d, \"ticks\": %d, \"changed_bytes\": %zu, \"coalesced_entries\": %zu, "
           "\"relay_received_bytes\": %zu, \"relay_forwarded_bytes\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d}\n",
           S, K, calls, w, h, T, tx.changed, kept, received, forwarded, (size_t)T * S * n, max_err);
    return 0;
}

// --compact --multi S [--burst K --coalesce] --datagram BYTES: a relay in front of a datagram socket (UDP, RTP, QUIC datagrams,
// multicast).  It holds no frame: it uploads every camera's records as they came off its socket -- one tick, or with --burst K
// --coalesce a burst that it first coalesces into one record per camera -- and cuts them into pieces of at most BYTES bytes with
// ONE mi355_cwire_split_cwire_batch.  Every piece is one datagram (one write, one read).  The receiver needs nothing new: pieces
// are records.  It stages each camera's pieces in a shuffled order (the tool's seeded generator), padded with n = 0 records to a
// common count, and applies them with mi355_apply_multi_stream_cwire_batch, kDatagramRound pieces of every camera per call.
// After every tick each camera's state at the receiver must equal the frame of a host client (mi355_cwire_apply_host) that applied
// the original records, and the sender's state.  The line also says how many pieces and bytes a tick made.
// --fec G[,K] (G = 1 .. 255 pieces per group, K = 1 or 2 parity datagrams per group, default 1): the link loses datagrams and the
// receiver rebuilds them.  The relay calls mi355_cwire_fec_batch behind the split call with no wait in between; every parity block
// is one more datagram.  The side information of a datagram -- stream, group, slot, members, fec_len, parity or not -- is this
// tool's own framing, outside the payload.  The seeded generator loses 0 .. K of every group's m + K datagrams, class by class in
// turn: nothing; one piece; a piece and P; a piece and Q; two pieces; parity only -- and the run fails unless it met every class
// that K allows.  The receiver takes the lost pieces' headers from the 8-byte prefixes (mi355_cwire_fec_repair_host), rebuilds what
// is missing with ONE mi355_cwire_fec_repair_batch per tick, requires clean verdicts, checks the rebuilt pieces with
// mi355_cwire_check_batch and then applies survivors and rebuilt pieces in a shuffled order as without --fec.  Losing more than K
// of a group is the resync mode's business, not this one's.
static const int kDatagramRound = 64;

static int run_multi_datagram(int w, int h, int T, int S, int K, long max_bytes, int G, int Kp) {
    const bool coalesce = K > 0;
    if (!coalesce) K = 1;
    Session ss(w, h);
    const size_t n = ss.n, M = (size_t)max_bytes;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver relay, rcv;
    if (tx.open(ss, S, K) || relay.open(ss, S, S * K, S * K, false) || rcv.open(ss, S, S * kDatagramRound, S)) return 1;
    // what any S records of the frame can need: at most n entries, at most n escapes each
    const size_t pcap = (size_t)S * mi355_cwire_split_pieces_max((uint32_t)n, (uint32_t)n, M);
    const size_t bcap = (size_t)S * mi355_cwire_split_bytes_max((uint32_t)n, (uint32_t)n, M);
    const size_t stage_cap = bcap + 8 * (size_t)S * kDatagramRound;
    void *d_roff = ss.dev(relay.core, sizeof(uint32_t) * (S + 1)), *d_rpos = ss.dev(relay.core, sizeof(uint64_t) * (S + 1));
    void *d_fwd = ss.dev(relay.core, rcv.cap);
    void *d_first = ss.dev(relay.core, sizeof(uint32_t) * (S + 1)), *d_ppos = ss.dev(relay.core, sizeof(uint64_t) * (pcap + 1));
    void *d_pieces = ss.dev(relay.core, bcap), *d_stage = ss.dev(rcv.core, stage_cap);
    if (!ss.ok()) return 1;
    std::vector<uint8_t> host_frames((size_t)S * n), pieces(bcap), arrived(bcap), stage(stage_cap);
    std::vector<uint32_t> roff(S + 1), first(S + 1), cnt(S), esc(S), pc((size_t)S * kDatagramRound), pe((size_t)S * kDatagramRound);
    std::vector<uint64_t> rpos(S + 1), ppos(pcap + 1);
    std::vector<std::vector<uint32_t>> order(S);
    // --fec: the relay's parity outputs; the receiver's copy of what arrived (pieces, then parity blocks), its rebuilt blocks
    const size_t gcap = G ? mi355_cwire_fec_groups_max(pcap, S, G) : 0, par_cap = gcap * (size_t)Kp * M;
    const int jobs_cap = S * kDatagramRound;   // (the receiver's max_batch)
    void *d_ffirst = nullptr, *d_flen = nullptr, *d_par = nullptr, *d_frx = nullptr, *d_rep = nullptr, *d_vd = nullptr, *d_chk = nullptr;
    if (G) {
        d_ffirst = ss.dev(relay.core, sizeof(uint32_t) * (S + 1));
        d_flen = ss.dev(relay.core, sizeof(uint32_t) * gcap);
        d_par = ss.dev(relay.core, par_cap);
        d_frx = ss.dev(rcv.core, bcap + par_cap);
        d_rep = ss.dev(rcv.core, 2 * (size_t)jobs_cap * M);
        d_vd = ss.dev(rcv.core, sizeof(uint32_t) * 6 * (size_t)jobs_cap);   // (the repair's verdicts, then the check's)
        d_chk = ss.dev(rcv.core, (size_t)jobs_cap * M);
        if (!ss.ok()) return 1;
    }
    std::vector<uint8_t> par(par_cap), par_arrived(par_cap), rebuilt(G ? 2 * (size_t)jobs_cap * M : 0), chk(G ? (size_t)jobs_cap * M : 0);
    std::vector<uint32_t> ffirst(S + 1), flen(gcap), job_first, slot_len, job_len, vd(4 * (size_t)jobs_cap), job_piece;
    std::vector<uint64_t> slot_off, par_off;
    size_t parity_datagrams = 0, parity_bytes = 0, pieces_lost = 0, pieces_rebuilt = 0, met[5] = {0, 0, 0, 0, 0}, turn = 0;
    if (cams.start(ss, tx, rcv, host_frames.data())) return 1;
    size_t received = 0, datagrams = 0, datagram_bytes = 0, largest = 0;
    int max_err = 0, calls = 0, steps = 0;
    for (int t0 = 0; t0 < T; t0 += K, steps++) {
        const int nb = T - t0 < K ? T - t0 : K;
        cams.fill(tx.frames.data(), t0, nb);
        // ---- server: one tick -> S records, or nb ticks -> S * nb records, in one call
        if (tx.step(nb, coalesce)) return 1;
        // ---- the sockets into the relay; a host client beside it applies every original record
        if (slices_to_node(ss, tx, relay, nb, host_frames.data(), nullptr)) return 1;
        received += tx.cb;
        // ---- relay: (the burst -> one record per camera, then) the S records -> pieces, in one call; no frame exists here
        const void *d_rec = relay.d_rx;
        if (coalesce) {
            OK(mi355_cwire_coalesce_cwire_batch(relay.core, relay.d_rx, relay.counts.data(), relay.escapes.data(), S, nb, d_roff, d_rpos,
                                                d_fwd, rcv.cap));
            OK(mi355_download(relay.core, roff.data(), d_roff, sizeof(uint32_t) * (S + 1)));
            OK(mi355_download(relay.core, rpos.data(), d_rpos, sizeof(uint64_t) * (S + 1)));
            if (rpos[S] > rcv.cap) { fprintf(stderr, "coalesced stream larger than its bound\n"); return 1; }
            for (int s = 0; s < S; s++) {
                cnt[s] = roff[s + 1] - roff[s];
                esc[s] = (uint32_t)((rpos[s + 1] - rpos[s] - mi355_cwire_frame_bytes(cnt[s], 0)) / 4);
            }
            d_rec = d_fwd;
        } else {
            for (int s = 0; s < S; s++) {
                cnt[s] = relay.counts[s];
                esc[s] = relay.escapes[s];
            }
        }
        OK(mi355_cwire_split_cwire_batch(relay.core, d_rec, cnt.data(), esc.data(), S, M, d_first, d_ppos, pcap, d_pieces, bcap));
        if (G)   // the parity blocks of what the split call is still writing: same stream, no wait
            OK(mi355_cwire_fec_batch(relay.core, d_pieces, bcap, d_first, d_ppos, pcap, S, G, Kp, M, d_ffirst, d_flen, gcap, d_par, par_cap));
        calls++;
        OK(mi355_download(relay.core, first.data(), d_first, sizeof(uint32_t) * (S + 1)));
        const size_t np = first[S];
        if (np > pcap) { fprintf(stderr, "more pieces than their bound\n"); return 1; }
        OK(mi355_download(relay.core, ppos.data(), d_ppos, sizeof(uint64_t) * (np + 1)));
        if (ppos[np] > bcap) { fprintf(stderr, "pieces larger than their bound\n"); return 1; }
        OK(mi355_download(relay.core, pieces.data(), d_pieces, (size_t)ppos[np]));
        // ---- the datagram socket: a piece is one write and one read
        for (size_t p = 0; p < np; p++) {
            const size_t len = (size_t)(ppos[p + 1] - ppos[p]);
            if (len > M) { fprintf(stderr, "tick %d: piece %zu has %zu bytes > %zu\n", t0, p, len, M); return 1; }
            if (!ss.send(pieces.data() + ppos[p], arrived.data() + ppos[p], len)) return 1;
            largest = std::max(largest, len);
        }
        datagrams += np;
        datagram_bytes += (size_t)ppos[np];
        if (G) {
            // ---- the parity datagrams, and what the link loses of every group
            OK(mi355_download(relay.core, ffirst.data(), d_ffirst, sizeof(uint32_t) * (S + 1)));
            const size_t ng = ffirst[S];
            if (ng > gcap) { fprintf(stderr, "more groups than their bound\n"); return 1; }
            if (ng) OK(mi355_download(relay.core, flen.data(), d_flen, sizeof(uint32_t) * ng));
            if (ng) OK(mi355_download(relay.core, par.data(), d_par, ng * (size_t)Kp * M));
            job_first.assign(1, 0u);
            slot_off.clear(); slot_len.clear(); par_off.clear(); job_len.clear(); job_piece.clear();
            for (int s = 0; s < S; s++)
                for (uint32_t g = ffirst[s]; g < ffirst[s + 1]; g++) {
                    const uint32_t p0 = first[s] + (g - ffirst[s]) * (uint32_t)G, m = std::min((uint32_t)G, first[s + 1] - p0), L = flen[g];
                    if (L == 0 || L > M) { fprintf(stderr, "tick %d: group %u of camera %d has fec_len %u\n", t0, g, s, L); return 1; }
                    for (int q = 0; q < Kp; q++) {
                        const size_t at = ((size_t)g * Kp + q) * M;
                        if (!ss.send(par.data() + at, par_arrived.data() + at, L)) return 1;
                    }
                    parity_datagrams += Kp;
                    parity_bytes += (size_t)Kp * L;
                    // the classes in turn: 0 nothing, 1 one piece, 2 a piece and P, 3 a piece and Q, 4 two pieces, 5 parity only
                    const int cls = Kp == 2 ? (int)(turn % 6) : (int)(turn % 3 == 2 ? 5 : turn % 3);
                    turn++;
                    int lost[2] = {-1, -1};
                    bool have_p = true, have_q = Kp == 2;
                    if (cls >= 1 && cls <= 4) lost[0] = (int)(rnd() % m);
                    if (cls == 4 && m >= 2) {
                        lost[1] = (int)((lost[0] + 1 + rnd() % (m - 1)) % m);
                        if (lost[1] < lost[0]) std::swap(lost[0], lost[1]);
                    }
                    if (cls == 2) have_p = false;
                    if (cls == 3) have_q = false;
                    if (cls == 5) { if (Kp == 2 && (rnd() & 1)) have_q = false; else have_p = false; }
                    if (cls >= 1) met[cls == 4 && m < 2 ? 0 : cls - 1]++;
                    if (!have_p) memset(par_arrived.data() + (size_t)g * Kp * M, 0xEE, L);
                    if (Kp == 2 && !have_q) memset(par_arrived.data() + ((size_t)g * Kp + 1) * M, 0xEE, L);
                    if (lost[0] < 0) continue;
                    // ---- receiver: the lost pieces' headers from the 8-byte prefixes; then one job of the tick's repair call
                    const void *pre[255];
                    uint32_t pre_len[255], hdr[2][2] = {{0, 0}, {0, 0}}, pre_vd[2];
                    for (uint32_t i = 0; i < m; i++) {
                        const bool gone = (int)i == lost[0] || (int)i == lost[1];
                        const size_t at = (size_t)ppos[p0 + i], len = (size_t)(ppos[p0 + i + 1] - ppos[p0 + i]);
                        if (gone) memset(arrived.data() + at, 0xEE, len);
                        pre[i] = gone ? nullptr : arrived.data() + at;
                        pre_len[i] = 8;
                        slot_off.push_back(gone ? MI355_FEC_ABSENT : (uint64_t)at);
                        slot_len.push_back((uint32_t)len);
                        if (gone) job_piece.push_back(p0 + i);
                    }
                    if (lost[1] < 0) job_piece.push_back(UINT32_MAX);
                    const uint8_t *pp = par_arrived.data() + (size_t)g * Kp * M, *pq = pp + M;
                    OK(mi355_cwire_fec_repair_host((int)m, pre, pre_len, have_p ? pp : nullptr, have_q ? pq : nullptr, 8, hdr[0], hdr[1], pre_vd));
                    for (int k = 0; k < 2 && lost[k] >= 0; k++)
                        if (mi355_cwire_frame_bytes(hdr[k][0], hdr[k][1]) != (size_t)(ppos[p0 + lost[k] + 1] - ppos[p0 + lost[k]])) {
                            fprintf(stderr, "tick %d: the prefix repair gave a wrong header for piece %u\n", t0, p0 + lost[k]);
                            return 1;
                        }
                    par_off.push_back(have_p ? (uint64_t)(bcap + (size_t)g * Kp * M) : MI355_FEC_ABSENT);
                    par_off.push_back(have_q ? (uint64_t)(bcap + ((size_t)g * Kp + 1) * M) : MI355_FEC_ABSENT);
                    job_len.push_back(L);
                    job_first.push_back((uint32_t)slot_off.size());
                    pieces_lost += lost[1] >= 0 ? 2 : 1;
                }
            const int njobs = (int)job_len.size();
            if (njobs > jobs_cap) { fprintf(stderr, "tick %d: %d groups to repair, the receiver's core takes %d\n", t0, njobs, jobs_cap); return 1; }
            if (njobs) {
                OK(mi355_upload(rcv.core, d_frx, arrived.data(), (size_t)ppos[np]));
                OK(mi355_upload(rcv.core, (uint8_t *)d_frx + bcap, par_arrived.data(), ng * (size_t)Kp * M));
                OK(mi355_cwire_fec_repair_batch(rcv.core, d_frx, bcap + par_cap, njobs, job_first.data(), slot_off.data(), slot_len.data(),
                                                par_off.data(), job_len.data(), d_rep, M, d_vd));
                OK(mi355_download(rcv.core, rebuilt.data(), d_rep, 2 * (size_t)njobs * M));
                OK(mi355_download(rcv.core, vd.data(), d_vd, sizeof(uint32_t) * 2 * njobs));
                // the rebuilt pieces back to back, checked before they are applied: clean verdicts are no replacement for that
                for (size_t b0 = 0; b0 < 2 * (size_t)njobs; b0 += jobs_cap) {
                    const size_t b1 = std::min(b0 + (size_t)jobs_cap, 2 * (size_t)njobs);
                    size_t q = 0;
                    int nc = 0;
                    for (size_t b = b0; b < b1; b++) {
                        const uint32_t p = job_piece[b];
                        if (p == UINT32_MAX) continue;
                        if (vd[b]) { fprintf(stderr, "tick %d: rebuilt piece %u has verdict %u\n", t0, p, vd[b]); return 1; }
                        const size_t len = (size_t)(ppos[p + 1] - ppos[p]);
                        memcpy(chk.data() + q, rebuilt.data() + b * M, len);
                        memcpy(&pc[nc], chk.data() + q, 4);
                        memcpy(&pe[nc], chk.data() + q + 4, 4);
                        if (mi355_cwire_frame_bytes(pc[nc], pe[nc]) != len) { fprintf(stderr, "tick %d: rebuilt piece %u: framing broken\n", t0, p); return 1; }
                        q += len;
                        nc++;
                    }
                    if (!nc) continue;
                    OK(mi355_upload(rcv.core, d_chk, chk.data(), q));
                    OK(mi355_cwire_check_batch(rcv.core, d_chk, pc.data(), pe.data(), nc, (uint8_t *)d_vd + sizeof(uint32_t) * 2 * njobs));
                    std::vector<uint32_t> cv(4 * (size_t)nc);
                    OK(mi355_download(rcv.core, cv.data(), (uint8_t *)d_vd + sizeof(uint32_t) * 2 * njobs, sizeof(uint32_t) * 4 * nc));
                    for (int i = 0; i < nc; i++)
                        if (cv[4 * (size_t)i]) { fprintf(stderr, "tick %d: a rebuilt piece is refused by the check (flags %u)\n", t0, cv[4 * (size_t)i]); return 1; }
                }
                for (size_t b = 0; b < 2 * (size_t)njobs; b++) {
                    const uint32_t p = job_piece[b];
                    if (p == UINT32_MAX) continue;
                    const size_t len = (size_t)(ppos[p + 1] - ppos[p]);
                    if (memcmp(rebuilt.data() + b * M, pieces.data() + ppos[p], len) != 0) {
                        fprintf(stderr, "tick %d: rebuilt piece %u differs from the piece that was sent\n", t0, p);
                        return 1;
                    }
                    memcpy(arrived.data() + ppos[p], rebuilt.data() + b * M, len);
                    pieces_rebuilt++;
                }
            }
        }
        // ---- receiver: every camera's pieces in an order of their own, kDatagramRound of each per call, empty records behind them
        size_t most = 0;
        for (int s = 0; s < S; s++) {
            order[s].clear();
            for (uint32_t p = first[s]; p < first[s + 1]; p++) order[s].push_back(p);
            for (size_t i = order[s].size(); i > 1; i--) std::swap(order[s][i - 1], order[s][rnd() % i]);
            most = std::max(most, order[s].size());
        }
        for (size_t r0 = 0; r0 < most; r0 += kDatagramRound) {
            const int nr = (int)std::min(most - r0, (size_t)kDatagramRound);
            size_t q = 0;
            for (int s = 0; s < S; s++)
                for (int j = 0; j < nr; j++) {
                    const size_t b = (size_t)s * nr + j;
                    if (r0 + j < order[s].size()) {
                        const uint32_t p = order[s][r0 + j];
                        const size_t len = (size_t)(ppos[p + 1] - ppos[p]);
                        memcpy(stage.data() + q, arrived.data() + ppos[p], len);
                        memcpy(&pc[b], stage.data() + q, 4);
                        memcpy(&pe[b], stage.data() + q + 4, 4);
                        if (mi355_cwire_frame_bytes(pc[b], pe[b]) != len) { fprintf(stderr, "stream framing broken\n"); return 1; }
                        q += len;
                    } else {
                        memset(stage.data() + q, 0, 8);
                        pc[b] = pe[b] = 0;
                        q += 8;
                    }
                }
            OK(mi355_upload(rcv.core, d_stage, stage.data(), q));
            OK(mi355_apply_multi_stream_cwire_batch(rcv.core, d_stage, pc.data(), pe.data(), S, nr, rcv.d_states, n, nullptr, 0));
        }
        if (rcv.get_states()) return 1;
        // ---- checks
        for (int s = 0; s < S; s++)
            if (memcmp(&host_frames[(size_t)s * n], &rcv.states[(size_t)s * n], n) != 0) {
                fprintf(stderr, "tick %d: camera %d: receiver state != host client that applied the %d original records\n", t0, s, nb);
                return 1;
            }
        if (states_equal(tx, rcv, t0)) return 1;
        for (int s = 0; s < S; s++)
            max_err = std::max(max_err, max_abs_error(&rcv.states[(size_t)s * n], &tx.frames[((size_t)s * nb + nb - 1) * n], n));
    }
    if (!datagrams) { fprintf(stderr, "--datagram: no piece was made\n"); return 1; }
    if (G) {
        static const char *const names[5] = {"one piece", "a piece and P", "a piece and Q", "two pieces", "parity only"};
        for (int c = 0; c < 5; c++)
            if (!met[c] && (Kp == 2 || c == 0 || c == 4)) { fprintf(stderr, "--fec: no group lost %s\n", names[c]); return 1; }
        if (pieces_rebuilt != pieces_lost) { fprintf(stderr, "--fec: %zu pieces lost, %zu rebuilt\n", pieces_lost, pieces_rebuilt); return 1; }
    }
    if (within_threshold(max_err, ss) || ss.close()) return 1;
    if (G) {
        printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"coalesce\": %s, \"datagram\": %zu, "
               "\"fec\": [%d, %d], \"relay_calls\": %d, \"width\": %d, \"height\": %d, \"ticks\": %d, \"changed_bytes\": %zu, "
               "\"relay_received_bytes\": %zu, \"pieces\": %zu, \"piece_bytes\": %zu, \"parity_datagrams\": %zu, \"parity_bytes\": %zu, "
               "\"pieces_lost\": %zu, \"pieces_rebuilt\": %zu, \"largest_piece\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d}\n",
               S, coalesce ? K : 0, coalesce ? "true" : "false", M, G, Kp, calls, w, h, T, tx.changed, received, datagrams, datagram_bytes,
               parity_datagrams, parity_bytes, pieces_lost, pieces_rebuilt, largest, (size_t)T * S * n, max_err);
        return 0;
    }
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"coalesce\": %s, \"datagram\": %zu, "
           "\"relay_calls\": %d, \"width\": %d, \"height\": %d, \"ticks\": %d, \"changed_bytes\": %zu, \"relay_received_bytes\": %zu, "
           "\"pieces\": %zu, \"piece_bytes\": %zu, \"pieces_per_tick\": %.2f, \"piece_bytes_per_tick\": %.1f, \"largest_piece\": %zu, "
           "\"raw_bytes\": %zu, \"max_abs_error\": %d}\n",
           S, coalesce ? K : 0, coalesce ? "true" : "false", M, calls, w, h, T, tx.changed, received, datagrams, datagram_bytes,
           (double)datagrams / steps, (double)datagram_bytes / steps, largest, (size_t)T * S * n, max_err);
    return 0;
}

// --compact --multi S --crop X,Y,W,H [--burst K]: a relay for viewers that zoomed into their cameras.  It holds no frame: it
// uploads every camera's records as they came off its socket (one tick, or a burst of K), cuts them to the rectangle with ONE
// mi355_cwire_crop_cwire_batch -- of a burst, the crop of the coalesced burst -- and forwards those S records, indexed in the
// rectangle's own W x H frame.  The receiver is a core of W x H pixels: its states are seeded from the crops of the base frames
// and take the records with one mi355_apply_multi_cwire_batch.  After every tick or burst each of its states must equal the
// crop of the sender's state and of a full-size host client (mi355_cwire_apply_host) that applied the original records.
static void crop_frame(uint8_t *dst, const uint8_t *src, int w, const int32_t *r) {
    for (int y = 0; y < r[3]; y++) memcpy(dst + (size_t)y * 3 * r[2], src + ((size_t)(r[1] + y) * w + r[0]) * 3, (size_t)3 * r[2]);
}

static int run_multi_crop(int w, int h, int T, int S, int K, const int32_t *rect) {
    const bool burst = K > 0;
    if (!burst) K = 1;
    Session ss(w, h), view(rect[2], rect[3]);
    const size_t n = ss.n, m = view.n;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver relay, rcv;
    if (tx.open(ss, S, K) || relay.open(ss, S, S * K, S * K, false) || rcv.open(view, S, S, S)) return 1;
    void *d_roff = ss.dev(relay.core, sizeof(uint32_t) * (S + 1)), *d_rpos = ss.dev(relay.core, sizeof(uint64_t) * (S + 1));
    void *d_fwd = ss.dev(relay.core, rcv.cap);   // S records of a W x H frame at most: the sum of the rectangles' bounds
    if (!ss.ok() || !view.ok()) return 1;
    std::vector<uint8_t> host_frames((size_t)S * n), fwd(rcv.cap), cropped((size_t)S * m), seed((size_t)S * m);
    std::vector<int32_t> rects((size_t)4 * S);
    for (int s = 0; s < S; s++) memcpy(&rects[(size_t)4 * s], rect, 4 * sizeof(int32_t));
    std::vector<uint32_t> roff(S + 1);
    std::vector<uint64_t> rpos(S + 1);
    // the sender's states and the full-size host clients from the base frames; the receiver's from their crops, through the pipe
    OK(mi355_upload(tx.core, tx.d_states, cams.bases.data(), cams.bases.size()));
    memcpy(host_frames.data(), cams.bases.data(), cams.bases.size());
    for (int s = 0; s < S; s++) crop_frame(&cropped[(size_t)s * m], &cams.bases[(size_t)s * n], w, rect);
    if (!ss.send(cropped.data(), seed.data(), seed.size())) return 1;
    OK(mi355_upload(rcv.core, rcv.d_states, seed.data(), seed.size()));
    size_t received = 0, forwarded = 0, kept = 0;
    int calls = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K;
        cams.fill(tx.frames.data(), t0, nb);
        // ---- server: nb ticks of S cameras -> S * nb records in one call
        if (tx.step(nb, burst)) return 1;
        // ---- the sockets into the relay; a full-size host client beside it applies every original record
        if (slices_to_node(ss, tx, relay, nb, host_frames.data(), nullptr)) return 1;
        received += tx.cb;
        // ---- relay: the records -> one cropped record per camera, in one call; no frame exists here
        OK(mi355_cwire_crop_cwire_batch(relay.core, relay.d_rx, relay.counts.data(), relay.escapes.data(), S, nb, rects.data(), 0u, d_roff,
                                        d_rpos, d_fwd, rcv.cap));
        calls++;
        OK(mi355_download(relay.core, roff.data(), d_roff, sizeof(uint32_t) * (S + 1)));
        OK(mi355_download(relay.core, rpos.data(), d_rpos, sizeof(uint64_t) * (S + 1)));
        if (rpos[S] > rcv.cap) { fprintf(stderr, "cropped stream larger than its bound\n"); return 1; }
        const size_t fb = (size_t)rpos[S];
        OK(mi355_download(relay.core, fwd.data(), d_fwd, fb));
        kept += roff[S];
        // ---- the sockets out of the relay, one record per camera; the receiver finds them from their headers
        if (!ss.send(fwd.data(), rcv.rx.data(), fb)) return 1;
        forwarded += fb;
        if (rcv.walk(0, fb, 0, S)) return 1;
        // ---- receiver: one call per tick or burst, on W x H states
        OK(mi355_upload(rcv.core, rcv.d_rx, rcv.rx.data(), fb));
        if (rcv.apply_tick() || rcv.get_states() || tx.get_states()) return 1;
        // ---- checks: the crop of the sender's states, and of the host clients that applied all the original records
        for (int s = 0; s < S; s++) {
            crop_frame(&cropped[(size_t)s * m], &tx.states[(size_t)s * n], w, rect);
            if (same(&cropped[(size_t)s * m], &rcv.states[(size_t)s * m], m, "receiver state != crop of the sender's state", t0)) return 1;
            crop_frame(&cropped[(size_t)s * m], &host_frames[(size_t)s * n], w, rect);
            if (same(&cropped[(size_t)s * m], &rcv.states[(size_t)s * m], m, "receiver state != crop of the host client's frame", t0)) return 1;
        }
    }
    if (kept == 0) { fprintf(stderr, "no entry fell into the rectangle: nothing was checked\n"); return 1; }
    if (ss.close() || view.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"crop\": [%d, %d, %d, %d], \"relay_calls\": %d, "
           "\"width\": %d, \"height\": %d, \"ticks\": %d, \"changed_bytes\": %zu, \"cropped_entries\": %zu, "
           "\"relay_received_bytes\": %zu, \"relay_forwarded_bytes\": %zu, \"cropped_states_equal_every_step\": true}\n",
           S, burst ? K : 0, rect[0], rect[1], rect[2], rect[3], calls, w, h, T, tx.changed, kept, received, forwarded);
    return 0;
}

// --compact --multi S --mosaic CxR [--burst K]: a multiview relay.  It holds no frame: it uploads every camera's records as they
// came off its socket (one tick, or a burst of K) and makes ONE record of a canvas of C x R cells with ONE
// mi355_cwire_mosaic_cwire_batch, camera s whole in cell (s % C, s / C); S <= C*R, the cells behind the last camera stay empty.
// The receiver is a viewer that holds one C*W x R*H host state, seeded with the tiling of the base frames, reads one socket and
// applies the record with mi355_cwire_apply_host.  After every tick or burst its canvas must equal the tiling of the sender's
// states and of full-size host clients that applied the original records.
static void tile_frames(uint8_t *canvas, const uint8_t *frames, int S, int w, int h, int C) {
    const size_t n = (size_t)3 * w * h, row = (size_t)3 * w, crow = row * C;
    for (int s = 0; s < S; s++)
        for (int y = 0; y < h; y++)
            memcpy(canvas + ((size_t)(s / C) * h + y) * crow + (size_t)(s % C) * row, frames + (size_t)s * n + (size_t)y * row, row);
}

static int run_multi_mosaic(int w, int h, int T, int S, int K, int C, int R) {
    const bool burst = K > 0;
    if (!burst) K = 1;
    Session ss(w, h);
    const size_t n = ss.n, nc = n * C * R;
    const int cw = C * w, ch = R * h;
    ss.runs.w = cw;   // (--runs: the records that cross the link are the canvas')
    ss.runs.h = ch;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver relay;
    // the relay's core keeps one fact word per 4096-byte tile of the canvas where it keeps those of max_batch frames: C*R suffice
    if (tx.open(ss, S, K) || relay.open(ss, S, S * K > C * R ? S * K : C * R, S * K, false)) return 1;
    const size_t cap = mi355_cwire_bytes_max(nc, 1);
    void *d_roff = ss.dev(relay.core, sizeof(uint32_t) * 2), *d_rpos = ss.dev(relay.core, sizeof(uint64_t) * 2);
    void *d_fwd = ss.dev(relay.core, cap);
    if (!ss.ok()) return 1;
    std::vector<uint8_t> host_frames((size_t)S * n), fwd(cap), rx(cap), tiled(nc, 0), canvas(nc, 0);
    std::vector<int32_t> place((size_t)6 * S);
    for (int s = 0; s < S; s++) {
        const int32_t p[6] = {0, 0, w, h, (s % C) * w, (s / C) * h};
        memcpy(&place[(size_t)6 * s], p, sizeof p);
    }
    uint32_t roff[2];
    uint64_t rpos[2];
    // the sender's states and the full-size host clients from the base frames; the viewer's canvas from their tiling, through the pipe
    OK(mi355_upload(tx.core, tx.d_states, cams.bases.data(), cams.bases.size()));
    memcpy(host_frames.data(), cams.bases.data(), cams.bases.size());
    tile_frames(tiled.data(), cams.bases.data(), S, w, h, C);
    if (!ss.send(tiled.data(), canvas.data(), nc)) return 1;
    size_t received = 0, forwarded = 0, kept = 0;
    int calls = 0;
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K;
        cams.fill(tx.frames.data(), t0, nb);
        // ---- server: nb ticks of S cameras -> S * nb records in one call
        if (tx.step(nb, burst)) return 1;
        // ---- the sockets into the relay; a full-size host client beside it applies every original record
        if (slices_to_node(ss, tx, relay, nb, host_frames.data(), nullptr)) return 1;
        received += tx.cb;
        // ---- relay: the records -> ONE record of the canvas, in one call; no frame exists here
        OK(mi355_cwire_mosaic_cwire_batch(relay.core, relay.d_rx, relay.counts.data(), relay.escapes.data(), S, nb, place.data(), cw, ch,
                                          d_roff, d_rpos, d_fwd, cap));
        calls++;
        OK(mi355_download(relay.core, roff, d_roff, sizeof roff));
        OK(mi355_download(relay.core, rpos, d_rpos, sizeof rpos));
        if (roff[0] != 0 || rpos[0] != 0 || rpos[1] > cap) { fprintf(stderr, "canvas record larger than its bound\n"); return 1; }
        const size_t fb = (size_t)rpos[1];
        OK(mi355_download(relay.core, fwd.data(), d_fwd, fb));
        kept += roff[1];
        // ---- the ONE socket out of the relay; the viewer reads the header and applies the record to its canvas
        if (!ss.send_records(fwd.data(), rx.data(), fb, 1)) return 1;
        forwarded += fb;
        uint32_t cnt, esc;
        size_t at[2];
        if (walk_records(rx.data(), 0, fb, 1, &cnt, &esc, at) || cnt != roff[1]) { fprintf(stderr, "canvas record framing broken\n"); return 1; }
        if (host_apply(canvas.data(), nc, rx.data(), at, 0)) return 1;
        // ---- checks: the tiling of the sender's states, and of the host clients that applied all the original records
        if (tx.get_states()) return 1;
        tile_frames(tiled.data(), tx.states.data(), S, w, h, C);
        if (same(tiled.data(), canvas.data(), nc, "viewer's canvas != tiling of the sender's states", t0)) return 1;
        tile_frames(tiled.data(), host_frames.data(), S, w, h, C);
        if (same(tiled.data(), canvas.data(), nc, "viewer's canvas != tiling of the host clients' frames", t0)) return 1;
    }
    if (kept == 0) { fprintf(stderr, "no entry reached the canvas: nothing was checked\n"); return 1; }
    if (ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"mosaic\": [%d, %d], \"relay_calls\": %d, "
           "\"width\": %d, \"height\": %d, \"canvas\": [%d, %d], \"ticks\": %d, \"changed_bytes\": %zu, \"canvas_entries\": %zu, "
           "\"relay_received_bytes\": %zu, \"relay_forwarded_bytes\": %zu, \"canvases_equal_every_step\": true}\n",
           S, burst ? K : 0, C, R, calls, w, h, cw, ch, T, tx.changed, kept, received, forwarded);
    return 0;
}

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
struct FrameReceiver {
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

// --compact --per-frame: the per-frame server, one host frame per call and no device pointer in sight.  The sender feeds
// host frames through mi355_pipe_submit_cwire, four in flight, and writes each frame's record to the pipe with ONE write()
// from the pinned buffer it arrived in; the receiver -- a thread with no core -- reads header and body, applies the record
// with mi355_cwire_apply_host and compares its frame, frame by frame, with that of a host client of the plain path
// (mi355_exec on a second core: frame[xs[i]] += diff[i], client/opencv.cpp:64-66).
static int run_per_frame(int w, int h, int T) {
    const int depth = 4;
    Session ss(w, h);
    const size_t n = ss.n, cap = mi355_cwire_bytes_max(n, 1);
    Cameras cam(1, w, h);
    mi355_core *server = ss.core(1), *plain = ss.core(1);
    if (!ss.ok()) return 1;
    std::vector<uint8_t> frame(n), p_frame(cam.bases), s_state(n);
    OK(mi355_set_state(server, cam.bases.data()));
    OK(mi355_set_state(plain, cam.bases.data()));
    OK(mi355_prepare(server, MI355_PREPARE_EXEC_CWIRE));
    void *h_frame[depth], *h_rec[depth];
    for (int i = 0; i < depth; i++) {
        h_frame[i] = ss.pinned(n);
        h_rec[i] = ss.pinned(cap);
    }
    void *p_in = ss.pinned(n), *p_xs = ss.pinned(n * sizeof(int32_t));
    if (!ss.ok()) return 1;
    OK(mi355_pipe_open(server, depth));
    // (from here to receiver.join() an error ends the loop, not the function: the thread is joined first)
    Expected expected;
    FrameReceiver rx;
    rx.fd = ss.fds[0]; rx.frames = T; rx.n = n; rx.expected = &expected;
    signal(SIGPIPE, SIG_IGN);   // (a write to a pipe the receiver has closed returns an error)
    std::thread receiver(&FrameReceiver::run, &rx);
    auto send = [&](const void *p, size_t len) {   // ONE write per record; the loop only serves a short write
        const uint8_t *b = (const uint8_t *)p;
        while (len) {
            const ssize_t k = write(ss.fds[1], b, len);
            if (k <= 0) return false;
            b += k;
            len -= (size_t)k;
        }
        return true;
    };
    const bool ok = send(cam.bases.data(), n);   // threads.cpp:220
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
    auto submit = [&](int t) -> int {
        cam.fill(frame.data(), t, 1);
        // the plain path beside it: mi355_exec on its own core, and its host client
        memcpy(p_in, frame.data(), n);
        uint32_t pos = 0;
        OK(mi355_exec(plain, (uint8_t *)p_in, nullptr, nullptr, &pos, (int32_t *)p_xs));
        for (uint32_t i = 0; i < pos; i++) p_frame[((const int32_t *)p_xs)[i]] += ((const uint8_t *)p_in)[i];
        expected.push(p_frame);
        // the elaboration loop: one host frame in, a ticket out
        memcpy(h_frame[t % depth], frame.data(), n);
        OK(mi355_pipe_submit_cwire(server, (const uint8_t *)h_frame[t % depth], nullptr, nullptr, h_rec[t % depth], cap, &tickets[t % depth]));
        return 0;
    };
    for (int t = 0; t < T && ok && !rc; t++) {
        if (t >= depth) rc = finish(t - depth);
        if (!rc) rc = submit(t);
    }
    for (int t = T > depth ? T - depth : 0; t < T && ok && !rc; t++) rc = finish(t);
    close(ss.fds[1]);   // (a receiver that still waits for bytes sees the end of the stream)
    if (rc || !ok)
        for (int t = 0; t < T; t++) expected.push(std::vector<uint8_t>());   // ... and one that waits for a frame gets a wrong one
    receiver.join();
    if (rc || !ok) return 1;
    if (!rx.error.empty()) { fprintf(stderr, "%s\n", rx.error.c_str()); return 1; }
    OK(mi355_pipe_close(server));
    OK(mi355_get_state(server, s_state.data()));
    if (same(s_state.data(), p_frame.data(), n, "server state != plain client frame") || ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"per_frame\": true, \"depth\": %d, \"width\": %d, \"height\": %d, "
           "\"frames\": %d, \"frames_equal\": %d, \"changed_bytes\": %zu, \"wire_bytes\": %zu, \"reference_wire_bytes\": %zu, "
           "\"raw_bytes\": %zu}\n",
           depth, w, h, T, rx.equal, changed, sent_bytes, mi355_wire_bytes(T, changed), (size_t)T * n);
    return rx.equal == T ? 0 : 1;
}

// --compact --multi S --resync R [--burst K]: a receiver that lost a record finds its way back.  At tick R the receiver drops one
// camera's record (it applies an empty record in its place), so that camera's frame is wrong from then on.  After tick R + 1 it
// digests its states (mi355_state_digest_batch, checked against mi355_state_digest_host) and sends the digests up; the sender
// answers behind its latest tick -- with --burst K the end of the burst it has already made -- with a tile mask and one refresh
// record per camera (mi355_refresh_cwire_batch); the receiver applies the ticks that were in flight, clears the masked tiles
// (mi355_state_clear_tiles_batch) and applies the refresh records like any others.  Checked: the dropped camera's frame differs
// from the sender's at every tick between the loss and the refresh, and every other frame of every tick -- all of them from the
// refresh on -- equals the sender's; the dropped camera has mask bits and, unless ticks were in flight, only that camera (the
// others get the 8-byte record); a host client that clears the tiles itself and calls mi355_cwire_apply_host ends at the same
// frames.
static int run_multi_resync(int w, int h, int T, int S, int R, int K, int wall_k) {
    if (R < 0 || R + 1 >= T) { fprintf(stderr, "--resync K needs 0 <= K and K + 1 < --frames\n"); return 2; }
    if (K < 1) K = 1;
    Session ss(w, h);
    const size_t n = ss.n;
    const int B = S * K, victim = R % S;
    const size_t tiles = mi355_state_tiles(n), mask_words = (tiles + 31) / 32;
    const size_t dig_bytes = 8 * (size_t)S * tiles, mask_bytes = 4 * (size_t)S * mask_words;
    Cameras cams(S, w, h);
    Sender tx;
    Receiver rcv;
    WallCheck wall;
    if (tx.open(ss, S, K) || rcv.open(ss, S, S, S)) return 1;
    void *d_peer = ss.dev(tx.core, dig_bytes), *d_smask = ss.dev(tx.core, mask_bytes);   // the sender's refresh
    void *d_roff = ss.dev(tx.core, sizeof(uint32_t) * (S + 1)), *d_rpos = ss.dev(tx.core, sizeof(uint64_t) * (S + 1));
    void *d_rcw = ss.dev(tx.core, rcv.cap);
    void *d_dig = ss.dev(rcv.core, dig_bytes), *d_cmask = ss.dev(rcv.core, mask_bytes);   // the receiver's question, its clear
    if (!ss.ok()) return 1;
    if (int rc = wall.open(ss, rcv.core, wall_k, S)) return rc;
    // truth: a host client per camera that applies EVERY record -- the sender's state after every tick
    std::vector<uint8_t> truth((size_t)S * n), burst(tx.cap), host_client;
    if (cams.start(ss, tx, rcv, truth.data())) return 1;
    if (int rc = wall.full(rcv.d_states)) return rc;
    std::vector<uint32_t> b_counts(B), b_escapes(B), dig(2 * (size_t)S * tiles), dig_up(dig.size()), dig_host(2 * tiles),
        mask(S * mask_words), mask_rx(mask.size());
    std::vector<uint64_t> rpos(S + 1);
    std::vector<size_t> b_at(B + 1);
    size_t sent_bytes = 0, refresh_bytes = 0, lost_entries = 0, tiles_selected = 0;
    int wrong_ticks = 0, right_ticks_after = 0;
    bool lost = false, refreshed = false;
    // the receiver's frames of tick t against the truth: while the record is lost the victim's differs and only the victim's
    auto compare = [&](int t) -> int {
        for (int s = 0; s < S; s++) {
            const bool same_frame = memcmp(&truth[(size_t)s * n], &rcv.states[(size_t)s * n], n) == 0;
            const bool wrong = lost && !refreshed && s == victim;
            if (same_frame == wrong) {
                fprintf(stderr, "tick %d: camera %d: the receiver's frame %s the sender's\n", t, s, same_frame ? "equals" : "differs from");
                return 1;
            }
        }
        if (lost && !refreshed) wrong_ticks++;
        if (refreshed) right_ticks_after++;
        return 0;
    };
    for (int t0 = 0; t0 < T; t0 += K) {
        const int nb = T - t0 < K ? T - t0 : K;
        cams.fill(tx.frames.data(), t0, nb);
        // ---- server: nb ticks of S cameras; the sockets; the records of every socket, found from their headers
        if (tx.step(nb, K != 1)) return 1;
        if (!ss.send_records(tx.bytes.data(), burst.data(), tx.cb, S * nb)) return 1;
        sent_bytes += tx.cb;
        if (walk_records(burst.data(), 0, tx.cb, S * nb, b_counts.data(), b_escapes.data(), b_at.data())) return 1;
        // ---- client: tick k = record (s, k) of every s back to back, one upload, one call
        bool asked = false;
        for (int k = 0; k < nb; k++) {
            const int t = t0 + k;
            for (int s = 0; s < S; s++)
                if (host_apply(&truth[(size_t)s * n], n, burst.data(), b_at.data(), s * nb + k)) return 1;
            if (t == R) {   // the loss: the receiver has nothing to apply for this camera
                lost_entries = b_counts[victim * nb + k];
                if (lost_entries == 0) { fprintf(stderr, "--resync: the record to drop holds no entry\n"); return 1; }
                lost = true;
            }
            const size_t q = rcv.stage(burst.data(), b_at.data(), nb, k, t == R ? victim : -1);
            OK(mi355_upload(rcv.core, rcv.d_rx, rcv.rx.data(), q));
            if (rcv.apply_tick()) return 1;
            if (int rc = wall.update(rcv.d_rx, rcv.counts.data(), rcv.escapes.data(), 1, rcv.d_states)) return rc;   // (the wall shows what it holds)
            if (t == R + 1) {   // the receiver asks: its digests go up
                OK(mi355_state_digest_batch(rcv.core, rcv.d_states, n, S, d_dig));
                OK(mi355_download(rcv.core, dig.data(), d_dig, dig_bytes));
                asked = true;
            }
            if (rcv.get_states()) return 1;
            for (int s = 0; s < S && t == R + 1; s++) {
                OK(mi355_state_digest_host(&rcv.states[(size_t)s * n], n, dig_host.data()));
                if (memcmp(dig_host.data(), &dig[2 * (size_t)s * tiles], 8 * tiles) != 0) {
                    fprintf(stderr, "tick %d: camera %d: device digests != host digests\n", t, s);
                    return 1;
                }
            }
            if (int rc = compare(t)) return rc;
            if (int rc = wall.compare(rcv.states.data(), t)) return rc;
        }
        // ---- the states at both ends of the burst: the truth is the sender's
        if (tx.get_states() || same(tx.states.data(), truth.data(), truth.size(), "host client frames != sender states", t0)) return 1;
        if (!asked) continue;
        const bool in_flight = t0 + nb - 1 > R + 1;
        // ---- server: the answer, behind its latest tick
        if (!ss.send(dig.data(), dig_up.data(), dig_bytes)) return 1;
        OK(mi355_upload(tx.core, d_peer, dig_up.data(), dig_bytes));
        OK(mi355_refresh_cwire_batch(tx.core, tx.d_states, n, S, d_peer, d_smask, d_roff, d_rpos, d_rcw, rcv.cap));
        OK(mi355_download(tx.core, rpos.data(), d_rpos, sizeof(uint64_t) * (S + 1)));
        OK(mi355_download(tx.core, mask.data(), d_smask, mask_bytes));
        refresh_bytes = (size_t)rpos[S];
        if (refresh_bytes > rcv.cap) { fprintf(stderr, "refresh stream larger than its bound\n"); return 1; }
        OK(mi355_download(tx.core, tx.bytes.data(), d_rcw, refresh_bytes));
        if (!ss.send(mask.data(), mask_rx.data(), mask_bytes)) return 1;
        if (!ss.send_records(tx.bytes.data(), rcv.rx.data(), refresh_bytes, S)) return 1;
        // ---- client: clear, then apply like any other records; a host client does the same beside it
        if (rcv.walk(0, refresh_bytes, 0, S)) return 1;
        host_client = rcv.states;
        for (int s = 0; s < S; s++) {
            size_t bits = 0;
            for (size_t tl = 0; tl < tiles; tl++)
                if (mask_rx[s * mask_words + (tl >> 5)] >> (tl & 31) & 1u) {
                    bits++;
                    const size_t lo = tl * 4096, hi = lo + 4096 < n ? lo + 4096 : n;
                    memset(&host_client[(size_t)s * n + lo], 0, hi - lo);
                }
            // (ticks in flight behind the digests changed tiles of every camera: those are selected too, wasteful and never wrong)
            if (s == victim ? bits == 0 : !in_flight && (bits != 0 || rcv.counts[s] != 0)) {
                fprintf(stderr, "refresh: camera %d: %zu tiles selected, %u entries\n", s, bits, rcv.counts[s]);
                return 1;
            }
            tiles_selected += bits;
            if (host_apply(&host_client[(size_t)s * n], n, rcv.rx.data(), rcv.at.data(), s)) return 1;
        }
        OK(mi355_upload(rcv.core, d_cmask, mask_rx.data(), mask_bytes));
        OK(mi355_upload(rcv.core, rcv.d_rx, rcv.rx.data(), refresh_bytes));
        OK(mi355_state_clear_tiles_batch(rcv.core, rcv.d_states, n, S, d_cmask));
        if (rcv.apply_tick()) return 1;
        if (int rc = wall.masked(d_cmask, rcv.d_states)) return rc;   // the refresh's own mask: what was cleared and refilled is repainted
        if (rcv.get_states()) return 1;
        if (int rc = wall.compare(rcv.states.data(), t0 + nb - 1)) return rc;
        refreshed = true;
        if (same(rcv.states.data(), host_client.data(), host_client.size(), "refresh: receiver states != host client frames")) return 1;
        if (same(rcv.states.data(), tx.states.data(), tx.states.size(), "refresh: receiver states != sender states")) return 1;
    }
    if (!refreshed || wrong_ticks < 1) { fprintf(stderr, "--resync: no refresh happened\n"); return 1; }
    if (int rc = wall.close()) return rc;
    if (ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"multi\": %d, \"burst\": %d, \"resync\": %d, \"width\": %d, \"height\": %d, "
           "\"ticks\": %d, \"dropped_camera\": %d, \"dropped_entries\": %zu, \"wrong_ticks\": %d, \"ticks_equal_after_refresh\": %d, "
           "\"tiles\": %zu, \"tiles_selected\": %zu, \"digest_bytes\": %zu, \"mask_bytes\": %zu, \"refresh_bytes\": %zu, "
           "\"key_frame_bytes\": %zu, \"wire_bytes\": %zu%s}\n",
           S, K, R, w, h, T, victim, lost_entries, wrong_ticks, right_ticks_after, tiles, tiles_selected, dig_bytes, mask_bytes,
           refresh_bytes, (size_t)S * n, sent_bytes, wall.json().c_str());
    return 0;
}

// One camera, the state inside the cores (mi355_set_state / mi355_get_state): the start both single-camera modes share
struct Single {
    int B;
    Session ss;
    Cameras cam;
    mi355_core *server = nullptr, *client = nullptr;
    void *d_frames = nullptr, *d_off = nullptr;
    std::vector<uint8_t> frames, got_base, s_state, c_state;
    std::vector<uint32_t> off, counts, escapes;

    Single(int w, int h, int B_) : B(B_), ss(w, h), cam(1, w, h), frames((size_t)B * ss.n), got_base(ss.n), s_state(ss.n), c_state(ss.n), off(B + 1),
                                  counts(B), escapes(B) {}
    int start() {
        server = ss.core(B);
        client = ss.core(B);
        d_frames = ss.dev(server, (size_t)B * ss.n);
        d_off = ss.dev(server, sizeof(uint32_t) * (B + 1));
        if (!ss.ok()) return 1;
        OK(mi355_set_state(server, cam.bases.data()));                  // kernels.cu:406
        // the base frame first (threads.cpp:220); the client's start-up reads it (opencv.cpp:38-46)
        if (!ss.send(cam.bases.data(), got_base.data(), ss.n)) return 1;
        OK(mi355_set_state(client, got_base.data()));
        return 0;
    }
};

// (no option): the plain wire format, as the head of the file says
static int run_single_wire(int w, int h, int T, int B) {
    Single one(w, h, B);
    Session &ss = one.ss;
    const size_t n = ss.n, wire_cap = mi355_wire_bytes(B, (uint64_t)B * n);
    if (one.start()) return 1;
    mi355_core *server = one.server, *client = one.client;
    void *d_wire = ss.dev(server, wire_cap), *d_rx = ss.dev(client, wire_cap), *d_shown = ss.dev(client, (size_t)B * n);
    if (!ss.ok()) return 1;
    std::vector<uint8_t> wire_host(wire_cap), rx(wire_cap), shown((size_t)B * n);
    size_t sent_bytes = 0, changed = 0;
    int max_err = 0;
    for (int t0 = 0; t0 < T; t0 += B) {
        const int nb = T - t0 < B ? T - t0 : B;
        one.cam.fill(one.frames.data(), t0, nb);
        // ---- server: one batch -> the socket bytes of nb frames
        OK(mi355_upload(server, one.d_frames, one.frames.data(), (size_t)nb * n));
        OK(mi355_diff_stream_wire_batch(server, one.d_frames, n, nb, one.d_off, d_wire, wire_cap));
        OK(mi355_download(server, one.off.data(), one.d_off, sizeof(uint32_t) * (nb + 1)));
        const size_t wb = mi355_wire_bytes(nb, one.off[nb]);
        OK(mi355_download(server, wire_host.data(), d_wire, wb));
        changed += one.off[nb];
        // ---- the socket (a pipe here)
        if (!ss.send(wire_host.data(), rx.data(), wb)) return 1;
        sent_bytes += wb;
        // ---- client: parse the headers as opencv.cpp:52 does, hand the bytes to the device
        size_t at = 0;
        for (int k = 0; k < nb; k++) {
            memcpy(&one.counts[k], &rx[at], 4);
            at += 4 + (size_t)5 * one.counts[k];
        }
        if (at != wb) { fprintf(stderr, "stream framing broken\n"); return 1; }
        OK(mi355_upload(client, d_rx, rx.data(), wb));
        OK(mi355_apply_wire_batch(client, d_rx, one.counts.data(), nb, d_shown, n));
        OK(mi355_download(client, shown.data(), d_shown, (size_t)nb * n));
        // ---- checks
        OK(mi355_get_state(server, one.s_state.data()));
        OK(mi355_get_state(client, one.c_state.data()));
        if (same(one.s_state.data(), one.c_state.data(), n, "client state != server state")) return 1;
        if (same(&shown[(size_t)(nb - 1) * n], one.c_state.data(), n, "last shown frame != state")) return 1;
        max_err = std::max(max_err, max_abs_error(shown.data(), one.frames.data(), (size_t)nb * n));
    }
    if (within_threshold(max_err, ss) || ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"width\": %d, \"height\": %d, \"frames\": %d, \"batch\": %d, "
           "\"changed_bytes\": %zu, \"wire_bytes\": %zu, \"raw_bytes\": %zu, \"max_abs_error\": %d}\n",
           w, h, T, B, changed, sent_bytes, (size_t)T * n, max_err);
    return 0;
}

// --compact: the same over the compact wire format (include/mi355diff.h): the server packs a batch and encodes it on the
// GPU (mi355_diff_stream_batch, mi355_cwire_encode_batch), the records cross the same pipe, and the client -- with no
// core and no GPU -- rebuilds every frame on the host with mi355_cwire_apply_host; each rebuilt frame is checked against
// the frame that was sent, and the client's frame against the server's state after every batch.
// --compact --direct: the server makes the records in one call (mi355_diff_stream_cwire_batch), without the xs / diff arrays.
// --compact --gpu-client: the client core also uploads the received records and applies them in one call
// (mi355_apply_cwire_batch) into its shown frames; every shown frame must equal the host client's frame after that record,
// and the client core's state the server's state after every batch.
static int run_single_compact(int w, int h, int T, int B, bool direct, bool gpu_client) {
    Single one(w, h, B);
    Session &ss = one.ss;
    const size_t n = ss.n, cap = (size_t)B * n, cw_cap = mi355_cwire_bytes_max(n, B);
    if (one.start()) return 1;
    mi355_core *server = one.server, *client = one.client;
    // (the one-call form needs no arrays of 5 bytes per entry; only the GPU client needs device buffers at the receiving end)
    void *d_xs = direct ? nullptr : ss.dev(server, cap * 4), *d_df = direct ? nullptr : ss.dev(server, cap);
    void *d_pos = ss.dev(server, sizeof(uint64_t) * (B + 1)), *d_cw = ss.dev(server, cw_cap);
    void *d_rx = gpu_client ? ss.dev(client, cw_cap) : nullptr, *d_shown = gpu_client ? ss.dev(client, (size_t)B * n) : nullptr;
    if (!ss.ok()) return 1;
    std::vector<uint8_t> cw_host(cw_cap), rx(cw_cap), c_frame(one.got_base), shown(gpu_client ? (size_t)B * n : 0);
    std::vector<uint64_t> pos(B + 1);
    std::vector<size_t> at(B + 1);
    size_t sent_bytes = 0, changed = 0;
    int max_err = 0;
    for (int t0 = 0; t0 < T; t0 += B) {
        const int nb = T - t0 < B ? T - t0 : B;
        one.cam.fill(one.frames.data(), t0, nb);
        // ---- sender: pack + encode on the GPU, or both in one call
        OK(mi355_upload(server, one.d_frames, one.frames.data(), (size_t)nb * n));
        if (direct) {
            OK(mi355_diff_stream_cwire_batch(server, one.d_frames, n, nb, one.d_off, d_pos, d_cw, cw_cap));
        } else {
            OK(mi355_diff_stream_batch(server, one.d_frames, n, nb, one.d_off, d_xs, d_df, cap));
            OK(mi355_cwire_encode_batch(server, one.d_off, d_xs, d_df, cap, nb, d_pos, d_cw, cw_cap));
        }
        OK(mi355_download(server, one.off.data(), one.d_off, sizeof(uint32_t) * (nb + 1)));
        OK(mi355_download(server, pos.data(), d_pos, sizeof(uint64_t) * (nb + 1)));
        if (pos[nb] > cw_cap) { fprintf(stderr, "compact stream larger than its bound\n"); return 1; }
        const size_t cb = (size_t)pos[nb];
        OK(mi355_download(server, cw_host.data(), d_cw, cb));
        changed += one.off[nb];
        if (!ss.send(cw_host.data(), rx.data(), cb)) return 1;
        sent_bytes += cb;
        // ---- client: the headers as it reads them from the stream; the GPU client: one upload, one call for the batch
        if (walk_records(rx.data(), 0, cb, nb, one.counts.data(), one.escapes.data(), at.data())) return 1;
        if (gpu_client) {
            OK(mi355_upload(client, d_rx, rx.data(), cb));
            OK(mi355_apply_cwire_batch(client, d_rx, one.counts.data(), one.escapes.data(), nb, d_shown, n));
            OK(mi355_download(client, shown.data(), d_shown, (size_t)nb * n));
        }
        for (int k = 0; k < nb; k++) {   // the host client, one frame at a time: what the client shows after each
            if (host_apply(c_frame.data(), n, rx.data(), at.data(), k)) return 1;
            if (gpu_client && same(&shown[(size_t)k * n], c_frame.data(), n, "GPU client frame != host client frame", t0 + k)) return 1;
            max_err = std::max(max_err, max_abs_error(c_frame.data(), &one.frames[(size_t)k * n], n));
        }
        OK(mi355_get_state(server, one.s_state.data()));
        if (same(one.s_state.data(), c_frame.data(), n, "client frame != server state")) return 1;
        if (gpu_client) {
            OK(mi355_get_state(client, one.c_state.data()));
            if (same(one.s_state.data(), one.c_state.data(), n, "GPU client state != server state")) return 1;
        }
    }
    if (within_threshold(max_err, ss) || ss.close()) return 1;
    printf("{\"roundtrip\": \"ok\", \"format\": \"compact\", \"direct\": %s, \"gpu_client\": %s, \"width\": %d, \"height\": %d, \"frames\": %d, \"batch\": %d, "
           "\"changed_bytes\": %zu, \"wire_bytes\": %zu, \"reference_wire_bytes\": %zu, \"raw_bytes\": %zu, "
           "\"max_abs_error\": %d}\n",
           direct ? "true" : "false", gpu_client ? "true" : "false", w, h, T, B, changed, sent_bytes, mi355_wire_bytes(T, changed), (size_t)T * n, max_err);
    return 0;
}

static int run_single(int w, int h, int T, int B, bool compact, bool direct, bool gpu_client) {
    return compact ? run_single_compact(w, h, T, B, direct, gpu_client) : run_single_wire(w, h, T, B);
}

static int usage(const char *text) {
    fprintf(stderr, "%s\n", text);
    return 2;
}

int main(int argc, char **argv) {
    long w = 320, h = 180, T = 24, B = 8, multi = 0, burst = 0, activity = -1, resync = -1, wall = 0, budget = -1, datagram = -1, thumb = 0, thumb_drop = -1, despeckle = -1;
    bool compact = false, direct = false, gpu_client = false, burst_client = false, coalesce = false, per_frame = false, check = false;
    const struct { const char *name; bool *on; } flags[] = {
        {"--compact", &compact}, {"--direct", &direct}, {"--gpu-client", &gpu_client}, {"--burst-client", &burst_client},
        {"--coalesce", &coalesce}, {"--per-frame", &per_frame}, {"--check", &check}, {"--runs", &g_runs}};
    const long any = INT32_MIN;   // (no least value)
    const struct { const char *name; long *value, least, below; } valued[] = {   // a value below `least` is taken as `below`
        {"--width", &w, any, 0}, {"--height", &h, any, 0}, {"--frames", &T, any, 0}, {"--batch", &B, any, 0}, {"--multi", &multi, any, 0},
        {"--burst", &burst, any, 0}, {"--activity", &activity, 0, 0}, {"--resync", &resync, 0, 0}, {"--wall", &wall, 1, -1},
        {"--budget", &budget, 0, 0}, {"--datagram", &datagram, 0, 0}, {"--thumb", &thumb, 1, -1}, {"--thumb-drop", &thumb_drop, 0, -2},
        {"--despeckle", &despeckle, 0, -2}};
    int32_t crop[4] = {0, 0, 0, 0};
    bool cropped = false, crop_ok = true;
    int grid[2] = {0, 0};
    bool mosaic = false, mosaic_ok = true;
    int fec[2] = {0, 0};
    bool fec_on = false, fec_ok = true;
    for (int i = 1; i < argc; i++) {   // (an option the tool does not know is ignored)
        if (!strcmp(argv[i], "--fec") && i + 1 < argc) {
            char tail = 0;
            fec_on = true;
            fec[1] = 1;
            const int got = sscanf(argv[++i], "%d,%d%c", &fec[0], &fec[1], &tail);
            fec_ok = got == 1 || got == 2;
            continue;
        }
        if (!strcmp(argv[i], "--crop") && i + 1 < argc) {
            char tail = 0;
            cropped = true;
            crop_ok = sscanf(argv[++i], "%d,%d,%d,%d%c", &crop[0], &crop[1], &crop[2], &crop[3], &tail) == 4;
            continue;
        }
        if (!strcmp(argv[i], "--mosaic") && i + 1 < argc) {
            char tail = 0;
            mosaic = true;
            mosaic_ok = sscanf(argv[++i], "%dx%d%c", &grid[0], &grid[1], &tail) == 2;
            continue;
        }
        for (const auto &f : flags)
            if (!strcmp(argv[i], f.name)) *f.on = true;
        for (const auto &v : valued)
            if (!strcmp(argv[i], v.name) && i + 1 < argc) {
                const long x = atol(argv[++i]);
                *v.value = x < v.least ? v.below : x;
                break;
            }
    }
    if (direct && !compact) return usage("--direct needs --compact");
    if (gpu_client && !compact) return usage("--gpu-client needs --compact");
    if (burst && (!multi || burst < 0)) return usage("--burst K needs --multi S and K >= 1");
    if (burst_client && (!compact || !multi || !burst)) return usage("--burst-client needs --compact --multi S --burst K");
    if (coalesce && (!compact || !multi || !burst || burst_client)) return usage("--coalesce needs --compact --multi S --burst K, without --burst-client");
    if (budget >= 0 && (!compact || !multi || burst || direct || gpu_client || per_frame)) return usage("--budget BYTES needs --compact --multi S alone");
    if (activity >= 0 && (activity == 0 || !compact || !multi || budget >= 0 || coalesce || (burst && !burst_client)))
        return usage("--activity CELL needs CELL >= 1 and --compact --multi S, alone or with --burst K --burst-client");
    if (activity < 0) activity = 0;
    if (check && (!compact || !multi || budget >= 0 || coalesce || per_frame || (burst && !burst_client)))
        return usage("--check needs --compact --multi S, alone or with --burst K --burst-client");
    if (resync >= 0 && (!compact || !multi || budget >= 0 || coalesce || per_frame || burst_client || activity || check))
        return usage("--resync K needs --compact --multi S, alone or with --burst B");
    if (wall && (wall < 0 || wall > 16 || !compact || !multi || budget >= 0 || coalesce || per_frame || (burst && !burst_client && resync < 0)))
        return usage("--wall K needs 1 <= K <= 16 and --compact --multi S, alone, with --burst B --burst-client or with --resync R");
    if (cropped) {
        if (!compact || !multi || budget >= 0 || coalesce || per_frame || burst_client || activity || check || resync >= 0 || wall)
            return usage("--crop X,Y,W,H needs --compact --multi S, alone or with --burst K");
        if (!crop_ok || crop[0] < 0 || crop[1] < 0 || crop[2] < 1 || crop[3] < 1 || (long)crop[0] + crop[2] > w || (long)crop[1] + crop[3] > h)
            return usage("--crop X,Y,W,H needs a rectangle of at least one pixel inside the frame");
    }
    if (mosaic) {
        if (!compact || !multi || cropped || budget >= 0 || coalesce || per_frame || burst_client || activity || check || resync >= 0 || wall)
            return usage("--mosaic CxR needs --compact --multi S, alone or with --burst K");
        if (!mosaic_ok || grid[0] < 1 || grid[1] < 1 || (long)grid[0] * grid[1] < multi || (long)grid[0] * grid[1] > 4096 ||
            3.0 * w * h * grid[0] * grid[1] >= 2147483648.0)
            return usage("--mosaic CxR needs C, R >= 1, S <= C*R <= 4096 cells and a canvas below 2^31 bytes");
    }
    if (datagram >= 0) {
        if (!compact || !multi || cropped || mosaic || budget >= 0 || per_frame || burst_client || activity || check || resync >= 0 || wall ||
            (burst && !coalesce))
            return usage("--datagram BYTES needs --compact --multi S, alone or behind --burst K --coalesce");
        if (datagram < 64 || datagram > (long)MI355_CWIRE_SPLIT_BLOCK || datagram % 4)
            return usage("--datagram BYTES needs a multiple of 4 in [64, 65536]");
    }
    if (fec_on && (datagram < 0 || !fec_ok || fec[0] < 1 || fec[0] > 255 || fec[1] < 1 || fec[1] > 2))
        return usage("--fec G[,K] needs --datagram BYTES, G in 1 .. 255 and K = 1 or 2");
    if (thumb || thumb_drop != -1) {
        if (thumb < 1 || thumb > 16 || !compact || !multi || cropped || mosaic || datagram >= 0 || budget >= 0 || coalesce || per_frame ||
            burst_client || activity || check || resync >= 0 || wall)
            return usage("--thumb K needs 1 <= K <= 16 and --compact --multi S, alone or with --burst T");
        if (thumb_drop < -1 || thumb_drop >= T) return usage("--thumb-drop TICK needs --thumb K and 0 <= TICK < --frames");
    }
    if (g_runs && (!compact || !multi || datagram >= 0 || cropped || budget >= 0 || thumb || per_frame))
        return usage("--runs needs --compact --multi S, alone or with --burst K [--burst-client | --coalesce], --mosaic CxR or --resync K; not with --datagram");
    if (despeckle != -1 && (despeckle < 0 || despeckle > 8 || !compact || !multi || burst || direct || gpu_client || per_frame || budget >= 0 ||
                            coalesce || burst_client || activity || check || resync >= 0 || wall || cropped || mosaic || datagram >= 0 || thumb ||
                            g_runs))
        return usage("--despeckle NEED needs 0 <= NEED <= 8 and --compact --multi S alone");
    if (per_frame) {
        if (!compact || direct || gpu_client || multi) return usage("--per-frame needs --compact alone");
        return run_per_frame(w, h, T);
    }
    if (!multi) return run_single(w, h, T, B, compact, direct, gpu_client);
    if (!compact || direct || gpu_client || multi < 0) return usage("--multi S needs --compact alone and S >= 1");
    if (thumb) return run_multi_thumb(w, h, T, multi, burst, thumb, thumb_drop);
    if (resync >= 0) return run_multi_resync(w, h, T, multi, resync, burst, wall);
    if (cropped) return run_multi_crop(w, h, T, multi, burst, crop);
    if (mosaic) return run_multi_mosaic(w, h, T, multi, burst, grid[0], grid[1]);
    if (datagram >= 0) return run_multi_datagram(w, h, T, multi, coalesce ? burst : 0, datagram, fec[0], fec[1]);
    if (coalesce) return run_multi_burst_coalesce(w, h, T, multi, burst);
    if (budget >= 0) return run_multi_budget(w, h, T, multi, budget);
    if (despeckle >= 0) return run_multi_despeckle(w, h, T, multi, despeckle);
    if (burst && !burst_client) return run_multi_burst(w, h, T, multi, burst);
    return run_multi(w, h, T, multi, burst, activity, check, wall);   // (burst == 0: tick by tick)
}

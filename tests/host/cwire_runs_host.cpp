// cwire_runs_host.cpp -- the two host forms of the run-coded records (include/mi355diff.h, "Run-coded records") from plain C++,
// with its own main: records of several index patterns are encoded under both policies into exactly sized heap buffers, decoded,
// and compared with the input; the sizes are checked against the formula.  Built by tests/test_cwire_runs_abi.py against the
// library; with the host sanitizers it is the memory check of the two functions (exact-size buffers: one byte too far is seen).
//   c++ -std=c++17 -I include tests/host/cwire_runs_host.cpp cudavideostream_amd/libmi355diff.so -o cwire_runs_host
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mi355diff.h"

static size_t pad4(size_t x) { return (x + 3) & ~(size_t)3; }

// the compact record of the ascending indices xs
static std::vector<uint8_t> record(const std::vector<uint32_t> &xs) {
    std::vector<uint8_t> code(pad4(xs.size())), diff(pad4(xs.size()));
    std::vector<uint32_t> esc;
    uint32_t end = 0;
    for (size_t k = 0; k < xs.size(); k++) {
        const uint32_t g = xs[k] - end;
        end = xs[k] + 1;
        code[k] = (uint8_t)(g < 255 ? g : 255);
        if (g >= 255) esc.push_back(g);
        diff[k] = (uint8_t)(1 + k % 255);
    }
    const uint32_t head[2] = {(uint32_t)xs.size(), (uint32_t)esc.size()};
    std::vector<uint8_t> out(8 + 2 * code.size() + 4 * esc.size());
    memcpy(out.data(), head, 8);
    if (!code.empty()) memcpy(out.data() + 8, code.data(), code.size());
    if (!esc.empty()) memcpy(out.data() + 8 + code.size(), esc.data(), 4 * esc.size());
    if (!diff.empty()) memcpy(out.data() + 8 + code.size() + 4 * esc.size(), diff.data(), diff.size());
    return out;
}

static int fail(const char *what, int policy) {
    fprintf(stderr, "FAILED: %s (policy %d): %s\n", what, policy, mi355_last_error());
    return 1;
}

int main() {
    const uint32_t N = 57600;
    std::vector<std::vector<uint32_t>> pats;
    pats.push_back({});
    pats.push_back({0});
    pats.push_back({N - 1});
    {
        std::vector<uint32_t> v;
        for (uint32_t i = 0; i < N; i++) v.push_back(i);
        pats.push_back(v);
    }
    {
        std::vector<uint32_t> v;
        for (uint32_t i = 0; i < N; i += 2) v.push_back(i);
        pats.push_back(v);
    }
    for (uint32_t n : {255u, 256u, 257u, 4095u, 4096u, 4097u}) {
        std::vector<uint32_t> v;
        for (uint32_t i = 0; i < n; i++) v.push_back(1 + i);
        pats.push_back(v);
    }
    {
        std::vector<uint32_t> v;   // a 255 code at entries 256 and 4096
        for (uint32_t i = 0; i < 4200; i++) v.push_back(i + (i >= 256 ? 300 : 0) + (i >= 4096 ? 300 : 0));
        pats.push_back(v);
    }
    {
        std::vector<uint32_t> v;   // runs of 1 .. 700 entries, a seeded mix
        uint32_t x = 3, s = 12345;
        for (;;) {
            s = s * 1664525u + 1013904223u;
            const uint32_t len = 1 + (s >> 8) % 700, gap = 1 + (s >> 20) % 600;
            if (x + len > N) break;
            for (uint32_t i = 0; i < len; i++) v.push_back(x + i);
            x += len + gap;
        }
        pats.push_back(v);
    }
    std::vector<uint8_t> in;
    std::vector<uint32_t> counts, escapes;
    for (const auto &xs : pats) {
        const std::vector<uint8_t> rec = record(xs);
        uint32_t head[2];
        memcpy(head, rec.data(), 8);
        counts.push_back(head[0]);
        escapes.push_back(head[1]);
        in.insert(in.end(), rec.begin(), rec.end());
    }
    const int nrec = (int)pats.size();
    for (int policy : {MI355_RUNS_WHERE_SMALLER, MI355_RUNS_ALWAYS}) {
        std::vector<uint32_t> forms(4 * (size_t)nrec);
        std::vector<uint64_t> pos((size_t)nrec + 1), frame_pos((size_t)nrec + 1);
        // a first pass with no room at all gives the exact sizes ...
        uint8_t none = 0;
        if (mi355_cwire_runs_encode_host(N, in.data(), in.size(), counts.data(), escapes.data(), nrec, policy, forms.data(), pos.data(), &none, 0))
            return fail("sizing pass", policy);
        if (pos[nrec] > mi355_cwire_runs_bytes_max(N, nrec, policy)) return fail("bytes_max is below the output", policy);
        // ... and the second one writes into exactly that many bytes
        std::vector<uint8_t> link((size_t)pos[nrec]);
        if (mi355_cwire_runs_encode_host(N, in.data(), in.size(), counts.data(), escapes.data(), nrec, policy, forms.data(), pos.data(),
                                         link.data(), link.size()))
            return fail("encode", policy);
        for (int b = 0; b < nrec; b++) {
            const uint32_t *f = &forms[4 * (size_t)b];
            const size_t want = f[0] == MI355_RUNS_FORM_RUNS ? mi355_cwire_runs_frame_bytes(f[1], f[2], f[3]) : mi355_cwire_frame_bytes(f[1], f[2]);
            if (pos[b + 1] - pos[b] != want || f[1] != counts[b] || f[2] != escapes[b]) return fail("forms / pos", policy);
            if (policy == MI355_RUNS_WHERE_SMALLER && want > mi355_cwire_frame_bytes(f[1], f[2])) return fail("larger than compact", policy);
        }
        std::vector<uint8_t> back(in.size());
        if (mi355_cwire_runs_decode_host(N, link.data(), link.size(), forms.data(), nrec, frame_pos.data(), back.data(), back.size()))
            return fail("decode", policy);
        if (frame_pos[nrec] != in.size() || memcmp(back.data(), in.data(), in.size()) != 0) return fail("round trip", policy);
        // a truncated link is refused
        if (mi355_cwire_runs_decode_host(N, link.data(), link.size() - 4, forms.data(), nrec, frame_pos.data(), back.data(), back.size()) !=
            MI355_ERR_INVALID)
            return fail("truncated input accepted", policy);
    }
    printf("ok: %d records, %zu bytes\n", nrec, in.size());
    return 0;
}

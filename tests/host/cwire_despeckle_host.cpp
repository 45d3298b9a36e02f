// cwire_despeckle_host.cpp -- the host form of the despeckle call (include/mi355diff.h, "A tick without its speckle") from plain
// C++, with its own main: records of pseudo-random pixel sets on several shapes, every need 0 .. 8, exactly sized heap buffers
// (the state with no byte behind its N), the result compared with a plain count over the eight neighbours.  Built by
// tests/test_cwire_despeckle_spec.py against the library; with the host sanitizers it is the memory check of the function.
//   c++ -std=c++17 -I include tests/host/cwire_despeckle_host.cpp cudavideostream_amd/libmi355diff.so -o cwire_despeckle_host
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mi355diff.h"

static size_t pad4(size_t x) { return (x + 3) & ~(size_t)3; }

// the compact record of the ascending indices xs with the differences df
static std::vector<uint8_t> record(const std::vector<uint32_t> &xs, const std::vector<uint8_t> &df, uint32_t *e_out) {
    std::vector<uint8_t> code(pad4(xs.size())), diff(pad4(xs.size()));
    std::vector<uint32_t> esc;
    uint32_t end = 0;
    for (size_t k = 0; k < xs.size(); k++) {
        const uint32_t g = xs[k] - end;
        end = xs[k] + 1;
        code[k] = (uint8_t)(g < 255 ? g : 255);
        if (g >= 255) esc.push_back(g);
        diff[k] = df[k];
    }
    const uint32_t head[2] = {(uint32_t)xs.size(), (uint32_t)esc.size()};
    std::vector<uint8_t> out(8 + 2 * code.size() + 4 * esc.size());
    memcpy(out.data(), head, 8);
    if (!code.empty()) memcpy(out.data() + 8, code.data(), code.size());
    if (!esc.empty()) memcpy(out.data() + 8 + code.size(), esc.data(), 4 * esc.size());
    if (!diff.empty()) memcpy(out.data() + 8 + code.size() + 4 * esc.size(), diff.data(), diff.size());
    *e_out = (uint32_t)esc.size();
    return out;
}

static uint32_t rnd(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

int main() {
    const int shapes[][2] = {{37, 11}, {64, 48}, {1400, 3}, {1, 64}, {2, 40}, {64, 1}};
    int runs = 0;
    for (const auto &sh : shapes) {
        const int w = sh[0], h = sh[1];
        const uint32_t P = (uint32_t)w * h, N = 3 * P;
        for (uint32_t per_mille : {50u, 300u, 700u}) {
            uint32_t seed = 7 * w + h + per_mille;
            std::vector<uint8_t> changed(P, 0);
            std::vector<uint32_t> xs;
            std::vector<uint8_t> df;
            for (uint32_t p = 0; p < P; p++) {
                if (rnd(seed) % 1000 >= per_mille) continue;
                changed[p] = 1;
                const uint32_t first = rnd(seed) % 3;
                for (uint32_t c = 0; c < 3; c++)
                    if (c == first || rnd(seed) % 2) {
                        xs.push_back(3 * p + c);
                        df.push_back((uint8_t)(1 + rnd(seed) % 255));
                    }
            }
            uint32_t e = 0;
            const std::vector<uint8_t> rec = record(xs, df, &e);
            const uint32_t n = (uint32_t)xs.size();
            for (uint32_t need = 0; need <= 8; need++) {
                std::vector<uint8_t> state(N, 100);
                for (size_t k = 0; k < xs.size(); k++) state[xs[k]] = (uint8_t)(100 + df[k]);
                // the expectation, by a plain count
                std::vector<uint32_t> kx;
                std::vector<uint8_t> kd, want_state = state;
                for (size_t k = 0; k < xs.size(); k++) {
                    const int p = (int)(xs[k] / 3), px = p % w, py = p / w;
                    uint32_t c = 0;
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++)
                            if ((dx || dy) && px + dx >= 0 && px + dx < w && py + dy >= 0 && py + dy < h) c += changed[(py + dy) * w + px + dx];
                    if (need == 0 || c >= need) {
                        kx.push_back(xs[k]);
                        kd.push_back(df[k]);
                    } else {
                        want_state[xs[k]] = 100;
                    }
                }
                uint32_t we = 0;
                const std::vector<uint8_t> want = record(kx, kd, &we);
                std::vector<uint8_t> out(want.size());   // exactly what is needed
                uint32_t dropped = 77, offsets[2] = {77, 77};
                uint64_t pos[2] = {77, 77};
                const int rc = mi355_cwire_despeckle_host(w, h, rec.data(), rec.size(), &n, &e, state.data(), N, 1, &need, &dropped, offsets, pos,
                                                          out.data(), out.size());
                if (rc != MI355_OK) {
                    fprintf(stderr, "FAILED: %dx%d density %u need %u: %s\n", w, h, per_mille, need, mi355_last_error());
                    return 1;
                }
                if (dropped != n - kx.size() || offsets[0] != 0 || offsets[1] != kx.size() || pos[0] != 0 || pos[1] != want.size() ||
                    out != want || state != want_state) {
                    fprintf(stderr, "FAILED: %dx%d density %u need %u: the result differs from the plain count\n", w, h, per_mille, need);
                    return 1;
                }
                runs++;
            }
        }
    }
    // a refusal writes nothing
    {
        const uint32_t n = 1, e = 0, need = 9;
        uint32_t dropped = 77, offsets[2] = {77, 77};
        uint64_t pos[2] = {77, 77};
        uint8_t rec[16] = {1, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 9, 0, 0, 0}, state[12], out[16];
        memset(state, 100, sizeof state);
        memset(out, 0x5C, sizeof out);
        if (mi355_cwire_despeckle_host(2, 2, rec, sizeof rec, &n, &e, state, 12, 1, &need, &dropped, offsets, pos, out, sizeof out) !=
                MI355_ERR_INVALID ||
            dropped != 77 || offsets[0] != 77 || pos[1] != 77 || out[0] != 0x5C || state[5] != 100) {
            fprintf(stderr, "FAILED: need 9 was not refused cleanly\n");
            return 1;
        }
    }
    printf("ok: %d runs\n", runs);
    return 0;
}

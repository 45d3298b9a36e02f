// tools/diffbench.hip -- C++ harness over the C-ABI (include/mi355diff.h): the same workload as
// bench.py (S1 `webcam` stream, B frames resident in HBM, stateful diff+threshold+pack) without
// Python/PyTorch in the process.  Used for the rocprofv3 --pmc passes (the counter-collection
// interposer crashes under PyTorch's own kernels on this image) and as a plain C++ example of the
// boundary.  The synthetic generator is a device-side restatement of cudavideostream_amd/synth.py
// (tests/test_tools_gpu.py checks the two produce identical bytes).
//
//   diffbench [--width W] [--height H] [--batch B] [--steps K] [--warmup W] [--seed S]
//             [--pairs] [--checksum T] [--cores C] [--digest]
//             [--regime s0|flip|static] [--apart]   pairs of the dense / static regimes; pairs that share no frame
//             [--lib-alloc]             the two output arrays from mi355_alloc_outputs (a pair placed for the dense expansion)
//   diffbench --consecutive [--width W] [--height H] [--batch B] [--steps K]   mi355_diff_consecutive_batch on one buffer of
//                                                   B + 1 frames, then mi355_diff_pairs_batch on the same views: us per pair
//                                                   of both, and whether offsets and entries are equal (exit 5 if not)
//   diffbench --filters [--batch B] [--steps K]     the filter kernels and the BASELINE config 3 / 4 chains
//                                                   (same lines as tools/bench_filters.py, for the --pmc passes)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/mi355diff.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(3); } } while (0)
#define MI_OK(x) do { int r_ = (x); if (r_ != 0) { fprintf(stderr, "%s: %s\n", #x, mi355_last_error()); exit(4); } } while (0)

__host__ __device__ inline uint32_t hash32(uint32_t x) {  // lowbias32, synth.py hash32
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// synth.py webcam_frame(t, width, height, seed): t = -1 is the base frame.
__global__ void k_webcam_frame(uint8_t *out, int t, int width, int height, uint32_t seed) {
    const uint32_t n = 3u * width * height;
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const uint32_t tt = (uint32_t)(t + 1) & 0xFFFFu;
    const uint32_t key = hash32(hash32(idx) + tt * 0x9E3779B9u + seed * 0x85EBCA6Bu);
    const int nz = (int)((key & 0xFFFFu) % 17u) - 8;
    const uint32_t pix = idx / 3u;
    const int c = (int)(idx - pix * 3u);
    const int y = (int)(pix / (uint32_t)width), x = (int)(pix % (uint32_t)width);
    const int tex = (int)((hash32(idx + 0x5BD1E995u) >> 8) % 7u);
    int val = 40 + (x * 150) / width + (y * 40) / height + 5 * c + tex;
    if (t >= 0) {
        const int rw = width / 4, rh = height / 4;
        const int speed = width / 240 > 1 ? width / 240 : 1;
        const int x0 = (t * speed) % (width - rw), y0 = height / 3;
        if (x >= x0 && x < x0 + rw && y >= y0 && y < y0 + rh) val = 120 + 10 * c + (x - x0) / 16;
    }
    val += nz;
    if (t >= 0 && ((key >> 16) & 0xFFFFu) < 786u) val = (int)(hash32(key ^ 0xABCDEFu) & 0xFFu);
    out[idx] = (uint8_t)(val < 0 ? 0 : val > 255 ? 255 : val);
}

// synth.py refrand_frame(n, seed): S0, bytes uniform on 0..254 (the generator of tests/algorithms_benchmarks.cu:4-10);
// flip != 0: the same frame with bit 7 of every byte flipped (P = N against the unflipped one)
__global__ void k_refrand_frame(uint8_t *out, uint32_t n, uint32_t seed, int flip) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const uint32_t v = hash32(hash32(idx) + seed * 0x85EBCA6Bu) % 255u;
    out[idx] = (uint8_t)(flip ? v ^ 0x80u : v);
}

// --corun valu|mem|lds: a background kernel of single-wave workgroups on a stream of its own while the timed batches run
// (what does the pack kernel share with a co-runner: issue slots or the memory system?).  Experiment only.
__global__ __launch_bounds__(64) void k_corun_valu(uint32_t *out, int iters) {
    uint32_t a = threadIdx.x * 2654435761u, b = blockIdx.x + 17u, c = a ^ 0x9e3779b9u, d = b + a;
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int k = 0; k < 16; k++) { a = (a | 0x80808080u) - (b & 0x7f7f7f7fu); b = (b ^ c) + d; c = (c + a) ^ (d >> 3); d = d * 5u + b; }
    }
    if ((a ^ b ^ c ^ d) == 0x12345u) out[0] = a;
}
__global__ __launch_bounds__(64) void k_corun_mem(const uint4 *buf, size_t nvec, uint32_t *out, int iters) {
    uint32_t x = (blockIdx.x * 64u + threadIdx.x) * 2654435761u, acc = 0;
    for (int i = 0; i < iters; i++) {   // every group of 4 lanes reads one random 64-byte piece
        x = x * 1664525u + 1013904223u;
        const uint32_t piece = __builtin_amdgcn_readfirstlane(0) + ((x >> 2) | 0u);
        const size_t idx = (((size_t)(piece ^ (threadIdx.x >> 2) * 0x9E3779B1u)) % (nvec / 4)) * 4 + (threadIdx.x & 3);
        const uint4 v = buf[idx];
        acc += v.x ^ v.w;
    }
    if (acc == 0x12345u) out[0] = acc;
}

int main(int argc, char **argv) {
    int W = 1920, H = 1080, B = 256, K = 20, WU = 3, checksum_t = -2, ncores = 1;
    uint32_t seed = 21;
    bool pairs = false, filters = false, digest = false, apart = false, consecutive = false;
    bool lib_alloc = false;   // the two output arrays from mi355_alloc_outputs (a pair placed for the dense expansion)
    const char *corun = nullptr; int corun_blocks = 2048;
    const char *regime = nullptr;   // --regime s0|flip|static: pairs of the dense / static regimes (tools/bench_regimes.py's inputs)
    for (int i = 1; i < argc; i++) {
        auto next = [&](int &v) { if (i + 1 < argc) v = atoi(argv[++i]); };
        if (!strcmp(argv[i], "--width")) next(W);
        else if (!strcmp(argv[i], "--height")) next(H);
        else if (!strcmp(argv[i], "--batch")) next(B);
        else if (!strcmp(argv[i], "--steps")) next(K);
        else if (!strcmp(argv[i], "--warmup")) next(WU);
        else if (!strcmp(argv[i], "--seed")) { int s = 21; next(s); seed = (uint32_t)s; }
        else if (!strcmp(argv[i], "--checksum")) next(checksum_t);
        else if (!strcmp(argv[i], "--pairs")) pairs = true;
        else if (!strcmp(argv[i], "--apart")) { pairs = true; apart = true; }   // pairs (0,1), (2,3), ...: no frame is an operand twice (round-robin sharding)
        else if (!strcmp(argv[i], "--cores")) next(ncores);
        else if (!strcmp(argv[i], "--filters")) filters = true;
        else if (!strcmp(argv[i], "--consecutive")) consecutive = true;
        else if (!strcmp(argv[i], "--digest")) digest = true;
        else if (!strcmp(argv[i], "--corun") && i + 1 < argc) corun = argv[++i];
        else if (!strcmp(argv[i], "--regime") && i + 1 < argc) { regime = argv[++i]; pairs = true; }
        else if (!strcmp(argv[i], "--corun-blocks")) next(corun_blocks);
        else if (!strcmp(argv[i], "--lib-alloc")) lib_alloc = true;
    }
    const size_t n = (size_t)3 * W * H;
    if (checksum_t >= -1) {  // print a checksum of one generated frame (generator cross-check)
        uint8_t *d; HIP_OK(hipMalloc((void **)&d, n));
        hipLaunchKernelGGL(k_webcam_frame, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, checksum_t, W, H, seed);
        std::vector<uint8_t> h(n);
        HIP_OK(hipMemcpy(h.data(), d, n, hipMemcpyDeviceToHost));
        uint64_t s1 = 0, s2 = 0;
        for (size_t i = 0; i < n; i++) { s1 += h[i]; s2 += (uint64_t)h[i] * (uint64_t)(i % 65521 + 1); }
        printf("{\"frame\": %d, \"sum\": %llu, \"wsum\": %llu}\n", checksum_t, (unsigned long long)s1, (unsigned long long)s2);
        return 0;
    }

    mi355_config cfg{};
    cfg.width = W; cfg.height = H; cfg.threshold = 20; cfg.max_batch = B; cfg.device = -1;
    if (ncores > 1) {   // several independent streams, one core (own HIP stream) each, submitted round-robin
        std::vector<mi355_core *> cores(ncores);
        std::vector<uint8_t *> fr(ncores);
        std::vector<uint32_t *> off(ncores);
        std::vector<int32_t *> xs(ncores);
        std::vector<uint8_t *> df(ncores);
        const size_t cap = (size_t)B * n / 8 > (1u << 20) ? (size_t)B * n / 8 : (1u << 20);
        const dim3 g((unsigned)((n + 255) / 256)), b(256);
        std::vector<uint8_t> h_base(n);
        for (int c = 0; c < ncores; c++) {
            MI_OK(mi355_create(&cfg, &cores[c]));
            HIP_OK(hipMalloc((void **)&fr[c], n * (size_t)(B + 1)));
            for (int t = -1; t < B; t++)
                hipLaunchKernelGGL(k_webcam_frame, g, b, 0, 0, fr[c] + (size_t)(t + 1) * n, t, W, H, seed + c);
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(h_base.data(), fr[c], n, hipMemcpyDeviceToHost));
            MI_OK(mi355_set_state(cores[c], h_base.data()));
            HIP_OK(hipMalloc((void **)&off[c], sizeof(uint32_t) * (B + 1)));
            HIP_OK(hipMalloc((void **)&xs[c], sizeof(int32_t) * cap));
            HIP_OK(hipMalloc((void **)&df[c], cap));
        }
        auto round = [&]() {
            for (int c = 0; c < ncores; c++)
                MI_OK(mi355_diff_stream_batch(cores[c], fr[c] + n, n, B, off[c], xs[c], df[c], cap));
        };
        for (int i = 0; i < WU; i++) round();
        for (int c = 0; c < ncores; c++) MI_OK(mi355_synchronize(cores[c]));
        const auto t0 = std::chrono::high_resolution_clock::now();
        for (int i = 0; i < K; i++) round();
        for (int c = 0; c < ncores; c++) MI_OK(mi355_synchronize(cores[c]));
        const double sec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        printf("{\"harness\": \"diffbench\", \"mode\": \"stream\", \"cores\": %d, \"batch\": %d, \"steps\": %d, "
               "\"frames_per_s\": %.1f, \"ms_per_round\": %.4f}\n",
               ncores, B, K, (double)ncores * B * K / sec, sec / K * 1e3);
        for (auto c : cores) mi355_destroy(c);
        return 0;
    }
    if (filters) {   // mi355_filter_batch per kernel, then the two chains; B frames resident, K repetitions each
        mi355_core *core = nullptr;
        MI_OK(mi355_create(&cfg, &core));
        uint8_t *fr, *out, *filt; uint32_t *off; int32_t *xs; uint8_t *df;
        const size_t cap = (size_t)B * n / 4;
        HIP_OK(hipMalloc((void **)&fr, n * (size_t)(B + 1)));
        HIP_OK(hipMalloc((void **)&out, n * (size_t)B));
        HIP_OK(hipMalloc((void **)&filt, n * (size_t)B));
        HIP_OK(hipMalloc((void **)&off, sizeof(uint32_t) * (B + 1)));
        HIP_OK(hipMalloc((void **)&xs, sizeof(int32_t) * cap));
        HIP_OK(hipMalloc((void **)&df, cap));
        const dim3 g((unsigned)((n + 255) / 256)), b(256);
        for (int t = 0; t <= B; t++) hipLaunchKernelGGL(k_webcam_frame, g, b, 0, 0, fr + (size_t)t * n, t - 1, W, H, seed);
        HIP_OK(hipDeviceSynchronize());
        std::vector<uint8_t> h_base(n);
        HIP_OK(hipMemcpy(h_base.data(), fr, n, hipMemcpyDeviceToHost));
        MI_OK(mi355_set_state(core, h_base.data()));
        float k9[9];   // a normalised 3x3 Gaussian, sigma 1.5 (symmetric like the server's)
        { double s = 0; for (int i = 0; i < 9; i++) { const int y = i / 3 - 1, x = i % 3 - 1; k9[i] = (float)exp(-(x * x + y * y) / 4.5); s += k9[i]; }
          for (float &v : k9) v = (float)(v / s); }
        MI_OK(mi355_set_conv_kernel(core, k9));
        const uint8_t *cur = fr + n, *prev = fr;
        struct Op { const char *name; int op; bool two; double alg; };
        const double N = (double)n;
        const Op ops[] = {{"gray_avg", MI355_OP_GRAY_AVG, false, 2 * N}, {"gray_weighted", MI355_OP_GRAY_WEIGHTED, false, 2 * N},
                          {"gray_weighted+binarize fused (config 3 visualiser)", MI355_OP_GRAY_WEIGHTED_BINARIZE, false, 3 * N},
                          {"heat_map", MI355_OP_HEAT_MAP, true, 3 * N}, {"red_dense", MI355_OP_RED_DENSE, true, 3 * N},
                          {"conv3x3", MI355_OP_CONV3X3, false, 2 * N}, {"median5x5", MI355_OP_MEDIAN5X5, false, 2 * N}};
        auto timed = [&](const char *kind, const char *name, double alg, auto fn) {
            for (int i = 0; i < 2; i++) fn();
            MI_OK(mi355_synchronize(core));
            const auto t0 = std::chrono::high_resolution_clock::now();
            for (int i = 0; i < K; i++) fn();
            MI_OK(mi355_synchronize(core));
            const double us = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count() * 1e6 / ((double)K * B);
            printf("{\"%s\": \"%s\", \"us_per_frame\": %.3f, \"algorithmic_bytes_per_frame\": %.0f, \"achieved_gbps\": %.1f, \"frac_of_8TBps\": %.4f, \"batch\": %d}\n",
                   kind, name, us, alg, alg / (us * 1e-6) / 1e9, alg / (us * 1e-6) / 1e9 / 8000.0, B);
        };
        for (const Op &o : ops)
            timed("filter", o.name, o.alg, [&]() { MI_OK(mi355_filter_batch(core, o.op, cur, o.two ? prev : nullptr, out, n, B)); });
        uint32_t h_tot = 0;
        timed("chain", "config 3: gray-weighted + binarize + diff/threshold/pack", 4 * N, [&]() {
            MI_OK(mi355_filter_batch(core, MI355_OP_GRAY_WEIGHTED_BINARIZE, cur, nullptr, out, n, B));
            MI_OK(mi355_diff_stream_batch(core, cur, n, B, off, xs, df, cap)); });
        timed("chain", "config 4: noise filter + diff/threshold/pack + red motion map", 5 * N, [&]() {
            MI_OK(mi355_filter_batch(core, MI355_OP_CONV3X3, cur, nullptr, filt, n, B));
            MI_OK(mi355_diff_stream_batch(core, filt, n, B, off, xs, df, cap));
            MI_OK(mi355_red_stream_batch(core, off, xs, B, out, n, 1)); });
        HIP_OK(hipMemcpy(&h_tot, off + B, sizeof h_tot, hipMemcpyDeviceToHost));
        printf("{\"note\": \"chains: algorithmic bytes above exclude the 5P of the packed stream\", \"last_chain_changed_bytes_per_frame\": %.1f}\n", (double)h_tot / B);
        mi355_destroy(core);
        return 0;
    }
    if (consecutive) {   // ONE buffer of B + 1 frames; frame t against frame t - 1: the new call, then the pair form on the same views
        mi355_core *core = nullptr;
        MI_OK(mi355_create(&cfg, &core));
        uint8_t *buf = nullptr;
        HIP_OK(hipMalloc((void **)&buf, n * (size_t)(B + 1)));
        const dim3 g((unsigned)((n + 255) / 256)), b(256);
        for (int t = 0; t <= B; t++) hipLaunchKernelGGL(k_webcam_frame, g, b, 0, 0, buf + (size_t)t * n, t - 1, W, H, seed);
        HIP_OK(hipDeviceSynchronize());
        const size_t cap = (size_t)B * n / 8 > (1u << 20) ? (size_t)B * n / 8 : (1u << 20);
        uint32_t *d_off[2]; int32_t *d_xs[2]; uint8_t *d_df[2];
        for (int k = 0; k < 2; k++) {
            HIP_OK(hipMalloc((void **)&d_off[k], sizeof(uint32_t) * (B + 1)));
            HIP_OK(hipMalloc((void **)&d_xs[k], sizeof(int32_t) * cap));
            HIP_OK(hipMalloc((void **)&d_df[k], cap));
            HIP_OK(hipMemset(d_off[k], 0xEE, sizeof(uint32_t) * (B + 1)));
        }
        const uint8_t *first_prev = buf, *frames = buf + n;
        auto step = [&](int k) {
            if (k == 0) MI_OK(mi355_diff_consecutive_batch(core, first_prev, frames, n, B, d_off[0], d_xs[0], d_df[0], cap));
            else MI_OK(mi355_diff_pairs_batch(core, frames, first_prev, n, B, d_off[1], d_xs[1], d_df[1], cap));
        };
        double us[2] = {0, 0};
        for (int k = 0; k < 2; k++) {
            for (int i = 0; i < WU; i++) step(k);
            MI_OK(mi355_synchronize(core));
            const auto t0 = std::chrono::high_resolution_clock::now();
            for (int i = 0; i < K; i++) step(k);
            MI_OK(mi355_synchronize(core));
            us[k] = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count() * 1e6 / ((double)K * B);
        }
        std::vector<uint32_t> off[2];
        bool equal = true;
        for (int k = 0; k < 2; k++) {
            off[k].resize(B + 1);
            HIP_OK(hipMemcpy(off[k].data(), d_off[k], sizeof(uint32_t) * (B + 1), hipMemcpyDeviceToHost));
        }
        equal = off[0] == off[1] && off[0][0] == 0;
        const size_t p = equal ? (off[0][B] < cap ? off[0][B] : cap) : 0;
        if (equal) {
            std::vector<int32_t> hx[2]; std::vector<uint8_t> hd[2];
            for (int k = 0; k < 2; k++) {
                hx[k].resize(p); hd[k].resize(p);
                HIP_OK(hipMemcpy(hx[k].data(), d_xs[k], sizeof(int32_t) * p, hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(hd[k].data(), d_df[k], p, hipMemcpyDeviceToHost));
            }
            equal = hx[0] == hx[1] && hd[0] == hd[1];
        }
        printf("{\"harness\": \"diffbench\", \"mode\": \"consecutive\", \"width\": %d, \"height\": %d, \"batch\": %d, \"steps\": %d, "
               "\"consecutive_us_per_pair\": %.3f, \"pairs_us_per_pair\": %.3f, \"changed_bytes_per_frame\": %.1f, \"outputs\": \"%s\"}\n",
               W, H, B, K, us[0], us[1], (double)off[0][B] / B, equal ? "equal" : "DIFFERENT");
        mi355_destroy(core);
        return equal ? 0 : 5;
    }
    mi355_core *core = nullptr;
    MI_OK(mi355_create(&cfg, &core));

    uint8_t *d_frames = nullptr, *d_base = nullptr;
    const int nfr = apart ? 2 * B : B + 1;
    HIP_OK(hipMalloc((void **)&d_frames, n * (size_t)nfr));
    HIP_OK(hipMalloc((void **)&d_base, n));
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_webcam_frame, g, b, 0, 0, d_base, -1, W, H, seed);
    for (int t = 0; t < nfr; t++)
        hipLaunchKernelGGL(k_webcam_frame, g, b, 0, 0, d_frames + (size_t)t * n, t, W, H, seed);
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint8_t> h_base(n);
    HIP_OK(hipMemcpy(h_base.data(), d_base, n, hipMemcpyDeviceToHost));
    MI_OK(mi355_set_state(core, h_base.data()));

    uint8_t *d_cur = d_frames + n, *d_prev = d_frames;   // pairs: consecutive frames of the stream
    if (regime) {   // cur = refrand(100 + B + t) (s0) / prev ^ 0x80 (flip) / prev (static), prev = refrand(100 + t)
        uint8_t *d_r;
        HIP_OK(hipMalloc((void **)&d_r, n * (size_t)(2 * B)));
        for (int t = 0; t < B; t++) {
            hipLaunchKernelGGL(k_refrand_frame, g, b, 0, 0, d_r + (size_t)t * n, (uint32_t)n, 100u + t, 0);
            const bool s0 = !strcmp(regime, "s0");
            hipLaunchKernelGGL(k_refrand_frame, g, b, 0, 0, d_r + (size_t)(B + t) * n, (uint32_t)n, s0 ? 100u + B + t : 100u + t,
                               !strcmp(regime, "flip") ? 1 : 0);
        }
        HIP_OK(hipDeviceSynchronize());
        d_prev = d_r; d_cur = d_r + (size_t)B * n;
    }
    const size_t cap = regime ? (size_t)B * n : ((size_t)B * n / 8 > (1u << 20) ? (size_t)B * n / 8 : (1u << 20));
    uint32_t *d_off; int32_t *d_xs; uint8_t *d_df;
    HIP_OK(hipMalloc((void **)&d_off, sizeof(uint32_t) * (B + 1)));
    if (lib_alloc) {
        void *a = nullptr, *b2 = nullptr; int draws = 0;
        const auto ta = std::chrono::high_resolution_clock::now();
        MI_OK(mi355_alloc_outputs(core, cap, &a, &b2, &draws));
        fprintf(stderr, "mi355_alloc_outputs: %d value array(s) drawn in %.1f ms\n", draws, std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - ta).count() * 1e3);
        d_xs = (int32_t *)a; d_df = (uint8_t *)b2;
    } else {
        HIP_OK(hipMalloc((void **)&d_xs, sizeof(int32_t) * cap));
        HIP_OK(hipMalloc((void **)&d_df, cap));
    }

    auto step = [&]() {
        if (pairs) MI_OK(mi355_diff_pairs_batch(core, d_cur, d_prev, apart ? 2 * n : n, B, d_off, d_xs, d_df, cap));
        else MI_OK(mi355_diff_stream_batch(core, d_frames, n, B, d_off, d_xs, d_df, cap));
    };
    for (int i = 0; i < WU; i++) step();
    MI_OK(mi355_synchronize(core));
    MI_OK(mi355_set_timing(core, getenv("DIFFBENCH_NO_TIMING") ? 0 : 1));   // per-kernel HIP events (5 per batch) off: what do they cost?
    MI_OK(mi355_reset_timing(core));
    hipStream_t cs = nullptr; uint32_t *d_sink = nullptr; uint4 *d_big = nullptr; const size_t big = (size_t)2 << 30;
    if (corun) {
        HIP_OK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        HIP_OK(hipMalloc((void **)&d_sink, 64));
        if (!strcmp(corun, "mem")) { HIP_OK(hipMalloc((void **)&d_big, big)); HIP_OK(hipMemset(d_big, 1, big)); }
        // long enough to cover the timed region (a few tens of ms)
        if (!strcmp(corun, "valu")) hipLaunchKernelGGL(k_corun_valu, dim3(corun_blocks), dim3(64), 0, cs, d_sink, 400000);
        else hipLaunchKernelGGL(k_corun_mem, dim3(corun_blocks), dim3(64), 0, cs, d_big, big / 16, d_sink, 20000);
    }
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (int i = 0; i < K; i++) step();
    MI_OK(mi355_synchronize(core));
    const double sec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    if (corun) {
        const bool still = hipStreamQuery(cs) == hipErrorNotReady;   // the co-runner must have covered the whole timed region
        HIP_OK(hipStreamSynchronize(cs));
        const double csec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        fprintf(stderr, "corun %s: %d blocks, covered the timed region: %s, ran %.1f ms ", corun, corun_blocks, still ? "yes" : "NO", csec * 1e3);
    }
    double ms_pack = 0, ms_total = 0; int launches = 0;
    MI_OK(mi355_get_timing(core, &ms_pack, &ms_total, &launches));
    std::vector<uint32_t> off(B + 1);
    HIP_OK(hipMemcpy(off.data(), d_off, sizeof(uint32_t) * (B + 1), hipMemcpyDeviceToHost));
    const double p = off[B];
    if (digest) {   // order-sensitive digest of everything the batch produced (A/B builds must agree)
        std::vector<int32_t> hx((size_t)off[B]); std::vector<uint8_t> hd((size_t)off[B]);
        HIP_OK(hipMemcpy(hx.data(), d_xs, sizeof(int32_t) * hx.size(), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(hd.data(), d_df, hd.size(), hipMemcpyDeviceToHost));
        uint64_t h = 1469598103934665603ull;
        for (int t = 0; t <= B; t++) h = (h ^ off[t]) * 1099511628211ull;
        for (size_t i = 0; i < hx.size(); i++) h = (h ^ ((uint64_t)(uint32_t)hx[i] << 8 | hd[i])) * 1099511628211ull;
        fprintf(stderr, "digest %016llx\n", (unsigned long long)h);
    }
    const double pack_ms = ms_pack / (launches ? launches : 1);
    const double alg = 2.0 * n * B + 5.0 * p;
    double k_pack = 0, k_scan = 0, k_exp = 0; int kl = 0;
    MI_OK(mi355_get_kernel_timing(core, &k_pack, &k_scan, &k_exp, &kl));
    double mhz = 0;
    if (!getenv("DIFFBENCH_NO_CLOCK")) MI_OK(mi355_probe_clock(core, 50, &mhz));   // right behind the timed region: the chip is warm
    double hbm = 0;
    if (getenv("DIFFBENCH_HBM_PROBE")) MI_OK(mi355_probe_hbm_read(core, 2048, &hbm));
    printf("{\"harness\": \"diffbench\", \"mode\": \"%s\", \"width\": %d, \"height\": %d, \"batch\": %d, \"steps\": %d, "
           "\"frames_per_s\": %.1f, \"ms_per_step\": %.4f, \"frac\": %.4f, \"kernel_ms\": %.4f, \"all_kernels_ms\": %.4f, \"kernels_us\": [%.1f, %.1f, %.1f], "
           "\"changed_bytes_per_frame\": %.1f, \"achieved_gbps\": %.1f, \"shader_mhz\": %.0f, \"hbm_read_probe_gbps\": %.0f, \"workspace_bytes\": %zu}\n",
           pairs ? "pairs" : "stream", W, H, B, K, (double)B * K / sec, sec / K * 1e3, alg / (sec / K) / 8e12, pack_ms, ms_total / (launches ? launches : 1),
           k_pack / (kl ? kl : 1) * 1e3, k_scan / (kl ? kl : 1) * 1e3, k_exp / (kl ? kl : 1) * 1e3,
           p / B, alg / (pack_ms * 1e-3) / 1e9, mhz, hbm, mi355_workspace_bytes(core));
    mi355_destroy(core);
    return 0;
}

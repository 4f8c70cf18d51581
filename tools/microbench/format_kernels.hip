// Device time of k_format in every format beside k_ln_apply<int16_t> (the loudness apply pass with the 16-bit sink's
// rule, gain 1: 8 B in and 2 B out per sample, the yardstick), on the same f64 samples in one process, each launch
// between two HIP events.  The kernels are the library's own, through its launch functions; nothing is copied here.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I jbonsai_amd/csrc tools/microbench/format_kernels.hip \
//       -L jbonsai_amd -ljbonsai_amd -Wl,-rpath,'$ORIGIN/../../jbonsai_amd' -o tools/microbench/format_kernels
//   tools/microbench/format_kernels [utterances=256] [samples per utterance=6131040] [repeats=7]
//
// The default is BASELINE config 2's slab: 256 utterances of 25,546 frames of 240 samples.  Prints one line per
// kernel: every repeat's time after two warm-up launches, the median, and the traffic it stands for.
#include "jb_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                                       \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) {                                                                                        \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                                                    \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

// speech-like values in 16-bit scale from the sample's index alone (the kernels' time does not depend on them)
__global__ void k_fill(double *x, uint64_t n)
{
    for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        x[k] = 9000.0 * sin(0.013 * (double)(k % 100003)) + (double)(jb::fmt_mix(k) >> 52) - 2048.0;
}

int main(int argc, char **argv)
{
    const uint64_t B = argc > 1 ? strtoull(argv[1], nullptr, 10) : 256;
    const uint64_t n = argc > 2 ? strtoull(argv[2], nullptr, 10) : 25546ull * 240;
    const int reps = argc > 3 ? atoi(argv[3]) : 7;
    const uint64_t N = B * n;
    double *x = nullptr;
    uint8_t *y = nullptr;
    jb::FormatUtt *fu = nullptr;
    jb::LoudnessUtt *lu = nullptr;
    jb::LoudnessResult *res = nullptr;
    const uint64_t ystride = (n * 4 + 15) & ~15ull;
    CHECK(hipMalloc((void **)&x, N * sizeof(double)));
    CHECK(hipMalloc((void **)&y, B * ystride));
    CHECK(hipMalloc((void **)&fu, B * sizeof *fu));
    CHECK(hipMalloc((void **)&lu, B * sizeof *lu));
    CHECK(hipMalloc((void **)&res, B * sizeof *res));
    std::vector<jb::FormatUtt> hf(B);
    std::vector<jb::LoudnessUtt> hl(B);
    std::vector<jb::LoudnessResult> hr(B);
    const uint64_t ftiles = (n + jb::kFmtTile - 1) / jb::kFmtTile, atiles = (n + jb::kLnApplyTile - 1) / jb::kLnApplyTile;
    for (uint64_t u = 0; u < B; u++) {
        hf[u] = {x + u * n, y + u * ystride, n, u * ftiles};
        hl[u] = jb::LoudnessUtt{};
        hl[u].x = x + u * n;
        hl[u].y = y + u * ystride;
        hl[u].n = n;
        hl[u].at0 = u * atiles;
        hl[u].slot = (uint32_t)u;
        hr[u] = jb::LoudnessResult{};
        hr[u].g = 1.0;
    }
    CHECK(hipMemcpy(fu, hf.data(), B * sizeof *fu, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(lu, hl.data(), B * sizeof *lu, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(res, hr.data(), B * sizeof *res, hipMemcpyHostToDevice));
    hipStream_t s;
    hipEvent_t e0, e1;
    CHECK(hipStreamCreate(&s));
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, s, x, N);
    CHECK(hipStreamSynchronize(s));
    printf("%llu utterances of %llu samples: %.3f G samples, %.2f GB of f64; %d timed launches after 2 warm-up\n",
           (unsigned long long)B, (unsigned long long)n, N / 1e9, N * 8 / 1e9, reps);
    struct Case {
        const char *name;
        uint32_t fmt, dither, bytes;
    };
    const Case cases[] = {{"k_ln_apply<int16_t>", 0, 0, 2},
                          {"k_format<S16>", jb::kFmtS16, 0, 2},
                          {"k_format<S16, TPDF>", jb::kFmtS16, 1, 2},
                          {"k_format<F32>", jb::kFmtF32, 0, 4},
                          {"k_format<S24>", jb::kFmtS24, 0, 3},
                          {"k_format<S24, TPDF>", jb::kFmtS24, 1, 3},
                          {"k_format<ULAW>", jb::kFmtUlaw, 0, 1},
                          {"k_format<ALAW>", jb::kFmtAlaw, 0, 1},
                          {"k_ln_apply<int16_t> again", 0, 0, 2}};
    for (const Case &c : cases) {
        std::vector<float> ms;
        for (int r = 0; r < reps + 2; r++) {
            CHECK(hipEventRecord(e0, s));
            if (c.fmt)
                CHECK(jb::launch_format(c.fmt, c.dither, 1, fu, (uint32_t)B, B * ftiles, s));
            else
                CHECK(jb::launch_loudness_apply(lu, (uint32_t)B, B * atiles, res, true, s));
            CHECK(hipEventRecord(e1, s));
            CHECK(hipEventSynchronize(e1));
            float t = 0;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            if (r >= 2)
                ms.push_back(t);
        }
        printf("%-28s", c.name);
        for (float t : ms)
            printf(" %.3f", t);
        std::sort(ms.begin(), ms.end());
        const double med = ms[ms.size() / 2], gb = N * (8.0 + c.bytes) / 1e9;
        printf("  ms; median %.3f (min %.3f, max %.3f); %.2f GB -> %.2f TB/s\n", med, ms.front(), ms.back(), gb,
               gb / med);
    }
    return 0;
}

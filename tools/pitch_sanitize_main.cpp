// The host half of the pitch stage (jbonsai_amd/csrc/jb_pitch.cpp with the rule of jb_pitch.h) under AddressSanitizer +
// UBSan, as a program of its own (tools/pitch_sanitize.sh builds and runs it; no GPU is touched and nothing is loaded
// into python): jb_pitch_host on both grids, at rates of 1, 40 and 160 phases, over lengths around the frame edges and
// the sums' tile, in every output mode, every input and every output a heap block of exactly its elements, so that one
// sample read in front of a unit or behind it, or one element written behind a matrix, is an error the sanitizer
// reports.  Then the smallest and the largest lag grid, and the refusals.
#include "../jbonsai_amd/csrc/jb_host.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace jb {
static std::string g_last;
void set_error(const std::string &s) { g_last = s; } // (the library's own lives beside the batch code)
} // namespace jb

#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, jb::g_last.c_str());                           \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

static int run(const jb_pitch_opts &o, uint32_t hz, size_t n, uint64_t *seed, size_t *runs)
{
    jb_pitch_geometry_t g{};
    CHECK(jb_pitch_geometry(&o, hz, n, &g) == JB_OK);
    std::unique_ptr<double[]> x(new double[n]);
    for (size_t i = 0; i < n; i++) {
        *seed = *seed * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = 3000.0 * sin(0.05 * (double)i) + (double)(int64_t)(*seed >> 54) - 512.0 + 150.0;
    }
    const size_t bytes = (size_t)g.T * g.width * g.elem;
    std::unique_ptr<uint8_t[]> out(new uint8_t[bytes]);
    std::unique_ptr<uint32_t[]> idx(new uint32_t[g.T]);
    std::unique_ptr<double[]> Q(new double[g.T * g.S]), P(new double[g.T * g.S]);
    CHECK(jb_pitch_host(x.get(), n, hz, &o, out.get(), bytes, idx.get(), Q.get(), P.get()) == JB_OK);
    for (uint64_t t = 0; t < g.T; t++)
        CHECK(idx[t] < g.S);
    if (bytes)
        CHECK(jb_pitch_host(x.get(), n, hz, &o, out.get(), bytes - 1, nullptr, nullptr, nullptr) == JB_ERR_BUFFER);
    ++*runs;
    return 0;
}

int main()
{
    uint64_t seed = 1;
    size_t runs = 0;
    for (uint32_t hz : {8000u, 11025u, 44100u})
        for (uint32_t grid : {JB_PITCH_SNIP, JB_PITCH_KALDI})
            for (uint32_t flags : {0u, JB_PITCH_F64 | JB_PITCH_RAW, JB_PITCH_RAW_LOG}) {
                jb_pitch_opts o;
                CHECK(jb_pitch_kaldi(&o) == JB_OK);
                o.grid = grid;
                o.flags = flags;
                jb_pitch_geometry_t g{};
                CHECK(jb_pitch_geometry(&o, hz, 0, &g) == JB_OK);
                const size_t tile = (size_t)1024 * hz / 4000;
                for (size_t n : {(size_t)0, (size_t)1, (size_t)g.wl - 1, (size_t)g.wl, (size_t)g.wl + g.hop, tile - 1, tile, tile + 1})
                    if (run(o, hz, n, &seed, &runs))
                        return 1;
            }
    jb_pitch_opts o;
    jb_pitch_kaldi(&o);
    o.delta_pitch = 0.002034; // 1024 lags
    if (run(o, 16000, 2000, &seed, &runs))
        return 1;
    o.min_f0 = 399.0;
    o.delta_pitch = 0.002; // 2 lags
    if (run(o, 16000, 2000, &seed, &runs))
        return 1;
    jb_pitch_kaldi(&o);
    o.win_us = 25100;
    CHECK(jb_pitch_geometry(&o, 16000, 0, nullptr) == JB_ERR_INVALID && jb::g_last.find("win_us") != std::string::npos);
    jb_pitch_kaldi(&o);
    CHECK(jb_pitch_geometry(&o, 3999, 0, nullptr) == JB_ERR_INVALID);
    CHECK(jb_pitch_geometry(&o, 44101, 0, nullptr) == JB_ERR_UNSUPPORTED);
    double lags[417];
    size_t S = 0;
    CHECK(jb_pitch_lags(&o, lags, 416, &S) == JB_ERR_BUFFER && S == 417);
    CHECK(jb_pitch_lags(&o, lags, 417, nullptr) == JB_OK);
    printf("pitch_sanitize: %zu runs clean\n", runs);
    return 0;
}

// The host half of the limiter stage (jbonsai_amd/csrc/jb_limiter.cpp, with the true-peak table of jb_loudness.hip)
// under AddressSanitizer + UBSan, as a program of its own (tools/limiter_sanitize.sh builds and runs it; no GPU is
// touched and nothing is loaded into python): jb_limiter_window, jb_limiter_host and jb_limiter_host_i16 over lengths
// around the look-ahead, the hold and the device's tile, both detectors, three rates and the widest geometry, every
// input and every output a heap block of exactly its samples, so that one sample read in front of an utterance or
// behind it, or written behind the output, is an error the sanitizer reports.
#include "../include/jbonsai_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

namespace jb {
static std::string g_last;
void set_error(const std::string &s) { g_last = s; } // (the library's own lives beside the batch code)
int hip_fail(hipError_t, const char *what)
{
    g_last = what;
    return JB_ERR_DEVICE;
}
} // namespace jb

int main()
{
    const size_t lengths[] = {0, 1, 2, 11, 12, 31, 32, 33, 160, 161, 1023, 1024, 1025, 3000, 5000};
    const uint32_t rates[] = {8000, 16000, 48000};
    uint64_t r = 88172645463325252ull;
    auto rnd = [&] {
        r ^= r << 13;
        r ^= r >> 7;
        r ^= r << 17;
        return (double)(int64_t)(r >> 11) / 9007199254740992.0 * 2.0 - 1.0;
    };
    size_t runs = 0;
    for (uint32_t hz : rates)
        for (int geo = 0; geo < 3; geo++) {
            // the defaults; the shortest; the widest the device takes at 48 kHz (2 L + H = 2048)
            jb_limiter_opts o = {2.0, 8.0, 6.0, JB_LIMITER_EXACT, 0};
            if (geo == 1)
                o = {0.01, 0.0, 6.0, JB_LIMITER_EXACT, 0};
            if (geo == 2)
                o = {10.0, hz == 48000 ? 1088.0 / 48.0 : 50.0, 24.0, JB_LIMITER_EXACT, 0};
            uint32_t L = 0, H = 0;
            if (jb_limiter_window(hz, &o, &L, &H, nullptr, 0) != JB_OK) {
                std::fprintf(stderr, "window: %s\n", jb::g_last.c_str());
                return 1;
            }
            std::unique_ptr<double[]> w(new double[L + 1]);
            if (jb_limiter_window(hz, &o, nullptr, nullptr, w.get(), L + 1) != JB_OK ||
                jb_limiter_window(hz, &o, nullptr, nullptr, w.get(), L) != JB_ERR_BUFFER)
                return 1;
            double sum = 0.0;
            for (uint32_t j = 0; j <= L; j++)
                sum += w[j];
            if (std::fabs(sum - 1.0) > 1e-13)
                return 1;
            for (size_t n : lengths)
                for (uint32_t mode = 0; mode < 2; mode++) {
                    std::unique_ptr<double[]> x(new double[n]), y(new double[n]);
                    std::unique_ptr<int16_t[]> y16(new int16_t[n]);
                    for (size_t i = 0; i < n; i++)
                        x[i] = rnd() * 9000.0;
                    if (n) {
                        x[0] = 70000.0;
                        x[n - 1] = -65000.0;
                        x[n / 2] = 40000.0;
                    }
                    jb_limiter_report rep{}, rep16{};
                    if (jb_limiter_host(x.get(), n, hz, 1.3, -1.0, mode, &o, y.get(), &rep) != JB_OK ||
                        jb_limiter_host_i16(x.get(), n, hz, 1.3, -1.0, mode, &o, y16.get(), &rep16) != JB_OK) {
                        std::fprintf(stderr, "host seam: %s\n", jb::g_last.c_str());
                        return 1;
                    }
                    const double c = 32768.0 * std::pow(10.0, -1.0 / 20.0);
                    for (size_t i = 0; i < n; i++)
                        if (!(std::fabs(y[i]) <= c) || y16[i] != (int16_t)y[i]) {
                            std::fprintf(stderr, "sample %zu of %zu at %u Hz: %g, %d\n", i, n, hz, y[i], (int)y16[i]);
                            return 1;
                        }
                    if (rep.lookahead != L || rep.hold != H || rep.limited_samples != rep16.limited_samples ||
                        (n && rep.limited_samples == 0))
                        return 1;
                    runs++;
                }
        }
    std::printf("limiter host seam under ASan + UBSan: %zu runs clean\n", runs);
    return 0;
}

// The host half of the join stage (jbonsai_amd/csrc/jb_join.cpp, with the layout of jb_output.cpp) under
// AddressSanitizer + UBSan, as a program of its own (tools/join_sanitize.sh builds and runs it; no GPU is touched and
// nothing is loaded into python): jb_join_host and jb_join_i16_host over members, pads and fades around the group and
// tile sizes, every input and every output a heap block of exactly its samples, so that one sample read in front of a
// member, behind it, or written behind a programme is an error the sanitizer reports.
#include "../include/jbonsai_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace jb {
static std::string g_last;
void set_error(const std::string &s) { g_last = s; } // (the library's own lives beside the batch code)
} // namespace jb

static double weight(uint64_t k, uint32_t fade)
{
    const double t = (double)(2 * k + 1) / (double)(2 * (uint64_t)fade);
    return (t * t) * (3.0 - 2.0 * t);
}

template <class T, class Fn> static int run(Fn join, const char *what, size_t *runs)
{
    const size_t lengths[] = {0, 1, 7, 8, 63, 64, 65, 4095, 4096, 4097};
    const uint64_t pads[] = {0, 1, 3, 4097};
    uint64_t r = 88172645463325252ull;
    auto rnd = [&] {
        r ^= r << 13;
        r ^= r >> 7;
        r ^= r << 17;
        return r;
    };
    for (int shape = 0; shape < 3; shape++) {   // one programme of all, every member its own, two interleaved
        for (int fade = 0; fade < 5; fade++) {  // 0, 1, 2, n, n + 5
            const size_t n = sizeof lengths / sizeof *lengths;
            std::vector<std::unique_ptr<T[]>> in(n);
            std::vector<const T *> inp(n);
            std::vector<size_t> nin(n);
            std::vector<jb_join_utt> req(n);
            for (size_t u = 0; u < n; u++) {
                nin[u] = lengths[u];
                in[u].reset(new T[nin[u]]); // exactly the samples
                for (size_t k = 0; k < nin[u]; k++)
                    in[u][k] = (T)((double)(int64_t)(rnd() % 65536) - 32768.0);
                inp[u] = in[u].get();
                const uint32_t f[] = {0, 1, 2, (uint32_t)nin[u], (uint32_t)nin[u] + 5};
                req[u] = jb_join_utt{shape == 0 ? 3u : shape == 1 ? JB_JOIN_NONE : (uint32_t)(u & 1), f[fade],
                                     f[(fade + 2) % 5], 0, pads[u % 4], pads[(u / 2) % 4]};
            }
            std::vector<uint32_t> prog(n);
            std::vector<uint64_t> start(n), ps(n);
            size_t P = 0;
            if (jb_join_geometry(req.data(), nin.data(), nullptr, n, prog.data(), start.data(), &P, ps.data())) {
                fprintf(stderr, "FAILED: %s geometry (%s)\n", what, jb::g_last.c_str());
                return 1;
            }
            std::vector<std::unique_ptr<T[]>> out(P);
            std::vector<T *> outp(P);
            std::vector<size_t> cap(P);
            for (size_t p = 0; p < P; p++) {
                cap[p] = (size_t)ps[p];
                out[p].reset(new T[cap[p]]); // exactly the programme
                outp[p] = out[p].get();
            }
            if (join(inp.data(), nin.data(), n, req.data(), outp.data(), cap.data())) {
                fprintf(stderr, "FAILED: %s (%s)\n", what, jb::g_last.c_str());
                return 1;
            }
            // every member's samples where the geometry puts them, under their fades
            for (size_t u = 0; u < n; u++)
                for (size_t k = 0; k < nin[u]; k++) {
                    double v = (double)in[u][k];
                    const bool fi = k < req[u].fade_in, fo = nin[u] - 1 - k < req[u].fade_out;
                    if (fi)
                        v = v * weight(k, req[u].fade_in);
                    if (fo)
                        v = v * weight(nin[u] - 1 - k, req[u].fade_out);
                    const T want = (fi || fo) ? (sizeof(T) == 2 ? (T)(int32_t)v : (T)v) : in[u][k];
                    if (memcmp(&want, &out[prog[u]][start[u] + k], sizeof(T))) {
                        fprintf(stderr, "FAILED: %s member %zu sample %zu (shape %d, fade %d)\n", what, u, k, shape, fade);
                        return 1;
                    }
                }
            if (P && cap[0] && join(inp.data(), nin.data(), n, req.data(), outp.data(),
                                    std::vector<size_t>(P, cap[0] - 1).data()) != JB_ERR_BUFFER) {
                fprintf(stderr, "FAILED: %s short buffer\n", what);
                return 1;
            }
            (*runs)++;
        }
    }
    return 0;
}

int main()
{
    size_t runs = 0;
    if (run<double>(jb_join_host, "jb_join_host", &runs) || run<int16_t>(jb_join_i16_host, "jb_join_i16_host", &runs))
        return 1;
    printf("join host code: %zu runs clean\n", runs);
    return 0;
}

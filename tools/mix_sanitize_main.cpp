// The host half of the mix stage (jbonsai_amd/csrc/jb_mix.cpp, with the layout of jb_output.cpp) under
// AddressSanitizer + UBSan, as a program of its own (tools/mix_sanitize.sh builds and runs it; no GPU is touched and
// nothing is loaded into python): jb_mix_geometry, jb_mix_host and jb_mix_i16_host over overlapping members around the
// group and tile sizes, every input and every output a heap block of exactly its samples, so that one sample read in
// front of a member, behind it, or written behind a programme is an error the sanitizer reports.
#include "../include/jbonsai_amd.h"

#include <cmath>
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

template <class T, class Fn> static int run(Fn mix, const char *what, size_t *runs)
{
    const size_t lengths[] = {0, 1, 7, 8, 63, 64, 65, 4095, 4096, 4097};
    const uint64_t starts[] = {0, 1, 3, 4097, 60, 2047, 2048, 2049, 8191, 5};
    const double gains[] = {0.0, -6.5, 12.0, -INFINITY};
    uint64_t r = 88172645463325252ull;
    auto rnd = [&] {
        r ^= r << 13;
        r ^= r >> 7;
        r ^= r << 17;
        return r;
    };
    for (int shape = 0; shape < 3; shape++) {   // one programme of all, every member its own, two interleaved
        for (int fade = 0; fade < 5; fade++) {  // 0, 1, 2, n, n + 5
            for (int fit = 0; fit < 2; fit++) {
                const size_t n = sizeof lengths / sizeof *lengths;
                std::vector<std::unique_ptr<T[]>> in(n);
                std::vector<const T *> inp(n);
                std::vector<size_t> nin(n);
                std::vector<jb_mix_utt> req(n);
                for (size_t u = 0; u < n; u++) {
                    nin[u] = lengths[u];
                    in[u].reset(new T[nin[u]]); // exactly the samples
                    for (size_t k = 0; k < nin[u]; k++)
                        in[u][k] = (T)((double)(int64_t)(rnd() % 65536) - 32768.0);
                    inp[u] = in[u].get();
                    const uint32_t f[] = {0, 1, 2, (uint32_t)nin[u], (uint32_t)nin[u] + 5};
                    req[u] = jb_mix_utt{shape == 0 ? 3u : shape == 1 ? JB_MIX_NONE : (uint32_t)(u & 1),
                                        f[fade],
                                        f[(fade + 2) % 5],
                                        0,
                                        starts[(u + shape) % 10],
                                        starts[(u / 2) % 4],
                                        gains[(u + fade) % 4],
                                        0};
                }
                const jb_mix_opts opts = {fit ? JB_MIX_FIT : 0u, 0, -3.0};
                std::vector<uint32_t> prog(n), depth(n);
                std::vector<uint64_t> start(n), ps(n), overlap(n);
                size_t P = 0;
                if (jb_mix_geometry(req.data(), nin.data(), nullptr, n, &opts, prog.data(), start.data(), &P, ps.data(),
                                    depth.data(), overlap.data())) {
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
                std::vector<jb_mix_report> rep(P);
                if (mix(inp.data(), nin.data(), n, req.data(), &opts, nullptr, outp.data(), cap.data(), rep.data())) {
                    fprintf(stderr, "FAILED: %s (%s)\n", what, jb::g_last.c_str());
                    return 1;
                }
                const double c = 32768.0 * pow(10.0, -3.0 / 20.0);
                for (size_t p = 0; p < P; p++) {
                    if (rep[p].depth != depth[p] || rep[p].overlap != overlap[p] || !(rep[p].scale <= 1.0)) {
                        fprintf(stderr, "FAILED: %s report of programme %zu\n", what, p);
                        return 1;
                    }
                    for (size_t k = 0; fit && k < cap[p]; k++)
                        if (!(fabs((double)out[p][k]) <= c)) {
                            fprintf(stderr, "FAILED: %s programme %zu sample %zu above the ceiling\n", what, p, k);
                            return 1;
                        }
                }
                if (P && cap[0] && mix(inp.data(), nin.data(), n, req.data(), &opts, nullptr, outp.data(),
                                       std::vector<size_t>(P, cap[0] - 1).data(), nullptr) != JB_ERR_BUFFER) {
                    fprintf(stderr, "FAILED: %s short buffer\n", what);
                    return 1;
                }
                (*runs)++;
            }
        }
    }
    return 0;
}

int main()
{
    size_t runs = 0;
    if (run<double>(jb_mix_host, "jb_mix_host", &runs) || run<int16_t>(jb_mix_i16_host, "jb_mix_i16_host", &runs))
        return 1;
    printf("mix host code: %zu runs clean\n", runs);
    return 0;
}

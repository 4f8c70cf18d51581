// The host half of the mix stage (jbonsai_amd/csrc/jb_mix.cpp, with the layout of jb_output.cpp) under
// AddressSanitizer + UBSan, as a program of its own (tools/mix_sanitize.sh builds and runs it; no GPU is touched and
// nothing is loaded into python): jb_mix_geometry, jb_mix_host and jb_mix_i16_host over overlapping members around the
// group and tile sizes, every input and every output a heap block of exactly its samples, so that one sample read in
// front of a member, behind it, or written behind a programme is an error the sanitizer reports.  Then the one layout
// and the list builder (mix_layout, mix_lists) over join requests in the mix's words (join_as_mix): every member,
// segment and list index is held to its bounds.
#include "../jbonsai_amd/csrc/jb_host.h"

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

#define HOLD(cond)                                                                                                     \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            fprintf(stderr, "FAILED: join request %zu, elem %zu: %s\n", which, elem, #cond);                           \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

// One join request through join_as_mix, the layout and the list builder, the PCM blocks of exactly their bytes
static int join_request_holds(size_t which, const std::vector<jb::JoinUtt> &req, const std::vector<uint64_t> &n, size_t elem)
{
    const size_t B = req.size();
    const std::vector<jb::MixUtt> m = jb::join_as_mix(req.data(), B);
    jb::MixLayout lay;
    HOLD(jb::mix_layout_checked(m.data(), true, n.data(), nullptr, B, elem, nullptr, &lay, "join") == JB_OK);
    std::vector<uint64_t> xoff(B);
    uint64_t in_total = 0;
    for (size_t u = 0; u < B; u++) {
        xoff[u] = in_total;
        in_total += n[u];
    }
    std::unique_ptr<char[]> x(new char[in_total * elem]), y(new char[lay.total * elem]);
    std::vector<jb::ProgMember> members;
    std::vector<jb::ProgSpan> spans;
    uint64_t tiles = 0, t = 0;
    jb::mix_lists(lay, m.data(), n.data(), xoff.data(), x.get(), y.get(), elem, &members, &spans, &tiles);
    const size_t P = lay.units.size();
    HOLD(members.size() == B && spans.size() == P && lay.seg_first.size() == P + 1 && lay.progs.members.size() == B);
    for (size_t p = 0; p < P; p++) {
        const jb::ProgSpan &w = spans[p];
        HOLD((char *)w.y >= y.get() && (char *)w.y + w.n * elem <= y.get() + lay.total * elem);
        HOLD(((char *)w.y - y.get()) % 16 == 0 && w.k0 == 0 && w.k1 == w.n && w.t0 == t && w.pk0 == t && w.prog == p);
        t += jb::prog_tiles(0, w.n, elem == 2);
        HOLD(w.nm >= 1 && (size_t)w.m0 + w.nm <= B && (size_t)w.s0 + w.ns <= lay.segs.size());
        uint64_t end = 0; // where the member in front ends: a join's members follow each other
        for (uint32_t i = w.m0; i < w.m0 + w.nm; i++) {
            const jb::ProgMember &mm = members[i];
            HOLD(lay.progs.members[i] < B && lay.progs.group_of[lay.progs.members[i]] == p);
            HOLD((const char *)mm.x >= x.get() && (const char *)mm.x + mm.n * elem <= x.get() + in_total * elem);
            HOLD(mm.start >= end && mm.start + mm.n <= w.n && mm.g == 1.0);
            end = mm.start + mm.n;
        }
        uint64_t k = 0;
        for (uint32_t i = w.s0; i < w.s0 + w.ns; i++) {
            const jb::MixSeg &g = lay.segs[i];
            HOLD(g.k0 == k && g.k1 > g.k0 && g.nl <= 1 && (size_t)g.l0 + g.nl <= lay.lists.size());
            for (uint32_t j = g.l0; j < g.l0 + g.nl; j++) {
                const uint32_t at = lay.lists[j];
                HOLD(at >= w.m0 && at < w.m0 + w.nm && members[at].start <= g.k0 && g.k1 <= members[at].start + members[at].n);
            }
            k = g.k1;
        }
        HOLD(k == w.n && lay.depth[p] <= 1 && lay.overlap[p] == 0);
    }
    HOLD(t == tiles);
    return 0;
}

// The join requests of tests/test_join_plan.py: the routing table's, the lengths against the pads in one programme, in
// two and each alone, members of no samples
static int run_joins(size_t *runs)
{
    const uint64_t n6[] = {7 * 240, 0, 13 * 240, 240, 3 * 240, 2 * 240};
    const jb::JoinUtt req6[] = {{0, 240, 240, 0, 24000, 3}, {1, 0, 7, 0, 1, 0}, {0, 0, 0, 0, 0, 5},
                                {1, 3, 0, 0, 7, 9},         {0, 5, 5, 0, 0, 11}, {jb::kJoinNone, 1, 1, 0, 2, 4}};
    const uint64_t lengths[] = {0, 1, 7, 8, 63, 64, 65, 4095, 4096, 4097};
    const uint64_t pads[] = {0, 1, 3, 4097};
    std::vector<std::pair<std::vector<jb::JoinUtt>, std::vector<uint64_t>>> cases;
    for (int rate = 0; rate < 2; rate++) {
        std::vector<uint64_t> n(n6, n6 + 6);
        for (uint64_t &k : n)
            k = rate ? (k * 147 + 159) / 160 : k;
        cases.push_back({std::vector<jb::JoinUtt>(req6, req6 + 6), n});
    }
    cases.push_back({std::vector<jb::JoinUtt>(req6, req6 + 6), std::vector<uint64_t>(6, 0)});
    for (int shape = 0; shape < 3; shape++) { // one programme, two interleaved, every member its own
        std::vector<jb::JoinUtt> req;
        std::vector<uint64_t> n;
        for (uint32_t u = 0; u < 20; u++) {
            n.push_back(lengths[u < 10 ? u : 19 - u]);
            const uint32_t f[] = {0, 1, 2, (uint32_t)n[u], (uint32_t)n[u] + 5};
            req.push_back({shape == 0 ? 0u : shape == 1 ? u % 2 : jb::kJoinNone, f[u % 5], f[(u + 2) % 5], 0, pads[u % 4],
                           pads[(u / 4) % 4]});
        }
        cases.push_back({req, n});
    }
    for (size_t which = 0; which < cases.size(); which++)
        for (size_t elem : {(size_t)8, (size_t)2}) {
            if (join_request_holds(which, cases[which].first, cases[which].second, elem))
                return 1;
            (*runs)++;
        }
    return 0;
}

int main()
{
    size_t runs = 0, joins = 0;
    if (run<double>(jb_mix_host, "jb_mix_host", &runs) || run<int16_t>(jb_mix_i16_host, "jb_mix_i16_host", &runs) ||
        run_joins(&joins))
        return 1;
    printf("mix host code: %zu runs clean; join requests through the layout and the lists: %zu clean\n", runs, joins);
    return 0;
}

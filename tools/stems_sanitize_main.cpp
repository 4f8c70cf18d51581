// The host half of the stems of a mix (jbonsai_amd/csrc/jb_mix.cpp, with the layout of jb_output.cpp) under
// AddressSanitizer + UBSan, as a program of its own (tools/stems_sanitize.sh builds and runs it; no GPU is touched and
// nothing is loaded into python): jb_mix_stems_geometry, jb_mix_stems_host and jb_mix_stems_i16_host with the levels,
// and jb_mix_levels_host, over overlapping members around the group, tile and partial sizes, every input and every
// output a heap block of exactly its samples, so that one sample read in front of a member, behind it, or written
// behind a unit is an error the sanitizer reports.  Then the layout, the list builder and the level items (mix_layout
// with stem_of, mix_lists, mix_level_items): every member, segment, list and tile index is held to its bounds.
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

#define HOLD(cond)                                                                                                     \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            fprintf(stderr, "FAILED: %s shape %d fade %d fit %d: %s (%s)\n", what, shape, fade, fit, #cond,             \
                    jb::g_last.c_str());                                                                               \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

template <class T, class Fn, class Lv> static int run(Fn mix, Lv levels, const char *what, size_t *runs)
{
    const size_t lengths[] = {0, 1, 7, 8, 255, 256, 1023, 1024, 1025, 4097};
    const uint64_t starts[] = {0, 1, 3, 4097, 60, 1023, 1024, 1025, 8191, 5};
    const double gains[] = {0.0, -6.5, 12.0, -INFINITY};
    uint64_t r = 88172645463325252ull;
    auto rnd = [&] {
        r ^= r << 13;
        r ^= r >> 7;
        r ^= r << 17;
        return r;
    };
    for (int shape = 0; shape < 4; shape++) {  // one stem of all, every member its own, three talkers, some without
        for (int fade = 0; fade < 5; fade++) { // 0, 1, 2, n, n + 5
            for (int fit = 0; fit < 2; fit++) {
                const size_t n = sizeof lengths / sizeof *lengths;
                std::vector<std::unique_ptr<T[]>> in(n);
                std::vector<const T *> inp(n);
                std::vector<size_t> nin(n);
                std::vector<jb_mix_utt> req(n);
                std::vector<uint32_t> stem_of(n);
                for (size_t u = 0; u < n; u++) {
                    nin[u] = lengths[u];
                    in[u].reset(new T[nin[u]]); // exactly the samples
                    for (size_t k = 0; k < nin[u]; k++)
                        in[u][k] = (T)((double)(int64_t)(rnd() % 65536) - 32768.0);
                    inp[u] = in[u].get();
                    const uint32_t f[] = {0, 1, 2, (uint32_t)nin[u], (uint32_t)nin[u] + 5};
                    req[u] = jb_mix_utt{u == 9 ? JB_MIX_NONE : (uint32_t)(u & 1),
                                        f[fade],
                                        f[(fade + 2) % 5],
                                        0,
                                        starts[(u + shape) % 10],
                                        starts[(u / 2) % 4],
                                        gains[(u + fade) % 4],
                                        0};
                    stem_of[u] = shape == 0   ? 4u
                                 : shape == 1 ? (uint32_t)u
                                 : shape == 2 ? (uint32_t)(u % 3)
                                              : (u % 3 ? (uint32_t)(u % 3) : JB_MIX_NO_STEM);
                }
                const jb_mix_opts opts = {fit ? JB_MIX_FIT : 0u, 0, -3.0};
                const size_t cap2 = 2 * n;
                std::vector<int64_t> unit_of(n);
                std::vector<uint64_t> ns(cap2), first(cap2), end(cap2);
                std::vector<uint32_t> prog(cap2), id(cap2), mem(cap2), depth(cap2);
                size_t P = 0, U = 0;
                HOLD(jb_mix_stems_geometry(req.data(), stem_of.data(), nin.data(), nullptr, n, &opts, &P, &U, unit_of.data(),
                                           ns.data(), prog.data(), id.data(), mem.data(), first.data(), end.data(),
                                           depth.data()) == JB_OK);
                HOLD(P >= 1 && U >= P && U <= cap2);
                std::vector<std::unique_ptr<T[]>> out(U);
                std::vector<T *> outp(U);
                std::vector<size_t> cap(U);
                for (size_t p = 0; p < U; p++) {
                    HOLD(prog[p] < P && ns[p] == ns[prog[p]] && first[p] <= end[p] && end[p] <= ns[p]);
                    cap[p] = (size_t)ns[p];
                    out[p].reset(new T[cap[p]]); // exactly the unit
                    outp[p] = out[p].get();
                }
                std::vector<jb_mix_report> rep(P);
                std::vector<jb_stem_report> srep(U - P + 1);
                HOLD(mix(inp.data(), nin.data(), n, req.data(), stem_of.data(), JB_MIX_STEM_LEVELS, &opts, nullptr,
                         outp.data(), cap.data(), rep.data(), srep.data()) == JB_OK);
                for (size_t p = P; p < U; p++) {
                    double e_s = 0, d = 0, e_p = 0;
                    HOLD(levels(outp[p], outp[prog[p]], cap[p], first[p], end[p], &e_s, &d, &e_p) == JB_OK);
                    const jb_stem_report &s = srep[p - P];
                    HOLD(s.e_s == e_s && s.d == d && s.e_p == e_p && s.scale == rep[prog[p]].scale);
                    for (size_t k = 0; k < cap[p]; k++) // a stem is silent outside its extent
                        HOLD((k >= first[p] && k < end[p]) || out[p][k] == (T)0);
                }
                if (cap[U - 1])
                    HOLD(mix(inp.data(), nin.data(), n, req.data(), stem_of.data(), 0, &opts, nullptr, outp.data(),
                             std::vector<size_t>(U, cap[U - 1] - 1).data(), nullptr, nullptr) == JB_ERR_BUFFER);
                // the layout, the lists and the level items of the same request, for 8- and 2-byte samples
                for (size_t elem : {sizeof(double), sizeof(int16_t)}) {
                    std::vector<uint64_t> n64(nin.begin(), nin.end()), xoff(n);
                    uint64_t in_total = 0;
                    for (size_t u = 0; u < n; u++) {
                        xoff[u] = in_total;
                        in_total += n64[u];
                    }
                    jb::MixLayout lay;
                    HOLD(jb::mix_layout_checked((const jb::MixUtt *)req.data(), false, n64.data(), nullptr, n, elem,
                                                (const jb::MixOpts *)&opts, &lay, what, stem_of.data()) == JB_OK);
                    std::unique_ptr<char[]> x(new char[in_total * elem + 1]), y(new char[lay.total * elem + 1]);
                    std::vector<jb::ProgMember> members;
                    std::vector<jb::ProgSpan> spans;
                    uint64_t tiles = 0, t = 0;
                    jb::mix_lists(lay, (const jb::MixUtt *)req.data(), n64.data(), xoff.data(), x.get(), y.get(), elem,
                                  &members, &spans, &tiles);
                    HOLD(lay.units.size() == U && spans.size() == U && lay.seg_first.size() == U + 1 &&
                         lay.stems.size() == U - P);
                    for (size_t p = 0; p < U; p++) {
                        const jb::ProgSpan &w = spans[p];
                        HOLD((char *)w.y >= y.get() && (char *)w.y + w.n * elem <= y.get() + lay.total * elem);
                        HOLD(((char *)w.y - y.get()) % 16 == 0 && w.k1 == w.n && w.t0 == t && w.prog == p);
                        HOLD(w.parent == (p < P ? p : lay.stems[p - P].programme) && w.n == spans[w.parent].n);
                        t += jb::prog_tiles(0, w.n, elem == 2);
                        HOLD((size_t)w.s0 + w.ns <= lay.segs.size());
                        for (uint32_t s = w.s0; s < w.s0 + w.ns; s++) {
                            const jb::MixSeg &g = lay.segs[s];
                            HOLD(g.k0 < g.k1 && g.k1 <= w.n && (size_t)g.l0 + g.nl <= lay.lists.size());
                            for (uint32_t i = g.l0; i < g.l0 + g.nl; i++) {
                                HOLD(lay.lists[i] >= w.m0 && lay.lists[i] < w.m0 + w.nm);
                                const jb::ProgMember &m = members[lay.lists[i]];
                                HOLD(m.start <= g.k0 && g.k1 <= m.start + m.n); // every listed member holds the segment
                            }
                        }
                    }
                    HOLD(t == tiles);
                    std::vector<jb::LevelItem> items;
                    uint64_t lt = 0, scratch = 0;
                    jb::mix_level_items(lay, y.get(), elem, {}, &items, &lt, &scratch);
                    size_t with_stems = 0; // (a programme without a stem has no item)
                    for (size_t q = 0; q < P; q++)
                        for (const jb::MixStem &st : lay.stems)
                            if (st.programme == q) {
                                with_stems++;
                                break;
                            }
                    HOLD(items.size() == U - P + with_stems && lt == scratch);
                    uint64_t at = 0;
                    for (const jb::LevelItem &it : items) {
                        HOLD(it.t0 == at && it.s0 == at && (it.nt == 0 || (it.tile0 + it.nt - 1) * jb::kLevelTile < it.n));
                        HOLD((const char *)it.a + it.n * elem <= y.get() + lay.total * elem);
                        at += it.nt;
                    }
                    std::vector<uint8_t> mask(U, 0);
                    mask[0] = 1;
                    mask[U - 1] = 1;
                    jb::mix_level_items(lay, y.get(), elem, mask, &items, &lt, nullptr);
                    HOLD(items.size() == (U > 1 ? 2u : 1u) && items[0].t0 == 0 && lt <= scratch);
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
    if (run<double>(jb_mix_stems_host, jb_mix_levels_host, "jb_mix_stems_host", &runs) ||
        run<int16_t>(jb_mix_stems_i16_host, jb_mix_levels_i16_host, "jb_mix_stems_i16_host", &runs))
        return 1;
    // refusals touch nothing
    const double x[4] = {1, 2, 3, 4};
    const double *in[2] = {x, x};
    const size_t nin[2] = {4, 4};
    const jb_mix_utt req[2] = {{0, 0, 0, 0, 0, 0, 0.0, 0}, {0, 0, 0, 0, 2, 0, 0.0, 0}};
    const uint32_t bad[2] = {0, 2};
    double *out[4] = {nullptr, nullptr, nullptr, nullptr};
    const size_t cap[4] = {0, 0, 0, 0};
    if (jb_mix_stems_host(in, nin, 2, req, bad, 0, nullptr, nullptr, out, cap, nullptr, nullptr) != JB_ERR_INVALID ||
        jb::g_last.find("stem id") == std::string::npos) {
        fprintf(stderr, "FAILED: a stem id of the batch size is not refused (%s)\n", jb::g_last.c_str());
        return 1;
    }
    printf("stems sanitize: %zu requests clean\n", runs);
    return 0;
}

// The host half of the speech-activity stage (jbonsai_amd/csrc/jb_activity.cpp, with the layout and the packed steps of
// jb_activity.h) under AddressSanitizer + UBSan, as a program of its own (tools/activity_sanitize.sh builds and runs
// it; no GPU is touched and nothing is loaded into python): jb_activity_host and jb_activity_members_host on every
// grid over windows, hops and lengths around the frame edges, every input and every output a heap block of exactly its
// elements, so that one sample read in front of a member or behind it, or one label written behind the matrix, is an
// error the sanitizer reports.  Then act_layout over the same members (every column's frames inside its unit's T, its
// energies inside the scratch), and the packed smoothing steps word by word against the labels of the host rule.
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

#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, jb::g_last.c_str());                           \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

int main()
{
    uint64_t r = 88172645463325252ull;
    auto rnd = [&] {
        r ^= r << 13;
        r ^= r >> 7;
        r ^= r << 17;
        return r;
    };
    const uint32_t windows[] = {2, 63, 64, 65, 400, 4096};
    size_t runs = 0;
    for (uint32_t grid = 0; grid < 4; grid++)
        for (uint32_t wl : windows)
            for (uint32_t hop : {1u, wl, wl + 7, 160u})
                for (int smooth = 0; smooth < 2; smooth++) {
                    if (wl == 4096 && hop < 160) // (sixteen thousand frames of 4096 samples each: minutes under ASan)
                        continue;
                    jb_activity_opts o{};
                    o.win_us = wl;
                    o.hop_us = hop;
                    o.gate_db = 30.0;
                    o.grid = grid;
                    o.flags = JB_ACTIVITY_SAMPLES;
                    if (smooth)
                        o.min_speech = 3, o.min_gap = 2, o.hang_before = 70, o.hang_after = 1;
                    // members around the frame edges in a unit a little longer than the last of them
                    const size_t lengths[] = {0, 1, wl - 1, wl, (size_t)wl + hop, 3 * (size_t)wl + 5};
                    const size_t m = sizeof lengths / sizeof *lengths;
                    std::vector<std::unique_ptr<double[]>> in(m);
                    std::vector<const double *> inp(m);
                    std::vector<size_t> n_in(lengths, lengths + m);
                    std::vector<uint64_t> start(m);
                    std::vector<double> gain(m, 0.0);
                    gain[3] = -INFINITY;
                    uint64_t n_unit = 0;
                    for (size_t j = 0; j < m; j++) {
                        in[j].reset(new double[lengths[j]]);
                        for (size_t k = 0; k < lengths[j]; k++)
                            in[j][k] = (double)(int64_t)(rnd() % 60001) - 30000.0;
                        inp[j] = in[j].get();
                        start[j] = rnd() % (2 * (uint64_t)wl + 3);
                        n_unit = std::max<uint64_t>(n_unit, start[j] + lengths[j]);
                    }
                    n_unit += rnd() % 3;
                    uint64_t T = 0;
                    CHECK(jb_activity_geometry(&o, 0, n_unit, nullptr, nullptr, &T) == JB_OK);
                    std::unique_ptr<uint8_t[]> out(new uint8_t[T * m]);
                    std::vector<jb_activity_report> cols(m);
                    jb_activity_unit_report unit{};
                    CHECK(jb_activity_members_host(inp.data(), n_in.data(), start.data(), gain.data(), m, n_unit, 0, &o,
                                                   out.get(), T * m, cols.data(), &unit) == JB_OK);
                    CHECK(unit.frames == T && unit.none + unit.one + unit.many == T);
                    // each member alone, as a unit of exactly its samples
                    for (size_t j = 0; j < m; j++) {
                        uint64_t Tj = 0;
                        CHECK(jb_activity_geometry(&o, 0, lengths[j], nullptr, nullptr, &Tj) == JB_OK);
                        std::unique_ptr<uint8_t[]> lab(new uint8_t[Tj]);
                        jb_activity_report rep{};
                        CHECK(jb_activity_host(inp[j], lengths[j], 0, &o, lab.get(), Tj, &rep) == JB_OK);
                        CHECK(rep.active <= Tj && (rep.active ? rep.first <= rep.last && rep.last < Tj : rep.first == Tj));
                        // the packed steps on the raw bits of this column are the host rule's labels
                        jb_activity_opts raw = o;
                        raw.min_speech = raw.min_gap = raw.hang_before = raw.hang_after = 0;
                        std::unique_ptr<uint8_t[]> bits(new uint8_t[Tj]);
                        CHECK(jb_activity_host(inp[j], lengths[j], 0, &raw, bits.get(), Tj, nullptr) == JB_OK);
                        std::vector<uint64_t> w((Tj + 63) / 64, 0);
                        for (uint64_t t = 0; t < Tj; t++)
                            if (bits[t])
                                w[t / 64] |= 1ull << (t % 64);
                        auto step = [&](int kind) {
                            const size_t nw = w.size();
                            std::vector<uint64_t> src(w);
                            if (kind == 1)
                                for (auto &x : src)
                                    x = ~x;
                            std::vector<int64_t> before(nw), behind(nw);
                            int64_t c = -1;
                            for (size_t i = 0; i < nw; i++) {
                                before[i] = c;
                                if (src[i])
                                    c = (int64_t)(i * 64) + 63 - __builtin_clzll(src[i]);
                            }
                            c = (int64_t)1 << 62;
                            for (size_t i = nw; i-- > 0;) {
                                behind[i] = c;
                                if (src[i])
                                    c = (int64_t)(i * 64) + __builtin_ctzll(src[i]);
                            }
                            for (size_t i = 0; i < nw; i++) {
                                const int64_t b = (int64_t)(i * 64);
                                w[i] = kind == 0   ? jb::act_close_word(src[i], b, before[i], behind[i], (int64_t)Tj, o.min_gap)
                                       : kind == 1 ? jb::act_open_word(src[i], b, before[i], behind[i], (int64_t)Tj, o.min_speech)
                                                   : jb::act_hang_word(src[i], b, before[i], behind[i], (int64_t)Tj,
                                                                       o.hang_before, o.hang_after);
                            }
                        };
                        if (o.min_gap)
                            step(0);
                        if (o.min_speech > 1)
                            step(1);
                        if (o.hang_before || o.hang_after)
                            step(2);
                        for (uint64_t t = 0; t < Tj; t++)
                            CHECK(((w[t / 64] >> (t % 64)) & 1) == lab[t]);
                    }
                    // the layout of the same unit: frames inside T, energies inside the scratch
                    const uint32_t first[2] = {0, (uint32_t)m};
                    std::vector<uint32_t> members(m);
                    std::vector<uint64_t> ns(n_in.begin(), n_in.end());
                    std::vector<double> g(m, 1.0);
                    g[3] = 0.0;
                    for (size_t j = 0; j < m; j++)
                        members[j] = (uint32_t)j;
                    jb::ActLayout lay;
                    size_t bad = 0;
                    bool unsupported = false;
                    CHECK(!jb::act_layout(*(const jb::ActOpts *)&o, 1, &n_unit, nullptr, first, members.data(), start.data(),
                                          ns.data(), g.data(), &lay, &bad, &unsupported));
                    CHECK(lay.units.size() == 1 && lay.units[0].T == T && lay.cols.size() == m && lay.bytes >= T * m);
                    uint64_t e = 0;
                    for (const jb::ActLayCol &c : lay.cols) {
                        CHECK(c.f0 + c.nf <= T && c.e0 == e);
                        e += c.nf;
                    }
                    CHECK(e == lay.energies && lay.cols[3].nf == 0 && lay.cols[0].nf == 0);
                    runs++;
                }
    printf("activity_sanitize: %zu units clean\n", runs);
    return 0;
}

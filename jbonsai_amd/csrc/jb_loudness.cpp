// jb_loudness.cpp -- the host statement of the loudness rules behind the measure passes (jb_loudness_rules.h): what
// k_ln_gate_group, k_ln_windows and k_ln_range compute, from hop energies and peaks the caller holds, one member
// after the other.  No GPU is touched.
#include "jb_host.h"

#include <algorithm>
#include <cmath>

namespace jb {

namespace {
struct HostHopZ {
    const double *z;
    double operator()(uint64_t h) const { return z[h]; }
};

// the members' partials of one pass (each: the lanes' strided sums, the tree), added in member order
template <class Member> void gate_pass(size_t n, Member member, int pass, double gamma, double *gsum, uint64_t *gcnt)
{
    *gsum = 0.0;
    *gcnt = 0;
    double sum[kLnLanes];
    uint32_t cnt[kLnLanes];
    for (size_t m = 0; m < n; m++) {
        for (uint32_t lane = 0; lane < kLnLanes; lane++)
            member(m, lane, pass, gamma, &sum[lane], &cnt[lane]);
        ln_tree(sum, cnt);
        *gsum += sum[0];
        *gcnt += cnt[0];
    }
}

// the R128 fields of the members [m0, m0 + n): sw[m] their windows' mean squares, mom[m] their momentary maxima
void range_of(const std::vector<std::vector<double>> &sw, const double *mom, size_t m0, size_t n, LoudnessRange *out)
{
    LoudnessRange r{};
    r.max_momentary = -INFINITY;
    double st = 0.0;
    for (size_t m = m0; m < m0 + n; m++) {
        r.max_momentary = std::fmax(r.max_momentary, mom[m]);
        for (double v : sw[m])
            st = std::fmax(st, v);
    }
    r.max_short_term = ln_loudness(st);
    auto member = [&](size_t m, uint32_t lane, int pass, double gamma, double *sum, uint32_t *cnt) {
        const std::vector<double> &w = sw[m0 + m];
        ln_lane_partial([&](uint64_t i) { return w[i]; }, w.size(), lane, pass, gamma, sum, cnt);
    };
    double gamma = -INFINITY, gsum;
    uint64_t gcnt;
    gate_pass(n, member, 0, gamma, &gsum, &gcnt);
    if (gcnt) {
        gamma = ln_loudness(gsum / (double)gcnt) + kLnRangeGate;
        gate_pass(n, member, 1, gamma, &gsum, &gcnt);
        r.n = gcnt;
    }
    r.lra = 0.0;
    r.lra_low = r.lra_high = NAN;
    if (r.n) {
        uint64_t rank[2] = {ln_rank(r.n, kLnRangeLo), ln_rank(r.n, kLnRangeHi)}, prefix[2] = {0, 0};
        for (uint32_t pass = 0; pass < 8; pass++) {
            uint32_t hist[2][256] = {};
            for (size_t m = m0; m < m0 + n; m++)
                for (double v : sw[m]) {
                    if (!ln_keep(ln_loudness(v), 1, gamma))
                        continue;
                    const uint64_t bits = ln_bits(v);
                    for (int k = 0; k < 2; k++)
                        if (ln_radix_in(bits, prefix[k], pass))
                            hist[k][ln_radix_digit(bits, pass)]++;
                }
            for (int k = 0; k < 2; k++)
                prefix[k] = (prefix[k] << 8) | ln_radix_pick(hist[k], &rank[k]);
        }
        const double lo = ln_from_bits(prefix[0]), hi = ln_from_bits(prefix[1]);
        r.lra = 10.0 * std::log10(hi / lo);
        r.lra_low = ln_loudness(lo);
        r.lra_high = ln_loudness(hi);
    }
    *out = r;
}
} // namespace

void loudness_gate_host(const double *const *z, const size_t *nh, size_t n, uint32_t hop, const double *peak,
                        const double *true_peak, double target, double ceiling, LoudnessGroupResult *group,
                        LoudnessRange *range, LoudnessRange *member_range)
{
    auto member = [&](size_t m, uint32_t lane, int pass, double gamma, double *sum, uint32_t *cnt) {
        const HostHopZ hz{z[m]};
        ln_lane_partial([&](uint64_t i) { return ln_block_ms(hz, i, hop); }, ln_blocks(nh[m]), lane, pass, gamma, sum,
                        cnt);
    };
    double gamma = -INFINITY, L = -INFINITY, gsum;
    uint64_t gcnt;
    gate_pass(n, member, 0, gamma, &gsum, &gcnt);
    if (gcnt) {
        gamma = ln_loudness(gsum / (double)gcnt) + kLnRelGate;
        gate_pass(n, member, 1, gamma, &gsum, &gcnt);
        if (gcnt)
            L = ln_loudness(gsum / (double)gcnt);
    }
    double p = 0.0, t = 0.0;
    for (size_t m = 0; m < n; m++) {
        p = std::fmax(p, peak[m]);
        if (true_peak)
            t = std::fmax(t, std::fmax(peak[m], true_peak[m]));
    }
    LoudnessGroupResult g{};
    g.lufs = L;
    g.peak_dbfs = 20.0 * std::log10(p / 32768.0);
    g.true_peak_dbtp = true_peak ? 20.0 * std::log10(t / 32768.0) : NAN;
    g.gain_db = ln_gain_db(target, L, ceiling, true_peak ? g.true_peak_dbtp : g.peak_dbfs);
    g.g = std::pow(10.0, g.gain_db / 20.0);
    *group = g;
    if (!range && !member_range)
        return;
    std::vector<std::vector<double>> sw(n);
    std::vector<double> mom(n);
    for (size_t m = 0; m < n; m++) {
        const HostHopZ hz{z[m]};
        sw[m].resize((size_t)ln_windows(nh[m]));
        for (size_t i = 0; i < sw[m].size(); i++)
            sw[m][i] = ln_window_ms(hz, i, hop);
        double mx = 0.0;
        for (uint64_t i = 0; i < ln_blocks(nh[m]); i++)
            mx = std::fmax(mx, ln_block_ms(hz, i, hop));
        mom[m] = ln_loudness(mx);
    }
    if (range)
        range_of(sw, mom.data(), 0, n, range);
    for (size_t m = 0; member_range && m < n; m++)
        range_of(sw, mom.data(), m, 1, &member_range[m]);
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_loudness_gate_host(const double *const *z, const size_t *n_hops, size_t n, uint32_t hop, const double *peak,
                          const double *true_peak, double target_lufs, double ceiling_db,
                          jb_loudness_group_report *group, jb_loudness_r128 *member_r128)
{
    if (!group || hop == 0 || (n && (!z || !n_hops || !peak))) {
        set_error("jb_loudness_gate_host: a null argument, or a hop of 0 samples");
        return JB_ERR_INVALID;
    }
    for (size_t m = 0; m < n; m++)
        if (n_hops[m] && !z[m]) {
            set_error("jb_loudness_gate_host: a member with hops and no energies");
            return JB_ERR_INVALID;
        }
    LoudnessGroupResult g{};
    LoudnessRange r{};
    std::vector<LoudnessRange> mr(member_r128 ? n : 0);
    loudness_gate_host(z, n_hops, n, hop, peak, true_peak, target_lufs, ceiling_db, &g, &r,
                       member_r128 ? mr.data() : nullptr);
    loudness_group_report(g, true_peak ? JB_PEAK_TRUE : JB_PEAK_SAMPLE, 0, (uint32_t)n, &r, group);
    for (size_t m = 0; m < mr.size(); m++)
        loudness_r128_out(mr[m], &member_r128[m]);
    return JB_OK;
}

} // extern "C"

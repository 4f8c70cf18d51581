#pragma once
// jb_mix.h -- the mix stage (include/jbonsai_amd.h "Mix"), the join's sibling: a programme's PCM is the sum of its
// members, each at a start of its own, under its own edge fades (jb_join.h's, not restated) and a gain of its own.
// The rules of one sample, of the gain and of the fit, stated once for the kernel (jb_mix.hip), for the host seam
// (jb_mix.cpp) and for the output plan (jb_output.cpp), and the segments of the work lists (members and spans: jb_join.h).
// Plain C++17 and header-only; under hipcc the rules compile for the host and the device alike.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "jb_join.h"

namespace jb {

// jb_mix_utt, jb_mix_opts and jb_mix_report of the public header, restated (this header stands without it; jb_mix.cpp
// asserts that the two agree)
struct MixUtt {
    uint32_t programme;         // a caller's id below B, or kMixNone
    uint32_t fade_in, fade_out; // samples at the output rate
    uint32_t reserved;
    uint64_t start;     // the member's first sample within the programme
    uint64_t pad_after; // zero samples the member claims behind its last one
    double gain_db;     // finite in [kMixMinDb, kMixMaxDb], or -INFINITY: muted, the member counts for the length alone
    uint64_t reserved2;
};
static_assert(sizeof(MixUtt) == 48 && offsetof(MixUtt, start) == 16 && offsetof(MixUtt, gain_db) == 32,
              "jb_mix_utt is 48 bytes");
struct MixOpts {
    uint32_t flags, reserved;
    double ceiling_db; // dBFS, with kMixFit
};
struct MixReport {
    double peak, scale;       // M_p and s_p
    uint32_t depth, reserved; // the largest number of unmuted members over one sample
    uint64_t overlap;         // samples under two or more unmuted members
};
constexpr uint32_t kMixNone = kJoinNone; // JB_MIX_NONE: the utterance is a programme of its own
constexpr uint32_t kMixFit = 1u;         // JB_MIX_FIT
constexpr double kMixMinDb = -120.0, kMixMaxDb = 40.0, kMixMinCeilingDb = -120.0;
constexpr uint64_t kMixMaxList = 1ull << 24; // entries of the segments' member lists

constexpr uint32_t kMixWaves = kProgLanes / 64; // a tile leaves one |acc| maximum per wave

// One segment of a programme: samples [k0, k1) lie under the same unmuted members, lists[l0 .. l0 + nl) in ascending
// utterance index (entries: places in the members' list).  A programme's segments follow each other from 0 to its
// length without a hole; nl == 0 is silence
struct MixSeg {
    uint64_t k0, k1;
    uint32_t l0, nl;
};

// What k_mix_peak leaves per programme
struct MixResult {
    double peak, scale;
};

// g = 10^(gain_db / 20), formed in long double and rounded once; 0 dB is exactly 1, -INFINITY exactly 0.  A host
// function: the device reads g from its work list
inline double mix_gain(double gain_db)
{
    if (gain_db == 0.0)
        return 1.0;
    if (gain_db == -INFINITY)
        return 0.0;
    return (double)powl(10.0L, (long double)gain_db / 20.0L);
}

// The term of one member at its sample k: the join's faded sample in f64 (a 16-bit sample enters as its (double): no
// truncation per member), times the gain where that is not 1
JB_JOIN_HD double mix_term(double x, uint64_t k, uint64_t n, uint32_t fade_in, uint32_t fade_out, double g)
{
    double t = join_sample(x, k, n, fade_in, fade_out);
    if (g != 1.0)
        t = t * g;
    return t;
}

// The sum at sample k of a programme under the members list[0 .. nl): the first term starts it, the others are added
// in list order; +0.0 under no member
template <class T> JB_JOIN_HD double mix_acc(const ProgMember *members, const uint32_t *list, uint32_t nl, uint64_t k)
{
    double acc = 0.0;
    for (uint32_t i = 0; i < nl; i++) {
        const ProgMember m = members[list[i]];
        const uint64_t ka = k - m.start;
        const double t = mix_term((double)((const T *)m.x)[ka], ka, m.n, m.fade_in, m.fade_out, m.g);
        acc = i ? acc + t : t;
    }
    return acc;
}

// The segment of sample k among segs[lo .. hi] (the last one with k0 <= k)
JB_JOIN_HD uint32_t mix_find(const MixSeg *segs, uint32_t lo, uint32_t hi, uint64_t k)
{
    while (hi > lo) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].k0 <= k)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The fit, in the limiter's words (jb_limiter.h lim_ceiling, lim_ratio and lim_out, spelt again here: this header is
// compiled where that one is not): c the ceiling in sample units, s = c / M where the peak M lies above it, and a
// scaled sample held inside [-c, c] exactly
inline double mix_ceiling(double ceiling_db) { return 32768.0 * pow(10.0, ceiling_db / 20.0); } // (the host's)
JB_JOIN_HD double mix_scale(double M, double c) { return M > c ? c / M : 1.0; }
JB_JOIN_HD double mix_fit(double acc, double s, double c) { return fmin(fmax(acc * s, -c), c); }

// The sinks: f64 as it is, 16 bits by the 16-bit sink's rule (jb_format.h fmt_quant without dither: clamp, then
// truncate toward zero)
JB_JOIN_HD void mix_store(double v, double *o) { *o = v; }
JB_JOIN_HD void mix_store(double v, int16_t *o)
{
    v = fmin(v, 32767.0);
    v = fmax(v, -32768.0);
    *o = (int16_t)(int32_t)v;
}

// ---- Stems (jb_batch_set_mix_stems): the members of one programme that carry the same stem id form one stem, a unit
// of the programme's length and rate behind the programmes.  Sample k of a stem is mix_acc over the stem's own members
// alone -- ascending utterance index, the first term starts the sum, acc + t behind it, +0.0 under none: the mix rule
// over a subset.  With kMixFit and s_p != 1 the stored value is acc * s_p, s_p the PROGRAMME's scale; a stem has no
// scale of its own and is not held under the ceiling (a stem may peak above its mixture; a clamp would break
// additivity).  The 16-bit sink clamps and truncates as it always does.
// So, in f64 with s_p == 1 and every unmuted member under an id: at a sample under at most two members the stems added
// in unit order equal the mixture (==); under a depth d only the association differs, |sum - mix| <= (d - 1) 2^-52
// sum |t|; in 16 bits, where no term and no sum leaves [-32768, 32767], the stems' sum is within d counts.
constexpr uint32_t kMixNoStem = 0xffffffffu; // JB_MIX_NO_STEM: the utterance belongs to no stem
constexpr uint32_t kMixStemLevels = 1u;      // JB_MIX_STEM_LEVELS
JB_JOIN_HD double mix_stem_fit(double acc, double s) { return acc * s; }

// One stem of a layout (unit P + its index)
struct MixStem {
    uint32_t programme, id; // the dense programme, the caller's id
    uint32_t n_members, reserved; // members that carry the id, muted ones and those of no samples included
    uint64_t first, end;    // [first, end): from the first sample to behind the last one of its unmuted members of at
                            // least one sample; 0, 0 without one
};

// ---- Levels (kMixStemLevels): E_s = sum s[k]^2, D = sum s[k] m[k] over the programme's tiles that touch the stem's
// extent, E_p = sum m[k]^2 over all of the programme's tiles, of the units as stored (a 16-bit sample enters as its
// (double)).  The order is the noise stage's (jb_noise.h), stated again here (this header is compiled where that one is
// not): tiles of kLevelTile samples in programme coordinates; partial l of tile i takes the samples
// i kLevelTile + l + kLevelLanes j, j = 0, 1, ... below the programme's length: the first product starts it, each later
// one is fused on (fma), a partial without a sample is +0.0; the partials fold by p[l] = p[l] + p[l + h], h = 128 ... 1;
// the tile sums are added in ascending order, the first tile starts the sum (no tile: +0.0)
constexpr uint32_t kLevelTile = 1024, kLevelLanes = 256, kLevelWave = 64;
constexpr uint64_t level_tiles(uint64_t n) { return (n + kLevelTile - 1) / kLevelTile; }
// the tiles [*t0, *t0 + count) of a programme of n samples that touch [first, end)
JB_JOIN_HD uint64_t level_extent_tiles(uint64_t first, uint64_t end, uint64_t *t0)
{
    *t0 = first / kLevelTile;
    return end > first ? (end + kLevelTile - 1) / kLevelTile - *t0 : 0;
}
// at(k, &a, &b): the two factors of sample k
template <class Z> JB_JOIN_HD double level_partial(uint64_t N, uint64_t i, uint32_t l, Z at)
{
    double p = 0.0;
    bool first = true;
    for (uint32_t j = 0; j < kLevelTile / kLevelLanes; j++) {
        const uint64_t k = i * kLevelTile + l + (uint64_t)kLevelLanes * j;
        if (k >= N)
            break;
        double a, b;
        at(k, &a, &b);
        p = first ? a * b : __builtin_fma(a, b, p);
        first = false;
    }
    return p;
}
// What the fold leaves of one unit: a stem's E_s and D, a programme's E_p (twice)
struct MixSums {
    double e, d;
};
// One item of a level launch: the sums of unit `unit` (a of N samples) against its programme m over the tiles
// [tile0, tile0 + nt) in programme coordinates; a programme's own item has a == m.  t0: the prefix sum of the list's
// tiles, s0: the item's first tile in the tile-sum scratch
struct LevelItem {
    const void *a, *m;
    uint64_t n, tile0, nt, t0, s0;
    uint32_t unit, self;
};
// The host's statement of the whole order: sum a[k] b[k] over the tiles [t0, t0 + nt) of units of N samples
template <class T> inline double level_sum_host(const T *a, const T *b, uint64_t N, uint64_t t0, uint64_t nt)
{
    double S = 0.0;
    for (uint64_t i = t0; i < t0 + nt; i++) {
        double p[kLevelLanes];
        for (uint32_t l = 0; l < kLevelLanes; l++)
            p[l] = level_partial(N, i, l, [&](uint64_t k, double *x, double *y) {
                *x = (double)a[k];
                *y = (double)b[k];
            });
        for (uint32_t h = kLevelLanes / 2; h; h >>= 1)
            for (uint32_t l = 0; l < h; l++)
                p[l] = p[l] + p[l + h];
        S = i == t0 ? p[0] : S + p[0];
    }
    return S;
}
// The three dB values of a stem report, from the three sums, in long double: +INFINITY where a denominator is not above
// 0, -INFINITY where E_s == 0 (a host function)
inline void level_db_of(double e_s, double d, double e_p, double *level, double *sir, double *si_sdr)
{
    const long double Es = e_s, D = d, Ep = e_p;
    auto db = [&](long double num, long double den) {
        if (e_s == 0.0)
            return -(double)INFINITY;
        if (!(den > 0.0L))
            return (double)INFINITY;
        return (double)(10.0L * log10l(num / den));
    };
    *level = db(Es, Ep);
    *sir = db(Es, Ep - 2.0L * D + Es);
    const long double a = e_s == 0.0 ? 0.0L : D * D / Es;
    *si_sdr = db(a, Ep - a);
}

} // namespace jb

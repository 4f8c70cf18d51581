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

} // namespace jb

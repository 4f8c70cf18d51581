#pragma once
// jb_limiter.h -- the look-ahead peak limiter (include/jbonsai_amd.h "Limiter"): the request's check and the rules of
// one sample, stated once for the kernel (jb_limiter.hip) and for the host seam (jb_limiter.cpp), and the stage's work
// list.  Plain C++17; under hipcc the rules compile for the host and the device alike.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
// (spelt without the HIP runtime header, as jb_adpcm.h)
#define JB_LIM_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_LIM_HD inline
#endif

namespace jb {

constexpr uint32_t kLimLanes = 256;
constexpr uint32_t kLimTile = 1024;    // samples per workgroup, from the utterance's length alone
constexpr uint32_t kLimMaxSpan = 2048; // 2 L + H at most: a tile's halo
constexpr uint32_t kLimMaxL = kLimMaxSpan / 2;
constexpr uint32_t kLimTaps = 12, kLimMaxF = 64; // the true-peak interpolator's (kTpTaps, kTpMaxF of jb_host.h)
// b[n - 1] reads u[n - 6 .. n + 5], b[n] reads u[n - 5 .. n + 6]
constexpr uint32_t kLimTpHalo = 6;
constexpr uint32_t kLimExact = 1u, kLimOff = 2u; // JB_LIMITER_EXACT, JB_LIMITER_OFF
constexpr double kLimDefLookaheadMs = 2.0, kLimDefHoldMs = 8.0, kLimDefDepthDb = 6.0;
constexpr double kLimMaxLookaheadMs = 10.0, kLimMaxHoldMs = 50.0, kLimMaxDepthDb = 24.0;

// jb_limiter_opts of the public header (this header stands without it)
struct LimOpts {
    double lookahead_ms, hold_ms, max_reduction_db;
    uint32_t flags, reserved;
};

// The request with its defaults filled in (flags: kLimExact, or kLimOff alone); false (and *field names what is wrong) for a request that is refused
JB_LIM_HD bool lim_resolve(const LimOpts *o, LimOpts *out, const char **field)
{
    LimOpts r = {kLimDefLookaheadMs, kLimDefHoldMs, kLimDefDepthDb, kLimExact, 0};
    if (o) {
        if (o->flags & ~(kLimExact | kLimOff)) {
            *field = "flags";
            return false;
        }
        if (o->reserved) {
            *field = "reserved";
            return false;
        }
        if (o->flags & kLimOff) { // (its values are not read)
            r.flags = kLimOff;
            *out = r;
            return true;
        }
        const bool exact = (o->flags & kLimExact) != 0;
        if (exact || o->lookahead_ms != 0.0)
            r.lookahead_ms = o->lookahead_ms;
        if (exact || o->hold_ms != 0.0)
            r.hold_ms = o->hold_ms;
        if (exact || o->max_reduction_db != 0.0)
            r.max_reduction_db = o->max_reduction_db;
    }
    if (!(r.lookahead_ms > 0.0 && r.lookahead_ms <= kLimMaxLookaheadMs)) { // (a NaN fails every comparison)
        *field = "lookahead_ms";
        return false;
    }
    if (!(r.hold_ms >= 0.0 && r.hold_ms <= kLimMaxHoldMs)) {
        *field = "hold_ms";
        return false;
    }
    if (!(r.max_reduction_db >= 0.0 && r.max_reduction_db <= kLimMaxDepthDb)) {
        *field = "max_reduction_db";
        return false;
    }
    *out = r;
    return true;
}

// ms at hz in samples: floor(v + 0.5)
JB_LIM_HD uint64_t lim_samples(double ms, uint32_t hz) { return (uint64_t)floor(ms * (double)hz / 1000.0 + 0.5); }
JB_LIM_HD uint32_t lim_lookahead(const LimOpts &r, uint32_t hz)
{
    const uint64_t L = lim_samples(r.lookahead_ms, hz);
    return (uint32_t)(L < 1 ? 1 : L);
}
JB_LIM_HD uint32_t lim_hold(const LimOpts &r, uint32_t hz) { return (uint32_t)lim_samples(r.hold_ms, hz); }

// the ceiling in sample units
JB_LIM_HD double lim_ceiling(double ceiling_db) { return 32768.0 * pow(10.0, ceiling_db / 20.0); }

// step 2: b of the 12 samples v[0..12) = u[n - 5 .. n + 6], h the [F - 1][12] taps
template <class H> JB_LIM_HD double lim_between(H h, uint32_t F, const double *v)
{
    double b = 0.0;
    for (uint32_t p = 0; p + 1 < F; p++) {
        double y = h[p * kLimTaps] * v[0];
#pragma unroll
        for (uint32_t q = 1; q < kLimTaps; q++)
            y = __builtin_fma(h[p * kLimTaps + q], v[q], y);
        b = fmax(b, fabs(y));
    }
    return b;
}

// step 3
JB_LIM_HD double lim_ratio(double c, double d) { return d > c ? c / d : 1.0; }

// step 5 without its last minimum: m(j) = m[n - j], j = 0..L
template <class W, class M> JB_LIM_HD double lim_smooth(W w, uint32_t L, M m)
{
    double v = m(0), lo = v;
    double a = w[0] * v;
    for (uint32_t j = 1; j <= L; j++) {
        v = m(j);
        lo = fmin(lo, v);
        a = __builtin_fma(w[j], v, a);
    }
    return lo == 1.0 ? 1.0 : a;
}

// the rest of step 5, and step 6
JB_LIM_HD double lim_gain(double a, double r) { return fmin(a, r); }
JB_LIM_HD double lim_out(double u, double a, double c) { return fmin(fmax(u * a, -c), c); }

// the report's first field of the smallest a
JB_LIM_HD double lim_reduction_db(double min_a) { return min_a < 1.0 ? -20.0 * log10(min_a) : 0.0; }

// The device table of one (rate, L, H, detector) class
struct LimiterClass {
    uint32_t L, H;
    uint32_t F;   // 1: the sample detector; else the true-peak oversampling factor of the rate
    uint32_t pad;
    double w[kLimMaxL + 1];
    double tp[(kLimMaxF - 1) * kLimTaps];
};
constexpr uint32_t kLimNoSlot = 0xffffffffu;
// One utterance of a limiter launch.  Launch lists are in utterance order; t0 is the prefix sum of the list's tiles,
// s0 the utterance's place in the per-tile scratch (fixed per batch)
struct LimiterUtt {
    const double *x; // f64 PCM in front of the gain
    void *y;         // output (f64 or i16, by the launch)
    uint64_t n, t0, s0;
    double c;        // the ceiling in sample units (with cls == kLimNoSlot: unused)
    double g;        // the gain where slot == kLimNoSlot
    uint32_t slot;   // the utterance's LoudnessResult, whose g is the gain; kLimNoSlot: g above
    uint32_t cls;    // its LimiterClass; kLimNoSlot: not limited, y = x g
    uint32_t rslot;  // its place in the results
    uint32_t pad;
};
struct LimiterTile { // per tile: the smallest a and the samples with a < 1
    double min_a;
    uint64_t count;
};
using LimiterResult = LimiterTile; // per utterance: the same over its tiles

JB_LIM_HD uint64_t limiter_tiles(uint64_t n) { return (n + kLimTile - 1) / kLimTile; }

} // namespace jb

#pragma once
// jb_filter.h -- the output filter (include/jbonsai_amd.h "Filter"): a cascade of up to four second-order sections at
// the output rate.  The rules of one sample, stated once for the kernels (jb_filter.hip) and for the host seam
// (jb_filter.cpp); the design of a section (Audio EQ Cookbook forms, host only: the device never calls sin or cos);
// the stage's device table and work list.
// Plain C++17; under hipcc the recursion compiles for the host and the device alike.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define JB_FILT_HD __host__ __device__ __forceinline__
#else
#define JB_FILT_HD inline
#endif

namespace jb {

// JB_FILTER_* of the public header, as plain values (this header stands without it)
constexpr uint32_t kFiltHighpass = 1, kFiltLowpass = 2, kFiltPeaking = 3, kFiltLowshelf = 4, kFiltHighshelf = 5,
                   kFiltNotch = 6, kFiltRaw = 7;
constexpr uint32_t kFiltMaxSections = 4;
constexpr uint32_t kFiltMaxD = 2 * kFiltMaxSections; // doubles of state of the longest cascade: a tile's slot in `st`
constexpr uint32_t kFiltS = 16;                      // samples of a lane's segment
constexpr uint32_t kFiltLanes = 256;
constexpr uint32_t kFiltTile = kFiltLanes * kFiltS;  // 4,096 samples per workgroup: from the utterance's length alone
// the utterance scan gives every lane 2^j tiles, so that every transition it needs is a table entry A^(4096 2^k):
// 2^j <= 2^20 tiles per lane, times up to 32 lanes back
constexpr uint32_t kFiltTilePows = 26;
constexpr uint64_t kFiltMaxTiles = 64ull << 20;

// One section: b0 b1 b2 a1 a2 with a0 = 1 (jb_biquad)
constexpr uint32_t kFiltCoefs = 5;

// One sample through a cascade of ns sections, transposed direct form II with explicit FMAs, every section in the
// term order of the loudness K-weighting (jb_loudness.hip ln_step).  c: [ns][5], s: [ns][2].  This one function is the
// host seam's recursion, the recursion of a lane's segment, and (x = 0 from a unit state) a column of the transition
// matrix
JB_FILT_HD double filt_step(const double *c, double *s, double x, uint32_t ns)
{
    for (uint32_t k = 0; k < ns; k++) {
        const double *b = c + k * kFiltCoefs;
        double *z = s + 2 * k;
        const double y = __builtin_fma(b[0], x, z[0]);
        z[0] = __builtin_fma(b[1], x, __builtin_fma(-b[3], y, z[1]));
        z[1] = __builtin_fma(b[2], x, -b[4] * y);
        x = y;
    }
    return x;
}

// The device table of one distinct (filter, output rate) pair, host-built.  D = 2 ns; matrices are D x D, row-major,
// packed; the identity class (ns = 0: a copy) has none
struct FilterClass {
    double c[kFiltMaxSections * kFiltCoefs];
    double P[8][kFiltMaxD * kFiltMaxD];              // A^(S 2^k), k = 0..7: over 2^k segments
    double Pt[kFiltTilePows][kFiltMaxD * kFiltMaxD]; // A^(4096 2^k): over 2^k tiles
    uint32_t ns, pad_;
};

// One utterance of a filter launch.  A launch list is sorted by the section count of its utterances' classes; t0 is
// the prefix sum of tiles within the utterances of one count, tile0 the utterance's place in the per-tile state
// scratch (kFiltMaxD doubles per tile, fixed per batch)
struct FilterUtt {
    const double *x; // f64 PCM, 16-bit scale
    void *y;         // f64 or 16-bit, by the launch
    uint64_t n, tile0, t0;
    uint32_t ntiles, cls;
};

constexpr uint64_t filter_tiles(uint64_t n) { return (n + kFiltTile - 1) / kFiltTile; }

// A section request, as jb_filter_section lays it out
struct FilterSection {
    uint32_t kind, reserved;
    double f0_hz, q, gain_db;
    double raw[kFiltCoefs];
};
struct FilterSpec {
    FilterSection section[kFiltMaxSections];
    uint32_t n_sections, reserved;
};

// The poles of 1 + a1 z^-1 + a2 z^-2 strictly inside the unit circle
inline bool filt_stable(double a1, double a2) { return fabs(a2) < 1.0 && fabs(a1) < 1.0 + a2; }

// nullptr: the section is accepted at `hz`; else the name of the first field that is not (host only)
inline const char *filt_section_bad_field(const FilterSection &s, uint32_t hz)
{
    if (s.kind < kFiltHighpass || s.kind > kFiltRaw)
        return "kind";
    if (s.reserved)
        return "reserved";
    if (s.kind == kFiltRaw) {
        static const char *const names[kFiltCoefs] = {"b0", "b1", "b2", "a1", "a2"};
        for (uint32_t i = 0; i < kFiltCoefs; i++)
            if (!isfinite(s.raw[i]))
                return names[i];
        if (!(fabs(s.raw[4]) < 1.0))
            return "a2";
        if (!filt_stable(s.raw[3], s.raw[4]))
            return "a1";
        return nullptr;
    }
    if (!isfinite(s.f0_hz) || !(s.f0_hz > 0.0) || !(s.f0_hz < 0.5 * (double)hz))
        return "f0_hz";
    if (!isfinite(s.q) || !(s.q > 0.0))
        return "q";
    if (!isfinite(s.gain_db))
        return "gain_db";
    return nullptr;
}

// The Audio EQ Cookbook forms of an accepted section at fs = hz, normalised by a0 (host only).  w0 = 2 pi f0 / fs and
// alpha = sin(w0) / (2 q) for every kind; the shelves use the same alpha with A = 10^(gain_db / 40)
inline void filt_design_section(const FilterSection &s, uint32_t hz, double *c)
{
    if (s.kind == kFiltRaw) {
        for (uint32_t i = 0; i < kFiltCoefs; i++)
            c[i] = s.raw[i];
        return;
    }
    const double w0 = 2.0 * M_PI * s.f0_hz / (double)hz;
    const double cw = cos(w0), alpha = sin(w0) / (2.0 * s.q);
    const double A = pow(10.0, s.gain_db / 40.0);
    double b0, b1, b2, a0, a1, a2;
    switch (s.kind) {
    case kFiltHighpass:
        b0 = (1.0 + cw) / 2.0, b1 = -(1.0 + cw), b2 = (1.0 + cw) / 2.0;
        a0 = 1.0 + alpha, a1 = -2.0 * cw, a2 = 1.0 - alpha;
        break;
    case kFiltLowpass:
        b0 = (1.0 - cw) / 2.0, b1 = 1.0 - cw, b2 = (1.0 - cw) / 2.0;
        a0 = 1.0 + alpha, a1 = -2.0 * cw, a2 = 1.0 - alpha;
        break;
    case kFiltPeaking:
        b0 = 1.0 + alpha * A, b1 = -2.0 * cw, b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A, a1 = -2.0 * cw, a2 = 1.0 - alpha / A;
        break;
    case kFiltNotch:
        b0 = 1.0, b1 = -2.0 * cw, b2 = 1.0;
        a0 = 1.0 + alpha, a1 = -2.0 * cw, a2 = 1.0 - alpha;
        break;
    case kFiltLowshelf: {
        const double t = 2.0 * sqrt(A) * alpha;
        b0 = A * ((A + 1.0) - (A - 1.0) * cw + t), b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cw);
        b2 = A * ((A + 1.0) - (A - 1.0) * cw - t);
        a0 = (A + 1.0) + (A - 1.0) * cw + t, a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cw);
        a2 = (A + 1.0) + (A - 1.0) * cw - t;
        break;
    }
    default: { // kFiltHighshelf
        const double t = 2.0 * sqrt(A) * alpha;
        b0 = A * ((A + 1.0) + (A - 1.0) * cw + t), b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cw);
        b2 = A * ((A + 1.0) + (A - 1.0) * cw - t);
        a0 = (A + 1.0) - (A - 1.0) * cw + t, a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cw);
        a2 = (A + 1.0) - (A - 1.0) * cw - t;
        break;
    }
    }
    c[0] = b0 / a0, c[1] = b1 / a0, c[2] = b2 / a0, c[3] = a1 / a0, c[4] = a2 / a0;
}

// 0: the filter is accepted at `hz` and c ([n_sections][5], may be null) holds its coefficients; else 1 + the index of
// the offending section (kFiltMaxSections + 1: n_sections itself) and *field names what is wrong with it (host only)
inline uint32_t filt_design(const FilterSpec &f, uint32_t hz, double *c, const char **field)
{
    if (f.n_sections > kFiltMaxSections || f.reserved) {
        *field = f.n_sections > kFiltMaxSections ? "n_sections" : "reserved";
        return kFiltMaxSections + 1;
    }
    for (uint32_t k = 0; k < f.n_sections; k++) {
        if ((*field = filt_section_bad_field(f.section[k], hz)))
            return k + 1;
        double w[kFiltCoefs];
        filt_design_section(f.section[k], hz, w);
        bool ok = filt_stable(w[3], w[4]);
        for (uint32_t i = 0; i < kFiltCoefs; i++)
            ok = ok && isfinite(w[i]);
        if (!ok) {
            *field = "poles";
            return k + 1;
        }
        if (c)
            for (uint32_t i = 0; i < kFiltCoefs; i++)
                c[k * kFiltCoefs + i] = w[i];
    }
    return 0;
}

} // namespace jb

#pragma once
// jb_melspec.h -- mel spectrograms in the librosa / Whisper convention (include/jbonsai_amd.h "Mel spectrograms"): the
// geometry of a unit, the tables of one (rate, options) pair, the pass schedule and the butterflies of radix 2, 3 and 5
// of one frame's mixed-radix transform, stated once for the kernel (jb_melspec.hip) and for the host half
// (jb_melspec.cpp), and the stage's work list.  Plain C++17; under hipcc the rules compile for the host and the device
// alike.  The radix-2 butterfly and the untangling of the packed transform are jb_fbank.h's (they hold for any even N).
#include "jb_fbank.h"

#define JB_MEL_HD JB_FBANK_HD

namespace jb {

// jb_melspec_opts of the public header, restated (jb_melspec.cpp asserts the two agree)
struct MelOpts {
    uint32_t n_fft, win_length, hop_length, n_mels;
    double f_min_hz, f_max_hz;
    double floor, range, offset, scale;
    uint32_t mel_scale, norm, pad, log, flags;
    uint32_t reserved[3];
};
static_assert(sizeof(MelOpts) == 96 && offsetof(MelOpts, f_min_hz) == 16 && offsetof(MelOpts, floor) == 32 &&
                  offsetof(MelOpts, mel_scale) == 64 && offsetof(MelOpts, flags) == 80 &&
                  offsetof(MelOpts, reserved) == 84,
              "jb_melspec_opts is 96 bytes");

constexpr uint32_t kMelHtk = 0, kMelSlaney = 1;                        // JB_MEL_HTK, _SLANEY
constexpr uint32_t kMelNormNone = 0, kMelNormSlaney = 1;               // JB_MEL_NORM_NONE, _SLANEY
constexpr uint32_t kMelPadReflect = 0, kMelPadZero = 1, kMelPadNone = 2; // JB_MEL_PAD_REFLECT, _ZERO, _NONE
constexpr uint32_t kMelLogNone = 0, kMelLogLn = 1, kMelLog10 = 2, kMelLogDb = 3; // JB_MEL_LOG_NONE, _LN, _LOG10, _DB
constexpr uint32_t kMelMagnitude = 1, kMelDropLast = 2, kMelF64 = 4;   // JB_MEL_MAGNITUDE, _DROP_LAST, _F64
constexpr uint32_t kMelMinFft = 64, kMelMaxFft = 4096, kMelMaxMels = 128;
constexpr uint32_t kMelLanes = 256;             // threads of a workgroup
constexpr uint32_t kMelPoints = kMelMaxFft / 2; // complex points of the largest packed transform
constexpr uint32_t kMelMaxPasses = 11;          // 2048 = 2^11

// Lanes that share a frame and frames a workgroup takes, by n_fft alone: a wave up to 1024, two up to 2048, four above
constexpr uint32_t mel_frame_lanes(uint32_t n_fft) { return n_fft <= 1024 ? 64 : n_fft <= 2048 ? 128 : 256; }
constexpr uint32_t mel_wg_frames(uint32_t n_fft) { return kMelLanes / mel_frame_lanes(n_fft); }
constexpr uint64_t mel_elem(uint32_t flags) { return (flags & kMelF64) ? 8 : 4; }

// The options at one rate, resolved
struct MelGeom {
    uint32_t n_fft, wl, hop, n_mels;
    uint32_t woff; // the window's place in the frame: (n_fft - wl) / 2
    double f_min, f_max;
    double floor;   // the clamp in front of the logarithm
    double y_floor; // its logarithm (ln, log10 or 10 log10 by `log`) in long double, rounded once: what an energy at
                    // or below the floor gives; under JB_MEL_LOG_NONE unused
    double scale;
};

// T of n samples
constexpr uint64_t mel_frames(uint64_t n, uint32_t n_fft, uint32_t hop, uint32_t pad, uint32_t flags)
{
    if (pad == kMelPadNone)
        return n >= n_fft ? 1 + (n - n_fft) / hop : 0;
    if (pad == kMelPadReflect && n <= n_fft / 2)
        return 0;
    const uint64_t T = 1 + n / hop;
    return (flags & kMelDropLast) ? T - 1 : T;
}
// Sample `idx` of the padded unit (idx may lie outside [0, n)) as an index into the unit, or -1: it reads as 0.
// Reflection does not repeat the edge sample; with n > n_fft / 2 one reflection reaches every sample a frame asks for
JB_MEL_HD int64_t mel_sample_at(int64_t idx, uint64_t n, uint32_t pad)
{
    if (pad == kMelPadReflect) {
        if (idx < 0)
            idx = -idx;
        else if ((uint64_t)idx >= n)
            idx = 2 * (int64_t)(n - 1) - idx;
    }
    return idx >= 0 && (uint64_t)idx < n ? idx : -1;
}

// What is wrong with the options whatever the rate, naming the field; null: nothing
inline const char *mel_opts_fault(const MelOpts &o)
{
    if (o.reserved[0] || o.reserved[1] || o.reserved[2])
        return "reserved must be 0";
    if (o.flags & ~(kMelMagnitude | kMelDropLast | kMelF64))
        return "flags has an unknown bit";
    if (o.mel_scale != kMelHtk && o.mel_scale != kMelSlaney)
        return "mel_scale is JB_MEL_HTK or JB_MEL_SLANEY";
    if (o.norm != kMelNormNone && o.norm != kMelNormSlaney)
        return "norm is JB_MEL_NORM_NONE or JB_MEL_NORM_SLANEY";
    if (o.pad > kMelPadNone)
        return "pad is JB_MEL_PAD_REFLECT, JB_MEL_PAD_ZERO or JB_MEL_PAD_NONE";
    if (o.log > kMelLogDb)
        return "log is JB_MEL_LOG_NONE, JB_MEL_LOG_LN, JB_MEL_LOG_LOG10 or JB_MEL_LOG_DB";
    if ((o.flags & kMelDropLast) && o.pad == kMelPadNone)
        return "flags: JB_MEL_DROP_LAST needs JB_MEL_PAD_REFLECT or JB_MEL_PAD_ZERO";
    uint32_t rest = o.n_fft;
    for (uint32_t p : {2u, 3u, 5u})
        while (rest && rest % p == 0)
            rest /= p;
    if (o.n_fft < kMelMinFft || o.n_fft > kMelMaxFft || (o.n_fft & 1) || rest != 1)
        return "n_fft is even, in 64..4096 and has no prime factor above 5";
    if (o.win_length && (o.win_length < 2 || o.win_length > o.n_fft))
        return "win_length is 0 (n_fft) or in 2..n_fft";
    if (o.hop_length < 1)
        return "hop_length is at least 1";
    if (o.n_mels < 1 || o.n_mels > kMelMaxMels)
        return "n_mels is in 1..128";
    if (!(o.f_min_hz >= 0.0) || !std::isfinite(o.f_min_hz))
        return "f_min_hz is at least 0";
    if (!(o.f_max_hz >= 0.0) || !std::isfinite(o.f_max_hz))
        return "f_max_hz is 0 (half the rate) or above f_min_hz";
    if (!(o.floor >= 0.0) || !std::isfinite(o.floor))
        return "floor is a positive number, or 0 for 1e-10";
    if (!(o.range >= 0.0) || !std::isfinite(o.range))
        return "range is 0 (none) or a positive number";
    if (!std::isfinite(o.offset))
        return "offset is a finite number";
    if (!std::isfinite(o.scale))
        return "scale is a finite number, or 0 for 1.0";
    return nullptr;
}

// What is out of its limits at hz, naming the field; null: nothing, and the geometry is in *out (may be null)
inline const char *mel_geometry_fault(const MelOpts &o, uint32_t hz, MelGeom *out)
{
    MelGeom g{};
    if (hz == 0)
        return "the rate is 0";
    g.n_fft = o.n_fft;
    g.wl = o.win_length ? o.win_length : o.n_fft;
    g.woff = (g.n_fft - g.wl) / 2;
    g.hop = o.hop_length;
    g.n_mels = o.n_mels;
    g.f_min = o.f_min_hz;
    g.f_max = o.f_max_hz == 0.0 ? 0.5 * hz : o.f_max_hz;
    g.floor = o.floor == 0.0 ? 1e-10 : o.floor;
    const long double lf = std::log((long double)g.floor);
    g.y_floor = o.log == kMelLogLn      ? (double)lf
                : o.log == kMelLog10    ? (double)std::log10((long double)g.floor)
                : o.log == kMelLogDb    ? (double)(10.0L * std::log10((long double)g.floor))
                                        : 0.0;
    g.scale = o.scale == 0.0 ? 1.0 : o.scale;
    if (!(g.f_min < g.f_max))
        return "f_min_hz is below f_max_hz";
    if (g.f_max > 0.5 * hz)
        return "f_max_hz is at most half the rate";
    if (out)
        *out = g;
    return nullptr;
}
// Pure, for a plan: false where the options or their geometry at hz are refused
inline bool mel_geometry_quiet(const MelOpts &opts, uint32_t hz, MelGeom *g)
{
    return !mel_opts_fault(opts) && !mel_geometry_fault(opts, hz, g);
}
// JB_OK, or JB_ERR_INVALID with set_error naming the field (jb_melspec.cpp)
int mel_check_opts(const MelOpts *opts, const char *who);
int mel_geometry(const MelOpts *opts, uint32_t hz, const char *who, MelGeom *g);

// The passes of the packed transform of M = n_fft / 2 points: the factors 5, then 3, then 2 of M.  Pass s has radix
// r[s] and span L[s] = r[0] ... r[s - 1]; inv[s] = floor(2^32 / L[s]) + 1 divides a butterfly's index by the span
// (mel_div: exact for indices below 2^16; L = 1 is spelt out)
struct MelSchedule {
    uint32_t n = 0;
    uint32_t r[kMelMaxPasses] = {}, L[kMelMaxPasses] = {}, inv[kMelMaxPasses] = {};
};
inline MelSchedule mel_schedule(uint32_t M)
{
    MelSchedule s;
    uint32_t span = 1;
    for (uint32_t p : {5u, 3u, 2u})
        while (M % p == 0 && s.n < kMelMaxPasses) {
            s.r[s.n] = p;
            s.L[s.n] = span;
            s.inv[s.n] = span > 1 ? (uint32_t)(0x100000000ull / span) + 1 : 0;
            s.n++;
            span *= p;
            M /= p;
        }
    return s;
}
// Where input point j of the transform is stored: its digits in the schedule's radices, reversed
inline uint32_t mel_digit_reverse(const MelSchedule &s, uint32_t j)
{
    uint32_t at = 0;
    for (uint32_t p = s.n; p-- > 0;) {
        at += (j % s.r[p]) * s.L[p];
        j /= s.r[p];
    }
    return at;
}
JB_MEL_HD uint32_t mel_div(uint32_t j, uint32_t L, uint32_t inv)
{
    return L == 1 ? j : (uint32_t)(((uint64_t)j * inv) >> 32);
}

// The butterflies, decimation in time: the inputs behind the first are multiplied by their twiddles (c + i sn: powers of
// W_{rL}), then the r-point transform is taken with W_r = e^{-2 pi i / r}; written product by product and sum by sum
// (no contraction: the translation units are built with it off)
JB_MEL_HD void mel_twiddle(double &r, double &i, double c, double sn)
{
    const double tr = c * r - sn * i, ti = c * i + sn * r;
    r = tr;
    i = ti;
}
JB_MEL_HD void mel_bfly3(double &ar, double &ai, double &br, double &bi, double &cr, double &ci, double c1, double s1,
                         double c2, double s2)
{
    constexpr double kS3 = 0.86602540378443864676; // sin(2 pi / 3)
    mel_twiddle(br, bi, c1, s1);
    mel_twiddle(cr, ci, c2, s2);
    const double tr = br + cr, ti = bi + ci;
    const double dr = kS3 * (br - cr), di = kS3 * (bi - ci);
    const double mr = ar - 0.5 * tr, mi = ai - 0.5 * ti;
    ar = ar + tr;
    ai = ai + ti;
    br = mr + di; // m - i d
    bi = mi - dr;
    cr = mr - di; // m + i d
    ci = mi + dr;
}
JB_MEL_HD void mel_bfly5(double &ar, double &ai, double &br, double &bi, double &cr, double &ci, double &dr, double &di,
                         double &er, double &ei, const double *c, const double *s)
{
    constexpr double kC1 = 0.30901699437494742410, kC2 = -0.80901699437494742410; // cos(2 pi / 5), cos(4 pi / 5)
    constexpr double kS1 = 0.95105651629515357212, kS2 = 0.58778525229247312917;  // sin(2 pi / 5), sin(4 pi / 5)
    mel_twiddle(br, bi, c[0], s[0]);
    mel_twiddle(cr, ci, c[1], s[1]);
    mel_twiddle(dr, di, c[2], s[2]);
    mel_twiddle(er, ei, c[3], s[3]);
    const double s1r = br + er, s1i = bi + ei, s2r = cr + dr, s2i = ci + di;
    const double d1r = br - er, d1i = bi - ei, d2r = cr - dr, d2i = ci - di;
    const double m1r = (ar + kC1 * s1r) + kC2 * s2r, m1i = (ai + kC1 * s1i) + kC2 * s2i;
    const double m2r = (ar + kC2 * s1r) + kC1 * s2r, m2i = (ai + kC2 * s1i) + kC1 * s2i;
    const double n1r = kS1 * d1r + kS2 * d2r, n1i = kS1 * d1i + kS2 * d2i;
    const double n2r = kS2 * d1r - kS1 * d2r, n2i = kS2 * d1i - kS1 * d2i;
    ar = (ar + s1r) + s2r;
    ai = (ai + s1i) + s2i;
    br = m1r + n1i; // m1 - i n1
    bi = m1i - n1r;
    er = m1r - n1i; // m1 + i n1
    ei = m1i + n1r;
    cr = m2r + n2i; // m2 - i n2
    ci = m2i - n2r;
    dr = m2r - n2i; // m2 + i n2
    di = m2i + n2r;
}
// Butterfly j (of M / r) of a pass of radix r and span L of the in-place transform of M points whose input was stored
// in digit-reversed order.  twc, tws: cos and -sin of 2 pi p / M, p < M; at(i): where point i lies in re and im
template <class At>
JB_MEL_HD void mel_butterfly(double *re, double *im, const double *twc, const double *tws, uint32_t M, uint32_t r,
                             uint32_t L, uint32_t inv, uint32_t j, At at)
{
    const uint32_t blk = mel_div(j, L, inv), pos = j - blk * L;
    const uint32_t i0 = blk * L * r + pos;
    const uint32_t p = (M / (L * r)) * pos; // W_{rL}^pos = W_M^p; q p < M for q < r
    const uint32_t a = at(i0), b = at(i0 + L);
    if (r == 2) {
        fbank_bfly(re[a], im[a], re[b], im[b], twc[p], tws[p]);
    } else if (r == 3) {
        const uint32_t c = at(i0 + 2 * L);
        mel_bfly3(re[a], im[a], re[b], im[b], re[c], im[c], twc[p], tws[p], twc[2 * p], tws[2 * p]);
    } else {
        const uint32_t c = at(i0 + 2 * L), d = at(i0 + 3 * L), e = at(i0 + 4 * L);
        const double tc[4] = {twc[p], twc[2 * p], twc[3 * p], twc[4 * p]};
        const double ts[4] = {tws[p], tws[2 * p], tws[3 * p], tws[4 * p]};
        mel_bfly5(re[a], im[a], re[b], im[b], re[c], im[c], re[d], im[d], re[e], im[e], tc, ts);
    }
}

// The tables of one geometry, built in long double and rounded once
struct MelTables {
    std::vector<double> win;      // [wl]
    std::vector<double> tw;       // [n_fft / 2 + 1][2]: cos, -sin of 2 pi k / n_fft (the untangling)
    std::vector<double> twc, tws; // [n_fft / 2]: cos, -sin of 2 pi p / (n_fft / 2) (the passes)
    std::vector<uint32_t> rev;    // [n_fft / 2]: mel_digit_reverse
    MelSchedule sched;
    std::vector<double> wts;      // the filters' weights over their supports, filter after filter
    std::vector<uint32_t> first, count, woff, rise; // [n_mels], as FbankTables has them
    std::vector<double> wr, wf;   // [n_fft / 2 + 1] the bin's weight in its rising / falling filter (0: none)
    double wmax = 0.0;
};
void mel_window(uint32_t wl, double *w);
// dense [n_mels][n_fft / 2 + 1]
void mel_filterbank(const MelGeom &g, uint32_t hz, uint32_t mel_scale, uint32_t norm, double *W);
// false: a bin came out on the same side of two filters (not expected)
bool mel_tables(const MelGeom &g, uint32_t hz, const MelOpts &o, MelTables *t);

// The logarithm of step 7 and the affine step of step 9, one text for both sides
JB_MEL_HD double mel_log(double e, uint32_t log, double floor, double y_floor)
{
    if (log == kMelLogNone)
        return e;
    if (!(e > floor))
        return y_floor;
    return log == kMelLogLn ? ::log(e) : log == kMelLog10 ? ::log10(e) : 10.0 * ::log10(e);
}
JB_MEL_HD double mel_affine(double y, double offset, double scale) { return (y + offset) * scale; }

// The device's view of one geometry's tables
struct MelClass {
    const double *win, *tw, *twc, *tws, *wr, *wf;
    const uint32_t *rev, *first, *count, *rise;
    uint32_t n_fft, wl, woff, hop;
    uint32_t n_mels, flags, pad, log;
    uint32_t n_pass, pad0;
    uint32_t r[kMelMaxPasses], L[kMelMaxPasses], inv[kMelMaxPasses];
    uint32_t pad1;
    double floor, y_floor, range, offset, scale;
};

// One unit of a launch.  Launch lists are in unit order; g0 is the prefix sum of the list's workgroups
// (mel_wg_frames frames each; workgroups never cross units)
struct MelUtt {
    const double *x; // the chain's final f64 PCM, in 16-bit scale
    uint8_t *y;      // its [T][n_mels] elements, 16-byte aligned
    double *s;       // with range > 0: its [T][n_mels] f64 values in front of the clamp (scratch); else null
    uint64_t n, T, g0;
    uint32_t cls, pad;
};

} // namespace jb

#pragma once
// jb_fbank.h -- log-mel filterbank features (include/jbonsai_amd.h "Filterbank features"): the geometry of a unit, the
// tables of one (rate, options) pair, the butterfly and the untangling of one frame's transform, stated once for the
// kernel (jb_fbank.hip), for the host half (jb_fbank.cpp) and for the output plan (jb_output.cpp), and the stage's work
// list.  Plain C++17; under hipcc the rules compile for the host and the device alike.
#include <cmath>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#ifdef __HIPCC__
// (spelt without the HIP runtime header: jb_output.cpp includes this file without it)
#define JB_FBANK_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_FBANK_HD inline
#endif

namespace jb {

// jb_fbank_opts of the public header, restated (this header stands without it; jb_fbank.cpp asserts the two agree)
struct FbankOpts {
    uint32_t win_us, hop_us;
    uint32_t n_fft, n_mels;
    double f_min_hz, f_max_hz;
    double log_floor;
    uint32_t window, flags;
    uint32_t reserved[4];
};
static_assert(sizeof(FbankOpts) == 64 && offsetof(FbankOpts, f_min_hz) == 16 && offsetof(FbankOpts, window) == 40 &&
                  offsetof(FbankOpts, reserved) == 48,
              "jb_fbank_opts is 64 bytes");

constexpr uint32_t kFbHann = 0, kFbHamming = 1;                          // JB_FBANK_HANN, _HAMMING
constexpr uint32_t kFbCenter = 1, kFbLinear = 2, kFbUnit = 4, kFbF64 = 8; // JB_FBANK_CENTER, _LINEAR, _UNIT, _F64
constexpr uint32_t kFbMinFft = 64, kFbMaxFft = 4096, kFbMaxMels = 128;
constexpr uint32_t kFbLanes = 256; // threads of a workgroup
// The packed transform of a frame has M = n_fft / 2 complex points; a workgroup holds kFbPoints of them in LDS
constexpr uint32_t kFbPoints = kFbMaxFft / 2;

// Lanes that share a frame and frames a workgroup takes, by n_fft alone: a wave up to 1024, two at 2048, four at 4096
constexpr uint32_t fbank_frame_lanes(uint32_t n_fft) { return n_fft <= 1024 ? 64 : n_fft == 2048 ? 128 : 256; }
constexpr uint32_t fbank_wg_frames(uint32_t n_fft) { return kFbLanes / fbank_frame_lanes(n_fft); }

// The geometry of the options at one rate
struct FbankGeom {
    uint32_t wl, hop, n_fft, n_mels;
    double f_min, f_max, log_floor;
    double ln_floor; // ln(log_floor) in long double, rounded once: what an energy at or below the floor gives
};
constexpr uint64_t fbank_round_us(uint32_t hz, uint32_t us) { return ((uint64_t)hz * us + 500000) / 1000000; }
// T of n samples
constexpr uint64_t fbank_frames(uint64_t n, uint32_t wl, uint32_t hop, bool center)
{
    return center ? (n + hop - 1) / hop : n >= wl ? 1 + (n - wl) / hop : 0;
}
constexpr uint64_t fbank_elem(uint32_t flags) { return (flags & kFbF64) ? 8 : 4; }

// What is wrong with the options whatever the rate (a bad window, flag or reserved word, a log_floor that is no
// positive number, n_mels, n_fft or a band edge out of range), naming the field; null: nothing
inline const char *fbank_opts_fault(const FbankOpts &o)
{
    if (o.window != kFbHann && o.window != kFbHamming)
        return "window is JB_FBANK_HANN or JB_FBANK_HAMMING";
    if (o.flags & ~(kFbCenter | kFbLinear | kFbUnit | kFbF64))
        return "flags has an unknown bit";
    if (o.reserved[0] || o.reserved[1] || o.reserved[2] || o.reserved[3])
        return "reserved must be 0";
    if (!(o.log_floor >= 0.0) || !std::isfinite(o.log_floor))
        return "log_floor is a positive number, or 0 for 2^-52";
    if (o.n_mels < 1 || o.n_mels > kFbMaxMels)
        return "n_mels is in 1..128";
    if (o.n_fft && (o.n_fft < kFbMinFft || o.n_fft > kFbMaxFft || (o.n_fft & (o.n_fft - 1))))
        return "n_fft is 0 or a power of two in 64..4096";
    if (!(o.f_min_hz >= 0.0) || !std::isfinite(o.f_min_hz))
        return "f_min_hz is at least 0";
    if (!(o.f_max_hz >= 0.0) || !std::isfinite(o.f_max_hz))
        return "f_max_hz is 0 (half the rate) or above f_min_hz";
    return nullptr;
}

// What is out of its limits at hz, naming the field; null: nothing, and the geometry is in *out (may be null)
inline const char *fbank_geometry_fault(const FbankOpts &o, uint32_t hz, FbankGeom *out)
{
    FbankGeom g{};
    const uint64_t wl = fbank_round_us(hz, o.win_us), hop = fbank_round_us(hz, o.hop_us);
    if (hz == 0)
        return "the rate is 0";
    if (wl < 2 || wl > kFbMaxFft)
        return "win_us gives a window of 2..4096 samples (and at most n_fft)";
    if (hop < 1 || hop > 0xffffffffull)
        return "hop_us gives a hop of at least 1 sample";
    uint32_t n_fft = o.n_fft;
    if (!n_fft)
        for (n_fft = 1; n_fft < wl;)
            n_fft <<= 1;
    if (n_fft < kFbMinFft || n_fft > kFbMaxFft)
        return "n_fft (0: the smallest power of two that holds the window) is in 64..4096";
    if (wl > n_fft)
        return "win_us gives a window longer than n_fft";
    g.wl = (uint32_t)wl;
    g.hop = (uint32_t)hop;
    g.n_fft = n_fft;
    g.n_mels = o.n_mels;
    g.f_min = o.f_min_hz;
    g.f_max = o.f_max_hz == 0.0 ? 0.5 * hz : o.f_max_hz;
    g.log_floor = o.log_floor == 0.0 ? 0x1p-52 : o.log_floor;
    g.ln_floor = (double)std::log((long double)g.log_floor);
    if (!(g.f_min < g.f_max))
        return "f_min_hz is below f_max_hz";
    if (g.f_max > 0.5 * hz)
        return "f_max_hz is at most half the rate";
    if (out)
        *out = g;
    return nullptr;
}

// Pure, for the plan: false where the options or their geometry at hz are refused
inline bool fbank_geometry_quiet(const FbankOpts &opts, uint32_t hz, FbankGeom *g)
{
    return !fbank_opts_fault(opts) && !fbank_geometry_fault(opts, hz, g);
}
// JB_OK, or JB_ERR_INVALID with set_error naming the field (jb_fbank.cpp): the options alone, and with their geometry
// at hz into *g (may be null)
int fbank_check_opts(const FbankOpts *opts, const char *who);
int fbank_geometry(const FbankOpts *opts, uint32_t hz, const char *who, FbankGeom *g);

// The tables of one geometry, built in long double and rounded once
struct FbankTables {
    std::vector<double> win;      // [wl]
    std::vector<double> tw;       // [n_fft / 2 + 1][2]: cos, -sin of 2 pi k / n_fft
    std::vector<double> wts;      // the filters' weights over their supports, filter after filter
    std::vector<uint32_t> first;  // [n_mels] a filter's first bin with a weight above 0
    std::vector<uint32_t> count;  // [n_mels] its bins (0: it covers none)
    std::vector<uint32_t> woff;   // [n_mels] its first weight in wts
    // The same weights by bin, for the kernel.  A bin lies on the rising side of at most one filter (mu_k at or below
    // its centre) and on the falling side of at most one; a filter's support is its `rise` rising bins, then its
    // falling ones
    std::vector<uint32_t> rise;   // [n_mels]
    std::vector<double> wr, wf;   // [n_fft / 2 + 1] the bin's weight in its rising / falling filter (0: none)
};
void fbank_window(uint32_t window, uint32_t wl, double *w);
// dense [n_mels][n_fft / 2 + 1]
void fbank_filterbank(const FbankGeom &g, uint32_t hz, double *W);
// false: a bin came out on the same side of two filters (the by-bin form does not hold it; not expected)
bool fbank_tables(const FbankGeom &g, uint32_t hz, uint32_t window, FbankTables *t);

// The device's view of one geometry's tables
struct FbankClass {
    const double *win, *tw, *wr, *wf;
    const uint32_t *first, *count, *rise;
    uint32_t wl, hop, n_fft, log2m;
    uint32_t n_mels, flags;
    double log_floor, ln_floor;
};

// One unit of a launch.  Launch lists are in unit order; g0 is the prefix sum of the list's workgroups
// (fbank_wg_frames frames each; workgroups never cross units)
struct FbankUtt {
    const double *x; // the chain's final f64 PCM, in 16-bit scale
    uint8_t *y;      // its [T][n_mels] elements, 16-byte aligned
    uint64_t n, T, g0;
    uint32_t cls, pad;
};

// One butterfly of stage s (spans of 2^s) of the in-place decimation-in-time transform of M = 2^log2m points whose
// input was stored in bit-reversed order: butterfly j of M / 2.  tw: the n_fft = 2 M table
// (a, b) <- (a + w b, a - w b), w = c + i sn
JB_FBANK_HD void fbank_bfly(double &ar, double &ai, double &br, double &bi, double c, double sn)
{
    const double tr = c * br - sn * bi, ti = c * bi + sn * br;
    br = ar - tr;
    bi = ai - ti;
    ar = ar + tr;
    ai = ai + ti;
}
JB_FBANK_HD void fbank_butterfly(double *re, double *im, const double *tw, uint32_t log2m, uint32_t s, uint32_t j)
{
    const uint32_t half = 1u << s, pos = j & (half - 1);
    const uint32_t i0 = ((j >> s) << (s + 1)) | pos, i1 = i0 + half;
    const uint32_t k = pos << (log2m - s); // pos n_fft / (2 half): always even
    fbank_bfly(re[i0], im[i0], re[i1], im[i1], tw[2 * k], tw[2 * k + 1]);
}

// |X_k|^2 of the real transform from the packed one, Z in (re, im)[0..M): X_k = Fe + w_k Fo with Fe = (Z_k +
// conj Z_{M-k}) / 2 and Fo = -i (Z_k - conj Z_{M-k}) / 2 (Z_M = Z_0)
JB_FBANK_HD double fbank_power(double ar, double ai, double zr, double zi, double c, double sn)
{
    const double br = zr, bi = -zi;
    const double fer = 0.5 * (ar + br), fei = 0.5 * (ai + bi);
    const double fr = 0.5 * (ai - bi), fi = -0.5 * (ar - br);
    const double xr = fer + (c * fr - sn * fi), xi = fei + (c * fi + sn * fr);
    return xr * xr + xi * xi;
}
// The pair k, M - k (k in 0..M/2) of the M + 1 powers, in place: P_k into re[k], P_{M-k} into re[M - k] (re has a
// slot M); nothing else of the arrays is read
// (c0, s0), (c1, s1): entries k and M - k of the n_fft table
JB_FBANK_HD void fbank_untangle(double *re, double *im, uint32_t M, uint32_t k, double c0, double s0, double c1,
                                double s1)
{
    const uint32_t kk = M - k, kz = kk == M ? 0 : kk;
    const double ar = re[k], ai = im[k], zr = re[kz], zi = im[kz];
    const double p0 = fbank_power(ar, ai, zr, zi, c0, s0);
    const double p1 = fbank_power(zr, zi, ar, ai, c1, s1);
    re[k] = p0;
    if (kk != k)
        re[kk] = p1;
}
JB_FBANK_HD void fbank_untangle(double *re, double *im, const double *tw, uint32_t M, uint32_t k)
{
    fbank_untangle(re, im, M, k, tw[2 * k], tw[2 * k + 1], tw[2 * (M - k)], tw[2 * (M - k) + 1]);
}

} // namespace jb

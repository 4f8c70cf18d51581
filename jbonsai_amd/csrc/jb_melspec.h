#pragma once
// jb_melspec.h -- mel spectrograms in the librosa / Whisper convention (include/jbonsai_amd.h "Mel spectrograms"): the
// geometry of a unit, the tables of one (rate, options) pair, stated once for the kernel (jb_melspec.hip) and for the
// host half (jb_melspec.cpp), and the stage's work list.  The mixed-radix transform of a frame is jb_rfft.h's, the bank
// of filters jb_melbank.h's.  Plain C++17; under hipcc the rules compile for the host and the device alike.
#include "jb_melbank.h"

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
constexpr uint32_t kMelMaxPasses = kRfftMaxPasses;

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
JB_RFFT_HD int64_t mel_sample_at(int64_t idx, uint64_t n, uint32_t pad)
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

// The tables of one geometry, built in long double and rounded once
struct MelTables {
    std::vector<double> win; // [wl]
    RfftPlan fft;            // of n_fft
    MelBank bank;            // over the n_fft / 2 + 1 bins
    double wmax = 0.0;       // the largest weight
};
void mel_window(uint32_t wl, double *w);
// dense [n_mels][n_fft / 2 + 1]
void mel_filterbank(const MelGeom &g, uint32_t hz, uint32_t mel_scale, uint32_t norm, double *W);
// false: a bin came out on the same side of two filters (not expected)
bool mel_tables(const MelGeom &g, uint32_t hz, const MelOpts &o, MelTables *t);

// The logarithm of step 7 and the affine step of step 9, one text for both sides
JB_RFFT_HD double mel_log(double e, uint32_t log, double floor, double y_floor)
{
    if (log == kMelLogNone)
        return e;
    if (!(e > floor))
        return y_floor;
    return log == kMelLogLn ? ::log(e) : log == kMelLog10 ? ::log10(e) : 10.0 * ::log10(e);
}
JB_RFFT_HD double mel_affine(double y, double offset, double scale) { return (y + offset) * scale; }

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

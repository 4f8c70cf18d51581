#pragma once
// jb_fbank.h -- log-mel filterbank features (include/jbonsai_amd.h "Filterbank features"): the geometry of a unit, the
// tables of one (rate, options) pair, stated once for the kernel (jb_fbank.hip), for the host half (jb_fbank.cpp) and
// for the output plan (jb_output.cpp), and the stage's work list.  The transform of a frame is jb_rfft.h's, the bank of
// filters jb_melbank.h's.  Plain C++17.
#include "jb_melbank.h"

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

// Frame conditioning (include/jbonsai_amd.h "Frame conditioning"): jb_frame_opts restated, and the rule's pieces that
// the kernel, the host form and the plan share.
// A plain request is the all-zero frame request: under FrameOpts{} frame_count and frame_start are the plain stage's
// and frame_condition leaves win[i] * v_i, so the host holds one rule and the entries without a request run it with
// FrameOpts{}.  Only the device asks frame_is_identity, to pick the loader without the conditioning's two barriers
struct FrameOpts {
    double preemph;
    uint32_t window, flags;
    uint32_t reserved[4];
};
static_assert(sizeof(FrameOpts) == 32 && offsetof(FrameOpts, window) == 8 && offsetof(FrameOpts, reserved) == 16,
              "jb_frame_opts is 32 bytes");
constexpr uint32_t kFrWindowOpts = 0, kFrPovey = 1, kFrHannSym = 2, kFrRect = 3, kFrBlackman = 4; // JB_FRAME_POVEY, ..
constexpr uint32_t kFrRemoveDc = 1, kFrReflect = 2, kFrEnergy = 4; // JB_FRAME_REMOVE_DC, _REFLECT, _ENERGY

// The zero request is the identity: the device then runs k_fbank<false> (rate_launch, jb_host.h)
inline bool frame_is_identity(const FrameOpts &f)
{
    return f.preemph == 0.0 && f.window == kFrWindowOpts && f.flags == 0;
}
// What is wrong with the request on its own, naming the field; null: nothing
inline const char *frame_opts_fault(const FrameOpts &f)
{
    if (f.window > kFrBlackman)
        return "window is JB_FRAME_WINDOW_OPTS, _POVEY, _HANN_SYM, _RECT or _BLACKMAN";
    if (f.flags & ~(kFrRemoveDc | kFrReflect | kFrEnergy))
        return "flags has an unknown bit";
    if (f.reserved[0] || f.reserved[1] || f.reserved[2] || f.reserved[3])
        return "reserved must be 0";
    if (!(f.preemph >= 0.0 && f.preemph <= 1.0))
        return "preemph is in 0..1";
    return nullptr;
}
// ... and beside the filterbank options it conditions; cepstra: the request is an mfcc one with n_ceps >= 1
inline const char *frame_pair_fault(const FbankOpts &o, const FrameOpts &f, bool cepstra)
{
    if ((f.flags & kFrReflect) && (o.flags & kFbCenter))
        return "flags: JB_FRAME_REFLECT does not go with JB_FBANK_CENTER";
    if ((f.flags & kFrEnergy) && !cepstra)
        return "flags: JB_FRAME_ENERGY needs an mfcc request with n_ceps >= 1";
    return nullptr;
}
// T of n samples and the first sample of frame t (below 0 or behind n: outside the unit), with and without
// JB_FRAME_REFLECT
constexpr uint64_t frame_count(uint64_t n, uint32_t wl, uint32_t hop, bool center, bool reflect)
{
    return reflect ? (n + hop / 2) / hop : center ? (n + hop - 1) / hop : n >= wl ? 1 + (n - wl) / hop : 0;
}
constexpr uint64_t frame_count(uint64_t n, const FbankGeom &g, const FbankOpts &o, const FrameOpts &f)
{
    return frame_count(n, g.wl, g.hop, (o.flags & kFbCenter) != 0, (f.flags & kFrReflect) != 0);
}
JB_RFFT_HD constexpr int64_t frame_start(uint64_t t, uint32_t wl, uint32_t hop, bool center, bool reflect)
{
    return (int64_t)(t * hop) + (reflect ? (int64_t)(hop / 2) - (int64_t)(wl / 2) : center ? -(int64_t)(wl / 2) : 0);
}
// Sample k of a unit of n >= 1 samples under JB_FRAME_REFLECT: mirrored at the edges (the edge sample repeats) until
// it lies inside
JB_RFFT_HD constexpr uint64_t frame_reflect(int64_t k, uint64_t n)
{
    while (k < 0 || (uint64_t)k >= n)
        k = k < 0 ? -k - 1 : 2 * (int64_t)n - 1 - k;
    return (uint64_t)k;
}
// The sum of step 2: f(i), i < wl, into 64 partial sums p_j (i = j mod 64, from 0.0 in ascending i), folded p_j +=
// p_{j + w} for w = 32, 16, .., 1.  A function of wl alone; the kernel's 64 lanes do the same additions
template <class F> inline double frame_sum(uint32_t wl, F f)
{
    double p[64];
    for (uint32_t j = 0; j < 64; j++) {
        p[j] = 0.0;
        for (uint32_t i = j; i < wl; i += 64)
            p[j] = p[j] + f(i);
    }
    for (uint32_t w = 32; w; w >>= 1)
        for (uint32_t j = 0; j < w; j++)
            p[j] = p[j] + p[j + w];
    return p[0];
}
// Steps 2 to 5 on the host, in place: v[0..wl) the samples of step 1 -> the windowed frame; the energy of step 3 into
// *energy (may be null)
inline void frame_condition(const FrameOpts &f, const double *win, uint32_t wl, double *v, double *energy)
{
    if (f.flags & kFrRemoveDc) {
        const double mean = frame_sum(wl, [&](uint32_t i) { return v[i]; }) / (double)wl;
        for (uint32_t i = 0; i < wl; i++)
            v[i] = v[i] - mean;
    }
    if (energy)
        *energy = frame_sum(wl, [&](uint32_t i) { return v[i] * v[i]; });
    const double c = f.preemph;
    double prev = v[0];
    for (uint32_t i = 0; i < wl; i++) {
        const double cur = v[i], cp = c * prev;
        v[i] = win[i] * (c > 0.0 ? cur - cp : cur);
        prev = cur;
    }
}
// The window of a conditioned frame: the request's, or with JB_FRAME_WINDOW_OPTS the filterbank options' (jb_fbank.cpp)
void frame_window(uint32_t fbank_window, uint32_t frame_window, uint32_t wl, double *w);
// JB_OK, or JB_ERR_INVALID with set_error naming the field: the filterbank options, the request and the pair
int frame_check(const FbankOpts *opts, const FrameOpts *fr, bool cepstra, const char *who);
// The rule on the host under the name of the entry `who` (jb_fbank_host's body with FrameOpts{}, jb_fbank_framed_host's
// with its request); o is checked here (null: refused); energy: the frames' energies of step 3 (may be null)
int fbank_framed_host(const double *in, size_t n, uint32_t hz, const FbankOpts *o, const FrameOpts &fr, uint8_t *out,
                      size_t cap, const char *who, std::vector<double> *energy);

// The tables of one geometry, built in long double and rounded once
struct FbankTables {
    std::vector<double> win; // [wl]
    RfftPlan fft;            // of n_fft (passes of 2 alone)
    MelBank bank;            // over the n_fft / 2 + 1 bins
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
    double preemph;         // the frame request (win is its window already); all zero: none
    uint32_t fr_flags, pad; // JB_FRAME_REMOVE_DC | _REFLECT
};

// One unit of a launch.  Launch lists are in unit order; g0 is the prefix sum of the list's workgroups
// (fbank_wg_frames frames each; workgroups never cross units)
struct FbankUtt {
    const double *x; // the chain's final f64 PCM, in 16-bit scale
    uint8_t *y;      // its [T][n_mels] elements, 16-byte aligned
    double *e;       // [T] the frames' energies (step 3 of the frame request); null: none
    uint64_t n, T, g0;
    uint32_t cls, pad;
};

} // namespace jb

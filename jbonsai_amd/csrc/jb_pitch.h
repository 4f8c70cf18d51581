#pragma once
// jb_pitch.h -- the pitch stage (include/jbonsai_amd.h "Pitch features"): the pitch columns of the Kaldi recipes
// (compute-kaldi-pitch-feats | process-kaldi-pitch-feats; Ghahremani et al., ICASSP 2014) of a unit, on the frame grid
// of the filterbank stage.  The rule, stated once for the kernels (jb_pitch.hip) and for the host rule (jb_pitch.cpp):
// the decimator to 4 kHz and its sums, the frames, the lag grid, the NCCF of a frame, the Viterbi step and the columns
// of the post-processing; the request check; the stage's device items.  The frame grid is jb_fbank.h's frame_count /
// frame_start / fbank_round_us, called and not restated; a frame's sums are frame_sum's (the kernels do frame_sum's
// additions on a wave, as the activity stage does).  f64 throughout, every table formed in long double on the host
// and rounded once, every sum in a fixed order, products rounded before they are added (no fma).
// Plain C++17; under hipcc the rule compiles for the host and the device alike.
#include <math.h>

#include "jb_fbank.h"

namespace jb {

// jb_pitch_opts of the public header, restated (this header stands without it; jb_pitch.cpp asserts the two agree)
struct PitchOpts {
    uint32_t win_us, hop_us; // multiples of 250 us
    double min_f0, max_f0, delta_pitch, penalty_factor, soft_min_f0, nccf_ballast;
    double pov_scale, pitch_scale, delta_scale;
    uint32_t norm_left, norm_right; // frames of the normalisation window in front of a frame and behind it
    uint32_t grid, flags;
    uint32_t reserved[4];
};
static_assert(sizeof(PitchOpts) == 112 && offsetof(PitchOpts, min_f0) == 8 && offsetof(PitchOpts, pov_scale) == 56 &&
                  offsetof(PitchOpts, norm_left) == 80 && offsetof(PitchOpts, grid) == 88 &&
                  offsetof(PitchOpts, reserved) == 96,
              "jb_pitch_opts is 112 bytes");

constexpr uint32_t kPitchSnip = 0, kPitchKaldi = 1;                // JB_PITCH_SNIP, _KALDI
constexpr uint32_t kPitchF64 = 1, kPitchRaw = 2, kPitchRawLog = 4; // JB_PITCH_F64, _RAW, _RAW_LOG
constexpr uint32_t kPitchRate = 4000, kPitchCut = 1000;            // r and the decimator's cutoff c, in Hz
constexpr uint32_t kPitchUp = 5;                                   // u: the width of the lag interpolation
constexpr uint32_t kPitchTaps = 11;                                // at most this many integer lags under a grid lag
constexpr uint32_t kPitchMaxStates = 1024, kPitchMaxLag = 255, kPitchMinWin = 8, kPitchMaxWin = 512;
constexpr uint32_t kPitchMaxNorm = 4096;  // frames on either side of the normalisation window
constexpr uint32_t kPitchMaxDown = 4096;  // JB_PITCH_MAX_DOWN: weights of a rate's phase table (32 KiB of LDS)
// JB_PITCH_MAX_SCRATCH: the bytes of the tracker's stored choices over a call, 2 S per frame (pitch_choice_bytes)
constexpr uint64_t kPitchMaxScratch = 1ull << 32;
constexpr uint64_t pitch_choice_bytes(uint32_t S) { return 2ull * S; }

// The launch shape.  k_pitch_down: a workgroup per tile of the sums, kPitchTile output samples, each lane the four
// samples of its partial.  The tracker: one workgroup per unit.  k_pitch_post: a wave per frame.  k_pitch_cols: a lane
// per frame
constexpr uint32_t kPitchLanes = 256, kPitchTile = 1024;
constexpr uint32_t kPitchTrackLanes = 512;
constexpr uint32_t kPitchPostFrames = kPitchLanes / 64;
constexpr uint64_t pitch_tiles(uint64_t n4) { return (n4 + kPitchTile - 1) / kPitchTile; }
constexpr uint64_t pitch_post_wgs(uint64_t T) { return (T + kPitchPostFrames - 1) / kPitchPostFrames; }
constexpr uint64_t pitch_cols_wgs(uint64_t T) { return (T + kPitchLanes - 1) / kPitchLanes; }

constexpr uint32_t pitch_width(uint32_t flags) { return (flags & kPitchRaw) ? 2 : (flags & kPitchRawLog) ? 4 : 3; }
constexpr uint32_t pitch_elem(uint32_t flags) { return (flags & kPitchF64) ? 8 : 4; }

// What is wrong with the options whatever the rate, naming the field; null: nothing
inline const char *pitch_opts_fault(const PitchOpts &o)
{
    if (o.grid > kPitchKaldi)
        return "grid is JB_PITCH_SNIP or JB_PITCH_KALDI";
    if (o.flags & ~(kPitchF64 | kPitchRaw | kPitchRawLog))
        return "flags has an unknown bit";
    if ((o.flags & kPitchRaw) && (o.flags & kPitchRawLog))
        return "flags: JB_PITCH_RAW does not go with JB_PITCH_RAW_LOG";
    if (o.reserved[0] || o.reserved[1] || o.reserved[2] || o.reserved[3])
        return "reserved must be 0";
    if (o.win_us % 250 || o.win_us / 250 < kPitchMinWin || o.win_us / 250 > kPitchMaxWin)
        return "win_us is a multiple of 250 that gives 8..512 samples at 4 kHz";
    if (o.hop_us % 250 || o.hop_us == 0)
        return "hop_us is a multiple of 250, at least 250";
    if (!(o.min_f0 > 0.0) || !std::isfinite(o.min_f0))
        return "min_f0 is above 0";
    if (!(o.max_f0 > o.min_f0) || !(o.max_f0 <= 0.5 * kPitchRate))
        return "max_f0 is above min_f0 and at most 2000";
    if (!(o.delta_pitch >= 1e-4 && o.delta_pitch <= 1.0))
        return "delta_pitch is in [0.0001, 1]";
    if (!(o.penalty_factor >= 0.0) || !std::isfinite(o.penalty_factor))
        return "penalty_factor is at least 0";
    if (!(o.soft_min_f0 >= 0.0) || !std::isfinite(o.soft_min_f0))
        return "soft_min_f0 is at least 0";
    if (!(o.nccf_ballast >= 0.0) || !std::isfinite(o.nccf_ballast))
        return "nccf_ballast is at least 0";
    if (!std::isfinite(o.pov_scale))
        return "pov_scale is finite";
    if (!std::isfinite(o.pitch_scale))
        return "pitch_scale is finite";
    if (!std::isfinite(o.delta_scale))
        return "delta_scale is finite";
    if (o.norm_left > kPitchMaxNorm)
        return "norm_left is in 0..4096 frames";
    if (o.norm_right > kPitchMaxNorm)
        return "norm_right is in 0..4096 frames";
    return nullptr;
}

// The windowed sinc of steps 1 and 4: f(t) = 2c sinc(2ct) (1 + cos(2 pi c t / w)) / 2 inside |t| < w / (2c), else 0
inline long double pitch_filter(long double c, long double w, long double t)
{
    if (!(fabsl(t) < w / (2.0L * c)))
        return 0.0L;
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double x = 2.0L * c * t;
    const long double s = x == 0.0L ? 1.0L : sinl(pi * x) / (pi * x);
    return 2.0L * c * s * 0.5L * (1.0L + cosl(2.0L * pi * c * t / w));
}

// Step 3 and the tables of steps 4 to 6, of the options alone (the analysis rate is fixed, so one set serves every
// unit of a call).  The recipe of the lags: lag_0 = 1 / max_f0 and lag_{i+1} = lag_i (1 + delta), each one long double
// operation, while lag_i <= 1 / min_f0 in long double; `lag` is each one rounded to double
struct PitchGrid {
    uint32_t S = 0, a = 0, b = 0, wl4 = 0, sh4 = 0;
    std::vector<double> lag, inv_lag, log_pitch, soft; // [S]: lag_i, 1 / lag_i, ln(1 / lag_i), soft_min_f0 lag_i
    std::vector<double> G;                             // [S][kPitchTaps]: g_i[L0_i + k], +0.0 behind the count
    std::vector<uint32_t> tap;                         // [S]: (L0_i - a) | count << 16
    double kappa = 0.0;                                // penalty_factor ln(1 + delta)^2
};
// What is out of its limits, naming the field; null: nothing, and the grid is in *out
inline const char *pitch_grid_fault(const PitchOpts &o, PitchGrid *out)
{
    PitchGrid g;
    const long double r = kPitchRate, top = 1.0L / (long double)o.min_f0, step = 1.0L + (long double)o.delta_pitch;
    std::vector<long double> lags;
    for (long double l = 1.0L / (long double)o.max_f0; l <= top; l = l * step) {
        if (lags.size() == kPitchMaxStates)
            return "min_f0, max_f0 and delta_pitch give more than 1024 lags";
        lags.push_back(l);
    }
    const long double lo = floorl(r / (long double)o.max_f0 - 0.5L * kPitchUp);
    const long double hi = ceill(r / (long double)o.min_f0 + 0.5L * kPitchUp);
    if (hi > (long double)kPitchMaxLag)
        return "min_f0 gives an integer lag above 255";
    g.S = (uint32_t)lags.size();
    g.a = lo < 0.0L ? 0u : (uint32_t)lo;
    g.b = (uint32_t)hi;
    g.wl4 = o.win_us / 250;
    g.sh4 = o.hop_us / 250;
    g.G.assign((size_t)g.S * kPitchTaps, 0.0);
    const long double ln_step = logl(step);
    g.kappa = (double)((long double)o.penalty_factor * ln_step * ln_step);
    for (uint32_t i = 0; i < g.S; i++) {
        const long double l = lags[i], x = l * r;
        g.lag.push_back((double)l);
        g.inv_lag.push_back((double)(1.0L / l));
        g.log_pitch.push_back((double)logl(1.0L / l));
        g.soft.push_back((double)((long double)o.soft_min_f0 * l));
        long double first = floorl(x - (long double)kPitchUp) + 1.0L, last = ceill(x + (long double)kPitchUp) - 1.0L;
        first = first < (long double)g.a ? (long double)g.a : first;
        last = last > (long double)g.b ? (long double)g.b : last;
        const uint32_t L0 = (uint32_t)first, cnt = last >= first ? (uint32_t)(last - first) + 1 : 0;
        if (cnt > kPitchTaps)
            return "delta_pitch gives a lag with more than 11 taps (not expected)";
        for (uint32_t k = 0; k < cnt; k++)
            g.G[(size_t)i * kPitchTaps + k] =
                (double)(pitch_filter(0.5L * r, (long double)kPitchUp, (long double)(L0 + k) / r - l) / r);
        g.tap.push_back((L0 - g.a) | (cnt << 16));
    }
    *out = std::move(g);
    return nullptr;
}

// Step 1's phase table at one rate.  With g = gcd(hz, r), P = r / g phases and hzp = hz / g: output m sits at input
// position m hzp / P = c_m + ph / P, and weight j of phase ph belongs to the input sample c_m + j - D,
// W[ph][j] = f(((j - D) - ph / P) / hz) / hz: 2D + 1 weights, D = ceil(hz / 2c), +0.0 outside the filter's support
struct PitchDown {
    uint32_t P = 0, D = 0, hzp = 0;
    std::vector<double> W; // [P][2 D + 1]
};
// null, or what the rate is refused for (*unsupported: past a cap)
inline const char *pitch_down_fault(uint32_t hz, PitchDown *out, bool *unsupported)
{
    *unsupported = false;
    if (hz < kPitchRate)
        return "hz is at least 4000 (the analysis rate)";
    uint32_t g = hz, h = kPitchRate;
    while (h) {
        const uint32_t t = g % h;
        g = h;
        h = t;
    }
    PitchDown d;
    d.P = kPitchRate / g;
    d.hzp = hz / g;
    d.D = (hz + 2 * kPitchCut - 1) / (2 * kPitchCut);
    const uint32_t taps = 2 * d.D + 1;
    *unsupported = true;
    if ((uint64_t)d.P * taps > kPitchMaxDown)
        return "hz gives a phase table above JB_PITCH_MAX_DOWN weights";
    *unsupported = false;
    d.W.resize((size_t)d.P * taps);
    for (uint32_t ph = 0; ph < d.P; ph++)
        for (uint32_t j = 0; j < taps; j++) {
            const long double t = (((long double)j - (long double)d.D) - (long double)ph / (long double)d.P) / (long double)hz;
            d.W[(size_t)ph * taps + j] = (double)(pitch_filter((long double)kPitchCut, 1.0L, t) / (long double)hz);
        }
    *out = std::move(d);
    return nullptr;
}
constexpr uint64_t pitch_n4(uint64_t n, uint32_t hz) { return (n * kPitchRate + hz - 1) / hz; }
constexpr uint64_t pitch_frames(uint32_t grid, uint64_t n, uint32_t wl, uint32_t hop)
{
    return frame_count(n, wl, hop, false, grid == kPitchKaldi);
}

// Sample m of the 4 kHz signal of a unit of n samples (at(k): sample k): from +0.0, the products of the taps whose
// sample lies in [0, n), in ascending k
template <class X>
JB_RFFT_HD double pitch_down_sample(uint64_t m, uint64_t n, uint32_t hzp, uint32_t P, uint32_t D, const double *W, X at)
{
    const uint64_t pos = m * hzp, c = pos / P;
    const double *w = W + (size_t)(pos % P) * (2 * D + 1);
    double acc = 0.0;
    for (uint32_t j = 0; j <= 2 * D; j++) {
        const int64_t k = (int64_t)c + (int64_t)j - (int64_t)D;
        if (k < 0 || (uint64_t)k >= n)
            continue;
        const double t = at((uint64_t)k) * w[j];
        acc = acc + t;
    }
    return acc;
}
// Partial l of tile i of the sums of y[0..N): the in-range indices 1024 i + l + 256 j, j = 0..3 ascending; the first
// term starts the partial, every later one is rounded and then added; none in range: +0.0.  The noise stage's order
// (tiles of 1,024, 256 partials, the tree 128, 64, .., 1, the tiles added in ascending order); its noise_partial is not
// called, because it fuses the square onto the sum
template <class Z> JB_RFFT_HD void pitch_partial(uint64_t N, uint64_t i, uint32_t l, Z at, double *s1, double *s2)
{
    double p1 = 0.0, p2 = 0.0;
    bool first = true;
    for (uint32_t j = 0; j < kPitchTile / kPitchLanes; j++) {
        const uint64_t m = i * kPitchTile + l + (uint64_t)kPitchLanes * j;
        if (m >= N)
            break;
        const double z = at(m), zz = z * z;
        p1 = first ? z : p1 + z;
        p2 = first ? zz : p2 + zz;
        first = false;
    }
    *s1 = p1;
    *s2 = p2;
}
// The ballast of a unit from its sums: sigma^2 = S2 / n4 - (S1 / n4)^2, B = ballast (sigma^2 wl4)^2
JB_RFFT_HD double pitch_ballast(double S1, double S2, uint64_t n4, uint32_t wl4, double ballast)
{
    if (n4 == 0)
        return 0.0;
    const double dn = (double)n4, m = S1 / dn, mm = m * m;
    const double s = (S2 / dn - mm) * (double)wl4, ss = s * s;
    return ballast * ss;
}
// The first 4 kHz sample of frame t (below 0 or behind n4: outside the unit, read as 0)
JB_RFFT_HD int64_t pitch_start(uint32_t grid, uint64_t t, uint32_t wl4, uint32_t sh4)
{
    return frame_start(t, wl4, sh4, false, grid == kPitchKaldi);
}
// q_L and p_L from the three sums; +0.0 where the denominator is 0
JB_RFFT_HD double pitch_nccf(double inner, double e0, double eL, double B)
{
    const double ee = e0 * eL, den = ee + B;
    return den == 0.0 ? 0.0 : inner / sqrt(den);
}
// The local cost of a grid value Q at a lag with soft = soft_min_f0 lag
JB_RFFT_HD double pitch_local(double Q, double soft)
{
    const double sq = soft * Q;
    return (1.0 - Q) + sq;
}
// The cost of coming to state i from state j with the forward cost F
JB_RFFT_HD double pitch_cand(double F, double kappa, uint32_t i, uint32_t j)
{
    const uint32_t d = i > j ? i - j : j - i;
    const double pen = kappa * (double)(d * d);
    return F + pen;
}
// Step 6, of p alone: the POV feature without its scale, and the weight pi of the normalisation
JB_RFFT_HD double pitch_pov_feature(double p)
{
    const double c = p < -1.0 ? -1.0 : p > 1.0 ? 1.0 : p;
    return pow(1.0001 - c, 0.15) - 1.0;
}
JB_RFFT_HD double pitch_pov_weight(double p)
{
    double a = fabs(p);
    a = a > 1.0 ? 1.0 : a;
    double rho = -5.2;
    const double t1 = 5.4 * exp(7.5 * (a - 1.0)), t2 = 4.8 * a, t3 = 2.0 * exp(-10.0 * a), t4 = 4.2 * exp(20.0 * (a - 1.0));
    rho = rho + t1;
    rho = rho + t2;
    rho = rho - t3;
    rho = rho + t4;
    return 1.0 / (1.0 + exp(-rho));
}
// The columns of frame t of T from the frames' chosen lags, p and pi: out[0..width)
template <class I> JB_RFFT_HD void pitch_columns(uint64_t t, uint64_t T, const I *idx, const double *pv, const double *pw,
                                                 const double *log_pitch, double pov_scale, double pitch_scale,
                                                 double delta_scale, uint32_t left, uint32_t right, uint32_t width,
                                                 double *out)
{
    const uint64_t j0 = t > left ? t - left : 0, j1 = t + right < T - 1 ? t + right : T - 1;
    double num = 0.0, den = 0.0;
    for (uint64_t j = j0; j <= j1; j++) {
        const double wl = pw[j] * log_pitch[idx[j]];
        num = num + wl;
        den = den + pw[j];
    }
    const double l = log_pitch[idx[t]];
    double d = 0.0;
    for (int k = -2; k <= 2; k++) {
        const int64_t u = (int64_t)t + k;
        const uint64_t c = u < 0 ? 0 : (uint64_t)u > T - 1 ? T - 1 : (uint64_t)u;
        const double term = (double)k * log_pitch[idx[c]];
        d = d + term;
    }
    out[0] = pov_scale * pitch_pov_feature(pv[t]);
    out[1] = pitch_scale * (l - num / den);
    out[2] = delta_scale * (d / 10.0);
    if (width > 3)
        out[3] = l;
}

// The tables of a call on the device and the request's share of every launch
struct PitchClass {
    const double *G, *soft, *inv_lag, *log_pitch;
    const uint32_t *tap;
    double kappa, ballast, pov_scale, pitch_scale, delta_scale;
    uint32_t S, a, b, wl4, sh4, grid, flags, left, right, pad;
};
// One unit of a launch.  Launch lists are in unit order; t0, g0 and c0 are the prefix sums of the list's tiles
// (k_pitch_down), of k_pitch_post's workgroups and of k_pitch_cols' (workgroups never cross units)
struct PitchUtt {
    const double *x;  // the unit's f64 PCM
    const double *W;  // its rate's phase table
    double *y4;       // [n4] the 4 kHz signal
    double *tile;     // [tiles][2] the tiles' sums
    uint16_t *choice; // [T][S] the tracker's choices
    uint32_t *idx;    // [T] the chosen lag of every frame
    double *pv, *pw;  // [T] p at the chosen lag, and its weight pi
    uint8_t *out;     // [T][width] elements, 16-byte aligned
    uint64_t n, n4, T, t0, g0, c0;
    uint32_t hzp, P, D, pad;
};

// The three prefix sums of a launch list, and their totals
inline void pitch_number(std::vector<PitchUtt> *list, uint64_t *tiles, uint64_t *post, uint64_t *cols)
{
    *tiles = *post = *cols = 0;
    for (PitchUtt &u : *list) {
        u.t0 = *tiles;
        u.g0 = *post;
        u.c0 = *cols;
        *tiles += pitch_tiles(u.n4);
        *post += pitch_post_wgs(u.T);
        *cols += pitch_cols_wgs(u.T);
    }
}

} // namespace jb

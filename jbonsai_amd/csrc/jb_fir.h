#pragma once
// jb_fir.h -- the convolution stage (include/jbonsai_amd.h "Convolution"): the output PCM convolved with an impulse
// response of up to 131,072 taps at the output rate, in the filter stage's place and in front of its sections.  The
// rule of one sample, stated once for the direct kernel (jb_fir.hip) and for the host rule (jb_fir.cpp); the geometry
// of a tap count (mode, block, partitions: from K alone); the stage's device tables and work list.
// Plain C++17; under hipcc the rule compiles for the host and the device alike.
// Partitioned mode takes the packed real transform of jb_rfft.h.
#include "jb_rfft.h"

#include <math.h>

namespace jb {

constexpr uint32_t kFirMaxTaps = 131072, kFirDirectMax = 256; // JB_FIR_MAX_TAPS, JB_FIR_DIRECT_MAX
constexpr uint32_t kFirDirect = 0, kFirPartitioned = 1;       // JB_FIR_DIRECT, JB_FIR_PARTITIONED
constexpr uint32_t kFirLanes = 256;                           // threads of a workgroup, every kernel
constexpr uint32_t kFirTile = 2048;                           // direct mode: outputs of a workgroup
constexpr uint32_t kFirSmallFft = 2048, kFirLargeFft = 4096;  // partitioned mode: n_fft by K alone
constexpr uint32_t kFirSmallMax = 4096;                       // the largest K that takes the small transform
constexpr uint32_t kFirPoints = kFirLargeFft / 2;             // complex points of the largest packed transform

// The geometry of K taps.  Direct: one workgroup per kFirTile outputs, one partition.  Partitioned: blocks of
// Bk = n_fft / 2 outputs, n_fft 2048 up to K = 4096 (at most four partitions) and 4096 above (at most 64)
struct FirGeom {
    uint32_t mode, block, partitions, n_fft;
};
constexpr FirGeom fir_geometry(uint32_t K)
{
    return K <= kFirDirectMax ? FirGeom{kFirDirect, kFirTile, 1, 0}
           : K <= kFirSmallMax
               ? FirGeom{kFirPartitioned, kFirSmallFft / 2, (K + kFirSmallFft / 2 - 1) / (kFirSmallFft / 2), kFirSmallFft}
               : FirGeom{kFirPartitioned, kFirLargeFft / 2, (K + kFirLargeFft / 2 - 1) / (kFirLargeFft / 2), kFirLargeFft};
}
constexpr uint64_t fir_blocks(uint64_t n, uint32_t block) { return (n + block - 1) / block; }
// Partitioned mode: the delay's d samples in front of an utterance's first block are `lead` blocks of their own
// (block -lead .. -1: their windows hold samples that block 0's sum needs), so an utterance of nb > 0 blocks has
// nb + lead spectra
constexpr uint32_t fir_lead(uint32_t delay, uint32_t block) { return (delay + block - 1) / block; }
constexpr uint64_t fir_frames(uint64_t n, uint32_t delay, uint32_t block)
{
    return n ? fir_blocks(n, block) + fir_lead(delay, block) : 0;
}

// jb_fir of the public header, restated (this header stands without it; jb_fir.cpp asserts the two agree)
struct FirSpec {
    const double *taps;
    uint32_t n_taps, hz, delay, reserved;
};

// What is wrong with a request at the output rate `hz`, naming the field; null: nothing (taps == NULL with
// n_taps == 0 is no response and is accepted)
inline const char *fir_fault(const FirSpec &f, uint32_t hz)
{
    if (f.reserved)
        return "reserved must be 0";
    if (!f.taps)
        return f.n_taps ? "taps is NULL with n_taps above 0" : nullptr;
    if (f.n_taps == 0)
        return "n_taps is 0 with taps given";
    if (f.n_taps > kFirMaxTaps)
        return "n_taps is above JB_FIR_MAX_TAPS (131072)";
    for (uint32_t k = 0; k < f.n_taps; k++)
        if (!isfinite(f.taps[k]))
            return "taps holds a value that is not finite";
    if (f.delay >= f.n_taps)
        return "delay must be below n_taps";
    if (f.hz != hz)
        return "hz differs from the utterance's output rate (a response is never resampled)";
    return nullptr;
}

// y[n] of x[0..N) under h[0..K) and the delay d < K: the terms h[k] x[n + d - k] whose index lies in [0, N), in
// ascending k; the first starts the sum, every later one is fused onto it; none: +0.0.  at(i): sample i of x
template <class X> JB_RFFT_HD double fir_sample(const double *h, uint32_t K, uint32_t d, uint64_t N, uint64_t n, X at)
{
    const uint64_t top = n + d; // the index of the term k = 0
    const uint64_t klo = top >= N ? top - (N - 1) : 0, khi = top < K - 1 ? top : K - 1;
    if (N == 0 || klo > khi)
        return 0.0;
    double acc = h[klo] * at(top - klo);
    for (uint64_t k = klo + 1; k <= khi; k++)
        acc = __builtin_fma(h[k], at(top - k), acc);
    return acc;
}

// The output plan's filter flag of every utterance (jb_output.h: OutPlanIn::filter): a section or a response.
// sections: [B] or empty (no filter request); fir_of: [B] an utterance's response, -1: none, or empty (no request)
inline std::vector<uint8_t> fir_stage_flags(const std::vector<uint8_t> &sections, const std::vector<int32_t> &fir_of)
{
    std::vector<uint8_t> flags = sections;
    if (fir_of.empty())
        return flags;
    flags.resize(fir_of.size(), 0);
    for (size_t u = 0; u < fir_of.size(); u++)
        flags[u] = flags[u] || fir_of[u] >= 0;
    return flags;
}

// One distinct response (taps, delay, rate) on the host, with its geometry and, in partitioned mode, its tables
// (fir_spectra)
struct FirResponse {
    std::vector<double> taps;
    uint32_t hz = 0, delay = 0;
    FirGeom g{};
    std::vector<double> H, tw;
};

// The device's view of one response.  Direct: h alone.  Partitioned: H[p][k] = (re, im) of bin k <= M of partition
// p's transform over n_fft points, scaled by 1 / M (M = n_fft / 2: the inverse transform's factor, a power of two),
// and tw[k] = (cos, -sin)(2 pi k / n_fft), k <= M
struct FirClass {
    const double *h, *H, *tw;
    uint32_t K, delay, mode, block, partitions, n_fft, log2m, lead; // lead: fir_lead(delay, block)
};

// One utterance of a launch.  Launch lists are in utterance order; g0 is the prefix sum of the list's workgroups
// (direct: tiles of kFirTile outputs; partitioned: blocks) and f0 that of its spectra (partitioned: fir_frames), s0 the
// utterance's first bin in the spectrum scratch (fixed per batch; block + 1 bins of 16 bytes per spectrum)
struct FirUtt {
    const double *x; // f64 PCM, 16-bit scale
    void *y;         // f64, or 16-bit where i16 is set
    uint64_t n, g0, f0, s0;
    uint32_t cls, i16;
};

} // namespace jb

#pragma once
// jb_noise.h -- the noise stage (include/jbonsai_amd.h "Noise"): background noise added to the output PCM at a target
// signal-to-noise ratio, behind the convolution and in front of the filter's sections.  The rule, stated once for the
// kernels (jb_noise.hip) and for the host rule (jb_noise.cpp): the noise sequence (a looped bed, or the counter-based
// white generator), the power sum in its fixed order, the active test, the gain and the per-utterance variation; the
// request check; the stage's device items.
// Plain C++17; under hipcc the rule compiles for the host and the device alike.
#include "jb_format.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#ifdef __HIPCC__
#define JB_NOISE_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_NOISE_HD inline
#endif

namespace jb {

constexpr uint32_t kNoiseBed = 0, kNoiseWhite = 1;        // JB_NOISE_BED, JB_NOISE_WHITE
constexpr uint32_t kNoiseRefWhole = 0, kNoiseRefActive = 1; // JB_NOISE_REF_WHOLE, JB_NOISE_REF_ACTIVE
constexpr uint32_t kNoiseVary = 1;                        // JB_NOISE_VARY
constexpr uint32_t kNoiseMaxBed = 1u << 24;               // JB_NOISE_MAX_BED
constexpr uint64_t kNoiseMaxBeds = 1ull << 26;            // samples of a batch's distinct beds
constexpr uint32_t kNoiseLanes = 256;                     // partials of a tile; threads of k_noise_sums / _apply
constexpr uint32_t kNoiseTile = 1024;                     // samples of a tile of the power sum
constexpr uint32_t kNoiseApplyTile = 4096;                // samples of a workgroup of the apply pass
constexpr uint32_t kNoiseWave = 64;                       // k_noise_gain: one wave per utterance

constexpr uint64_t noise_tiles(uint64_t n) { return (n + kNoiseTile - 1) / kNoiseTile; }
constexpr uint64_t noise_apply_tiles(uint64_t n) { return (n + kNoiseApplyTile - 1) / kNoiseApplyTile; }

// jb_noise of the public header, restated (this header stands without it; jb_noise.cpp asserts the two agree)
struct NoiseSpec {
    const double *bed;
    uint64_t seed;
    double snr_db, gate_db;
    uint32_t kind, bed_len, hz, offset, reference, flags, reserved;
};

// "no request for this utterance"
inline bool noise_none(const NoiseSpec &s) { return s.kind == kNoiseBed && !s.bed && s.bed_len == 0; }

// What is wrong with a request at the output rate `hz`, naming the field; null: nothing
inline const char *noise_fault(const NoiseSpec &s, uint32_t hz)
{
    if (s.reserved)
        return "reserved must be 0";
    if (s.kind != kNoiseBed && s.kind != kNoiseWhite)
        return "kind is neither JB_NOISE_BED nor JB_NOISE_WHITE";
    if (s.flags & ~kNoiseVary)
        return "flags holds an unknown flag";
    if (s.reference != kNoiseRefWhole && s.reference != kNoiseRefActive)
        return "reference is neither JB_NOISE_REF_WHOLE nor JB_NOISE_REF_ACTIVE";
    if (noise_none(s))
        return nullptr;
    if (s.kind == kNoiseBed) {
        if (!s.bed)
            return "bed is NULL with bed_len above 0";
        if (s.bed_len == 0)
            return "bed_len is 0 with a bed given";
        if (s.bed_len > kNoiseMaxBed)
            return "bed_len is above JB_NOISE_MAX_BED (16777216)";
        for (uint32_t k = 0; k < s.bed_len; k++)
            if (!isfinite(s.bed[k]))
                return "bed holds a value that is not finite";
        if (s.offset >= s.bed_len)
            return "offset must be below bed_len";
        if (s.hz != hz)
            return "hz differs from the utterance's output rate (a bed is never resampled)";
    } else if (s.bed || s.bed_len) {
        return "bed is given with JB_NOISE_WHITE";
    }
    if (!(s.snr_db >= -40.0 && s.snr_db <= 100.0) && !(s.snr_db > 0 && isinf(s.snr_db)))
        return "snr_db is not in [-40, 100] or +INFINITY";
    if (s.reference == kNoiseRefActive ? !(s.gate_db >= 1.0 && s.gate_db <= 60.0) : !(s.gate_db == 0.0))
        return s.reference == kNoiseRefActive ? "gate_db is not in [1, 60]" : "gate_db must be 0 with JB_NOISE_REF_WHOLE";
    return nullptr;
}

// Sample n of the white sequence; mseed = fmt_mix(seed).  The four 16-bit fields of one splitmix64 word, summed:
// an exact integer in +-131070
JB_NOISE_HD double noise_white(uint64_t mseed, uint64_t n)
{
    const uint64_t r = fmt_mix(mseed ^ n);
    const int32_t s = (int32_t)((r & 0xffffu) + ((r >> 16) & 0xffffu) + ((r >> 32) & 0xffffu) + (r >> 48));
    return (double)(s - 131070);
}

// JB_NOISE_VARY: what the utterance of index k uses of (seed, bed_len)
JB_NOISE_HD void noise_vary(uint64_t seed, uint64_t k, uint32_t bed_len, uint64_t *seed_k, uint32_t *offset_k)
{
    const uint64_t z = fmt_mix(fmt_mix(seed) ^ k);
    *seed_k = z;
    *offset_k = bed_len ? (uint32_t)(fmt_mix(z) % bed_len) : 0u;
}

// Partial l of tile i of the power sum of z[0..N) (at(n): sample n): the in-range indices 1024 i + l + 256 j,
// j = 0..3 ascending; the first term is the product, every later one is fused on; none in range: +0.0
template <class Z> JB_NOISE_HD double noise_partial(uint64_t N, uint64_t i, uint32_t l, Z at)
{
    double p = 0.0;
    bool first = true;
    for (uint32_t j = 0; j < kNoiseTile / kNoiseLanes; j++) {
        const uint64_t n = i * kNoiseTile + l + (uint64_t)kNoiseLanes * j;
        if (n >= N)
            break;
        const double z = at(n);
        p = first ? z * z : __builtin_fma(z, z, p);
        first = false;
    }
    return p;
}

// Is a tile of sum t and c samples active?  Sq = S(x) q, dn = (double)N
JB_NOISE_HD bool noise_active(double t, double dn, double Sq, uint32_t c) { return t * dn >= Sq * (double)c; }

// The gain of speech sum A over C samples and noise sum Bs over N samples at the power ratio r = 10^(snr_db / 10)
// (r == +inf: snr_db == +INFINITY)
JB_NOISE_HD double noise_gain(double A, uint64_t C, double Bs, uint64_t N, double r)
{
    if (A == 0.0 || Bs == 0.0 || C == 0 || r == (double)INFINITY)
        return 0.0;
    return sqrt(((A * (double)N) / (Bs * (double)C)) / r);
}

// 10^(db / 10) in long double, rounded once (the host's; the device is handed the double)
inline double noise_ratio(double db) { return isinf(db) ? db : (double)powl(10.0L, (long double)db / 10.0L); }

// The output plan's filter flag of every utterance beside fir_stage_flags: `flags` ([B] or empty) or a noise request.
// noise_of: [B] 1 = the utterance has a request (snr_db = +INFINITY included), or empty (no request)
inline std::vector<uint8_t> noise_stage_flags(const std::vector<uint8_t> &flags_in, const std::vector<uint8_t> &noise_of)
{
    std::vector<uint8_t> flags = flags_in;
    if (noise_of.empty())
        return flags;
    flags.resize(noise_of.size(), 0);
    for (size_t u = 0; u < noise_of.size(); u++)
        flags[u] = flags[u] || noise_of[u];
    return flags;
}

// One distinct bed on the device: its samples, its length and 256 mod len (the step between a lane's terms)
struct NoiseBed {
    const double *w;
    uint32_t len, hz;
};

// One utterance of a launch.  Launch lists are in utterance order; t0 and a0 are the prefix sums of the list's sum
// tiles and apply tiles, s0 the utterance's first tile in the sum scratch (fixed per batch: two doubles per tile),
// rep its record
struct NoiseUtt {
    const double *x; // f64 PCM, 16-bit scale
    void *y;         // f64 (may be x itself), or 16-bit where i16 is set
    const double *bed; // null: white
    uint64_t n, t0, a0, s0, mseed; // mseed: fmt_mix(seed)
    double r, q;     // 10^(snr_db / 10) (+inf: no mixing), 10^(-gate_db / 10)
    uint32_t lb, offset, active, i16, rep, pad;
};

// What k_noise_gain leaves of one utterance
struct NoiseRecord {
    double A, Bs, gain;
    uint64_t C;
};

} // namespace jb

#pragma once
// jb_loudness_rules.h -- the loudness rules behind the measure passes (include/jbonsai_amd.h "loudness", steps 2-4 and
// 6-8): a block's and a window's mean square, the two gates, the fixed order of a member's partial sums, the gain, the
// nearest-rank rule of the loudness range and one pass of its radix selection, stated once for the kernels
// (jb_loudness.hip: k_ln_gate, k_ln_gate_group, k_ln_windows, k_ln_range) and for the host statement
// (jb_loudness_gate_host, jb_loudness_host.cpp).
// Plain C++17 and header-only; under hipcc the rules compile for the host and the device alike.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
// (spelt without the HIP runtime header, as jb_adpcm.h)
#define JB_LN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_LN_HD inline
#endif

namespace jb {

constexpr uint32_t kLnLanes = 256;      // threads of every loudness workgroup: the width of a member's partial sums
constexpr uint32_t kLnBlockHops = 4;    // a gating block: 400 ms
constexpr uint32_t kLnWindowHops = 30;  // a short-term window: 3 s
constexpr double kLnAbsGate = -70.0;    // LUFS: the absolute gate of the integrated loudness and of the range
constexpr double kLnRelGate = -10.0;    // LU under the loudness of the absolutely gated mean (integrated)
constexpr double kLnRangeGate = -20.0;  // the same of the loudness range (Tech 3342)
constexpr double kLnRangeLo = 0.10, kLnRangeHi = 0.95;

JB_LN_HD uint64_t ln_blocks(uint64_t nh) { return nh >= kLnBlockHops ? nh - (kLnBlockHops - 1) : 0; }
JB_LN_HD uint64_t ln_windows(uint64_t nh) { return nh >= kLnWindowHops ? nh - (kLnWindowHops - 1) : 0; }

// loudness of a mean square (LUFS)
JB_LN_HD double ln_loudness(double ms) { return -0.691 + 10.0 * log10(ms); }

// mean square of block i: hops i..i+3 of z (any callable hop -> z_j), added in ascending order
template <class Z> JB_LN_HD double ln_block_ms(Z z, uint64_t i, uint32_t H)
{
    return (((z(i) + z(i + 1)) + z(i + 2)) + z(i + 3)) / (4.0 * (double)H);
}

// mean square of short-term window i: hops i..i+29, added in ascending order
template <class Z> JB_LN_HD double ln_window_ms(Z z, uint64_t i, uint32_t H)
{
    double s = z(i);
    for (uint32_t k = 1; k < kLnWindowHops; k++)
        s += z(i + k);
    return s / ((double)kLnWindowHops * (double)H);
}

// the gates: pass 0 keeps l above the absolute gate, pass 1 above the relative one (gamma) as well
JB_LN_HD bool ln_keep(double l, int pass, double gamma) { return l > kLnAbsGate && (pass == 0 || l > gamma); }

// A member's partial of one pass, lane `lane` of kLnLanes: the kept values of ms(i), i = lane, lane + 256, ... < n,
// added in that order.  The lanes' (sum, count) then go through ln_tree (the device: the same tree in LDS)
template <class MS> JB_LN_HD void ln_lane_partial(MS ms, uint64_t n, uint32_t lane, int pass, double gamma, double *sum,
                                                   uint32_t *cnt)
{
    double s = 0.0;
    uint32_t c = 0;
    for (uint64_t i = lane; i < n; i += kLnLanes) {
        const double v = ms(i);
        if (ln_keep(ln_loudness(v), pass, gamma)) {
            s += v;
            c++;
        }
    }
    *sum = s;
    *cnt = c;
}

// the tree over the kLnLanes lanes' partials, in place: lane t takes lane t + w for w = 128, 64, ..., 1
JB_LN_HD void ln_tree(double *sum, uint32_t *cnt)
{
    for (uint32_t w = kLnLanes / 2; w > 0; w >>= 1)
        for (uint32_t t = 0; t < w; t++) {
            sum[t] += sum[t + w];
            cnt[t] += cnt[t + w];
        }
}

// step 4: min(T - L, C - P) over the finite terms, 0 without one
JB_LN_HD double ln_gain_db(double target, double L, double ceiling, double P)
{
    double gain = 0.0;
    bool any = false;
    const double tl = target - L, cp = ceiling - P;
    if (isfinite(tl)) {
        gain = tl;
        any = true;
    }
    if (isfinite(cp)) {
        gain = any ? fmin(gain, cp) : cp;
        any = true;
    }
    return gain;
}

// the nearest-rank rule: the element of n ascending values that stands for the fraction p (n > 0)
JB_LN_HD uint64_t ln_rank(uint64_t n, double p) { return (uint64_t)floor((double)(n - 1) * p + 0.5); }

// The order of positive doubles is the integer order of their bit patterns: the selection works on these
JB_LN_HD uint64_t ln_bits(double v)
{
    union {
        double d;
        uint64_t u;
    } c;
    c.d = v;
    return c.u;
}
JB_LN_HD double ln_from_bits(uint64_t u)
{
    union {
        double d;
        uint64_t u;
    } c;
    c.u = u;
    return c.d;
}

// Radix selection, most significant byte first, 8 passes of 8 bits.  Pass p (0..7) looks at the values whose bytes
// above byte 7 - p equal `prefix` (p bytes; every value in pass 0) and counts them by that byte into 256 bins
JB_LN_HD bool ln_radix_in(uint64_t bits, uint64_t prefix, uint32_t pass)
{
    return pass == 0 || (bits >> (64 - 8 * pass)) == prefix;
}
JB_LN_HD uint32_t ln_radix_digit(uint64_t bits, uint32_t pass) { return (uint32_t)(bits >> (56 - 8 * pass)) & 255u; }
// the bin that holds element *rank of the counted values; *rank becomes its rank inside that bin
JB_LN_HD uint32_t ln_radix_pick(const uint32_t *hist, uint64_t *rank)
{
    uint64_t r = *rank;
    uint32_t b = 0;
    while (b < 255 && r >= hist[b]) {
        r -= hist[b];
        b++;
    }
    *rank = r;
    return b;
}

// What the gates give for one utterance or one group
struct LnGateOut {
    double lufs;          // L or L_G
    double rel_gate;      // Gamma (-INFINITY without a block above the absolute gate)
};
struct LnRangeOut {
    double max_momentary;  // LUFS, -INFINITY without a block
    double max_short_term; // LUFS, -INFINITY without a window
    double lra;            // LU, 0 for n = 0
    double lra_low, lra_high; // LUFS of the two percentile windows (NaN for n = 0)
    uint64_t n;            // windows above both gates
};

} // namespace jb

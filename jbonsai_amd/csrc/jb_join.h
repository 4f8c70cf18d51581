#pragma once
// jb_join.h -- the join stage (include/jbonsai_amd.h "Join"): a programme's PCM is its members one after the other, each
// between its own pads of zero samples and under its own edge fades.  The rules of one sample and of the geometry,
// stated once for the kernel (jb_join.hip), for the host seam (jb_join.cpp) and for the output plan (jb_output.cpp),
// and the work lists' entries of the programme stage, which the mix (jb_mix.h) shares.
// Plain C++17 and header-only; under hipcc the rules compile for the host and the device alike.
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
// (spelt without the HIP runtime header: jb_output.cpp includes this file without it)
#define JB_JOIN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_JOIN_HD inline
#endif

namespace jb {

// jb_join_utt of the public header, restated (this header stands without it; jb_join.cpp asserts the two agree)
struct JoinUtt {
    uint32_t programme;         // a caller's id below B, or kJoinNone
    uint32_t fade_in, fade_out; // samples at the output rate
    uint32_t reserved;
    uint64_t pad_before, pad_after;
};
static_assert(sizeof(JoinUtt) == 32 && offsetof(JoinUtt, pad_before) == 16, "jb_join_utt is 32 bytes");
constexpr uint32_t kJoinNone = 0xffffffffu; // JB_JOIN_NONE: the utterance is a programme of its own

// The programme stage's launch shape, the join's and the mix's alike
constexpr uint32_t kProgLanes = 256;
constexpr uint32_t kProgTileBytes = 16384; // destination bytes per workgroup: four 16-byte groups per lane
constexpr uint32_t kProgGroupBytes = 16;   // what one store writes; programmes start on such a boundary in their slab

// One member of a programme launch, in the order of its programme (ascending utterance index; in a join that is
// ascending by start)
struct ProgMember {
    const void *x;  // its final PCM: f64 or 16-bit samples (by the launch)
    uint64_t start; // its first sample within the programme (in a join: behind its pad_before)
    uint64_t n;
    uint32_t fade_in, fade_out;
    double g; // mix_gain of its gain_db (a join: 1, and not read)
};

// One span of a programme launch: samples [k0, k1) of one programme, k0 a multiple of a group's samples, k1 one too or
// the programme's end.  A run lists every programme whole, and so does a mix's redo; a join's redo lists the spans of
// the members that changed.  t0 is the prefix sum of the list's tiles (tiles never cross spans), pk0 the programme's
// first tile in the mix's peak scratch (the full run's numbering: a redo keeps it); the programme owns
// members[m0 .. m0 + nm), nm >= 1, and segs[s0 .. s0 + ns) (jb_mix.h).  A stem of a mix (jb_mix.h) is a span like any
// other, with its programme's members, segments of its own and `parent` naming the programme whose scale it takes
struct ProgSpan {
    void *y;    // the programme's first sample in its slab, 16-byte aligned
    uint64_t n; // the programme's samples
    uint64_t k0, k1, t0, pk0;
    uint32_t m0, nm;
    uint32_t s0, ns;
    uint32_t prog, parent; // (a programme: parent == prog)
};

// tiles of a span [k0, k1) of 16-bit or f64 samples
constexpr uint64_t prog_tiles(uint64_t k0, uint64_t k1, bool i16)
{
    return k1 > k0 ? (k1 - k0 + kProgTileBytes / (i16 ? 2 : 8) - 1) / (kProgTileBytes / (i16 ? 2 : 8)) : 0;
}

// floor(ms hz / 1000 + 0.5); 0 for a negative or NaN duration
JB_JOIN_HD uint64_t join_ms_to_samples(double ms, uint32_t hz)
{
    const double v = ms * (double)hz / 1000.0 + 0.5;
    return v >= 1.0 ? (uint64_t)v : 0; // (the conversion truncates: the floor of a positive value)
}

// The smoothstep weight of sample k < fade of a fade of `fade` samples, counted from the edge: evaluated as written,
// without contraction (the library is built with -ffp-contract=off), so that the host and the device agree bit for bit
JB_JOIN_HD double join_fade(uint64_t k, uint32_t fade)
{
    const double t = (double)(2 * k + 1) / (double)(2 * (uint64_t)fade);
    return (t * t) * (3.0 - 2.0 * t);
}

// samples [ka, kb] of a member of n samples lie outside both fades: they are copied
JB_JOIN_HD bool join_plain(uint64_t ka, uint64_t kb, uint64_t n, uint32_t fade_in, uint32_t fade_out)
{
    return ka >= fade_in && n - 1 - kb >= fade_out;
}

// Sample k of a member of n samples: x * s_in * s_out in that order, each factor only where its fade reaches; a sample
// outside both is returned as it came.  From f64 the product stays f64
JB_JOIN_HD double join_sample(double x, uint64_t k, uint64_t n, uint32_t fade_in, uint32_t fade_out)
{
    if (k < fade_in)
        x = x * join_fade(k, fade_in);
    const uint64_t kr = n - 1 - k;
    if (kr < fade_out)
        x = x * join_fade(kr, fade_out);
    return x;
}

// From 16 bits the product is truncated toward zero (the weights are in [0, 1]: no clamp)
JB_JOIN_HD int16_t join_sample(int16_t x, uint64_t k, uint64_t n, uint32_t fade_in, uint32_t fade_out)
{
    if (join_plain(k, k, n, fade_in, fade_out))
        return x;
    return (int16_t)(int32_t)join_sample((double)x, k, n, fade_in, fade_out);
}

// The member that holds sample k of a programme, among members[0 .. nm) ascending by start: the last one with
// start <= k searched in [lo, hi], or -1 where k lies in front of the first.  *inside: k is one of its samples (else
// k lies in a pad)
JB_JOIN_HD int32_t join_find(const ProgMember *members, int32_t lo, int32_t hi, uint64_t k, bool *inside)
{
    if (members[lo].start > k) {
        *inside = false;
        return lo - 1;
    }
    while (hi > lo) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (members[mid].start <= k)
            lo = mid;
        else
            hi = mid - 1;
    }
    *inside = k - members[lo].start < members[lo].n;
    return lo;
}

// Sample k of a programme by the rules above: a member's sample, or the zero of a pad
template <class T> JB_JOIN_HD T join_value(const ProgMember *members, int32_t lo, int32_t hi, uint64_t k)
{
    bool inside;
    const int32_t j = join_find(members, lo, hi, k, &inside);
    if (!inside)
        return (T)0;
    const ProgMember m = members[j];
    return join_sample(((const T *)m.x)[k - m.start], k - m.start, m.n, m.fade_in, m.fade_out);
}

} // namespace jb

#pragma once
// jb_adpcm.h -- IMA ADPCM (WAV format tag 0x0011, mono; include/jbonsai_amd.h "IMA ADPCM"): the geometry of a stream,
// the rules of one block and of one sample, stated once for the kernel (jb_adpcm.hip), for the host half
// (jb_adpcm.cpp) and for the output plan (jb_output.cpp), and the stage's work list.
// Plain C++17 and header-only; under hipcc the rules compile for the host and the device alike.
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
// (spelt without the HIP runtime header: jb_output.cpp includes this file without it)
#define JB_ADPCM_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_ADPCM_HD inline
#endif

namespace jb {

// jb_adpcm_opts of the public header, restated (this header stands without it; jb_adpcm.cpp asserts the two agree)
struct AdpcmOpts {
    uint32_t block_align;
    uint32_t reserved[3];
};
static_assert(sizeof(AdpcmOpts) == 16 && offsetof(AdpcmOpts, reserved) == 4, "jb_adpcm_opts is 16 bytes");

constexpr uint32_t kAdpcmSteps = 89;
constexpr uint32_t kAdpcmLanes = 256; // blocks per workgroup: one lane each, a wave 64 consecutive ones
constexpr uint32_t kAdpcmSub = 64;    // samples of each block a round stages in LDS (8 packed dwords out)

// a request's block_align: 0 (by the rate) or a multiple of 4 in 32..8192
constexpr bool adpcm_align_ok(uint32_t a) { return a == 0 || (a >= 32 && a <= 8192 && a % 4 == 0); }
// A of a stream at hz: the request's, or the Microsoft convention by the rate
constexpr uint32_t adpcm_block_align(uint32_t hz, uint32_t a) { return a ? a : hz < 22050 ? 256 : hz < 44100 ? 512 : 1024; }
constexpr uint32_t adpcm_spb(uint32_t A) { return 2 * (A - 4) + 1; } // samples per block
constexpr uint64_t adpcm_blocks(uint64_t n, uint32_t A) { return (n + adpcm_spb(A) - 1) / adpcm_spb(A); }
constexpr uint64_t adpcm_bytes(uint64_t n, uint32_t A) { return adpcm_blocks(n, A) * A; }

// One utterance of an ADPCM launch.  Launch lists are in utterance order; g0 is the prefix sum of the list's
// workgroups (kAdpcmLanes blocks each; workgroups never cross utterances)
struct AdpcmUtt {
    const void *x; // the chain's final PCM: f64 in 16-bit scale, or 16-bit samples (by the launch)
    uint8_t *y;    // its blocks, 16-byte aligned
    uint64_t n, g0;
    uint32_t A, spb;
};

// the standard IMA step table
JB_ADPCM_HD int32_t adpcm_step_of(uint32_t i)
{
    constexpr int32_t t[kAdpcmSteps] = {
        7,     8,     9,     10,    11,    12,    13,    14,    16,    17,    19,    21,    23,    25,    28,
        31,    34,    37,    41,    45,    50,    55,    60,    66,    73,    80,    88,    97,    107,   118,
        130,   143,   157,   173,   190,   209,   230,   253,   279,   307,   337,   371,   408,   449,   494,
        544,   598,   658,   724,   796,   876,   963,   1060,  1166,  1282,  1411,  1552,  1707,  1878,  2066,
        2272,  2499,  2749,  3024,  3327,  3660,  4026,  4428,  4871,  5358,  5894,  6484,  7132,  7845,  8630,
        9493,  10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};
    return t[i];
}

// i0 of a block: the smallest i with tab[i] >= d, 88 if there is none; d = floor(sum_{k=1..8} |b[k] - b[k-1]| / 8)
template <class Tab> JB_ADPCM_HD int32_t adpcm_start_index(int32_t d, Tab tab)
{
    int32_t lo = 0, hi = (int32_t)kAdpcmSteps - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (tab[mid] >= d)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// One sample s against the state (pred, idx), step = STEP[idx]: its 4-bit code; the state moves on as a decoder's
JB_ADPCM_HD uint32_t adpcm_code(int32_t s, int32_t step, int32_t &pred, int32_t &idx)
{
    int32_t diff = s - pred;
    const uint32_t sign = diff < 0 ? 8u : 0u;
    diff = diff < 0 ? -diff : diff;
    uint32_t delta = 0;
    int32_t vp = step >> 3;
    if (diff >= step) {
        delta = 4;
        diff -= step;
        vp += step;
    }
    step >>= 1;
    if (diff >= step) {
        delta |= 2;
        diff -= step;
        vp += step;
    }
    step >>= 1;
    if (diff >= step) {
        delta |= 1;
        vp += step;
    }
    pred = sign ? pred - vp : pred + vp;
    pred = pred > 32767 ? 32767 : pred < -32768 ? -32768 : pred;
    idx += delta < 4 ? -1 : ((int32_t)delta - 3) * 2; // IDX = {-1, -1, -1, -1, 2, 4, 6, 8}
    idx = idx < 0 ? 0 : idx > 88 ? 88 : idx;
    return delta | sign;
}

// The decoder's step: the same vp from the code's bits
JB_ADPCM_HD void adpcm_decode(uint32_t code, int32_t step, int32_t &pred, int32_t &idx)
{
    int32_t vp = step >> 3;
    if (code & 4)
        vp += step;
    if (code & 2)
        vp += step >> 1;
    if (code & 1)
        vp += step >> 2;
    pred = (code & 8) ? pred - vp : pred + vp;
    pred = pred > 32767 ? 32767 : pred < -32768 ? -32768 : pred;
    const uint32_t delta = code & 7;
    idx += delta < 4 ? -1 : ((int32_t)delta - 3) * 2;
    idx = idx < 0 ? 0 : idx > 88 ? 88 : idx;
}

// JB_OK, or JB_ERR_INVALID (set_error says why): a null pointer, a bad block_align, a non-zero reserved word
int adpcm_check_opts(const AdpcmOpts *opts, const char *who);

} // namespace jb

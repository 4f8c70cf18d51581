#pragma once
// jb_format.h -- the output sample formats (include/jbonsai_amd.h "Output sample formats"): the rules of one sample,
// stated once for the kernel (jb_format.hip) and for the host seam (jb_format.cpp), and the stage's work list.
// Plain C++17; under hipcc the rules compile for the host and the device alike.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define JB_FMT_HD __host__ __device__ __forceinline__
#else
#define JB_FMT_HD inline
#endif

namespace jb {

// JB_FMT_* / JB_DITHER_* of the public header, as plain values (this header stands without it)
constexpr uint32_t kFmtNone = 0, kFmtF32 = 1, kFmtS16 = 2, kFmtS24 = 3, kFmtUlaw = 4, kFmtAlaw = 5;
constexpr uint32_t kDitherNone = 0, kDitherTpdf = 1;
constexpr uint32_t kFmtTile = 4096; // samples per workgroup: a multiple of every format's per-lane group and of 16
constexpr uint32_t kFmtLanes = 256;

constexpr size_t format_bytes(uint32_t fmt)
{
    return fmt == kFmtF32 ? 4 : fmt == kFmtS16 ? 2 : fmt == kFmtS24 ? 3 : (fmt == kFmtUlaw || fmt == kFmtAlaw) ? 1 : 0;
}

// One utterance of a format launch.  Launch lists are in utterance order; ft0 is the prefix sum of the list's tiles
struct FormatUtt {
    const double *x; // the chain's final f64, 16-bit scale
    uint8_t *y;      // its bytes, 16-byte aligned
    uint64_t n, ft0;
};

// the splitmix64 finaliser
JB_FMT_HD uint64_t fmt_mix(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// TPDF dither of sample k of its utterance, in (-1, 1) LSB; mseed = fmt_mix(seed)
JB_FMT_HD double fmt_dither(uint64_t mseed, uint64_t k)
{
    const uint64_t r = fmt_mix(mseed ^ k);
    return ((double)(uint32_t)(r >> 32) - (double)(uint32_t)r) * 0x1p-32;
}

// q(x) into [lo, hi]: the 16-bit sink's rule (clamp, then truncate toward zero; jb_vocoder.hip pcm_i16) without
// dither, floor((x + d) + 0.5) clamped with it
template <bool kDither> JB_FMT_HD int32_t fmt_quant(double x, double lo, double hi, uint64_t mseed, uint64_t k)
{
    if (kDither)
        x = floor((x + fmt_dither(mseed, k)) + 0.5);
    x = fmin(x, hi);
    x = fmax(x, lo);
    return (int32_t)x;
}

JB_FMT_HD int fmt_top_bit(uint32_t m) // index of m's highest set bit, m > 0
{
#ifdef __HIP_DEVICE_COMPILE__
    return 31 - __clz((int)m);
#else
    return 31 - __builtin_clz(m);
#endif
}

// G.711 of a 16-bit sample, as the common C implementation has it (14-bit mu-law with the clip at 8159, 13-bit A-law)
JB_FMT_HD uint32_t fmt_ulaw(int32_t s)
{
    const int32_t p = s >> 2;
    const bool neg = p < 0;
    const uint32_t mag = (uint32_t)(neg ? -p : p);
    const uint32_t m = (mag > 8159u ? 8159u : mag) + 33u;
    const int seg = fmt_top_bit(m) - 5;
    // (the clip plus the bias reaches 2^13, one past the last segment: the largest code, as that implementation
    // returns it)
    const uint32_t code = seg >= 8 ? 0x7Fu : ((uint32_t)seg << 4) | ((m >> (seg + 1)) & 15u);
    return code ^ (neg ? 0x7Fu : 0xFFu);
}

JB_FMT_HD uint32_t fmt_alaw(int32_t s)
{
    const int32_t p = s >> 3;
    const bool neg = p < 0;
    const uint32_t m = (uint32_t)(neg ? -p - 1 : p);
    int seg = fmt_top_bit(m > 1u ? m : 1u) - 4;
    seg = seg < 0 ? 0 : seg;
    const uint32_t code = ((uint32_t)seg << 4) | ((m >> (seg < 2 ? 1 : seg)) & 15u);
    return code ^ (neg ? 0x55u : 0xD5u);
}

// Sample k of its utterance in format kFmt: the value its bytes spell, little-endian (F32: the float's bits)
template <uint32_t kFmt, bool kDither> JB_FMT_HD uint32_t fmt_sample(double v, uint64_t mseed, uint64_t k)
{
    if (kFmt == kFmtF32) {
        const float f = (float)(v * 0x1p-15);
        uint32_t u;
        __builtin_memcpy(&u, &f, 4);
        return u;
    }
    if (kFmt == kFmtS24)
        return (uint32_t)fmt_quant<kDither>(256.0 * v, -8388608.0, 8388607.0, mseed, k) & 0xffffffu;
    const int32_t s = fmt_quant<kDither>(v, -32768.0, 32767.0, mseed, k);
    if (kFmt == kFmtUlaw)
        return fmt_ulaw(s);
    if (kFmt == kFmtAlaw)
        return fmt_alaw(s);
    return (uint32_t)s & 0xffffu;
}

// JB_OK, or JB_ERR_INVALID (set_error says why): a null pointer, an unknown format, dither where it has no meaning
int format_check_opts(uint32_t format, uint32_t dither, const char *who);

} // namespace jb

#pragma once
// jb_md5.h -- the metadata of a FLAC stream that needs its samples or its frame offsets (include/jbonsai_amd.h
// "FLAC"): MD5 (RFC 1321) of the 16-bit output as STREAMINFO carries it, and the geometry of the SEEKTABLE, stated once
// for the kernels (jb_flac.hip), for the host half (jb_flac.cpp) and for the plan.
// Plain C++17 and header-only; under hipcc the rules compile for the host and the device alike.
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
// (spelt without the HIP runtime header, as jb_adpcm.h does)
#define JB_MD5_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_MD5_HD inline
#endif

namespace jb {

// jb_flac_meta of the public header, restated (this header stands without it; jb_flac.cpp asserts the two agree)
struct FlacMeta {
    uint32_t flags;
    uint32_t seek_interval_ms;
    uint32_t reserved[2];
};
static_assert(sizeof(FlacMeta) == 16 && offsetof(FlacMeta, reserved) == 8, "jb_flac_meta is 16 bytes");
constexpr uint32_t kFlacMetaMd5 = 1u; // JB_FLAC_MD5

// ---- MD5 ----
// The message of an utterance is its 16-bit output as little-endian bytes, 2 N of them (FLAC's definition for mono
// 16-bit); a block is 16 little-endian words.  Padding: one 0x80 byte, zeros to 56 mod 64, the bit length (16 N) as a
// 64-bit little-endian count.  The digest is A, B, C, D, each little-endian, in that order.
constexpr uint32_t kMd5Init[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};

JB_MD5_HD uint32_t md5_k(int i)
{
    constexpr uint32_t k[64] = {
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
        0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
        0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
        0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
        0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
        0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
        0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
        0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
    return k[i];
}
JB_MD5_HD uint32_t md5_s(int i)
{
    constexpr uint8_t s[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    return s[(i >> 4) * 4 + (i & 3)];
}

// One block m[0..16) into the state st.  Every index is a constant once the loop is unrolled: on the device the 64
// steps are straight-line code over registers (F and G as bit selects, H a three-way xor, the sums three-way adds)
JB_MD5_HD void md5_block(uint32_t st[4], const uint32_t m[16])
{
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        uint32_t f;
        int g;
        if (i < 16) {
            f = d ^ (b & (c ^ d)); // b ? c : d
            g = i;
        } else if (i < 32) {
            f = c ^ (d & (b ^ c)); // d ? b : c
            g = (5 * i + 1) & 15;
        } else if (i < 48) {
            f = b ^ c ^ d;
            g = (3 * i + 5) & 15;
        } else {
            f = c ^ (b | ~d);
            g = (7 * i) & 15;
        }
        const uint32_t t = a + f + (m[g] + md5_k(i));
        a = d;
        d = c;
        c = b;
        b += __builtin_rotateleft32(t, md5_s(i));
    }
    st[0] += a;
    st[1] += b;
    st[2] += c;
    st[3] += d;
}

// Blocks of the padded message of n samples (32 samples to a block; the 0x80 byte and the count need 9 bytes)
JB_MD5_HD uint64_t md5_blocks(uint64_t n) { return (2 * n + 9 + 63) / 64; }
// The bit length of n samples.  16 n needs more than 32 bits from 2^28 samples on and its 64 bits cannot overflow
// below 2^60 samples (FLAC's STREAMINFO counts 36 bits): computed in 64 bits, never truncated
JB_MD5_HD uint64_t md5_bit_length(uint64_t n) { return 16 * n; }

// Bits sh .. sh + 31 of hi:lo (sh is 0 or 16)
JB_MD5_HD uint32_t md5_cut(uint32_t hi, uint32_t lo, uint32_t sh)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#endif
}

// The chain of one utterance of n samples that starts on a dword (odd false) or a half-word behind one (odd true:
// an utterance starts at a prefix sum of sample counts in a slab that starts on a dword).  dword(i) is aligned dword
// i counted from the one that holds sample 0: with an odd start it holds samples 2 i - 1 and 2 i, and dword 0 the
// sample in front of the utterance, inside the slab.  sample(i) is sample i.  Blocks with a sample behind them
// (32 k + 32 <= n - 1) are read as dwords, 16 of them, and a 17th where the start is odd, cut to words by a shift;
// the next block's are asked for before this one is hashed.  The last one or two blocks -- the samples left, the
// 0x80 byte, zeros, the bit count -- are built from single samples: nothing behind sample n - 1 is read.
template <class Dword, class Sample>
JB_MD5_HD void md5_samples(uint64_t n, bool odd, Dword dword, Sample sample, uint32_t st[4])
{
    const uint32_t sh = odd ? 16u : 0u;
    const uint64_t nfull = n ? (n - 1) / 32 : 0, nb = md5_blocks(n), bits = md5_bit_length(n);
    for (int j = 0; j < 4; j++)
        st[j] = kMd5Init[j];
    uint32_t nx[17];
    for (int j = 0; j < 17; j++)
        nx[j] = 0;
    if (nfull) {
#pragma unroll
        for (int j = 0; j < 16; j++)
            nx[j] = dword(j);
        if (odd)
            nx[16] = dword(16);
    }
    for (uint64_t k = 0; k < nb; k++) {
        uint32_t m[16];
        if (k < nfull) {
            uint32_t cur[17];
#pragma unroll
            for (int j = 0; j < 17; j++)
                cur[j] = nx[j];
            if (k + 1 < nfull) {
#pragma unroll
                for (int j = 0; j < 16; j++)
                    nx[j] = dword(16 * (k + 1) + j);
                if (odd)
                    nx[16] = dword(16 * (k + 1) + 16);
            }
#pragma unroll
            for (int j = 0; j < 16; j++)
                m[j] = md5_cut(cur[j + 1], cur[j], sh);
        } else {
#pragma unroll
            for (int j = 0; j < 32; j++) {
                const uint64_t i = 32 * k + j;
                const uint32_t h = i < n ? (uint32_t)(uint16_t)sample(i) : i == n ? 0x80u : 0u;
                if (j & 1)
                    m[j >> 1] |= h << 16;
                else
                    m[j >> 1] = h;
            }
            if (k == nb - 1) {
                m[14] = (uint32_t)bits;
                m[15] = (uint32_t)(bits >> 32);
            }
        }
        md5_block(st, m);
    }
}

// ---- SEEKTABLE geometry ----
constexpr uint32_t kFlacStreamInfoBytes = 42; // fLaC + the STREAMINFO block
constexpr uint32_t kFlacSeekPointBytes = 18;  // u64 sample number, u64 byte offset, u16 samples; big-endian
constexpr uint32_t kFlacMaxSeekPoints = 65535;

struct SeekGeometry {
    uint32_t step, n_points, header_bytes; // frames between points (0 with no table), points, bytes before frame 0
};
// interval_ms == 0: no table.  Otherwise the points are the frames 0, step, 2 step, ... below nframes with
// step = max(1, round(interval / block duration)), raised until at most kFlacMaxSeekPoints remain; nframes == 0 has
// no table either (STREAMINFO stays the last block)
JB_MD5_HD SeekGeometry flac_seek_geometry(uint64_t n_samples, uint32_t bs, uint32_t hz, uint32_t interval_ms)
{
    SeekGeometry g{0, 0, kFlacStreamInfoBytes};
    const uint64_t nframes = (n_samples + bs - 1) / bs;
    if (!interval_ms || !nframes)
        return g;
    uint64_t step = ((uint64_t)interval_ms * hz + 500ull * bs) / (1000ull * bs);
    if (step < 1)
        step = 1;
    const uint64_t cap = (nframes + kFlacMaxSeekPoints - 1) / kFlacMaxSeekPoints;
    if (step < cap)
        step = cap;
    g.step = (uint32_t)(step > 0xffffffffull ? 0xffffffffull : step);
    g.n_points = (uint32_t)((nframes + g.step - 1) / g.step);
    g.header_bytes = kFlacStreamInfoBytes + 4 + kFlacSeekPointBytes * g.n_points;
    return g;
}

} // namespace jb

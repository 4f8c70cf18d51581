// jb_format.hip -- the output sample formats on the device: the chain's final f64 PCM as float32, 16- or 24-bit PCM
// (with or without TPDF dither) or G.711, by the rules of jb_format.h.
//
//   k_format<FMT, DITHER>   one workgroup per tile of kFmtTile samples of one utterance (tiles never cross
//                           utterances; every utterance's bytes start on a 16-byte boundary).  A lane takes groups
//                           of G consecutive samples -- 4 (F32, S24), 8 (S16) or 16 (G.711) -- loads them 16 B at a
//                           time and stores the group's bytes as whole dwords: one dwordx4 (F32, S16, G.711) or one
//                           dwordx3 packed in registers (S24).  Only an utterance's last partial group goes out
//                           sample by sample.  A pure streaming pass: per sample and independent, so the bytes of
//                           an utterance do not depend on the batch around it.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

// the f64 slabs are 8-byte aligned per utterance (an odd offset is allowed), the S24 groups 4-byte aligned
// (plain vector types: a load or a store through a pointer with a named address space needs no class operator)
typedef double FmtD2 __attribute__((ext_vector_type(2), aligned(8)));
typedef uint32_t FmtU3 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t FmtU4 __attribute__((ext_vector_type(4)));
// (a pointer read from the work list is generic to the compiler: named global, the accesses are global_ ones)
#define JB_FMT_GLOBAL __attribute__((address_space(1)))

constexpr uint32_t fmt_group(uint32_t fmt)
{
    return fmt == kFmtS16 ? 8 : (fmt == kFmtUlaw || fmt == kFmtAlaw) ? 16 : 4;
}

template <uint32_t kFmt, bool kDither>
__global__ __launch_bounds__(kFmtLanes) void k_format(const FormatUtt *__restrict__ utts, uint32_t n_utts,
                                                      uint64_t mseed)
{
    constexpr uint32_t G = fmt_group(kFmt);
    constexpr uint32_t NB = (uint32_t)format_bytes(kFmt);
    static_assert(kFmtTile % (kFmtLanes * G) == 0 && kFmtTile % 16 == 0, "a tile is whole groups of every lane");
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x, &FormatUtt::ft0);
    const FormatUtt U = utts[u];
    const uint64_t k0 = (blockIdx.x - U.ft0) * (uint64_t)kFmtTile;
    if (k0 >= U.n)
        return;
    const uint64_t k1 = std::min<uint64_t>(k0 + kFmtTile, U.n);
    const JB_FMT_GLOBAL double *gx = (const JB_FMT_GLOBAL double *)U.x;
    JB_FMT_GLOBAL uint8_t *gy = (JB_FMT_GLOBAL uint8_t *)U.y;
#pragma unroll
    for (uint32_t i = 0; i < kFmtTile / (kFmtLanes * G); i++) {
        const uint64_t ks = k0 + (uint64_t)(i * kFmtLanes + threadIdx.x) * G;
        if (ks + G <= k1) {
            uint32_t w[G];
#pragma unroll
            for (uint32_t j = 0; j < G; j += 2) {
                const FmtD2 v = *(const JB_FMT_GLOBAL FmtD2 *)(gx + ks + j);
                w[j] = fmt_sample<kFmt, kDither>(v.x, mseed, ks + j);
                w[j + 1] = fmt_sample<kFmt, kDither>(v.y, mseed, ks + j + 1);
            }
            JB_FMT_GLOBAL uint8_t *y = gy + ks * NB;
            if constexpr (kFmt == kFmtF32) {
                *(JB_FMT_GLOBAL FmtU4 *)y = FmtU4{w[0], w[1], w[2], w[3]};
            } else if constexpr (kFmt == kFmtS16) {
                *(JB_FMT_GLOBAL FmtU4 *)y =
                    FmtU4{w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16)};
            } else if constexpr (kFmt == kFmtS24) {
                *(JB_FMT_GLOBAL FmtU3 *)y =
                    FmtU3{w[0] | (w[1] << 24), (w[1] >> 8) | (w[2] << 16), (w[2] >> 16) | (w[3] << 8)};
            } else {
                uint32_t d[4];
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    d[q] = w[4 * q] | (w[4 * q + 1] << 8) | (w[4 * q + 2] << 16) | (w[4 * q + 3] << 24);
                *(JB_FMT_GLOBAL FmtU4 *)y = FmtU4{d[0], d[1], d[2], d[3]};
            }
        } else if (ks < k1) {
            // the utterance's last partial group
            for (uint64_t k = ks; k < k1; k++) {
                const uint32_t w = fmt_sample<kFmt, kDither>(gx[k], mseed, k);
                JB_FMT_GLOBAL uint8_t *y = gy + k * NB;
                if constexpr (NB == 4) {
                    *(JB_FMT_GLOBAL uint32_t *)y = w;
                } else if constexpr (NB == 2) {
                    *(JB_FMT_GLOBAL uint16_t *)y = (uint16_t)w;
                } else {
                    for (uint32_t j = 0; j < NB; j++)
                        y[j] = (uint8_t)(w >> (8 * j));
                }
            }
        }
    }
}

template <uint32_t kFmt, bool kDither>
void format_launch(uint64_t mseed, const FormatUtt *utts, uint32_t n, uint32_t tiles, hipStream_t s)
{
    hipLaunchKernelGGL((k_format<kFmt, kDither>), dim3(tiles), dim3(kFmtLanes), 0, s, utts, n, mseed);
}

} // namespace

hipError_t launch_format(uint32_t format, uint32_t dither, uint64_t seed, const FormatUtt *utts_dev, uint32_t n,
                         uint64_t tiles, hipStream_t stream)
{
    if (n == 0 || tiles == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    const uint64_t ms = fmt_mix(seed);
    const uint32_t t = (uint32_t)tiles;
    const bool d = dither == kDitherTpdf;
    switch (format) {
    case kFmtF32:
        format_launch<kFmtF32, false>(ms, utts_dev, n, t, stream);
        break;
    case kFmtS16:
        d ? format_launch<kFmtS16, true>(ms, utts_dev, n, t, stream)
          : format_launch<kFmtS16, false>(ms, utts_dev, n, t, stream);
        break;
    case kFmtS24:
        d ? format_launch<kFmtS24, true>(ms, utts_dev, n, t, stream)
          : format_launch<kFmtS24, false>(ms, utts_dev, n, t, stream);
        break;
    case kFmtUlaw:
        format_launch<kFmtUlaw, false>(ms, utts_dev, n, t, stream);
        break;
    case kFmtAlaw:
        format_launch<kFmtAlaw, false>(ms, utts_dev, n, t, stream);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_format_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_format_opts *opts,
                        int32_t device, uint8_t **out, size_t *n_bytes)
{
    if (!opts) {
        set_error("jb_format_pcm_batch: opts is NULL");
        return JB_ERR_INVALID;
    }
    int rc = format_check_opts(opts->format, opts->dither, "jb_format_pcm_batch");
    if (rc)
        return rc;
    if ((rc = pcm_check((const void *const *)in, n_in, n, out && n_bytes, (void **)out, n_bytes)))
        return rc;
    const size_t nb = format_bytes(opts->format);
    DeviceScratch ds;
    if ((rc = ds.open(device, "jb_format_pcm_batch")))
        return rc;
    // the inputs packed one after the other (8-byte aligned, as a batch's slab has them), every output on a
    // 16-byte boundary
    std::vector<uint64_t> xoff;
    const double *dx = ds.pack(in, n_in, n, &xoff);
    std::vector<FormatUtt> utts(n);
    std::vector<PcmShare> shares(n);
    uint64_t bytes = 0, tiles = 0;
    for (size_t u = 0; u < n; u++) {
        utts[u].n = n_in[u];
        utts[u].ft0 = tiles;
        shares[u] = {bytes, n_in[u] * nb};
        bytes += (n_in[u] * nb + 15) & ~(uint64_t)15;
        tiles += (n_in[u] + kFmtTile - 1) / kFmtTile;
    }
    uint8_t *dy = ds.alloc<uint8_t>(std::max<uint64_t>(bytes, 16));
    for (size_t u = 0; u < n; u++) {
        utts[u].x = dx + xoff[u];
        utts[u].y = dy + shares[u].off;
    }
    const FormatUtt *du = ds.upload(utts);
    if (ds.ok())
        ds.err = launch_format(opts->format, opts->dither, opts->seed, du, (uint32_t)n, tiles, ds.stream);
    std::vector<uint8_t> host;
    ds.read_back(&host, dy, bytes);
    if ((rc = ds.status()))
        return rc;
    return hand_out(host.data(), 1, shares, (void **)out, n_bytes);
}

} // extern "C"

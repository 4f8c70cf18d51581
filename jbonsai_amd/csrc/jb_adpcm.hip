// jb_adpcm.hip -- IMA ADPCM on the device: the chain's final PCM (f64 or 16-bit) as 4-bit WAV blocks, by the rules of
// jb_adpcm.h.
//
//   k_adpcm<SRC>   one lane per block, a wave 64 consecutive blocks of one utterance, a workgroup kAdpcmLanes of them
//                  (workgroups never cross utterances; every utterance's bytes start on a 16-byte boundary).  A lane's
//                  samples lie spb samples from its neighbour's, so the block is walked in rounds of kAdpcmSub samples
//                  staged through LDS: the wave loads each of its blocks' sub-tile in contiguous 16-byte pieces
//                  (a row of 64 f64 is 512 B in a run, of 64 int16 128 B), quantises them and parks them two to a
//                  dword in rows of 33 dwords (the odd stride spreads the 32 lanes of a half over the 32 banks); each
//                  lane then walks its own row with pred and idx in registers and the step table in LDS, packs eight
//                  codes per dword into rows of 9 dwords, and the wave stores them as whole dwords, eight lanes to a
//                  block's run of 32 B.  The padded tail of an utterance's last block repeats sample n - 1 and reads
//                  nothing behind it.  Integer and per block: an utterance's bytes do not depend on the batch.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

typedef double AdD2 __attribute__((ext_vector_type(2), aligned(8)));
typedef int16_t AdS8 __attribute__((ext_vector_type(8), aligned(2)));
#define JB_ADPCM_GLOBAL __attribute__((address_space(1)))

constexpr uint32_t kRowDw = kAdpcmSub / 2 + 1; // a block's sub-tile, two samples to a dword, padded
constexpr uint32_t kOutDw = kAdpcmSub / 8 + 1; // its packed codes, padded
constexpr uint32_t kWaves = kAdpcmLanes / 64;

__device__ __forceinline__ int32_t ad_sample(double v) { return fmt_quant<false>(v, -32768.0, 32767.0, 0, 0); }
__device__ __forceinline__ int32_t ad_sample(int16_t v) { return v; }
__device__ __forceinline__ uint32_t ad_pack(int32_t a, int32_t b) { return ((uint32_t)a & 0xffffu) | ((uint32_t)b << 16); }

// The wave's rows [0, nrows) of this round: samples [k0 + row * spb, + ns) of the utterance, ns a multiple of 8,
// quantised and packed into tile[row * kRowDw ..]; an index past n - 1 reads sample n - 1
__device__ __forceinline__ void ad_stage(const JB_ADPCM_GLOBAL double *x, uint64_t n, uint64_t k0, uint32_t spb,
                                         uint32_t nrows, uint32_t ns, uint32_t lane, uint32_t *tile)
{
    const uint32_t c = lane & 31; // the row's pair of samples
#pragma unroll 8
    for (uint32_t i = 0; i < 32; i++) {
        const uint32_t row = 2 * i + (lane >> 5);
        if (row < nrows && 2 * c < ns) {
            const uint64_t k = k0 + (uint64_t)row * spb + 2 * c;
            double a, b;
            if (k + 1 < n) {
                const AdD2 v = *(const JB_ADPCM_GLOBAL AdD2 *)(x + k);
                a = v.x;
                b = v.y;
            } else {
                a = x[std::min<uint64_t>(k, n - 1)];
                b = x[n - 1];
            }
            tile[row * kRowDw + c] = ad_pack(ad_sample(a), ad_sample(b));
        }
    }
}

__device__ __forceinline__ void ad_stage(const JB_ADPCM_GLOBAL int16_t *x, uint64_t n, uint64_t k0, uint32_t spb,
                                         uint32_t nrows, uint32_t ns, uint32_t lane, uint32_t *tile)
{
    const uint32_t c = lane & 7; // the row's group of 8 samples
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
        const uint32_t row = 8 * i + (lane >> 3);
        if (row < nrows && 8 * c < ns) {
            const uint64_t k = k0 + (uint64_t)row * spb + 8 * c;
            int16_t s[8];
            if (k + 7 < n) {
                const AdS8 v = *(const JB_ADPCM_GLOBAL AdS8 *)(x + k);
#pragma unroll
                for (uint32_t j = 0; j < 8; j++)
                    s[j] = v[j];
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 8; j++)
                    s[j] = x[std::min<uint64_t>(k + j, n - 1)];
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                tile[row * kRowDw + 4 * c + j] = ad_pack(s[2 * j], s[2 * j + 1]);
        }
    }
}

template <class SRC>
__global__ __launch_bounds__(kAdpcmLanes) void k_adpcm(const AdpcmUtt *__restrict__ utts, uint32_t n_utts)
{
    __shared__ int32_t steps[kAdpcmSteps + 7];
    __shared__ uint32_t tiles[kWaves][64 * kRowDw];
    __shared__ uint32_t outs[kWaves][64 * kOutDw];
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x);
    const AdpcmUtt U = utts[u];
    const uint32_t A = U.A, spb = U.spb;
    const uint64_t n = U.n;
    const uint64_t nb = (n + spb - 1) / spb;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t wb0 = (blockIdx.x - U.g0) * (uint64_t)kAdpcmLanes + wave * 64; // the wave's first block
    const uint32_t nrows = wb0 < nb ? (uint32_t)std::min<uint64_t>(64, nb - wb0) : 0;
    const bool live = lane < nrows;
    const uint64_t blk = wb0 + lane;
    const JB_ADPCM_GLOBAL SRC *gx = (const JB_ADPCM_GLOBAL SRC *)U.x;
    JB_ADPCM_GLOBAL uint8_t *gy = (JB_ADPCM_GLOBAL uint8_t *)U.y;
    uint32_t *tile = tiles[wave], *outb = outs[wave];
    if (threadIdx.x < kAdpcmSteps)
        steps[threadIdx.x] = adpcm_step_of(threadIdx.x);
    // b[0] of the lane's block (a live block's first sample exists)
    int32_t pred = live ? ad_sample(gx[blk * spb]) : 0, idx = 0;
    const uint32_t ndw = A / 4 - 1; // dwords of codes per block, 8 samples each
    for (uint32_t r = 0; r * 8 < ndw; r++) {
        const uint32_t dws = std::min<uint32_t>(8, ndw - r * 8);
        ad_stage(gx, n, wb0 * spb + 1 + (uint64_t)r * kAdpcmSub, spb, nrows, dws * 8, lane, tile);
        __syncthreads();
        if (live) {
            const uint32_t *row = tile + lane * kRowDw;
            if (r == 0) {
                // the header: b[0], and i0 from b[0..8]
                int32_t d = 0, prev = pred;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t v = row[j];
                    const int32_t s0 = (int16_t)(v & 0xffffu), s1 = (int32_t)v >> 16;
                    d += abs(s0 - prev) + abs(s1 - s0);
                    prev = s1;
                }
                idx = adpcm_start_index(d >> 3, steps);
                *(JB_ADPCM_GLOBAL uint32_t *)(gy + blk * A) = ((uint32_t)pred & 0xffffu) | ((uint32_t)idx << 16);
            }
            for (uint32_t q = 0; q < dws; q++) {
                uint32_t w = 0;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t v = row[4 * q + j];
                    const int32_t s0 = (int16_t)(v & 0xffffu), s1 = (int32_t)v >> 16;
                    w |= adpcm_code(s0, steps[idx], pred, idx) << (8 * j);
                    w |= adpcm_code(s1, steps[idx], pred, idx) << (8 * j + 4);
                }
                outb[lane * kOutDw + q] = w;
            }
        }
        __syncthreads();
        // eight lanes to a block: its run of dws dwords
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) {
            const uint32_t row = 8 * i + (lane >> 3), q = lane & 7;
            if (row < nrows && q < dws)
                *(JB_ADPCM_GLOBAL uint32_t *)(gy + (wb0 + row) * A + 4 + (size_t)(r * 8 + q) * 4) =
                    outb[row * kOutDw + q];
        }
    }
}

} // namespace

hipError_t launch_adpcm(bool i16, const AdpcmUtt *utts_dev, uint32_t n, uint64_t groups, hipStream_t stream)
{
    if (n == 0 || groups == 0)
        return hipSuccess;
    if (groups > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (i16)
        hipLaunchKernelGGL((k_adpcm<int16_t>), dim3((uint32_t)groups), dim3(kAdpcmLanes), 0, stream, utts_dev, n);
    else
        hipLaunchKernelGGL((k_adpcm<double>), dim3((uint32_t)groups), dim3(kAdpcmLanes), 0, stream, utts_dev, n);
    return hipGetLastError();
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_adpcm_encode_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                              const jb_adpcm_opts *opts, int32_t device, uint8_t **out, size_t *n_bytes)
{
    int rc = adpcm_check_opts((const AdpcmOpts *)opts, "jb_adpcm_encode_pcm_batch");
    if (rc)
        return rc;
    if ((rc = pcm_check((const void *const *)in, n_in, n, hz && out && n_bytes, (void **)out, n_bytes)))
        return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, "jb_adpcm_encode_pcm_batch")))
        return rc;
    // the inputs packed one after the other (8-byte aligned, as a batch's slab has them), every output on a
    // 16-byte boundary
    std::vector<uint64_t> xoff;
    const double *dx = ds.pack(in, n_in, n, &xoff);
    std::vector<AdpcmUtt> utts(n);
    std::vector<PcmShare> shares(n);
    uint64_t bytes = 0, groups = 0;
    for (size_t u = 0; u < n; u++) {
        AdpcmUtt &w = utts[u];
        w.n = n_in[u];
        w.g0 = groups;
        w.A = adpcm_block_align(hz[u], opts->block_align);
        w.spb = adpcm_spb(w.A);
        shares[u] = {bytes, adpcm_bytes(w.n, w.A)};
        bytes += (shares[u].n + 15) & ~(uint64_t)15;
        groups += (adpcm_blocks(w.n, w.A) + kAdpcmLanes - 1) / kAdpcmLanes;
    }
    uint8_t *dy = ds.alloc<uint8_t>(std::max<uint64_t>(bytes, 16));
    for (size_t u = 0; u < n; u++) {
        utts[u].x = dx + xoff[u];
        utts[u].y = dy + shares[u].off;
    }
    const AdpcmUtt *du = ds.upload(utts);
    if (ds.ok())
        ds.err = launch_adpcm(false, du, (uint32_t)n, groups, ds.stream);
    std::vector<uint8_t> host;
    ds.read_back(&host, dy, bytes);
    if ((rc = ds.status()))
        return rc;
    return hand_out(host.data(), 1, shares, (void **)out, n_bytes);
}

} // extern "C"

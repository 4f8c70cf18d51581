#pragma once
// jb_rfft_dev.h -- what the kernels of the packed real transform (jb_rfft.h) share and only a kernel can say: the
// radix-2 passes two to a barrier (k_fbank, k_fir_spectrum, k_fir_mac) and a filter's sum over the by-bin products
// (k_fbank, k_melspec).
#include "jb_rfft.h"

#include <hip/hip_runtime.h>

namespace jb {

// The log2(M) in-place radix-2 passes over points stored in bit-reversed order at their padded places (rfft_at), two to
// a barrier: a lane holds the four points {i, i + h, i + 2h, i + 3h} in registers and does the two butterflies of pass
// s and the two of pass s + 1 on them -- the arithmetic of the separate passes, operation for operation -- and a last
// single pass where log2(M) is odd.  twc, tws: W_M^p, p < M / 2 (every second entry of rfft_twiddles).  The lanes
// lane, lane + stride, ... share the frame; every lane of the workgroup calls (the barriers), and one that is not
// `live` touches nothing.  Ends behind a barrier
__device__ __forceinline__ void rfft_passes(double *re, double *im, const double *twc, const double *tws, uint32_t M,
                                            uint32_t log2m, uint32_t lane, uint32_t stride, bool live)
{
    uint32_t s = 0;
    for (; s + 1 < log2m; s += 2) { // passes s and s + 1
        __syncthreads();
        if (live) {
            const uint32_t h = 1u << s;
#pragma unroll 2
            for (uint32_t q = lane; q < M / 4; q += stride) {
                const uint32_t pos = q & (h - 1);
                const uint32_t i0 = ((q >> s) << (s + 2)) | pos;
                const uint32_t ia = rfft_at(i0), ib = rfft_at(i0 + h), ic = rfft_at(i0 + 2 * h), id = rfft_at(i0 + 3 * h);
                double ar = re[ia], ai = im[ia], br = re[ib], bi = im[ib];
                double cr = re[ic], ci = im[ic], dr = re[id], di = im[id];
                const uint32_t p0 = pos << (log2m - s - 1), p1 = pos << (log2m - s - 2), p2 = (pos + h) << (log2m - s - 2);
                rfft_bfly(ar, ai, br, bi, twc[p0], tws[p0]);
                rfft_bfly(cr, ci, dr, di, twc[p0], tws[p0]);
                rfft_bfly(ar, ai, cr, ci, twc[p1], tws[p1]);
                rfft_bfly(br, bi, dr, di, twc[p2], tws[p2]);
                re[ia] = ar, im[ia] = ai, re[ib] = br, im[ib] = bi;
                re[ic] = cr, im[ic] = ci, re[id] = dr, im[id] = di;
            }
        }
    }
    if (s < log2m) { // log2(M) is odd: the last pass alone, spans of M / 2 and twiddles W_M^j
        __syncthreads();
        if (live)
            for (uint32_t j = lane; j < M / 2; j += stride) {
                const uint32_t ia = rfft_at(j), ib = rfft_at(j + M / 2);
                rfft_bfly(re[ia], im[ia], re[ib], im[ib], twc[j], tws[j]);
            }
    }
    __syncthreads();
}

// A filter's sum once every bin's two products lie at the padded places: the rising ones in im[k0..k1), the falling
// ones in re[k1..k2), added in ascending order
__device__ __forceinline__ double mel_bank_sum(const double *re, const double *im, uint32_t k0, uint32_t k1, uint32_t k2)
{
    double e = 0.0;
#pragma unroll 4
    for (uint32_t k = k0; k < k1; k++)
        e += im[rfft_at(k)];
#pragma unroll 4
    for (uint32_t k = k1; k < k2; k++)
        e += re[rfft_at(k)];
    return e;
}

} // namespace jb

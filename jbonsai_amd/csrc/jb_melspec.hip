// jb_melspec.hip -- mel spectrograms on the device: the chain's final f64 PCM as [T][n_mels] frames, by the rule of
// jb_melspec.h.
//
//   k_melspec         a workgroup takes mel_wg_frames(n_fft) consecutive frames of one unit (workgroups never cross
//                     units), a frame mel_frame_lanes(n_fft) lanes: a wave up to n_fft 1024, two up to 2048, all four
//                     above, so that a workgroup holds at most kMelPoints complex points (33 KB of LDS in f64 with the
//                     pads) beside the 32 KB of the passes' twiddles W_M^p, p < M (the whole circle: a radix-5 pass
//                     asks for four fifths of it), staged once per workgroup: two workgroups to a CU.
//                     A frame's n_fft real samples are windowed on the way in -- predicated: the reflection is an index
//                     map (mel_sample_at), nothing outside the unit or the window is read -- and packed two to a
//                     complex point, stored at its digit-reversed place (a table: M entries).  The in-place passes of
//                     the factors 5, 3 and 2 of M follow, one to a barrier; a lane takes butterflies l, l + fl, ... of
//                     the pass's M / r and holds one butterfly's r points in registers (rfft_butterfly, the host's
//                     text); no two passes are fused.  Each lane then untangles pairs (k, M - k) into |X_k|^2 in place
//                     (rfft_power; the square root under JB_MEL_MAGNITUDE), every bin is multiplied by its weight in
//                     its rising and in its falling filter, and one lane per filter adds its products in ascending
//                     order, takes the logarithm and, without a range, the affine step and writes the element.  The
//                     spectrum never leaves LDS.
//                     LDS places: one pad double behind every 32 (rfft_at, as k_fbank).  The passes of 5 and 3 come
//                     first, where the span is odd: a half-wave's reads of one operand step by r doubles (pass 0) or
//                     by one double with a jump of (r - 1) L at a block's end: conflict-free but for those jumps.  The
//                     passes of 2 that follow have spans of a multiple of the odd part: consecutive lanes read
//                     consecutive doubles.  For a power of two the first pass steps by two doubles (two-way), the
//                     digit-reversed stores of the load are spread by the pad.
//                     Every operation of a frame is its own butterfly, pair, bin or filter: its order does not depend
//                     on the lanes that share the frame, on the frame's place in the workgroup or on the batch.
//   with range > 0    k_melspec writes the f64 values in front of the clamp to the unit's scratch and the largest of its
//                     workgroup to gmax[blockIdx] (a tree in LDS; a maximum has no order);
//   k_melspec_max     a workgroup per unit folds the unit's entries of gmax into umax[unit];
//   k_melspec_finish  the grid of k_melspec again: each workgroup streams its frames' elements through the clamp, the
//                     affine step and the element conversion.
// The launch list -- classes, units, g0 and the workgroup count that gmax is numbered by -- is RatePass's (jb_host.h),
// for jb_melspec_pcm_batch below (check, build, attach the pointers, launch, hand out) and for a batch's output chain.
#include "jb_host.h"
#include "jb_rfft_dev.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

// the frames of a workgroup at the padded places of rfft_at: 4 x (rfft_at(512) + 1), 2 x (rfft_at(1024) + 1) or
// rfft_at(2048) + 1 slots
constexpr uint32_t kMelSlots = 4 * (rfft_at(kMelPoints / 4) + 1) + 4;

__global__ __launch_bounds__(kMelLanes) void k_melspec(const MelClass *__restrict__ classes,
                                                       const MelUtt *__restrict__ utts, uint32_t n_utts,
                                                       double *__restrict__ gmax)
{
    // (a frame's arrays hold M + 1 values, the untangling leaves S_M in the last one, at the padded places of rfft_at)
    __shared__ double s_re[kMelSlots], s_im[kMelSlots];
    __shared__ double s_twc[kMelPoints], s_tws[kMelPoints];
    __shared__ double s_max[kMelLanes];
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x);
    const MelUtt U = utts[u];
    const MelClass &C = classes[U.cls];
    const uint32_t N = C.n_fft, M = N / 2;
    const uint32_t fl = mel_frame_lanes(N), nf = kMelLanes / fl;
    const uint32_t f = threadIdx.x / fl, l = threadIdx.x % fl;
    const uint64_t t = (blockIdx.x - U.g0) * (uint64_t)nf + f;
    const bool live = t < U.T; // (a workgroup's last frames may lie behind the unit's: they load, store and sum nothing)
    double *re = s_re + f * (rfft_at(M) + 1), *im = s_im + f * (rfft_at(M) + 1);
    const uint32_t pad = C.pad, wl = C.wl, woff = C.woff;
    const int64_t k0 = (int64_t)(t * C.hop) - (pad == kMelPadNone ? 0 : (int64_t)M);
    for (uint32_t p = threadIdx.x; p < M; p += kMelLanes) {
        s_twc[p] = C.twc[p];
        s_tws[p] = C.tws[p];
    }
    if (live)
        for (uint32_t j = l; j < M; j += fl) {
            double v[2];
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t i = 2 * j + h; // (i < n_fft; the window lies at [woff, woff + wl))
                const int64_t k = mel_sample_at(k0 + (int64_t)i, U.n, pad);
                const bool in = i >= woff && i < woff + wl && k >= 0;
                v[h] = in ? C.win[i - woff] * (U.x[k] * 0x1p-15) : 0.0;
            }
            const uint32_t r = rfft_at(C.rev[j]);
            re[r] = v[0];
            im[r] = v[1];
        }
    const uint32_t n_pass = C.n_pass;
    for (uint32_t s = 0; s < n_pass; s++) {
        __syncthreads();
        const uint32_t r = C.r[s], L = C.L[s], inv = C.inv[s];
        if (live)
            for (uint32_t j = l; j < M / r; j += fl)
                rfft_butterfly(re, im, s_twc, s_tws, M, r, L, inv, j, [](uint32_t i) { return rfft_at(i); });
    }
    __syncthreads();
    const bool magnitude = (C.flags & kMelMagnitude) != 0;
    if (live)
        for (uint32_t k = l; k <= M / 2; k += fl) { // rfft_untangle at the padded places
            const uint32_t kk = M - k, ik = rfft_at(k), iz = rfft_at(kk == M ? 0 : kk);
            const double ar = re[ik], ai = im[ik], zr = re[iz], zi = im[iz];
            const double p0 = rfft_power(ar, ai, zr, zi, C.tw[2 * k], C.tw[2 * k + 1]);
            re[ik] = magnitude ? sqrt(p0) : p0;
            if (kk != k) {
                const double p1 = rfft_power(zr, zi, ar, ai, C.tw[2 * kk], C.tw[2 * kk + 1]);
                re[rfft_at(kk)] = magnitude ? sqrt(p1) : p1;
            }
        }
    __syncthreads();
    // every bin's two products: rising into im, falling in place
    if (live)
        for (uint32_t k = l; k <= M; k += fl) {
            const double p = re[rfft_at(k)];
            im[rfft_at(k)] = C.wr[k] * p;
            re[rfft_at(k)] = C.wf[k] * p;
        }
    __syncthreads();
    const bool ranged = C.range > 0.0;
    double top = -HUGE_VAL;
    if (live) {
        const uint64_t row = t * C.n_mels;
        for (uint32_t m = l; m < C.n_mels; m += fl) {
            const uint32_t k0m = C.first[m], k1m = k0m + C.rise[m], k2m = k0m + C.count[m];
            const double e = mel_bank_sum(re, im, k0m, k1m, k2m);
            const double y = mel_log(e, C.log, C.floor, C.y_floor);
            if (ranged) {
                U.s[row + m] = y;
                top = y > top ? y : top;
            } else {
                const double v = mel_affine(y, C.offset, C.scale);
                if (C.flags & kMelF64)
                    ((double *)U.y)[row + m] = v;
                else
                    ((float *)U.y)[row + m] = (float)v;
            }
        }
    }
    if (!ranged) // (uniform over the workgroup)
        return;
    s_max[threadIdx.x] = top;
    for (uint32_t h = kMelLanes / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (threadIdx.x < h) {
            const double o = s_max[threadIdx.x + h];
            s_max[threadIdx.x] = o > s_max[threadIdx.x] ? o : s_max[threadIdx.x];
        }
    }
    if (threadIdx.x == 0)
        gmax[blockIdx.x] = s_max[0];
}

// Unit blockIdx.x: the largest of its workgroups' maxima (its entries of gmax follow one another from g0)
__global__ __launch_bounds__(kMelLanes) void k_melspec_max(const MelClass *__restrict__ classes,
                                                           const MelUtt *__restrict__ utts,
                                                           const double *__restrict__ gmax, double *__restrict__ umax)
{
    __shared__ double s_max[kMelLanes];
    const MelUtt U = utts[blockIdx.x];
    const uint32_t nf = mel_wg_frames(classes[U.cls].n_fft);
    const uint64_t groups = (U.T + nf - 1) / nf;
    double top = -HUGE_VAL;
    for (uint64_t g = threadIdx.x; g < groups; g += kMelLanes) {
        const double o = gmax[U.g0 + g];
        top = o > top ? o : top;
    }
    s_max[threadIdx.x] = top;
    for (uint32_t h = kMelLanes / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (threadIdx.x < h) {
            const double o = s_max[threadIdx.x + h];
            s_max[threadIdx.x] = o > s_max[threadIdx.x] ? o : s_max[threadIdx.x];
        }
    }
    if (threadIdx.x == 0)
        umax[blockIdx.x] = s_max[0];
}

// The grid of k_melspec: a workgroup's frames' elements from the scratch through the clamp, the affine step and the
// element conversion
__global__ __launch_bounds__(kMelLanes) void k_melspec_finish(const MelClass *__restrict__ classes,
                                                              const MelUtt *__restrict__ utts, uint32_t n_utts,
                                                              const double *__restrict__ umax)
{
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x);
    const MelUtt U = utts[u];
    const MelClass &C = classes[U.cls];
    const uint32_t nf = mel_wg_frames(C.n_fft);
    const uint64_t t0 = (blockIdx.x - U.g0) * (uint64_t)nf;
    const uint64_t t1 = t0 + nf < U.T ? t0 + nf : U.T;
    const double low = umax[u] - C.range, offset = C.offset, scale = C.scale;
    const bool f64 = (C.flags & kMelF64) != 0;
    for (uint64_t i = t0 * C.n_mels + threadIdx.x; i < t1 * C.n_mels; i += kMelLanes) {
        const double y = U.s[i];
        const double v = mel_affine(y > low ? y : low, offset, scale);
        if (f64)
            ((double *)U.y)[i] = v;
        else
            ((float *)U.y)[i] = (float)v;
    }
}

} // namespace

hipError_t launch_melspec(const MelClass *classes_dev, const MelUtt *utts_dev, uint32_t n, uint64_t groups, bool ranged,
                          double *gmax, double *umax, hipStream_t stream)
{
    if (n == 0 || groups == 0)
        return hipSuccess;
    if (groups > 0x7fffffffull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_melspec, dim3((uint32_t)groups), dim3(kMelLanes), 0, stream, classes_dev, utts_dev, n, gmax);
    if (ranged) {
        hipLaunchKernelGGL(k_melspec_max, dim3(n), dim3(kMelLanes), 0, stream, classes_dev, utts_dev, gmax, umax);
        hipLaunchKernelGGL(k_melspec_finish, dim3((uint32_t)groups), dim3(kMelLanes), 0, stream, classes_dev, utts_dev,
                           n, umax);
    }
    return hipGetLastError();
}

template <>
void MelClasses::bind(const MelOpts &opts, const double *dev, std::vector<double> *image,
                      std::vector<MelClass> *out) const
{
    TableImage img(dev);
    out->clear();
    for (size_t i = 0; i < tables.size(); i++) {
        const MelTables &t = tables[i];
        const MelGeom &g = geom[i];
        MelClass c{};
        c.win = img.put(t.win);
        c.tw = img.put(t.fft.tw);
        c.twc = img.put(t.fft.twc);
        c.tws = img.put(t.fft.tws);
        c.wr = img.put(t.bank.wr);
        c.wf = img.put(t.bank.wf);
        c.rev = img.put(t.fft.rev);
        c.first = img.put(t.bank.first);
        c.count = img.put(t.bank.count);
        c.rise = img.put(t.bank.rise);
        c.n_fft = g.n_fft;
        c.wl = g.wl;
        c.woff = g.woff;
        c.hop = g.hop;
        c.n_mels = g.n_mels;
        c.flags = opts.flags;
        c.pad = opts.pad;
        c.log = opts.log;
        c.n_pass = t.fft.sched.n;
        for (uint32_t s = 0; s < t.fft.sched.n; s++) {
            c.r[s] = t.fft.sched.r[s];
            c.L[s] = t.fft.sched.L[s];
            c.inv[s] = t.fft.sched.inv[s];
        }
        c.floor = g.floor;
        c.y_floor = g.y_floor;
        c.range = opts.range;
        c.offset = opts.offset;
        c.scale = g.scale;
        out->push_back(c);
    }
    *image = std::move(img.words);
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_melspec_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                         const jb_melspec_opts *opts, int32_t device, uint8_t **out, size_t *n_bytes)
{
    const MelOpts *o = (const MelOpts *)opts;
    int rc = mel_check_opts(o, "jb_melspec_pcm_batch");
    if (rc)
        return rc;
    if ((rc = pcm_check((const void *const *)in, n_in, n, hz && out && n_bytes, (void **)out, n_bytes)))
        return rc;
    // (every rate's geometry and every unit's frames before a device is touched: RatePass, jb_host.h)
    MelPass pass;
    pass.start(*o);
    for (size_t u = 0; u < n; u++)
        if ((rc = pass.add(hz[u], n_in[u], "jb_melspec_pcm_batch")))
            return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, "jb_melspec_pcm_batch")))
        return rc;
    // the inputs packed one after the other (8-byte aligned, as a batch's slab has them), every output on a
    // 16-byte boundary; with a range the f64 values in front of the clamp in a scratch of their own
    const bool ranged = o->range > 0.0;
    std::vector<uint64_t> xoff;
    const double *dx = ds.pack(in, n_in, n, &xoff);
    std::vector<PcmShare> shares(n);
    std::vector<uint64_t> soff(n);
    uint64_t bytes = 0, values = 0;
    for (size_t u = 0; u < n; u++) {
        const uint64_t elems = pass.list.host[u].T * o->n_mels;
        shares[u] = {bytes, elems * mel_elem(o->flags)};
        soff[u] = values;
        bytes += (shares[u].n + 15) & ~(uint64_t)15;
        values += elems;
    }
    uint8_t *dy = ds.alloc<uint8_t>(std::max<uint64_t>(bytes, 16));
    double *dsc = ranged ? ds.alloc<double>(values) : nullptr;
    double *gmax = ranged ? ds.alloc<double>(pass.groups) : nullptr;
    double *umax = ranged ? ds.alloc<double>(n) : nullptr;
    for (size_t u = 0; u < n; u++) {
        pass.list.host[u].x = dx + xoff[u];
        pass.list.host[u].y = dy + shares[u].off;
        pass.list.host[u].s = ranged ? dsc + soff[u] : nullptr;
    }
    pass.bind(ds, "jb_melspec_pcm_batch");
    if (ds.ok())
        ds.err = pass.launch(ds.stream, gmax, umax);
    std::vector<uint8_t> host;
    ds.read_back(&host, dy, bytes);
    if ((rc = ds.status()))
        return rc;
    return hand_out(host.data(), 1, shares, (void **)out, n_bytes);
}

} // extern "C"

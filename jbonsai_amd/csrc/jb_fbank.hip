// jb_fbank.hip -- log-mel filterbank features on the device: the chain's final f64 PCM as [T][n_mels] frames, by the
// rule of jb_fbank.h.
//
//   k_fbank   a workgroup takes fbank_wg_frames(n_fft) consecutive frames of one unit (workgroups never cross units),
//             a frame fbank_frame_lanes(n_fft) lanes: a wave up to n_fft 1024, two at 2048, all four at 4096, so that
//             a workgroup always holds at most kFbPoints complex points, 32 KB of LDS in f64, beside the 16 KB of the
//             passes' twiddles (W_M^p, p < M / 2: every second entry of the host's table), staged once per workgroup.
//             A frame's n_fft real samples are windowed on the way in (predicated: nothing outside the unit is read;
//             the zero tail beyond wl comes from the table's length) and packed two to a complex point, stored in
//             bit-reversed order.  The log2(M) in-place radix-2 passes then run two to a barrier: a lane holds the four
//             points {i, i + h, i + 2h, i + 3h} in registers and does the two butterflies of pass s and the two of
//             pass s + 1 on them -- the arithmetic of the separate passes, operation for operation -- and a last
//             single pass where log2(M) is odd.  Each lane then untangles the pairs (k, M - k) into |X_k|^2 in place
//             (its twiddles, read once, from global memory), every bin is multiplied by its weight in its rising and
//             in its falling filter (the by-bin tables: coalesced), and one lane per filter adds its products in
//             ascending order.  The spectrum never leaves LDS.  re and im are separate arrays: lanes that follow one
//             another read doubles that follow one another except in the first pair of passes (a stride of four
//             doubles: two-way on ds_read_b64's 64 banks).
//             With a frame request (k_fbank<true>; jb_fbank.h "Frame conditioning") the loader is load_conditioned:
//             DC removal, the frame's energy, pre-emphasis and the request's window in front of the same transform.
//             Every operation of a frame is its own butterfly, pair, bin or filter: its order does not depend on the
//             lanes that share the frame, on the frame's place in the workgroup or on the batch.
// The launch list -- classes, units, g0, the workgroup count and the choice of loader -- is RatePass's (jb_host.h), for
// the entries below and for a batch's output chain alike.
#include "jb_host.h"
#include "jb_rfft_dev.h"

#include <algorithm>
#include <map>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

// What a lane takes of its frame, at most: points to load (M / fl), pairs to untangle ((M / 2 + 1) / fl, rounded up) and
// bins to weigh ((M + 1) / fl, rounded up); fl is 64 up to M = 512, then M / 8
constexpr uint32_t kLoadIts = 8, kPairIts = 5, kBinIts = 9;

// the frames of a workgroup at the padded places of rfft_at: 4 x 529, 2 x 1057, 2113
constexpr uint32_t kFbSlots = 4 * (rfft_at(kFbPoints / 4) + 1) + 4;

// Value i < wl of a frame while it is conditioned: the frame's re area, then its im area (2 M >= wl values), at the
// padded places -- lanes that follow one another read doubles that follow one another, in the strided sums too
__device__ __forceinline__ double *frame_slot(double *re, double *im, uint32_t M, uint32_t i)
{
    return i < M ? re + rfft_at(i) : im + rfft_at(i - M);
}

// The sum of step 2 (frame_sum of jb_fbank.h) by the first 64 lanes of a frame, one wave: lane j adds f(i) over i = j
// mod 64 from 0.0 in ascending i, then p_j += p_{j + w} for w = 32, .., 1 across the wave (lanes from w on add what no
// one reads).  Lane 0 returns the sum
template <class F> __device__ __forceinline__ double frame_sum_wave(uint32_t wl, uint32_t lane, F f)
{
    double p = 0.0;
    for (uint32_t i0 = lane; i0 < wl; i0 += 4 * 64) { // (four reads in flight; the additions keep their order)
        double a[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; q++)
            a[q] = i0 + 64 * q < wl ? f(i0 + 64 * q) : 0.0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++)
            if (i0 + 64 * q < wl)
                p = p + a[q];
    }
#pragma unroll
    for (uint32_t w = 32; w; w >>= 1) {
        const double q = __shfl_down(p, w, 64);
        p = p + q;
    }
    return p;
}

// The conditioned loader (jb_fbank.h "Frame conditioning"): the frame's wl samples staged where its points will lie,
// every lane's v_i and v_{i-1} into registers while one wave forms the mean and the energy in the rule's order, the
// mean back through LDS, and only then, behind the second barrier, the windowed points in bit-reversed order.  Every
// lane of the workgroup calls (two barriers); one that is not `live` touches nothing
__device__ __forceinline__ void load_conditioned(const FbankClass &C, const FbankUtt &U, double *re, double *im,
                                                 uint32_t M, uint32_t log2m, uint32_t l, uint32_t fl, uint64_t t,
                                                 bool live, double scale)
{
    const bool reflect = (C.fr_flags & kFrReflect) != 0, dc = (C.fr_flags & kFrRemoveDc) != 0;
    const int64_t k0 = frame_start(t, C.wl, C.hop, (C.flags & kFbCenter) != 0, reflect);
    double v[2 * kLoadIts], wv[2 * kLoadIts];
    if (live) {
        // Every index first -- a reflected one takes a loop -- then a lane's loads all at once, as the plain loader's,
        // so that their latencies overlap.
        // A value that is not read counts as 0 and loads sample 0 (a live frame has n >= 1 in every mode), so that no
        // load waits behind a branch
        uint64_t kx[2 * kLoadIts];
        bool rd[2 * kLoadIts];
#pragma unroll
        for (uint32_t q = 0; q < 2 * kLoadIts; q++) {
            const uint32_t i = 2 * (l + (q / 2) * fl) + (q & 1);
            const int64_t k = k0 + (int64_t)i;
            rd[q] = i < C.wl && (reflect || (k >= 0 && (uint64_t)k < U.n)); // (wl <= n_fft: a staged i is below 2 M)
            kx[q] = rd[q] && !reflect ? (uint64_t)k : 0;
        }
        if (reflect) {
#pragma unroll
            for (uint32_t q = 0; q < 2 * kLoadIts; q++)
                if (rd[q])
                    kx[q] = frame_reflect(k0 + (int64_t)(2 * (l + (q / 2) * fl) + (q & 1)), U.n);
        }
#pragma unroll
        for (uint32_t q = 0; q < 2 * kLoadIts; q++) {
            const uint32_t i = 2 * (l + (q / 2) * fl) + (q & 1);
            v[q] = U.x[kx[q]];
            wv[q] = C.win[i < C.wl ? i : 0];
        }
#pragma unroll
        for (uint32_t q = 0; q < 2 * kLoadIts; q++) {
            const uint32_t i = 2 * (l + (q / 2) * fl) + (q & 1);
            v[q] = rd[q] ? v[q] * scale : 0.0;
            wv[q] = i < C.wl ? wv[q] : 0.0;
        }
#pragma unroll
        for (uint32_t it = 0; it < 2 * kLoadIts; it++) {
            const uint32_t i = 2 * (l + (it / 2) * fl) + (it & 1);
            if (i < C.wl)
                *frame_slot(re, im, M, i) = v[it];
        }
    }
    __syncthreads();
    // every lane's v_{i-1} (y_0 = v_0 - c v_0) into registers beside its own v_i, while the frame's first wave sums
    double pv[kLoadIts];
    if (live) {
#pragma unroll
        for (uint32_t it = 0; it < kLoadIts; it++) {
            const uint32_t i = 2 * (l + it * fl);
            pv[it] = i > 0 && i <= C.wl ? *frame_slot(re, im, M, i - 1) : v[2 * it];
        }
    }
    // (slot M of im is no point's and no staged value's: the mean's way back)
    if ((dc || U.e) && live && l < 64) {
        double mean = 0.0;
        if (dc) {
            const double s = frame_sum_wave(C.wl, l, [&](uint32_t i) { return *frame_slot(re, im, M, i); });
            mean = __shfl(s, 0, 64) / (double)C.wl;
        }
        if (U.e) {
            const double e = frame_sum_wave(C.wl, l, [&](uint32_t i) {
                const double a = *frame_slot(re, im, M, i), b = dc ? a - mean : a;
                return b * b;
            });
            if (l == 0)
                U.e[t] = e;
        }
        if (l == 0)
            im[rfft_at(M)] = mean;
    }
    __syncthreads();
    // (nothing reads the staged values from here on: the points take their places)
    if (live) {
        const double mean = dc ? im[rfft_at(M)] : 0.0, c = C.preemph;
#pragma unroll
        for (uint32_t it = 0; it < kLoadIts; it++) {
            const uint32_t i = 2 * (l + it * fl), j = l + it * fl;
            const double a = dc ? v[2 * it] - mean : v[2 * it], b = dc ? v[2 * it + 1] - mean : v[2 * it + 1];
            const double pa = dc ? pv[it] - mean : pv[it];
            const double ca = c * pa, cb = c * a;
            const double y0 = c > 0.0 ? a - ca : a, y1 = c > 0.0 ? b - cb : b;
            if (j < M) {
                const uint32_t r = __brev(j) >> (32 - log2m);
                re[rfft_at(r)] = i < C.wl ? wv[2 * it] * y0 : 0.0;
                im[rfft_at(r)] = i + 1 < C.wl ? wv[2 * it + 1] * y1 : 0.0;
            }
        }
    }
}

// FR: the classes carry a frame request (uniform over a launch); without it the loader is the plain one, untouched
template <bool FR>
__global__ __launch_bounds__(kFbLanes) void k_fbank(const FbankClass *__restrict__ classes,
                                                    const FbankUtt *__restrict__ utts, uint32_t n_utts)
{
    // (a frame's arrays hold M + 1 values, the untangling leaves P_M in the last one, at the padded places of rfft_at)
    __shared__ double s_re[kFbSlots], s_im[kFbSlots];
    __shared__ double s_twc[kFbPoints / 2], s_tws[kFbPoints / 2];
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x);
    const FbankUtt U = utts[u];
    const FbankClass C = classes[U.cls];
    const uint32_t M = C.n_fft / 2, log2m = C.log2m;
    const uint32_t fl = fbank_frame_lanes(C.n_fft), nf = kFbLanes / fl;
    const uint32_t f = threadIdx.x / fl, l = threadIdx.x % fl;
    const uint64_t t = (blockIdx.x - U.g0) * (uint64_t)nf + f;
    const bool live = t < U.T; // (a workgroup's last frames may lie behind the unit's: they load, store and sum nothing)
    double *re = s_re + f * (rfft_at(M) + 1), *im = s_im + f * (rfft_at(M) + 1);
    const bool center = (C.flags & kFbCenter) != 0;
    const double scale = (C.flags & kFbUnit) ? 0x1p-15 : 1.0;
    const int64_t k0 = (int64_t)(t * C.hop) - (center ? (int64_t)(C.wl / 2) : 0);
    for (uint32_t p = threadIdx.x; p < M / 2; p += kFbLanes) {
        s_twc[p] = C.tw[4 * p];
        s_tws[p] = C.tw[4 * p + 1];
    }
    // (a lane's loads all at once -- at most kLoadIts points of two samples each: M / fl is 8 from n_fft 1024 on --
    // so that their latencies overlap; what lies outside the window or the unit is not read and counts as 0)
    if (FR) {
        load_conditioned(C, U, re, im, M, log2m, l, fl, t, live, scale);
    } else if (live) {
        double xv[2 * kLoadIts], wv[2 * kLoadIts];
#pragma unroll
        for (uint32_t it = 0; it < kLoadIts; it++)
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t i = 2 * (l + it * fl) + h;
                const int64_t k = k0 + (int64_t)i;
                const bool in = i < C.wl && k >= 0 && (uint64_t)k < U.n; // (wl <= n_fft: i < 2 M)
                xv[2 * it + h] = in ? U.x[k] : 0.0;
                wv[2 * it + h] = in ? C.win[i] : 0.0;
            }
#pragma unroll
        for (uint32_t it = 0; it < kLoadIts; it++) {
            const uint32_t j = l + it * fl;
            if (j < M) {
                const uint32_t r = __brev(j) >> (32 - log2m);
                re[rfft_at(r)] = wv[2 * it] * (xv[2 * it] * scale);
                im[rfft_at(r)] = wv[2 * it + 1] * (xv[2 * it + 1] * scale);
            }
        }
    }
    rfft_passes(re, im, s_twc, s_tws, M, log2m, l, fl, live);
    // (the pairs' twiddles, then the bins' weights, loaded the same way: all of a lane's at once)
    if (live) {
        double tw[4 * kPairIts];
#pragma unroll
        for (uint32_t it = 0; it < kPairIts; it++) {
            const uint32_t k = l + it * fl, kc = k <= M / 2 ? k : 0;
            tw[4 * it] = C.tw[2 * kc], tw[4 * it + 1] = C.tw[2 * kc + 1];
            tw[4 * it + 2] = C.tw[2 * (M - kc)], tw[4 * it + 3] = C.tw[2 * (M - kc) + 1];
        }
#pragma unroll
        for (uint32_t it = 0; it < kPairIts; it++) {
            const uint32_t k = l + it * fl;
            if (k <= M / 2) { // rfft_untangle at the padded places
                const uint32_t kk = M - k, ik = rfft_at(k), iz = rfft_at(kk == M ? 0 : kk);
                const double ar = re[ik], ai = im[ik], zr = re[iz], zi = im[iz];
                re[ik] = rfft_power(ar, ai, zr, zi, tw[4 * it], tw[4 * it + 1]);
                if (kk != k)
                    re[rfft_at(kk)] = rfft_power(zr, zi, ar, ai, tw[4 * it + 2], tw[4 * it + 3]);
            }
        }
    }
    __syncthreads();
    // every bin's two products: rising into im, falling in place
    if (live) {
        double wr[kBinIts], wf[kBinIts];
#pragma unroll
        for (uint32_t it = 0; it < kBinIts; it++) {
            const uint32_t k = l + it * fl, kc = k <= M ? k : 0;
            wr[it] = C.wr[kc], wf[it] = C.wf[kc];
        }
#pragma unroll
        for (uint32_t it = 0; it < kBinIts; it++) {
            const uint32_t k = l + it * fl;
            if (k <= M) {
                const double p = re[rfft_at(k)];
                im[rfft_at(k)] = wr[it] * p;
                re[rfft_at(k)] = wf[it] * p;
            }
        }
    }
    __syncthreads();
    if (!live)
        return;
    uint8_t *row = U.y + t * C.n_mels * fbank_elem(C.flags);
    for (uint32_t m = l; m < C.n_mels; m += fl) {
        const uint32_t k0m = C.first[m], k1m = k0m + C.rise[m], k2m = k0m + C.count[m];
        const double e = mel_bank_sum(re, im, k0m, k1m, k2m);
        const double v = (C.flags & kFbLinear) ? e : e > C.log_floor ? log(e) : C.ln_floor;
        if (C.flags & kFbF64)
            ((double *)row)[m] = v;
        else
            ((float *)row)[m] = (float)v;
    }
}

} // namespace

hipError_t launch_fbank(const FbankClass *classes_dev, const FbankUtt *utts_dev, uint32_t n, uint64_t groups,
                        hipStream_t stream, bool framed)
{
    if (n == 0 || groups == 0)
        return hipSuccess;
    if (groups > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (framed)
        hipLaunchKernelGGL(k_fbank<true>, dim3((uint32_t)groups), dim3(kFbLanes), 0, stream, classes_dev, utts_dev, n);
    else
        hipLaunchKernelGGL(k_fbank<false>, dim3((uint32_t)groups), dim3(kFbLanes), 0, stream, classes_dev, utts_dev, n);
    return hipGetLastError();
}

template <>
void FbankClasses::bind(const FbankOpts &opts, const double *dev, std::vector<double> *image,
                        std::vector<FbankClass> *out) const
{
    TableImage img(dev);
    out->clear();
    for (size_t i = 0; i < tables.size(); i++) {
        const FbankTables &t = tables[i];
        const FbankGeom &g = geom[i];
        FbankClass c{};
        c.win = img.put(t.win);
        c.tw = img.put(t.fft.tw);
        c.wr = img.put(t.bank.wr);
        c.wf = img.put(t.bank.wf);
        c.first = img.put(t.bank.first);
        c.count = img.put(t.bank.count);
        c.rise = img.put(t.bank.rise);
        c.wl = g.wl;
        c.hop = g.hop;
        c.n_fft = g.n_fft;
        for (c.log2m = 0; (2u << c.log2m) < g.n_fft;)
            c.log2m++;
        c.n_mels = g.n_mels;
        c.flags = opts.flags;
        c.log_floor = g.log_floor;
        c.ln_floor = g.ln_floor;
        c.preemph = cond.preemph;
        c.fr_flags = cond.flags & (kFrRemoveDc | kFrReflect);
        out->push_back(c);
    }
    *image = std::move(img.words);
}

namespace {

// The seam's body: opts with the frame request fr (all zero: none), under the entry's name -- check, put the pass
// together (RatePass, jb_host.h), attach the units' pointers, launch, hand out
int fbank_pcm_run(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz, const FbankOpts *o,
                  const FrameOpts &fr, int32_t device, uint8_t **out, size_t *n_bytes, const char *who)
{
    int rc = pcm_check((const void *const *)in, n_in, n, hz && out && n_bytes, (void **)out, n_bytes);
    if (rc)
        return rc;
    // (every rate's geometry and every unit's frames before a device is touched)
    FbankPass pass;
    pass.start(*o, fr);
    for (size_t u = 0; u < n; u++)
        if ((rc = pass.add(hz[u], n_in[u], who)))
            return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    // the inputs packed one after the other (8-byte aligned, as a batch's slab has them), every output on a
    // 16-byte boundary
    std::vector<uint64_t> xoff;
    const double *dx = ds.pack(in, n_in, n, &xoff);
    std::vector<PcmShare> shares(n);
    uint64_t bytes = 0;
    for (size_t u = 0; u < n; u++) {
        shares[u] = {bytes, pass.list.host[u].T * o->n_mels * fbank_elem(o->flags)};
        bytes += (shares[u].n + 15) & ~(uint64_t)15;
    }
    uint8_t *dy = ds.alloc<uint8_t>(std::max<uint64_t>(bytes, 16));
    for (size_t u = 0; u < n; u++) {
        pass.list.host[u].x = dx + xoff[u];
        pass.list.host[u].y = dy + shares[u].off;
    }
    pass.bind(ds, who);
    if (ds.ok())
        ds.err = pass.launch(ds.stream);
    std::vector<uint8_t> host;
    ds.read_back(&host, dy, bytes);
    if ((rc = ds.status()))
        return rc;
    return hand_out(host.data(), 1, shares, (void **)out, n_bytes);
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_fbank_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                       const jb_fbank_opts *opts, int32_t device, uint8_t **out, size_t *n_bytes)
{
    const FbankOpts *o = (const FbankOpts *)opts;
    const int rc = fbank_check_opts(o, "jb_fbank_pcm_batch");
    return rc ? rc : fbank_pcm_run(in, n_in, n, hz, o, FrameOpts{}, device, out, n_bytes, "jb_fbank_pcm_batch");
}

int jb_fbank_framed_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                              const jb_fbank_opts *opts, const jb_frame_opts *fr, int32_t device, uint8_t **out,
                              size_t *n_bytes)
{
    const FbankOpts *o = (const FbankOpts *)opts;
    const int rc = frame_check(o, (const FrameOpts *)fr, false, "jb_fbank_framed_pcm_batch");
    return rc ? rc
              : fbank_pcm_run(in, n_in, n, hz, o, *(const FrameOpts *)fr, device, out, n_bytes,
                              "jb_fbank_framed_pcm_batch");
}

} // extern "C"

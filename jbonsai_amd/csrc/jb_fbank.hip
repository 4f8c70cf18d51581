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
//             Every operation of a frame is its own butterfly, pair, bin or filter: its order does not depend on the
//             lanes that share the frame, on the frame's place in the workgroup or on the batch.
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
    if (live) {
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
                        hipStream_t stream)
{
    if (n == 0 || groups == 0)
        return hipSuccess;
    if (groups > 0x7fffffffull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fbank, dim3((uint32_t)groups), dim3(kFbLanes), 0, stream, classes_dev, utts_dev, n);
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
        out->push_back(c);
    }
    *image = std::move(img.words);
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_fbank_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                       const jb_fbank_opts *opts, int32_t device, uint8_t **out, size_t *n_bytes)
{
    const FbankOpts *o = (const FbankOpts *)opts;
    int rc = fbank_check_opts(o, "jb_fbank_pcm_batch");
    if (rc)
        return rc;
    if ((rc = pcm_check((const void *const *)in, n_in, n, hz && out && n_bytes, (void **)out, n_bytes)))
        return rc;
    // (every rate's geometry before a device is touched)
    FbankClasses cls;
    std::vector<FbankUtt> utts(n);
    for (size_t u = 0; u < n; u++)
        if ((rc = cls.find(*o, hz[u], "jb_fbank_pcm_batch", &utts[u].cls)))
            return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, "jb_fbank_pcm_batch")))
        return rc;
    // the inputs packed one after the other (8-byte aligned, as a batch's slab has them), every output on a
    // 16-byte boundary
    std::vector<uint64_t> xoff;
    const double *dx = ds.pack(in, n_in, n, &xoff);
    std::vector<PcmShare> shares(n);
    const bool center = (o->flags & kFbCenter) != 0;
    uint64_t bytes = 0, groups = 0;
    for (size_t u = 0; u < n; u++) {
        FbankUtt &w = utts[u];
        const FbankGeom &g = cls.geom[w.cls];
        w.n = n_in[u];
        w.T = fbank_frames(w.n, g.wl, g.hop, center);
        w.g0 = groups;
        shares[u] = {bytes, w.T * g.n_mels * fbank_elem(o->flags)};
        bytes += (shares[u].n + 15) & ~(uint64_t)15;
        groups += (w.T + fbank_wg_frames(g.n_fft) - 1) / fbank_wg_frames(g.n_fft);
    }
    uint8_t *dy = ds.alloc<uint8_t>(std::max<uint64_t>(bytes, 16));
    for (size_t u = 0; u < n; u++) {
        utts[u].x = dx + xoff[u];
        utts[u].y = dy + shares[u].off;
    }
    double *dt = ds.alloc<double>(cls.words());
    std::vector<double> image;
    std::vector<FbankClass> classes;
    cls.bind(*o, dt, &image, &classes);
    if (ds.ok() && !image.empty())
        ds.err = hipMemcpyAsync(dt, image.data(), sizeof(double) * image.size(), hipMemcpyHostToDevice, ds.stream);
    const FbankClass *dc = ds.upload(classes);
    const FbankUtt *du = ds.upload(utts);
    if (ds.ok())
        ds.err = launch_fbank(dc, du, (uint32_t)n, groups, ds.stream);
    std::vector<uint8_t> host;
    ds.read_back(&host, dy, bytes);
    if ((rc = ds.status()))
        return rc;
    return hand_out(host.data(), 1, shares, (void **)out, n_bytes);
}

} // extern "C"

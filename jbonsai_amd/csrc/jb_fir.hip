// jb_fir.hip -- the convolution stage on the device (jb_fir.h): the f64 PCM at the output rate convolved with an
// impulse response, in front of the filter's sections.  Two modes, by the tap count alone:
//
//   k_fir_direct    K <= 256.  A workgroup takes kFirTile outputs of one utterance: its inputs with the K - 1 in front
//                   (shifted by the delay; what lies outside the utterance is never part of a sum) and the taps are
//                   staged in LDS, every lane sums its outputs by the host rule, term for term, and the workgroup
//                   stores the tile in whole aligned 16-byte stores.  A tile whose outputs all have their K terms
//                   inside the utterance: a lane takes 8 outputs that follow one another and keeps their 8 inputs of
//                   the present tap in registers, one new LDS read per tap (a pad double behind every 8: the lanes'
//                   stride of 9 doubles spreads over the banks); each output's sum still starts with h[0] x and fuses
//                   the taps in ascending order.  A tile at an edge of the utterance: fir_sample, one output at a
//                   time, the terms outside skipped.
//   k_fir_spectrum  K > 256, uniform partitioned overlap-save in f64.  Per (utterance, block j): the real transform of
//                   the n_fft samples that end at the end of block j, shifted by the delay (j from -lead: the delay's
//                   samples in front of block 0 are lead = ceil(d / Bk) blocks of their own), out-of-range samples
//                   predicated to zero, packed two to a complex point; k_fbank's pass structure and LDS padding
//                   (rfft_passes: two radix-2 passes to a barrier, re and im apart, a pad double behind every 32); the
//                   untangled Bk + 1 bins go to the spectrum scratch.
//   k_fir_mac       Per (utterance, block j): Y = sum over p of X[j - p] H[p], p ascending from 0 to min(P - 1, j + lead),
//                   every bin's sum in one lane; the untangling inverted, the inverse transform as the forward one of
//                   the conjugate (1 / M is in H), the last Bk samples kept: f64 in whole 16-byte stores, or the
//                   16-bit sink's rule.
// Blocks and tiles are counted from the utterance's own first sample, and every operation of a block is its own
// butterfly, pair or bin: a sample's bits depend on its utterance's samples, the taps, the delay and K only.
#include "jb_host.h"
#include "jb_rfft_dev.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

#define JB_FIR_GLOBAL __attribute__((address_space(1)))
typedef double FirD2 __attribute__((ext_vector_type(2)));
typedef int16_t FirS8 __attribute__((ext_vector_type(8)));

template <class T> struct FirVec;
template <> struct FirVec<double> {
    typedef FirD2 V;
};
template <> struct FirVec<int16_t> {
    typedef FirS8 V;
};

__device__ __forceinline__ void fir_out(double v, double *o) { *o = v; }
__device__ __forceinline__ void fir_out(double v, int16_t *o)
{
    *o = (int16_t)fmt_quant<false>(v, -32768.0, 32767.0, 0, 0);
}

constexpr uint32_t kFirSlots = rfft_at(kFirPoints) + 1; // a block at the padded places of rfft_at
constexpr uint32_t kFirLoadIts = kFirPoints / kFirLanes;              // points a lane loads, at most
constexpr uint32_t kFirPairIts = (kFirPoints / 2 + kFirLanes) / kFirLanes; // pairs (k, M - k), k <= M / 2, of a lane

// `len` values out of `src` (src(e): value e) to y[0 .. len): the elements in front of y's first 16-byte boundary one
// by one, whole aligned 16-byte groups behind them, the last partial group one by one (k_join's and the filter's form)
template <class T, class Src> __device__ __forceinline__ void fir_store(T *y, uint32_t len, uint32_t tid, Src src)
{
    typedef typename FirVec<T>::V V;
    constexpr uint32_t G = 16 / sizeof(T);
    JB_FIR_GLOBAL T *gy = (JB_FIR_GLOBAL T *)y;
    const uint32_t head = std::min<uint32_t>((uint32_t)((16u - ((uintptr_t)y & 15u)) & 15u) / (uint32_t)sizeof(T), len);
    if (tid < head) {
        T o;
        fir_out(src(tid), &o);
        gy[tid] = o;
    }
    for (uint32_t e0 = head + tid * G; e0 < len; e0 += kFirLanes * G) {
        if (e0 + G <= len) {
            V v;
#pragma unroll
            for (uint32_t q = 0; q < G; q++) {
                T o;
                fir_out(src(e0 + q), &o);
                v[q] = o;
            }
            *(JB_FIR_GLOBAL V *)(gy + e0) = v;
        } else {
            for (uint32_t e = e0; e < len; e++) {
                T o;
                fir_out(src(e), &o);
                gy[e] = o;
            }
        }
    }
}
template <class Src> __device__ __forceinline__ void fir_store_utt(const FirUtt &U, uint64_t start, uint32_t len, uint32_t tid, Src src)
{
    if (U.i16)
        fir_store<int16_t>((int16_t *)U.y + start, len, tid, src);
    else
        fir_store<double>((double *)U.y + start, len, tid, src);
}

// Where sample i of a direct tile lies in LDS: one pad double behind every 8
__host__ __device__ __forceinline__ constexpr uint32_t fir_pad(uint32_t i) { return i + (i >> 3); }
constexpr uint32_t kFirRun = kFirTile / kFirLanes; // outputs of a lane

__global__ __launch_bounds__(kFirLanes) void k_fir_direct(const FirClass *__restrict__ classes,
                                                          const FirUtt *__restrict__ utts, uint32_t n_utts)
{
    __shared__ double xs[fir_pad(kFirTile + kFirDirectMax)]; // the tile's inputs behind the K - 1 in front of them
    __shared__ double hs[kFirDirectMax];
    __shared__ double ys[fir_pad(kFirTile)];
    const uint32_t tid = threadIdx.x;
    const FirUtt U = utts[find_unit(utts, n_utts, blockIdx.x)];
    const uint64_t start = (blockIdx.x - U.g0) * (uint64_t)kFirTile;
    if (start >= U.n)
        return;
    const FirClass C = classes[U.cls];
    const uint32_t K = std::min<uint32_t>(C.K, kFirDirectMax + 0u), d = C.delay;
    const uint32_t len = (uint32_t)std::min<uint64_t>(kFirTile, U.n - start);
    const int64_t base = (int64_t)start + (int64_t)d - (int64_t)(K - 1); // the sample in xs[0]
    const uint32_t span = len + K - 1;
    for (uint32_t i = tid; i < span; i += kFirLanes) {
        const int64_t k = base + (int64_t)i;
        xs[fir_pad(i)] = k >= 0 && (uint64_t)k < U.n ? U.x[k] : 0.0;
    }
    for (uint32_t i = tid; i < K; i += kFirLanes)
        hs[i] = C.h[i];
    __syncthreads();
    if (len == kFirTile && base >= 0 && start + kFirTile - 1 + d < U.n) { // every term of every output is in range
        const uint32_t e0 = tid * kFirRun;
        double w[kFirRun], acc[kFirRun]; // w[c]: the sample under the present tap of output e0 + c
#pragma unroll
        for (uint32_t c = 0; c < kFirRun; c++)
            w[c] = xs[fir_pad(e0 + c + K - 1)];
        const double h0 = hs[0];
#pragma unroll
        for (uint32_t c = 0; c < kFirRun; c++)
            acc[c] = h0 * w[c];
#pragma unroll 8
        for (uint32_t k = 1; k < K; k++) {
#pragma unroll
            for (uint32_t c = kFirRun - 1; c > 0; c--)
                w[c] = w[c - 1];
            w[0] = xs[fir_pad(e0 + K - 1 - k)];
            const double hk = hs[k];
#pragma unroll
            for (uint32_t c = 0; c < kFirRun; c++)
                acc[c] = __builtin_fma(hk, w[c], acc[c]);
        }
#pragma unroll
        for (uint32_t c = 0; c < kFirRun; c++)
            ys[fir_pad(e0 + c)] = acc[c];
    } else {
        for (uint32_t e = tid; e < len; e += kFirLanes)
            ys[fir_pad(e)] = fir_sample(hs, K, d, U.n, start + e,
                                        [&](uint64_t k) { return xs[fir_pad((uint32_t)((int64_t)k - base))]; });
    }
    __syncthreads();
    fir_store_utt(U, start, len, tid, [&](uint32_t e) { return ys[fir_pad(e)]; });
}

// X_k of the real transform from the packed one (rfft_bin) as the spectrum scratch holds it
__device__ __forceinline__ FirD2 fir_untangle(double ar, double ai, double zr, double zi, double c, double sn)
{
    double xr, xi;
    rfft_bin(ar, ai, zr, zi, c, sn, &xr, &xi);
    FirD2 x;
    x[0] = xr;
    x[1] = xi;
    return x;
}
// The inverse: conj Z_k of the packed transform from a = Y_k and y = Y_(M - k)
__device__ __forceinline__ FirD2 fir_tangle(double ar, double ai, double yr, double yi, double c, double sn)
{
    const double br = yr, bi = -yi;
    const double fer = 0.5 * (ar + br), fei = 0.5 * (ai + bi);
    const double gr = 0.5 * (ar - br), gi = 0.5 * (ai - bi);
    const double fr = c * gr + sn * gi, fi = c * gi - sn * gr; // conj(w_k) G
    FirD2 z;
    z[0] = fer - fi;
    z[1] = -(fei + fr);
    return z;
}

__global__ __launch_bounds__(kFirLanes) void k_fir_spectrum(const FirClass *__restrict__ classes,
                                                            const FirUtt *__restrict__ utts, uint32_t n_utts,
                                                            double *__restrict__ spec)
{
    __shared__ double s_re[kFirSlots], s_im[kFirSlots];
    __shared__ double s_twc[kFirPoints / 2], s_tws[kFirPoints / 2];
    const uint32_t l = threadIdx.x;
    const FirUtt U = utts[find_unit(utts, n_utts, blockIdx.x, &FirUtt::f0)];
    const FirClass C = classes[U.cls];
    const uint32_t M = std::min<uint32_t>(C.n_fft / 2, kFirPoints + 0u), log2m = C.log2m, Bk = M;
    const uint64_t f = blockIdx.x - U.f0; // spectrum f is block j = f - lead
    if (f >= fir_frames(U.n, C.delay, Bk))
        return;
    for (uint32_t p = l; p < M / 2; p += kFirLanes) {
        s_twc[p] = C.tw[4 * p];
        s_tws[p] = C.tw[4 * p + 1];
    }
    // the window: samples (j - 1) Bk + d + i, i < n_fft; all of a lane's loads at once
    const int64_t k0 = ((int64_t)f - (int64_t)C.lead - 1) * (int64_t)Bk + (int64_t)C.delay;
    {
        double xv[2 * kFirLoadIts];
#pragma unroll
        for (uint32_t it = 0; it < kFirLoadIts; it++)
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t i = 2 * (l + it * kFirLanes) + h;
                const int64_t k = k0 + (int64_t)i;
                const bool in = i < 2 * M && k >= 0 && (uint64_t)k < U.n;
                xv[2 * it + h] = in ? U.x[k] : 0.0;
            }
#pragma unroll
        for (uint32_t it = 0; it < kFirLoadIts; it++) {
            const uint32_t q = l + it * kFirLanes;
            if (q < M) {
                const uint32_t r = __brev(q) >> (32 - log2m);
                s_re[rfft_at(r)] = xv[2 * it];
                s_im[rfft_at(r)] = xv[2 * it + 1];
            }
        }
    }
    rfft_passes(s_re, s_im, s_twc, s_tws, M, log2m, l, kFirLanes, true);
    JB_FIR_GLOBAL FirD2 *X = (JB_FIR_GLOBAL FirD2 *)spec + (U.s0 + f * (uint64_t)(M + 1));
#pragma unroll
    for (uint32_t it = 0; it < kFirPairIts; it++) {
        const uint32_t k = l + it * kFirLanes;
        if (k <= M / 2) {
            const uint32_t kk = M - k, ik = rfft_at(k), iz = rfft_at(kk == M ? 0 : kk);
            const double ar = s_re[ik], ai = s_im[ik], zr = s_re[iz], zi = s_im[iz];
            X[k] = fir_untangle(ar, ai, zr, zi, C.tw[2 * k], C.tw[2 * k + 1]);
            if (kk != k)
                X[kk] = fir_untangle(zr, zi, ar, ai, C.tw[2 * kk], C.tw[2 * kk + 1]);
        }
    }
}

__global__ __launch_bounds__(kFirLanes) void k_fir_mac(const FirClass *__restrict__ classes,
                                                       const FirUtt *__restrict__ utts, uint32_t n_utts,
                                                       const double *__restrict__ spec)
{
    __shared__ double s_re[kFirSlots], s_im[kFirSlots];
    __shared__ double s_twc[kFirPoints / 2], s_tws[kFirPoints / 2];
    const uint32_t l = threadIdx.x;
    const FirUtt U = utts[find_unit(utts, n_utts, blockIdx.x)];
    const FirClass C = classes[U.cls];
    const uint32_t M = std::min<uint32_t>(C.n_fft / 2, kFirPoints + 0u), log2m = C.log2m, Bk = M;
    const uint64_t j = blockIdx.x - U.g0;
    if (j >= fir_blocks(U.n, Bk))
        return;
    for (uint32_t p = l; p < M / 2; p += kFirLanes) {
        s_twc[p] = C.tw[4 * p];
        s_tws[p] = C.tw[4 * p + 1];
    }
    const uint32_t np = (uint32_t)std::min<uint64_t>(C.partitions - 1, j + C.lead) + 1;
    const JB_FIR_GLOBAL FirD2 *X0 = (const JB_FIR_GLOBAL FirD2 *)spec + (U.s0 + (j + C.lead) * (uint64_t)(M + 1));
    const JB_FIR_GLOBAL FirD2 *H0 = (const JB_FIR_GLOBAL FirD2 *)C.H;
    for (uint32_t it = 0; it < kFirPairIts; it++) {
        const uint32_t k = l + it * kFirLanes;
        if (k > M / 2)
            continue;
        const uint32_t kk = M - k;
        // Y_k and Y_(M - k): partition after partition, each sum in this lane alone
        double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
#pragma unroll 4
        for (uint32_t p = 0; p < np; p++) {
            const JB_FIR_GLOBAL FirD2 *X = X0 - (uint64_t)p * (M + 1), *H = H0 + (uint64_t)p * (M + 1);
            const FirD2 xa = X[k], ha = H[k], xb = X[kk], hb = H[kk];
            ar = __builtin_fma(-xa[1], ha[1], __builtin_fma(xa[0], ha[0], ar));
            ai = __builtin_fma(xa[1], ha[0], __builtin_fma(xa[0], ha[1], ai));
            br = __builtin_fma(-xb[1], hb[1], __builtin_fma(xb[0], hb[0], br));
            bi = __builtin_fma(xb[1], hb[0], __builtin_fma(xb[0], hb[1], bi));
        }
        const FirD2 zk = fir_tangle(ar, ai, br, bi, C.tw[2 * k], C.tw[2 * k + 1]);
        const uint32_t rk = __brev(k) >> (32 - log2m);
        s_re[rfft_at(rk)] = zk[0];
        s_im[rfft_at(rk)] = zk[1];
        if (kk != k && kk != M) {
            const FirD2 zz = fir_tangle(br, bi, ar, ai, C.tw[2 * kk], C.tw[2 * kk + 1]);
            const uint32_t rz = __brev(kk) >> (32 - log2m);
            s_re[rfft_at(rz)] = zz[0];
            s_im[rfft_at(rz)] = zz[1];
        }
    }
    rfft_passes(s_re, s_im, s_twc, s_tws, M, log2m, l, kFirLanes, true);
    // z = conj of what the passes left; samples Bk .. 2 Bk of the block's window are points M / 2 .. M
    const uint64_t start = j * (uint64_t)Bk;
    const uint32_t len = (uint32_t)std::min<uint64_t>(Bk, U.n - start);
    fir_store_utt(U, start, len, l, [&](uint32_t e) {
        const uint32_t q = rfft_at(M / 2 + (e >> 1));
        return (e & 1u) ? -s_im[q] : s_re[q];
    });
}

} // namespace

hipError_t launch_fir(const FirClass *classes_dev, const FirUtt *direct_dev, uint32_t n_direct, uint64_t tiles,
                      const FirUtt *part_dev, uint32_t n_part, uint64_t blocks, uint64_t frames, double *spec,
                      hipStream_t stream)
{
    if (tiles > 0x7fffffffull || blocks > 0x7fffffffull || frames > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (n_direct && tiles)
        hipLaunchKernelGGL(k_fir_direct, dim3((uint32_t)tiles), dim3(kFirLanes), 0, stream, classes_dev, direct_dev,
                           n_direct);
    if (n_part && blocks) {
        hipLaunchKernelGGL(k_fir_spectrum, dim3((uint32_t)frames), dim3(kFirLanes), 0, stream, classes_dev, part_dev,
                           n_part, spec);
        hipLaunchKernelGGL(k_fir_mac, dim3((uint32_t)blocks), dim3(kFirLanes), 0, stream, classes_dev, part_dev, n_part,
                           spec);
    }
    return hipGetLastError();
}

void fir_launch_lists(const std::vector<FirResponse> &resp, const std::vector<FirUtt> &utts,
                      const std::vector<uint8_t> &has, const std::vector<uint8_t> *only, FirLaunch *out)
{
    *out = FirLaunch{};
    for (size_t u = 0; u < utts.size(); u++) {
        if (!has[u] || (only && !(*only)[u]))
            continue;
        FirUtt w = utts[u];
        const FirGeom &g = resp[w.cls].g;
        if (g.mode == kFirDirect) {
            w.g0 = out->tiles;
            out->tiles += fir_blocks(w.n, kFirTile);
            out->direct.push_back(w);
        } else {
            w.g0 = out->blocks;
            w.f0 = out->frames;
            out->blocks += fir_blocks(w.n, g.block);
            out->frames += fir_frames(w.n, resp[w.cls].delay, g.block);
            out->part.push_back(w);
        }
    }
}

namespace {

// jb_fir_pcm_batch / _i16: the inputs packed one after the other on the device (as a batch's slab has them), the
// outputs the same way; an utterance without a response goes through the one-tap identity
template <class T>
int fir_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_fir *f, const uint32_t *hz,
                  int32_t device, T **out, size_t *n_out, const char *who)
{
    int rc = pcm_check((const void *const *)in, n_in, n, f && hz && out && n_out, (void **)out, n_out);
    if (rc)
        return rc;
    static const double one = 1.0;
    FirClasses cls;
    std::vector<FirUtt> utts(n);
    std::vector<uint8_t> has(n, 1);
    uint64_t bins = 0;
    for (size_t u = 0; u < n; u++) {
        if ((rc = fir_check(&f[u], hz[u], u, who)))
            return rc;
        const FirSpec id{&one, 1, hz[u], 0, 0};
        const uint32_t c = cls.find(f[u].taps ? *(const FirSpec *)&f[u] : id);
        utts[u] = {nullptr, nullptr, n_in[u], 0, 0, bins, c, sizeof(T) == 2};
        const FirGeom &g = cls.resp[c].g;
        if (g.mode == kFirPartitioned)
            bins += fir_frames(n_in[u], cls.resp[c].delay, g.block) * (g.block + 1);
    }
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    std::vector<uint64_t> off;
    const double *dx = ds.pack(in, n_in, n, &off);
    T *dy = ds.alloc<T>(off[n]);
    double *spec = ds.alloc<double>(2 * bins);
    for (size_t u = 0; u < n; u++) {
        utts[u].x = dx + off[u];
        utts[u].y = dy + off[u];
    }
    FirLaunch l;
    fir_launch_lists(cls.resp, utts, has, nullptr, &l);
    double *dt = ds.alloc<double>(cls.words());
    std::vector<double> image;
    std::vector<FirClass> classes;
    cls.bind(dt, &image, &classes);
    if (ds.ok() && !image.empty())
        ds.err = hipMemcpyAsync(dt, image.data(), sizeof(double) * image.size(), hipMemcpyHostToDevice, ds.stream);
    const FirClass *dc = ds.upload(classes);
    const FirUtt *dd = ds.upload(l.direct);
    const FirUtt *dp = ds.upload(l.part);
    if (ds.ok())
        ds.err = launch_fir(dc, dd, (uint32_t)l.direct.size(), l.tiles, dp, (uint32_t)l.part.size(), l.blocks, l.frames,
                            spec, ds.stream);
    std::vector<T> host;
    ds.read_back(&host, dy, off[n]);
    if ((rc = ds.status()))
        return rc;
    std::vector<PcmShare> shares(n);
    for (size_t u = 0; u < n; u++)
        shares[u] = {off[u], n_in[u]};
    return hand_out(host.data(), sizeof(T), shares, (void **)out, n_out);
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_fir_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_fir *f, const uint32_t *hz,
                     int32_t device, double **out, size_t *n_out)
{
    return fir_pcm_batch(in, n_in, n, f, hz, device, out, n_out, "jb_fir_pcm_batch");
}

int jb_fir_pcm_batch_i16(const double *const *in, const size_t *n_in, size_t n, const jb_fir *f, const uint32_t *hz,
                         int32_t device, int16_t **out, size_t *n_out)
{
    return fir_pcm_batch(in, n_in, n, f, hz, device, out, n_out, "jb_fir_pcm_batch_i16");
}

} // extern "C"

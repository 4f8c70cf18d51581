// jb_limiter.hip -- the limiter stage on the device (the rules: jb_limiter.h; the host half: jb_limiter.cpp), in the
// place of the loudness apply pass.  FIR only: a tile needs its samples and a halo, nothing from another workgroup.
//
//   k_ln_limit<T>     one workgroup per tile of 1,024 samples of one utterance (found by bisection over the list's tile
//                     prefix sums).  u = x g of the tile, L + H (+ 6) samples in front and L (+ 6) behind goes through
//                     LDS in 16-byte loads.  The detector (in true-peak mode the interpolated phases between every pair
//                     of samples, taps as scalar operands) and r follow; without a d > c in reach the workgroup streams
//                     u out (workgroup-uniform).  Otherwise the sliding minimum m by doubling in place in LDS (log2 of
//                     the window passes, then two overlapping power-of-two windows), the smoothing FMA chain where a
//                     wave's span holds an m < 1 (wave-uniform), the last minimum and the clamp.  The tile leaves in
//                     whole aligned 16-byte stores; its smallest a and its count of a < 1 go to the per-tile scratch.
//                     An utterance of the list without a limiter is the plain apply pass: y = x g.
//   k_ln_limit_fold   one wave per utterance of the list: its tiles' scratch into its result.
// No atomics, no spins, no scratch memory: a redo round needs nothing reset.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

typedef const __attribute__((address_space(4))) double cdouble;
#define JB_LIM_GLOBAL __attribute__((address_space(1)))
typedef double LimD2 __attribute__((ext_vector_type(2)));
typedef int16_t LimS8 __attribute__((ext_vector_type(8)));

template <class T> struct LimVec;
template <> struct LimVec<double> {
    typedef LimD2 V;
};
template <> struct LimVec<int16_t> {
    typedef LimS8 V;
};

constexpr uint32_t kLimR = kLimTile + kLimMaxSpan;     // r slots of a tile at most
constexpr uint32_t kLimU = kLimR + 2 * kLimTpHalo + 2; // u slots: the detector's halo, one for the 16-byte parity
constexpr uint32_t kLimPer = kLimR / kLimLanes;        // r slots per lane
constexpr uint32_t kLimOwn = kLimTile / kLimLanes;     // samples per lane
static_assert(kLimR % kLimLanes == 0 && kLimTile % kLimLanes == 0 && (kLimU * 8 + (kLimR + 1) * 8) < 60 * 1024,
              "the tile and its halo fit static LDS");

__device__ __forceinline__ void lim_put(double v, double *o) { *o = v; }
__device__ __forceinline__ void lim_put(double v, int16_t *o)
{
    *o = (int16_t)fmt_quant<false>(v, -32768.0, 32767.0, 0, 0);
}

// A tile of `len` values out of `src` (src(e): value e of the tile) to y[0 .. len): the elements in front of y's first
// 16-byte boundary one by one, whole aligned 16-byte groups behind them, the last partial group one by one
template <class T, class Src> __device__ __forceinline__ void lim_store_tile(T *y, uint32_t len, uint32_t tid, Src src)
{
    typedef typename LimVec<T>::V V;
    constexpr uint32_t G = 16 / sizeof(T);
    JB_LIM_GLOBAL T *gy = (JB_LIM_GLOBAL T *)y;
    const uint32_t head = std::min<uint32_t>((uint32_t)((16u - ((uintptr_t)y & 15u)) & 15u) / (uint32_t)sizeof(T), len);
    if (tid < head) {
        T o;
        lim_put(src(tid), &o);
        gy[tid] = o;
    }
#pragma unroll
    for (uint32_t i = 0; i < (kLimTile + kLimLanes * G - 1) / (kLimLanes * G); i++) {
        const uint32_t e0 = head + (i * kLimLanes + tid) * G;
        if (e0 + G <= len) {
            V v;
#pragma unroll
            for (uint32_t q = 0; q < G; q++) {
                T o;
                lim_put(src(e0 + q), &o);
                v[q] = o;
            }
            *(JB_LIM_GLOBAL V *)(gy + e0) = v;
        } else if (e0 < len) {
            for (uint32_t e = e0; e < len; e++) {
                T o;
                lim_put(src(e), &o);
                gy[e] = o;
            }
        }
    }
}

template <class T>
__global__ __launch_bounds__(kLimLanes) void k_ln_limit(const LimiterClass *__restrict__ classes,
                                                        const LimiterUtt *__restrict__ utts, uint32_t n_utts,
                                                        const LoudnessResult *__restrict__ res,
                                                        LimiterTile *__restrict__ tiles)
{
    __shared__ double us[kLimU];     // slot s: u of sample lo + s
    __shared__ double rs[kLimR + 1]; // b, then r, its windowed minima, m; at last the lanes' partial results
    __shared__ uint32_t cs[kLimLanes];
    const uint32_t tid = threadIdx.x;
    const LimiterUtt U = utts[find_unit(utts, n_utts, blockIdx.x, &LimiterUtt::t0)];
    const uint64_t t = blockIdx.x - U.t0;
    const uint64_t start = t * kLimTile;
    if (start >= U.n || !U.y)
        return;
    const uint32_t len = (uint32_t)std::min<uint64_t>(kLimTile, U.n - start);
    const double g = U.slot == kLimNoSlot ? U.g : res[U.slot].g;
    const JB_LIM_GLOBAL double *x = (const JB_LIM_GLOBAL double *)U.x;
    T *y = (T *)U.y + start;
    if (U.cls == kLimNoSlot) { // the plain apply pass
        lim_store_tile<T>(y, len, tid, [&](uint32_t e) { return x[start + e] * g; });
        if (tid == 0)
            tiles[U.s0 + t] = LimiterTile{1.0, 0};
        return;
    }
    const LimiterClass *K = classes + U.cls;
    const uint32_t L = K->L, H = K->H, F = K->F;
    const double c = U.c;
    const int64_t N = (int64_t)U.n;
    const uint32_t R = len + 2 * L + H; // r slot q: sample start - L - H + q
    const uint32_t S = R + 2 * kLimTpHalo;
    const int64_t base = (int64_t)start - (int64_t)(L + H + kLimTpHalo); // the first sample the tile needs
    const int64_t lo = base - (((int64_t)((uintptr_t)U.x >> 3) + base) & 1); // ... and a 16-byte boundary at or below
    const uint32_t o = (uint32_t)(base - lo);
    for (uint32_t p = tid; 2 * p < S + o; p += kLimLanes) {
        const int64_t i0 = lo + 2 * (int64_t)p;
        double v0, v1;
        if (i0 >= 0 && i0 + 1 < N) {
            const LimD2 v = *(const JB_LIM_GLOBAL LimD2 *)(x + i0);
            v0 = v[0];
            v1 = v[1];
        } else { // u = 0 outside [0, N)
            v0 = (i0 >= 0 && i0 < N) ? x[i0] : 0.0;
            v1 = (i0 + 1 >= 0 && i0 + 1 < N) ? x[i0 + 1] : 0.0;
        }
        us[2 * p] = v0 * g;
        us[2 * p + 1] = v1 * g;
    }
    __syncthreads();
    double *uu = us + o; // slot s: sample base + s
    if (F > 1) {
        // b slot j: between samples start - L - H - 1 + j and the next, of uu[j .. j + 12)
        cdouble *h = (cdouble *)K->tp;
        for (uint32_t j = tid; j <= R; j += kLimLanes) {
            double v[kLimTaps];
#pragma unroll
            for (uint32_t q = 0; q < kLimTaps; q++)
                v[q] = uu[j + q];
            rs[j] = lim_between(h, F, v);
        }
        __syncthreads();
    }
    double rv[kLimPer];
    bool over = false;
#pragma unroll
    for (uint32_t i = 0; i < kLimPer; i++) {
        const uint32_t q = tid + i * kLimLanes;
        rv[i] = 1.0;
        if (q < R) {
            const int64_t n = (int64_t)start - (int64_t)(L + H) + q;
            double d = fabs(uu[q + kLimTpHalo]);
            if (F > 1)
                d = fmax(d, fmax(rs[q], rs[q + 1]));
            if (n >= 0 && n < N) {
                rv[i] = lim_ratio(c, d);
                over = over || d > c;
            }
        }
    }
    const uint32_t own0 = L + H + kLimTpHalo; // uu slot of the tile's first sample
    if (!__syncthreads_or(over)) {            // nothing in reach: u as it is
        lim_store_tile<T>(y, len, tid, [&](uint32_t e) { return uu[own0 + e]; });
        if (tid == 0)
            tiles[U.s0 + t] = LimiterTile{1.0, 0};
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < kLimPer; i++) {
        const uint32_t q = tid + i * kLimLanes;
        if (q < R)
            rs[q] = rv[i];
    }
    __syncthreads();
    double r_own[kLimOwn], u_own[kLimOwn];
#pragma unroll
    for (uint32_t i = 0; i < kLimOwn; i++) {
        const uint32_t e = tid + i * kLimLanes;
        r_own[i] = e < len ? rs[e + L + H] : 1.0;
        u_own[i] = e < len ? uu[own0 + e] : 0.0;
    }
    // the sliding minimum over W = H + L + 1 slots: rs[q] = min r[q .. q + k) for k = 2, 4, .. <= W, in place (every
    // lane reads, all wait, every lane writes); past the end stands 1
    const uint32_t W = H + L + 1;
    uint32_t k = 1;
    for (; 2 * k <= W; k *= 2) {
#pragma unroll
        for (uint32_t i = 0; i < kLimPer; i++) {
            const uint32_t q = tid + i * kLimLanes;
            if (q < R)
                rv[i] = fmin(rs[q], q + k < R ? rs[q + k] : 1.0);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kLimPer; i++) {
            const uint32_t q = tid + i * kLimLanes;
            if (q < R)
                rs[q] = rv[i];
        }
        __syncthreads();
    }
    // m slot q: m[start - L + q] = min r[q .. q + W) = the two windows of k that cover it
#pragma unroll
    for (uint32_t i = 0; i < kLimPer; i++) {
        const uint32_t q = tid + i * kLimLanes;
        if (q < len + L)
            rv[i] = fmin(rs[q], q + W - k < R ? rs[q + W - k] : 1.0);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < kLimPer; i++) {
        const uint32_t q = tid + i * kLimLanes;
        if (q < len + L)
            rs[q] = rv[i];
    }
    __syncthreads();
    cdouble *w = (cdouble *)K->w;
    double min_a = 1.0;
    uint32_t count = 0;
#pragma unroll
    for (uint32_t i = 0; i < kLimOwn; i++) {
        const uint32_t e = tid + i * kLimLanes;
        // the wave's samples e read m slots [e0, e0 + 64 + L): is one of them below 1?
        const uint32_t e0 = e & ~63u, end = std::min<uint32_t>(e0 + 64 + L, len + L);
        bool below = false;
        for (uint32_t s = e0 + (tid & 63u); s < end; s += 64)
            below = below || rs[s] < 1.0;
        double a = 1.0;
        if (__any(below) && e < len)
            a = lim_smooth(w, L, [&](uint32_t j) { return rs[e + L - j]; });
        if (e < len) {
            a = lim_gain(a, r_own[i]);
            uu[own0 + e] = lim_out(u_own[i], a, c); // (its own slot; nothing reads u any more)
            min_a = fmin(min_a, a);
            count += a < 1.0;
        }
    }
    __syncthreads();
    rs[tid] = min_a;
    cs[tid] = count;
    __syncthreads();
    for (uint32_t s = kLimLanes / 2; s > 0; s >>= 1) {
        if (tid < s) {
            rs[tid] = fmin(rs[tid], rs[tid + s]);
            cs[tid] += cs[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0)
        tiles[U.s0 + t] = LimiterTile{rs[0], cs[0]};
    lim_store_tile<T>(y, len, tid, [&](uint32_t e) { return uu[own0 + e]; });
}

__global__ __launch_bounds__(64) void k_ln_limit_fold(const LimiterUtt *__restrict__ utts,
                                                      const LimiterTile *__restrict__ tiles,
                                                      LimiterResult *__restrict__ out)
{
    __shared__ double ms[64];
    __shared__ uint64_t ns[64];
    const uint32_t tid = threadIdx.x;
    const LimiterUtt U = utts[blockIdx.x];
    const uint64_t nt = limiter_tiles(U.n);
    double m = 1.0;
    uint64_t n = 0;
    for (uint64_t i = tid; i < nt; i += 64) {
        const LimiterTile v = tiles[U.s0 + i];
        m = fmin(m, v.min_a);
        n += v.count;
    }
    ms[tid] = m;
    ns[tid] = n;
    __syncthreads();
    for (uint32_t s = 32; s > 0; s >>= 1) {
        if (tid < s) {
            ms[tid] = fmin(ms[tid], ms[tid + s]);
            ns[tid] += ns[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0)
        out[U.rslot] = LimiterResult{ms[0], ns[0]};
}

} // namespace

hipError_t launch_limiter(const LimiterClass *classes_dev, const LimiterUtt *utts_dev, uint32_t n, uint64_t tiles,
                          const LoudnessResult *res, LimiterTile *scratch, LimiterResult *out, bool i16,
                          hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (tiles && i16)
        hipLaunchKernelGGL(k_ln_limit<int16_t>, dim3((uint32_t)tiles), dim3(kLimLanes), 0, stream, classes_dev,
                           utts_dev, n, res, scratch);
    else if (tiles)
        hipLaunchKernelGGL(k_ln_limit<double>, dim3((uint32_t)tiles), dim3(kLimLanes), 0, stream, classes_dev, utts_dev,
                           n, res, scratch);
    hipLaunchKernelGGL(k_ln_limit_fold, dim3(n), dim3(64), 0, stream, utts_dev, scratch, out);
    return hipGetLastError();
}

namespace {

// jb_limiter_pcm_batch / _i16: the inputs packed one after the other on the device (as a batch's slab has them), the
// outputs the same way
template <class T>
int limiter_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz, const double *gain,
                      const double *ceiling_db, const uint32_t *mode, const jb_limiter_opts *opts, int32_t device,
                      T **out, jb_limiter_report *reports, const char *who)
{
    int rc = pcm_check((const void *const *)in, n_in, n, hz && gain && ceiling_db && mode && opts && out,
                       (void **)out);
    if (rc)
        return rc;
    LimiterClasses classes;
    std::vector<LimiterUtt> utts(n);
    std::vector<uint32_t> Ls(n), Hs(n);
    uint64_t tiles = 0;
    for (size_t u = 0; u < n; u++) {
        if (mode[u] != JB_PEAK_SAMPLE && mode[u] != JB_PEAK_TRUE) {
            set_error(std::string(who) + ": a mode is JB_PEAK_SAMPLE or JB_PEAK_TRUE");
            return JB_ERR_INVALID;
        }
        LimOpts r{};
        uint32_t cls = kLimNoSlot;
        // (an utterance that is not limited has no geometry: its values are not read)
        if ((rc = limiter_check(&opts[u], u, who, &r)) ||
            (!(r.flags & kLimOff) && ((rc = limiter_geometry(r, hz[u], u, who, &Ls[u], &Hs[u])) ||
                                      (rc = classes.find(hz[u], Ls[u], Hs[u], mode[u], &cls)))))
            return rc;
        utts[u] = LimiterUtt{nullptr, nullptr,    n_in[u],    tiles, tiles, lim_ceiling(ceiling_db[u]),
                             gain[u], kLimNoSlot, cls,        (uint32_t)u, 0};
        tiles += limiter_tiles(n_in[u]);
    }
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    std::vector<uint64_t> off;
    const double *dx = ds.pack(in, n_in, n, &off);
    T *dy = ds.alloc<T>(off[n]);
    for (size_t u = 0; u < n; u++) {
        utts[u].x = dx + off[u];
        utts[u].y = dy + off[u];
    }
    const LimiterClass *dc = ds.upload(classes.tables);
    const LimiterUtt *du = ds.upload(utts);
    LimiterTile *dt = ds.alloc<LimiterTile>(tiles);
    LimiterResult *dr = ds.alloc<LimiterResult>(n);
    if (ds.ok())
        ds.err = launch_limiter(dc, du, (uint32_t)n, tiles, nullptr, dt, dr, sizeof(T) == 2, ds.stream);
    std::vector<T> host;
    std::vector<LimiterResult> results;
    ds.read_back(&host, dy, off[n]);
    ds.read_back(&results, dr, n);
    if ((rc = ds.status()))
        return rc;
    std::vector<PcmShare> shares(n);
    for (size_t u = 0; u < n; u++)
        shares[u] = {off[u], n_in[u]};
    if ((rc = hand_out(host.data(), sizeof(T), shares, (void **)out, nullptr)))
        return rc;
    for (size_t u = 0; reports && u < n; u++)
        reports[u] = jb_limiter_report{lim_reduction_db(results[u].min_a), results[u].count, Ls[u], Hs[u]};
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_limiter_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz, const double *gain,
                         const double *ceiling_dbfs, const uint32_t *peak_mode, const jb_limiter_opts *opts,
                         int32_t device, double **out, jb_limiter_report *reports)
{
    return limiter_pcm_batch(in, n_in, n, hz, gain, ceiling_dbfs, peak_mode, opts, device, out, reports,
                             "jb_limiter_pcm_batch");
}

int jb_limiter_pcm_batch_i16(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                             const double *gain, const double *ceiling_dbfs, const uint32_t *peak_mode,
                             const jb_limiter_opts *opts, int32_t device, int16_t **out, jb_limiter_report *reports)
{
    return limiter_pcm_batch(in, n_in, n, hz, gain, ceiling_dbfs, peak_mode, opts, device, out, reports,
                             "jb_limiter_pcm_batch_i16");
}

} // extern "C"

// jb_filter.hip -- the filter stage on the device: a cascade of up to four second-order sections (jb_filter.h) over the
// f64 PCM at the output rate, chunk-parallel and exact up to rounding, as the loudness K-weighting is measured
// (jb_loudness.hip): tiles are filtered from zero state, their states are carried by a scan of the affine maps
// s -> A^len s + e, and the tiles are filtered again from their true start states -- here the signal itself is kept.
// A tile is 256 segments of 16 samples, from the utterance's length alone.
//
//   k_filter_tiles<NS, false>  one workgroup per tile: the tile is staged through LDS (coalesced loads; lane l's
//                              segment at l * 17, an odd stride), every lane filters its segment from zero state, a
//                              Hillis-Steele scan over the lanes with the host-built A^(16 2^k) (wave-uniform, scalar
//                              operands) gives every segment's start state for a zero tile start, and the last active
//                              lane leaves the tile's zero-state end state
//   k_filter_scan<NS>          one wave per utterance: lane l folds the end states of its 2^j tiles (A^4096), a shuffle
//                              scan with A^(4096 2^(j + k)) carries the chunks, and every lane walks its chunk again and
//                              leaves each tile's true start state in place of its end state
//   k_filter_tiles<NS, true>   the same pass and scan from the tile's true start state; every lane filters its segment
//                              from its start state and writes y over x in LDS; the workgroup stores the tile in whole
//                              aligned 16-byte stores (f64, or the 16-bit sink's rule on the same y)
//   k_filter_copy              utterances without sections: a copy, or the 16-bit conversion alone
// NS is a template argument: state and the matrix-vector products live in registers.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

typedef const __attribute__((address_space(4))) double cdouble;
#define JB_FILT_GLOBAL __attribute__((address_space(1)))
typedef double FiltD2 __attribute__((ext_vector_type(2)));
typedef int16_t FiltS8 __attribute__((ext_vector_type(8)));

template <class T> struct FiltVec;
template <> struct FiltVec<double> {
    typedef FiltD2 V;
};
template <> struct FiltVec<int16_t> {
    typedef FiltS8 V;
};

__device__ __forceinline__ void filt_out(double v, double *o) { *o = v; }
__device__ __forceinline__ void filt_out(double v, int16_t *o)
{
    *o = (int16_t)fmt_quant<false>(v, -32768.0, 32767.0, 0, 0);
}

// v += P w (P wave-uniform: scalar operands)
template <uint32_t D> __device__ __forceinline__ void filt_mv_add(cdouble *P, const double *w, double *v)
{
#pragma unroll
    for (uint32_t i = 0; i < D; i++) {
        double acc = v[i];
#pragma unroll
        for (uint32_t k = 0; k < D; k++)
            acc = __builtin_fma(P[i * D + k], w[k], acc);
        v[i] = acc;
    }
}

// A tile of `len` values out of `src` (src(e): value e of the tile) to gy[0 .. len): the elements in front of gy's
// first 16-byte boundary one by one, whole aligned 16-byte groups behind them, the last partial group one by one
template <class T, class Src> __device__ __forceinline__ void filt_store_tile(T *y, uint32_t len, uint32_t tid, Src src)
{
    typedef typename FiltVec<T>::V V;
    constexpr uint32_t G = 16 / sizeof(T);
    JB_FILT_GLOBAL T *gy = (JB_FILT_GLOBAL T *)y;
    const uint32_t head = std::min<uint32_t>((uint32_t)((16u - ((uintptr_t)y & 15u)) & 15u) / (uint32_t)sizeof(T), len);
    if (tid < head) {
        T o;
        filt_out(src(tid), &o);
        gy[tid] = o;
    }
#pragma unroll
    for (uint32_t i = 0; i < kFiltTile / (kFiltLanes * G); i++) {
        const uint32_t e0 = head + (i * kFiltLanes + tid) * G;
        if (e0 + G <= len) {
            V v;
#pragma unroll
            for (uint32_t q = 0; q < G; q++) {
                T o;
                filt_out(src(e0 + q), &o);
                v[q] = o;
            }
            *(JB_FILT_GLOBAL V *)(gy + e0) = v;
        } else if (e0 < len) {
            for (uint32_t e = e0; e < len; e++) {
                T o;
                filt_out(src(e), &o);
                gy[e] = o;
            }
        }
    }
}

template <uint32_t NS, bool kOut, class T>
__global__ __launch_bounds__(kFiltLanes) void k_filter_tiles(const FilterClass *__restrict__ classes,
                                                             const FilterUtt *__restrict__ utts, uint32_t n_utts,
                                                             double *__restrict__ st)
{
    constexpr uint32_t D = 2 * NS, S = kFiltS, Sp = S | 1u;
    __shared__ double xs[kFiltLanes * Sp]; // lane l's segment at l * Sp: odd strides, no bank conflict
    __shared__ double sc[D * kFiltLanes];  // component i of lane l at i * 256 + l
    const uint32_t tid = threadIdx.x;
    const FilterUtt U = utts[find_unit(utts, n_utts, blockIdx.x, &FilterUtt::t0)];
    const uint64_t t = blockIdx.x - U.t0;
    const uint64_t start = t * kFiltTile;
    if (t >= U.ntiles || start >= U.n)
        return;
    const uint32_t len = (uint32_t)std::min<uint64_t>(kFiltTile, U.n - start);
    const FilterClass *R = classes + U.cls;
    const JB_FILT_GLOBAL double *x = (const JB_FILT_GLOBAL double *)U.x + start;
    // stage: element e to slot (e / S) * Sp + e % S.  All of a thread's loads are issued before the first store
    {
        double xv[S];
#pragma unroll
        for (uint32_t i = 0; i < S; i++) {
            const uint32_t e = tid + i * kFiltLanes;
            xv[i] = e < len ? x[e] : 0.0;
        }
#pragma unroll
        for (uint32_t i = 0; i < S; i++) {
            const uint32_t e = tid + i * kFiltLanes;
            xs[(e / S) * Sp + e % S] = xv[i];
        }
    }
    __syncthreads();
    double c[NS * kFiltCoefs];
#pragma unroll
    for (uint32_t i = 0; i < NS * kFiltCoefs; i++)
        c[i] = ((cdouble *)R->c)[i];
    const uint32_t seg0 = tid * S;
    const uint32_t sl = seg0 < len ? std::min(S, len - seg0) : 0u;
    double *xl = xs + tid * Sp;
    // every segment from zero state: its end state
    double v[D];
#pragma unroll
    for (uint32_t i = 0; i < D; i++)
        v[i] = 0.0;
    for (uint32_t i = 0; i < sl; i++)
        filt_step(c, v, xl[i], NS);
#pragma unroll
    for (uint32_t i = 0; i < D; i++)
        sc[i * kFiltLanes + tid] = v[i];
    __syncthreads();
    // inclusive scan of v_0 = tile start state, v_l = e_(l-1): s_l = sum_(m <= l) A^(S (l - m)) v_m
#pragma unroll
    for (uint32_t i = 0; i < D; i++) {
        double s0 = 0.0;
        if (kOut)
            s0 = st[(U.tile0 + t) * kFiltMaxD + i];
        v[i] = tid == 0 ? s0 : sc[i * kFiltLanes + tid - 1];
    }
    const uint32_t nact = (len + S - 1) / S;
    for (uint32_t kk = 0; (1u << kk) < nact; kk++) {
        const uint32_t d = 1u << kk;
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < D; i++)
            sc[i * kFiltLanes + tid] = v[i];
        __syncthreads();
        if (tid >= d) {
            double w[D];
#pragma unroll
            for (uint32_t i = 0; i < D; i++)
                w[i] = sc[i * kFiltLanes + tid - d];
            filt_mv_add<D>((cdouble *)R->P[kk], w, v);
        }
    }
    // v: the state at the start of this lane's segment
    if (!kOut) {
        if (tid == nact - 1) {
            for (uint32_t i = 0; i < sl; i++)
                filt_step(c, v, xl[i], NS);
#pragma unroll
            for (uint32_t i = 0; i < D; i++)
                st[(U.tile0 + t) * kFiltMaxD + i] = v[i];
        }
        return;
    }
    for (uint32_t i = 0; i < sl; i++)
        xl[i] = filt_step(c, v, xl[i], NS);
    __syncthreads();
    filt_store_tile<T>((T *)U.y + start, len, tid, [&](uint32_t e) { return xs[(e / S) * Sp + e % S]; });
}

// One wave per utterance: every tile gets its true start state (in place of its zero-state end state)
template <uint32_t NS>
__global__ __launch_bounds__(64) void k_filter_scan(const FilterClass *__restrict__ classes,
                                                    const FilterUtt *__restrict__ utts, double *__restrict__ st)
{
    constexpr uint32_t D = 2 * NS;
    const FilterUtt U = utts[blockIdx.x];
    const uint64_t nt = U.ntiles;
    uint32_t lc = 0; // a lane's chunk: 2^lc tiles
    while ((64ull << lc) < nt)
        lc++;
    if (nt == 0 || lc + 6 > kFiltTilePows)
        return;
    const FilterClass *R = classes + U.cls;
    const uint32_t lane = threadIdx.x;
    const uint64_t cl = 1ull << lc;
    const uint64_t t0 = std::min<uint64_t>(lane * cl, nt), t1 = std::min<uint64_t>(t0 + cl, nt);
    double *sb = st + U.tile0 * kFiltMaxD;
    cdouble *Pt = (cdouble *)R->Pt[0];
    // the chunk's end state from zero
    double F[D];
#pragma unroll
    for (uint32_t i = 0; i < D; i++)
        F[i] = 0.0;
    for (uint64_t t = t0; t < t1; t++) {
        double e[D];
#pragma unroll
        for (uint32_t i = 0; i < D; i++)
            e[i] = sb[t * kFiltMaxD + i];
        filt_mv_add<D>(Pt, F, e);
#pragma unroll
        for (uint32_t i = 0; i < D; i++)
            F[i] = e[i];
    }
    // inclusive scan across the lanes (a lane in front of a ragged or empty chunk has a full one), then each lane's
    // chunk start is its predecessor's value
    for (uint32_t j = 0; j < 6; j++) {
        const uint32_t d = 1u << j;
        double w[D];
#pragma unroll
        for (uint32_t i = 0; i < D; i++)
            w[i] = __shfl_up(F[i], d, 64);
        if (lane >= d)
            filt_mv_add<D>((cdouble *)R->Pt[lc + j], w, F);
    }
    double s[D];
#pragma unroll
    for (uint32_t i = 0; i < D; i++) {
        const double w = __shfl_up(F[i], 1, 64);
        s[i] = lane == 0 ? 0.0 : w;
    }
    for (uint64_t t = t0; t < t1; t++) {
        double e[D];
#pragma unroll
        for (uint32_t i = 0; i < D; i++) {
            e[i] = sb[t * kFiltMaxD + i];
            sb[t * kFiltMaxD + i] = s[i];
        }
        filt_mv_add<D>(Pt, s, e);
#pragma unroll
        for (uint32_t i = 0; i < D; i++)
            s[i] = e[i];
    }
}

template <class T>
__global__ __launch_bounds__(kFiltLanes) void k_filter_copy(const FilterUtt *__restrict__ utts, uint32_t n_utts)
{
    const FilterUtt U = utts[find_unit(utts, n_utts, blockIdx.x, &FilterUtt::t0)];
    const uint64_t t = blockIdx.x - U.t0;
    const uint64_t start = t * kFiltTile;
    if (t >= U.ntiles || start >= U.n)
        return;
    const uint32_t len = (uint32_t)std::min<uint64_t>(kFiltTile, U.n - start);
    const JB_FILT_GLOBAL double *x = (const JB_FILT_GLOBAL double *)U.x + start;
    filt_store_tile<T>((T *)U.y + start, len, threadIdx.x, [&](uint32_t e) { return x[e]; });
}

template <uint32_t NS>
void filter_launch_ns(const FilterClass *classes, const FilterUtt *utts, uint32_t n, uint32_t tiles, double *st, bool i16,
                      hipStream_t stream)
{
    hipLaunchKernelGGL((k_filter_tiles<NS, false, double>), dim3(tiles), dim3(kFiltLanes), 0, stream, classes, utts, n,
                       st);
    hipLaunchKernelGGL((k_filter_scan<NS>), dim3(n), dim3(64), 0, stream, classes, utts, st);
    if (i16)
        hipLaunchKernelGGL((k_filter_tiles<NS, true, int16_t>), dim3(tiles), dim3(kFiltLanes), 0, stream, classes, utts,
                           n, st);
    else
        hipLaunchKernelGGL((k_filter_tiles<NS, true, double>), dim3(tiles), dim3(kFiltLanes), 0, stream, classes, utts,
                           n, st);
}

} // namespace

hipError_t launch_filter(const FilterClass *classes_dev, const FilterUtt *utts_dev, const FilterLaunch &l, double *st,
                         bool i16, hipStream_t stream)
{
    uint32_t off = 0;
    for (uint32_t ns = 0; ns <= kFiltMaxSections; ns++) {
        const uint32_t n = l.count[ns];
        const FilterUtt *utts = utts_dev + off;
        off += n;
        if (n == 0 || l.tiles[ns] == 0)
            continue;
        if (l.tiles[ns] > 0x7fffffffull)
            return hipErrorInvalidValue;
        const uint32_t tiles = (uint32_t)l.tiles[ns];
        switch (ns) {
        case 0:
            if (i16)
                hipLaunchKernelGGL((k_filter_copy<int16_t>), dim3(tiles), dim3(kFiltLanes), 0, stream, utts, n);
            else
                hipLaunchKernelGGL((k_filter_copy<double>), dim3(tiles), dim3(kFiltLanes), 0, stream, utts, n);
            break;
        case 1:
            filter_launch_ns<1>(classes_dev, utts, n, tiles, st, i16, stream);
            break;
        case 2:
            filter_launch_ns<2>(classes_dev, utts, n, tiles, st, i16, stream);
            break;
        case 3:
            filter_launch_ns<3>(classes_dev, utts, n, tiles, st, i16, stream);
            break;
        default:
            filter_launch_ns<4>(classes_dev, utts, n, tiles, st, i16, stream);
            break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

namespace {

// jb_filter_pcm_batch / _i16: the inputs packed one after the other on the device (as a batch's slab has them), the
// outputs the same way
template <class T>
int filter_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_filter *f, const uint32_t *hz,
                     int32_t device, T **out, size_t *n_out, const char *who)
{
    int rc = pcm_check((const void *const *)in, n_in, n, f && hz && out && n_out, (void **)out, n_out);
    if (rc)
        return rc;
    std::vector<FilterClass> classes;
    std::vector<uint32_t> cls_of;
    if ((rc = filter_classes(f, n, hz, n, &classes, &cls_of, who)))
        return rc;
    std::vector<FilterUtt> utts(n);
    uint64_t tiles = 0;
    for (size_t u = 0; u < n; u++) {
        if (filter_tiles(n_in[u]) > kFiltMaxTiles) {
            set_error(std::string(who) + ": utterance " + std::to_string(u) + " is too long");
            return JB_ERR_UNSUPPORTED;
        }
        utts[u] = {nullptr, nullptr, n_in[u], tiles, 0, (uint32_t)filter_tiles(n_in[u]), cls_of[u]};
        tiles += utts[u].ntiles;
    }
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    std::vector<uint64_t> off;
    const double *dx = ds.pack(in, n_in, n, &off);
    T *dy = ds.alloc<T>(off[n]);
    double *st = ds.alloc<double>(tiles * kFiltMaxD);
    for (size_t u = 0; u < n; u++) {
        utts[u].x = dx + off[u];
        utts[u].y = dy + off[u];
    }
    FilterLaunch l;
    if ((rc = filter_launch_list(classes, utts, nullptr, &l)))
        return rc;
    const FilterClass *dc = ds.upload(classes);
    const FilterUtt *du = ds.upload(l.utts);
    if (ds.ok())
        ds.err = launch_filter(dc, du, l, st, sizeof(T) == 2, ds.stream);
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

int jb_filter_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_filter *f, const uint32_t *hz,
                        int32_t device, double **out, size_t *n_out)
{
    return filter_pcm_batch(in, n_in, n, f, hz, device, out, n_out, "jb_filter_pcm_batch");
}

int jb_filter_pcm_batch_i16(const double *const *in, const size_t *n_in, size_t n, const jb_filter *f,
                            const uint32_t *hz, int32_t device, int16_t **out, size_t *n_out)
{
    return filter_pcm_batch(in, n_in, n, f, hz, device, out, n_out, "jb_filter_pcm_batch_i16");
}

} // extern "C"

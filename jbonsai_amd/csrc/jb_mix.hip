// jb_mix.hip -- the mix stage on the device: the chain's final PCM, f64 or 16-bit, summed into programmes (each member
// at its start, under its fades and its gain) by the rules of jb_mix.h.
//
//   k_mix<T, kFit>   one workgroup per tile of kProgTileBytes of one programme (every programme starts on a 16-byte
//               boundary of its slab and is listed whole).  A lane takes groups of 16 destination bytes -- 2 f64 or 8
//               16-bit samples -- and stores each as one dwordx4.  A group inside one segment loads each covering
//               member's samples in one load at whatever alignment they have (as k_join does; nothing in front of a
//               member's first sample or behind its last one is read), with the fade weights and the gain only where
//               they reach, and adds in list order, so the work per sample follows the depth at that sample.  A group
//               under one member at 0 dB outside its fades is a plain copy; a group of silence is zeros; a group across
//               a segment boundary and a programme's last partial group go sample by sample.  The tile's first and
//               last segment are found once per workgroup (uniform), so a lane bisects only in tiles that hold a
//               boundary.  Each wave leaves the maximum of |acc| over its samples: a wave reduction and one store,
//               no LDS, no atomics (a maximum does not depend on the order).  kFit: the second pass of JB_MIX_FIT --
//               the workgroups of a programme with s == 1 leave at once, the others form the sums again from the
//               members and store fmin(fmax(acc s, -c), c) through the sink.
//   k_mix_peak  one wave per programme: the maximum of its tiles' maxima, and the scale.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

typedef double MixD2 __attribute__((ext_vector_type(2)));
typedef double MixD2u __attribute__((ext_vector_type(2), aligned(8)));
typedef int16_t MixS8 __attribute__((ext_vector_type(8)));
typedef int16_t MixS8u __attribute__((ext_vector_type(8), aligned(2)));
// (a pointer read from the work list is generic to the compiler: named global, the accesses are global_ ones)
#define JB_MIX_GLOBAL __attribute__((address_space(1)))

template <class T> struct MixVec;
template <> struct MixVec<double> {
    typedef MixD2 V;
    typedef MixD2u U;
};
template <> struct MixVec<int16_t> {
    typedef MixS8 V;
    typedef MixS8u U;
};

__device__ __forceinline__ uint32_t mix_span_of(const ProgSpan *spans, uint32_t n, uint64_t idx)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (spans[mid].t0 <= idx)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double mix_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// the sum at sample k of the programme whose segments are segs[lo .. hi]
template <class T>
__device__ __forceinline__ double mix_value(const MixSeg *segs, uint32_t lo, uint32_t hi, const ProgMember *members,
                                            const uint32_t *lists, uint64_t k)
{
    const MixSeg g = segs[mix_find(segs, lo, hi, k)];
    return mix_acc<T>(members, lists + g.l0, g.nl, k);
}

template <class T, bool kFit>
__global__ __launch_bounds__(kProgLanes) void k_mix(const ProgSpan *__restrict__ spans, uint32_t n_spans,
                                                   const ProgMember *__restrict__ members,
                                                   const MixSeg *__restrict__ segs_all,
                                                   const uint32_t *__restrict__ lists, double *__restrict__ tile_peak,
                                                   const MixResult *__restrict__ res, double c)
{
    constexpr uint32_t G = kProgGroupBytes / sizeof(T);
    constexpr uint32_t kTile = kProgTileBytes / sizeof(T);
    static_assert(kTile % (kProgLanes * G) == 0, "a tile is whole groups of every lane");
    typedef typename MixVec<T>::V V;
    typedef typename MixVec<T>::U U;
    const ProgSpan S = spans[mix_span_of(spans, n_spans, blockIdx.x)];
    double s = 1.0;
    if (kFit) {
        s = res[S.prog].scale;
        if (s == 1.0)
            return;
    }
    const uint64_t tile = blockIdx.x - S.t0;
    const uint64_t k0 = tile * (uint64_t)kTile;
    if (k0 >= S.n)
        return;
    const uint64_t k1 = std::min<uint64_t>(k0 + kTile, S.n);
    const MixSeg *segs = segs_all + S.s0;
    // the segments of the tile's first and last sample (uniform): a lane's search stays between them
    const uint32_t slo = mix_find(segs, 0, S.ns - 1, k0);
    const uint32_t shi = mix_find(segs, slo, S.ns - 1, k1 - 1);
    JB_MIX_GLOBAL T *gy = (JB_MIX_GLOBAL T *)S.y;
    double pk = 0.0;
    // one finished sum on its way out: the peak in the first pass, the fit in the second, then the sink
    auto out = [&](double acc) {
        if (!kFit)
            pk = fmax(pk, fabs(acc));
        T o;
        mix_store(kFit ? mix_fit(acc, s, c) : acc, &o);
        return o;
    };
#pragma unroll
    for (uint32_t i = 0; i < kTile / (kProgLanes * G); i++) {
        const uint64_t ks = k0 + (uint64_t)(i * kProgLanes + threadIdx.x) * G;
        if (ks + G <= k1) {
            const MixSeg g = segs[mix_find(segs, slo, shi, ks)];
            V v = (V)(T)0;
            if (ks + G <= g.k1 && g.nl == 0) {
                // silence: zeros (the fit of +0.0 is +0.0)
            } else if (ks + G <= g.k1) {
                // inside one segment: every listed member holds the whole group
                const uint32_t *list = lists + g.l0;
                double acc[G];
                bool copied = false;
                for (uint32_t j = 0; j < g.nl; j++) {
                    const ProgMember m = members[list[j]];
                    const uint64_t ka = ks - m.start;
                    const V x = *(const JB_MIX_GLOBAL U *)((const JB_MIX_GLOBAL T *)m.x + ka);
                    const bool plain = join_plain(ka, ka + G - 1, m.n, m.fade_in, m.fade_out);
                    if (!kFit && g.nl == 1 && plain && m.g == 1.0) {
                        // one member at 0 dB outside its fades: a plain copy
                        v = x;
#pragma unroll
                        for (uint32_t q = 0; q < G; q++)
                            pk = fmax(pk, fabs((double)x[q]));
                        copied = true;
                        break;
                    }
#pragma unroll
                    for (uint32_t q = 0; q < G; q++) {
                        double t = (double)x[q];
                        if (!plain)
                            t = join_sample(t, ka + q, m.n, m.fade_in, m.fade_out);
                        if (m.g != 1.0)
                            t = t * m.g;
                        acc[q] = j ? acc[q] + t : t;
                    }
                }
                if (!copied) {
#pragma unroll
                    for (uint32_t q = 0; q < G; q++)
                        v[q] = out(acc[q]);
                }
            } else {
                // across a segment boundary
#pragma unroll
                for (uint32_t q = 0; q < G; q++)
                    v[q] = out(mix_value<T>(segs, slo, shi, members, lists, ks + q));
            }
            *(JB_MIX_GLOBAL V *)(gy + ks) = v;
        } else if (ks < k1) {
            // the programme's last partial group
            for (uint64_t k = ks; k < k1; k++)
                gy[k] = out(mix_value<T>(segs, slo, shi, members, lists, k));
        }
    }
    if (!kFit) {
        pk = mix_wave_max(pk);
        if ((threadIdx.x & 63u) == 0)
            tile_peak[(S.pk0 + tile) * kMixWaves + (threadIdx.x >> 6)] = pk;
    }
}

// One wave per programme of the list: M over its tiles' maxima (tile_samples: kProgTileBytes in samples), and s
__global__ __launch_bounds__(64) void k_mix_peak(const ProgSpan *__restrict__ spans, uint32_t tile_samples,
                                                 const double *__restrict__ tile_peak, MixResult *__restrict__ res,
                                                 bool fit, double c)
{
    const ProgSpan S = spans[blockIdx.x];
    const uint64_t slots = (S.n + tile_samples - 1) / tile_samples * kMixWaves;
    const double *pk = tile_peak + S.pk0 * kMixWaves;
    double m = 0.0;
    for (uint64_t i = threadIdx.x; i < slots; i += 64)
        m = fmax(m, pk[i]);
    m = mix_wave_max(m);
    if (threadIdx.x == 0)
        res[S.prog] = MixResult{m, fit ? mix_scale(m, c) : 1.0};
}

template <class T>
void mix_launch(const ProgSpan *spans_dev, uint32_t n, uint64_t tiles, const MixLaunch &L, hipStream_t stream)
{
    if (tiles)
        hipLaunchKernelGGL((k_mix<T, false>), dim3((uint32_t)tiles), dim3(kProgLanes), 0, stream, spans_dev, n, L.members,
                           L.segs, L.lists, L.tile_peak, (const MixResult *)L.res, L.ceiling);
    hipLaunchKernelGGL(k_mix_peak, dim3(n), dim3(64), 0, stream, spans_dev, (uint32_t)(kProgTileBytes / sizeof(T)),
                       (const double *)L.tile_peak, L.res, L.fit, L.ceiling);
    if (tiles && L.fit)
        hipLaunchKernelGGL((k_mix<T, true>), dim3((uint32_t)tiles), dim3(kProgLanes), 0, stream, spans_dev, n, L.members,
                           L.segs, L.lists, L.tile_peak, (const MixResult *)L.res, L.ceiling);
}

} // namespace

hipError_t launch_mix(bool i16, const ProgSpan *spans_dev, uint32_t n, uint64_t tiles, const MixLaunch &L,
                      hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (i16)
        mix_launch<int16_t>(spans_dev, n, tiles, L, stream);
    else
        mix_launch<double>(spans_dev, n, tiles, L, stream);
    return hipGetLastError();
}

namespace {

// jb_join_pcm_batch, jb_mix_pcm_batch and their _i16 forms: the inputs packed one after the other on the device (as a
// batch's slab has them), the programmes of the geometry each on a 16-byte boundary.  `chained`: request is a join's
// (jb_join_utt[n]; else jb_mix_utt[n]), without options and reports, and the launch is the join's
template <class T>
int programme_pcm_batch(const T *const *in, const size_t *n_in, size_t n, const void *request, bool chained,
                        const MixOpts *opts, int32_t device, T **out, size_t *n_out, size_t *n_programmes,
                        jb_mix_report *reports, const char *who)
{
    if (n_programmes)
        *n_programmes = 0;
    int rc = pcm_check((const void *const *)in, n_in, n, request && out && n_out, (void **)out, n_out);
    if (rc)
        return rc;
    const std::vector<MixUtt> as_mix = chained ? join_as_mix((const JoinUtt *)request, n) : std::vector<MixUtt>();
    const MixUtt *req = chained ? as_mix.data() : (const MixUtt *)request;
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    if ((rc = mix_layout_checked(req, chained, ns.data(), nullptr, n, sizeof(T), opts, &lay, who)))
        return rc;
    const size_t P = lay.units.size();
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    std::vector<uint64_t> xoff;
    const T *dx = ds.pack(in, n_in, n, &xoff);
    T *dy = ds.alloc<T>(lay.total);
    std::vector<ProgMember> members;
    std::vector<ProgSpan> spans;
    uint64_t tiles = 0;
    mix_lists(lay, req, ns.data(), xoff.data(), dx, dy, sizeof(T), &members, &spans, &tiles);
    MixLaunch L{};
    L.members = ds.upload(members);
    if (!chained) { // (the join's kernel reads the members alone)
        L.segs = ds.upload(lay.segs);
        L.lists = ds.upload(lay.lists);
        L.tile_peak = ds.alloc<double>(tiles * kMixWaves);
        L.res = ds.alloc<MixResult>(P);
        L.fit = opts && (opts->flags & kMixFit);
        L.ceiling = L.fit ? mix_ceiling(opts->ceiling_db) : 0.0;
    }
    const ProgSpan *dsp = ds.upload(spans);
    if (ds.ok())
        ds.err = chained ? launch_join(sizeof(T) == 2, dsp, (uint32_t)P, tiles, L.members, ds.stream)
                         : launch_mix(sizeof(T) == 2, dsp, (uint32_t)P, tiles, L, ds.stream);
    std::vector<T> host;
    std::vector<MixResult> res;
    ds.read_back(&host, dy, lay.total);
    if (!chained)
        ds.read_back(&res, (const MixResult *)L.res, P);
    if ((rc = ds.status()))
        return rc;
    std::vector<PcmShare> shares(P);
    for (size_t p = 0; p < P; p++)
        shares[p] = {lay.units[p].off, lay.units[p].n};
    if ((rc = hand_out(host.data(), sizeof(T), shares, (void **)out, n_out)))
        return rc;
    for (size_t p = 0; reports && !chained && p < P; p++)
        reports[p] = {res[p].peak, res[p].scale, lay.depth[p], 0, lay.overlap[p]};
    if (n_programmes)
        *n_programmes = P;
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_join_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_join_utt *req, int32_t device,
                      double **out, size_t *n_out, size_t *n_programmes)
{
    return programme_pcm_batch(in, n_in, n, req, true, nullptr, device, out, n_out, n_programmes, nullptr,
                               "jb_join_pcm_batch");
}

int jb_join_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_join_utt *req,
                          int32_t device, int16_t **out, size_t *n_out, size_t *n_programmes)
{
    return programme_pcm_batch(in, n_in, n, req, true, nullptr, device, out, n_out, n_programmes, nullptr,
                               "jb_join_pcm_batch_i16");
}

int jb_mix_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                     const jb_mix_opts *opts, int32_t device, double **out, size_t *n_out, size_t *n_programmes,
                     jb_mix_report *reports)
{
    return programme_pcm_batch(in, n_in, n, req, false, (const MixOpts *)opts, device, out, n_out, n_programmes, reports,
                               "jb_mix_pcm_batch");
}

int jb_mix_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                         const jb_mix_opts *opts, int32_t device, int16_t **out, size_t *n_out, size_t *n_programmes,
                         jb_mix_report *reports)
{
    return programme_pcm_batch(in, n_in, n, req, false, (const MixOpts *)opts, device, out, n_out, n_programmes, reports,
                               "jb_mix_pcm_batch_i16");
}

} // extern "C"

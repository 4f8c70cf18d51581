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
//               kStem (a template parameter, as k_fbank's frame loader: the plain mix compiles from the code it had):
//               the fit pass of the stems (jb_mix.h "Stems"), units behind the programmes with segments over their own
//               members.  Their first pass is the plain one; in the fit pass a stem reads the scale of its PARENT
//               programme's slot, stores acc * s without the clamp, and its blocks are counted behind the programmes'
//               tiles (tile0).  A stem's own peak goes to the stem's slot.
//   k_mix_peak  one wave per programme: the maximum of its tiles' maxima, and the scale (a stem: its peak alone).
//   k_mix_levels<T>  one workgroup of 256 lanes per tile of 1,024 samples in programme coordinates of one level item
//               (a stem against its programme over the tiles of its extent, or a programme over all of its tiles), of
//               the units as stored.  Lane l forms partial l of sum a a and of sum a m by the rule of jb_mix.h
//               (level_partial: the first product, then fma), coalesced; the tree runs in the rule's order, h = 128
//               and 64 through LDS, h = 32 .. 1 by lane shifts; lane 0 stores the tile's two sums as one 16-byte
//               store.  No atomics, nothing whose order the scheduling sets.
//   k_mix_levels_fold  one wave per item: the tile sums loaded 64 at a time and added in ascending order by lane 0.
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

template <class T, bool kFit, bool kStem = false>
__global__ __launch_bounds__(kProgLanes) void k_mix(const ProgSpan *__restrict__ spans, uint32_t n_spans,
                                                   const ProgMember *__restrict__ members,
                                                   const MixSeg *__restrict__ segs_all,
                                                   const uint32_t *__restrict__ lists, double *__restrict__ tile_peak,
                                                   const MixResult *__restrict__ res, double c, uint32_t tile0)
{
    static_assert(kFit || !kStem, "a stem's first pass is the plain one");
    const uint32_t block = kStem ? blockIdx.x + tile0 : blockIdx.x; // (the stems' tiles follow the programmes')
    constexpr uint32_t G = kProgGroupBytes / sizeof(T);
    constexpr uint32_t kTile = kProgTileBytes / sizeof(T);
    static_assert(kTile % (kProgLanes * G) == 0, "a tile is whole groups of every lane");
    typedef typename MixVec<T>::V V;
    typedef typename MixVec<T>::U U;
    const ProgSpan S = spans[mix_span_of(spans, n_spans, block)];
    double s = 1.0;
    if (kFit) {
        s = res[kStem ? S.parent : S.prog].scale;
        if (s == 1.0)
            return;
    }
    const uint64_t tile = block - S.t0;
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
        mix_store(kFit ? (kStem ? mix_stem_fit(acc, s) : mix_fit(acc, s, c)) : acc, &o);
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
        res[S.prog] = MixResult{m, fit && S.parent == S.prog ? mix_scale(m, c) : 1.0}; // (a stem has no scale)
}

template <class T>
__global__ __launch_bounds__(kLevelLanes) void k_mix_levels(const LevelItem *__restrict__ items, uint32_t n_items,
                                                           double *__restrict__ tile_sums)
{
    __shared__ double s_e[kLevelLanes], s_d[kLevelLanes];
    uint32_t lo = 0, hi = n_items;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (items[mid].t0 <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    const LevelItem I = items[lo];
    const uint64_t j = blockIdx.x - I.t0;
    if (j >= I.nt) // (uniform)
        return;
    const uint64_t i = I.tile0 + j;
    const uint32_t l = threadIdx.x;
    const JB_MIX_GLOBAL T *ga = (const JB_MIX_GLOBAL T *)I.a;
    const JB_MIX_GLOBAL T *gm = (const JB_MIX_GLOBAL T *)I.m;
    // (every sample read lies below I.n, the length of both units)
    double pe = level_partial(I.n, i, l, [&](uint64_t k, double *x, double *y) { *x = *y = (double)ga[k]; });
    double pd = pe;
    if (!I.self)
        pd = level_partial(I.n, i, l, [&](uint64_t k, double *x, double *y) {
            *x = (double)ga[k];
            *y = (double)gm[k];
        });
    // the tree: p[l] = p[l] + p[l + h], h = 128, 64 through LDS ...
    s_e[l] = pe;
    s_d[l] = pd;
    __syncthreads();
    if (l < 128) {
        pe = pe + s_e[l + 128];
        pd = pd + s_d[l + 128];
    }
    __syncthreads();
    if (l < 128) {
        s_e[l] = pe;
        s_d[l] = pd;
    }
    __syncthreads();
    if (l >= 64)
        return;
    pe = pe + s_e[l + 64];
    pd = pd + s_d[l + 64];
    // ... and h = 32 .. 1 inside the first wave: lane l adds lane l + h's (what the lanes at and above h make is not read)
#pragma unroll
    for (uint32_t h = 32; h; h >>= 1) {
        pe = pe + __shfl_down(pe, h, 64);
        pd = pd + __shfl_down(pd, h, 64);
    }
    if (l == 0)
        *(JB_MIX_GLOBAL MixD2 *)((JB_MIX_GLOBAL double *)tile_sums + 2 * (I.s0 + j)) = MixD2{pe, pd};
}

__global__ __launch_bounds__(kLevelWave) void k_mix_levels_fold(const LevelItem *__restrict__ items, uint32_t n_items,
                                                               const double *__restrict__ tile_sums,
                                                               MixSums *__restrict__ sums)
{
    __shared__ MixD2 s_t[kLevelWave];
    if (blockIdx.x >= n_items)
        return;
    const LevelItem I = items[blockIdx.x];
    const uint32_t l = threadIdx.x;
    const JB_MIX_GLOBAL MixD2 *gs = (const JB_MIX_GLOBAL MixD2 *)tile_sums + I.s0;
    double E = 0.0, D = 0.0;
    for (uint64_t c = 0; c < I.nt; c += kLevelWave) {
        __syncthreads();
        if (c + l < I.nt)
            s_t[l] = gs[c + l];
        __syncthreads();
        if (l == 0) {
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(kLevelWave, I.nt - c);
            for (uint32_t k = 0; k < cnt; k++) {
                const MixD2 v = s_t[k];
                E = c == 0 && k == 0 ? v[0] : E + v[0];
                D = c == 0 && k == 0 ? v[1] : D + v[1];
            }
        }
    }
    if (l == 0)
        sums[I.unit] = MixSums{E, D};
}

template <class T>
void mix_launch(const ProgSpan *spans_dev, uint32_t n, uint64_t tiles, const MixLaunch &L, hipStream_t stream)
{
    // (the first pass takes programmes and stems alike: a stem is the mix rule over its own segments)
    if (tiles)
        hipLaunchKernelGGL((k_mix<T, false>), dim3((uint32_t)tiles), dim3(kProgLanes), 0, stream, spans_dev, n, L.members,
                           L.segs, L.lists, L.tile_peak, (const MixResult *)L.res, L.ceiling, 0u);
    hipLaunchKernelGGL(k_mix_peak, dim3(n), dim3(64), 0, stream, spans_dev, (uint32_t)(kProgTileBytes / sizeof(T)),
                       (const double *)L.tile_peak, L.res, L.fit, L.ceiling);
    const uint64_t ptiles = tiles - L.stem_tiles; // the programmes' tiles stand in front
    if (ptiles && L.fit)
        hipLaunchKernelGGL((k_mix<T, true>), dim3((uint32_t)ptiles), dim3(kProgLanes), 0, stream, spans_dev, n - L.stems,
                           L.members, L.segs, L.lists, L.tile_peak, (const MixResult *)L.res, L.ceiling, 0u);
    if (L.stem_tiles && L.fit)
        hipLaunchKernelGGL((k_mix<T, true, true>), dim3((uint32_t)L.stem_tiles), dim3(kProgLanes), 0, stream, spans_dev, n,
                           L.members, L.segs, L.lists, L.tile_peak, (const MixResult *)L.res, L.ceiling,
                           (uint32_t)ptiles);
}

} // namespace

hipError_t launch_mix(bool i16, const ProgSpan *spans_dev, uint32_t n, uint64_t tiles, const MixLaunch &L,
                      hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull || L.stems > n || L.stem_tiles > tiles)
        return hipErrorInvalidValue;
    if (i16)
        mix_launch<int16_t>(spans_dev, n, tiles, L, stream);
    else
        mix_launch<double>(spans_dev, n, tiles, L, stream);
    return hipGetLastError();
}

hipError_t launch_mix_levels(bool i16, const LevelItem *items_dev, uint32_t n, uint64_t tiles, double *tile_sums,
                             MixSums *sums, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (tiles && i16)
        hipLaunchKernelGGL(k_mix_levels<int16_t>, dim3((uint32_t)tiles), dim3(kLevelLanes), 0, stream, items_dev, n,
                           tile_sums);
    else if (tiles)
        hipLaunchKernelGGL(k_mix_levels<double>, dim3((uint32_t)tiles), dim3(kLevelLanes), 0, stream, items_dev, n,
                           tile_sums);
    hipLaunchKernelGGL(k_mix_levels_fold, dim3(n), dim3(kLevelWave), 0, stream, items_dev, n,
                       (const double *)tile_sums, sums);
    return hipGetLastError();
}

namespace {

// jb_join_pcm_batch, jb_mix_pcm_batch and their _i16 forms: the inputs packed one after the other on the device (as a
// batch's slab has them), the programmes of the geometry each on a 16-byte boundary.  `chained`: request is a join's
// (jb_join_utt[n]; else jb_mix_utt[n]), without options and reports, and the launch is the join's.  stems (a mix's
// alone): the stems request; out and n_out then have 2 n entries, the P + S units (*n_units), and stem_reports [n]
struct StemsCall {
    const uint32_t *stem_of;
    uint32_t flags;
    size_t *n_units;
    jb_stem_report *reports;
};
template <class T>
int programme_pcm_batch(const T *const *in, const size_t *n_in, size_t n, const void *request, bool chained,
                        const MixOpts *opts, int32_t device, T **out, size_t *n_out, size_t *n_programmes,
                        jb_mix_report *reports, const char *who, const StemsCall *stems = nullptr)
{
    if (n_programmes)
        *n_programmes = 0;
    if (stems && stems->n_units)
        *stems->n_units = 0;
    int rc = pcm_check((const void *const *)in, n_in, n, request && out && n_out && (!stems || stems->stem_of),
                       (void **)out, n_out);
    if (rc)
        return rc;
    for (size_t u = n; stems && u < 2 * n; u++) {
        out[u] = nullptr;
        n_out[u] = 0;
    }
    if (stems && (stems->flags & ~kMixStemLevels)) {
        set_error(std::string(who) + ": flags holds an unknown flag");
        return JB_ERR_INVALID;
    }
    const std::vector<MixUtt> as_mix = chained ? join_as_mix((const JoinUtt *)request, n) : std::vector<MixUtt>();
    const MixUtt *req = chained ? as_mix.data() : (const MixUtt *)request;
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    if ((rc = mix_layout_checked(req, chained, ns.data(), nullptr, n, sizeof(T), opts, &lay, who,
                                 stems ? stems->stem_of : nullptr)))
        return rc;
    const size_t P = lay.programmes(), U = lay.units.size();
    const bool levels = stems && (stems->flags & kMixStemLevels);
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
        L.res = ds.alloc<MixResult>(U);
        L.fit = opts && (opts->flags & kMixFit);
        L.ceiling = L.fit ? mix_ceiling(opts->ceiling_db) : 0.0;
        L.stems = (uint32_t)(U - P);
        for (size_t p = P; p < U; p++)
            L.stem_tiles += prog_tiles(0, spans[p].n, sizeof(T) == 2);
    }
    const ProgSpan *dsp = ds.upload(spans);
    if (ds.ok())
        ds.err = chained ? launch_join(sizeof(T) == 2, dsp, (uint32_t)P, tiles, L.members, ds.stream)
                         : launch_mix(sizeof(T) == 2, dsp, (uint32_t)U, tiles, L, ds.stream);
    // the levels behind the fit, of the units as stored
    MixSums *dsums = nullptr;
    if (levels) {
        std::vector<LevelItem> items;
        uint64_t ltiles = 0, scratch = 0;
        mix_level_items(lay, dy, sizeof(T), {}, &items, &ltiles, &scratch);
        double *tsums = ds.alloc<double>(2 * scratch);
        dsums = ds.alloc<MixSums>(U);
        const LevelItem *di = ds.upload(items);
        if (ds.ok())
            ds.err = launch_mix_levels(sizeof(T) == 2, di, (uint32_t)items.size(), ltiles, tsums, dsums, ds.stream);
    }
    std::vector<T> host;
    std::vector<MixResult> res;
    std::vector<MixSums> sums;
    ds.read_back(&host, dy, lay.total);
    if (!chained)
        ds.read_back(&res, (const MixResult *)L.res, U);
    if (levels)
        ds.read_back(&sums, (const MixSums *)dsums, U);
    if ((rc = ds.status()))
        return rc;
    std::vector<PcmShare> shares(U);
    for (size_t p = 0; p < U; p++)
        shares[p] = {lay.units[p].off, lay.units[p].n};
    if ((rc = hand_out(host.data(), sizeof(T), shares, (void **)out, n_out)))
        return rc;
    for (size_t p = 0; reports && !chained && p < P; p++)
        reports[p] = {res[p].peak, res[p].scale, lay.depth[p], 0, lay.overlap[p]};
    for (size_t p = P; stems && stems->reports && p < U; p++)
        stems->reports[p - P] = stem_report_of(res[p].peak, res[lay.stems[p - P].programme].scale, levels,
                                               levels ? sums[p] : MixSums{}, levels ? sums[lay.stems[p - P].programme].e : 0.0);
    if (n_programmes)
        *n_programmes = P;
    if (stems && stems->n_units)
        *stems->n_units = U;
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

int jb_mix_stems_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                           const uint32_t *stem_of, uint32_t flags, const jb_mix_opts *opts, int32_t device,
                           double **out, size_t *n_out, size_t *n_programmes, size_t *n_units, jb_mix_report *reports,
                           jb_stem_report *stem_reports)
{
    const StemsCall st{stem_of, flags, n_units, stem_reports};
    return programme_pcm_batch(in, n_in, n, req, false, (const MixOpts *)opts, device, out, n_out, n_programmes, reports,
                               "jb_mix_stems_pcm_batch", &st);
}

int jb_mix_stems_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                               const uint32_t *stem_of, uint32_t flags, const jb_mix_opts *opts, int32_t device,
                               int16_t **out, size_t *n_out, size_t *n_programmes, size_t *n_units,
                               jb_mix_report *reports, jb_stem_report *stem_reports)
{
    const StemsCall st{stem_of, flags, n_units, stem_reports};
    return programme_pcm_batch(in, n_in, n, req, false, (const MixOpts *)opts, device, out, n_out, n_programmes, reports,
                               "jb_mix_stems_pcm_batch_i16", &st);
}

} // extern "C"

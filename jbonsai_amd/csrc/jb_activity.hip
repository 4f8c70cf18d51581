// jb_activity.hip -- the speech-activity stage on the device: per-frame 0/1 labels of every column of every unit by the
// rules of jb_activity.h.
//
//   k_act_energy<T>  one workgroup per run of act_wg_frames(wl, hop) consecutive frames of one column (only the frames
//               that touch the column's source are listed).  The run's samples, (frames - 1) hop + wl <= kActLds of
//               them, are staged in LDS once as f64 -- zeros where they lie outside the source -- so with hop < wl
//               each sample is loaded once and serves wl / hop frames; a lane issues all its loads before its first
//               store (one wait for memory per workgroup, not one per sample: 7.4 -> 4.7 ms on config 2,
//               profiles/r31_activity.txt).  A wave takes a frame: lane j sums the products
//               of the samples i = j mod 64 in ascending i from 0.0, then the lanes fold 32, 16, .., 1: frame_sum's
//               additions in frame_sum's order.  The energy goes to the column's compact scratch, and each wave's
//               largest one into the column's maximum by an integer atomic max on the bit pattern (the values are
//               non-negative doubles: their order is their patterns' order, and a maximum does not depend on it).
//   k_act_label  one wave per column, in blocks of kActBlockWords words of 64 frames.  The raw bits are packed by
//               ballot, word w of a block kept by lane w.  Each smoothing step with a length is two walks over the
//               words, lane = word: forward, a wave scan of every word's last set bit carries the nearest set bit in
//               front of each word from block to block; backward, the scan of the first set bits carries the nearest
//               one behind, and the lane forms its word of the step (act_close_word, act_open_word over the
//               complements, act_hang_word) from its own bits by clz / ctz and the two carried frames.  A last walk
//               stores the bytes and folds the column's report.  A lane reads only words it wrote itself.
//   k_act_unit  a lane per frame of a unit: the row's sum, counted into the unit's report (which the unit's first
//               column cleared in k_act_label) by wave ballots and integer atomic adds.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

constexpr int64_t kActFar = (int64_t)1 << 62; // no set bit behind

template <class I> __device__ __forceinline__ uint32_t act_find(const I *items, uint32_t n, uint64_t idx)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (items[mid].g0 <= idx)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void act_swap(uint64_t *&a, uint64_t *&b)
{
    uint64_t *t = a;
    a = b;
    b = t;
}

__device__ __forceinline__ int64_t act_shfl(int64_t v, uint32_t lane)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)(uint64_t)v, (int)lane, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), (int)lane, 64);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <class T>
__global__ __launch_bounds__(kActEnergyLanes) void k_act_energy(const ActCol *__restrict__ cols, uint32_t n_cols, uint32_t grid,
                                                         unsigned long long *__restrict__ col_max)
{
    __shared__ double s[kActLds];
    const uint32_t ci = act_find(cols, n_cols, blockIdx.x);
    const ActCol c = cols[ci];
    const uint32_t F = act_wg_frames(c.wl, c.hop);
    const uint64_t fa = (blockIdx.x - c.g0) * (uint64_t)F;
    if (fa >= c.nf)
        return;
    const uint32_t frames = (uint32_t)std::min<uint64_t>(F, c.nf - fa);
    // the run's first sample, counted from the source's first one
    const int64_t k0 = act_start(grid, c.f0 + fa, c.wl, c.hop) - (int64_t)c.start;
    const uint32_t span = (frames - 1) * c.hop + c.wl; // <= kActLds by act_wg_frames
    const T *x = (const T *)c.x;
    // (every load of a lane issued before the first store: a lane holds its kActLds / kActEnergyLanes samples in
    // registers, so the staging waits for memory once and not once per sample)
    constexpr uint32_t kPer = kActLds / kActEnergyLanes;
    static_assert(kPer * kActEnergyLanes == kActLds, "a lane stages a whole number of samples");
    T r[kPer];
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint32_t i = threadIdx.x + j * kActEnergyLanes;
        const int64_t k = k0 + (int64_t)i;
        r[j] = i < span && k >= 0 && (uint64_t)k < c.n ? x[k] : (T)0;
    }
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint32_t i = threadIdx.x + j * kActEnergyLanes;
        if (i < span)
            s[i] = (double)r[j];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double mx = 0.0;
    for (uint32_t f = wave; f < frames; f += kActEnergyLanes / 64) {
        const double *v = s + f * c.hop;
        double p = 0.0;
        for (uint32_t i = lane; i < c.wl; i += 64) {
            const double t = v[i] * v[i];
            p = p + t;
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1)
            p = p + __shfl_down(p, w, 64);
        if (lane == 0) {
            c.e[fa + f] = p;
            if (p > mx)
                mx = p;
        }
    }
    if (lane == 0 && mx > 0.0)
        atomicMax(col_max + ci, (unsigned long long)__double_as_longlong(mx));
}

// One step over the words src[0..nw) of a column into dst (lane = word of a block; `before` is scratch of nw words).
// kStep 0: close, 1: open, 2: hang
template <int kStep>
__device__ __forceinline__ void act_step(const uint64_t *src, uint64_t *dst, int64_t *before, uint64_t nw, int64_t T,
                                         const ActLaunch &L)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t blocks = (nw + kActBlockWords - 1) / kActBlockWords;
    // (open walks the complements: a clear frame is a set bit, and so is every frame at T and behind)
    auto load = [&](uint64_t wi) {
        const uint64_t w = wi < nw ? src[wi] : 0;
        return kStep == 1 ? ~w : w;
    };
    int64_t carry = -1;
    for (uint64_t blk = 0; blk < blocks; blk++) {
        const uint64_t wi = blk * kActBlockWords + lane;
        const uint64_t w = load(wi);
        int64_t incl = w ? (int64_t)(wi * 64) + 63 - (int64_t)__builtin_clzll(w) : -1;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const int64_t o = act_shfl(incl, lane >= d ? lane - d : lane);
            if (lane >= d && o > incl)
                incl = o;
        }
        int64_t excl = act_shfl(incl, lane ? lane - 1 : 0);
        if (lane == 0 || carry > excl)
            excl = carry;
        if (wi < nw)
            before[wi] = excl;
        const int64_t all = act_shfl(incl, 63);
        if (all > carry)
            carry = all;
    }
    carry = kActFar;
    for (uint64_t blk = blocks; blk-- > 0;) {
        const uint64_t wi = blk * kActBlockWords + lane;
        const uint64_t w = load(wi);
        int64_t incl = w ? (int64_t)(wi * 64) + (int64_t)__builtin_ctzll(w) : kActFar;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const int64_t o = act_shfl(incl, lane + d < 64 ? lane + d : lane);
            if (lane + d < 64 && o < incl)
                incl = o;
        }
        int64_t excl = act_shfl(incl, lane < 63 ? lane + 1 : 63);
        if (lane == 63 || carry < excl)
            excl = carry;
        if (wi < nw) {
            const int64_t b = (int64_t)(wi * 64), a = before[wi];
            dst[wi] = kStep == 0   ? act_close_word(w, b, a, excl, T, L.min_gap)
                      : kStep == 1 ? act_open_word(w, b, a, excl, T, L.min_speech)
                                   : act_hang_word(w, b, a, excl, T, L.hang_before, L.hang_after);
        }
        const int64_t all = act_shfl(incl, 0);
        if (all < carry)
            carry = all;
    }
}

__global__ __launch_bounds__(64) void k_act_label(const ActCol *__restrict__ cols,
                                                  const unsigned long long *__restrict__ col_max,
                                                  ActReport *__restrict__ reports,
                                                  ActUnitReport *__restrict__ unit_reports, ActLaunch L)
{
    const ActCol c = cols[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    if (c.col == 0 && lane == 0) // (k_act_unit, behind this kernel, counts into it)
        unit_reports[c.unit] = ActUnitReport{0, 0, 0, 0};
    const double peak = __longlong_as_double((long long)col_max[blockIdx.x]);
    const double thr = act_threshold(L.ref_abs != 0, c.q, c.thr_abs, peak);
    const bool smooth = L.smooth();
    const uint64_t blocks = (c.nw + kActBlockWords - 1) / kActBlockWords;
    uint64_t active = 0;
    int64_t first = (int64_t)c.T, last = -1;
    // the words of a block, lane = word, on their way out: the bytes and the report
    auto emit = [&](uint64_t blk, uint64_t mine) {
        const uint64_t wb = blk * kActBlockWords;
        for (uint32_t w = 0; w < kActBlockWords && wb + w < c.nw; w++) {
            const uint64_t word = (uint64_t)act_shfl((int64_t)mine, w);
            const uint64_t t = (wb + w) * 64 + lane;
            if (t < c.T)
                c.y[t * c.C] = (uint8_t)((word >> lane) & 1u);
        }
        if (mine) {
            const int64_t b = (int64_t)((wb + lane) * 64);
            active += (uint64_t)__builtin_popcountll(mine);
            first = std::min<int64_t>(first, b + (int64_t)__builtin_ctzll(mine));
            last = std::max<int64_t>(last, b + 63 - (int64_t)__builtin_clzll(mine));
        }
    };
    uint64_t *w0 = c.words, *w1 = c.words + c.nw;
    int64_t *before = (int64_t *)(c.words + 2 * c.nw);
    for (uint64_t blk = 0; blk < blocks; blk++) {
        const uint64_t wb = blk * kActBlockWords;
        uint64_t mine = 0;
        for (uint32_t w = 0; w < kActBlockWords && wb + w < c.nw; w++) {
            const uint64_t t = (wb + w) * 64 + lane;
            bool bit = false;
            if (t >= c.f0 && t - c.f0 < c.nf)
                bit = act_raw(c.e[t - c.f0], thr);
            const uint64_t word = __ballot(bit);
            if (lane == w)
                mine = word;
        }
        if (!smooth)
            emit(blk, mine);
        else if (wb + lane < c.nw)
            w0[wb + lane] = mine;
    }
    if (smooth) {
        const int64_t T = (int64_t)c.T;
        if (L.min_gap) {
            act_step<0>(w0, w1, before, c.nw, T, L);
            act_swap(w0, w1);
        }
        if (L.min_speech > 1) {
            act_step<1>(w0, w1, before, c.nw, T, L);
            act_swap(w0, w1);
        }
        if (L.hang_before || L.hang_after) {
            act_step<2>(w0, w1, before, c.nw, T, L);
            act_swap(w0, w1);
        }
        for (uint64_t blk = 0; blk < blocks; blk++) {
            const uint64_t wi = blk * kActBlockWords + lane;
            emit(blk, wi < c.nw ? w0[wi] : 0);
        }
    }
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        active += (uint64_t)act_shfl((int64_t)active, lane ^ d);
        first = std::min<int64_t>(first, act_shfl(first, lane ^ d));
        last = std::max<int64_t>(last, act_shfl(last, lane ^ d));
    }
    if (lane == 0)
        reports[c.slot] = ActReport{active, (uint64_t)first, last < 0 ? c.T : (uint64_t)last, peak, thr};
}

__global__ __launch_bounds__(kActLanes) void k_act_unit(const ActUnit *__restrict__ units, uint32_t n_units,
                                                       ActUnitReport *__restrict__ reports)
{
    const uint32_t ui = act_find(units, n_units, blockIdx.x);
    const ActUnit U = units[ui];
    const uint64_t t = (blockIdx.x - U.g0) * (uint64_t)kActLanes + threadIdx.x;
    uint32_t k = 0;
    if (t < U.T) {
        const uint8_t *row = U.y + t * U.C;
        for (uint32_t j = 0; j < U.C; j++)
            k += row[j];
    }
    const bool in = t < U.T;
    const uint64_t none = __ballot(in && k == 0), one = __ballot(in && k == 1), many = __ballot(in && k >= 2);
    if ((threadIdx.x & 63u) == 0) {
        unsigned long long *r = (unsigned long long *)(reports + U.unit);
        if (none)
            atomicAdd(r + 1, (unsigned long long)__builtin_popcountll(none));
        if (one)
            atomicAdd(r + 2, (unsigned long long)__builtin_popcountll(one));
        if (many)
            atomicAdd(r + 3, (unsigned long long)__builtin_popcountll(many));
    }
    if (blockIdx.x == U.g0 && threadIdx.x == 0)
        atomicAdd((unsigned long long *)(reports + U.unit), (unsigned long long)U.T);
}

} // namespace

hipError_t launch_activity(bool i16, const ActCol *cols_dev, uint32_t n_cols, uint64_t energy_wgs,
                           const ActUnit *units_dev, uint32_t n_units, uint64_t unit_wgs, uint64_t *col_max,
                           ActReport *reports, ActUnitReport *unit_reports, const ActLaunch &L, hipStream_t stream)
{
    if (energy_wgs > 0x7fffffffull || unit_wgs > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (n_cols) {
        hipError_t e;
        if ((e = hipMemsetAsync(col_max, 0, sizeof(uint64_t) * n_cols, stream)) != hipSuccess)
            return e;
        if (energy_wgs) {
            if (i16)
                hipLaunchKernelGGL(k_act_energy<int16_t>, dim3((uint32_t)energy_wgs), dim3(kActEnergyLanes), 0, stream, cols_dev,
                                   n_cols, L.grid, (unsigned long long *)col_max);
            else
                hipLaunchKernelGGL(k_act_energy<double>, dim3((uint32_t)energy_wgs), dim3(kActEnergyLanes), 0, stream, cols_dev,
                                   n_cols, L.grid, (unsigned long long *)col_max);
        }
        hipLaunchKernelGGL(k_act_label, dim3(n_cols), dim3(64), 0, stream, cols_dev, (const unsigned long long *)col_max,
                           reports, unit_reports, L);
    }
    if (n_units && unit_wgs)
        hipLaunchKernelGGL(k_act_unit, dim3((uint32_t)unit_wgs), dim3(kActLanes), 0, stream, units_dev, n_units,
                           unit_reports);
    return hipGetLastError();
}

namespace {

// jb_activity_pcm_batch and its _i16 form: the inputs packed one after the other on the device, the units laid out by
// act_layout; with JB_ACTIVITY_UNIT and a request the programmes are mixed first (launch_mix) and measured whole
template <class T>
int activity_pcm_batch(const T *const *in, const size_t *n_in, size_t n, const MixUtt *request, const MixOpts *mix_opts,
                       const uint32_t *hz, const ActOpts *opts, int32_t device, uint8_t **out, uint64_t *Ts, uint32_t *Cs,
                       size_t *n_units, jb_activity_report *col_reports, jb_activity_unit_report *unit_reports,
                       const char *who)
{
    if (n_units)
        *n_units = 0;
    int rc = pcm_check((const void *const *)in, n_in, n, out && Ts && Cs, (void **)out, nullptr);
    if (rc)
        return rc;
    if ((rc = act_check_opts(opts, who)))
        return rc;
    if (!hz && !(opts->flags & kActSamples)) {
        set_error(std::string(who) + ": hz is NULL without JB_ACTIVITY_SAMPLES");
        return JB_ERR_INVALID;
    }
    std::vector<MixUtt> own;
    if (!request) {
        own.assign(n, MixUtt{kMixNone, 0, 0, 0, 0, 0, 0.0, 0});
        request = own.data();
    }
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    if ((rc = mix_layout_checked(request, false, ns.data(), hz, n, sizeof(T), mix_opts, &lay, who)))
        return rc;
    const size_t P = lay.units.size();
    const bool whole = opts->columns == kActUnit;
    std::vector<uint64_t> unit_n(P);
    std::vector<uint32_t> unit_hz(P);
    for (size_t p = 0; p < P; p++) {
        unit_n[p] = lay.units[p].n;
        unit_hz[p] = lay.units[p].hz;
    }
    ActLayout al;
    if ((rc = act_layout_checked(*opts, P, unit_n.data(), hz ? unit_hz.data() : nullptr, lay.progs.first.data(),
                                 lay.progs.members.data(), lay.start.data(), ns.data(), lay.gain.data(), &al, who)))
        return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    std::vector<uint64_t> xoff;
    const T *dx = ds.pack(in, n_in, n, &xoff);
    const T *dmix = nullptr;
    if (whole) { // the units' own PCM: the mixture
        T *dy = ds.alloc<T>(lay.total);
        std::vector<ProgMember> members;
        std::vector<ProgSpan> spans;
        uint64_t tiles = 0;
        mix_lists(lay, request, ns.data(), xoff.data(), dx, dy, sizeof(T), &members, &spans, &tiles);
        MixLaunch M{};
        M.members = ds.upload(members);
        M.segs = ds.upload(lay.segs);
        M.lists = ds.upload(lay.lists);
        M.tile_peak = ds.alloc<double>(tiles * kMixWaves);
        M.res = ds.alloc<MixResult>(P);
        M.fit = mix_opts && (mix_opts->flags & kMixFit);
        M.ceiling = M.fit ? mix_ceiling(mix_opts->ceiling_db) : 0.0;
        const ProgSpan *dsp = ds.upload(spans);
        if (ds.ok())
            ds.err = launch_mix(sizeof(T) == 2, dsp, (uint32_t)P, tiles, M, ds.stream);
        dmix = dy;
    }
    uint8_t *dlab = ds.alloc<uint8_t>(al.bytes);
    double *de = ds.alloc<double>(al.energies);
    uint64_t *dw = ds.alloc<uint64_t>(al.words);
    const size_t NC = al.cols.size();
    uint64_t *dmax = ds.alloc<uint64_t>(NC);
    ActReport *drep = ds.alloc<ActReport>(NC);
    ActUnitReport *durep = ds.alloc<ActUnitReport>(P);
    ActLaunch L{opts->grid, opts->reference == kActRefAbs, opts->min_speech, opts->min_gap, opts->hang_before,
                opts->hang_after};
    std::vector<ActCol> cols(NC);
    std::vector<ActUnit> units(P);
    uint64_t energy_wgs = 0, unit_wgs = 0;
    const double q = act_ratio(opts->gate_db);
    for (size_t p = 0; p < P; p++) {
        const ActLayUnit &U = al.units[p];
        units[p] = ActUnit{dlab + U.off, U.T, unit_wgs, U.C, (uint32_t)p};
        unit_wgs += act_unit_wgs(U.T);
        for (uint32_t j = 0; j < U.C; j++) {
            const ActLayCol &a = al.cols[U.col0 + j];
            ActCol &c = cols[U.col0 + j];
            c.x = whole ? (const void *)(dmix + lay.units[p].off) : (const void *)(dx + xoff[a.utt]);
            c.y = dlab + U.off + j;
            c.e = de + a.e0;
            c.words = L.smooth() ? dw + a.w0 : nullptr;
            c.start = a.start;
            c.n = a.n;
            c.T = U.T;
            c.f0 = a.f0;
            c.nf = a.nf;
            c.g0 = energy_wgs;
            c.nw = (U.T + 63) / 64;
            c.q = q;
            c.thr_abs = act_abs_threshold(opts->gate_db, U.wl);
            c.C = U.C;
            c.wl = U.wl;
            c.hop = U.hop;
            c.col = j;
            c.slot = U.col0 + j;
            c.unit = (uint32_t)p;
            energy_wgs += act_energy_wgs(a.nf, U.wl, U.hop);
        }
    }
    const ActCol *dcols = ds.upload(cols);
    const ActUnit *dunits = ds.upload(units);
    if (ds.ok())
        ds.err = launch_activity(sizeof(T) == 2, dcols, (uint32_t)NC, energy_wgs, dunits, (uint32_t)P, unit_wgs, dmax,
                                 drep, durep, L, ds.stream);
    std::vector<uint8_t> host;
    std::vector<ActReport> rep;
    std::vector<ActUnitReport> urep;
    ds.read_back(&host, (const uint8_t *)dlab, al.bytes);
    ds.read_back(&rep, (const ActReport *)drep, NC);
    ds.read_back(&urep, (const ActUnitReport *)durep, P);
    if ((rc = ds.status()))
        return rc;
    std::vector<PcmShare> shares(P);
    for (size_t p = 0; p < P; p++)
        shares[p] = {al.units[p].off, al.units[p].T * al.units[p].C};
    if ((rc = hand_out(host.data(), 1, shares, (void **)out, nullptr)))
        return rc;
    for (size_t p = 0; p < P; p++) {
        Ts[p] = al.units[p].T;
        Cs[p] = al.units[p].C;
        if (unit_reports)
            memcpy(unit_reports + p, &urep[p], sizeof(ActUnitReport));
    }
    if (col_reports && NC)
        memcpy(col_reports, rep.data(), sizeof(ActReport) * NC);
    if (n_units)
        *n_units = P;
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_activity_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                          const jb_mix_opts *mix_opts, const uint32_t *hz, const jb_activity_opts *opts, int32_t device,
                          uint8_t **out, uint64_t *T, uint32_t *C, size_t *n_units, jb_activity_report *cols,
                          jb_activity_unit_report *units)
{
    return activity_pcm_batch(in, n_in, n, (const MixUtt *)req, (const MixOpts *)mix_opts, hz, (const ActOpts *)opts,
                              device, out, T, C, n_units, cols, units, "jb_activity_pcm_batch");
}

int jb_activity_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                              const jb_mix_opts *mix_opts, const uint32_t *hz, const jb_activity_opts *opts,
                              int32_t device, uint8_t **out, uint64_t *T, uint32_t *C, size_t *n_units,
                              jb_activity_report *cols, jb_activity_unit_report *units)
{
    return activity_pcm_batch(in, n_in, n, (const MixUtt *)req, (const MixOpts *)mix_opts, hz, (const ActOpts *)opts,
                              device, out, T, C, n_units, cols, units, "jb_activity_pcm_batch_i16");
}

} // extern "C"

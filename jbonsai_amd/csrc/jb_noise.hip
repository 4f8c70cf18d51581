// jb_noise.hip -- the noise stage on the device (jb_noise.h): background noise added to the f64 PCM at the output rate
// at a target signal-to-noise ratio, behind the convolution and in front of the filter's sections.  Three kernels, all
// bound by memory:
//
//   k_noise_sums    one workgroup of 256 lanes per tile of 1,024 samples of one utterance.  Lane l forms partial l of
//                   the tile's power sums of x and of the noise w by the rule of jb_noise.h (noise_partial: x read once,
//                   coalesced; the bed gathered at (offset + n) mod Lb with one modulo per lane and a
//                   compare-and-subtract per term -- Lb may be 1, a tile may wrap many times; white noise made in the
//                   lane).  The partial tree runs in the rule's order: h = 128 and 64 through LDS, h = 32 .. 1 inside
//                   the first wave by lane shifts.  Lane 0 stores the tile's two sums as one 16-byte store to the
//                   scratch: 16 bytes per 1,024 samples.  No atomics, nothing whose order the scheduling sets.
//   k_noise_gain    one wave per utterance.  The tile sums are loaded 64 at a time, one 16-byte load per lane, through
//                   two LDS buffers (the next chunk is on its way while the present one is added), and added in
//                   ascending order by lane 0; with JB_NOISE_REF_ACTIVE a second walk over the same sums takes the
//                   active tiles; then the gain and the utterance's record.
//   k_noise_apply   one workgroup per 4,096 samples of one utterance, streaming: a lane takes groups of 16 output bytes
//                   -- 2 f64 or 8 16-bit samples -- loads x 16 bytes at a time at whatever alignment the utterance has
//                   (the f64 slabs are 8-byte aligned; k_join's under-aligned form), gathers the bed or makes the white
//                   samples, y = fma(g, w, x), and stores the group as one vector store; only an utterance's last
//                   partial group goes out sample by sample.  g == 0: y = x, bit for bit.  y may be x itself (the
//                   chain's intermediate is rewritten in place): a lane reads its group before it writes it and no
//                   other lane touches it.
// Tiles are counted from the utterance's own first sample and a sample is its own fma: a sample's bits depend on its
// utterance's samples, the request and the gain only.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

#define JB_NOISE_GLOBAL __attribute__((address_space(1)))
typedef double NoiseD2 __attribute__((ext_vector_type(2)));
typedef double NoiseD2u __attribute__((ext_vector_type(2), aligned(8)));
typedef int16_t NoiseS8u __attribute__((ext_vector_type(8), aligned(2)));

template <class T> struct NoiseVec;
template <> struct NoiseVec<double> {
    typedef NoiseD2u U;
};
template <> struct NoiseVec<int16_t> {
    typedef NoiseS8u U;
};

__device__ __forceinline__ void noise_out(double v, double *o) { *o = v; }
__device__ __forceinline__ void noise_out(double v, int16_t *o)
{
    *o = (int16_t)fmt_quant<false>(v, -32768.0, 32767.0, 0, 0);
}

__global__ __launch_bounds__(kNoiseLanes) void k_noise_sums(const NoiseUtt *__restrict__ utts, uint32_t n_utts,
                                                            double *__restrict__ sums)
{
    __shared__ double s_x[kNoiseLanes], s_w[kNoiseLanes];
    const NoiseUtt U = utts[find_unit(utts, n_utts, blockIdx.x, &NoiseUtt::t0)];
    const uint64_t i = blockIdx.x - U.t0;
    if (i * kNoiseTile >= U.n)
        return;
    const uint32_t l = threadIdx.x;
    const JB_NOISE_GLOBAL double *gx = (const JB_NOISE_GLOBAL double *)U.x;
    const JB_NOISE_GLOBAL double *gb = (const JB_NOISE_GLOBAL double *)U.bed;
    double px = noise_partial(U.n, i, l, [&](uint64_t k) { return gx[k]; });
    double pw;
    if (gb) {
        // the lane's terms are 256 samples apart: one modulo, then a step of 256 mod Lb with a compare-and-subtract
        const uint32_t lb = U.lb, step = kNoiseLanes % lb;
        uint32_t idx = (uint32_t)((U.offset + i * kNoiseTile + l) % lb);
        pw = noise_partial(U.n, i, l, [&](uint64_t) {
            const double w = gb[idx];
            idx += step;
            idx = idx >= lb ? idx - lb : idx;
            return w;
        });
    } else {
        const uint64_t ms = U.mseed;
        pw = noise_partial(U.n, i, l, [&](uint64_t k) { return noise_white(ms, k); });
    }
    // the tree: p[l] = p[l] + p[l + h], h = 128, 64 through LDS ...
    s_x[l] = px;
    s_w[l] = pw;
    __syncthreads();
    if (l < 128) {
        px = px + s_x[l + 128];
        pw = pw + s_w[l + 128];
    }
    __syncthreads();
    if (l < 128) {
        s_x[l] = px;
        s_w[l] = pw;
    }
    __syncthreads();
    if (l >= 64)
        return;
    px = px + s_x[l + 64];
    pw = pw + s_w[l + 64];
    // ... and h = 32 .. 1 inside the first wave: lane l adds lane l + h's (what the lanes at and above h make is not read)
#pragma unroll
    for (uint32_t h = 32; h; h >>= 1) {
        px = px + __shfl_down(px, h, 64);
        pw = pw + __shfl_down(pw, h, 64);
    }
    if (l == 0)
        *(JB_NOISE_GLOBAL NoiseD2 *)((JB_NOISE_GLOBAL double *)sums + 2 * (U.s0 + i)) = NoiseD2{px, pw};
}

__global__ __launch_bounds__(kNoiseWave) void k_noise_gain(const NoiseUtt *__restrict__ utts, uint32_t n_utts,
                                                           const double *__restrict__ sums,
                                                           NoiseRecord *__restrict__ rec)
{
    __shared__ NoiseD2 s_t[2][kNoiseWave];
    if (blockIdx.x >= n_utts)
        return;
    const NoiseUtt U = utts[blockIdx.x];
    const uint64_t nt = noise_tiles(U.n);
    const uint32_t l = threadIdx.x;
    const JB_NOISE_GLOBAL NoiseD2 *gs = (const JB_NOISE_GLOBAL NoiseD2 *)sums + U.s0;
    double Sx = 0.0, Sw = 0.0;
    {
        NoiseD2 cur = l < nt ? gs[l] : NoiseD2{0.0, 0.0};
        uint32_t b = 0;
        for (uint64_t c = 0; c < nt; c += kNoiseWave, b ^= 1u) {
            s_t[b][l] = cur;
            cur = c + kNoiseWave + l < nt ? gs[c + kNoiseWave + l] : NoiseD2{0.0, 0.0};
            __syncthreads();
            if (l == 0) {
                const uint32_t cnt = (uint32_t)std::min<uint64_t>(kNoiseWave, nt - c);
                for (uint32_t k = 0; k < cnt; k++) {
                    const NoiseD2 v = s_t[b][k];
                    if (c == 0 && k == 0) {
                        Sx = v[0];
                        Sw = v[1];
                    } else {
                        Sx = Sx + v[0];
                        Sw = Sw + v[1];
                    }
                }
            }
        }
    }
    double A = Sx;
    uint64_t C = U.n;
    if (U.active) {
        const double Sq = Sx * U.q, dn = (double)U.n;
        bool first = true;
        A = 0.0;
        C = 0;
        __syncthreads();
        NoiseD2 cur = l < nt ? gs[l] : NoiseD2{0.0, 0.0};
        uint32_t b = 0;
        for (uint64_t c = 0; c < nt; c += kNoiseWave, b ^= 1u) {
            s_t[b][l] = cur;
            cur = c + kNoiseWave + l < nt ? gs[c + kNoiseWave + l] : NoiseD2{0.0, 0.0};
            __syncthreads();
            if (l == 0) {
                const uint32_t cnt = (uint32_t)std::min<uint64_t>(kNoiseWave, nt - c);
                for (uint32_t k = 0; k < cnt; k++) {
                    const double t = s_t[b][k][0];
                    const uint32_t ci = (uint32_t)std::min<uint64_t>(kNoiseTile, U.n - (c + k) * kNoiseTile);
                    if (!noise_active(t, dn, Sq, ci))
                        continue;
                    A = first ? t : A + t;
                    C += ci;
                    first = false;
                }
            }
        }
    }
    if (l == 0) {
        JB_NOISE_GLOBAL NoiseRecord *o = (JB_NOISE_GLOBAL NoiseRecord *)rec + U.rep;
        o->A = A;
        o->Bs = Sw;
        o->gain = noise_gain(A, C, Sw, U.n, U.r);
        o->C = C;
    }
}

// The tile [k0, k1) of U under the gain g, in groups of 16 output bytes
template <class T> __device__ __forceinline__ void noise_apply_tile(const NoiseUtt &U, uint64_t k0, uint64_t k1, double g)
{
    typedef typename NoiseVec<T>::U V;
    constexpr uint32_t G = 16 / sizeof(T);
    static_assert(kNoiseApplyTile % (kNoiseLanes * G) == 0, "a tile is whole groups of every lane");
    const JB_NOISE_GLOBAL double *gx = (const JB_NOISE_GLOBAL double *)U.x;
    const JB_NOISE_GLOBAL double *gb = (const JB_NOISE_GLOBAL double *)U.bed;
    JB_NOISE_GLOBAL T *gy = (JB_NOISE_GLOBAL T *)U.y;
    const bool mix = g != 0.0;
    const uint32_t lb = gb ? U.lb : 1u, step = (kNoiseLanes * G) % lb;
    const uint64_t ks0 = k0 + (uint64_t)threadIdx.x * G, ms = U.mseed;
    uint32_t idx = gb ? (uint32_t)((U.offset + ks0) % lb) : 0u; // of the group's first sample
#pragma unroll
    for (uint32_t it = 0; it < kNoiseApplyTile / (kNoiseLanes * G); it++) {
        const uint64_t ks = ks0 + (uint64_t)it * kNoiseLanes * G;
        uint32_t j = idx;
        auto w = [&](uint64_t k) {
            if (!gb)
                return noise_white(ms, k);
            const double v = gb[j];
            j = j + 1 >= lb ? 0u : j + 1;
            return v;
        };
        if (ks + G <= k1) {
            double x[G];
#pragma unroll
            for (uint32_t q = 0; q < G; q += 2) {
                const NoiseD2u v = *(const JB_NOISE_GLOBAL NoiseD2u *)(gx + ks + q);
                x[q] = v[0];
                x[q + 1] = v[1];
            }
            V o;
#pragma unroll
            for (uint32_t q = 0; q < G; q++) {
                T e;
                noise_out(mix ? __builtin_fma(g, w(ks + q), x[q]) : x[q], &e);
                o[q] = e;
            }
            *(JB_NOISE_GLOBAL V *)(gy + ks) = o;
        } else if (ks < k1) {
            // the utterance's last partial group
            for (uint64_t k = ks; k < k1; k++) {
                const double x = gx[k];
                T e;
                noise_out(mix ? __builtin_fma(g, w(k), x) : x, &e);
                gy[k] = e;
            }
        }
        idx += step;
        idx = idx >= lb ? idx - lb : idx;
    }
}

// (x and y are not restrict: the chain's intermediate is rewritten in place)
__global__ __launch_bounds__(kNoiseLanes) void k_noise_apply(const NoiseUtt *utts, uint32_t n_utts,
                                                             const NoiseRecord *rec)
{
    const NoiseUtt U = utts[find_unit(utts, n_utts, blockIdx.x, &NoiseUtt::a0)];
    const uint64_t k0 = (blockIdx.x - U.a0) * (uint64_t)kNoiseApplyTile;
    if (k0 >= U.n)
        return;
    const uint64_t k1 = std::min<uint64_t>(k0 + kNoiseApplyTile, U.n);
    const double g = rec[U.rep].gain;
    if (U.i16)
        noise_apply_tile<int16_t>(U, k0, k1, g);
    else
        noise_apply_tile<double>(U, k0, k1, g);
}

} // namespace

hipError_t launch_noise(const NoiseUtt *utts_dev, uint32_t n, uint64_t tiles, uint64_t apply, double *sums,
                        NoiseRecord *rec, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull || apply > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (tiles)
        hipLaunchKernelGGL(k_noise_sums, dim3((uint32_t)tiles), dim3(kNoiseLanes), 0, stream, utts_dev, n, sums);
    hipLaunchKernelGGL(k_noise_gain, dim3(n), dim3(kNoiseWave), 0, stream, utts_dev, n, sums, rec);
    if (apply)
        hipLaunchKernelGGL(k_noise_apply, dim3((uint32_t)apply), dim3(kNoiseLanes), 0, stream, utts_dev, n, rec);
    return hipGetLastError();
}

void noise_launch_list(const std::vector<NoiseUtt> &utts, const std::vector<uint8_t> &has,
                       const std::vector<uint8_t> *only, NoiseLaunch *out)
{
    *out = NoiseLaunch{};
    for (size_t u = 0; u < utts.size(); u++) {
        if (!has[u] || (only && !(*only)[u]))
            continue;
        NoiseUtt w = utts[u];
        w.t0 = out->tiles;
        w.a0 = out->apply;
        out->tiles += noise_tiles(w.n);
        out->apply += noise_apply_tiles(w.n);
        out->utts.push_back(w);
    }
}

namespace {

// jb_noise_pcm_batch / _i16: the inputs packed one after the other on the device (as a batch's slab has them), the
// outputs the same way; an utterance without a request is copied by the host (the stage never sees it)
template <class T>
int noise_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_noise *req, const uint32_t *hz,
                    int32_t device, T **out, size_t *n_out, jb_noise_report *reports, const char *who)
{
    int rc = pcm_check((const void *const *)in, n_in, n, req && hz && out && n_out, (void **)out, n_out);
    if (rc)
        return rc;
    NoiseBeds beds;
    std::vector<NoiseItem> items(n);
    for (size_t u = 0; u < n; u++) {
        if ((rc = noise_check(&req[u], hz[u], u, who)))
            return rc;
        if (req[u].flags & kNoiseVary) {
            set_error(std::string(who) + ": utterance " + std::to_string(u) +
                      ": flags: JB_NOISE_VARY needs one request over many utterances");
            return JB_ERR_INVALID;
        }
        if (noise_none(*(const NoiseSpec *)&req[u]))
            continue;
        items[u] = noise_resolve(req[u], false, u,
                                 req[u].kind == kNoiseBed ? beds.find(req[u].bed, req[u].bed_len, req[u].hz) : -1);
    }
    if (beds.words() > kNoiseMaxBeds) {
        set_error(std::string(who) + ": the distinct beds hold more than 2^26 samples");
        return JB_ERR_UNSUPPORTED;
    }
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    std::vector<uint64_t> off;
    const double *dx = ds.pack(in, n_in, n, &off);
    T *dy = ds.alloc<T>(off[n]);
    double *db = ds.alloc<double>(beds.words());
    std::vector<double> image;
    std::vector<NoiseBed> cls;
    beds.bind(db, &image, &cls);
    if (ds.ok() && !image.empty())
        ds.err = hipMemcpyAsync(db, image.data(), sizeof(double) * image.size(), hipMemcpyHostToDevice, ds.stream);
    std::vector<NoiseUtt> utts(n);
    std::vector<uint8_t> has(n, 0);
    uint64_t tiles = 0;
    for (size_t u = 0; u < n; u++) {
        const NoiseItem &it = items[u];
        has[u] = it.on;
        if (!it.on)
            continue;
        NoiseUtt w{};
        w.x = dx + off[u];
        w.y = dy + off[u];
        w.bed = it.bed >= 0 ? cls[(size_t)it.bed].w : nullptr;
        w.n = n_in[u];
        w.s0 = tiles;
        w.mseed = fmt_mix(it.seed);
        w.r = it.r;
        w.q = it.q;
        w.lb = it.bed >= 0 ? cls[(size_t)it.bed].len : 0;
        w.offset = it.offset;
        w.active = it.active;
        w.i16 = sizeof(T) == 2;
        w.rep = (uint32_t)u;
        utts[u] = w;
        tiles += noise_tiles(n_in[u]);
    }
    NoiseLaunch l;
    noise_launch_list(utts, has, nullptr, &l);
    double *sums = ds.alloc<double>(2 * tiles);
    NoiseRecord *drec = ds.alloc<NoiseRecord>(n);
    const NoiseUtt *du = ds.upload(l.utts);
    if (ds.ok())
        ds.err = launch_noise(du, (uint32_t)l.utts.size(), l.tiles, l.apply, sums, drec, ds.stream);
    std::vector<T> host;
    std::vector<NoiseRecord> recs;
    ds.read_back(&host, dy, off[n]);
    ds.read_back(&recs, drec, n);
    if ((rc = ds.status()))
        return rc;
    host.resize(off[n]);
    for (size_t u = 0; u < n; u++) {
        if (!items[u].on) {
            for (size_t k = 0; k < n_in[u]; k++) {
                if (sizeof(T) == 2)
                    host[off[u] + k] = (T)fmt_quant<false>(in[u][k], -32768.0, 32767.0, 0, 0);
                else
                    host[off[u] + k] = (T)in[u][k];
            }
        }
        if (reports)
            reports[u] = items[u].on ? noise_report_of(items[u], recs[u], n_in[u]) : jb_noise_report{};
    }
    std::vector<PcmShare> shares(n);
    for (size_t u = 0; u < n; u++)
        shares[u] = {off[u], n_in[u]};
    return hand_out(host.data(), sizeof(T), shares, (void **)out, n_out);
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_noise_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_noise *req, const uint32_t *hz,
                       int32_t device, double **out, size_t *n_out, jb_noise_report *reports)
{
    return noise_pcm_batch(in, n_in, n, req, hz, device, out, n_out, reports, "jb_noise_pcm_batch");
}

int jb_noise_pcm_batch_i16(const double *const *in, const size_t *n_in, size_t n, const jb_noise *req,
                           const uint32_t *hz, int32_t device, int16_t **out, size_t *n_out, jb_noise_report *reports)
{
    return noise_pcm_batch(in, n_in, n, req, hz, device, out, n_out, reports, "jb_noise_pcm_batch_i16");
}

} // extern "C"

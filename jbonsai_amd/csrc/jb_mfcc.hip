// jb_mfcc.hip -- cepstral features on the device: f64 log-mel frames [T][n_mels] as rows [c' | delta | delta-delta], by
// the rule of jb_mfcc.h.  The stage streams: every kernel reads its frames once, in whole rows, and sums in the rule's
// order, so the seam gives the host form's bits wherever the device takes no square root.
//
//   k_ceps        a workgroup takes kMfTile consecutive frames of one unit (workgroups never cross units) and stages
//                 their L rows in LDS (the tile is one run of memory: coalesced; rows padded to an odd stride).  One
//                 lane per (frame, coefficient) walks m ascending: L from LDS (the lanes of a frame read one address: a
//                 broadcast), D from the transposed [m][i] table, so lanes that follow one another read doubles that
//                 follow one another.  The f64 statics go to scratch.  Not launched with n_ceps = 0: the statics are L.
//                 With the frames' energies (JB_FRAME_ENERGY: k_fbank wrote them) column 0 is their logarithm.
//   k_mfcc_block  one lane per (unit, block of kMfBlock frames, dimension): the block's sum from 0.0 in ascending t,
//                 of c in the mean's pass and of (c - mu)^2 in the variance's.
//   k_mfcc_fold   one lane per (unit, dimension): the block sums from 0.0 in ascending order, times r_T; the mean's pass
//                 leaves mu, the variance's sqrt(max(var, floor)).  No atomics, nothing whose order the scheduling sets.
//   k_delta       a workgroup takes kMfTile frames by kMfCols columns of one unit, stages them with a halo of
//                 delta_order N frames on both sides (clamped at the unit's ends) in LDS, normalised on the way in,
//                 and writes every row's share of [c' | out_1 | out_2] with whole-dword (f32) or whole-qword stores.
// The launch count does not depend on the batch: the lists are laid out like FbankUtt's (prefix sums, a binary search).
// The filterbank pass in front (mfcc_pcm_run here, the output chain's prepare_mfcc) is a RatePass of jb_host.h, as the
// filterbank stage's own; only the cepstral lists are put together here.
#include "jb_host.h"
#include "jb_mfcc.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

constexpr uint32_t kMfRowMax = kFbMaxMels | 1u;                     // an L row in LDS: n_mels | 1 doubles
constexpr uint32_t kMfHaloMax = kMfMaxOrder * kMfMaxWindow;         // frames on each side of a k_delta tile
constexpr uint32_t kMfStage = (kMfTile + 2 * kMfHaloMax) * kMfCols; // doubles of a k_delta tile

__global__ __launch_bounds__(kMfLanes) void k_ceps(MfccParams P, const MfccUtt *__restrict__ utts, uint32_t n_utts)
{
    __shared__ double s_L[kMfTile * kMfRowMax];
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x);
    const MfccUtt U = utts[u];
    const uint64_t t0 = (blockIdx.x - U.g0) * (uint64_t)kMfTile;
    if (t0 >= U.T) // (not reached: a unit's tiles cover its frames)
        return;
    const uint32_t nf = (uint32_t)(U.T - t0 < kMfTile ? U.T - t0 : kMfTile);
    const uint32_t nm = P.n_mels, rs = nm | 1u, nc = P.n_ceps;
    const double *src = U.L + t0 * nm;
    for (uint32_t e = threadIdx.x; e < nf * nm; e += kMfLanes)
        s_L[(e / nm) * rs + e % nm] = src[e];
    __syncthreads();
    double *dst = U.c + t0 * nc;
    for (uint32_t e = threadIdx.x; e < nf * nc; e += kMfLanes) {
        const uint32_t f = e / nc, i = e % nc;
        dst[e] = i == 0 && U.e ? mfcc_c0(U.e[t0 + f], P.e_floor, P.e_ln_floor)
                               : mfcc_cep(s_L + f * rs, P.Dt + i, nc, nm, P.lift[i]);
    }
}

__global__ __launch_bounds__(kMfLanes) void k_mfcc_block(MfccParams P, const MfccUtt *__restrict__ utts, uint32_t n_utts,
                                                         uint64_t items, uint32_t var)
{
    const uint64_t item = (uint64_t)blockIdx.x * kMfLanes + threadIdx.x;
    if (item >= items)
        return;
    const uint64_t gb = item / P.d;
    const uint32_t i = (uint32_t)(item % P.d);
    const uint32_t u = find_unit(utts, n_utts, gb, &MfccUtt::b0);
    const MfccUtt U = utts[u];
    const uint64_t blk = gb - U.b0, t0 = blk * kMfBlock;
    if (t0 >= U.T)
        return;
    const uint64_t t1 = U.T - t0 < kMfBlock ? U.T : t0 + kMfBlock;
    const double mu = var ? U.stat[i] : 0.0;
    double acc = 0.0;
    for (uint64_t t = t0; t < t1; t++)
        acc = acc + mfcc_stat_term(U.c[t * P.d + i], mu, var != 0);
    U.bs[blk * P.d + i] = acc;
}

__global__ __launch_bounds__(kMfLanes) void k_mfcc_fold(MfccParams P, const MfccUtt *__restrict__ utts, uint32_t n_utts,
                                                        uint32_t var)
{
    const uint64_t item = (uint64_t)blockIdx.x * kMfLanes + threadIdx.x;
    if (item >= (uint64_t)n_utts * P.d)
        return;
    const uint32_t u = (uint32_t)(item / P.d), i = (uint32_t)(item % P.d);
    const MfccUtt U = utts[u];
    if (U.T == 0)
        return;
    const uint64_t nb = mfcc_blocks(U.T);
    double total = 0.0;
    for (uint64_t b = 0; b < nb; b++)
        total = total + U.bs[b * P.d + i];
    const double v = total * U.r_T;
    if (var)
        U.stat[P.d + i] = mfcc_sd(v, P.floor);
    else
        U.stat[i] = v;
}

__global__ __launch_bounds__(kMfLanes) void k_delta(MfccParams P, const MfccUtt *__restrict__ utts, uint32_t n_utts)
{
    __shared__ double s_c[kMfStage];
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x);
    const MfccUtt U = utts[u];
    const uint64_t t0 = (blockIdx.x - U.g0) * (uint64_t)kMfTile;
    if (t0 >= U.T)
        return;
    const uint32_t nf = (uint32_t)(U.T - t0 < kMfTile ? U.T - t0 : kMfTile);
    const uint32_t d = P.d, col0 = blockIdx.y * kMfCols, w = d - col0 < kMfCols ? d - col0 : kMfCols;
    const int32_t N = (int32_t)P.N, H = (int32_t)(P.order * P.N); // H <= kMfHaloMax
    const uint32_t rows = nf + 2 * (uint32_t)H;
    for (uint32_t e = threadIdx.x; e < rows * w; e += kMfLanes) {
        const uint32_t r = e / w, col = e % w;
        int64_t g = (int64_t)t0 - H + (int64_t)r;
        g = g < 0 ? 0 : g >= (int64_t)U.T ? (int64_t)U.T - 1 : g;
        const double c = U.c[(uint64_t)g * d + col0 + col];
        double mu = 0.0, sd = 1.0;
        if (P.cmvn != kMfCmvnNone)
            mu = U.stat[col0 + col];
        if (P.cmvn == kMfCmvnMeanVar)
            sd = U.stat[d + col0 + col];
        s_c[e] = mfcc_norm(c, mu, sd, P.cmvn);
    }
    __syncthreads();
    const uint32_t width = d * (P.order + 1);
    const bool f64 = (P.flags & kMfF64) != 0;
    for (uint32_t e = threadIdx.x; e < nf * w; e += kMfLanes) {
        const uint32_t f = e / w, col = e % w;
        const double *at = s_c + (f + (uint32_t)H) * w + col; // c'[t][i]; frame t + j lies j w doubles on
        const uint64_t o = (t0 + f) * width + col0 + col;
        for (uint32_t q = 0; q <= P.order; q++) {
            const double v = q == 0 ? at[0]
                                    : mfcc_delta(q == 1 ? P.s1 : P.s2, (int32_t)q * N,
                                                 [&](int32_t j) { return at[j * (int32_t)w]; });
            if (f64)
                ((double *)U.y)[o + (uint64_t)q * d] = v;
            else
                ((float *)U.y)[o + (uint64_t)q * d] = (float)v;
        }
    }
}

} // namespace

hipError_t launch_mfcc(const MfccParams &P, const MfccUtt *utts_dev, uint32_t n, uint64_t tiles, uint64_t blocks,
                       hipStream_t stream)
{
    if (n == 0 || tiles == 0)
        return hipSuccess;
    const uint64_t items = blocks * P.d, bgroups = (items + kMfLanes - 1) / kMfLanes;
    const uint64_t fgroups = ((uint64_t)n * P.d + kMfLanes - 1) / kMfLanes;
    if (tiles > 0x7fffffffull || bgroups > 0x7fffffffull || fgroups > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (P.n_ceps)
        hipLaunchKernelGGL(k_ceps, dim3((uint32_t)tiles), dim3(kMfLanes), 0, stream, P, utts_dev, n);
    for (uint32_t var = 0; var < P.cmvn; var++) { // the mean's pass; under MEAN_VAR the variance's behind it
        hipLaunchKernelGGL(k_mfcc_block, dim3((uint32_t)bgroups), dim3(kMfLanes), 0, stream, P, utts_dev, n, items, var);
        hipLaunchKernelGGL(k_mfcc_fold, dim3((uint32_t)fgroups), dim3(kMfLanes), 0, stream, P, utts_dev, n, var);
    }
    hipLaunchKernelGGL(k_delta, dim3((uint32_t)tiles, (P.d + kMfCols - 1) / kMfCols), dim3(kMfLanes), 0, stream, P,
                       utts_dev, n);
    return hipGetLastError();
}

namespace {

// The stage behind log-mel frames that stand on the device (unit u: T[u] frames at dL + loff[u] doubles), through ds;
// the outputs are handed out
int mfcc_run(DeviceScratch &ds, const MfccOpts &o, uint32_t n_mels, const double *dL, const std::vector<uint64_t> &loff,
             const std::vector<uint64_t> &T, uint8_t **out, size_t *n_bytes, const double *de = nullptr,
             const std::vector<uint64_t> *eoff = nullptr, const FbankGeom *g = nullptr)
{
    const size_t n = T.size();
    MfccTables tab;
    mfcc_tables(o, n_mels, &tab);
    MfccParams P = mfcc_params(o, n_mels, tab);
    if (g) // (the frames' energies at de + eoff[u], held to the filterbank's floor)
        P.e_floor = g->log_floor, P.e_ln_floor = g->ln_floor;
    const uint32_t d = P.d, width = mfcc_width(o, n_mels);
    std::vector<MfccUtt> utts(n);
    std::vector<PcmShare> shares(n);
    std::vector<uint64_t> coff(n);
    uint64_t bytes = 0, tiles = 0, blocks = 0, frames = 0;
    for (size_t u = 0; u < n; u++) {
        MfccUtt &w = utts[u];
        w.T = T[u];
        w.g0 = tiles;
        w.b0 = blocks;
        w.r_T = mfcc_r(T[u]);
        coff[u] = frames * d;
        shares[u] = {bytes, T[u] * width * mfcc_elem(o.flags)};
        bytes += (shares[u].n + 15) & ~(uint64_t)15;
        tiles += mfcc_tiles(T[u]);
        blocks += mfcc_blocks(T[u]);
        frames += T[u];
    }
    uint8_t *dy = ds.alloc<uint8_t>(std::max<uint64_t>(bytes, 16));
    double *dc = o.n_ceps ? ds.alloc<double>(frames * d) : nullptr;
    double *dbs = ds.alloc<double>(blocks * d), *dst = ds.alloc<double>(2 * n * d);
    const double *dDt = ds.upload(tab.Dt), *dlift = ds.upload(tab.lift);
    P.Dt = dDt;
    P.lift = dlift;
    for (size_t u = 0; u < n; u++) {
        MfccUtt &w = utts[u];
        w.L = dL + loff[u];
        w.c = o.n_ceps ? dc + coff[u] : const_cast<double *>(w.L);
        w.bs = dbs + w.b0 * d;
        w.stat = dst + 2 * u * d;
        w.y = dy + shares[u].off;
        w.e = de ? de + (*eoff)[u] : nullptr;
    }
    const MfccUtt *du = ds.upload(utts);
    if (ds.ok())
        ds.err = launch_mfcc(P, du, (uint32_t)n, tiles, blocks, ds.stream);
    std::vector<uint8_t> host;
    ds.read_back(&host, dy, bytes);
    if (const int rc = ds.status())
        return rc;
    return hand_out(host.data(), 1, shares, (void **)out, n_bytes);
}

// The whole stage on PCM the caller holds: fopts and o with the frame request fr (all zero: none), under the entry's name
int mfcc_pcm_run(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz, const FbankOpts *fopts,
                 const MfccOpts *o, const FrameOpts &fr, int32_t device, uint8_t **out, size_t *n_bytes, const char *who)
{
    int rc = mfcc_check_fbank(fopts, who);
    if (rc)
        return rc;
    const FbankOpts f = mfcc_fbank_opts(*fopts);
    if ((rc = mfcc_check_opts(o, f.n_mels, who)) || (rc = frame_check(&f, &fr, o->n_ceps >= 1, who)))
        return rc;
    if ((rc = pcm_check((const void *const *)in, n_in, n, hz && out && n_bytes, (void **)out, n_bytes)))
        return rc;
    // (every rate's geometry and every unit's frames before a device is touched)
    FbankPass pass;
    pass.start(f, fr);
    for (size_t u = 0; u < n; u++)
        if ((rc = pass.add(hz[u], n_in[u], who)))
            return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    // the filterbank pass as jb_fbank_pcm_batch runs it (RatePass, jb_host.h), its f64 logarithms into a slab of the
    // call (a unit's frames on a 16-byte boundary), then the cepstral kernels behind it on the same stream
    std::vector<uint64_t> xoff;
    const double *dx = ds.pack(in, n_in, n, &xoff);
    const bool energy = (fr.flags & kFrEnergy) != 0;
    std::vector<uint64_t> loff(n), eoff(n), T(n);
    uint64_t words = 0, frames = 0;
    for (size_t u = 0; u < n; u++) {
        T[u] = pass.list.host[u].T;
        loff[u] = words;
        eoff[u] = frames;
        words += (T[u] * f.n_mels + 1) & ~(uint64_t)1;
        frames += T[u];
    }
    double *dL = ds.alloc<double>(std::max<uint64_t>(words, 2));
    double *de = energy ? ds.alloc<double>(std::max<uint64_t>(frames, 1)) : nullptr;
    for (size_t u = 0; u < n; u++) {
        pass.list.host[u].x = dx + xoff[u];
        pass.list.host[u].y = (uint8_t *)(dL + loff[u]);
        pass.list.host[u].e = de ? de + eoff[u] : nullptr;
    }
    pass.bind(ds, who);
    if (ds.ok())
        ds.err = pass.launch(ds.stream);
    // (the pass lives to the wait inside mfcc_run)
    return mfcc_run(ds, *o, f.n_mels, dL, loff, T, out, n_bytes, de, &eoff, n && de ? &pass.cls.geom[0] : nullptr);
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_mfcc_frames_batch(const double *const *L, const size_t *T, size_t n, uint32_t n_mels, const jb_mfcc_opts *opts,
                         int32_t device, uint8_t **out, size_t *n_bytes)
{
    const MfccOpts *o = (const MfccOpts *)opts;
    int rc = mfcc_check_opts(o, n_mels, "jb_mfcc_frames_batch");
    if (rc)
        return rc;
    if (n && (!T || !out || !n_bytes))
        return JB_ERR_INVALID;
    std::vector<size_t> n_in(n);
    std::vector<uint64_t> frames(n);
    for (size_t u = 0; u < n; u++) {
        frames[u] = T[u];
        n_in[u] = T[u] * (size_t)n_mels;
    }
    if ((rc = pcm_check((const void *const *)L, n_in.data(), n, true, (void **)out, n_bytes)))
        return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, "jb_mfcc_frames_batch")))
        return rc;
    std::vector<uint64_t> loff;
    const double *dL = ds.pack(L, n_in.data(), n, &loff);
    return mfcc_run(ds, *o, n_mels, dL, loff, frames, out, n_bytes);
}

int jb_mfcc_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                      const jb_fbank_opts *fopts, const jb_mfcc_opts *opts, int32_t device, uint8_t **out,
                      size_t *n_bytes)
{
    return mfcc_pcm_run(in, n_in, n, hz, (const FbankOpts *)fopts, (const MfccOpts *)opts, FrameOpts{}, device, out,
                        n_bytes, "jb_mfcc_pcm_batch");
}

int jb_mfcc_framed_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                             const jb_fbank_opts *fopts, const jb_mfcc_opts *opts, const jb_frame_opts *fr,
                             int32_t device, uint8_t **out, size_t *n_bytes)
{
    if (!fr) {
        set_error("jb_mfcc_framed_pcm_batch: the frame request is NULL");
        return JB_ERR_INVALID;
    }
    return mfcc_pcm_run(in, n_in, n, hz, (const FbankOpts *)fopts, (const MfccOpts *)opts, *(const FrameOpts *)fr,
                        device, out, n_bytes, "jb_mfcc_framed_pcm_batch");
}

} // extern "C"

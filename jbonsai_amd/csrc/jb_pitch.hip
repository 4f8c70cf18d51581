// jb_pitch.hip -- the pitch stage on the device: the pitch columns of every unit by the rules of jb_pitch.h.
//
//   k_pitch_down   one workgroup per tile of kPitchTile samples of a unit's 4 kHz signal, the rate's phase table staged
//               in LDS.  Lane l forms the (at most four) samples 1024 i + l + 256 j of its partial of the sums, each
//               from +0.0 over its taps in ascending k, stores them and folds the 256 partials 128, 64, .., 1 in LDS:
//               pitch_partial's additions in pitch_partial's order.  The tile's two sums go to the unit's scratch; the
//               tracker adds the tiles in ascending order.
//   k_pitch_track  one workgroup of kPitchTrackLanes per unit, serial over its frames.  Per frame: the wl4 + b samples
//               into LDS (zeros outside the unit), the mean on wave 0, then a wave per integer lag: lane j sums the
//               products i = j mod 64 in ascending i from 0.0 and the lanes fold 32, 16, .., 1 (frame_sum's additions
//               in frame_sum's order) for inner_L and e_L; q_L goes to LDS.  Then a lane per grid lag: Q_i over its at
//               most 11 taps, the exact minimum over all S predecessors by brute force (F in LDS, every lane reads the
//               same F[j]: a broadcast), the choice as 16 bits to the unit's [T][S] scratch, and the block's minimum
//               taken off.  Lane 0 walks the choices back at the end.  The brute-force step is S^2 add-compares per
//               frame (174k at the defaults) behind six barriers: the kernel is bound by that step's latency on one
//               CU, and a call of one long unit runs on one workgroup.
//   k_pitch_post   a wave per frame: the frame's NCCF again, at the at most 11 integer lags under the chosen grid lag
//               alone, for p there (the same additions as the tracker's, so the same bits) and its weight pi; with
//               JB_PITCH_RAW the row is written here.
//   k_pitch_cols   a lane per frame: step 6 (pitch_columns) from the frames' lags, p and pi.
#include "jb_host.h"

#include <algorithm>
#include <map>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

// The unit of workgroup idx of a list whose prefix sums are pre(unit): the last one with pre <= idx
template <class P> __device__ __forceinline__ uint32_t pitch_find(const PitchUtt *utts, uint32_t n, uint64_t idx, P pre)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre(utts[mid]) <= idx)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// frame_sum's fold of the 64 partials; every lane gets the sum
__device__ __forceinline__ double pitch_fold(double p)
{
#pragma unroll
    for (int w = 32; w > 0; w >>= 1)
        p = p + __shfl_down(p, w, 64);
    return __shfl(p, 0, 64);
}

__global__ __launch_bounds__(kPitchLanes) void k_pitch_down(const PitchUtt *__restrict__ utts, uint32_t n_utts)
{
    __shared__ double W[kPitchMaxDown];
    __shared__ double r1[kPitchLanes], r2[kPitchLanes];
    const uint32_t ui = pitch_find(utts, n_utts, blockIdx.x, [](const PitchUtt &u) { return u.t0; });
    const PitchUtt U = utts[ui];
    const uint64_t tile = blockIdx.x - U.t0;
    if (tile >= pitch_tiles(U.n4))
        return;
    const uint32_t tid = threadIdx.x, nw = U.P * (2 * U.D + 1); // <= kPitchMaxDown by pitch_down_fault
    for (uint32_t i = tid; i < nw; i += kPitchLanes)
        W[i] = U.W[i];
    __syncthreads();
    double s1, s2;
    pitch_partial(
        U.n4, tile, tid,
        [&](uint64_t m) {
            const double y = pitch_down_sample(m, U.n, U.hzp, U.P, U.D, W, [&](uint64_t k) { return U.x[k]; });
            U.y4[m] = y;
            return y;
        },
        &s1, &s2);
    r1[tid] = s1;
    r2[tid] = s2;
    __syncthreads();
    for (uint32_t h = kPitchLanes / 2; h; h >>= 1) {
        if (tid < h) {
            r1[tid] = r1[tid] + r1[tid + h];
            r2[tid] = r2[tid] + r2[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        U.tile[2 * tile] = r1[0];
        U.tile[2 * tile + 1] = r2[0];
    }
}

// The frame's samples from s0 into v[0..span): zeros outside [0, n4)
__device__ __forceinline__ void pitch_stage(const double *__restrict__ y, uint64_t n4, int64_t s0, uint32_t span, double *v,
                                            uint32_t first, uint32_t step)
{
    for (uint32_t i = first; i < span; i += step) {
        const int64_t k = s0 + (int64_t)i;
        v[i] = k >= 0 && (uint64_t)k < n4 ? y[k] : 0.0;
    }
}

__global__ __launch_bounds__(kPitchTrackLanes) void k_pitch_track(const PitchUtt *__restrict__ utts, const PitchClass C)
{
    __shared__ double v[kPitchMaxWin + kPitchMaxLag + 1];
    __shared__ double q[kPitchMaxLag + 1];
    __shared__ double F[2][kPitchMaxStates];
    __shared__ double red[kPitchTrackLanes / 64];
    __shared__ double sh[2];
    const PitchUtt U = utts[blockIdx.x];
    if (U.T == 0)
        return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    constexpr uint32_t kWaves = kPitchTrackLanes / 64;
    const uint32_t S = C.S, wl4 = C.wl4, span = C.wl4 + C.b;
    if (tid == 0) {
        double S1 = 0.0, S2 = 0.0;
        const uint64_t tiles = pitch_tiles(U.n4);
        for (uint64_t i = 0; i < tiles; i++) {
            S1 = i ? S1 + U.tile[2 * i] : U.tile[0];
            S2 = i ? S2 + U.tile[2 * i + 1] : U.tile[1];
        }
        sh[1] = pitch_ballast(S1, S2, U.n4, wl4, C.ballast);
    }
    for (uint32_t i = tid; i < S; i += kPitchTrackLanes)
        F[0][i] = 0.0;
    __syncthreads();
    const double B = sh[1];
    uint32_t cur = 0;
    for (uint64_t t = 0; t < U.T; t++) {
        pitch_stage(U.y4, U.n4, pitch_start(C.grid, t, wl4, C.sh4), span, v, tid, kPitchTrackLanes);
        __syncthreads();
        if (wave == 0) {
            double p = 0.0;
            for (uint32_t i = lane; i < wl4; i += 64)
                p = p + v[i];
            p = pitch_fold(p);
            if (lane == 0)
                sh[0] = p / (double)wl4;
        }
        __syncthreads();
        const double mean = sh[0];
        for (uint32_t i = tid; i < span; i += kPitchTrackLanes)
            v[i] = v[i] - mean;
        __syncthreads();
        double e0 = 0.0;
        for (uint32_t i = lane; i < wl4; i += 64) {
            const double s = v[i] * v[i];
            e0 = e0 + s;
        }
        e0 = pitch_fold(e0);
        for (uint32_t L = C.a + wave; L <= C.b; L += kWaves) {
            double in = 0.0, eL = 0.0;
            for (uint32_t i = lane; i < wl4; i += 64) {
                const double x0 = v[i], xL = v[i + L], s = x0 * xL, s2 = xL * xL;
                in = in + s;
                eL = eL + s2;
            }
            in = pitch_fold(in);
            eL = pitch_fold(eL);
            if (lane == 0)
                q[L - C.a] = pitch_nccf(in, e0, eL, B);
        }
        __syncthreads();
        const double *Fp = F[cur];
        double *Fn = F[cur ^ 1];
        double m = (double)INFINITY;
        for (uint32_t i = tid; i < S; i += kPitchTrackLanes) {
            const uint32_t k0 = C.tap[i] & 0xffffu, cnt = C.tap[i] >> 16;
            double Q = 0.0;
            for (uint32_t k = 0; k < cnt; k++) {
                const double s = q[k0 + k] * C.G[(size_t)i * kPitchTaps + k];
                Q = Q + s;
            }
            double best = pitch_cand(Fp[0], C.kappa, i, 0);
            uint32_t bj = 0;
            for (uint32_t j = 1; j < S; j++) {
                const double c = pitch_cand(Fp[j], C.kappa, i, j);
                if (c < best) {
                    best = c;
                    bj = j;
                }
            }
            const double fn = best + pitch_local(Q, C.soft[i]);
            Fn[i] = fn;
            U.choice[t * S + i] = (uint16_t)bj;
            m = fn < m ? fn : m;
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
            const double o = __shfl_xor(m, w, 64);
            m = o < m ? o : m;
        }
        if (lane == 0)
            red[wave] = m;
        __syncthreads();
        double mn = red[0];
        for (uint32_t w = 1; w < kWaves; w++)
            mn = red[w] < mn ? red[w] : mn;
        for (uint32_t i = tid; i < S; i += kPitchTrackLanes)
            Fn[i] = Fn[i] - mn;
        cur ^= 1;
        __syncthreads();
    }
    if (tid == 0) {
        const double *Fl = F[cur];
        uint32_t s = 0;
        for (uint32_t i = 1; i < S; i++)
            if (Fl[i] < Fl[s])
                s = i;
        for (uint64_t t = U.T; t-- > 0;) {
            U.idx[t] = s;
            s = U.choice[t * S + s];
        }
    }
}

template <class T> __device__ __forceinline__ void pitch_store(uint8_t *out, uint64_t t, uint32_t width, const double *c)
{
    T *row = (T *)out + t * width;
    for (uint32_t k = 0; k < width; k++)
        row[k] = (T)c[k];
}

__global__ __launch_bounds__(kPitchLanes) void k_pitch_post(const PitchUtt *__restrict__ utts, uint32_t n_utts,
                                                            const PitchClass C)
{
    __shared__ double vs[kPitchPostFrames][kPitchMaxWin + kPitchMaxLag + 1];
    const uint32_t ui = pitch_find(utts, n_utts, blockIdx.x, [](const PitchUtt &u) { return u.g0; });
    const PitchUtt U = utts[ui];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t t = (blockIdx.x - U.g0) * kPitchPostFrames + wave;
    const bool on = t < U.T; // (every wave keeps to the barriers)
    double *v = vs[wave];
    const uint32_t wl4 = C.wl4, span = C.wl4 + C.b;
    if (on)
        pitch_stage(U.y4, U.n4, pitch_start(C.grid, t, wl4, C.sh4), span, v, lane, 64);
    __syncthreads();
    double mean = 0.0;
    if (on) {
        double p = 0.0;
        for (uint32_t i = lane; i < wl4; i += 64)
            p = p + v[i];
        mean = pitch_fold(p) / (double)wl4;
    }
    __syncthreads();
    if (on)
        for (uint32_t i = lane; i < span; i += 64)
            v[i] = v[i] - mean;
    __syncthreads();
    if (!on)
        return;
    double e0 = 0.0;
    for (uint32_t i = lane; i < wl4; i += 64) {
        const double s = v[i] * v[i];
        e0 = e0 + s;
    }
    e0 = pitch_fold(e0);
    const uint32_t si = U.idx[t], k0 = C.tap[si] & 0xffffu, cnt = C.tap[si] >> 16;
    double ap = 0.0;
    for (uint32_t k = 0; k < cnt; k++) {
        const uint32_t L = C.a + k0 + k;
        double in = 0.0, eL = 0.0;
        for (uint32_t i = lane; i < wl4; i += 64) {
            const double x0 = v[i], xL = v[i + L], s = x0 * xL, s2 = xL * xL;
            in = in + s;
            eL = eL + s2;
        }
        in = pitch_fold(in);
        eL = pitch_fold(eL);
        const double s = pitch_nccf(in, e0, eL, 0.0) * C.G[(size_t)si * kPitchTaps + k];
        ap = ap + s;
    }
    if (lane == 0) {
        U.pv[t] = ap;
        if (C.flags & kPitchRaw) {
            const double c[2] = {ap, C.inv_lag[si]};
            if (C.flags & kPitchF64)
                pitch_store<double>(U.out, t, 2, c);
            else
                pitch_store<float>(U.out, t, 2, c);
        } else {
            U.pw[t] = pitch_pov_weight(ap);
        }
    }
}

__global__ __launch_bounds__(kPitchLanes) void k_pitch_cols(const PitchUtt *__restrict__ utts, uint32_t n_utts,
                                                            const PitchClass C)
{
    const uint32_t ui = pitch_find(utts, n_utts, blockIdx.x, [](const PitchUtt &u) { return u.c0; });
    const PitchUtt U = utts[ui];
    const uint64_t t = (blockIdx.x - U.c0) * kPitchLanes + threadIdx.x;
    if (t >= U.T)
        return;
    const uint32_t width = pitch_width(C.flags);
    double c[4];
    pitch_columns(t, U.T, U.idx, U.pv, U.pw, C.log_pitch, C.pov_scale, C.pitch_scale, C.delta_scale, C.left, C.right,
                  width, c);
    if (C.flags & kPitchF64)
        pitch_store<double>(U.out, t, width, c);
    else
        pitch_store<float>(U.out, t, width, c);
}

} // namespace

hipError_t launch_pitch(const PitchUtt *utts_dev, uint32_t n_utts, uint64_t tiles, uint64_t post_wgs, uint64_t cols_wgs,
                        const PitchClass &cls, hipStream_t stream)
{
    if (tiles > 0x7fffffffull || post_wgs > 0x7fffffffull || cols_wgs > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (!n_utts)
        return hipSuccess;
    if (tiles)
        hipLaunchKernelGGL(k_pitch_down, dim3((uint32_t)tiles), dim3(kPitchLanes), 0, stream, utts_dev, n_utts);
    if (post_wgs) {
        hipLaunchKernelGGL(k_pitch_track, dim3(n_utts), dim3(kPitchTrackLanes), 0, stream, utts_dev, cls);
        hipLaunchKernelGGL(k_pitch_post, dim3((uint32_t)post_wgs), dim3(kPitchLanes), 0, stream, utts_dev, n_utts, cls);
        if (!(cls.flags & kPitchRaw))
            hipLaunchKernelGGL(k_pitch_cols, dim3((uint32_t)cols_wgs), dim3(kPitchLanes), 0, stream, utts_dev, n_utts, cls);
    }
    return hipGetLastError();
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_pitch_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                       const jb_pitch_opts *opts, int32_t device, void **out, uint64_t *T, uint32_t *width,
                       uint32_t **lag_index)
{
    const char *who = "jb_pitch_pcm_batch";
    int rc = pcm_check((const void *const *)in, n_in, n, out && hz, out, nullptr);
    if (rc)
        return rc;
    for (size_t u = 0; u < n && lag_index; u++)
        lag_index[u] = nullptr;
    const PitchOpts *o = (const PitchOpts *)opts;
    PitchGrid g;
    if ((rc = pitch_check_opts(o, who, &g)))
        return rc;
    // the units' geometry, the distinct rates' phase tables and the slabs' layout
    std::vector<jb_pitch_geometry_t> geo(n);
    std::map<uint32_t, size_t> table_of; // rate -> its table's first weight
    std::vector<double> tables;
    std::vector<PitchDown> downs(n);
    std::vector<uint64_t> out_off(n + 1, 0), y_off(n + 1, 0), tile_off(n + 1, 0), fr_off(n + 1, 0), w_off(n);
    uint64_t tiles = 0, post_wgs = 0, cols_wgs = 0;
    std::vector<PitchUtt> utts(n);
    for (size_t u = 0; u < n; u++) {
        if ((rc = pitch_check_rate(hz[u], u, who, &downs[u])))
            return rc;
        if (!table_of.count(hz[u])) {
            table_of[hz[u]] = tables.size();
            tables.insert(tables.end(), downs[u].W.begin(), downs[u].W.end());
        }
        w_off[u] = table_of[hz[u]];
        geo[u] = pitch_geometry_of(*o, g, hz[u], n_in[u]);
        const uint64_t bytes = geo[u].T * geo[u].width * geo[u].elem;
        out_off[u + 1] = out_off[u] + ((bytes + 15) & ~15ull);
        y_off[u + 1] = y_off[u] + geo[u].n4;
        tile_off[u + 1] = tile_off[u] + pitch_tiles(geo[u].n4);
        fr_off[u + 1] = fr_off[u] + geo[u].T;
        if (fr_off[u + 1] > kPitchMaxScratch / pitch_choice_bytes(g.S)) {
            set_error(std::string(who) + ": the tracker's choices (" + std::to_string(pitch_choice_bytes(g.S)) +
                      " bytes per frame) pass JB_PITCH_MAX_SCRATCH");
            return JB_ERR_UNSUPPORTED;
        }
        utts[u].t0 = tiles;
        utts[u].g0 = post_wgs;
        utts[u].c0 = cols_wgs;
        tiles += pitch_tiles(geo[u].n4);
        post_wgs += pitch_post_wgs(geo[u].T);
        cols_wgs += pitch_cols_wgs(geo[u].T);
    }
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    std::vector<uint64_t> xoff;
    const double *dx = ds.pack(in, n_in, n, &xoff);
    const uint64_t frames = fr_off[n];
    uint8_t *dout = ds.alloc<uint8_t>(out_off[n]);
    double *dy = ds.alloc<double>(y_off[n]);
    double *dtile = ds.alloc<double>(2 * tile_off[n]);
    uint16_t *dchoice = ds.alloc<uint16_t>(frames * g.S);
    uint32_t *didx = ds.alloc<uint32_t>(frames);
    double *dpv = ds.alloc<double>(frames), *dpw = ds.alloc<double>(frames);
    const double *dW = ds.upload(tables);
    PitchClass C{};
    C.G = ds.upload(g.G);
    C.soft = ds.upload(g.soft);
    C.inv_lag = ds.upload(g.inv_lag);
    C.log_pitch = ds.upload(g.log_pitch);
    C.tap = ds.upload(g.tap);
    C.kappa = g.kappa;
    C.ballast = o->nccf_ballast;
    C.pov_scale = o->pov_scale;
    C.pitch_scale = o->pitch_scale;
    C.delta_scale = o->delta_scale;
    C.S = g.S;
    C.a = g.a;
    C.b = g.b;
    C.wl4 = g.wl4;
    C.sh4 = g.sh4;
    C.grid = o->grid;
    C.flags = o->flags;
    C.left = o->norm_left;
    C.right = o->norm_right;
    for (size_t u = 0; u < n && ds.ok(); u++) {
        PitchUtt &U = utts[u];
        U.x = dx + xoff[u];
        U.W = dW + w_off[u];
        U.y4 = dy + y_off[u];
        U.tile = dtile + 2 * tile_off[u];
        U.choice = dchoice + fr_off[u] * g.S;
        U.idx = didx + fr_off[u];
        U.pv = dpv + fr_off[u];
        U.pw = dpw + fr_off[u];
        U.out = dout + out_off[u];
        U.n = n_in[u];
        U.n4 = geo[u].n4;
        U.T = geo[u].T;
        U.hzp = downs[u].hzp;
        U.P = downs[u].P;
        U.D = downs[u].D;
    }
    const PitchUtt *dutts = ds.upload(utts);
    if (ds.ok())
        ds.err = launch_pitch(dutts, (uint32_t)n, tiles, post_wgs, cols_wgs, C, ds.stream);
    std::vector<uint8_t> host;
    std::vector<uint32_t> idx;
    ds.read_back(&host, (const uint8_t *)dout, out_off[n]);
    ds.read_back(&idx, (const uint32_t *)didx, frames);
    if ((rc = ds.status()))
        return rc;
    std::vector<PcmShare> shares(n);
    for (size_t u = 0; u < n; u++)
        shares[u] = {out_off[u], geo[u].T * geo[u].width * geo[u].elem};
    if ((rc = hand_out(host.data(), 1, shares, out, nullptr)))
        return rc;
    if (lag_index) {
        for (size_t u = 0; u < n; u++)
            shares[u] = {fr_off[u], geo[u].T};
        if ((rc = hand_out(idx.data(), sizeof(uint32_t), shares, (void **)lag_index, nullptr))) {
            for (size_t u = 0; u < n; u++) {
                free(out[u]);
                out[u] = nullptr;
            }
            return rc;
        }
    }
    for (size_t u = 0; u < n; u++) {
        if (T)
            T[u] = geo[u].T;
        if (width)
            width[u] = geo[u].width;
    }
    return JB_OK;
}

} // extern "C"

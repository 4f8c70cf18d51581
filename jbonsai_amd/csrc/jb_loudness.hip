// Loudness normalization of synthesized PCM (new surface: the reference's only level control is the fixed
// `volume` gain).  The definition is in include/jbonsai_amd.h ("loudness"); in short: K-weighting (two biquads,
// BS.1770-4) of x / 32768 from zero state per utterance, hop sums z_j of y^2 over [jH, (j+1)H), H = (fs + 5) / 10,
// four-hop gating blocks, the -70 LUFS absolute and the -10 LU relative gate, the sample peak, and
// gain_dB = min(T - L, C - P) over the finite terms; in true-peak mode (JB_PEAK_TRUE) the true peak TP, the largest
// magnitude of x and of its F - 1 interpolated phases (12 taps each), stands in for P in that rule.
//
// The filter is linear and time-invariant, so a recursion cut into pieces is exact up to rounding: a piece filtered
// from zero state ends in e, and the state s at its start carries over as s -> A^len s + e (A: the 4x4 transition of
// one sample with x = 0, len: the piece's length).  Between pieces a state travels in the coordinates of ln_to_scan
// and the powers of A are made on the host in extended precision (mat_pow): both for the same reason, a DC offset
// that the high-pass holds as two large states of opposite sign.  Five kernels measure, one applies:
//   k_ln_tiles<false>  one workgroup per tile (<= 256 segments of S <= 16 samples, inside one hop): the tile is staged
//                      through LDS with coalesced loads (the sample peak on the way), every lane filters its segment
//                      from zero, a Hillis-Steele scan of the affine maps across the 256 lanes (matrices A^(S 2^k),
//                      wave-uniform) gives each segment's start state for a zero tile start, and the last lane
//                      filters its segment again: the tile's zero-state end state.
//   k_ln_scan          one wave per utterance: tiles fold into hops (A^G, A^r), hops into 64 lane chunks (A^H), a
//                      shuffle scan across the lanes (powers of A^(H c)), then each lane walks its chunk again and
//                      leaves every tile's true start state where its end state was.
//   k_ln_tiles<true>   the tile again, the same zero-state pass and scan, now from the tile's true start state;
//                      every lane filters its segment from its start state and sums y^2; a fixed tree gives the
//                      tile's share of its hop's z (tiles of the tail hop, in no block, are skipped).
//   k_ln_true_peak     (launched only with an utterance in true-peak mode; others' tiles return at once) the tile
//                      and a halo of 5 samples before and 6 after in LDS, zero outside the utterance; a lane takes
//                      samples l, l + 256, ..., holds the 12-sample window in registers and runs the phases with
//                      wave-uniform taps (scalar operands), each y one fixed FMA chain; a fixed fmax tree gives the
//                      tile's largest |y|.
//   k_ln_gate          one workgroup per utterance: z_j, the blocks, both gates, L, P, TP and the gain, every sum in
//                      a fixed order over a fixed thread count.
//   k_ln_apply         y = x * g, f64 or the 16-bit sink's rule (clamp, then truncate).
// Each sample is read from HBM twice to measure (both tile passes; a third time in true-peak mode) and once to apply.
// Every result is a function of
// the utterance's samples and rate alone: the tiling depends on nothing else (the fast invariant mode stays
// invariant).
#include "jb_host.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace jb {

namespace {
constexpr uint32_t kLnMaxS = 16; // samples per segment at most (tiles of at most 4096 samples)
constexpr uint32_t kLnMaxHop = 61439; // tph = ceil(H / 4096) <= 15: the hop's last tile is never empty
constexpr double kLnShelfHz = 1681.974450955533; // the shelf's centre: K = tan(pi fc / fs) > 0 only below Nyquist
using M4 = double[16];

// One sample through both stages (transposed direct form II); c: b0 b1 b2 a1 a2 of stage 1, then of stage 2
inline double host_step(const double *c, double *s, double x)
{
    const double w = std::fma(c[0], x, s[0]);
    s[0] = std::fma(c[1], x, std::fma(-c[3], w, s[1]));
    s[1] = std::fma(c[2], x, -c[4] * w);
    const double y = std::fma(c[5], w, s[2]);
    s[2] = std::fma(c[6], w, std::fma(-c[8], y, s[3]));
    s[3] = std::fma(c[7], w, -c[9] * y);
    return y;
}

void mat_mul(const long double *a, const long double *b, long double *out)
{
    long double t[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            long double acc = 0.0L;
            for (int k = 0; k < 4; k++)
                acc += a[i * 4 + k] * b[k * 4 + j];
            t[i * 4 + j] = acc;
        }
    std::copy(t, t + 16, out);
}

// A^n by squaring in extended precision, rounded once (as jb_filter.cpp's tables).  The high-pass has a nearly double
// pole at 1: what one entry of A^n is off by is carried for another 1 / (1 - r) samples, times a state of the size of
// x, into an output several hundred times smaller than that state.  Squared in f64 the powers cost 1e-9 LU on a DC
// offset at 48 kHz, 50 times what a serial f64 recursion loses (tests/test_gpu_loudness_ld.py,
// profiles/loudness_ld.txt)
void mat_pow(const double *a, uint64_t n, double *out)
{
    long double r[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, p[16];
    std::copy(a, a + 16, p);
    for (; n; n >>= 1) {
        if (n & 1)
            mat_mul(r, p, r);
        if (n > 1)
            mat_mul(p, p, p);
    }
    for (int i = 0; i < 16; i++)
        out[i] = (double)r[i];
}

double tp_bessel_i0(double x)
{
    // power series sum_k ((x/2)^k / k!)^2, as the resampler's table: 60 terms reach the rounding floor for x <= 10
    double sum = 1.0, term = 1.0;
    const double h = 0.25 * x * x;
    for (int k = 1; k < 60; k++) {
        term *= h / ((double)k * (double)k);
        sum += term;
    }
    return sum;
}
} // namespace

int true_peak_table(uint32_t hz, uint32_t *F, double *taps)
{
    if (hz == 0) {
        set_error("true peak: a rate of 0 Hz");
        return JB_ERR_INVALID;
    }
    const uint32_t f = std::min<uint32_t>(kTpMaxF, (192000u + hz - 1) / hz);
    if (F)
        *F = f;
    if (!taps)
        return JB_OK;
    const double i0b = tp_bessel_i0(8.0), pi = 3.14159265358979323846;
    for (uint32_t p = 1; p < f; p++)
        for (uint32_t j = 0; j < kTpTaps; j++) {
            const double t = (double)p / (double)f + 5.0 - (double)j; // never 0, always inside (-6, 6)
            const double u = t / 6.0;
            taps[(size_t)(p - 1) * kTpTaps + j] =
                std::sin(pi * t) / (pi * t) * tp_bessel_i0(8.0 * std::sqrt(1.0 - u * u)) / i0b;
        }
    return JB_OK;
}

int loudness_filter(uint32_t hz, double b[6], double a[6], uint32_t *hop)
{
    if (hz == 0) {
        set_error("loudness: a rate of 0 Hz");
        return JB_ERR_INVALID;
    }
    const double fs = (double)hz;
    auto stage = [&](double fc, double Q, double *bb, double *aa, bool shelf) {
        const double K = std::tan(M_PI * fc / fs);
        const double a0 = 1.0 + K / Q + K * K;
        if (shelf) {
            const double Vh = std::pow(10.0, 3.999843853973347 / 20.0);
            const double Vb = std::pow(Vh, 0.4996667741545416);
            bb[0] = (Vh + Vb * K / Q + K * K) / a0;
            bb[1] = 2.0 * (K * K - Vh) / a0;
            bb[2] = (Vh - Vb * K / Q + K * K) / a0;
        } else {
            bb[0] = 1.0;
            bb[1] = -2.0;
            bb[2] = 1.0;
        }
        aa[0] = 1.0;
        aa[1] = 2.0 * (K * K - 1.0) / a0;
        aa[2] = (1.0 - K / Q + K * K) / a0;
    };
    double bb[6], aa[6];
    stage(kLnShelfHz, 0.7071752369554196, bb, aa, true);
    stage(38.13547087602444, 0.5003270373238773, bb + 3, aa + 3, false);
    if (b)
        std::copy(bb, bb + 6, b);
    if (a)
        std::copy(aa, aa + 6, a);
    if (hop)
        *hop = (hz + 5) / 10;
    return JB_OK;
}

int loudness_measurable(uint32_t hz)
{
    if (hz == 0 || 2.0 * kLnShelfHz < (double)hz)
        return JB_OK;
    set_error("loudness: at " + std::to_string(hz) + " Hz the shelf's centre (1681.97 Hz) is not below Nyquist (" +
              std::to_string(hz / 2) + (hz % 2 ? ".5" : "") + " Hz): the K-weighting is unstable; 3364 Hz and up are "
              "measured");
    return JB_ERR_UNSUPPORTED;
}

int loudness_rate(uint32_t hz, LoudnessRate *out)
{
    LoudnessRate r{};
    uint32_t H = 0;
    int rc = loudness_filter(hz, r.b, r.a, &H);
    if (rc)
        return rc;
    if (H == 0 || H > kLnMaxHop) {
        set_error("loudness: " + std::to_string(hz) + " Hz gives a hop of " + std::to_string(H) +
                  " samples (1.." + std::to_string(kLnMaxHop) + " are measured)");
        return JB_ERR_UNSUPPORTED;
    }
    if ((rc = true_peak_table(hz, &r.F, r.tp)))
        return rc;
    r.hz = hz;
    r.H = H;
    r.tph = (H + 4095) / 4096;
    r.S = (H + kLnLanes * r.tph - 1) / (kLnLanes * r.tph);
    r.G = kLnLanes * r.S;
    const uint64_t last = (uint64_t)H - (uint64_t)(r.tph - 1) * r.G;
    if (r.S > kLnMaxS || (uint64_t)(r.tph - 1) * r.G >= H || last > r.G) {
        set_error("loudness: no tiling for a hop of " + std::to_string(H));
        return JB_ERR_UNSUPPORTED;
    }
    // A: one sample with x = 0, column j from the unit state e_j -- the device's recursion, term for term -- in the
    // scan's coordinates (ln_to_scan): e_3 there is (t0, t1) = (-1, 1), and the image's pair is summed again
    const double c[10] = {r.b[0], r.b[1], r.b[2], r.a[1], r.a[2], r.b[3], r.b[4], r.b[5], r.a[4], r.a[5]};
    double A[16];
    for (int j = 0; j < 4; j++) {
        double s[4] = {0, 0, 0, 0};
        s[j] = 1.0;
        if (j == 3)
            s[2] = -1.0;
        host_step(c, s, 0.0);
        s[2] += s[3];
        for (int i = 0; i < 4; i++)
            A[i * 4 + j] = s[i];
    }
    for (int k = 0; k < 8; k++)
        mat_pow(A, (uint64_t)r.S << k, r.P[k]);
    mat_pow(A, r.G, r.Pt);
    mat_pow(A, last, r.Pr);
    mat_pow(A, H, r.Ph);
    *out = r;
    return JB_OK;
}

uint32_t loudness_tiles(const LoudnessRate &r, uint64_t n)
{
    if (n == 0)
        return 0;
    const uint64_t nh = (n + r.H - 1) / r.H;   // hops, the tail's included
    const uint64_t rem = n - (nh - 1) * r.H;   // samples of the last hop, 1..H
    return (uint32_t)((nh - 1) * r.tph + (rem + r.G - 1) / r.G);
}

// ---------------------------------------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) double cdouble;

__device__ __forceinline__ double ln_step(const double *c, double *s, double x)
{
    const double w = __builtin_fma(c[0], x, s[0]);
    s[0] = __builtin_fma(c[1], x, __builtin_fma(-c[3], w, s[1]));
    s[1] = __builtin_fma(c[2], x, -c[4] * w);
    const double y = __builtin_fma(c[5], w, s[2]);
    s[2] = __builtin_fma(c[6], w, __builtin_fma(-c[8], y, s[3]));
    s[3] = __builtin_fma(c[7], w, -c[9] * y);
    return y;
}

// The coordinates in which states are carried between pieces (sc, st, every matrix of LoudnessRate): the high-pass
// pair (t0, t1) as (t0 + t1, t1).  The high-pass has a nearly double pole at 1 and a DC offset c in its input sits in
// the pair as (-c, c).  In the recursion's own coordinates A^n has entries of size n that map that state by a
// difference of products n c, rounded at eps n c, and what is lost there lives on for another 1 / (1 - r) samples of
// an output that is several hundred times smaller than c.  In these coordinates the sum is 0 for the offset (exact:
// the two are within a factor of 2), the entries that meet t1 are small, and no product is larger than its result
__device__ __forceinline__ void ln_to_scan(double *s) { s[2] += s[3]; }
__device__ __forceinline__ void ln_from_scan(double *s) { s[2] -= s[3]; }

// v += P w (P wave-uniform: scalar operands)
__device__ __forceinline__ void ln_mv_add(cdouble *P, const double *w, double *v)
{
    for (int i = 0; i < 4; i++) {
        double acc = v[i];
        for (int k = 0; k < 4; k++)
            acc = __builtin_fma(P[i * 4 + k], w[k], acc);
        v[i] = acc;
    }
}

__device__ __forceinline__ void ln_coefs(const LoudnessRate *R, double *c)
{
    cdouble *b = (cdouble *)R->b, *a = (cdouble *)R->a;
    c[0] = b[0], c[1] = b[1], c[2] = b[2], c[3] = a[1], c[4] = a[2];
    c[5] = b[3], c[6] = b[4], c[7] = b[5], c[8] = a[4], c[9] = a[5];
}

template <bool kZ>
__global__ __launch_bounds__(kLnLanes) void k_ln_tiles(const LoudnessRate *__restrict__ rates,
                                                       const LoudnessUtt *__restrict__ utts, uint32_t n_utts,
                                                       double *__restrict__ st, double *__restrict__ pk,
                                                       double *__restrict__ z)
{
    __shared__ double xs[kLnLanes * (kLnMaxS + 1)]; // lane l's segment at l * (S | 1): odd strides, no bank conflict
    __shared__ double sc[kLnLanes * 4];
    __shared__ double red[kLnLanes];
    const uint32_t tid = threadIdx.x;
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x, &LoudnessUtt::lt0);
    const LoudnessUtt U = utts[u];
    const LoudnessRate *R = rates + U.rate;
    const uint32_t H = R->H, S = R->S, G = R->G, tph = R->tph;
    const uint64_t t = blockIdx.x - U.lt0;
    const uint64_t j = t / tph;
    const uint32_t k = (uint32_t)(t % tph);
    const uint64_t start = j * H + (uint64_t)k * G;
    if (t >= U.ntiles || start >= U.n)
        return;
    if (kZ && (j + 1) * (uint64_t)H > U.n) // the tail hop: in no gating block
        return;
    const uint32_t len = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(G, H - k * G), U.n - start);
    const uint32_t Sp = S | 1u;
    const double *x = U.x + start;
    // stage: element e to slot (e / S) * Sp + e % S, quotient and remainder carried along.  All of a thread's loads
    // (len <= 256 S: at most kLnMaxS) are issued before the first store, so they are in flight together
    double peak = 0.0;
    {
        double xv[kLnMaxS];
#pragma unroll
        for (uint32_t i = 0; i < kLnMaxS; i++) {
            const uint32_t e = tid + i * kLnLanes;
            xv[i] = e < len ? x[e] : 0.0;
        }
        uint32_t q = tid / S, r = tid % S;
        const uint32_t dq = kLnLanes / S, dr = kLnLanes % S;
#pragma unroll
        for (uint32_t i = 0; i < kLnMaxS; i++) {
            const uint32_t e = tid + i * kLnLanes;
            if (e >= len)
                break;
            const double v = xv[i];
            xs[q * Sp + r] = v;
            peak = fmax(peak, fabs(v));
            q += dq;
            r += dr;
            if (r >= S) {
                r -= S;
                q++;
            }
        }
    }
    __syncthreads();
    double c[10];
    ln_coefs(R, c);
    const double inv = 1.0 / 32768.0;
    const uint32_t seg0 = tid * S;
    const uint32_t sl = seg0 < len ? std::min(S, len - seg0) : 0u;
    const double *xl = xs + tid * Sp;
    // every segment from zero state: its end state
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < sl; i++)
        ln_step(c, v, xl[i] * inv);
    ln_to_scan(v);
    for (int i = 0; i < 4; i++)
        sc[tid * 4 + i] = v[i];
    __syncthreads();
    // inclusive scan of v_0 = tile start state, v_l = e_(l-1): s_l = sum_(m <= l) A^(S (l - m)) v_m
    for (int i = 0; i < 4; i++) {
        double s0 = 0.0;
        if (kZ)
            s0 = st[(U.tile0 + t) * 4 + i];
        v[i] = tid == 0 ? s0 : sc[(tid - 1) * 4 + i];
    }
    const uint32_t nact = (len + S - 1) / S;
    for (uint32_t kk = 0; (1u << kk) < nact; kk++) {
        const uint32_t d = 1u << kk;
        __syncthreads();
        for (int i = 0; i < 4; i++)
            sc[tid * 4 + i] = v[i];
        __syncthreads();
        if (tid >= d) {
            double w[4];
            for (int i = 0; i < 4; i++)
                w[i] = sc[(tid - d) * 4 + i];
            ln_mv_add((cdouble *)R->P[kk], w, v);
        }
    }
    // v: the state at the start of this lane's segment, back in the recursion's coordinates
    ln_from_scan(v);
    double acc = 0.0;
    if (kZ) {
        for (uint32_t i = 0; i < sl; i++) {
            const double y = ln_step(c, v, xl[i] * inv);
            acc = __builtin_fma(y, y, acc);
        }
    } else {
        if (tid == nact - 1) {
            for (uint32_t i = 0; i < sl; i++)
                ln_step(c, v, xl[i] * inv);
            ln_to_scan(v);
            for (int i = 0; i < 4; i++)
                st[(U.tile0 + t) * 4 + i] = v[i];
        }
        acc = peak;
    }
    red[tid] = acc;
    __syncthreads();
    for (uint32_t w = kLnLanes / 2; w > 0; w >>= 1) {
        if (tid < w)
            red[tid] = kZ ? red[tid] + red[tid + w] : fmax(red[tid], red[tid + w]);
        __syncthreads();
    }
    if (tid == 0) {
        if (kZ)
            z[U.tile0 + t] = red[0];
        else
            pk[U.tile0 + t] = red[0];
    }
}

__device__ __forceinline__ void ln_mat_mul(const double *a, const double *b, double *out)
{
    double r[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++)
                acc = __builtin_fma(a[i * 4 + k], b[k * 4 + j], acc);
            r[i * 4 + j] = acc;
        }
    for (int i = 0; i < 16; i++)
        out[i] = r[i];
}

// One wave per utterance: every tile of a full hop gets its true start state (in place of its zero-state end state)
__global__ __launch_bounds__(64) void k_ln_scan(const LoudnessRate *__restrict__ rates,
                                                const LoudnessUtt *__restrict__ utts, double *__restrict__ st)
{
    const LoudnessUtt U = utts[blockIdx.x];
    const LoudnessRate *R = rates + U.rate;
    const uint32_t H = R->H, tph = R->tph;
    const uint64_t nh = U.n / H; // full hops
    if (nh == 0)
        return;
    const uint32_t lane = threadIdx.x;
    const uint64_t cl = (nh + 63) / 64; // hops per lane
    const uint64_t h0 = std::min<uint64_t>(lane * cl, nh), h1 = std::min<uint64_t>(h0 + cl, nh);
    double *sb = st + U.tile0 * 4;
    cdouble *Pt = (cdouble *)R->Pt, *Pr = (cdouble *)R->Pr, *Ph = (cdouble *)R->Ph;
    // the chunk's end state from zero
    double F[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint64_t h = h0; h < h1; h++) {
        double e[4];
        for (int i = 0; i < 4; i++)
            e[i] = sb[(h * tph) * 4 + i];
        for (uint32_t k = 1; k < tph; k++) {
            double n[4];
            for (int i = 0; i < 4; i++)
                n[i] = sb[(h * tph + k) * 4 + i];
            ln_mv_add(k + 1 < tph ? Pt : Pr, e, n);
            for (int i = 0; i < 4; i++)
                e[i] = n[i];
        }
        ln_mv_add(Ph, F, e);
        for (int i = 0; i < 4; i++)
            F[i] = e[i];
    }
    // Q = A^(H cl), the transition over a full chunk
    double Q[16], p[16];
    for (int i = 0; i < 16; i++) {
        Q[i] = (i % 5) == 0 ? 1.0 : 0.0;
        p[i] = Ph[i];
    }
    for (uint64_t m = cl; m; m >>= 1) {
        if (m & 1)
            ln_mat_mul(Q, p, Q);
        if (m > 1)
            ln_mat_mul(p, p, p);
    }
    // inclusive scan across the lanes, then each lane's chunk start is its predecessor's value
    for (uint32_t d = 1; d < 64; d <<= 1) {
        double w[4];
        for (int i = 0; i < 4; i++)
            w[i] = __shfl_up(F[i], d, 64);
        if (lane >= d)
            for (int i = 0; i < 4; i++) {
                double acc = F[i];
                for (int k = 0; k < 4; k++)
                    acc = __builtin_fma(Q[i * 4 + k], w[k], acc);
                F[i] = acc;
            }
        ln_mat_mul(Q, Q, Q);
    }
    double s[4];
    for (int i = 0; i < 4; i++) {
        const double w = __shfl_up(F[i], 1, 64);
        s[i] = lane == 0 ? 0.0 : w;
    }
    for (uint64_t h = h0; h < h1; h++)
        for (uint32_t k = 0; k < tph; k++) {
            double *p4 = sb + (h * tph + k) * 4;
            double e[4];
            for (int i = 0; i < 4; i++) {
                e[i] = p4[i];
                p4[i] = s[i];
            }
            ln_mv_add(k + 1 < tph ? Pt : Pr, s, e);
            for (int i = 0; i < 4; i++)
                s[i] = e[i];
        }
}

constexpr uint32_t kTpBefore = 5, kTpAfter = 6; // the halo of a 12-tap window around sample n: x[n - 5 .. n + 6]

// True peak of the measure tiles (the tail hop's included): tp[tile] = max over the tile's samples n and the phases
// p = 1..F-1 of |y_p[n]|, y_p[n] = h[p][0] x[n - 5] and then FMAs in ascending j.  Tiles of an utterance in sample
// mode, or at a rate with F = 1, return at once: k_ln_gate does not read their slot
__global__ __launch_bounds__(kLnLanes) void k_ln_true_peak(const LoudnessRate *__restrict__ rates,
                                                           const LoudnessUtt *__restrict__ utts, uint32_t n_utts,
                                                           double *__restrict__ tp)
{
    __shared__ double xs[kLnLanes * kLnMaxS + kTpBefore + kTpAfter]; // slot i: sample start - 5 + i
    __shared__ double red[kLnLanes];
    const uint32_t tid = threadIdx.x;
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x, &LoudnessUtt::lt0);
    const LoudnessUtt U = utts[u];
    if (U.mode != JB_PEAK_TRUE)
        return;
    const LoudnessRate *R = rates + U.rate;
    const uint32_t H = R->H, G = R->G, tph = R->tph, F = R->F;
    if (F < 2)
        return;
    const uint64_t t = blockIdx.x - U.lt0;
    const uint64_t j = t / tph;
    const uint32_t k = (uint32_t)(t % tph);
    const uint64_t start = j * H + (uint64_t)k * G;
    if (t >= U.ntiles || start >= U.n)
        return;
    const uint32_t len = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(G, H - k * G), U.n - start);
    // stage x[start - 5, start + len + 6), zero outside [0, n): len + 11 <= 4096 + 11 slots, coalesced
    for (uint32_t i = tid; i < len + kTpBefore + kTpAfter; i += kLnLanes) {
        const uint64_t g = start + i; // sample g - 5
        xs[i] = (g >= kTpBefore && g - kTpBefore < U.n) ? U.x[g - kTpBefore] : 0.0;
    }
    __syncthreads();
    cdouble *h = (cdouble *)R->tp;
    double m = 0.0;
    for (uint32_t s = tid; s < len; s += kLnLanes) {
        double w[kTpTaps];
#pragma unroll
        for (uint32_t q = 0; q < kTpTaps; q++)
            w[q] = xs[s + q];
#pragma unroll 3
        for (uint32_t p = 0; p + 1 < F; p++) {
            cdouble *hp = h + p * kTpTaps;
            double y = hp[0] * w[0];
#pragma unroll
            for (uint32_t q = 1; q < kTpTaps; q++)
                y = __builtin_fma(hp[q], w[q], y);
            m = fmax(m, fabs(y));
        }
    }
    red[tid] = m;
    __syncthreads();
    for (uint32_t w = kLnLanes / 2; w > 0; w >>= 1) {
        if (tid < w)
            red[tid] = fmax(red[tid], red[tid + w]);
        __syncthreads();
    }
    if (tid == 0)
        tp[U.tile0 + t] = red[0];
}

// z of hop h of one utterance: its tiles' shares added in ascending order
struct LnHopZ {
    const double *zu;
    uint32_t tph;
    __device__ __forceinline__ double operator()(uint64_t h) const
    {
        double s = zu[h * tph];
        for (uint32_t k = 1; k < tph; k++)
            s += zu[h * tph + k];
        return s;
    }
};

// ln_tree (jb_loudness_rules.h) over the workgroup's lanes in LDS; every lane gets lane 0's result
__device__ __forceinline__ void ln_tree_lds(double *rs, uint32_t *rn, uint32_t tid, double *sum, uint32_t *cnt)
{
    rs[tid] = *sum;
    rn[tid] = *cnt;
    __syncthreads();
    for (uint32_t w = kLnLanes / 2; w > 0; w >>= 1) {
        if (tid < w) {
            rs[tid] += rs[tid + w];
            rn[tid] += rn[tid + w];
        }
        __syncthreads();
    }
    *sum = rs[0];
    *cnt = rn[0];
    __syncthreads();
}

__device__ __forceinline__ double ln_max_lds(double *rs, uint32_t tid, double v)
{
    rs[tid] = v;
    __syncthreads();
    for (uint32_t w = kLnLanes / 2; w > 0; w >>= 1) {
        if (tid < w)
            rs[tid] = fmax(rs[tid], rs[tid + w]);
        __syncthreads();
    }
    v = rs[0];
    __syncthreads();
    return v;
}

// One workgroup per utterance: z_j, blocks, gates, L, P, TP, gain -- fixed orders over a fixed thread count
__global__ __launch_bounds__(kLnLanes) void k_ln_gate(const LoudnessRate *__restrict__ rates,
                                                      const LoudnessUtt *__restrict__ utts,
                                                      const double *__restrict__ pk, const double *__restrict__ tp,
                                                      const double *__restrict__ z, LoudnessResult *__restrict__ res)
{
    __shared__ double rs[kLnLanes];
    __shared__ uint32_t rn[kLnLanes];
    const uint32_t tid = threadIdx.x;
    const LoudnessUtt U = utts[blockIdx.x];
    const LoudnessRate *R = rates + U.rate;
    const uint32_t H = R->H, tph = R->tph;
    double m = 0.0;
    for (uint32_t t = tid; t < U.ntiles; t += kLnLanes)
        m = fmax(m, pk[U.tile0 + t]);
    rs[tid] = m;
    __syncthreads();
    for (uint32_t w = kLnLanes / 2; w > 0; w >>= 1) {
        if (tid < w)
            rs[tid] = fmax(rs[tid], rs[tid + w]);
        __syncthreads();
    }
    const double peak = rs[0];
    __syncthreads();
    // true-peak mode: the tiles' oversampled maxima folded the same way, then with the sample peak (phase 0)
    const bool tmode = U.mode == JB_PEAK_TRUE;
    double tpeak = peak;
    if (tmode && R->F > 1) {
        m = 0.0;
        for (uint32_t t = tid; t < U.ntiles; t += kLnLanes)
            m = fmax(m, tp[U.tile0 + t]);
        rs[tid] = m;
        __syncthreads();
        for (uint32_t w = kLnLanes / 2; w > 0; w >>= 1) {
            if (tid < w)
                rs[tid] = fmax(rs[tid], rs[tid + w]);
            __syncthreads();
        }
        tpeak = fmax(peak, rs[0]);
        __syncthreads();
    }
    const uint64_t nh = U.n / H, nb = ln_blocks(nh);
    const LnHopZ hop_z{z + U.tile0, tph};
    auto ms = [&](uint64_t i) { return ln_block_ms(hop_z, i, H); };
    // pass 0: the absolute gate; pass 1: both gates
    double gamma = -INFINITY, L = -INFINITY;
    for (int pass = 0; pass < 2; pass++) {
        double sum;
        uint32_t cnt;
        ln_lane_partial(ms, nb, tid, pass, gamma, &sum, &cnt);
        ln_tree_lds(rs, rn, tid, &sum, &cnt);
        if (cnt == 0)
            break;
        const double lk = ln_loudness(sum / (double)cnt);
        if (pass == 0)
            gamma = lk + kLnRelGate;
        else
            L = lk;
    }
    if (tid == 0) {
        const double P = 20.0 * log10(peak / 32768.0);
        const double TP = tmode ? 20.0 * log10(tpeak / 32768.0) : NAN;
        const double gain = ln_gain_db(U.target, L, U.ceiling, tmode ? TP : P);
        LoudnessResult r;
        r.lufs = L;
        r.peak_dbfs = P;
        r.gain_db = gain;
        r.g = pow(10.0, gain / 20.0);
        r.true_peak_dbtp = TP;
        res[U.slot] = r;
    }
}

// One workgroup per group: the members' blocks through both gates as one set.  A member's partial of a pass is
// k_ln_gate's (the lanes' strided sums, the tree); the members' partials are added in the list's order, ascending
// utterance index.  P_G / TP_G: the largest of what k_ln_gate left for the members (log10 is monotone: the dB of the
// largest magnitude).  Every member's gain_db and g become the group's
__global__ __launch_bounds__(kLnLanes) void k_ln_gate_group(const LoudnessRate *__restrict__ rates,
                                                            const LoudnessUtt *__restrict__ utts,
                                                            const LoudnessSet *__restrict__ sets,
                                                            const uint32_t *__restrict__ members,
                                                            const double *__restrict__ z, LoudnessResult *res,
                                                            LoudnessGroupResult *__restrict__ gres)
{
    __shared__ double rs[kLnLanes];
    __shared__ uint32_t rn[kLnLanes];
    const uint32_t tid = threadIdx.x;
    const LoudnessSet S = sets[blockIdx.x];
    const uint32_t *mem = members + S.m0;
    double gamma = -INFINITY, L = -INFINITY;
    for (int pass = 0; pass < 2; pass++) {
        double gsum = 0.0;
        uint64_t gcnt = 0;
        for (uint32_t m = 0; m < S.nm; m++) {
            const LoudnessUtt U = utts[mem[m]];
            const LoudnessRate *R = rates + U.rate;
            const uint32_t H = R->H;
            const LnHopZ hop_z{z + U.tile0, R->tph};
            auto ms = [&](uint64_t i) { return ln_block_ms(hop_z, i, H); };
            double sum;
            uint32_t cnt;
            ln_lane_partial(ms, ln_blocks(U.n / H), tid, pass, gamma, &sum, &cnt);
            ln_tree_lds(rs, rn, tid, &sum, &cnt);
            gsum += sum;
            gcnt += cnt;
        }
        if (gcnt == 0)
            break;
        const double lk = ln_loudness(gsum / (double)gcnt);
        if (pass == 0)
            gamma = lk + kLnRelGate;
        else
            L = lk;
    }
    // the peaks: a max is exact in any order
    double p = -INFINITY, t = -INFINITY;
    for (uint32_t m = tid; m < S.nm; m += kLnLanes) {
        const LoudnessResult r = res[utts[mem[m]].slot];
        p = fmax(p, r.peak_dbfs);
        t = fmax(t, r.true_peak_dbtp); // (NaN in sample mode: fmax keeps -INFINITY, not used)
    }
    p = ln_max_lds(rs, tid, p);
    t = ln_max_lds(rs, tid, t);
    const LoudnessUtt U0 = utts[mem[0]];
    const bool tmode = U0.mode == JB_PEAK_TRUE;
    const double TP = tmode ? t : NAN;
    const double gain = ln_gain_db(U0.target, L, U0.ceiling, tmode ? TP : p);
    const double g = pow(10.0, gain / 20.0);
    if (tid == 0) {
        LoudnessGroupResult r;
        r.lufs = L;
        r.peak_dbfs = p;
        r.true_peak_dbtp = TP;
        r.gain_db = gain;
        r.g = g;
        gres[S.slot] = r;
    }
    for (uint32_t m = tid; m < S.nm; m += kLnLanes) {
        LoudnessResult *r = res + utts[mem[m]].slot;
        r->gain_db = gain;
        r->g = g;
    }
}

// One workgroup per utterance: short-term window i (hops i..i+29, ascending) to sw[tile0 + i] -- an utterance has no
// more windows than tiles -- and its largest momentary loudness, over every block without a gate, to mm[slot]
__global__ __launch_bounds__(kLnLanes) void k_ln_windows(const LoudnessRate *__restrict__ rates,
                                                         const LoudnessUtt *__restrict__ utts,
                                                         const double *__restrict__ z, double *__restrict__ sw,
                                                         double *__restrict__ mm)
{
    __shared__ double rs[kLnLanes];
    const uint32_t tid = threadIdx.x;
    const LoudnessUtt U = utts[blockIdx.x];
    const LoudnessRate *R = rates + U.rate;
    const uint32_t H = R->H;
    const uint64_t nh = U.n / H, nb = ln_blocks(nh), nw = ln_windows(nh);
    const LnHopZ hop_z{z + U.tile0, R->tph};
    for (uint64_t i = tid; i < nw; i += kLnLanes)
        sw[U.tile0 + i] = ln_window_ms(hop_z, i, H);
    double m = 0.0;
    for (uint64_t i = tid; i < nb; i += kLnLanes)
        m = fmax(m, ln_block_ms(hop_z, i, H));
    m = ln_max_lds(rs, tid, m);
    if (tid == 0)
        mm[U.slot] = ln_loudness(m); // (no block: log10(0), -INFINITY)
}

// One workgroup per set (an utterance, or a group's members): the largest momentary and short-term loudness and the
// loudness range.  The range's gate is a mean in the fixed order of k_ln_gate_group; its two order statistics come
// from a radix selection over the bit patterns of the kept windows' mean squares (positive doubles: their order is
// the integer order), 8 bits a pass into LDS histograms by integer atomics, both ranks through the same passes
__global__ __launch_bounds__(kLnLanes) void k_ln_range(const LoudnessRate *__restrict__ rates,
                                                       const LoudnessUtt *__restrict__ utts,
                                                       const LoudnessSet *__restrict__ sets,
                                                       const uint32_t *__restrict__ members,
                                                       const double *__restrict__ sw, const double *__restrict__ mm,
                                                       LoudnessRange *__restrict__ out)
{
    __shared__ double rs[kLnLanes];
    __shared__ uint32_t rn[kLnLanes];
    __shared__ uint32_t hist[2][256];
    const uint32_t tid = threadIdx.x;
    const LoudnessSet S = sets[blockIdx.x];
    const uint32_t *mem = members + S.m0;
    double mom = -INFINITY, st = 0.0;
    for (uint32_t m = tid; m < S.nm; m += kLnLanes)
        mom = fmax(mom, mm[utts[mem[m]].slot]);
    mom = ln_max_lds(rs, tid, mom);
    // the windows of member m: nw values at w
    auto windows = [&](uint32_t m, const double **w) {
        const LoudnessUtt U = utts[mem[m]];
        *w = sw + U.tile0;
        return ln_windows(U.n / rates[U.rate].H);
    };
    for (uint32_t m = 0; m < S.nm; m++) {
        const double *w;
        const uint64_t nw = windows(m, &w);
        for (uint64_t i = tid; i < nw; i += kLnLanes)
            st = fmax(st, w[i]);
    }
    st = ln_max_lds(rs, tid, st);
    // pass 0: the absolute gate and the relative gate's level; pass 1: the count of what both keep
    double gamma = -INFINITY;
    uint64_t n = 0;
    for (int pass = 0; pass < 2; pass++) {
        double gsum = 0.0;
        uint64_t gcnt = 0;
        for (uint32_t m = 0; m < S.nm; m++) {
            const double *w;
            const uint64_t nw = windows(m, &w);
            auto ms = [&](uint64_t i) { return w[i]; };
            double sum;
            uint32_t cnt;
            ln_lane_partial(ms, nw, tid, pass, gamma, &sum, &cnt);
            ln_tree_lds(rs, rn, tid, &sum, &cnt);
            gsum += sum;
            gcnt += cnt;
        }
        if (gcnt == 0)
            break;
        if (pass == 0)
            gamma = ln_loudness(gsum / (double)gcnt) + kLnRangeGate;
        else
            n = gcnt;
    }
    uint64_t rank[2] = {0, 0}, prefix[2] = {0, 0};
    if (n) {
        rank[0] = ln_rank(n, kLnRangeLo);
        rank[1] = ln_rank(n, kLnRangeHi);
    }
    for (uint32_t pass = 0; n && pass < 8; pass++) {
        hist[0][tid] = 0;
        hist[1][tid] = 0;
        __syncthreads();
        for (uint32_t m = 0; m < S.nm; m++) {
            const double *w;
            const uint64_t nw = windows(m, &w);
            for (uint64_t i = tid; i < nw; i += kLnLanes) {
                const double v = w[i];
                if (!ln_keep(ln_loudness(v), 1, gamma))
                    continue;
                const uint64_t bits = ln_bits(v);
                const uint32_t d = ln_radix_digit(bits, pass);
                if (ln_radix_in(bits, prefix[0], pass))
                    atomicAdd(&hist[0][d], 1u);
                if (ln_radix_in(bits, prefix[1], pass))
                    atomicAdd(&hist[1][d], 1u);
            }
        }
        __syncthreads();
        // (every thread walks the bins itself: the same answer everywhere, no broadcast)
        for (int k = 0; k < 2; k++)
            prefix[k] = (prefix[k] << 8) | ln_radix_pick(hist[k], &rank[k]);
        __syncthreads();
    }
    if (tid == 0) {
        LoudnessRange r;
        r.max_momentary = mom;
        r.max_short_term = ln_loudness(st); // (no window: -INFINITY)
        r.n = n;
        const double lo = ln_from_bits(prefix[0]), hi = ln_from_bits(prefix[1]);
        r.lra = n ? 10.0 * log10(hi / lo) : 0.0;
        r.lra_low = n ? ln_loudness(lo) : NAN;
        r.lra_high = n ? ln_loudness(hi) : NAN;
        out[S.rslot] = r;
    }
}

// the vocoder's 16-bit sink rule (jb_vocoder.hip pcm_i16): clamp, then truncate toward zero
__device__ __forceinline__ int16_t ln_i16(double v)
{
    v = fmin(v, 32767.0);
    v = fmax(v, -32768.0);
    return (int16_t)(int)v;
}

template <class T>
__global__ __launch_bounds__(kLnLanes) void k_ln_apply(const LoudnessUtt *__restrict__ utts, uint32_t n_utts,
                                                       const LoudnessResult *__restrict__ res)
{
    const uint32_t u = find_unit(utts, n_utts, blockIdx.x, &LoudnessUtt::at0);
    const LoudnessUtt U = utts[u];
    const uint64_t k0 = (blockIdx.x - U.at0) * (uint64_t)kLnApplyTile;
    if (k0 >= U.n || !U.y)
        return;
    const uint64_t k1 = std::min<uint64_t>(k0 + kLnApplyTile, U.n);
    const double g = res[U.slot].g;
    T *y = (T *)U.y;
#pragma unroll 8
    for (uint64_t k = k0 + threadIdx.x; k < k1; k += kLnLanes) {
        const double v = U.x[k] * g;
        if constexpr (sizeof(T) == 2)
            y[k] = ln_i16(v);
        else
            y[k] = v;
    }
}

hipError_t launch_loudness_measure(const LoudnessRate *rates_dev, const LoudnessUtt *utts_dev, uint32_t n,
                                   uint64_t tiles, double *st, double *pk, double *tp, double *z, LoudnessResult *res,
                                   bool true_peak, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (tiles) {
        hipLaunchKernelGGL(k_ln_tiles<false>, dim3((uint32_t)tiles), dim3(kLnLanes), 0, stream, rates_dev, utts_dev, n,
                           st, pk, z);
        hipLaunchKernelGGL(k_ln_scan, dim3(n), dim3(64), 0, stream, rates_dev, utts_dev, st);
        hipLaunchKernelGGL(k_ln_tiles<true>, dim3((uint32_t)tiles), dim3(kLnLanes), 0, stream, rates_dev, utts_dev, n,
                           st, pk, z);
        if (true_peak)
            hipLaunchKernelGGL(k_ln_true_peak, dim3((uint32_t)tiles), dim3(kLnLanes), 0, stream, rates_dev, utts_dev,
                               n, tp);
    }
    hipLaunchKernelGGL(k_ln_gate, dim3(n), dim3(kLnLanes), 0, stream, rates_dev, utts_dev, pk, tp, z, res);
    return hipGetLastError();
}

hipError_t launch_loudness_apply(const LoudnessUtt *utts_dev, uint32_t n, uint64_t atiles, const LoudnessResult *res,
                                 bool i16, hipStream_t stream)
{
    if (n == 0 || atiles == 0)
        return hipSuccess;
    if (atiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (i16)
        hipLaunchKernelGGL(k_ln_apply<int16_t>, dim3((uint32_t)atiles), dim3(kLnLanes), 0, stream, utts_dev, n, res);
    else
        hipLaunchKernelGGL(k_ln_apply<double>, dim3((uint32_t)atiles), dim3(kLnLanes), 0, stream, utts_dev, n, res);
    return hipGetLastError();
}

hipError_t launch_loudness_groups(const LoudnessRate *rates_dev, const LoudnessUtt *utts_all, const LoudnessSet *sets_dev,
                                  uint32_t n, const uint32_t *members, const double *z, LoudnessResult *res,
                                  LoudnessGroupResult *gres, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_ln_gate_group, dim3(n), dim3(kLnLanes), 0, stream, rates_dev, utts_all, sets_dev, members, z,
                       res, gres);
    return hipGetLastError();
}

hipError_t launch_loudness_range(const LoudnessRate *rates_dev, const LoudnessUtt *utts_dev, uint32_t n_utts,
                                 const LoudnessUtt *utts_all, const LoudnessSet *sets_dev, uint32_t n_sets,
                                 const uint32_t *members, const double *z, double *sw, double *mm,
                                 LoudnessRange *r128, hipStream_t stream)
{
    if (n_utts)
        hipLaunchKernelGGL(k_ln_windows, dim3(n_utts), dim3(kLnLanes), 0, stream, rates_dev, utts_dev, z, sw, mm);
    if (n_sets)
        hipLaunchKernelGGL(k_ln_range, dim3(n_sets), dim3(kLnLanes), 0, stream, rates_dev, utts_all, sets_dev, members,
                           sw, mm, r128);
    return hipGetLastError();
}

// The measurement on PCM the caller holds: out[u] of in[u]; mode: what every utterance's ceiling term would read
// gr (null: none): the utterances in these groups against one target and ceiling, with the R128 fields
struct PcmGroups {
    LnGroups plan;
    double target = NAN, ceiling = INFINITY;
    std::vector<LoudnessGroupResult> gres; // [G]
    std::vector<LoudnessRange> r128;       // [n] the utterances, then [G] the groups
};

int measure_pcm_batch(const double *const *in, const size_t *n_in, size_t n, uint32_t hz, int32_t device,
                      uint32_t mode, const char *what, std::vector<LoudnessResult> *res, PcmGroups *gr = nullptr)
{
    int rc = pcm_check((const void *const *)in, n_in, n);
    if (rc)
        return rc;
    if (hz == 0) {
        set_error("loudness: a rate of 0 Hz");
        return JB_ERR_INVALID;
    }
    LoudnessRate rate{};
    if ((rc = loudness_rate(hz, &rate)))
        return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, what)))
        return rc;
    std::vector<uint64_t> off;
    const double *dx = ds.pack(in, n_in, n, &off);
    std::vector<LoudnessUtt> utts(n);
    uint64_t tiles = 0;
    for (size_t u = 0; u < n; u++) {
        LoudnessUtt &w = utts[u];
        w = LoudnessUtt{};
        w.x = dx + off[u];
        w.n = n_in[u];
        w.ntiles = loudness_tiles(rate, w.n);
        w.tile0 = w.lt0 = tiles;
        w.slot = (uint32_t)u;
        w.mode = mode;
        w.target = gr ? gr->target : NAN;
        w.ceiling = gr ? gr->ceiling : INFINITY;
        tiles += w.ntiles;
    }
    double *dst = ds.alloc<double>(4 * std::max<uint64_t>(tiles, 1)), *dpk = ds.alloc<double>(tiles);
    double *dtp = ds.alloc<double>(tiles), *dz = ds.alloc<double>(tiles);
    const std::vector<LoudnessRate> rates(1, rate);
    const LoudnessRate *dr = ds.upload(rates);
    const LoudnessUtt *du = ds.upload(utts);
    LoudnessResult *dres = ds.alloc<LoudnessResult>(n);
    if (ds.ok())
        ds.err = launch_loudness_measure(dr, du, (uint32_t)n, tiles, dst, dpk, dtp, dz, dres, mode == JB_PEAK_TRUE,
                                         ds.stream);
    // the sets of a group request: every utterance (members: the identity), then every group
    const size_t G = gr ? gr->plan.size() : 0;
    std::vector<LoudnessSet> sets;
    std::vector<uint32_t> members;
    LoudnessGroupResult *dgres = nullptr;
    LoudnessRange *dr128 = nullptr;
    if (gr && n) {
        sets.resize(n + G);
        members.resize(2 * n);
        for (size_t u = 0; u < n; u++) {
            sets[u] = LoudnessSet{(uint32_t)u, 1, (uint32_t)u, (uint32_t)u};
            members[u] = (uint32_t)u;
            members[n + u] = gr->plan.members[u];
        }
        for (size_t g = 0; g < G; g++)
            sets[n + g] = LoudnessSet{(uint32_t)n + gr->plan.first[g], gr->plan.first[g + 1] - gr->plan.first[g],
                                      (uint32_t)g, (uint32_t)(n + g)};
        const LoudnessSet *dsets = ds.upload(sets);
        const uint32_t *dmem = ds.upload(members);
        dgres = ds.alloc<LoudnessGroupResult>(G);
        dr128 = ds.alloc<LoudnessRange>(n + G);
        double *dsw = ds.alloc<double>(tiles), *dmm = ds.alloc<double>(n);
        if (ds.ok())
            ds.err = launch_loudness_groups(dr, du, dsets + n, (uint32_t)G, dmem, dz, dres, dgres, ds.stream);
        if (ds.ok())
            ds.err = launch_loudness_range(dr, du, (uint32_t)n, du, dsets, (uint32_t)(n + G), dmem, dz, dsw, dmm, dr128,
                                           ds.stream);
    }
    res->assign(n, LoudnessResult{});
    ds.read_back(res, dres, n);
    if (gr && n) {
        gr->gres.assign(G, LoudnessGroupResult{});
        gr->r128.assign(n + G, LoudnessRange{});
        ds.read_back(&gr->gres, dgres, G);
        ds.read_back(&gr->r128, dr128, n + G);
    }
    return ds.status();
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_loudness_filter(uint32_t hz, double *b, double *a, uint32_t *hop) { return loudness_filter(hz, b, a, hop); }

int jb_loudness_pcm_batch(const double *const *in, const size_t *n_in, size_t n, uint32_t hz, int32_t device,
                          double *lufs, double *peak_dbfs)
{
    if (n && (!lufs || !peak_dbfs))
        return JB_ERR_INVALID;
    int rc = loudness_measurable(hz);
    if (rc)
        return rc;
    std::vector<LoudnessResult> out;
    if ((rc = measure_pcm_batch(in, n_in, n, hz, device, JB_PEAK_SAMPLE, "jb_loudness_pcm_batch", &out)))
        return rc;
    for (size_t u = 0; u < n; u++) {
        lufs[u] = out[u].lufs;
        peak_dbfs[u] = out[u].peak_dbfs;
    }
    return JB_OK;
}

int jb_loudness_groups_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *group,
                                 uint32_t hz, int32_t device, uint32_t mode, double target_lufs, double ceiling_db,
                                 uint32_t *group_of, jb_loudness_group_report *groups, size_t groups_cap,
                                 size_t *n_groups, jb_loudness_r128 *utt_r128, double *utt_lufs)
{
    if (mode != JB_PEAK_SAMPLE && mode != JB_PEAK_TRUE) {
        set_error("jb_loudness_groups_pcm_batch: a mode is JB_PEAK_SAMPLE or JB_PEAK_TRUE");
        return JB_ERR_INVALID;
    }
    if (n > 0x7fffffffu || (groups_cap && !groups))
        return JB_ERR_INVALID;
    PcmGroups gr;
    gr.target = target_lufs;
    gr.ceiling = ceiling_db;
    std::vector<uint32_t> own(n, kLnNoGroup);
    LnGroupsIn gi;
    gi.B = n;
    gi.group = group ? group : own.data();
    uint32_t bad = 0;
    const char *field = "";
    if (!plan_loudness_groups(gi, &gr.plan, &bad, &field)) {
        set_error("jb_loudness_groups_pcm_batch: " + std::string(field) + " " + std::to_string(bad) +
                  " (an id is below n, or JB_LOUDNESS_NO_GROUP)");
        return JB_ERR_INVALID;
    }
    const size_t G = gr.plan.size();
    if (n_groups)
        *n_groups = G;
    if (G > groups_cap && groups) {
        set_error("jb_loudness_groups_pcm_batch: " + std::to_string(G) + " groups, room for " +
                  std::to_string(groups_cap));
        return JB_ERR_BUFFER;
    }
    int rc = loudness_measurable(hz);
    if (rc)
        return rc;
    std::vector<LoudnessResult> out;
    if ((rc = measure_pcm_batch(in, n_in, n, hz, device, mode, "jb_loudness_groups_pcm_batch", &out, &gr)))
        return rc;
    uint32_t F = 1;
    if ((rc = true_peak_table(hz, &F, nullptr)))
        return rc;
    for (size_t u = 0; u < n; u++) {
        if (group_of)
            group_of[u] = gr.plan.group_of[u];
        if (utt_r128)
            loudness_r128_out(gr.r128[u], &utt_r128[u]);
        if (utt_lufs)
            utt_lufs[u] = out[u].lufs;
    }
    for (size_t g = 0; groups && g < G; g++)
        loudness_group_report(gr.gres[g], mode, F, gr.plan.first[g + 1] - gr.plan.first[g], &gr.r128[n + g],
                              &groups[g]);
    return JB_OK;
}

int jb_true_peak_filter(uint32_t hz, uint32_t *F, uint32_t *ntaps, double *taps, size_t cap)
{
    uint32_t f = 0;
    int rc = true_peak_table(hz, &f, nullptr);
    if (rc)
        return rc;
    if (F)
        *F = f;
    if (ntaps)
        *ntaps = kTpTaps;
    if (!taps)
        return JB_OK;
    if (cap < (size_t)(f - 1) * kTpTaps) {
        set_error("jb_true_peak_filter: the buffer holds fewer than (F - 1) * 12 taps");
        return JB_ERR_BUFFER;
    }
    double all[(kTpMaxF - 1) * kTpTaps];
    if ((rc = true_peak_table(hz, nullptr, all)))
        return rc;
    std::copy(all, all + (size_t)(f - 1) * kTpTaps, taps);
    return JB_OK;
}

int jb_true_peak_pcm_batch(const double *const *in, const size_t *n_in, size_t n, uint32_t hz, int32_t device,
                           double *true_peak_dbtp)
{
    if (n && !true_peak_dbtp)
        return JB_ERR_INVALID;
    std::vector<LoudnessResult> out;
    int rc = measure_pcm_batch(in, n_in, n, hz, device, JB_PEAK_TRUE, "jb_true_peak_pcm_batch", &out);
    if (rc)
        return rc;
    for (size_t u = 0; u < n; u++)
        true_peak_dbtp[u] = out[u].true_peak_dbtp;
    return JB_OK;
}

} // extern "C"

#pragma once
// jb_rfft.h -- the transform of a real frame of n_fft samples packed as M = n_fft / 2 complex points, stated once for
// the stages that take one (the filterbank features, the mel spectrograms, the convolution): the LDS place of a point,
// the butterflies of radix 2, 3 and 5, the pass schedule, the untangling of the packed transform, the two twiddle tables
// (long double, rounded once), the rule of one frame on the host and the image of a stage's device tables.  Plain C++17;
// under hipcc the rules compile for the host and the device alike.  What only a kernel can say (the passes two to a
// barrier that k_fbank and the convolution's kernels share) is in jb_rfft_dev.h.
#include <cmath>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#ifdef __HIPCC__
// (spelt without the HIP runtime header: jb_output.cpp includes this file without it)
#define JB_RFFT_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_RFFT_HD inline
#endif

namespace jb {

constexpr uint32_t kRfftMaxPasses = 11; // 2048 = 2^11: the packed transform of the largest frame, 4096 samples

// Where value i of a frame lies in its LDS arrays: one pad double behind every 32.  The digit-reversed stores of the
// load (a wave's addresses differ in their high bits only: without the pad all 64 on one bank) and the spans of 4, 16,
// ... of the early passes then spread over the banks
JB_RFFT_HD constexpr uint32_t rfft_at(uint32_t i) { return i + (i >> 5); }

// (a, b) <- (a + w b, a - w b), w = c + i sn
JB_RFFT_HD void rfft_bfly(double &ar, double &ai, double &br, double &bi, double c, double sn)
{
    const double tr = c * br - sn * bi, ti = c * bi + sn * br;
    br = ar - tr;
    bi = ai - ti;
    ar = ar + tr;
    ai = ai + ti;
}
// One butterfly of stage s (spans of 2^s) of the in-place decimation-in-time transform of M = 2^log2m points whose
// input was stored in bit-reversed order: butterfly j of M / 2.  tw: the n_fft = 2 M table of rfft_twiddles
JB_RFFT_HD void rfft_stage_butterfly(double *re, double *im, const double *tw, uint32_t log2m, uint32_t s, uint32_t j)
{
    const uint32_t half = 1u << s, pos = j & (half - 1);
    const uint32_t i0 = ((j >> s) << (s + 1)) | pos, i1 = i0 + half;
    const uint32_t k = pos << (log2m - s); // pos n_fft / (2 half): always even
    rfft_bfly(re[i0], im[i0], re[i1], im[i1], tw[2 * k], tw[2 * k + 1]);
}

// X_k of the real transform from the packed one, Z in (re, im)[0..M): a = Z_k, z = Z_(M - k) (Z_M = Z_0), w_k = c + i sn;
// X_k = Fe + w_k Fo with Fe = (Z_k + conj Z_{M-k}) / 2 and Fo = -i (Z_k - conj Z_{M-k}) / 2
JB_RFFT_HD void rfft_bin(double ar, double ai, double zr, double zi, double c, double sn, double *xr, double *xi)
{
    const double br = zr, bi = -zi;
    const double fer = 0.5 * (ar + br), fei = 0.5 * (ai + bi);
    const double fr = 0.5 * (ai - bi), fi = -0.5 * (ar - br);
    *xr = fer + (c * fr - sn * fi);
    *xi = fei + (c * fi + sn * fr);
}
// |X_k|^2
JB_RFFT_HD double rfft_power(double ar, double ai, double zr, double zi, double c, double sn)
{
    double xr, xi;
    rfft_bin(ar, ai, zr, zi, c, sn, &xr, &xi);
    return xr * xr + xi * xi;
}
// The pair k, M - k (k in 0..M/2) of the M + 1 powers, in place: P_k into re[k], P_{M-k} into re[M - k] (re has a
// slot M); nothing else of the arrays is read
// (c0, s0), (c1, s1): entries k and M - k of the n_fft table
JB_RFFT_HD void rfft_untangle(double *re, double *im, uint32_t M, uint32_t k, double c0, double s0, double c1, double s1)
{
    const uint32_t kk = M - k, kz = kk == M ? 0 : kk;
    const double ar = re[k], ai = im[k], zr = re[kz], zi = im[kz];
    const double p0 = rfft_power(ar, ai, zr, zi, c0, s0);
    const double p1 = rfft_power(zr, zi, ar, ai, c1, s1);
    re[k] = p0;
    if (kk != k)
        re[kk] = p1;
}
JB_RFFT_HD void rfft_untangle(double *re, double *im, const double *tw, uint32_t M, uint32_t k)
{
    rfft_untangle(re, im, M, k, tw[2 * k], tw[2 * k + 1], tw[2 * (M - k)], tw[2 * (M - k) + 1]);
}

// The passes of the packed transform of M points: the factors 5, then 3, then 2 of M (a power of two: passes of 2
// alone).  Pass s has radix r[s] and span L[s] = r[0] ... r[s - 1]; inv[s] = floor(2^32 / L[s]) + 1 divides a
// butterfly's index by the span (rfft_div: exact for indices below 2^16; L = 1 is spelt out)
struct RfftSchedule {
    uint32_t n = 0;
    uint32_t r[kRfftMaxPasses] = {}, L[kRfftMaxPasses] = {}, inv[kRfftMaxPasses] = {};
};
inline RfftSchedule rfft_schedule(uint32_t M)
{
    RfftSchedule s;
    uint32_t span = 1;
    for (uint32_t p : {5u, 3u, 2u})
        while (M % p == 0 && s.n < kRfftMaxPasses) {
            s.r[s.n] = p;
            s.L[s.n] = span;
            s.inv[s.n] = span > 1 ? (uint32_t)(0x100000000ull / span) + 1 : 0;
            s.n++;
            span *= p;
            M /= p;
        }
    return s;
}
// Where input point j of the transform is stored: its digits in the schedule's radices, reversed (passes of 2 alone:
// its bits)
inline uint32_t rfft_digit_reverse(const RfftSchedule &s, uint32_t j)
{
    uint32_t at = 0;
    for (uint32_t p = s.n; p-- > 0;) {
        at += (j % s.r[p]) * s.L[p];
        j /= s.r[p];
    }
    return at;
}
JB_RFFT_HD uint32_t rfft_div(uint32_t j, uint32_t L, uint32_t inv)
{
    return L == 1 ? j : (uint32_t)(((uint64_t)j * inv) >> 32);
}

// The butterflies, decimation in time: the inputs behind the first are multiplied by their twiddles (c + i sn: powers of
// W_{rL}), then the r-point transform is taken with W_r = e^{-2 pi i / r}; written product by product and sum by sum
// (no contraction: the translation units are built with it off)
JB_RFFT_HD void rfft_twiddle(double &r, double &i, double c, double sn)
{
    const double tr = c * r - sn * i, ti = c * i + sn * r;
    r = tr;
    i = ti;
}
JB_RFFT_HD void rfft_bfly3(double &ar, double &ai, double &br, double &bi, double &cr, double &ci, double c1, double s1,
                           double c2, double s2)
{
    constexpr double kS3 = 0.86602540378443864676; // sin(2 pi / 3)
    rfft_twiddle(br, bi, c1, s1);
    rfft_twiddle(cr, ci, c2, s2);
    const double tr = br + cr, ti = bi + ci;
    const double dr = kS3 * (br - cr), di = kS3 * (bi - ci);
    const double mr = ar - 0.5 * tr, mi = ai - 0.5 * ti;
    ar = ar + tr;
    ai = ai + ti;
    br = mr + di; // m - i d
    bi = mi - dr;
    cr = mr - di; // m + i d
    ci = mi + dr;
}
JB_RFFT_HD void rfft_bfly5(double &ar, double &ai, double &br, double &bi, double &cr, double &ci, double &dr, double &di,
                           double &er, double &ei, const double *c, const double *s)
{
    constexpr double kC1 = 0.30901699437494742410, kC2 = -0.80901699437494742410; // cos(2 pi / 5), cos(4 pi / 5)
    constexpr double kS1 = 0.95105651629515357212, kS2 = 0.58778525229247312917;  // sin(2 pi / 5), sin(4 pi / 5)
    rfft_twiddle(br, bi, c[0], s[0]);
    rfft_twiddle(cr, ci, c[1], s[1]);
    rfft_twiddle(dr, di, c[2], s[2]);
    rfft_twiddle(er, ei, c[3], s[3]);
    const double s1r = br + er, s1i = bi + ei, s2r = cr + dr, s2i = ci + di;
    const double d1r = br - er, d1i = bi - ei, d2r = cr - dr, d2i = ci - di;
    const double m1r = (ar + kC1 * s1r) + kC2 * s2r, m1i = (ai + kC1 * s1i) + kC2 * s2i;
    const double m2r = (ar + kC2 * s1r) + kC1 * s2r, m2i = (ai + kC2 * s1i) + kC1 * s2i;
    const double n1r = kS1 * d1r + kS2 * d2r, n1i = kS1 * d1i + kS2 * d2i;
    const double n2r = kS2 * d1r - kS1 * d2r, n2i = kS2 * d1i - kS1 * d2i;
    ar = (ar + s1r) + s2r;
    ai = (ai + s1i) + s2i;
    br = m1r + n1i; // m1 - i n1
    bi = m1i - n1r;
    er = m1r - n1i; // m1 + i n1
    ei = m1i + n1r;
    cr = m2r + n2i; // m2 - i n2
    ci = m2i - n2r;
    dr = m2r - n2i; // m2 + i n2
    di = m2i + n2r;
}
// Butterfly j (of M / r) of a pass of radix r and span L of the in-place transform of M points whose input was stored
// in digit-reversed order.  twc, tws: cos and -sin of 2 pi p / M, p < M; at(i): where point i lies in re and im
template <class At>
JB_RFFT_HD void rfft_butterfly(double *re, double *im, const double *twc, const double *tws, uint32_t M, uint32_t r,
                               uint32_t L, uint32_t inv, uint32_t j, At at)
{
    const uint32_t blk = rfft_div(j, L, inv), pos = j - blk * L;
    const uint32_t i0 = blk * L * r + pos;
    const uint32_t p = (M / (L * r)) * pos; // W_{rL}^pos = W_M^p; q p < M for q < r
    const uint32_t a = at(i0), b = at(i0 + L);
    if (r == 2) {
        rfft_bfly(re[a], im[a], re[b], im[b], twc[p], tws[p]);
    } else if (r == 3) {
        const uint32_t c = at(i0 + 2 * L);
        rfft_bfly3(re[a], im[a], re[b], im[b], re[c], im[c], twc[p], tws[p], twc[2 * p], tws[2 * p]);
    } else {
        const uint32_t c = at(i0 + 2 * L), d = at(i0 + 3 * L), e = at(i0 + 4 * L);
        const double tc[4] = {twc[p], twc[2 * p], twc[3 * p], twc[4 * p]};
        const double ts[4] = {tws[p], tws[2 * p], tws[3 * p], tws[4 * p]};
        rfft_bfly5(re[a], im[a], re[b], im[b], re[c], im[c], re[d], im[d], re[e], im[e], tc, ts);
    }
}

// The two tables, in long double and rounded once.  The untangling: [n_fft / 2 + 1][2], cos and -sin of 2 pi k / n_fft
inline std::vector<double> rfft_twiddles(uint32_t n_fft)
{
    const long double two_pi = 2.0L * acosl(-1.0L);
    std::vector<double> tw(2 * (size_t)(n_fft / 2 + 1));
    for (uint32_t k = 0; k <= n_fft / 2; k++) {
        tw[2 * k] = (double)cosl(two_pi * k / (long double)n_fft);
        tw[2 * k + 1] = (double)-sinl(two_pi * k / (long double)n_fft);
    }
    return tw;
}
// The passes: the whole circle, twc and tws [M], cos and -sin of 2 pi p / M
inline void rfft_circle(uint32_t M, std::vector<double> *twc, std::vector<double> *tws)
{
    const long double two_pi = 2.0L * acosl(-1.0L);
    twc->resize(M);
    tws->resize(M);
    for (uint32_t p = 0; p < M; p++) {
        (*twc)[p] = (double)cosl(two_pi * p / (long double)M);
        (*tws)[p] = (double)-sinl(two_pi * p / (long double)M);
    }
}

// What the transform of one n_fft needs on the host, and of it what a kernel asks for on the device
struct RfftPlan {
    uint32_t M = 0;
    RfftSchedule sched;
    std::vector<uint32_t> rev;    // [M]: rfft_digit_reverse
    std::vector<double> tw;       // rfft_twiddles
    std::vector<double> twc, tws; // rfft_circle
};
inline RfftPlan rfft_plan(uint32_t n_fft)
{
    RfftPlan p;
    p.M = n_fft / 2;
    p.sched = rfft_schedule(p.M);
    p.rev.resize(p.M);
    for (uint32_t j = 0; j < p.M; j++)
        p.rev[j] = rfft_digit_reverse(p.sched, j);
    p.tw = rfft_twiddles(n_fft);
    rfft_circle(p.M, &p.twc, &p.tws);
    return p;
}
// One frame by the rule: x(i), sample i < n_fft of the windowed frame, to the M + 1 powers |X_k|^2 in re[0..M]
// (re and im: M + 1 values each).  The digit-reversed store, the schedule's passes butterfly after butterfly, the pairs
template <class X> inline void rfft_frame_power(const RfftPlan &p, X x, double *re, double *im)
{
    const uint32_t M = p.M;
    for (uint32_t j = 0; j < M; j++) {
        re[p.rev[j]] = x(2 * j);
        im[p.rev[j]] = x(2 * j + 1);
    }
    const RfftSchedule &s = p.sched;
    for (uint32_t q = 0; q < s.n; q++)
        for (uint32_t j = 0; j < M / s.r[q]; j++)
            rfft_butterfly(re, im, p.twc.data(), p.tws.data(), M, s.r[q], s.L[q], s.inv[q], j,
                           [](uint32_t i) { return i; });
    for (uint32_t k = 0; k <= M / 2; k++)
        rfft_untangle(re, im, p.tw.data(), M, k);
}

// The device image of a stage's tables: lists appended in whole doubles, each handed back as the address it will have
// once the image lies at `dev`.  Lists of uint32 that follow one another share their doubles.  A null `dev` measures:
// the image's size is what the same calls will need
struct TableImage {
    std::vector<double> words;
    explicit TableImage(const double *dev) : base((uintptr_t)dev) {}
    const double *put(const std::vector<double> &v)
    {
        ints = false;
        const size_t at = words.size();
        words.insert(words.end(), v.begin(), v.end());
        return (const double *)(base + 8 * at);
    }
    const uint32_t *put(const std::vector<uint32_t> &v)
    {
        if (!ints)
            run = words.size(), n32 = 0, ints = true;
        const size_t at = n32;
        n32 += v.size();
        words.resize(run + (n32 + 1) / 2, 0.0);
        if (!v.empty())
            memcpy((char *)(words.data() + run) + 4 * at, v.data(), 4 * v.size());
        return (const uint32_t *)(base + 8 * run + 4 * at);
    }

  private:
    uintptr_t base;
    size_t run = 0, n32 = 0; // the open run of uint32 lists: its first double and its values so far
    bool ints = false;
};

} // namespace jb

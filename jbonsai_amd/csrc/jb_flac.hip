// FLAC encoding of the 16-bit output (new surface: the reference writes WAV only).  The contract is in
// include/jbonsai_amd.h ("FLAC"); in short: one complete mono 16-bit FLAC stream per utterance, fixed block size,
// streamable subset, decode(stream) == the 16-bit PCM bit for bit; on request the MD5 of the samples in STREAMINFO
// and a SEEKTABLE (the rules: jb_md5.h).
//
// Five kernels (launch_flac_encode, then launch_flac_pack), and two more on request (launch_flac_md5 in front of
// the pack, k_flac_seektable inside it):
//   k_flac_encode   one workgroup per block (<= 4608 samples, staged in LDS): CONSTANT test; FIXED 0-4 and LPC at
//                   a fixed set of orders (Tukey(0.5) window, autocorrelation, Levinson-Durbin and coefficient
//                   quantization in f64, every sum in a fixed order) each priced by partitioned Rice on the
//                   finest partitions (sums of the folded residuals) merged up a tree to partition order 0; the
//                   cheapest is coded exactly (a scan of the per-sample code lengths), falls back to VERBATIM where
//                   that is not smaller, and is packed MSB-first into a zeroed LDS bit buffer with atomicOr (no
//                   code touches more than two words).  The CRC-16 is parallel: every thread's byte segment from
//                   zero state, joined by multiplication with x^(8 len) mod the polynomial (the CRC is linear:
//                   zero init, no final xor).  The frame goes to its block's slot (the VERBATIM bound apart).
//   k_flac_md5      one lane per utterance (a chain cannot be split: the batch is the parallelism), the launch list
//                   longest first so that a wave's 64 chains have similar lengths.  A lane reads its 64-byte blocks
//                   as aligned dwords, shifted by a half-word where the utterance starts on an odd sample, one block
//                   ahead of the one it hashes; the last one or two blocks (the samples left, 0x80, zeros, the bit
//                   count) are built in registers from guarded 16-bit loads: nothing behind sample n - 1 is read.
//   k_flac_scan     one workgroup per utterance: frame offsets, stream size, min and max frame size.
//   k_flac_place    one workgroup: each utterance's place in the compact slab (a scan in utterance order).
//   k_flac_header / k_flac_compact: the 42-byte stream header (fLaC + STREAMINFO, the digest in it on request) and
//                   one workgroup per frame copying it from its slot to its byte offset: whole words inside, byte
//                   stores at a head and a tail that may share a word with a neighbour.
//   k_flac_seektable  one thread per seek point (launched only where some utterance has points): sample number,
//                   byte offset from the first frame's header, samples of the frame, from k_flac_scan's offsets.
// A stream's bytes are a function of its samples, its rate and the options alone (the fast invariant mode stays
// invariant): the block is the unit of every choice, and no result depends on the batch.
#include "jb_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace jb {

namespace {
constexpr int kT = 256;                  // threads per workgroup
constexpr uint32_t kMaxWords = (kFlacMaxBlock * 8) / 4; // LDS union: f64 window or the frame's bit buffer
constexpr int kMaxP = 8;                 // Rice partition order (subset)

enum { kConstant = 0, kVerbatim = 1, kFixed = 2, kLpc = 3 };

__device__ inline uint32_t lane_id() { return threadIdx.x & 63u; }

// MSB-first: nbits (1..32) of val at bit position pos of the big-endian word buffer w
__device__ inline void put_bits(uint32_t *w, uint32_t pos, uint32_t nbits, uint32_t val)
{
    const uint32_t wi = pos >> 5, b = pos & 31u;
    const uint64_t v = (uint64_t)val << (64u - nbits - b);
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    if (hi)
        atomicOr(&w[wi], hi);
    if (lo)
        atomicOr(&w[wi + 1], lo);
}

__device__ inline uint32_t get_byte(const uint32_t *w, uint32_t j) { return (w[j >> 2] >> (24u - 8u * (j & 3u))) & 0xffu; }

// Carry-less a * b mod x^16 + x^15 + x^2 + 1 (FLAC's CRC-16)
__device__ inline uint32_t gf_mulmod(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u)
            r ^= 0x18005u;
        if ((b >> i) & 1u)
            r ^= a;
    }
    return r;
}
// x^(8 len) mod the polynomial: what a CRC state becomes after len zero bytes
__device__ inline uint32_t gf_shift(uint32_t len)
{
    uint32_t r = 1, base = 0x100u;
    while (len) {
        if (len & 1u)
            r = gf_mulmod(r, base);
        base = gf_mulmod(base, base);
        len >>= 1;
    }
    return r;
}

template <class T> __device__ inline T wave_incl_scan(T v)
{
    const uint32_t l = lane_id();
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (l >= (uint32_t)d)
            v += o;
    }
    return v;
}

// Exclusive block scan over kT threads (integers: exact in any order); tot gets the sum
template <class T> __device__ inline T block_excl_scan(T v, T *wsum, T *tot)
{
    const T inc = wave_incl_scan(v);
    const uint32_t wv = threadIdx.x >> 6;
    if (lane_id() == 63)
        wsum[wv] = inc;
    __syncthreads();
    T base = 0;
    for (uint32_t k = 0; k < wv; k++)
        base += wsum[k];
    const T all = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    *tot = all;
    return base + inc - v;
}

// Residual of sample i (i >= order) under a FIXED (order 0..4) or an LPC predictor
__device__ inline int64_t residual(const int32_t *s, int i, int kind, int order, const int32_t *qc, int shift)
{
    if (kind == kFixed) {
        const int64_t a = s[i];
        switch (order) {
        case 0: return a;
        case 1: return a - s[i - 1];
        case 2: return a - 2 * (int64_t)s[i - 1] + s[i - 2];
        case 3: return a - 3 * (int64_t)s[i - 1] + 3 * (int64_t)s[i - 2] - s[i - 3];
        default: return a - 4 * (int64_t)s[i - 1] + 6 * (int64_t)s[i - 2] - 4 * (int64_t)s[i - 3] + s[i - 4];
        }
    }
    int64_t acc = 0;
#pragma unroll
    for (int j = 0; j < kFlacMaxLpc; j++)
        if (j < order)
            acc += (int64_t)(qc[j] * s[i - 1 - j]);
    return (int64_t)s[i] - (acc >> shift);
}

__device__ inline uint32_t fold(int64_t r) { return r >= 0 ? (uint32_t)(2 * r) : (uint32_t)(-2 * r - 1); }

// The Rice parameter of a partition of m samples whose folded residuals sum to S: the cheapest of k0 - 1 .. k0 + 1
// (k0 = floor(log2(S / m))) by libFLAC's estimate m (k + 1) + (S >> k); ties to the smaller k
__device__ inline uint32_t rice_param(uint64_t S, uint32_t m, uint32_t *cost)
{
    const uint64_t q = m ? S / m : 0;
    const int k0 = q ? 63 - __clzll((long long)q) : 0;
    uint32_t bk = 0;
    uint64_t bc = ~0ull;
    for (int k = max(0, k0 - 1); k <= min(30, k0 + 1); k++) {
        const uint64_t c = (uint64_t)m * (uint64_t)(k + 1) + (S >> k);
        if (c < bc) {
            bc = c;
            bk = (uint32_t)k;
        }
    }
    *cost = (uint32_t)(bc < 0x7fffffffull ? bc : 0x7fffffffull);
    return bk;
}

struct Cand {
    int kind, order, shift, prec, p;
    uint32_t bits; // subframe bits (estimate while choosing)
    int32_t qc[kFlacMaxLpc];
};

struct Smem {
    int32_t s[kFlacMaxBlock];
    union {
        double xw[kFlacMaxBlock];
        uint32_t bits[kMaxWords];
    } u;
    uint64_t tree[(2 << kMaxP) - 1]; // partition sums: level p at [2^p - 1, 2^(p+1) - 1)
    uint32_t lvl_cost[kMaxP + 1], lvl_kmax[kMaxP + 1];
    uint8_t kpar[1 << kMaxP];
    uint32_t crc_c[kT], crc_m[kT];
    uint32_t wsum32[4];
    double red[4][kFlacMaxLpc + 1];
    double lp[kFlacMaxLpc][kFlacMaxLpc];
    uint32_t flag, avail, qok;
    Cand cur, best;
    uint8_t hdr[16];
    uint32_t hdr_len;
};

// Price the candidate in sm.cur (kind, order, qc, shift) by partitioned Rice: sm.cur.bits and sm.cur.p; bits
// ~0u when no partition order is valid or an LPC residual does not fit in 32 bits.  All threads.
__device__ void price(Smem &sm, int n, int pfin)
{
    const int kind = sm.cur.kind, order = sm.cur.order, shift = sm.cur.shift;
    const uint32_t L = (uint32_t)n >> pfin, base = (1u << pfin) - 1u;
    const int t = threadIdx.x;
    for (uint32_t j = t; j < (1u << pfin); j += kT)
        sm.tree[base + j] = 0;
    if (t <= kMaxP) {
        sm.lvl_cost[t] = 0;
        sm.lvl_kmax[t] = 0;
    }
    if (t == 0)
        sm.flag = 0;
    __syncthreads();
    const int c = (n + kT - 1) / kT;
    const int lo = max(t * c, order), hi = min(n, (t + 1) * c);
    if (lo < hi) {
        uint32_t part = (uint32_t)lo / L, next = (part + 1) * L;
        uint64_t acc = 0;
        bool ovf = false;
        for (int i = lo; i < hi; i++) {
            if ((uint32_t)i >= next) {
                atomicAdd((unsigned long long *)&sm.tree[base + part], (unsigned long long)acc);
                acc = 0;
                part++;
                next += L;
            }
            const int64_t r = residual(sm.s, i, kind, order, sm.cur.qc, shift);
            ovf = ovf || r < INT32_MIN || r > INT32_MAX;
            acc += fold(r);
        }
        atomicAdd((unsigned long long *)&sm.tree[base + part], (unsigned long long)acc);
        if (ovf)
            atomicOr(&sm.flag, 1u);
    }
    __syncthreads();
    for (int p = pfin - 1; p >= 0; p--) {
        const uint32_t b = (1u << p) - 1u, bc = (2u << p) - 1u;
        for (uint32_t j = t; j < (1u << p); j += kT)
            sm.tree[b + j] = sm.tree[bc + 2 * j] + sm.tree[bc + 2 * j + 1];
        __syncthreads();
    }
    // each node of each valid level: its parameter and estimate
    for (uint32_t id = t; id < (2u << pfin) - 1u; id += kT) {
        const int p = 31 - __clz((int)(id + 1));
        const uint32_t j = id + 1 - (1u << p), len = (uint32_t)n >> p;
        if (len <= (uint32_t)order)
            continue;
        uint32_t cost;
        const uint32_t k = rice_param(sm.tree[id], len - (j == 0 ? order : 0), &cost);
        atomicAdd(&sm.lvl_cost[p], cost);
        atomicMax(&sm.lvl_kmax[p], k);
    }
    __syncthreads();
    if (t == 0) {
        uint32_t bestb = ~0u;
        int bp = 0;
        if (!sm.flag)
            for (int p = 0; p <= pfin; p++) {
                if (((uint32_t)n >> p) <= (uint32_t)order)
                    continue;
                const uint32_t w = sm.lvl_kmax[p] > 14 ? 5u : 4u;
                const uint32_t b = 6u + (w << p) + sm.lvl_cost[p];
                if (b < bestb) {
                    bestb = b;
                    bp = p;
                }
            }
        if (bestb != ~0u) {
            bestb += 8u + 16u * (uint32_t)order;
            if (kind == kLpc)
                bestb += 9u + (uint32_t)(sm.cur.prec * order);
        }
        sm.cur.bits = bestb;
        sm.cur.p = bp;
    }
    __syncthreads();
}

__device__ inline double tukey(int i, int n)
{
    const int np = n / 4 - 1; // Tukey(0.5) as libFLAC builds it
    if (np <= 0)
        return 1.0;
    if (i <= np)
        return 0.5 - 0.5 * cos(M_PI * (double)i / (double)np);
    if (i >= n - np - 1)
        return 0.5 - 0.5 * cos(M_PI * (double)(i - (n - np - 1) + np) / (double)np);
    return 1.0;
}

// LPC coefficient precision (bits, sign included) by block length, libFLAC's rule for 16-bit input
__device__ inline int lpc_precision(int n)
{
    return n <= 192 ? 7 : n <= 384 ? 8 : n <= 576 ? 9 : n <= 1152 ? 10 : n <= 2304 ? 11 : 12;
}

// Quantize lp[0..order) at precision prec: shift in 0..15 or false (libFLAC's rule, error feedback in order)
__device__ bool quantize(const double *lp, int order, int prec, int32_t *qc, int *shift)
{
    const int pr = prec - 1;
    const int32_t qmax = (1 << pr) - 1, qmin = -(1 << pr);
    double cmax = 0.0;
    for (int i = 0; i < order; i++)
        cmax = fmax(cmax, fabs(lp[i]));
    if (!(cmax > 0.0) || !isfinite(cmax))
        return false;
    int l2;
    (void)frexp(cmax, &l2);
    l2--;
    int sh = pr - l2 - 1;
    if (sh > 15)
        sh = 15;
    if (sh < 0)
        return false;
    double err = 0.0;
    for (int i = 0; i < order; i++) {
        err += lp[i] * (double)(1 << sh);
        double q = rint(err);
        q = fmin(fmax(q, (double)qmin), (double)qmax);
        err -= q;
        qc[i] = (int32_t)q;
    }
    *shift = sh;
    return true;
}

__device__ inline void copy_cand(Cand &d, const Cand &s)
{
    d.kind = s.kind;
    d.order = s.order;
    d.shift = s.shift;
    d.prec = s.prec;
    d.p = s.p;
    d.bits = s.bits;
    for (int j = 0; j < kFlacMaxLpc; j++)
        d.qc[j] = s.qc[j];
}

__device__ inline uint32_t crc8(const uint8_t *b, uint32_t n)
{
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; i++) {
        c ^= b[i];
        for (int k = 0; k < 8; k++)
            c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xffu : (c << 1) & 0xffu;
    }
    return c;
}

__global__ __launch_bounds__(kT) void k_flac_encode(FlacParams P, const FlacUtt *__restrict__ utts,
                                                    const FlacWork *__restrict__ work, uint32_t *__restrict__ fsize)
{
    __shared__ Smem sm;
    const int t = threadIdx.x;
    const FlacWork W = work[blockIdx.x];
    const FlacUtt &U = utts[W.utt];
    const uint64_t i0 = (uint64_t)W.frame * P.block_size;
    const int n = (int)(U.n - i0 < P.block_size ? U.n - i0 : P.block_size);
    const int16_t *x = U.x + i0;
    for (int i = t; i < n; i += kT)
        sm.s[i] = x[i];
    if (t == 0)
        sm.flag = 0;
    __syncthreads();
    {
        const int32_t s0 = sm.s[0];
        bool diff = false;
        for (int i = t; i < n; i += kT)
            diff = diff || sm.s[i] != s0;
        if (diff)
            atomicOr(&sm.flag, 1u);
    }
    __syncthreads();
    const bool constant = sm.flag == 0;
    int pfin = 0;
    while (pfin < kMaxP && ((uint32_t)n & ((2u << pfin) - 1u)) == 0)
        pfin++;
    if (t == 0) {
        sm.best.kind = constant ? kConstant : kVerbatim;
        sm.best.order = 0;
        sm.best.p = 0;
        sm.best.bits = constant ? 24u : 8u + 16u * (uint32_t)n;
    }
    __syncthreads();
    if (!constant) {
        // FIXED 0..4 (warm-up shorter than the block)
        for (int o = 0; o <= 4 && o < n; o++) {
            if (t == 0) {
                sm.cur.kind = kFixed;
                sm.cur.order = o;
                sm.cur.shift = 0;
                sm.cur.prec = 0;
            }
            __syncthreads();
            price(sm, n, pfin);
            if (t == 0 && sm.cur.bits < sm.best.bits)
                copy_cand(sm.best, sm.cur);
            __syncthreads();
        }
        const int mo = min((int)P.max_order, n - 1);
        if (mo > 0) {
            // window and autocorrelation, lags 0..mo: per-thread contiguous chunks, lane butterfly, then waves in order
            for (int i = t; i < n; i += kT)
                sm.u.xw[i] = (double)sm.s[i] * tukey(i, n);
            __syncthreads();
            double ac[kFlacMaxLpc + 1];
#pragma unroll
            for (int l = 0; l <= kFlacMaxLpc; l++)
                ac[l] = 0.0;
            const int c = (n + kT - 1) / kT;
            const int lo = t * c, hi = min(n, (t + 1) * c);
            for (int i = lo; i < hi; i++) {
                const double xi = sm.u.xw[i];
#pragma unroll
                for (int l = 0; l <= kFlacMaxLpc; l++)
                    if (l <= mo && i + l < n)
                        ac[l] += xi * sm.u.xw[i + l];
            }
#pragma unroll
            for (int l = 0; l <= kFlacMaxLpc; l++) {
                double v = ac[l];
                for (int d = 1; d < 64; d <<= 1)
                    v += __shfl_xor(v, d, 64);
                if (lane_id() == 0)
                    sm.red[t >> 6][l] = v;
            }
            __syncthreads();
            if (t == 0) {
                double acf[kFlacMaxLpc + 1], lpc[kFlacMaxLpc];
                for (int l = 0; l <= mo; l++)
                    acf[l] = ((sm.red[0][l] + sm.red[1][l]) + sm.red[2][l]) + sm.red[3][l];
                int avail = 0;
                double err = acf[0];
                if (err > 0.0 && isfinite(err)) {
                    for (int i = 0; i < mo; i++) {
                        double r = -acf[i + 1];
                        for (int j = 0; j < i; j++)
                            r -= lpc[j] * acf[i - j];
                        r /= err;
                        lpc[i] = r;
                        int j = 0;
                        for (; j < (i >> 1); j++) {
                            const double tmp = lpc[j];
                            lpc[j] += r * lpc[i - 1 - j];
                            lpc[i - 1 - j] += r * tmp;
                        }
                        if (i & 1)
                            lpc[j] += lpc[j] * r;
                        err *= (1.0 - r * r);
                        for (j = 0; j <= i; j++)
                            sm.lp[i][j] = -lpc[j];
                        avail = i + 1;
                        if (!(err > 0.0) || !isfinite(err))
                            break;
                    }
                }
                sm.avail = avail;
            }
            __syncthreads();
            const int ma = (int)sm.avail;
            for (int o = 1; o <= ma; o++) {
                if (!(o == ma || o == 2 || o == 4 || o == 8)) // a fixed set of orders: 2, 4, 8 and the highest
                    continue;
                if (t == 0) {
                    sm.cur.kind = kLpc;
                    sm.cur.order = o;
                    sm.cur.prec = lpc_precision(n);
                    sm.qok = quantize(sm.lp[o - 1], o, sm.cur.prec, sm.cur.qc, &sm.cur.shift) ? 1u : 0u;
                }
                __syncthreads();
                const bool ok = sm.qok != 0;
                __syncthreads();
                if (!ok)
                    continue; // (uniform)
                price(sm, n, pfin);
                if (t == 0 && sm.cur.bits < sm.best.bits)
                    copy_cand(sm.best, sm.cur);
                __syncthreads();
            }
        }
    }
    // the winner: Rice parameters of its partitions, then the exact code length by a scan
    const bool rice = sm.best.kind == kFixed || sm.best.kind == kLpc;
    uint32_t my_bits = 0, res_bits = 0, my_off = 0;
    int order = sm.best.order;
    uint32_t pw = 4, Lp = 1;
    const int c = (n + kT - 1) / kT;
    if (rice) {
        if (t == 0)
            copy_cand(sm.cur, sm.best);
        __syncthreads();
        price(sm, n, pfin);
        const int p = sm.best.p;
        Lp = (uint32_t)n >> p;
        for (uint32_t j = t; j < (1u << p); j += kT) {
            uint32_t cost;
            sm.kpar[j] = (uint8_t)rice_param(sm.tree[(1u << p) - 1u + j], Lp - (j == 0 ? order : 0), &cost);
        }
        __syncthreads();
        pw = sm.lvl_kmax[p] > 14 ? 5u : 4u;
        const int lo = max(t * c, order), hi = min(n, (t + 1) * c);
        for (int i = lo; i < hi; i++) {
            const uint32_t part = (uint32_t)i / Lp, k = sm.kpar[part];
            if (i == order || (uint32_t)i % Lp == 0)
                my_bits += pw;
            my_bits += 1u + k + (fold(residual(sm.s, i, sm.best.kind, order, sm.best.qc, sm.best.shift)) >> k);
        }
        my_off = block_excl_scan<uint32_t>(my_bits, sm.wsum32, &res_bits);
        if (t == 0) {
            uint32_t b = 8u + 16u * (uint32_t)order + 6u + res_bits;
            if (sm.best.kind == kLpc)
                b += 9u + (uint32_t)(sm.best.prec * order);
            sm.flag = b < 8u + 16u * (uint32_t)n ? b : 0u; // never larger than VERBATIM
        }
        __syncthreads();
    }
    const int kind = rice && sm.flag ? sm.best.kind : rice ? kVerbatim : sm.best.kind;
    if (kind == kVerbatim)
        order = 0;
    const uint32_t sub_bits = kind == kConstant ? 24u : kind == kVerbatim ? 8u + 16u * (uint32_t)n : sm.flag;
    // frame header (thread 0, bytes): sync, block size and rate codes, bit depth, frame number, extras, CRC-8
    if (t == 0) {
        uint8_t *h = sm.hdr;
        uint32_t bs_code, bs_extra = 0;
        if (n == 192)
            bs_code = 1;
        else if (n == 576 || n == 1152 || n == 2304 || n == 4608)
            bs_code = 2 + (uint32_t)(31 - __clz(n / 576));
        else if (n >= 256 && (n & (n - 1)) == 0)
            bs_code = 8 + (uint32_t)(31 - __clz(n / 256));
        else if (n <= 256)
            bs_code = 6, bs_extra = 8;
        else
            bs_code = 7, bs_extra = 16;
        h[0] = 0xff;
        h[1] = 0xf8;
        h[2] = (uint8_t)(bs_code << 4 | U.rate_code);
        h[3] = 0x08; // 16 bits per sample, mono
        uint32_t len = 4, v = W.frame;
        if (v < 0x80u) {
            h[len++] = (uint8_t)v;
        } else {
            int nb = v < 0x800u ? 2 : v < 0x10000u ? 3 : v < 0x200000u ? 4 : v < 0x4000000u ? 5 : 6;
            h[len++] = (uint8_t)((0xff00u >> nb) | (v >> (6 * (nb - 1))));
            for (int k = nb - 2; k >= 0; k--)
                h[len++] = (uint8_t)(0x80u | ((v >> (6 * k)) & 0x3fu));
        }
        if (bs_extra == 8)
            h[len++] = (uint8_t)(n - 1);
        else if (bs_extra == 16) {
            h[len++] = (uint8_t)((n - 1) >> 8);
            h[len++] = (uint8_t)(n - 1);
        }
        if (U.rate_bits == 8)
            h[len++] = (uint8_t)U.rate_val;
        else if (U.rate_bits == 16) {
            h[len++] = (uint8_t)(U.rate_val >> 8);
            h[len++] = (uint8_t)U.rate_val;
        }
        h[len] = (uint8_t)crc8(h, len);
        sm.hdr_len = len + 1;
    }
    __syncthreads();
    const uint32_t hdr_bits = sm.hdr_len * 8u;
    const uint32_t body = (hdr_bits + sub_bits + 7u) / 8u, frame_bytes = body + 2u;
    const uint32_t nwords = (frame_bytes + 3u) / 4u;
    for (uint32_t w = t; w <= nwords; w += kT)
        sm.u.bits[w] = 0;
    __syncthreads();
    uint32_t *bits = sm.u.bits;
    // header bytes, subframe header, warm-up, LPC header, residual header (thread 0)
    uint32_t pos = hdr_bits;
    if (t == 0) {
        for (uint32_t j = 0; j < sm.hdr_len; j++)
            put_bits(bits, 8u * j, 8, sm.hdr[j]);
        const uint32_t type = kind == kConstant ? 0u : kind == kVerbatim ? 1u : kind == kFixed ? 8u + (uint32_t)order
                                                                                                : 31u + (uint32_t)order;
        put_bits(bits, pos, 8, type << 1);
        pos += 8;
        if (kind == kConstant) {
            put_bits(bits, pos, 16, (uint16_t)sm.s[0]);
        } else if (kind != kVerbatim) {
            for (int j = 0; j < order; j++, pos += 16)
                put_bits(bits, pos, 16, (uint16_t)sm.s[j]);
            if (kind == kLpc) {
                const uint32_t pr = (uint32_t)sm.best.prec;
                put_bits(bits, pos, 4, pr - 1);
                put_bits(bits, pos + 4, 5, (uint32_t)sm.best.shift);
                pos += 9;
                for (int j = 0; j < order; j++, pos += pr)
                    put_bits(bits, pos, pr, (uint32_t)sm.best.qc[j] & ((1u << pr) - 1u));
            }
            put_bits(bits, pos, 2, pw == 5 ? 1u : 0u);
            put_bits(bits, pos + 2, 4, (uint32_t)sm.best.p);
        }
    }
    if (kind == kVerbatim) {
        for (int i = t; i < n; i += kT)
            put_bits(bits, hdr_bits + 8u + 16u * (uint32_t)i, 16, (uint16_t)sm.s[i]);
    } else if (kind != kConstant) {
        uint32_t q = hdr_bits + 8u + 16u * (uint32_t)order + 6u + my_off;
        if (kind == kLpc)
            q += 9u + (uint32_t)(sm.best.prec * order);
        const int lo = max(t * c, order), hi = min(n, (t + 1) * c);
        for (int i = lo; i < hi; i++) {
            const uint32_t part = (uint32_t)i / Lp, k = sm.kpar[part];
            if (i == order || (uint32_t)i % Lp == 0) {
                put_bits(bits, q, pw, k);
                q += pw;
            }
            const uint32_t uu = fold(residual(sm.s, i, kind, order, sm.best.qc, sm.best.shift));
            const uint32_t qq = uu >> k;
            put_bits(bits, q + qq, k + 1u, (1u << k) | (uu & ((1u << k) - 1u)));
            q += qq + 1u + k;
        }
    }
    __syncthreads();
    // CRC-16 of bytes [0, body): segments from zero state, joined in order by x^(8 len)
    {
        const uint32_t cb = (body + kT - 1) / kT, lo = min(body, (uint32_t)t * cb), hi = min(body, lo + cb);
        uint32_t crc = 0;
        for (uint32_t j = lo; j < hi; j++) {
            crc ^= get_byte(bits, j) << 8;
            for (int k = 0; k < 8; k++)
                crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xffffu : (crc << 1) & 0xffffu;
        }
        sm.crc_c[t] = crc;
        sm.crc_m[t] = gf_shift(hi - lo);
        __syncthreads();
        for (int s = 1; s < kT; s <<= 1) {
            if ((t & (2 * s - 1)) == 0) {
                sm.crc_c[t] = gf_mulmod(sm.crc_c[t], sm.crc_m[t + s]) ^ sm.crc_c[t + s];
                sm.crc_m[t] = gf_mulmod(sm.crc_m[t], sm.crc_m[t + s]);
            }
            __syncthreads();
        }
        if (t == 0) {
            put_bits(bits, 8u * body, 16, sm.crc_c[0]);
            fsize[U.frame0 + W.frame] = frame_bytes;
        }
        __syncthreads();
    }
    uint32_t *slot = (uint32_t *)(U.slots + (uint64_t)W.frame * P.slot_bytes);
    for (uint32_t w = t; w < nwords; w += kT)
        slot[w] = __builtin_bswap32(bits[w]);
}

// Per utterance: frame offsets in its stream (after its header), size, min and max frame size
__global__ __launch_bounds__(kT) void k_flac_scan(const FlacUtt *__restrict__ utts, const uint32_t *__restrict__ fsize,
                                                  uint64_t *__restrict__ foff, FlacOut *__restrict__ out)
{
    __shared__ uint64_t wsum[4];
    __shared__ uint32_t mn, mx;
    const FlacUtt &U = utts[blockIdx.x];
    const int t = threadIdx.x;
    const uint32_t nf = U.nframes, c = (nf + kT - 1) / kT, lo = min(nf, t * c), hi = min(nf, lo + c);
    if (t == 0) {
        mn = ~0u;
        mx = 0;
    }
    uint64_t acc = 0;
    uint32_t lmn = ~0u, lmx = 0;
    for (uint32_t f = lo; f < hi; f++) {
        const uint32_t z = fsize[U.frame0 + f];
        acc += z;
        lmn = min(lmn, z);
        lmx = max(lmx, z);
    }
    __syncthreads();
    if (lo < hi) {
        atomicMin(&mn, lmn);
        atomicMax(&mx, lmx);
    }
    uint64_t tot;
    uint64_t off = U.header_bytes + block_excl_scan<uint64_t>(acc, wsum, &tot);
    for (uint32_t f = lo; f < hi; f++) {
        foff[U.frame0 + f] = off;
        off += fsize[U.frame0 + f];
    }
    if (t == 0) {
        out[blockIdx.x].bytes = U.header_bytes + tot;
        out[blockIdx.x].min_frame = nf ? mn : 0;
        out[blockIdx.x].max_frame = nf ? mx : 0;
    }
}

// Each utterance's offset in the compact slab: utterance order
__global__ __launch_bounds__(kT) void k_flac_place(FlacOut *__restrict__ out, uint32_t n, uint64_t *__restrict__ total)
{
    __shared__ uint64_t wsum[4];
    const int t = threadIdx.x;
    const uint32_t c = (n + kT - 1) / kT, lo = min(n, t * c), hi = min(n, lo + c);
    uint64_t acc = 0;
    for (uint32_t u = lo; u < hi; u++)
        acc += out[u].bytes;
    uint64_t tot;
    uint64_t off = block_excl_scan<uint64_t>(acc, wsum, &tot);
    for (uint32_t u = lo; u < hi; u++) {
        out[u].off = off;
        off += out[u].bytes;
    }
    if (t == 0)
        *total = tot;
}

// fLaC, the STREAMINFO block header (type 0, 34 bytes; last unless a SEEKTABLE follows) and STREAMINFO, its MD5 from
// digests (null: zeros, "not computed"), then the SEEKTABLE's block header (last, type 3) where the utterance has
// points; byte stores (the first frame may share the last word)
__global__ __launch_bounds__(kT) void k_flac_header(FlacParams P, const FlacUtt *__restrict__ utts, uint32_t n,
                                                    const FlacOut *__restrict__ out, const uint32_t *__restrict__ digests,
                                                    uint8_t *__restrict__ dst)
{
    const uint32_t u = blockIdx.x * kT + threadIdx.x;
    if (u >= n)
        return;
    const FlacUtt &U = utts[u];
    const FlacOut &o = out[u];
    // 20 bits rate, 3 bits channels - 1, 5 bits depth - 1, 36 bits total samples
    const uint64_t v = ((uint64_t)U.hz << 44) | (15ull << 36) | (U.n & 0xfffffffffull);
    const uint64_t bs = P.block_size, mn = o.min_frame, mx = o.max_frame;
    const uint64_t w[4] = {U.n_points ? 0x664C614300000022ull : 0x664C614380000022ull, // fLaC, (last,) type 0, 34 bytes
                           (bs << 48) | (bs << 32) | (mn << 8) | (mx >> 16), ((mx & 0xffffull) << 48) | (v >> 16),
                           (v & 0xffffull) << 48};
    uint8_t *d = dst + o.off;
#pragma unroll
    for (int k = 0; k < 32; k++)
        d[k] = (uint8_t)(w[k >> 3] >> (56 - 8 * (k & 7)));
    // bytes 26..41: A, B, C, D of the digest, each little-endian
#pragma unroll
    for (int k = 0; k < 16; k++)
        d[26 + k] = digests ? (uint8_t)(digests[4 * (size_t)u + (k >> 2)] >> (8 * (k & 3))) : 0;
    if (U.n_points) {
        const uint32_t len = kFlacSeekPointBytes * U.n_points;
        d[42] = 0x83;
        d[43] = (uint8_t)(len >> 16);
        d[44] = (uint8_t)(len >> 8);
        d[45] = (uint8_t)len;
    }
}

// Seek point p of utterance blockIdx.x: frame p * seek_step
__global__ __launch_bounds__(kT) void k_flac_seektable(FlacParams P, const FlacUtt *__restrict__ utts,
                                                       const uint64_t *__restrict__ foff,
                                                       const FlacOut *__restrict__ out, uint8_t *__restrict__ dst)
{
    const FlacUtt &U = utts[blockIdx.x];
    const uint32_t p = blockIdx.y * kT + threadIdx.x;
    if (p >= U.n_points)
        return;
    const uint64_t f = (uint64_t)p * U.seek_step, s0 = f * P.block_size;
    const uint64_t off = foff[U.frame0 + f] - U.header_bytes;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(P.block_size, U.n - s0);
    uint8_t *d = dst + out[blockIdx.x].off + kFlacStreamInfoBytes + 4 + (uint64_t)kFlacSeekPointBytes * p;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        d[k] = (uint8_t)(s0 >> (56 - 8 * k));
        d[8 + k] = (uint8_t)(off >> (56 - 8 * k));
    }
    d[16] = (uint8_t)(cnt >> 8);
    d[17] = (uint8_t)cnt;
}

#define JB_FLAC_GLOBAL __attribute__((address_space(1)))

// One lane per utterance of the list: the chain of jb_md5.h over its samples, the digest by plain stores
__global__ __launch_bounds__(64) void k_flac_md5(const FlacUtt *__restrict__ utts, const uint32_t *__restrict__ order,
                                                 uint32_t n_order, uint32_t *__restrict__ digests)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_order)
        return;
    const uint32_t u = order[i];
    const JB_FLAC_GLOBAL int16_t *x = (const JB_FLAC_GLOBAL int16_t *)utts[u].x;
    const JB_FLAC_GLOBAL uint32_t *w = (const JB_FLAC_GLOBAL uint32_t *)((uintptr_t)x & ~(uintptr_t)3);
    uint32_t st[4];
    md5_samples(
        utts[u].n, ((uintptr_t)x & 2u) != 0, [&](uint64_t k) { return w[k]; }, [&](uint64_t k) { return x[k]; }, st);
    JB_FLAC_GLOBAL uint32_t *d = (JB_FLAC_GLOBAL uint32_t *)digests + 4 * (size_t)u;
#pragma unroll
    for (int j = 0; j < 4; j++)
        d[j] = st[j];
}

__global__ __launch_bounds__(kT) void k_flac_compact(FlacParams P, const FlacUtt *__restrict__ utts,
                                                     const FlacWork *__restrict__ work, const uint32_t *__restrict__ fsize,
                                                     const uint64_t *__restrict__ foff, const FlacOut *__restrict__ out,
                                                     uint8_t *__restrict__ dst)
{
    const FlacWork W = work[blockIdx.x];
    const FlacUtt &U = utts[W.utt];
    const uint64_t g = U.frame0 + W.frame;
    const uint32_t len = fsize[g];
    const uint8_t *src = U.slots + (uint64_t)W.frame * P.slot_bytes;
    const uint32_t *sw = (const uint32_t *)src;
    const uint64_t d0 = out[W.utt].off + foff[g], d1 = d0 + len;
    const uint64_t a = std::min<uint64_t>(d1, (d0 + 3) & ~3ull), b = std::max<uint64_t>(a, d1 & ~3ull);
    const int t = threadIdx.x;
    for (uint64_t k = d0 + t; k < a; k += kT)
        dst[k] = src[k - d0];
    for (uint64_t k = b + t; k < d1; k += kT)
        dst[k] = src[k - d0];
    const uint32_t sh = (uint32_t)((a - d0) & 3u) * 8u, w0 = (uint32_t)((a - d0) >> 2);
    uint32_t *dw = (uint32_t *)(dst + a);
    for (uint32_t w = t; w < (uint32_t)((b - a) >> 2); w += kT) {
        const uint32_t lo = sw[w0 + w];
        dw[w] = sh ? (lo >> sh) | (sw[w0 + w + 1] << (32u - sh)) : lo;
    }
}
} // namespace

hipError_t launch_flac_encode(const FlacParams &p, const FlacUtt *utts, const FlacWork *work, uint32_t n_work,
                              uint32_t *fsize, hipStream_t stream)
{
    if (n_work)
        hipLaunchKernelGGL(k_flac_encode, dim3(n_work), dim3(kT), 0, stream, p, utts, work, fsize);
    return hipGetLastError();
}

hipError_t launch_flac_md5(const FlacUtt *utts, const uint32_t *order, uint32_t n_order, uint32_t *digests,
                           hipStream_t stream)
{
    if (n_order)
        hipLaunchKernelGGL(k_flac_md5, dim3((n_order + 63) / 64), dim3(64), 0, stream, utts, order, n_order, digests);
    return hipGetLastError();
}

hipError_t launch_flac_pack(const FlacParams &p, const FlacUtt *utts, uint32_t n_utts, const FlacWork *work,
                            uint32_t n_frames, const uint32_t *fsize, uint64_t *foff, FlacOut *out, uint64_t *total,
                            uint8_t *dst, hipStream_t stream, const uint32_t *digests, uint32_t max_points)
{
    if (!n_utts)
        return hipSuccess;
    hipLaunchKernelGGL(k_flac_scan, dim3(n_utts), dim3(kT), 0, stream, utts, fsize, foff, out);
    hipLaunchKernelGGL(k_flac_place, dim3(1), dim3(kT), 0, stream, out, n_utts, total);
    hipLaunchKernelGGL(k_flac_header, dim3((n_utts + kT - 1) / kT), dim3(kT), 0, stream, p, utts, n_utts, out,
                       digests, dst);
    if (max_points)
        hipLaunchKernelGGL(k_flac_seektable, dim3(n_utts, (max_points + kT - 1) / kT), dim3(kT), 0, stream, p, utts,
                           foff, out, dst);
    if (n_frames)
        hipLaunchKernelGGL(k_flac_compact, dim3(n_frames), dim3(kT), 0, stream, p, utts, work, fsize, foff, out, dst);
    return hipGetLastError();
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_flac_encode_pcm_batch_meta(const int16_t *const *in, const size_t *n_in, size_t n, uint32_t hz,
                                  const jb_flac_opts *opts, const jb_flac_meta *meta, int32_t device, uint8_t **out,
                                  size_t *n_out)
{
    FlacParams p{};
    FlacMeta m{};
    int rc = flac_check_opts(opts, &p);
    if (rc || (rc = flac_check_meta(meta, &m)))
        return rc;
    const bool md5 = (m.flags & kFlacMetaMd5) != 0;
    if ((rc = pcm_check((const void *const *)in, n_in, n, out && n_out, (void **)out, n_out)))
        return rc;
    {
        uint32_t c, b, v;
        if ((rc = flac_rate_code(hz, &c, &b, &v)))
            return rc;
    }
    DeviceScratch ds;
    if ((rc = ds.open(device, "jb_flac_encode_pcm_batch")))
        return rc;
    std::vector<uint64_t> off;
    const int16_t *dx = ds.pack(in, n_in, n, &off);
    std::vector<uint64_t> ns(n_in, n_in + n);
    std::vector<uint32_t> hzs(n, hz);
    std::vector<const int16_t *> xs(n);
    for (size_t u = 0; u < n; u++)
        xs[u] = dx + off[u];
    std::vector<FlacUtt> utts;
    std::vector<FlacWork> work;
    std::vector<uint32_t> order;
    uint64_t slot_bytes = 0, bound = 0;
    if ((rc = flac_plan(p, m, xs.data(), ns.data(), hzs.data(), n, &utts, &work, &slot_bytes, &bound)))
        return rc;
    uint32_t max_points = 0;
    for (const FlacUtt &w : utts)
        max_points = std::max(max_points, w.n_points);
    uint32_t *dord = nullptr, *ddig = nullptr;
    if (md5) {
        flac_md5_order(utts, nullptr, &order);
        dord = ds.upload(order);
        ddig = ds.alloc<uint32_t>(4 * n);
    }
    uint8_t *dslots = ds.alloc<uint8_t>(std::max<uint64_t>(slot_bytes, 4));
    uint8_t *dout = ds.alloc<uint8_t>(std::max<uint64_t>(bound, 4));
    flac_bind(&utts, dslots);
    const FlacUtt *du = ds.upload(utts);
    const FlacWork *dw = ds.upload(work);
    uint32_t *dfs = ds.alloc<uint32_t>(work.size());
    uint64_t *dfo = ds.alloc<uint64_t>(work.size()), *dtot = ds.alloc<uint64_t>(1);
    FlacOut *dres = ds.alloc<FlacOut>(n);
    if (ds.ok())
        ds.err = launch_flac_encode(p, du, dw, (uint32_t)work.size(), dfs, ds.stream);
    if (ds.ok() && md5)
        ds.err = launch_flac_md5(du, dord, (uint32_t)order.size(), ddig, ds.stream);
    if (ds.ok())
        ds.err = launch_flac_pack(p, du, (uint32_t)n, dw, (uint32_t)work.size(), dfs, dfo, dres, dtot, dout, ds.stream,
                                  md5 ? ddig : nullptr, max_points);
    // the streams' sizes and places first, then the used part of the compact slab
    std::vector<FlacOut> res;
    std::vector<uint64_t> total;
    std::vector<uint8_t> host;
    ds.read_back(&res, dres, n);
    ds.read_back(&total, dtot, n ? 1 : 0);
    ds.read_back(&host, dout, total.empty() ? 0 : total[0]);
    if ((rc = ds.status()))
        return rc;
    std::vector<PcmShare> shares(n);
    for (size_t u = 0; u < n; u++)
        shares[u] = {res[u].off, res[u].bytes};
    return hand_out(host.data(), 1, shares, (void **)out, n_out);
}

int jb_flac_encode_pcm_batch(const int16_t *const *in, const size_t *n_in, size_t n, uint32_t hz,
                             const jb_flac_opts *opts, int32_t device, uint8_t **out, size_t *n_out)
{
    return jb_flac_encode_pcm_batch_meta(in, n_in, n, hz, opts, nullptr, device, out, n_out);
}

int jb_flac_md5_pcm_batch(const int16_t *const *in, const size_t *n_in, size_t n, int32_t device, uint8_t *digests)
{
    int rc = pcm_check((const void *const *)in, n_in, n, digests != nullptr);
    if (rc || !n)
        return rc;
    DeviceScratch ds;
    if ((rc = ds.open(device, "jb_flac_md5_pcm_batch")))
        return rc;
    // the inputs packed one after the other, as a batch's 16-bit slab has them: a start is only 2-byte aligned
    std::vector<uint64_t> off;
    const int16_t *dx = ds.pack(in, n_in, n, &off);
    std::vector<FlacUtt> utts(n);
    for (size_t u = 0; u < n; u++) {
        utts[u].x = dx + off[u];
        utts[u].n = n_in[u];
    }
    std::vector<uint32_t> order, dig;
    flac_md5_order(utts, nullptr, &order);
    const FlacUtt *du = ds.upload(utts);
    const uint32_t *dord = ds.upload(order);
    uint32_t *ddig = ds.alloc<uint32_t>(4 * n);
    if (ds.ok())
        ds.err = launch_flac_md5(du, dord, (uint32_t)n, ddig, ds.stream);
    ds.read_back(&dig, ddig, 4 * n);
    if ((rc = ds.status()))
        return rc;
    memcpy(digests, dig.data(), 16 * n); // A, B, C, D little-endian: the digest's byte order (a little-endian host)
    return JB_OK;
}

void jb_flac_free(uint8_t *p) { free(p); }

} // extern "C"

// Output-rate conversion of synthesized PCM (new surface: the reference only emits the voice's own rate).
//
// Filter: rational polyphase resampling with a Kaiser-windowed sinc, designed in f64 on the host
// (resample_design, the one definition; jb_resample_filter hands its table out so that tests recompute it):
//   g = gcd(in, out), L = out / g, M = in / g, r = min(1, L / M)
//   fc = 0.45 r cycles per input sample, H = 32 / (2 fc) input samples, C = ceil(H), ntaps = 2 C
//   h(t) = 2 fc sinc(2 fc t) I0(10 sqrt(1 - (t / H)^2)) / I0(10) for |t| < H, else 0
//   output k of an utterance of N input samples: q = floor(k M / L), p = k M mod L,
//   y[k] = sum_{j = 0}^{ntaps - 1} h[p][j] x[q - C + 1 + j],  h[p][j] = h(p / L + C - 1 - j),
//   x = 0 outside [0, N), n_out = ceil(N L / M)
// Every utterance is resampled alone: no filter reaches across an utterance boundary.
//
// k_resample: one workgroup (four waves) per tile of `rows` output rows; row m of an utterance holds its outputs
// k = m L + r, r = 0..L-1, whose phase (r M) mod L does not depend on m, and a wave computes output r of 64 rows: ONE
// phase p, so that h[p][j] is the same for every lane (a wave-uniform load: the scalar unit, not a per-lane gather of
// outputs x ntaps x 8 bytes).  Lane i's inputs start at (m0 + i) M + floor(r M / L) - C + 1: the tile's input window
// (rows M + ntaps samples) is staged in LDS first,
// zero outside the utterance, and read lane-strided from there.  Where M has a large power-of-two factor (22.05
// and 44.1 kHz from 48 kHz: M = 320, 160) that stride would put every lane of a half-wave on one bank pair; those
// tables store the window with one pad double per 2^s (s picked per M: conflict-free for 2, 160, 320).  A table whose window does not
// fit the LDS budget (extreme ratios) reads the utterance from global memory instead.
// Each output is h[p][0] x[.] followed by ntaps - 1 explicit FMAs in ascending j: a function of x and h alone, not
// of the tile, wave or lane it was computed on (the fast invariant mode stays invariant).  An identity table
// (L = M = 1, one tap 1.0) copies: 1.0 * x is x, the sign of a zero included.
#include "jb_host.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <numeric>
#include <tuple>

namespace jb {

namespace {
constexpr int kRsThreads = 256;          // four waves
// LDS slots of a tile's input window, pad doubles included: 64 KiB, the default limit of a launch's dynamic LDS (the
// hardware lets one workgroup take all 160 KiB once hipFuncSetAttribute raises that limit; this kernel does not: its
// windows of small M take a few KB, and at M = 320 even 160 KiB would hold 61 rows, one workgroup per CU -- the rows
// of large-M tables need another mapping, not more LDS)
constexpr uint32_t kRsLdsDoubles = 8192;
constexpr uint32_t kRsCopyRows = 16384; // outputs per tile of the identity table (a copy: no window, no taps)

constexpr size_t kRsLdsMaxBytes = sizeof(double) * kRsLdsDoubles;

// pad shift of a window: slot(e) = e + (e >> shift) spreads the bank pairs (slot mod 32) of a half-wave's 32 lanes,
// rows M apart; the shift (none, 4..7) with the fewest lanes on the busiest pair
uint32_t pick_pad_shift(uint32_t M)
{
    uint32_t best = 0, best_worst = 33;
    for (uint32_t sh : {0u, 4u, 5u, 6u, 7u}) {
        uint32_t cnt[32] = {}, worst = 0;
        for (uint32_t i = 0; i < 32; i++) {
            const uint64_t e = (uint64_t)i * M;
            worst = std::max(worst, ++cnt[(sh ? e + (e >> sh) : e) % 32]);
        }
        if (worst < best_worst) {
            best_worst = worst;
            best = sh;
        }
    }
    return best;
}

double bessel_i0(double x)
{
    // power series sum_k ((x/2)^k / k!)^2: all terms positive, 60 of them reach the rounding floor for x <= 10
    double sum = 1.0, term = 1.0;
    const double h = 0.25 * x * x;
    for (int k = 1; k < 60; k++) {
        term *= h / ((double)k * (double)k);
        sum += term;
    }
    return sum;
}
} // namespace

int resample_design(uint32_t in_hz, uint32_t out_hz, ResampleSpec *spec, std::vector<double> *taps)
{
    if (in_hz == 0 || out_hz == 0) {
        set_error("resample: a rate of 0 Hz");
        return JB_ERR_INVALID;
    }
    uint64_t L, M;
    resample_ratio(in_hz, out_hz, &L, &M);
    if (L > kResampleMaxLM || M > kResampleMaxLM) {
        set_error("resample: " + std::to_string(in_hz) + " Hz -> " + std::to_string(out_hz) + " Hz reduces to L/M = " +
                  std::to_string(L) + "/" + std::to_string(M) + "; supported are L <= 2048 and M <= 2048");
        return JB_ERR_UNSUPPORTED;
    }
    const double r = std::min(1.0, (double)L / (double)M);
    const double fc = 0.45 * r;
    const double H = 32.0 / (2.0 * fc);
    const uint32_t C = (uint32_t)std::ceil(H);
    ResampleSpec s{};
    s.L = (uint32_t)L;
    s.M = (uint32_t)M;
    s.C = C;
    s.ntaps = 2 * C;
    if (spec)
        *spec = s;
    if (taps) {
        taps->assign((size_t)s.L * s.ntaps, 0.0);
        const double i0b = bessel_i0(10.0), pi = 3.14159265358979323846;
        for (uint32_t p = 0; p < s.L; p++)
            for (uint32_t j = 0; j < s.ntaps; j++) {
                const double t = (double)p / (double)L + (double)C - 1.0 - (double)j;
                if (std::fabs(t) >= H)
                    continue;
                const double x = 2.0 * fc * t;
                const double sinc = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
                const double u = t / H;
                (*taps)[(size_t)p * s.ntaps + j] = 2.0 * fc * sinc * bessel_i0(10.0 * std::sqrt(1.0 - u * u)) / i0b;
            }
    }
    return JB_OK;
}

// The path of a pair: which mapping k_resample runs and with what tile, from (L, M, ntaps) alone -- no device
int resample_geometry(uint32_t in_hz, uint32_t out_hz, ResampleGeom *out, std::vector<double> *taps)
{
    ResampleSpec s{};
    const bool identity = in_hz == out_hz; // what a native-rate utterance of a converting batch goes through
    if (identity) {
        s = ResampleSpec{1, 1, 1, 1};
        if (taps)
            taps->assign(1, 1.0);
    } else {
        int rc = resample_design(in_hz, out_hz, &s, taps);
        if (rc)
            return rc;
    }
    ResampleGeom g{};
    g.L = s.L;
    g.M = s.M;
    g.C = s.C;
    g.ntaps = s.ntaps;
    // pad doubles where a half-wave's lane stride M hits few bank pairs (a double's pair is its index mod 32: rows M
    // apart take 32 / gcd(M, 32) of them)
    g.pad = pick_pad_shift(s.M);
    // rows per tile: the window (rows M + ntaps samples, and its pad) within the LDS budget, 64 rows per wave at most
    const uint64_t cap = g.pad ? ((uint64_t)(kRsLdsDoubles - 1) << g.pad) / ((1u << g.pad) + 1) : kRsLdsDoubles;
    const uint64_t fit = s.ntaps + (uint64_t)s.M <= cap ? (cap - s.ntaps) / s.M : 0;
    g.cap = (uint32_t)cap;
    g.fit = (uint32_t)fit;
    if (identity) {
        // a copy (or the 16-bit conversion alone): y[k] = x[k], large tiles straight from global memory
        g.identity = 1;
        g.lds = 0;
        g.pad = 0;
        g.rows = kRsCopyRows;
        g.row_waves = 4;
    } else if (fit == 0) {
        g.lds = 0;
        g.pad = 0;
        g.rows = 256;
        g.row_waves = 4;
    } else {
        g.lds = 1;
        if (fit >= 256) {
            g.rows = 256;
            g.row_waves = 4;
        } else if (fit >= 128) {
            g.rows = 128;
            g.row_waves = 2;
        } else {
            g.rows = (uint32_t)std::min<uint64_t>(fit, 64);
            g.row_waves = 1;
        }
        // a launch allocates only what its tiles' windows take (16 kHz from 48 kHz: 8 KB), so that up to eight
        // workgroups share a CU and hide the latency of each lane's chain of dependent FMAs
        const uint32_t wlen = g.rows * s.M + s.ntaps;
        g.lds_bytes = (uint32_t)(sizeof(double) * (g.pad ? wlen + (wlen >> g.pad) + 1 : wlen));
    }
    *out = g;
    return JB_OK;
}

// Device tables, one per (device, in_hz, out_hz), kept for the process (the largest of the common pairs is 179 KB)
namespace {
struct TableKey {
    int device;
    uint32_t in_hz, out_hz;
    bool operator<(const TableKey &o) const
    {
        return std::tie(device, in_hz, out_hz) < std::tie(o.device, o.in_hz, o.out_hz);
    }
};
std::mutex g_rs_mu;
std::map<TableKey, ResampleTable> &g_rs_tables = *new std::map<TableKey, ResampleTable>();
} // namespace

int resample_table(int device, uint32_t in_hz, uint32_t out_hz, ResampleTable *out)
{
    std::lock_guard<std::mutex> lk(g_rs_mu);
    auto it = g_rs_tables.find(TableKey{device, in_hz, out_hz});
    if (it != g_rs_tables.end()) {
        *out = it->second;
        return JB_OK;
    }
    ResampleGeom g{};
    std::vector<double> taps;
    int rc = resample_geometry(in_hz, out_hz, &g, &taps);
    if (rc)
        return rc;
    ResampleTable t{};
    t.L = g.L;
    t.M = g.M;
    t.C = g.C;
    t.ntaps = g.ntaps;
    t.rows = g.rows;
    t.row_waves = g.row_waves;
    t.lds = g.lds;
    t.pad = g.pad;
    t.lds_bytes = g.lds_bytes;
    t.identity = g.identity;
    // on `device`, whatever the calling thread has current (and that stays current afterwards)
    DeviceScratch scope;
    hipError_t e = scope.enter(device);
    if (e == hipSuccess)
        e = hipMalloc((void **)&t.h, sizeof(double) * taps.size());
    if (e == hipSuccess)
        e = hipMemcpy((void *)t.h, taps.data(), sizeof(double) * taps.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (t.h)
            (void)hipFree((void *)t.h);
        return hip_fail(e, "resample table");
    }
    g_rs_tables[TableKey{device, in_hz, out_hz}] = t;
    *out = t;
    return JB_OK;
}

void resample_tiles(const ResampleTable &t, uint32_t table, const double *x, uint64_t n_in, void *y, uint64_t n_out,
                    std::vector<ResampleTile> &tiles)
{
    const uint64_t rows = (n_out + t.L - 1) / t.L;
    for (uint64_t m0 = 0; m0 < rows; m0 += t.rows) {
        ResampleTile w{};
        w.x = x;
        w.y = y;
        w.n_in = n_in;
        w.n_out = n_out;
        w.m0 = m0;
        w.rows = (uint32_t)std::min<uint64_t>(t.rows, rows - m0);
        w.table = table;
        tiles.push_back(w);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// PCM sink of the reference's callers (examples/is-bonsai/main.rs:44-48): clamp, then truncate toward zero --
// the rule of the vocoder's 16-bit sink (jb_vocoder.hip pcm_i16)
__device__ __forceinline__ int16_t rs_i16(double v)
{
    v = fmin(v, 32767.0);
    v = fmax(v, -32768.0);
    return (int16_t)(int)v;
}
template <class T> __device__ __forceinline__ void rs_store(T *y, uint64_t k, double v);
template <> __device__ __forceinline__ void rs_store<double>(double *y, uint64_t k, double v) { y[k] = v; }
template <> __device__ __forceinline__ void rs_store<int16_t>(int16_t *y, uint64_t k, double v) { y[k] = rs_i16(v); }

template <bool kPad> __device__ __forceinline__ uint32_t rs_slot(uint32_t e, uint32_t sh)
{
    return kPad ? e + (e >> sh) : e;
}

// the tile's rows at the phases of this wave, inputs from `src` (LDS window, or the utterance in global memory)
template <class T, bool kLds, bool kPad>
__device__ __forceinline__ void rs_rows(const ResampleTable &tb, const ResampleTile &tl, const double *src, int64_t win0)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t L = tb.L, M = tb.M, ntaps = tb.ntaps;
    const uint32_t rw = tb.row_waves, pstep = (kRsThreads / 64) / rw;
    const uint32_t i = (wave % rw) * 64 + lane; // row of the tile
    const bool row_ok = i < tl.rows;
    T *y = (T *)tl.y;
    for (uint32_t r = wave / rw; r < L; r += pstep) {
        // output r of each row: k = m L + r, so k M = m L M + r M -- phase (r M) mod L and q = m M + floor(r M / L),
        // the same phase for every row (lane) of the wave
        const uint64_t k = (tl.m0 + i) * (uint64_t)L + r;
        const bool ok = row_ok && k < tl.n_out;
        const uint32_t qp = (uint32_t)(((uint64_t)r * M) / L);
        const uint32_t p = (uint32_t)(((uint64_t)r * M) % L);
        // the phase's taps through the constant address space: scalar loads (SGPR operands of the FMAs), not a vector
        // load of one address per lane
        const __attribute__((address_space(4))) double *h =
            (const __attribute__((address_space(4))) double *)(tb.h + (size_t)p * ntaps);
        double acc;
        if (kLds) {
            const uint32_t e0 = (ok ? i : 0) * M + qp; // window-relative first input of this output
            const uint32_t sh = tb.pad;
            acc = h[0] * src[rs_slot<kPad>(e0, sh)];
            for (uint32_t j = 1; j < ntaps; j++)
                acc = __builtin_fma(h[j], src[rs_slot<kPad>(e0 + j, sh)], acc);
        } else {
            const int64_t a0 = win0 + (int64_t)((ok ? i : 0) * (uint64_t)M + qp);
            auto xin = [&](int64_t a) { return (a >= 0 && a < (int64_t)tl.n_in) ? src[a] : 0.0; };
            acc = h[0] * xin(a0);
            for (uint32_t j = 1; j < ntaps; j++)
                acc = __builtin_fma(h[j], xin(a0 + j), acc);
        }
        if (ok)
            rs_store<T>(y, k, acc);
    }
}

template <class T>
__global__ __launch_bounds__(kRsThreads) void k_resample(const ResampleTable *__restrict__ tables,
                                                         const ResampleTile *__restrict__ tiles)
{
    extern __shared__ double win[];
    const ResampleTile tl = tiles[blockIdx.x];
    const ResampleTable tb = tables[tl.table];
    if (tb.identity) { // y = x (1.0 * x, the sign of a zero included), or its 16-bit conversion
        for (uint64_t k = tl.m0 + threadIdx.x; k < tl.m0 + tl.rows; k += kRsThreads)
            rs_store<T>((T *)tl.y, k, tl.x[k]);
        return;
    }
    // first input of the window: row m0, phase 0, tap 0
    const int64_t win0 = (int64_t)(tl.m0 * (uint64_t)tb.M) - (int64_t)tb.C + 1;
    if (!tb.lds) {
        rs_rows<T, false, false>(tb, tl, tl.x, win0);
        return;
    }
    const uint32_t wlen = tl.rows * tb.M + tb.ntaps; // covers row rows-1, phase L-1, tap ntaps-1
    for (uint32_t e = threadIdx.x; e < wlen; e += kRsThreads) {
        const int64_t a = win0 + (int64_t)e;
        const double v = (a >= 0 && a < (int64_t)tl.n_in) ? tl.x[a] : 0.0;
        if (tb.pad)
            win[rs_slot<true>(e, tb.pad)] = v;
        else
            win[e] = v;
    }
    __syncthreads();
    if (tb.pad)
        rs_rows<T, true, true>(tb, tl, win, win0);
    else
        rs_rows<T, true, false>(tb, tl, win, win0);
}

hipError_t launch_resample(const ResampleTable *tables_dev, const ResampleTile *tiles_dev, uint32_t n_tiles, bool i16,
                           size_t lds_bytes, hipStream_t stream)
{
    if (n_tiles == 0)
        return hipSuccess;
    const size_t lds = std::max<size_t>(lds_bytes, sizeof(double));
    if (lds > kRsLdsMaxBytes) // (resample_table keeps every window within it)
        return hipErrorInvalidValue;
    if (i16)
        hipLaunchKernelGGL(k_resample<int16_t>, dim3(n_tiles), dim3(kRsThreads), lds, stream, tables_dev, tiles_dev);
    else
        hipLaunchKernelGGL(k_resample<double>, dim3(n_tiles), dim3(kRsThreads), lds, stream, tables_dev, tiles_dev);
    return hipGetLastError();
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_resample_filter(uint32_t in_hz, uint32_t out_hz, uint32_t *L, uint32_t *M, uint32_t *ntaps, double *taps,
                       size_t cap)
{
    ResampleSpec s{};
    std::vector<double> h;
    int rc = resample_design(in_hz, out_hz, &s, taps ? &h : nullptr);
    if (rc)
        return rc;
    if (L)
        *L = s.L;
    if (M)
        *M = s.M;
    if (ntaps)
        *ntaps = s.ntaps;
    if (taps) {
        if (cap < h.size()) {
            set_error("resample filter: the table has " + std::to_string(h.size()) + " taps");
            return JB_ERR_BUFFER;
        }
        std::copy(h.begin(), h.end(), taps);
    }
    return JB_OK;
}

int jb_resample_geometry(uint32_t in_hz, uint32_t out_hz, jb_resample_geometry_t *out)
{
    if (!out) {
        set_error("jb_resample_geometry: out is NULL");
        return JB_ERR_INVALID;
    }
    if (in_hz == 0 || out_hz == 0) {
        set_error("resample: a rate of 0 Hz");
        return JB_ERR_INVALID;
    }
    ResampleGeom g{};
    int rc = resample_geometry(in_hz, out_hz, &g, nullptr);
    if (rc)
        return rc;
    *out = jb_resample_geometry_t{g.L, g.M, g.ntaps, g.pad, g.cap, g.fit, g.lds, g.rows, g.row_waves, g.lds_bytes,
                                  g.identity, 0};
    return JB_OK;
}

int jb_resample_pcm_batch(const double *const *in, const size_t *n_in, size_t n, uint32_t in_hz, uint32_t out_hz,
                          int32_t device, double **out, size_t *n_out)
{
    int rc = pcm_check((const void *const *)in, n_in, n, out && n_out, (void **)out, n_out);
    if (rc)
        return rc;
    if (in_hz == 0 || out_hz == 0) {
        set_error("resample: a rate of 0 Hz");
        return JB_ERR_INVALID;
    }
    // everything below (stream, allocations, launch) on the device where the table lives; the caller keeps its own
    DeviceScratch ds;
    ResampleTable t{};
    if ((rc = ds.open(device, "jb_resample_pcm_batch")) || (rc = resample_table(ds.device, in_hz, out_hz, &t)))
        return rc;
    std::vector<uint64_t> ioff;
    const double *dx = ds.pack(in, n_in, n, &ioff);
    std::vector<PcmShare> shares(n);
    uint64_t total = 0;
    for (size_t u = 0; u < n; u++) {
        shares[u] = {total, resample_out_len(n_in[u], t.L, t.M)};
        total += shares[u].n;
    }
    double *dy = ds.alloc<double>(total);
    std::vector<ResampleTile> tiles;
    for (size_t u = 0; u < n; u++)
        resample_tiles(t, 0, dx + ioff[u], n_in[u], dy + shares[u].off, shares[u].n, tiles);
    const std::vector<ResampleTable> tables(1, t);
    const ResampleTable *dt = ds.upload(tables);
    const ResampleTile *dtl = ds.upload(tiles);
    if (ds.ok())
        ds.err = launch_resample(dt, dtl, (uint32_t)tiles.size(), false, t.lds_bytes, ds.stream);
    std::vector<double> host;
    ds.read_back(&host, dy, total);
    if ((rc = ds.status()))
        return rc;
    return hand_out(host.data(), sizeof(double), shares, (void **)out, n_out);
}

} // extern "C"

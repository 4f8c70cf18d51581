// jb_fbank.cpp -- the host half of the filterbank features and of their frame conditioning (the request's window, check
// and Kaldi defaults): the option check, the geometry, the three tables (window, twiddles, mel weights; long double,
// rounded once) and the rule of jb_fbank.h over PCM the caller holds without a GPU, what the kernel is checked against:
// one body, fbank_framed_host, under jb_fbank_framed_host and -- with the all-zero request (jb_fbank.h "Frame
// conditioning") -- under jb_fbank_host; the two geometry entries share geometry_out the same way.
#include "jb_host.h"
#include "jb_mfcc.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(FbankOpts) == sizeof(jb_fbank_opts) && offsetof(FbankOpts, n_mels) == offsetof(jb_fbank_opts, n_mels) &&
                  offsetof(FbankOpts, f_max_hz) == offsetof(jb_fbank_opts, f_max_hz) &&
                  offsetof(FbankOpts, log_floor) == offsetof(jb_fbank_opts, log_floor) &&
                  offsetof(FbankOpts, flags) == offsetof(jb_fbank_opts, flags) &&
                  offsetof(FbankOpts, reserved) == offsetof(jb_fbank_opts, reserved),
              "jb_fbank.h restates the header's options");
static_assert(kFbHann == JB_FBANK_HANN && kFbHamming == JB_FBANK_HAMMING && kFbCenter == JB_FBANK_CENTER &&
                  kFbLinear == JB_FBANK_LINEAR && kFbUnit == JB_FBANK_UNIT && kFbF64 == JB_FBANK_F64,
              "jb_fbank.h restates the header's constants");
static_assert(sizeof(FrameOpts) == sizeof(jb_frame_opts) && offsetof(FrameOpts, window) == offsetof(jb_frame_opts, window) &&
                  offsetof(FrameOpts, flags) == offsetof(jb_frame_opts, flags) &&
                  offsetof(FrameOpts, reserved) == offsetof(jb_frame_opts, reserved),
              "jb_fbank.h restates the header's frame request");
static_assert(kFrWindowOpts == JB_FRAME_WINDOW_OPTS && kFrPovey == JB_FRAME_POVEY && kFrHannSym == JB_FRAME_HANN_SYM &&
                  kFrRect == JB_FRAME_RECT && kFrBlackman == JB_FRAME_BLACKMAN && kFrRemoveDc == JB_FRAME_REMOVE_DC &&
                  kFrReflect == JB_FRAME_REFLECT && kFrEnergy == JB_FRAME_ENERGY,
              "jb_fbank.h restates the header's frame constants");

namespace {

inline long double mel_of(long double f) { return 1127.0L * logl(1.0L + f / 700.0L); }

// One frame by the rule: z[0..wl) windowed already -> E[0..n_mels)
struct HostFrame {
    const FbankGeom &g;
    const FbankTables &t;
    std::vector<double> re, im;
    HostFrame(const FbankGeom &geom, const FbankTables &tab)
        : g(geom), t(tab), re(geom.n_fft / 2 + 1, 0.0), im(geom.n_fft / 2 + 1, 0.0)
    {
    }
    void run(const double *z, double *E)
    {
        rfft_frame_power(t.fft, [&](uint32_t i) { return i < g.wl ? z[i] : 0.0; }, re.data(), im.data());
        for (uint32_t m = 0; m < g.n_mels; m++)
            E[m] = mel_bank_energy(t.bank, m, re.data());
    }
};

// jb_fbank_geometry's body under the frame request fr (none: FrameOpts{}), the refusals under `who`
int geometry_out(uint32_t hz, const FbankOpts *o, const FrameOpts &fr, size_t n, uint32_t *wl, uint32_t *hop,
                 uint32_t *n_fft, size_t *T, size_t *n_bytes, const char *who)
{
    FbankGeom g{};
    const int rc = fbank_geometry(o, hz, who, &g);
    if (rc)
        return rc;
    const uint64_t frames = frame_count(n, g, *o, fr);
    if (wl)
        *wl = g.wl;
    if (hop)
        *hop = g.hop;
    if (n_fft)
        *n_fft = g.n_fft;
    if (T)
        *T = (size_t)frames;
    if (n_bytes)
        *n_bytes = (size_t)(frames * g.n_mels * fbank_elem(o->flags));
    return JB_OK;
}

} // namespace

int fbank_check_opts(const FbankOpts *opts, const char *who)
{
    if (!opts) {
        set_error(std::string(who) + ": opts is NULL");
        return JB_ERR_INVALID;
    }
    if (const char *f = fbank_opts_fault(*opts)) {
        set_error(std::string(who) + ": " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

int fbank_geometry(const FbankOpts *opts, uint32_t hz, const char *who, FbankGeom *g)
{
    const int rc = fbank_check_opts(opts, who);
    if (rc)
        return rc;
    if (const char *f = fbank_geometry_fault(*opts, hz, g)) {
        set_error(std::string(who) + ": at " + std::to_string(hz) + " Hz " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

void fbank_window(uint32_t window, uint32_t wl, double *w)
{
    const long double two_pi = 2.0L * acosl(-1.0L);
    for (uint32_t j = 0; j < wl; j++)
        w[j] = window == kFbHamming ? (double)(0.54L - 0.46L * cosl(two_pi * j / (long double)(wl - 1)))
                                    : (double)(0.5L - 0.5L * cosl(two_pi * j / (long double)wl));
}

void frame_window(uint32_t fbank_win, uint32_t frame_win, uint32_t wl, double *w)
{
    if (frame_win == kFrWindowOpts) {
        fbank_window(fbank_win, wl, w);
        return;
    }
    const long double a = 2.0L * acosl(-1.0L) / (long double)(wl - 1);
    for (uint32_t j = 0; j < wl; j++) {
        const long double h = 0.5L - 0.5L * cosl(a * j);
        w[j] = frame_win == kFrPovey      ? (double)powl(h, 0.85L)
               : frame_win == kFrHannSym  ? (double)h
               : frame_win == kFrBlackman ? (double)(0.42L - 0.5L * cosl(a * j) + 0.08L * cosl(2.0L * a * j))
                                          : 1.0;
    }
}

int frame_check(const FbankOpts *opts, const FrameOpts *fr, bool cepstra, const char *who)
{
    const int rc = fbank_check_opts(opts, who);
    if (rc)
        return rc;
    if (!fr) {
        set_error(std::string(who) + ": the frame request is NULL");
        return JB_ERR_INVALID;
    }
    const char *f = frame_opts_fault(*fr);
    if (!f)
        f = frame_pair_fault(*opts, *fr, cepstra);
    if (f) {
        set_error(std::string(who) + ": jb_frame_opts: " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

int fbank_framed_host(const double *in, size_t n, uint32_t hz, const FbankOpts *opts, const FrameOpts &fr, uint8_t *out,
                      size_t cap, const char *who, std::vector<double> *energy)
{
    FbankGeom g{};
    const int rc = fbank_geometry(opts, hz, who, &g);
    if (rc)
        return rc;
    const FbankOpts &o = *opts;
    const bool center = (o.flags & kFbCenter) != 0, reflect = (fr.flags & kFrReflect) != 0;
    const uint64_t T = frame_count(n, g, o, fr);
    if (cap < T * g.n_mels * fbank_elem(o.flags)) {
        set_error(std::string(who) + ": the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (n && (!in || (T && !out)))
        return JB_ERR_INVALID;
    FbankTables tab;
    fbank_tables(g, hz, o.window, &tab);
    frame_window(o.window, fr.window, g.wl, tab.win.data());
    HostFrame hf(g, tab);
    std::vector<double> E(g.n_mels), v(g.wl);
    const double scale = (o.flags & kFbUnit) ? 0x1p-15 : 1.0;
    if (energy)
        energy->assign(T, 0.0);
    for (uint64_t t = 0; t < T; t++) {
        const int64_t k0 = frame_start(t, g.wl, g.hop, center, reflect);
        for (uint32_t i = 0; i < g.wl; i++) {
            const int64_t k = k0 + (int64_t)i;
            v[i] = reflect ? in[frame_reflect(k, n)] * scale : k >= 0 && (uint64_t)k < n ? in[k] * scale : 0.0;
        }
        frame_condition(fr, tab.win.data(), g.wl, v.data(), energy ? &(*energy)[t] : nullptr);
        hf.run(v.data(), E.data());
        for (uint32_t m = 0; m < g.n_mels; m++) {
            const double y = (o.flags & kFbLinear) ? E[m] : E[m] > g.log_floor ? log(E[m]) : g.ln_floor;
            put_elem(out, (size_t)t * g.n_mels + m, y, (o.flags & kFbF64) != 0);
        }
    }
    return JB_OK;
}

void fbank_filterbank(const FbankGeom &g, uint32_t hz, double *W)
{
    const uint32_t K = g.n_fft / 2 + 1;
    const long double lo = mel_of(g.f_min), hi = mel_of(g.f_max);
    std::vector<long double> mu(K);
    for (uint32_t k = 0; k < K; k++)
        mu[k] = mel_of((long double)k * hz / g.n_fft);
    for (uint32_t m = 0; m < g.n_mels; m++) {
        const long double l = lo + (hi - lo) * m / (g.n_mels + 1), c = lo + (hi - lo) * (m + 1) / (g.n_mels + 1),
                          r = lo + (hi - lo) * (m + 2) / (g.n_mels + 1);
        for (uint32_t k = 0; k < K; k++) {
            const long double up = (mu[k] - l) / (c - l), down = (r - mu[k]) / (r - c);
            const long double v = up < down ? up : down;
            W[(size_t)m * K + k] = v > 0.0L ? (double)v : 0.0;
        }
    }
}

bool fbank_tables(const FbankGeom &g, uint32_t hz, uint32_t window, FbankTables *t)
{
    const uint32_t K = g.n_fft / 2 + 1;
    t->win.resize(g.wl);
    fbank_window(window, g.wl, t->win.data());
    t->fft = rfft_plan(g.n_fft);
    std::vector<double> W((size_t)g.n_mels * K);
    fbank_filterbank(g, hz, W.data());
    // (the centres as fbank_filterbank has them: a bin is on a filter's rising side where mu_k is at or below it)
    const long double lo = mel_of(g.f_min), hi = mel_of(g.f_max);
    return mel_bank_split(
        W.data(), g.n_mels, K,
        [&](uint32_t m, uint32_t k) {
            return mel_of((long double)k * hz / g.n_fft) <= lo + (hi - lo) * (m + 1) / (g.n_mels + 1);
        },
        &t->bank);
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_fbank_geometry(uint32_t hz, const jb_fbank_opts *opts, size_t n, uint32_t *wl, uint32_t *hop, uint32_t *n_fft,
                      size_t *T, size_t *n_bytes)
{
    return geometry_out(hz, (const FbankOpts *)opts, FrameOpts{}, n, wl, hop, n_fft, T, n_bytes, "jb_fbank_geometry");
}

int jb_fbank_window(uint32_t hz, const jb_fbank_opts *opts, double *w, size_t cap)
{
    FbankGeom g{};
    const int rc = fbank_geometry((const FbankOpts *)opts, hz, "jb_fbank_window", &g);
    if (rc)
        return rc;
    if (cap < g.wl) {
        set_error("jb_fbank_window: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (!w)
        return JB_ERR_INVALID;
    fbank_window(opts->window, g.wl, w);
    return JB_OK;
}

int jb_fbank_filterbank(uint32_t hz, const jb_fbank_opts *opts, double *W, size_t cap)
{
    FbankGeom g{};
    const int rc = fbank_geometry((const FbankOpts *)opts, hz, "jb_fbank_filterbank", &g);
    if (rc)
        return rc;
    if (cap < (size_t)g.n_mels * (g.n_fft / 2 + 1)) {
        set_error("jb_fbank_filterbank: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (!W)
        return JB_ERR_INVALID;
    fbank_filterbank(g, hz, W);
    return JB_OK;
}

int jb_fbank_host(const double *in, size_t n, uint32_t hz, const jb_fbank_opts *opts, uint8_t *out, size_t cap)
{
    return fbank_framed_host(in, n, hz, (const FbankOpts *)opts, FrameOpts{}, out, cap, "jb_fbank_host", nullptr);
}

int jb_frame_kaldi(uint32_t n_mels, jb_fbank_opts *f, jb_frame_opts *fr)
{
    if (!f || !fr) {
        set_error("jb_frame_kaldi: an out pointer is NULL");
        return JB_ERR_INVALID;
    }
    if (n_mels < 1 || n_mels > kFbMaxMels) {
        set_error("jb_frame_kaldi: n_mels is in 1..128");
        return JB_ERR_INVALID;
    }
    memset(f, 0, sizeof *f);
    memset(fr, 0, sizeof *fr);
    f->win_us = 25000;
    f->hop_us = 10000;
    f->n_mels = n_mels;
    f->f_min_hz = 20.0;
    f->log_floor = 0x1p-23;
    fr->preemph = 0.97;
    fr->window = JB_FRAME_POVEY;
    fr->flags = JB_FRAME_REMOVE_DC;
    return JB_OK;
}

int jb_frame_check(const jb_fbank_opts *fopts, const jb_mfcc_opts *mopts, const jb_frame_opts *fr)
{
    const FbankOpts *f = (const FbankOpts *)fopts;
    const MfccOpts *m = (const MfccOpts *)mopts;
    int rc = fbank_check_opts(f, "jb_frame_check");
    if (!rc && m && !(rc = mfcc_check_fbank(f, "jb_frame_check")))
        rc = mfcc_check_opts(m, f->n_mels, "jb_frame_check");
    return rc ? rc : frame_check(f, (const FrameOpts *)fr, m && m->n_ceps >= 1, "jb_frame_check");
}

int jb_fbank_framed_geometry(uint32_t hz, const jb_fbank_opts *opts, const jb_frame_opts *fr, size_t n, uint32_t *wl,
                             uint32_t *hop, uint32_t *n_fft, size_t *T, size_t *n_bytes)
{
    const int rc = frame_check((const FbankOpts *)opts, (const FrameOpts *)fr, true, "jb_fbank_framed_geometry");
    // (what the rate refuses keeps jb_fbank_geometry's name, as it always had)
    return rc ? rc
              : geometry_out(hz, (const FbankOpts *)opts, *(const FrameOpts *)fr, n, wl, hop, n_fft, T, n_bytes,
                             "jb_fbank_geometry");
}

int jb_frame_window(uint32_t hz, const jb_fbank_opts *opts, const jb_frame_opts *fr, double *w, size_t cap)
{
    int rc = frame_check((const FbankOpts *)opts, (const FrameOpts *)fr, true, "jb_frame_window");
    if (rc || (rc = jb_fbank_window(hz, opts, w, cap)))
        return rc;
    FbankGeom g{};
    fbank_geometry_fault(*(const FbankOpts *)opts, hz, &g);
    frame_window(opts->window, fr->window, g.wl, w);
    return JB_OK;
}

int jb_fbank_framed_host(const double *in, size_t n, uint32_t hz, const jb_fbank_opts *opts, const jb_frame_opts *fr,
                         uint8_t *out, size_t cap)
{
    const int rc = frame_check((const FbankOpts *)opts, (const FrameOpts *)fr, false, "jb_fbank_framed_host");
    if (rc)
        return rc;
    return fbank_framed_host(in, n, hz, (const FbankOpts *)opts, *(const FrameOpts *)fr, out, cap,
                             "jb_fbank_framed_host", nullptr);
}

void jb_fbank_free(uint8_t *p) { free(p); }

} // extern "C"

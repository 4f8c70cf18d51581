// jb_melspec.cpp -- the host half of the mel spectrograms: the option check, the geometry, the tables (window, twiddles,
// digit reversal, mel weights; long double, rounded once), Whisper's preset and the rule of jb_melspec.h over PCM the
// caller holds without a GPU (jb_melspec_host, what the kernel is checked against).
#include "jb_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(MelOpts) == sizeof(jb_melspec_opts) && offsetof(MelOpts, n_mels) == offsetof(jb_melspec_opts, n_mels) &&
                  offsetof(MelOpts, f_max_hz) == offsetof(jb_melspec_opts, f_max_hz) &&
                  offsetof(MelOpts, floor) == offsetof(jb_melspec_opts, floor) &&
                  offsetof(MelOpts, range) == offsetof(jb_melspec_opts, range) &&
                  offsetof(MelOpts, scale) == offsetof(jb_melspec_opts, scale) &&
                  offsetof(MelOpts, mel_scale) == offsetof(jb_melspec_opts, mel_scale) &&
                  offsetof(MelOpts, log) == offsetof(jb_melspec_opts, log) &&
                  offsetof(MelOpts, flags) == offsetof(jb_melspec_opts, flags) &&
                  offsetof(MelOpts, reserved) == offsetof(jb_melspec_opts, reserved),
              "jb_melspec.h restates the header's options");
static_assert(kMelHtk == JB_MEL_HTK && kMelSlaney == JB_MEL_SLANEY && kMelNormNone == JB_MEL_NORM_NONE &&
                  kMelNormSlaney == JB_MEL_NORM_SLANEY && kMelPadReflect == JB_MEL_PAD_REFLECT &&
                  kMelPadZero == JB_MEL_PAD_ZERO && kMelPadNone == JB_MEL_PAD_NONE && kMelLogNone == JB_MEL_LOG_NONE &&
                  kMelLogLn == JB_MEL_LOG_LN && kMelLog10 == JB_MEL_LOG_LOG10 && kMelLogDb == JB_MEL_LOG_DB &&
                  kMelMagnitude == JB_MEL_MAGNITUDE && kMelDropLast == JB_MEL_DROP_LAST && kMelF64 == JB_MEL_F64,
              "jb_melspec.h restates the header's constants");

namespace {

const long double kSlaneyStep = logl(6.4L) / 27.0L;

inline long double mel_of(long double f, uint32_t scale)
{
    if (scale == kMelHtk)
        return 2595.0L * log10l(1.0L + f / 700.0L);
    return f < 1000.0L ? 3.0L * f / 200.0L : 15.0L + logl(f / 1000.0L) / kSlaneyStep;
}
inline long double hz_of(long double m, uint32_t scale)
{
    if (scale == kMelHtk)
        return 700.0L * (powl(10.0L, m / 2595.0L) - 1.0L);
    return m < 15.0L ? 200.0L * m / 3.0L : 1000.0L * expl((m - 15.0L) * kSlaneyStep);
}
// the n_mels + 2 edges in Hz
std::vector<long double> mel_edges(const MelGeom &g, uint32_t scale)
{
    const long double lo = mel_of(g.f_min, scale), hi = mel_of(g.f_max, scale);
    std::vector<long double> f(g.n_mels + 2);
    for (uint32_t i = 0; i < g.n_mels + 2; i++)
        f[i] = hz_of(lo + (hi - lo) * i / (g.n_mels + 1), scale);
    return f;
}

// One frame by the rule: sample i of the frame (0 outside the unit) -> y[0..n_mels) in front of the range clamp
struct HostFrame {
    const MelGeom &g;
    const MelTables &t;
    const MelOpts &o;
    uint32_t M;
    std::vector<double> re, im;
    HostFrame(const MelGeom &geom, const MelTables &tab, const MelOpts &opts)
        : g(geom), t(tab), o(opts), M(geom.n_fft / 2), re(geom.n_fft / 2 + 1, 0.0), im(geom.n_fft / 2 + 1, 0.0)
    {
    }
    template <class X> void run(X x, double *y)
    {
        rfft_frame_power(
            t.fft,
            [&](uint32_t i) { return i >= g.woff && i < g.woff + g.wl ? t.win[i - g.woff] * (x(i) * 0x1p-15) : 0.0; },
            re.data(), im.data());
        if (o.flags & kMelMagnitude)
            for (uint32_t k = 0; k <= M; k++)
                re[k] = sqrt(re[k]);
        for (uint32_t m = 0; m < g.n_mels; m++)
            y[m] = mel_log(mel_bank_energy(t.bank, m, re.data()), o.log, g.floor, g.y_floor);
    }
};

} // namespace

int mel_check_opts(const MelOpts *opts, const char *who)
{
    if (!opts) {
        set_error(std::string(who) + ": opts is NULL");
        return JB_ERR_INVALID;
    }
    if (const char *f = mel_opts_fault(*opts)) {
        set_error(std::string(who) + ": " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

int mel_geometry(const MelOpts *opts, uint32_t hz, const char *who, MelGeom *g)
{
    const int rc = mel_check_opts(opts, who);
    if (rc)
        return rc;
    if (const char *f = mel_geometry_fault(*opts, hz, g)) {
        set_error(std::string(who) + ": at " + std::to_string(hz) + " Hz " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

void mel_window(uint32_t wl, double *w)
{
    const long double two_pi = 2.0L * acosl(-1.0L);
    for (uint32_t j = 0; j < wl; j++)
        w[j] = (double)(0.5L - 0.5L * cosl(two_pi * j / (long double)wl));
}

void mel_filterbank(const MelGeom &g, uint32_t hz, uint32_t mel_scale, uint32_t norm, double *W)
{
    const uint32_t K = g.n_fft / 2 + 1;
    const std::vector<long double> f = mel_edges(g, mel_scale);
    for (uint32_t m = 0; m < g.n_mels; m++) {
        const long double area = norm == kMelNormSlaney ? 2.0L / (f[m + 2] - f[m]) : 1.0L;
        for (uint32_t k = 0; k < K; k++) {
            const long double nu = (long double)k * hz / g.n_fft;
            const long double up = (nu - f[m]) / (f[m + 1] - f[m]), down = (f[m + 2] - nu) / (f[m + 2] - f[m + 1]);
            const long double v = up < down ? up : down;
            W[(size_t)m * K + k] = v > 0.0L ? (double)(v * area) : 0.0;
        }
    }
}

bool mel_tables(const MelGeom &g, uint32_t hz, const MelOpts &o, MelTables *t)
{
    const uint32_t K = g.n_fft / 2 + 1;
    t->win.resize(g.wl);
    mel_window(g.wl, t->win.data());
    t->fft = rfft_plan(g.n_fft);
    std::vector<double> W((size_t)g.n_mels * K);
    mel_filterbank(g, hz, o.mel_scale, o.norm, W.data());
    t->wmax = 0.0;
    for (double w : W)
        t->wmax = std::max(t->wmax, w);
    // (the centres as mel_filterbank has them: a bin is on a filter's rising side where nu_k is at or below it)
    const std::vector<long double> f = mel_edges(g, o.mel_scale);
    return mel_bank_split(
        W.data(), g.n_mels, K, [&](uint32_t m, uint32_t k) { return (long double)k * hz / g.n_fft <= f[m + 1]; },
        &t->bank);
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_melspec_whisper(uint32_t n_mels, jb_melspec_opts *opts)
{
    if (!opts) {
        set_error("jb_melspec_whisper: opts is NULL");
        return JB_ERR_INVALID;
    }
    jb_melspec_opts o{};
    o.n_fft = 400;
    o.win_length = 400;
    o.hop_length = 160;
    o.n_mels = n_mels;
    o.f_min_hz = 0.0;
    o.f_max_hz = 8000.0;
    o.floor = 1e-10;
    o.range = 8.0;
    o.offset = 4.0;
    o.scale = 0.25;
    o.mel_scale = JB_MEL_SLANEY;
    o.norm = JB_MEL_NORM_SLANEY;
    o.pad = JB_MEL_PAD_REFLECT;
    o.log = JB_MEL_LOG_LOG10;
    o.flags = JB_MEL_DROP_LAST;
    const int rc = mel_check_opts((const MelOpts *)&o, "jb_melspec_whisper");
    if (rc)
        return rc;
    *opts = o;
    return JB_OK;
}

int jb_melspec_geometry(uint32_t hz, const jb_melspec_opts *opts, size_t n, uint32_t *n_fft, uint32_t *win_length,
                        uint32_t *hop_length, size_t *T, size_t *n_bytes)
{
    MelGeom g{};
    const int rc = mel_geometry((const MelOpts *)opts, hz, "jb_melspec_geometry", &g);
    if (rc)
        return rc;
    const uint64_t frames = mel_frames(n, g.n_fft, g.hop, opts->pad, opts->flags);
    if (n_fft)
        *n_fft = g.n_fft;
    if (win_length)
        *win_length = g.wl;
    if (hop_length)
        *hop_length = g.hop;
    if (T)
        *T = (size_t)frames;
    if (n_bytes)
        *n_bytes = (size_t)(frames * g.n_mels * mel_elem(opts->flags));
    return JB_OK;
}

int jb_melspec_window(uint32_t hz, const jb_melspec_opts *opts, double *w, size_t cap)
{
    MelGeom g{};
    const int rc = mel_geometry((const MelOpts *)opts, hz, "jb_melspec_window", &g);
    if (rc)
        return rc;
    if (cap < g.n_fft) {
        set_error("jb_melspec_window: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (!w)
        return JB_ERR_INVALID;
    for (uint32_t i = 0; i < g.n_fft; i++)
        w[i] = 0.0;
    mel_window(g.wl, w + g.woff);
    return JB_OK;
}

int jb_melspec_filterbank(uint32_t hz, const jb_melspec_opts *opts, double *W, size_t cap)
{
    MelGeom g{};
    const int rc = mel_geometry((const MelOpts *)opts, hz, "jb_melspec_filterbank", &g);
    if (rc)
        return rc;
    if (cap < (size_t)g.n_mels * (g.n_fft / 2 + 1)) {
        set_error("jb_melspec_filterbank: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (!W)
        return JB_ERR_INVALID;
    mel_filterbank(g, hz, opts->mel_scale, opts->norm, W);
    return JB_OK;
}

int jb_melspec_host(const double *in, size_t n, uint32_t hz, const jb_melspec_opts *opts, uint8_t *out, size_t cap)
{
    const MelOpts *o = (const MelOpts *)opts;
    MelGeom g{};
    const int rc = mel_geometry(o, hz, "jb_melspec_host", &g);
    if (rc)
        return rc;
    const uint64_t T = mel_frames(n, g.n_fft, g.hop, o->pad, o->flags);
    if (cap < T * g.n_mels * mel_elem(o->flags)) {
        set_error("jb_melspec_host: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (n && (!in || (T && !out)))
        return JB_ERR_INVALID;
    MelTables tab;
    mel_tables(g, hz, *o, &tab);
    HostFrame fr(g, tab, *o);
    std::vector<double> y((size_t)T * g.n_mels);
    double ymax = -HUGE_VAL;
    for (uint64_t t = 0; t < T; t++) {
        const int64_t k0 = (int64_t)(t * g.hop) - (o->pad == kMelPadNone ? 0 : (int64_t)(g.n_fft / 2));
        double *row = y.data() + (size_t)t * g.n_mels;
        fr.run(
            [&](uint32_t i) {
                const int64_t k = mel_sample_at(k0 + (int64_t)i, n, o->pad);
                return k >= 0 ? in[k] : 0.0;
            },
            row);
        for (uint32_t m = 0; m < g.n_mels; m++)
            ymax = row[m] > ymax ? row[m] : ymax;
    }
    for (size_t i = 0; i < y.size(); i++) {
        double v = y[i];
        if (o->range > 0.0)
            v = v > ymax - o->range ? v : ymax - o->range;
        put_elem(out, i, mel_affine(v, o->offset, g.scale), (o->flags & kMelF64) != 0);
    }
    return JB_OK;
}

void jb_melspec_free(uint8_t *p) { free(p); }

} // extern "C"

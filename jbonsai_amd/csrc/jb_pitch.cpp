// jb_pitch.cpp -- the host half of the pitch stage: the request check, the geometry, the lag grid and the rule of
// jb_pitch.h over PCM the caller holds without a GPU (jb_pitch_host, what the kernels are checked against).  A frame's
// sums here are jb_fbank.h's frame_sum itself.
#include "jb_host.h"

#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(PitchOpts) == sizeof(jb_pitch_opts) && offsetof(PitchOpts, win_us) == offsetof(jb_pitch_opts, win_us) &&
                  offsetof(PitchOpts, hop_us) == offsetof(jb_pitch_opts, hop_us) &&
                  offsetof(PitchOpts, min_f0) == offsetof(jb_pitch_opts, min_f0) &&
                  offsetof(PitchOpts, max_f0) == offsetof(jb_pitch_opts, max_f0) &&
                  offsetof(PitchOpts, delta_pitch) == offsetof(jb_pitch_opts, delta_pitch) &&
                  offsetof(PitchOpts, penalty_factor) == offsetof(jb_pitch_opts, penalty_factor) &&
                  offsetof(PitchOpts, soft_min_f0) == offsetof(jb_pitch_opts, soft_min_f0) &&
                  offsetof(PitchOpts, nccf_ballast) == offsetof(jb_pitch_opts, nccf_ballast) &&
                  offsetof(PitchOpts, pov_scale) == offsetof(jb_pitch_opts, pov_scale) &&
                  offsetof(PitchOpts, pitch_scale) == offsetof(jb_pitch_opts, pitch_scale) &&
                  offsetof(PitchOpts, delta_scale) == offsetof(jb_pitch_opts, delta_scale) &&
                  offsetof(PitchOpts, norm_left) == offsetof(jb_pitch_opts, norm_left) &&
                  offsetof(PitchOpts, norm_right) == offsetof(jb_pitch_opts, norm_right) &&
                  offsetof(PitchOpts, grid) == offsetof(jb_pitch_opts, grid) &&
                  offsetof(PitchOpts, flags) == offsetof(jb_pitch_opts, flags) &&
                  offsetof(PitchOpts, reserved) == offsetof(jb_pitch_opts, reserved),
              "jb_pitch.h restates the header's options");
static_assert(kPitchSnip == JB_PITCH_SNIP && kPitchKaldi == JB_PITCH_KALDI && kPitchF64 == JB_PITCH_F64 &&
                  kPitchRaw == JB_PITCH_RAW && kPitchRawLog == JB_PITCH_RAW_LOG && kPitchMaxDown == JB_PITCH_MAX_DOWN &&
                  kPitchMaxScratch == JB_PITCH_MAX_SCRATCH && kPitchRate == JB_PITCH_RATE,
              "jb_pitch.h restates the header's constants");
static_assert(sizeof(jb_pitch_geometry_t) == 56, "the layout the bindings restate");

int pitch_check_opts(const PitchOpts *opts, const char *who, PitchGrid *grid)
{
    if (!opts) {
        set_error(std::string(who) + ": opts is NULL");
        return JB_ERR_INVALID;
    }
    const char *f = pitch_opts_fault(*opts);
    PitchGrid g;
    if (!f)
        f = pitch_grid_fault(*opts, &g);
    if (f) {
        set_error(std::string(who) + ": " + f);
        return JB_ERR_INVALID;
    }
    if (grid)
        *grid = std::move(g);
    return JB_OK;
}

int pitch_check_rate(uint32_t hz, size_t unit, const char *who, PitchDown *down)
{
    PitchDown d;
    bool unsupported = false;
    if (const char *f = pitch_down_fault(hz, &d, &unsupported)) {
        set_error(std::string(who) + ": " + f + " (unit " + std::to_string(unit) + ", " + std::to_string(hz) + " Hz)");
        return unsupported ? JB_ERR_UNSUPPORTED : JB_ERR_INVALID;
    }
    if (down)
        *down = std::move(d);
    return JB_OK;
}

jb_pitch_geometry_t pitch_geometry_of(const PitchOpts &o, const PitchGrid &g, uint32_t hz, uint64_t n)
{
    jb_pitch_geometry_t out{};
    out.wl = (uint32_t)fbank_round_us(hz, o.win_us);
    out.hop = (uint32_t)fbank_round_us(hz, o.hop_us);
    out.T = pitch_frames(o.grid, n, out.wl, out.hop);
    out.n4 = pitch_n4(n, hz);
    out.width = pitch_width(o.flags);
    out.elem = pitch_elem(o.flags);
    out.S = g.S;
    out.lag_first = g.a;
    out.lag_last = g.b;
    out.wl4 = g.wl4;
    out.sh4 = g.sh4;
    out.choice_bytes = (uint32_t)pitch_choice_bytes(g.S);
    return out;
}

namespace {

template <class T> void put_row(const double *v, uint32_t width, uint8_t *row)
{
    for (uint32_t c = 0; c < width; c++)
        ((T *)row)[c] = (T)v[c];
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_pitch_kaldi(jb_pitch_opts *opts)
{
    if (!opts)
        return JB_ERR_INVALID;
    memset(opts, 0, sizeof(*opts));
    opts->win_us = 25000;
    opts->hop_us = 10000;
    opts->min_f0 = 50.0;
    opts->max_f0 = 400.0;
    opts->delta_pitch = 0.005;
    opts->penalty_factor = 0.1;
    opts->soft_min_f0 = 10.0;
    opts->nccf_ballast = 7000.0;
    opts->pov_scale = 2.0;
    opts->pitch_scale = 2.0;
    opts->delta_scale = 10.0;
    opts->norm_left = 75;
    opts->norm_right = 75;
    opts->grid = JB_PITCH_KALDI;
    return JB_OK;
}

int jb_pitch_geometry(const jb_pitch_opts *opts, uint32_t hz, size_t n, jb_pitch_geometry_t *out)
{
    const char *who = "jb_pitch_geometry";
    PitchGrid g;
    int rc = pitch_check_opts((const PitchOpts *)opts, who, &g);
    if (rc || (rc = pitch_check_rate(hz, 0, who, nullptr)))
        return rc;
    if (out)
        *out = pitch_geometry_of(*(const PitchOpts *)opts, g, hz, n);
    return JB_OK;
}

int jb_pitch_lags(const jb_pitch_opts *opts, double *lags, size_t cap, size_t *S)
{
    PitchGrid g;
    const int rc = pitch_check_opts((const PitchOpts *)opts, "jb_pitch_lags", &g);
    if (rc)
        return rc;
    if (S)
        *S = g.S;
    if (lags) {
        if (cap < g.S) {
            set_error("jb_pitch_lags: the buffer is too small");
            return JB_ERR_BUFFER;
        }
        memcpy(lags, g.lag.data(), sizeof(double) * g.S);
    }
    return JB_OK;
}

int jb_pitch_host(const double *x, size_t n, uint32_t hz, const jb_pitch_opts *opts, void *out, size_t cap,
                  uint32_t *lag_index, double *grid_q, double *grid_p)
{
    const char *who = "jb_pitch_host";
    const PitchOpts *o = (const PitchOpts *)opts;
    PitchGrid g;
    PitchDown dn;
    int rc = pitch_check_opts(o, who, &g);
    if (rc || (rc = pitch_check_rate(hz, 0, who, &dn)))
        return rc;
    if (n && !x)
        return JB_ERR_INVALID;
    const jb_pitch_geometry_t geo = pitch_geometry_of(*o, g, hz, n);
    const uint64_t T = geo.T, n4 = geo.n4;
    const size_t row = (size_t)geo.width * geo.elem;
    if (cap < T * row || (T && !out)) {
        set_error(std::string(who) + ": the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (T == 0)
        return JB_OK;
    // step 1: the 4 kHz signal and its sums
    std::vector<double> y(n4);
    for (uint64_t m = 0; m < n4; m++)
        y[m] = pitch_down_sample(m, n, dn.hzp, dn.P, dn.D, dn.W.data(), [&](uint64_t k) { return x[k]; });
    double S1 = 0.0, S2 = 0.0;
    for (uint64_t i = 0; i < pitch_tiles(n4); i++) {
        double p1[kPitchLanes], p2[kPitchLanes];
        for (uint32_t l = 0; l < kPitchLanes; l++)
            pitch_partial(n4, i, l, [&](uint64_t m) { return y[m]; }, &p1[l], &p2[l]);
        for (uint32_t h = kPitchLanes / 2; h; h >>= 1)
            for (uint32_t l = 0; l < h; l++) {
                p1[l] = p1[l] + p1[l + h];
                p2[l] = p2[l] + p2[l + h];
            }
        S1 = i ? S1 + p1[0] : p1[0];
        S2 = i ? S2 + p2[0] : p2[0];
    }
    const double B = pitch_ballast(S1, S2, n4, g.wl4, o->nccf_ballast);
    // steps 2 to 5, frame by frame
    const uint32_t S = g.S, nl = g.b - g.a + 1, wl4 = g.wl4;
    std::vector<double> v(wl4 + g.b), q(nl), p(nl), Q(S), Pg(S), F(S, 0.0), Fn(S);
    std::vector<uint16_t> choice((size_t)T * S);
    std::vector<double> pgrid(grid_p ? 0 : (size_t)T * S); // p over the grid, for the chosen lag's value
    double *PG = grid_p ? grid_p : pgrid.data();
    for (uint64_t t = 0; t < T; t++) {
        const int64_t s0 = pitch_start(o->grid, t, wl4, g.sh4);
        for (uint32_t i = 0; i < wl4 + g.b; i++) {
            const int64_t k = s0 + (int64_t)i;
            v[i] = k >= 0 && (uint64_t)k < n4 ? y[k] : 0.0;
        }
        const double mean = frame_sum(wl4, [&](uint32_t i) { return v[i]; }) / (double)wl4;
        for (uint32_t i = 0; i < wl4 + g.b; i++)
            v[i] = v[i] - mean;
        const double e0 = frame_sum(wl4, [&](uint32_t i) { return v[i] * v[i]; });
        for (uint32_t L = g.a; L <= g.b; L++) {
            const double inner = frame_sum(wl4, [&](uint32_t i) { return v[i] * v[i + L]; });
            const double eL = frame_sum(wl4, [&](uint32_t i) { return v[i + L] * v[i + L]; });
            q[L - g.a] = pitch_nccf(inner, e0, eL, B);
            p[L - g.a] = pitch_nccf(inner, e0, eL, 0.0);
        }
        for (uint32_t i = 0; i < S; i++) {
            const uint32_t k0 = g.tap[i] & 0xffffu, cnt = g.tap[i] >> 16;
            double aq = 0.0, ap = 0.0;
            for (uint32_t k = 0; k < cnt; k++) {
                const double w = g.G[(size_t)i * kPitchTaps + k], tq = q[k0 + k] * w, tp = p[k0 + k] * w;
                aq = aq + tq;
                ap = ap + tp;
            }
            Q[i] = aq;
            PG[t * S + i] = ap;
            if (grid_q)
                grid_q[t * S + i] = aq;
        }
        double mn = 0.0;
        for (uint32_t i = 0; i < S; i++) {
            double best = pitch_cand(F[0], g.kappa, i, 0);
            uint32_t bj = 0;
            for (uint32_t j = 1; j < S; j++) {
                const double c = pitch_cand(F[j], g.kappa, i, j);
                if (c < best) {
                    best = c;
                    bj = j;
                }
            }
            Fn[i] = best + pitch_local(Q[i], g.soft[i]);
            choice[t * S + i] = (uint16_t)bj;
            mn = i == 0 || Fn[i] < mn ? Fn[i] : mn;
        }
        for (uint32_t i = 0; i < S; i++)
            F[i] = Fn[i] - mn;
    }
    std::vector<uint32_t> idx(T);
    uint32_t s = 0;
    for (uint32_t i = 1; i < S; i++)
        if (F[i] < F[s])
            s = i;
    for (uint64_t t = T; t-- > 0;) {
        idx[t] = s;
        s = choice[t * S + s];
    }
    // the raw pair, or step 6
    std::vector<double> pv(T), pw(T);
    for (uint64_t t = 0; t < T; t++) {
        pv[t] = PG[t * S + idx[t]];
        pw[t] = pitch_pov_weight(pv[t]);
    }
    for (uint64_t t = 0; t < T; t++) {
        double c[4];
        if (o->flags & kPitchRaw) {
            c[0] = pv[t];
            c[1] = g.inv_lag[idx[t]];
        } else {
            pitch_columns(t, T, idx.data(), pv.data(), pw.data(), g.log_pitch.data(), o->pov_scale, o->pitch_scale,
                          o->delta_scale, o->norm_left, o->norm_right, geo.width, c);
        }
        if (o->flags & kPitchF64)
            put_row<double>(c, geo.width, (uint8_t *)out + t * row);
        else
            put_row<float>(c, geo.width, (uint8_t *)out + t * row);
        if (lag_index)
            lag_index[t] = idx[t];
    }
    return JB_OK;
}

void jb_pitch_free(void *p) { free(p); }

} // extern "C"

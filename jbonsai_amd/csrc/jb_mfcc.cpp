// jb_mfcc.cpp -- the host half of the cepstral features: the option check, the tables (DCT, lifter, delta kernels; long
// double, rounded once) and the rule of jb_mfcc.h over frames or PCM the caller holds without a GPU (jb_mfcc_host,
// jb_mfcc_pcm_host: what the kernels are checked against).
#include "jb_host.h"
#include "jb_mfcc.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(MfccOpts) == sizeof(jb_mfcc_opts) && offsetof(MfccOpts, n_ceps) == offsetof(jb_mfcc_opts, n_ceps) &&
                  offsetof(MfccOpts, delta_order) == offsetof(jb_mfcc_opts, delta_order) &&
                  offsetof(MfccOpts, delta_window) == offsetof(jb_mfcc_opts, delta_window) &&
                  offsetof(MfccOpts, cmvn) == offsetof(jb_mfcc_opts, cmvn) &&
                  offsetof(MfccOpts, lifter) == offsetof(jb_mfcc_opts, lifter) &&
                  offsetof(MfccOpts, var_floor) == offsetof(jb_mfcc_opts, var_floor) &&
                  offsetof(MfccOpts, flags) == offsetof(jb_mfcc_opts, flags) &&
                  offsetof(MfccOpts, reserved) == offsetof(jb_mfcc_opts, reserved),
              "jb_mfcc.h restates the header's options");
static_assert(kMfCmvnNone == JB_CMVN_NONE && kMfCmvnMean == JB_CMVN_MEAN && kMfCmvnMeanVar == JB_CMVN_MEAN_VAR &&
                  kMfF64 == JB_MFCC_F64,
              "jb_mfcc.h restates the header's constants");

int mfcc_check_opts(const MfccOpts *opts, uint32_t n_mels, const char *who)
{
    if (!opts) {
        set_error(std::string(who) + ": the cepstral opts are NULL");
        return JB_ERR_INVALID;
    }
    if (n_mels < 1 || n_mels > kFbMaxMels) {
        set_error(std::string(who) + ": n_mels is in 1..128");
        return JB_ERR_INVALID;
    }
    if (const char *f = mfcc_opts_fault(*opts, n_mels)) {
        set_error(std::string(who) + ": " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

int mfcc_check_fbank(const FbankOpts *fopts, const char *who)
{
    const int rc = fbank_check_opts(fopts, who);
    if (rc)
        return rc;
    if (const char *f = mfcc_fbank_fault(*fopts)) {
        set_error(std::string(who) + ": " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

void mfcc_dct(uint32_t n_mels, uint32_t n_ceps, double lifter, double *D, double *lift)
{
    const long double pi = acosl(-1.0L), N = (long double)n_mels;
    const long double a0 = sqrtl(1.0L / N), a = sqrtl(2.0L / N);
    for (uint32_t i = 0; i < n_ceps; i++) {
        if (D)
            for (uint32_t m = 0; m < n_mels; m++) {
                // (the angle pi i (2 m + 1) / (2 N) with its integer part reduced first: i (2 m + 1) mod 4 N is exact)
                const uint64_t k = ((uint64_t)i * (2 * m + 1)) % (4ull * n_mels);
                D[(size_t)i * n_mels + m] = i == 0 ? (double)a0 : (double)(a * cosl(pi * (long double)k / (2.0L * N)));
            }
        if (lift)
            lift[i] = lifter > 0.0 ? (double)(1.0L + ((long double)lifter / 2.0L) *
                                                        sinl(pi * (long double)i / (long double)lifter))
                                   : 1.0;
    }
}

void mfcc_delta_kernel(uint32_t q, uint32_t N, double *s)
{
    long double den = 0.0L;
    for (int32_t j = -(int32_t)N; j <= (int32_t)N; j++)
        den += (long double)j * j;
    std::vector<long double> cur{1.0L};
    for (uint32_t r = 0; r < q; r++) { // cur * g, full
        std::vector<long double> next(cur.size() + 2 * N, 0.0L);
        for (size_t a = 0; a < cur.size(); a++)
            for (int32_t k = -(int32_t)N; k <= (int32_t)N; k++)
                next[a + (size_t)(k + (int32_t)N)] += cur[a] * ((long double)k / den);
        cur.swap(next);
    }
    for (size_t i = 0; i < cur.size(); i++)
        s[i] = (double)cur[i];
}

void mfcc_tables(const MfccOpts &o, uint32_t n_mels, MfccTables *t)
{
    t->D.assign((size_t)o.n_ceps * n_mels, 0.0);
    t->Dt.assign((size_t)o.n_ceps * n_mels, 0.0);
    t->lift.assign(o.n_ceps, 1.0);
    mfcc_dct(n_mels, o.n_ceps, o.lifter, t->D.data(), t->lift.data());
    for (uint32_t i = 0; i < o.n_ceps; i++)
        for (uint32_t m = 0; m < n_mels; m++)
            t->Dt[(size_t)m * o.n_ceps + i] = t->D[(size_t)i * n_mels + m];
    mfcc_delta_kernel(1, o.delta_window, t->s1);
    mfcc_delta_kernel(2, o.delta_window, t->s2);
}

namespace {

// A mean by the rule: term(t), t < T, in blocks of kMfBlock
template <class F> double blocked_mean(uint64_t T, double r_T, F term)
{
    double total = 0.0;
    for (uint64_t t0 = 0; t0 < T; t0 += kMfBlock) {
        double acc = 0.0;
        for (uint64_t t = t0; t < T && t < t0 + kMfBlock; t++)
            acc = acc + term(t);
        total = total + acc;
    }
    return total * r_T;
}

// The rule from the cepstra on: L [T][n_mels] -> out; energy (null: none): the frames' energies of JB_FRAME_ENERGY,
// held to the geometry's floor
void mfcc_rule(const double *L, uint64_t T, uint32_t n_mels, const MfccOpts &o, uint8_t *out,
               const double *energy = nullptr, const FbankGeom *g = nullptr)
{
    if (!T)
        return;
    MfccTables tab;
    mfcc_tables(o, n_mels, &tab);
    const MfccParams p = mfcc_params(o, n_mels, tab);
    const uint32_t d = p.d, width = d * (o.delta_order + 1);
    std::vector<double> c((size_t)T * d);
    for (uint64_t t = 0; t < T; t++)
        for (uint32_t i = 0; i < d; i++)
            c[t * d + i] = !o.n_ceps          ? L[t * n_mels + i]
                           : i == 0 && energy ? mfcc_c0(energy[t], g->log_floor, g->ln_floor)
                                              : mfcc_cep(L + t * n_mels, tab.D.data() + (size_t)i * n_mels, 1, n_mels,
                                                         tab.lift[i]);
    if (o.cmvn != kMfCmvnNone) {
        const double r_T = mfcc_r(T);
        for (uint32_t i = 0; i < d; i++) {
            const double mu = blocked_mean(T, r_T, [&](uint64_t t) { return mfcc_stat_term(c[t * d + i], 0.0, false); });
            double sd = 1.0;
            if (o.cmvn == kMfCmvnMeanVar)
                sd = mfcc_sd(blocked_mean(T, r_T, [&](uint64_t t) { return mfcc_stat_term(c[t * d + i], mu, true); }),
                             p.floor);
            for (uint64_t t = 0; t < T; t++)
                c[t * d + i] = mfcc_norm(c[t * d + i], mu, sd, o.cmvn);
        }
    }
    const int32_t N = (int32_t)o.delta_window;
    for (uint64_t t = 0; t < T; t++)
        for (uint32_t q = 0; q <= o.delta_order; q++)
            for (uint32_t i = 0; i < d; i++) {
                auto at = [&](int32_t j) {
                    const int64_t g = (int64_t)t + j;
                    return c[(size_t)(g < 0 ? 0 : g >= (int64_t)T ? (int64_t)T - 1 : g) * d + i];
                };
                const double v = q == 0 ? c[t * d + i] : mfcc_delta(q == 1 ? p.s1 : p.s2, (int32_t)q * N, at);
                put_elem(out, (size_t)t * width + (size_t)q * d + i, v, (o.flags & kMfF64) != 0);
            }
}

// The whole rule over PCM under the frame request *q and the entry's name `who`: jb_mfcc_framed_pcm_host's body, and
// with the all-zero request (jb_fbank.h "Frame conditioning") jb_mfcc_pcm_host's
int mfcc_pcm_host(const double *in, size_t n, uint32_t hz, const FbankOpts *fo, const MfccOpts *o, const FrameOpts *q,
                  uint8_t *out, size_t cap, const char *who)
{
    int rc = mfcc_check_fbank(fo, who);
    if (rc || (rc = mfcc_check_opts(o, fo->n_mels, who)) || (rc = frame_check(fo, q, o->n_ceps >= 1, who)))
        return rc;
    const FbankOpts f = mfcc_fbank_opts(*fo);
    FbankGeom g{};
    if ((rc = fbank_geometry(&f, hz, who, &g)))
        return rc;
    const uint64_t T = frame_count(n, g, f, *q);
    if (cap < T * mfcc_width(*o, g.n_mels) * mfcc_elem(o->flags)) {
        set_error(std::string(who) + ": the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (n && (!in || (T && !out)))
        return JB_ERR_INVALID;
    std::vector<double> L((size_t)T * f.n_mels + 1), energy;
    const bool e = (q->flags & kFrEnergy) != 0;
    if ((rc = fbank_framed_host(in, n, hz, &f, *q, (uint8_t *)L.data(), sizeof(double) * T * f.n_mels, who,
                                e ? &energy : nullptr)))
        return rc;
    mfcc_rule(L.data(), T, f.n_mels, *o, out, e ? energy.data() : nullptr, &g);
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_mfcc_geometry(uint32_t hz, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts, size_t n, size_t *T,
                     uint32_t *width, size_t *n_bytes)
{
    const FbankOpts *f = (const FbankOpts *)fopts;
    int rc = mfcc_check_fbank(f, "jb_mfcc_geometry");
    if (rc)
        return rc;
    if ((rc = mfcc_check_opts((const MfccOpts *)opts, f->n_mels, "jb_mfcc_geometry")))
        return rc;
    FbankGeom g{};
    if ((rc = fbank_geometry(f, hz, "jb_mfcc_geometry", &g)))
        return rc;
    const uint64_t frames = frame_count(n, g, *f, FrameOpts{});
    const uint32_t w = mfcc_width(*(const MfccOpts *)opts, g.n_mels);
    if (T)
        *T = (size_t)frames;
    if (width)
        *width = w;
    if (n_bytes)
        *n_bytes = (size_t)(frames * w * mfcc_elem(opts->flags));
    return JB_OK;
}

int jb_mfcc_dct(uint32_t n_mels, const jb_mfcc_opts *opts, double *D, size_t cap_D, double *lifter, size_t cap_l)
{
    const int rc = mfcc_check_opts((const MfccOpts *)opts, n_mels, "jb_mfcc_dct");
    if (rc)
        return rc;
    if ((D && cap_D < (size_t)opts->n_ceps * n_mels) || (lifter && cap_l < opts->n_ceps)) {
        set_error("jb_mfcc_dct: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    mfcc_dct(n_mels, opts->n_ceps, opts->lifter, D, lifter);
    return JB_OK;
}

int jb_mfcc_delta_kernel(uint32_t q, uint32_t N, double *s, size_t cap)
{
    if (q > kMfMaxOrder) {
        set_error("jb_mfcc_delta_kernel: delta_order is in 0..2");
        return JB_ERR_INVALID;
    }
    if (N < 1 || N > kMfMaxWindow) {
        set_error("jb_mfcc_delta_kernel: delta_window is in 1..5");
        return JB_ERR_INVALID;
    }
    if (cap < 2 * (size_t)q * N + 1) {
        set_error("jb_mfcc_delta_kernel: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (!s)
        return JB_ERR_INVALID;
    mfcc_delta_kernel(q, N, s);
    return JB_OK;
}

int jb_mfcc_host(const double *L, size_t T, uint32_t n_mels, const jb_mfcc_opts *opts, uint8_t *out, size_t cap)
{
    const MfccOpts *o = (const MfccOpts *)opts;
    const int rc = mfcc_check_opts(o, n_mels, "jb_mfcc_host");
    if (rc)
        return rc;
    if (cap < (uint64_t)T * mfcc_width(*o, n_mels) * mfcc_elem(o->flags)) {
        set_error("jb_mfcc_host: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (T && (!L || !out))
        return JB_ERR_INVALID;
    mfcc_rule(L, T, n_mels, *o, out);
    return JB_OK;
}

int jb_mfcc_pcm_host(const double *in, size_t n, uint32_t hz, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts,
                     uint8_t *out, size_t cap)
{
    // (what the options and the rate refuse keeps jb_mfcc_geometry's name, as it always had)
    const int rc = jb_mfcc_geometry(hz, fopts, opts, n, nullptr, nullptr, nullptr);
    const FrameOpts none{};
    return rc ? rc
              : mfcc_pcm_host(in, n, hz, (const FbankOpts *)fopts, (const MfccOpts *)opts, &none, out, cap,
                              "jb_mfcc_pcm_host");
}

int jb_mfcc_framed_pcm_host(const double *in, size_t n, uint32_t hz, const jb_fbank_opts *fopts,
                            const jb_mfcc_opts *opts, const jb_frame_opts *fr, uint8_t *out, size_t cap)
{
    return mfcc_pcm_host(in, n, hz, (const FbankOpts *)fopts, (const MfccOpts *)opts, (const FrameOpts *)fr, out, cap,
                         "jb_mfcc_framed_pcm_host");
}

void jb_mfcc_free(uint8_t *p) { free(p); }

} // extern "C"

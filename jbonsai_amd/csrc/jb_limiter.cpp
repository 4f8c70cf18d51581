// jb_limiter.cpp -- the host half of the limiter stage: the request check, the smoothing window, the device table of a
// class, and the rules of jb_limiter.h over PCM the caller holds without a GPU (jb_limiter_host, what the kernel is
// checked against).
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(LimOpts) == sizeof(jb_limiter_opts) &&
                  offsetof(LimOpts, lookahead_ms) == offsetof(jb_limiter_opts, lookahead_ms) &&
                  offsetof(LimOpts, hold_ms) == offsetof(jb_limiter_opts, hold_ms) &&
                  offsetof(LimOpts, max_reduction_db) == offsetof(jb_limiter_opts, max_reduction_db) &&
                  offsetof(LimOpts, flags) == offsetof(jb_limiter_opts, flags) &&
                  offsetof(LimOpts, reserved) == offsetof(jb_limiter_opts, reserved) && kLimExact == JB_LIMITER_EXACT && kLimOff == JB_LIMITER_OFF &&
                  kLimTaps == kTpTaps && kLimMaxF == kTpMaxF,
              "jb_limiter.h restates the header's request and the true-peak table's shape");

int limiter_check(const jb_limiter_opts *opts, size_t utt, const char *who, LimOpts *out)
{
    const char *field = "";
    LimOpts r{};
    if (!lim_resolve((const LimOpts *)opts, &r, &field)) {
        const std::string f = field;
        set_error(std::string(who) + ": utterance " + std::to_string(utt) + ": " + f +
                  (f == "flags"             ? " has a bit that is none of JB_LIMITER_*"
                   : f == "reserved"        ? " must be 0"
                   : f == "lookahead_ms"    ? " is not inside (0, 10]"
                   : f == "hold_ms"         ? " is not inside [0, 50]"
                                            : " is not inside [0, 24]"));
        return JB_ERR_INVALID;
    }
    if (out)
        *out = r;
    return JB_OK;
}

int limiter_geometry(const LimOpts &r, uint32_t hz, size_t utt, const char *who, uint32_t *L, uint32_t *H)
{
    if (hz == 0) {
        set_error(std::string(who) + ": a rate of 0 Hz (utterance " + std::to_string(utt) + ")");
        return JB_ERR_INVALID;
    }
    const uint64_t l = lim_lookahead(r, hz), h = lim_hold(r, hz);
    if (2 * l + h > kLimMaxSpan) {
        set_error(std::string(who) + ": utterance " + std::to_string(utt) + ": a look-ahead of " + std::to_string(l) +
                  " and a hold of " + std::to_string(h) + " samples at " + std::to_string(hz) +
                  " Hz (2 L + H is at most " + std::to_string(kLimMaxSpan) + ")");
        return JB_ERR_UNSUPPORTED;
    }
    *L = (uint32_t)l;
    *H = (uint32_t)h;
    return JB_OK;
}

void limiter_window(uint32_t L, double *w)
{
    // the interior of a Hann window of L + 3 points, i = 1 .. L + 1 of 0 .. L + 2: its first half, mirrored
    const long double pi = 3.14159265358979323846264338327950288L;
    std::vector<long double> h(L + 1);
    long double sum = 0.0L;
    for (uint32_t j = 0; j <= L; j++) {
        const uint32_t k = std::min(j, L - j);
        h[j] = 0.5L - 0.5L * cosl(2.0L * pi * (long double)(k + 1) / (long double)(L + 2));
    }
    for (uint32_t j = 0; j <= L; j++) // (ascending: the same sum from both ends is not needed, h is symmetric)
        sum += h[j];
    for (uint32_t j = 0; j <= L; j++)
        w[j] = (double)(h[std::min(j, L - j)] / sum);
}

int limiter_class_build(uint32_t hz, uint32_t L, uint32_t H, uint32_t mode, LimiterClass *out)
{
    memset(out, 0, sizeof *out);
    out->L = L;
    out->H = H;
    out->F = 1;
    limiter_window(L, out->w);
    if (mode == JB_PEAK_TRUE)
        return true_peak_table(hz, &out->F, out->tp);
    return JB_OK;
}

int LimiterClasses::find(uint32_t hz, uint32_t L, uint32_t H, uint32_t mode, uint32_t *cls)
{
    const uint32_t key = mode == JB_PEAK_TRUE ? hz : 0; // (the sample detector's table does not depend on the rate)
    for (size_t i = 0; i < tables.size(); i++)
        if (key_hz[i] == key && tables[i].L == L && tables[i].H == H) {
            *cls = (uint32_t)i;
            return JB_OK;
        }
    tables.emplace_back();
    key_hz.push_back(key);
    *cls = (uint32_t)tables.size() - 1;
    return limiter_class_build(hz, L, H, mode, &tables.back());
}

namespace {

inline void lim_store(double v, double *o) { *o = v; }
inline void lim_store(double v, int16_t *o) { *o = (int16_t)fmt_quant<false>(v, -32768.0, 32767.0, 0, 0); }

template <class T>
int limiter_host(const double *x, uint64_t n, uint32_t hz, double gain, double ceiling_db, uint32_t mode,
                 const jb_limiter_opts *opts, T *y, jb_limiter_report *report, const char *who)
{
    if (n && (!x || !y))
        return JB_ERR_INVALID;
    if (mode != JB_PEAK_SAMPLE && mode != JB_PEAK_TRUE) {
        set_error(std::string(who) + ": a mode is JB_PEAK_SAMPLE or JB_PEAK_TRUE");
        return JB_ERR_INVALID;
    }
    LimOpts r{};
    uint32_t L = 0, H = 0;
    int rc;
    if ((rc = limiter_check(opts, 0, who, &r)))
        return rc;
    if (r.flags & kLimOff) { // not limited: its values, and so a geometry, are not read
        for (uint64_t i = 0; i < n; i++)
            lim_store(x[i] * gain, &y[i]);
        if (report)
            *report = jb_limiter_report{0.0, 0, 0, 0};
        return JB_OK;
    }
    if ((rc = limiter_geometry(r, hz, 0, who, &L, &H)))
        return rc;
    std::unique_ptr<LimiterClass> K(new LimiterClass);
    if ((rc = limiter_class_build(hz, L, H, mode, K.get())))
        return rc;
    const double c = lim_ceiling(ceiling_db);
    const int64_t N = (int64_t)n;
    auto u = [&](int64_t i) { return i >= 0 && i < N ? x[i] * gain : 0.0; };
    // steps 2 and 3
    std::vector<double> b, rr(n);
    if (K->F > 1) {
        b.resize(n + 1); // b[i] is the rule's b[i - 1]
        for (int64_t i = -1; i < N; i++) {
            double v[kLimTaps];
            for (uint32_t q = 0; q < kLimTaps; q++)
                v[q] = u(i - 5 + (int64_t)q);
            b[(size_t)(i + 1)] = lim_between(K->tp, K->F, v);
        }
    }
    std::vector<uint64_t> over(n + 1, 0); // over[i]: samples below i with d > c
    for (int64_t i = 0; i < N; i++) {
        double d = fabs(u(i));
        if (K->F > 1)
            d = fmax(d, fmax(b[(size_t)i], b[(size_t)i + 1]));
        rr[(size_t)i] = lim_ratio(c, d);
        over[(size_t)i + 1] = over[(size_t)i] + (d > c);
    }
    auto any_over = [&](int64_t lo, int64_t hi) { // in [lo, hi]
        lo = std::max<int64_t>(lo, 0);
        hi = std::min<int64_t>(hi, N - 1);
        return lo <= hi && over[(size_t)hi + 1] != over[(size_t)lo];
    };
    auto rat = [&](int64_t i) { return i >= 0 && i < N ? rr[(size_t)i] : 1.0; };
    // step 4, where some d > c is in reach (1 elsewhere): slot k + L
    std::vector<double> m((size_t)(N + L), 1.0);
    for (int64_t k = -(int64_t)L; k < N; k++)
        if (any_over(k - H, k + L)) {
            double v = 1.0;
            for (int64_t i = k - H; i <= k + (int64_t)L; i++)
                v = fmin(v, rat(i));
            m[(size_t)(k + L)] = v;
        }
    double min_a = 1.0;
    uint64_t count = 0;
    for (int64_t i = 0; i < N; i++) {
        double a = 1.0;
        if (any_over(i - L - H, i + L)) {
            a = lim_smooth(K->w, L, [&](uint32_t j) { return m[(size_t)(i + L - j)]; });
            a = lim_gain(a, rr[(size_t)i]);
        }
        min_a = fmin(min_a, a);
        count += a < 1.0;
        lim_store(lim_out(u(i), a, c), &y[i]);
    }
    if (report)
        *report = jb_limiter_report{lim_reduction_db(min_a), count, L, H};
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_limiter_window(uint32_t hz, const jb_limiter_opts *opts, uint32_t *L, uint32_t *H, double *w, size_t cap)
{
    LimOpts r{};
    uint32_t l = 0, h = 0;
    int rc;
    if ((rc = limiter_check(opts, 0, "jb_limiter_window", &r)) ||
        (rc = limiter_geometry(r, hz, 0, "jb_limiter_window", &l, &h)))
        return rc;
    if (L)
        *L = l;
    if (H)
        *H = h;
    if (!w)
        return JB_OK;
    if (cap < (size_t)l + 1) {
        set_error("jb_limiter_window: the buffer holds fewer than L + 1 values");
        return JB_ERR_BUFFER;
    }
    limiter_window(l, w);
    return JB_OK;
}

int jb_limiter_host(const double *x, uint64_t n, uint32_t hz, double gain, double ceiling_dbfs, uint32_t peak_mode,
                    const jb_limiter_opts *opts, double *y, jb_limiter_report *report)
{
    return limiter_host(x, n, hz, gain, ceiling_dbfs, peak_mode, opts, y, report, "jb_limiter_host");
}

int jb_limiter_host_i16(const double *x, uint64_t n, uint32_t hz, double gain, double ceiling_dbfs,
                        uint32_t peak_mode, const jb_limiter_opts *opts, int16_t *y, jb_limiter_report *report)
{
    return limiter_host(x, n, hz, gain, ceiling_dbfs, peak_mode, opts, y, report, "jb_limiter_host_i16");
}

void jb_limiter_free(void *p) { free(p); }

} // extern "C"

// jb_fir.cpp -- the host half of the convolution stage: the request check, the distinct responses of a launch, their
// device tables (the taps; in partitioned mode the partitions' spectra and the twiddles, long double, rounded once) and
// the rule of jb_fir.h over PCM the caller holds without a GPU (jb_fir_host, what the kernels are checked against).
#include "jb_host.h"

#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(FirSpec) == sizeof(jb_fir) && offsetof(FirSpec, taps) == offsetof(jb_fir, taps) &&
                  offsetof(FirSpec, n_taps) == offsetof(jb_fir, n_taps) && offsetof(FirSpec, hz) == offsetof(jb_fir, hz) &&
                  offsetof(FirSpec, delay) == offsetof(jb_fir, delay) &&
                  offsetof(FirSpec, reserved) == offsetof(jb_fir, reserved),
              "jb_fir.h restates the header's request");
static_assert(kFirMaxTaps == JB_FIR_MAX_TAPS && kFirDirectMax == JB_FIR_DIRECT_MAX && kFirDirect == JB_FIR_DIRECT &&
                  kFirPartitioned == JB_FIR_PARTITIONED,
              "jb_fir.h restates the header's constants");
static_assert(fir_geometry(kFirMaxTaps).partitions == 64 && fir_geometry(kFirSmallMax).partitions == 4 &&
                  fir_geometry(kFirDirectMax + 1).n_fft == kFirSmallFft,
              "the partition counts of the two transforms");

int fir_check(const jb_fir *f, uint32_t hz, size_t utt, const char *who)
{
    const char *fault = f ? fir_fault(*(const FirSpec *)f, hz) : "the request is NULL";
    if (!fault)
        return JB_OK;
    std::string msg = std::string(who) + ": utterance " + std::to_string(utt) + ": " + fault;
    if (f && f->taps && f->n_taps && f->hz != hz && std::string(fault).rfind("hz", 0) == 0)
        msg += ": " + std::to_string(f->hz) + " Hz against " + std::to_string(hz) + " Hz";
    set_error(msg);
    return JB_ERR_INVALID;
}

uint32_t FirClasses::find(const FirSpec &f)
{
    for (size_t i = 0; i < resp.size(); i++) {
        const FirResponse &r = resp[i];
        if (r.hz == f.hz && r.delay == f.delay && r.taps.size() == f.n_taps &&
            !memcmp(r.taps.data(), f.taps, sizeof(double) * f.n_taps))
            return (uint32_t)i;
    }
    FirResponse r;
    r.taps.assign(f.taps, f.taps + f.n_taps);
    r.hz = f.hz;
    r.delay = f.delay;
    r.g = fir_geometry(f.n_taps);
    if (r.g.mode == kFirPartitioned)
        fir_spectra(r, &r.H, &r.tw);
    resp.push_back(std::move(r));
    return (uint32_t)resp.size() - 1;
}

namespace {

// In-place transform of n = 2^log2n points, e^(-2 pi i jk / n), in long double
void fft_ld(std::vector<long double> &re, std::vector<long double> &im, uint32_t log2n,
            const std::vector<long double> &c, const std::vector<long double> &s)
{
    const uint32_t n = 1u << log2n;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < log2n; b++)
            r |= ((i >> b) & 1u) << (log2n - 1 - b);
        if (r > i) {
            std::swap(re[i], re[r]);
            std::swap(im[i], im[r]);
        }
    }
    for (uint32_t st = 0; st < log2n; st++) {
        const uint32_t half = 1u << st;
        for (uint32_t j = 0; j < n / 2; j++) {
            const uint32_t pos = j & (half - 1), i0 = ((j >> st) << (st + 1)) | pos, i1 = i0 + half;
            const uint32_t k = pos << (log2n - st - 1);
            const long double tr = c[k] * re[i1] + s[k] * im[i1], ti = c[k] * im[i1] - s[k] * re[i1];
            re[i1] = re[i0] - tr, im[i1] = im[i0] - ti;
            re[i0] += tr, im[i0] += ti;
        }
    }
}

} // namespace

void fir_spectra(const FirResponse &r, std::vector<double> *H, std::vector<double> *tw)
{
    const uint32_t n_fft = r.g.n_fft, M = n_fft / 2, Bk = r.g.block, P = r.g.partitions;
    uint32_t log2n = 0;
    while ((1u << log2n) < n_fft)
        log2n++;
    const long double two_pi = 2.0L * acosl(-1.0L);
    std::vector<long double> c(M), s(M); // cos, sin of 2 pi k / n_fft
    for (uint32_t k = 0; k < M; k++) {
        c[k] = cosl(two_pi * k / (long double)n_fft);
        s[k] = sinl(two_pi * k / (long double)n_fft);
    }
    *tw = rfft_twiddles(n_fft);
    H->assign((size_t)P * (M + 1) * 2, 0.0);
    std::vector<long double> re(n_fft), im(n_fft);
    const size_t K = r.taps.size();
    for (uint32_t p = 0; p < P; p++) {
        for (uint32_t i = 0; i < n_fft; i++) {
            const size_t k = (size_t)p * Bk + i;
            re[i] = i < Bk && k < K ? (long double)r.taps[k] : 0.0L;
            im[i] = 0.0L;
        }
        fft_ld(re, im, log2n, c, s);
        double *out = H->data() + (size_t)p * (M + 1) * 2;
        for (uint32_t k = 0; k <= M; k++) {
            out[2 * k] = (double)(re[k] / (long double)M);
            out[2 * k + 1] = (double)(im[k] / (long double)M);
        }
    }
}

void FirClasses::bind(const double *dev, std::vector<double> *image, std::vector<FirClass> *out) const
{
    TableImage img(dev);
    out->clear();
    for (const FirResponse &r : resp) {
        FirClass c{};
        c.h = img.put(r.taps);
        c.K = (uint32_t)r.taps.size();
        c.delay = r.delay;
        c.mode = r.g.mode;
        c.block = r.g.block;
        c.partitions = r.g.partitions;
        c.n_fft = r.g.n_fft;
        if (r.g.mode == kFirPartitioned) {
            c.H = img.put(r.H);
            c.tw = img.put(r.tw);
            for (c.log2m = 0; (2u << c.log2m) < r.g.n_fft;)
                c.log2m++;
            c.lead = fir_lead(r.delay, r.g.block);
        }
        out->push_back(c);
    }
    *image = std::move(img.words);
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_fir_geometry(uint32_t n_taps, uint32_t *mode, uint32_t *block, uint32_t *partitions)
{
    if (n_taps == 0 || n_taps > kFirMaxTaps) {
        set_error("jb_fir_geometry: n_taps is in 1..JB_FIR_MAX_TAPS (131072)");
        return JB_ERR_INVALID;
    }
    const FirGeom g = fir_geometry(n_taps);
    if (mode)
        *mode = g.mode;
    if (block)
        *block = g.block;
    if (partitions)
        *partitions = g.partitions;
    return JB_OK;
}

int jb_fir_host(const double *in, size_t n, const jb_fir *f, double *out, size_t cap)
{
    if (n && (!in || !out))
        return JB_ERR_INVALID;
    const int rc = fir_check(f, f ? f->hz : 0, 0, "jb_fir_host");
    if (rc)
        return rc;
    if (cap < n) {
        set_error("jb_fir_host: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (!f->taps) {
        memmove(out, in, sizeof(double) * n);
        return JB_OK;
    }
    for (size_t i = 0; i < n; i++)
        out[i] = fir_sample(f->taps, f->n_taps, f->delay, n, i, [&](uint64_t k) { return in[k]; });
    return JB_OK;
}

void jb_fir_free(void *p) { free(p); }

} // extern "C"

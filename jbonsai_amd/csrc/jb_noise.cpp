// jb_noise.cpp -- the host half of the noise stage: the request check, the resolved request of an utterance (seed,
// offset, the two ratios), the distinct beds of a launch, and the rule of jb_noise.h over PCM the caller holds without
// a GPU (jb_noise_host, what the kernels are checked against).
#include "jb_host.h"

#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(NoiseSpec) == sizeof(jb_noise) && offsetof(NoiseSpec, bed) == offsetof(jb_noise, bed) &&
                  offsetof(NoiseSpec, seed) == offsetof(jb_noise, seed) &&
                  offsetof(NoiseSpec, snr_db) == offsetof(jb_noise, snr_db) &&
                  offsetof(NoiseSpec, gate_db) == offsetof(jb_noise, gate_db) &&
                  offsetof(NoiseSpec, kind) == offsetof(jb_noise, kind) &&
                  offsetof(NoiseSpec, bed_len) == offsetof(jb_noise, bed_len) &&
                  offsetof(NoiseSpec, hz) == offsetof(jb_noise, hz) &&
                  offsetof(NoiseSpec, offset) == offsetof(jb_noise, offset) &&
                  offsetof(NoiseSpec, reference) == offsetof(jb_noise, reference) &&
                  offsetof(NoiseSpec, flags) == offsetof(jb_noise, flags) &&
                  offsetof(NoiseSpec, reserved) == offsetof(jb_noise, reserved),
              "jb_noise.h restates the header's request");
static_assert(kNoiseBed == JB_NOISE_BED && kNoiseWhite == JB_NOISE_WHITE && kNoiseRefWhole == JB_NOISE_REF_WHOLE &&
                  kNoiseRefActive == JB_NOISE_REF_ACTIVE && kNoiseVary == JB_NOISE_VARY &&
                  kNoiseMaxBed == JB_NOISE_MAX_BED,
              "jb_noise.h restates the header's constants");
static_assert(sizeof(jb_noise) == 64 && sizeof(jb_noise_report) == 56, "the layouts the bindings restate");

int noise_check(const jb_noise *req, uint32_t hz, size_t utt, const char *who)
{
    const char *fault = req ? noise_fault(*(const NoiseSpec *)req, hz) : "the request is NULL";
    if (!fault)
        return JB_OK;
    std::string msg = std::string(who) + ": utterance " + std::to_string(utt) + ": " + fault;
    if (req && std::string(fault).rfind("hz", 0) == 0)
        msg += ": " + std::to_string(req->hz) + " Hz against " + std::to_string(hz) + " Hz";
    set_error(msg);
    return JB_ERR_INVALID;
}

NoiseItem noise_resolve(const jb_noise &req, bool vary, uint64_t k, int32_t bed)
{
    NoiseItem it;
    it.on = true;
    it.bed = bed;
    it.seed = req.seed;
    it.offset = req.kind == kNoiseBed ? req.offset : 0;
    if (vary)
        noise_vary(req.seed, k, req.kind == kNoiseBed ? req.bed_len : 0, &it.seed, &it.offset);
    it.snr_db = req.snr_db;
    it.r = noise_ratio(req.snr_db);
    it.active = req.reference == kNoiseRefActive;
    it.q = it.active ? noise_ratio(-req.gate_db) : 0.0;
    return it;
}

int32_t NoiseBeds::find(const double *w, uint32_t len, uint32_t hz)
{
    for (size_t i = 0; i < beds.size(); i++)
        if (rate[i] == hz && beds[i].size() == len && !memcmp(beds[i].data(), w, sizeof(double) * len))
            return (int32_t)i;
    beds.emplace_back(w, w + len);
    rate.push_back(hz);
    return (int32_t)beds.size() - 1;
}

uint64_t NoiseBeds::words() const
{
    uint64_t n = 0;
    for (const std::vector<double> &v : beds)
        n += v.size();
    return n;
}

void NoiseBeds::bind(const double *dev, std::vector<double> *image, std::vector<NoiseBed> *out) const
{
    image->clear();
    out->clear();
    for (size_t i = 0; i < beds.size(); i++) {
        out->push_back(NoiseBed{dev + image->size(), (uint32_t)beds[i].size(), rate[i]});
        image->insert(image->end(), beds[i].begin(), beds[i].end());
    }
}

jb_noise_report noise_report_of(const NoiseItem &it, const NoiseRecord &r, uint64_t n)
{
    jb_noise_report o{};
    o.speech_power = r.C ? r.A / (double)r.C : 0.0;
    o.noise_power = n ? r.Bs / (double)n : 0.0;
    o.gain = r.gain;
    o.snr_db = it.snr_db;
    o.active_samples = r.C;
    o.seed = it.seed;
    o.offset = it.offset;
    return o;
}

namespace {

// the tile sums of z[0..N), by the rule: 256 partials, the tree, p[0]
template <class Z> void tile_sums(uint64_t N, Z at, std::vector<double> *t)
{
    t->assign((size_t)noise_tiles(N), 0.0);
    double p[kNoiseLanes];
    for (uint64_t i = 0; i < t->size(); i++) {
        for (uint32_t l = 0; l < kNoiseLanes; l++)
            p[l] = noise_partial(N, i, l, at);
        for (uint32_t h = kNoiseLanes / 2; h; h >>= 1)
            for (uint32_t l = 0; l < h; l++)
                p[l] = p[l] + p[l + h];
        (*t)[i] = p[0];
    }
}

double total(const std::vector<double> &t)
{
    if (t.empty())
        return 0.0;
    double S = t[0];
    for (size_t i = 1; i < t.size(); i++)
        S = S + t[i];
    return S;
}

template <class T> void put(double v, T *o);
template <> void put<double>(double v, double *o) { *o = v; }
template <> void put<int16_t>(double v, int16_t *o) { *o = (int16_t)fmt_quant<false>(v, -32768.0, 32767.0, 0, 0); }

template <class T>
int noise_host(const double *x, size_t n, const jb_noise *req, const double *gain, T *y, size_t cap,
               jb_noise_report *report, const char *who)
{
    if (n && (!x || !y))
        return JB_ERR_INVALID;
    const int rc = noise_check(req, req ? req->hz : 0, 0, who);
    if (rc)
        return rc;
    if (cap < n) {
        set_error(std::string(who) + ": the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (report)
        *report = jb_noise_report{};
    if (noise_none(*(const NoiseSpec *)req)) {
        for (size_t i = 0; i < n; i++)
            put(x[i], &y[i]);
        return JB_OK;
    }
    const NoiseItem it = noise_resolve(*req, false, 0, req->kind == kNoiseBed ? 0 : -1);
    const uint64_t mseed = fmt_mix(it.seed);
    const double *bed = req->bed;
    const uint32_t lb = req->bed_len;
    auto w = [&](uint64_t k) { return bed ? bed[(it.offset + k) % lb] : noise_white(mseed, k); };
    std::vector<double> tx, tw;
    tile_sums(n, [&](uint64_t k) { return x[k]; }, &tx);
    tile_sums(n, w, &tw);
    NoiseRecord r{};
    const double Sx = total(tx);
    r.Bs = total(tw);
    r.A = Sx;
    r.C = n;
    if (it.active) {
        const double Sq = Sx * it.q, dn = (double)n;
        bool first = true;
        r.A = 0.0;
        r.C = 0;
        for (size_t i = 0; i < tx.size(); i++) {
            const uint32_t c = (uint32_t)std::min<uint64_t>(kNoiseTile, n - i * (uint64_t)kNoiseTile);
            if (!noise_active(tx[i], dn, Sq, c))
                continue;
            r.A = first ? tx[i] : r.A + tx[i];
            r.C += c;
            first = false;
        }
    }
    r.gain = gain ? *gain : noise_gain(r.A, r.C, r.Bs, n, it.r);
    for (size_t i = 0; i < n; i++)
        put(r.gain == 0.0 ? x[i] : __builtin_fma(r.gain, w(i), x[i]), &y[i]);
    if (report)
        *report = noise_report_of(it, r, n);
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_noise_host(const double *x, size_t n, const jb_noise *req, const double *gain, double *y, size_t cap,
                  jb_noise_report *report)
{
    return noise_host(x, n, req, gain, y, cap, report, "jb_noise_host");
}

int jb_noise_host_i16(const double *x, size_t n, const jb_noise *req, const double *gain, int16_t *y, size_t cap,
                      jb_noise_report *report)
{
    return noise_host(x, n, req, gain, y, cap, report, "jb_noise_host_i16");
}

int jb_noise_white(uint64_t seed, uint64_t first, size_t count, double *out)
{
    if (count && !out)
        return JB_ERR_INVALID;
    const uint64_t mseed = fmt_mix(seed);
    for (size_t i = 0; i < count; i++)
        out[i] = noise_white(mseed, first + i);
    return JB_OK;
}

int jb_noise_vary(uint64_t seed, uint64_t k, uint32_t bed_len, uint64_t *seed_k, uint32_t *offset_k)
{
    uint64_t s;
    uint32_t o;
    noise_vary(seed, k, bed_len, &s, &o);
    if (seed_k)
        *seed_k = s;
    if (offset_k)
        *offset_k = o;
    return JB_OK;
}

void jb_noise_free(void *p) { free(p); }

} // extern "C"

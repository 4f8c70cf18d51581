// jb_filter.cpp -- the host half of the filter stage: the request check, the design, the device tables (the transition
// matrices of a cascade and their powers), the work lists of a launch, and the rules of jb_filter.h over PCM the caller
// holds without a GPU (jb_filter_pcm_host, what the kernels are checked against).
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(FilterSection) == sizeof(jb_filter_section) && offsetof(FilterSection, kind) == offsetof(jb_filter_section, kind) &&
                  offsetof(FilterSection, f0_hz) == offsetof(jb_filter_section, f0_hz) &&
                  offsetof(FilterSection, q) == offsetof(jb_filter_section, q) &&
                  offsetof(FilterSection, gain_db) == offsetof(jb_filter_section, gain_db) &&
                  offsetof(FilterSection, raw) == offsetof(jb_filter_section, b0) &&
                  sizeof(FilterSpec) == sizeof(jb_filter) && offsetof(FilterSpec, n_sections) == offsetof(jb_filter, n_sections) &&
                  kFiltMaxSections == JB_FILTER_MAX_SECTIONS && kFiltHighpass == JB_FILTER_HIGHPASS &&
                  kFiltLowpass == JB_FILTER_LOWPASS && kFiltPeaking == JB_FILTER_PEAKING &&
                  kFiltLowshelf == JB_FILTER_LOWSHELF && kFiltHighshelf == JB_FILTER_HIGHSHELF &&
                  kFiltNotch == JB_FILTER_NOTCH && kFiltRaw == JB_FILTER_RAW && sizeof(jb_biquad) == kFiltCoefs * sizeof(double),
              "jb_filter.h restates the header's request");

int filter_design_checked(const jb_filter *f, uint32_t hz, size_t utt, double *c, const char *who)
{
    if (hz == 0) {
        set_error(std::string(who) + ": a rate of 0 Hz (utterance " + std::to_string(utt) + ")");
        return JB_ERR_INVALID;
    }
    const char *field = "";
    const uint32_t bad = filt_design(*(const FilterSpec *)f, hz, c, &field);
    if (!bad)
        return JB_OK;
    std::string msg = std::string(who) + ": utterance " + std::to_string(utt);
    if (bad > kFiltMaxSections) {
        msg += std::string(": ") + field +
               (field[0] == 'n' ? " is " + std::to_string(f->n_sections) + " (at most " +
                                      std::to_string(kFiltMaxSections) + " sections)"
                                : std::string(" must be 0"));
    } else {
        const jb_filter_section &s = f->section[bad - 1];
        msg += ", section " + std::to_string(bad - 1) + ": " + field;
        const std::string fl = field;
        if (fl == "kind")
            msg += " " + std::to_string(s.kind) + " is none of JB_FILTER_*";
        else if (fl == "reserved")
            msg += " must be 0";
        else if (fl == "f0_hz")
            msg += " = " + std::to_string(s.f0_hz) + " is not inside (0, " + std::to_string(0.5 * hz) + ") at " +
                   std::to_string(hz) + " Hz";
        else if (fl == "q")
            msg += " = " + std::to_string(s.q) + " is not a finite value above 0";
        else if (fl == "gain_db")
            msg += " is not finite";
        else if (fl == "poles")
            msg += " of the designed section are not strictly inside the unit circle";
        else if (fl == "a1" || fl == "a2")
            msg += isfinite(fl == "a1" ? s.a1 : s.a2)
                       ? " puts a pole on or outside the unit circle (|a2| < 1 and |a1| < 1 + a2 are required)"
                       : " is not finite";
        else
            msg += " is not finite";
    }
    set_error(msg);
    return JB_ERR_INVALID;
}

void filter_class_build(const double *c, uint32_t ns, FilterClass *out)
{
    FilterClass &fc = *out;
    memset(&fc, 0, sizeof(fc));
    fc.ns = ns;
    std::copy(c, c + ns * kFiltCoefs, fc.c);
    if (ns == 0)
        return;
    const uint32_t D = 2 * ns;
    // A: one sample with x = 0, column j from the unit state e_j -- the device's recursion, term for term.  Its
    // powers by squaring in extended precision, rounded once
    long double M[kFiltMaxD * kFiltMaxD], T[kFiltMaxD * kFiltMaxD];
    for (uint32_t j = 0; j < D; j++) {
        double s[kFiltMaxD] = {};
        s[j] = 1.0;
        filt_step(fc.c, s, 0.0, ns);
        for (uint32_t i = 0; i < D; i++)
            M[i * D + j] = s[i];
    }
    auto square = [&]() {
        for (uint32_t i = 0; i < D; i++)
            for (uint32_t j = 0; j < D; j++) {
                long double acc = 0.0L;
                for (uint32_t k = 0; k < D; k++)
                    acc += M[i * D + k] * M[k * D + j];
                T[i * D + j] = acc;
            }
        std::copy(T, T + D * D, M);
    };
    static_assert(kFiltS == 16 && kFiltTile == 4096, "A^16 by four squarings, A^4096 by eight more");
    for (int i = 0; i < 4; i++)
        square();
    for (uint32_t k = 0; k < 8; k++) {
        for (uint32_t i = 0; i < D * D; i++)
            fc.P[k][i] = (double)M[i];
        square();
    }
    for (uint32_t k = 0; k < kFiltTilePows; k++) {
        for (uint32_t i = 0; i < D * D; i++)
            fc.Pt[k][i] = (double)M[i];
        square();
    }
}

int filter_classes(const jb_filter *f, size_t nf, const uint32_t *hz, size_t B, std::vector<FilterClass> *classes,
                   std::vector<uint32_t> *cls_of, const char *who)
{
    classes->clear();
    cls_of->assign(B, 0);
    struct Key {
        uint32_t hz, ns;
        double c[kFiltMaxSections * kFiltCoefs];
        bool operator<(const Key &o) const { return memcmp(this, &o, sizeof(Key)) < 0; }
    };
    std::map<Key, uint32_t> seen;
    for (size_t u = 0; u < B; u++) {
        const jb_filter &fu = f[nf == 1 ? 0 : u];
        Key k;
        memset(&k, 0, sizeof(k));
        int rc = filter_design_checked(&fu, hz[u], u, k.c, who);
        if (rc)
            return rc;
        k.ns = fu.n_sections;
        k.hz = k.ns ? hz[u] : 0; // (one identity class for every rate)
        auto it = seen.find(k);
        if (it == seen.end()) {
            it = seen.emplace(k, (uint32_t)classes->size()).first;
            classes->emplace_back();
            filter_class_build(k.c, k.ns, &classes->back());
        }
        (*cls_of)[u] = it->second;
    }
    return JB_OK;
}

int filter_launch_list(const std::vector<FilterClass> &classes, const std::vector<FilterUtt> &utts,
                       const std::vector<uint8_t> *only, FilterLaunch *out)
{
    *out = FilterLaunch{};
    for (uint32_t ns = 0; ns <= kFiltMaxSections; ns++)
        for (size_t u = 0; u < utts.size(); u++) {
            if ((only && !(*only)[u]) || classes[utts[u].cls].ns != ns)
                continue;
            FilterUtt w = utts[u];
            w.t0 = out->tiles[ns];
            out->tiles[ns] += w.ntiles;
            out->count[ns]++;
            out->utts.push_back(w);
        }
    for (uint32_t ns = 0; ns <= kFiltMaxSections; ns++)
        if (out->tiles[ns] > 0x7fffffffull) {
            set_error("filter: too many tiles for one launch");
            return JB_ERR_UNSUPPORTED;
        }
    return JB_OK;
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_filter_design(const jb_filter *f, uint32_t hz, jb_biquad out[JB_FILTER_MAX_SECTIONS])
{
    if (!f)
        return JB_ERR_INVALID;
    double c[kFiltMaxSections * kFiltCoefs] = {};
    int rc = filter_design_checked(f, hz, 0, c, "jb_filter_design");
    if (rc)
        return rc;
    if (out)
        memcpy(out, c, sizeof(double) * kFiltCoefs * f->n_sections);
    return JB_OK;
}

int jb_filter_pcm_host(const double *in, size_t n, const jb_filter *f, uint32_t hz, double *out, size_t cap)
{
    if (!f || (n && (!in || !out)))
        return JB_ERR_INVALID;
    double c[kFiltMaxSections * kFiltCoefs] = {};
    int rc = filter_design_checked(f, hz, 0, c, "jb_filter_pcm_host");
    if (rc)
        return rc;
    if (cap < n) {
        set_error("jb_filter_pcm_host: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    double s[kFiltMaxD] = {};
    for (size_t i = 0; i < n; i++)
        out[i] = filt_step(c, s, in[i], f->n_sections);
    return JB_OK;
}

void jb_filter_free(void *p) { free(p); }

} // extern "C"

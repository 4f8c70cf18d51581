// jb_mix.cpp -- the host half of the mix stage: the request check, the geometry, the work lists of a launch and the
// rules of jb_mix.h over PCM the caller holds without a GPU (jb_mix_host, what the kernel is checked against).
#include "jb_host.h"

#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(MixUtt) == sizeof(jb_mix_utt) && offsetof(MixUtt, programme) == offsetof(jb_mix_utt, programme) &&
                  offsetof(MixUtt, fade_in) == offsetof(jb_mix_utt, fade_in) &&
                  offsetof(MixUtt, fade_out) == offsetof(jb_mix_utt, fade_out) &&
                  offsetof(MixUtt, reserved) == offsetof(jb_mix_utt, reserved) &&
                  offsetof(MixUtt, start) == offsetof(jb_mix_utt, start) &&
                  offsetof(MixUtt, pad_after) == offsetof(jb_mix_utt, pad_after) &&
                  offsetof(MixUtt, gain_db) == offsetof(jb_mix_utt, gain_db) &&
                  offsetof(MixUtt, reserved2) == offsetof(jb_mix_utt, reserved2) && kMixNone == JB_MIX_NONE,
              "jb_mix.h restates the header's request");
static_assert(sizeof(MixOpts) == sizeof(jb_mix_opts) && offsetof(MixOpts, ceiling_db) == offsetof(jb_mix_opts, ceiling_db) &&
                  kMixFit == JB_MIX_FIT,
              "jb_mix.h restates the header's options");
static_assert(sizeof(MixReport) == sizeof(jb_mix_report) && offsetof(MixReport, scale) == offsetof(jb_mix_report, scale) &&
                  offsetof(MixReport, depth) == offsetof(jb_mix_report, depth) &&
                  offsetof(MixReport, overlap) == offsetof(jb_mix_report, overlap),
              "jb_mix.h restates the header's report");

int mix_layout_checked(const MixUtt *req, bool chained, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem,
                       const MixOpts *opts, MixLayout *out, const char *who)
{
    auto refuse = [&](const std::string &what) {
        set_error(std::string(who) + ": " + what);
        return JB_ERR_INVALID;
    };
    if (opts) {
        if (opts->flags & ~kMixFit)
            return refuse("flags holds an unknown flag");
        if (opts->reserved)
            return refuse("reserved must be 0 (the options)");
        if ((opts->flags & kMixFit) && !(opts->ceiling_db >= kMixMinCeilingDb && opts->ceiling_db <= 0.0))
            return refuse("ceiling_db is finite, in [-120, 0]"); // (a NaN fails every comparison)
    }
    for (size_t u = 0; u < B; u++) {
        if (req[u].reserved || req[u].reserved2)
            return refuse("reserved must be 0 (utterance " + std::to_string(u) + ")");
        const double db = req[u].gain_db;
        if (!(db == -INFINITY || (db >= kMixMinDb && db <= kMixMaxDb)))
            return refuse("gain_db is in [-120, 40], or -INFINITY (utterance " + std::to_string(u) + ")");
    }
    uint32_t bad = 0;
    const char *field = "";
    if (!mix_layout(req, n, hz, B, elem, out, &bad, &field, chained)) {
        const std::string f = field;
        if (f == "programme id")
            return refuse("programme id " + std::to_string(bad) + " (an id is below the batch size, or " +
                          (chained ? "JB_JOIN_NONE)" : "JB_MIX_NONE)"));
        if (f == "length")
            return refuse(std::string(chained ? "the members in front + pad_before + " : "start + ") +
                          "samples + pad_after is too long (utterance " + std::to_string(bad) + ")");
        if (f == "slab length")
            return refuse("the programmes up to programme " + std::to_string(bad) + " are too long together");
        if (f == "work lists") {
            set_error(std::string(who) + ": the segments' member lists pass 2^24 entries (programme " +
                      std::to_string(bad) + ")");
            return JB_ERR_UNSUPPORTED;
        }
        return refuse("the members of programme " + std::to_string(bad) + " would disagree on the " + f);
    }
    return JB_OK;
}

void mix_lists(const MixLayout &lay, const MixUtt *req, const uint64_t *n, const uint64_t *xoff, const void *x, void *y,
               size_t elem, std::vector<ProgMember> *members, std::vector<ProgSpan> *spans, uint64_t *tiles)
{
    const size_t B = lay.start.size(), P = lay.units.size();
    members->assign(B, ProgMember{});
    spans->assign(P, ProgSpan{});
    *tiles = 0;
    for (size_t p = 0; p < P; p++) {
        const uint32_t m0 = lay.progs.first[p], m1 = lay.progs.first[p + 1];
        for (uint32_t i = m0; i < m1; i++) {
            const uint32_t u = lay.progs.members[i];
            (*members)[i] = {(const char *)x + xoff[u] * elem, lay.start[u], n[u], req[u].fade_in, req[u].fade_out,
                             lay.gain[u]};
        }
        ProgSpan &w = (*spans)[p];
        w.y = (char *)y + lay.units[p].off * elem;
        w.n = w.k1 = lay.units[p].n;
        w.t0 = w.pk0 = *tiles;
        w.m0 = m0;
        w.nm = m1 - m0;
        w.s0 = lay.seg_first[p];
        w.ns = lay.seg_first[p + 1] - lay.seg_first[p];
        w.prog = (uint32_t)p;
        *tiles += prog_tiles(0, w.n, elem == 2);
    }
}

namespace {

template <class T>
int mix_host(const T *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req, const jb_mix_opts *opts,
             const double *scale, T *const *out, const size_t *cap, jb_mix_report *reports, const char *who)
{
    if (n && (!in || !n_in || !req || !out || !cap))
        return JB_ERR_INVALID;
    for (size_t u = 0; u < n; u++)
        if (n_in[u] && !in[u])
            return JB_ERR_INVALID;
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    int rc = mix_layout_checked((const MixUtt *)req, false, ns.data(), nullptr, n, sizeof(T), (const MixOpts *)opts, &lay,
                                who);
    if (rc)
        return rc;
    const size_t P = lay.units.size();
    for (size_t p = 0; p < P; p++) {
        if (cap[p] < lay.units[p].n) {
            set_error(std::string(who) + ": the buffer is too small");
            return JB_ERR_BUFFER;
        }
        if (lay.units[p].n && !out[p])
            return JB_ERR_INVALID;
    }
    const bool fit = opts && (opts->flags & kMixFit);
    const double c = fit ? mix_ceiling(opts->ceiling_db) : 0.0;
    std::vector<double> acc;
    std::vector<uint8_t> have;
    for (size_t p = 0; p < P; p++) {
        const uint64_t N = lay.units[p].n;
        acc.assign(N, 0.0);
        have.assign(N, 0);
        // member after member in ascending utterance index: at every sample the terms meet in that order
        for (uint32_t i = lay.progs.first[p]; i < lay.progs.first[p + 1]; i++) {
            const uint32_t u = lay.progs.members[i];
            const double g = lay.gain[u];
            if (g == 0.0)
                continue;
            for (uint64_t j = 0; j < n_in[u]; j++) {
                const uint64_t k = lay.start[u] + j;
                const double t = mix_term((double)in[u][j], j, n_in[u], req[u].fade_in, req[u].fade_out, g);
                acc[k] = have[k] ? acc[k] + t : t;
                have[k] = 1;
            }
        }
        double M = 0.0;
        for (uint64_t k = 0; k < N; k++)
            M = fmax(M, fabs(acc[k]));
        const double s = scale ? scale[p] : fit ? mix_scale(M, c) : 1.0;
        for (uint64_t k = 0; k < N; k++)
            mix_store(fit && s != 1.0 ? mix_fit(acc[k], s, c) : acc[k], out[p] + k);
        if (reports)
            reports[p] = {M, s, lay.depth[p], 0, lay.overlap[p]};
    }
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

double jb_mix_gain(double gain_db) { return mix_gain(gain_db); }

int jb_mix_geometry(const jb_mix_utt *req, const size_t *n_in, const uint32_t *hz, size_t n, const jb_mix_opts *opts,
                    uint32_t *programme_of, uint64_t *member_start, size_t *n_programmes, uint64_t *programme_samples,
                    uint32_t *depth, uint64_t *overlap)
{
    if (n && (!req || !n_in))
        return JB_ERR_INVALID;
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    int rc = mix_layout_checked((const MixUtt *)req, false, ns.data(), hz, n, sizeof(double), (const MixOpts *)opts,
                                &lay, "jb_mix_geometry");
    if (rc)
        return rc;
    for (size_t u = 0; u < n; u++) {
        if (programme_of)
            programme_of[u] = lay.progs.group_of[u];
        if (member_start)
            member_start[u] = lay.start[u];
    }
    if (n_programmes)
        *n_programmes = lay.units.size();
    for (size_t p = 0; p < lay.units.size(); p++) {
        if (programme_samples)
            programme_samples[p] = lay.units[p].n;
        if (depth)
            depth[p] = lay.depth[p];
        if (overlap)
            overlap[p] = lay.overlap[p];
    }
    return JB_OK;
}

int jb_mix_host(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req, const jb_mix_opts *opts,
                const double *scale, double *const *out, const size_t *cap, jb_mix_report *reports)
{
    return mix_host(in, n_in, n, req, opts, scale, out, cap, reports, "jb_mix_host");
}

int jb_mix_i16_host(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                    const jb_mix_opts *opts, const double *scale, int16_t *const *out, const size_t *cap,
                    jb_mix_report *reports)
{
    return mix_host(in, n_in, n, req, opts, scale, out, cap, reports, "jb_mix_i16_host");
}

void jb_mix_free(void *p) { free(p); }

} // extern "C"

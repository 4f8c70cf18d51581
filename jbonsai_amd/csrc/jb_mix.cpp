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
static_assert(kMixNoStem == JB_MIX_NO_STEM && kMixStemLevels == JB_MIX_STEM_LEVELS, "jb_mix.h restates the stems' words");
static_assert(sizeof(MixReport) == sizeof(jb_mix_report) && offsetof(MixReport, scale) == offsetof(jb_mix_report, scale) &&
                  offsetof(MixReport, depth) == offsetof(jb_mix_report, depth) &&
                  offsetof(MixReport, overlap) == offsetof(jb_mix_report, overlap),
              "jb_mix.h restates the header's report");

int mix_layout_checked(const MixUtt *req, bool chained, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem,
                       const MixOpts *opts, MixLayout *out, const char *who, const uint32_t *stem_of)
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
    if (stem_of && chained)
        return refuse("stems stand behind a mix request, not behind a join");
    uint32_t bad = 0;
    const char *field = "";
    if (!mix_layout(req, n, hz, B, elem, out, &bad, &field, chained, stem_of)) {
        const std::string f = field;
        if (f == "stem id")
            return refuse("stem_of of utterance " + std::to_string(bad) + " (" + std::to_string(stem_of[bad]) +
                          "): a stem id is below the batch size, or JB_MIX_NO_STEM");
        if (f == "programme id")
            return refuse("programme id " + std::to_string(bad) + " (an id is below the batch size, or " +
                          (chained ? "JB_JOIN_NONE)" : "JB_MIX_NONE)"));
        if (f == "length")
            return refuse(std::string(chained ? "the members in front + pad_before + " : "start + ") +
                          "samples + pad_after is too long (utterance " + std::to_string(bad) + ")");
        if (f == "slab length")
            return refuse("the programmes" + std::string(stem_of ? " and stems up to unit " : " up to programme ") +
                          std::to_string(bad) + " are too long together");
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
    const size_t B = lay.start.size(), P = lay.programmes(), U = lay.units.size();
    members->assign(B, ProgMember{});
    spans->assign(U, ProgSpan{});
    *tiles = 0;
    for (size_t p = 0; p < U; p++) {
        // (a stem: its programme's members, segments of its own)
        const size_t parent = p < P ? p : lay.stems[p - P].programme;
        const uint32_t m0 = lay.progs.first[parent], m1 = lay.progs.first[parent + 1];
        for (uint32_t i = m0; i < m1 && p < P; i++) {
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
        w.parent = (uint32_t)parent;
        *tiles += prog_tiles(0, w.n, elem == 2);
    }
}

void mix_level_items(const MixLayout &lay, const void *y, size_t elem, const std::vector<uint8_t> &mask,
                     std::vector<LevelItem> *items, uint64_t *tiles, uint64_t *scratch)
{
    const size_t P = lay.programmes(), U = lay.units.size();
    items->clear();
    *tiles = 0;
    uint64_t s0 = 0;
    std::vector<uint8_t> asked(P, 0); // a programme without a stem has no E_p anyone reads: no item
    for (const MixStem &st : lay.stems)
        asked[st.programme] = 1;
    for (size_t p = 0; p < U; p++) {
        const size_t parent = p < P ? p : lay.stems[p - P].programme;
        if (p < P && !asked[p])
            continue;
        LevelItem it{};
        it.a = (const char *)y + lay.units[p].off * elem;
        it.m = (const char *)y + lay.units[parent].off * elem;
        it.n = lay.units[p].n;
        it.nt = p < P ? level_tiles(it.n) : level_extent_tiles(lay.stems[p - P].first, lay.stems[p - P].end, &it.tile0);
        it.s0 = s0;
        it.unit = (uint32_t)p;
        it.self = p < P;
        s0 += it.nt;
        if (!mask.empty() && !mask[p])
            continue;
        it.t0 = *tiles;
        *tiles += it.nt;
        items->push_back(it);
    }
    if (scratch)
        *scratch = s0;
}

namespace {

// (with stem_of: the P + S units of the stems request, out and cap of as many entries, stem_reports [S])
template <class T>
int mix_host(const T *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req, const jb_mix_opts *opts,
             const double *scale, T *const *out, const size_t *cap, jb_mix_report *reports, const char *who,
             const uint32_t *stem_of = nullptr, uint32_t stem_flags = 0, jb_stem_report *stem_reports = nullptr)
{
    if (n && (!in || !n_in || !req || !out || !cap))
        return JB_ERR_INVALID;
    for (size_t u = 0; u < n; u++)
        if (n_in[u] && !in[u])
            return JB_ERR_INVALID;
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    if (stem_flags & ~kMixStemLevels) {
        set_error(std::string(who) + ": flags holds an unknown flag");
        return JB_ERR_INVALID;
    }
    int rc = mix_layout_checked((const MixUtt *)req, false, ns.data(), nullptr, n, sizeof(T), (const MixOpts *)opts, &lay,
                                who, stem_of);
    if (rc)
        return rc;
    const size_t P = lay.programmes(), U = lay.units.size();
    for (size_t p = 0; p < U; p++) {
        if (cap[p] < lay.units[p].n) {
            set_error(std::string(who) + ": the buffer is too small");
            return JB_ERR_BUFFER;
        }
        if (lay.units[p].n && !out[p])
            return JB_ERR_INVALID;
    }
    const bool fit = opts && (opts->flags & kMixFit);
    const double c = fit ? mix_ceiling(opts->ceiling_db) : 0.0;
    std::vector<double> acc, scales(P, 1.0);
    std::vector<uint8_t> have;
    for (size_t p = 0; p < U; p++) {
        const uint64_t N = lay.units[p].n;
        const size_t parent = p < P ? p : lay.stems[p - P].programme;
        acc.assign(N, 0.0);
        have.assign(N, 0);
        // member after member in ascending utterance index: at every sample the terms meet in that order (a stem: its
        // own members alone)
        for (uint32_t i = lay.progs.first[parent]; i < lay.progs.first[parent + 1]; i++) {
            const uint32_t u = lay.progs.members[i];
            const double g = lay.gain[u];
            if (g == 0.0 || (p >= P && (size_t)lay.stem_unit[u] != p))
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
        if (p >= P) { // a stem: its programme's scale, no clamp
            const double s = scales[parent];
            for (uint64_t k = 0; k < N; k++)
                mix_store(fit && s != 1.0 ? mix_stem_fit(acc[k], s) : acc[k], out[p] + k);
            if (stem_reports) {
                const bool levels = (stem_flags & kMixStemLevels) != 0;
                MixSums own{};
                double e_p = 0.0;
                if (levels) {
                    const MixStem &st = lay.stems[p - P];
                    uint64_t t0 = 0;
                    const uint64_t nt = level_extent_tiles(st.first, st.end, &t0);
                    own.e = level_sum_host(out[p], out[p], N, t0, nt);
                    own.d = level_sum_host(out[p], out[parent], N, t0, nt);
                    e_p = level_sum_host(out[parent], out[parent], N, 0, level_tiles(N));
                }
                stem_reports[p - P] = stem_report_of(M, s, levels, own, e_p);
            }
            continue;
        }
        const double s = scale ? scale[p] : fit ? mix_scale(M, c) : 1.0;
        scales[p] = s;
        for (uint64_t k = 0; k < N; k++)
            mix_store(fit && s != 1.0 ? mix_fit(acc[k], s, c) : acc[k], out[p] + k);
        if (reports)
            reports[p] = {M, s, lay.depth[p], 0, lay.overlap[p]};
    }
    return JB_OK;
}

template <class T>
int levels_host(const T *stem, const T *mix, size_t n, uint64_t first, uint64_t end, double *e_s, double *d, double *e_p,
                const char *who)
{
    if ((n && (!stem || !mix)) || first > end || end > n) {
        set_error(std::string(who) + ": needs both signals and first_sample <= end_sample <= n");
        return JB_ERR_INVALID;
    }
    uint64_t t0 = 0;
    const uint64_t nt = level_extent_tiles(first, end, &t0);
    if (e_s)
        *e_s = level_sum_host(stem, stem, n, t0, nt);
    if (d)
        *d = level_sum_host(stem, mix, n, t0, nt);
    if (e_p)
        *e_p = level_sum_host(mix, mix, n, 0, level_tiles(n));
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

int jb_mix_stems_geometry(const jb_mix_utt *req, const uint32_t *stem_of, const size_t *n_in, const uint32_t *hz, size_t n,
                          const jb_mix_opts *opts, size_t *n_programmes, size_t *n_units, int64_t *stem_unit,
                          uint64_t *unit_samples, uint32_t *unit_programme, uint32_t *unit_stem_id,
                          uint32_t *unit_members, uint64_t *unit_first, uint64_t *unit_end, uint32_t *unit_depth)
{
    if (n && (!req || !n_in || !stem_of))
        return JB_ERR_INVALID;
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    int rc = mix_layout_checked((const MixUtt *)req, false, ns.data(), hz, n, sizeof(double), (const MixOpts *)opts,
                                &lay, "jb_mix_stems_geometry", stem_of);
    if (rc)
        return rc;
    const size_t P = lay.programmes(), U = lay.units.size();
    if (n_programmes)
        *n_programmes = P;
    if (n_units)
        *n_units = U;
    for (size_t u = 0; u < n && stem_unit; u++)
        stem_unit[u] = lay.stem_unit[u];
    for (size_t p = 0; p < U; p++) {
        const MixStem st = p < P ? MixStem{(uint32_t)p, kMixNoStem, lay.progs.first[p + 1] - lay.progs.first[p], 0, 0,
                                           lay.units[p].n}
                                 : lay.stems[p - P];
        if (unit_samples)
            unit_samples[p] = lay.units[p].n;
        if (unit_programme)
            unit_programme[p] = st.programme;
        if (unit_stem_id)
            unit_stem_id[p] = st.id;
        if (unit_members)
            unit_members[p] = st.n_members;
        if (unit_first)
            unit_first[p] = st.first;
        if (unit_end)
            unit_end[p] = st.end;
        if (unit_depth)
            unit_depth[p] = lay.depth[p];
    }
    return JB_OK;
}

int jb_mix_stems_host(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                      const uint32_t *stem_of, uint32_t flags, const jb_mix_opts *opts, const double *scale,
                      double *const *out, const size_t *cap, jb_mix_report *reports, jb_stem_report *stem_reports)
{
    if (n && !stem_of)
        return JB_ERR_INVALID;
    return mix_host(in, n_in, n, req, opts, scale, out, cap, reports, "jb_mix_stems_host", stem_of, flags, stem_reports);
}

int jb_mix_stems_i16_host(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                          const uint32_t *stem_of, uint32_t flags, const jb_mix_opts *opts, const double *scale,
                          int16_t *const *out, const size_t *cap, jb_mix_report *reports, jb_stem_report *stem_reports)
{
    if (n && !stem_of)
        return JB_ERR_INVALID;
    return mix_host(in, n_in, n, req, opts, scale, out, cap, reports, "jb_mix_stems_i16_host", stem_of, flags,
                    stem_reports);
}

int jb_mix_levels_host(const double *stem, const double *mix, size_t n, uint64_t first_sample, uint64_t end_sample,
                       double *e_s, double *d, double *e_p)
{
    return levels_host(stem, mix, n, first_sample, end_sample, e_s, d, e_p, "jb_mix_levels_host");
}

int jb_mix_levels_i16_host(const int16_t *stem, const int16_t *mix, size_t n, uint64_t first_sample,
                           uint64_t end_sample, double *e_s, double *d, double *e_p)
{
    return levels_host(stem, mix, n, first_sample, end_sample, e_s, d, e_p, "jb_mix_levels_i16_host");
}

void jb_mix_levels_db(double e_s, double d, double e_p, double *level_db, double *sir_db, double *si_sdr_db)
{
    double a, b, c;
    level_db_of(e_s, d, e_p, &a, &b, &c);
    if (level_db)
        *level_db = a;
    if (sir_db)
        *sir_db = b;
    if (si_sdr_db)
        *si_sdr_db = c;
}

} // extern "C"

// jb_activity.cpp -- the host half of the speech-activity stage: the request check, the geometry, the layout's refusals
// and the rule of jb_activity.h over PCM the caller holds without a GPU (jb_activity_host and jb_activity_members_host,
// what the kernels are checked against).  The smoothing steps here walk the bytes frame by frame; the kernel's packed
// form (act_close_word and its kin) is not used.
#include "jb_host.h"

#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(ActOpts) == sizeof(jb_activity_opts) && offsetof(ActOpts, win_us) == offsetof(jb_activity_opts, win_us) &&
                  offsetof(ActOpts, hop_us) == offsetof(jb_activity_opts, hop_us) &&
                  offsetof(ActOpts, gate_db) == offsetof(jb_activity_opts, gate_db) &&
                  offsetof(ActOpts, grid) == offsetof(jb_activity_opts, grid) &&
                  offsetof(ActOpts, reference) == offsetof(jb_activity_opts, reference) &&
                  offsetof(ActOpts, columns) == offsetof(jb_activity_opts, columns) &&
                  offsetof(ActOpts, flags) == offsetof(jb_activity_opts, flags) &&
                  offsetof(ActOpts, min_speech) == offsetof(jb_activity_opts, min_speech) &&
                  offsetof(ActOpts, min_gap) == offsetof(jb_activity_opts, min_gap) &&
                  offsetof(ActOpts, hang_before) == offsetof(jb_activity_opts, hang_before) &&
                  offsetof(ActOpts, hang_after) == offsetof(jb_activity_opts, hang_after) &&
                  offsetof(ActOpts, reserved) == offsetof(jb_activity_opts, reserved),
              "jb_activity.h restates the header's options");
static_assert(kActSnip == JB_ACTIVITY_SNIP && kActCenter == JB_ACTIVITY_CENTER && kActKaldi == JB_ACTIVITY_KALDI &&
                  kActStft == JB_ACTIVITY_STFT && kActRefPeak == JB_ACTIVITY_REF_PEAK && kActRefAbs == JB_ACTIVITY_REF_ABS &&
                  kActMembers == JB_ACTIVITY_MEMBERS && kActUnit == JB_ACTIVITY_UNIT && kActSamples == JB_ACTIVITY_SAMPLES &&
                  kActMaxCells == JB_ACTIVITY_MAX_CELLS,
              "jb_activity.h restates the header's constants");
static_assert(sizeof(ActReport) == sizeof(jb_activity_report) && offsetof(ActReport, first) == offsetof(jb_activity_report, first) &&
                  offsetof(ActReport, last) == offsetof(jb_activity_report, last) &&
                  offsetof(ActReport, peak) == offsetof(jb_activity_report, peak) &&
                  offsetof(ActReport, thr) == offsetof(jb_activity_report, thr),
              "jb_activity.h restates the header's column report");
static_assert(sizeof(ActUnitReport) == sizeof(jb_activity_unit_report) &&
                  offsetof(ActUnitReport, none) == offsetof(jb_activity_unit_report, none) &&
                  offsetof(ActUnitReport, one) == offsetof(jb_activity_unit_report, one) &&
                  offsetof(ActUnitReport, many) == offsetof(jb_activity_unit_report, many),
              "jb_activity.h restates the header's unit report");

int act_check_opts(const ActOpts *opts, const char *who)
{
    if (!opts) {
        set_error(std::string(who) + ": opts is NULL");
        return JB_ERR_INVALID;
    }
    if (const char *f = act_opts_fault(*opts)) {
        set_error(std::string(who) + ": " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

int act_layout_checked(const ActOpts &o, size_t P, const uint64_t *unit_n, const uint32_t *unit_hz, const uint32_t *first,
                       const uint32_t *members, const uint64_t *start, const uint64_t *n, const double *gain,
                       ActLayout *out, const char *who)
{
    size_t unit = 0;
    bool unsupported = false;
    const char *f = act_layout(o, P, unit_n, unit_hz, first, members, start, n, gain, out, &unit, &unsupported);
    if (!f)
        return JB_OK;
    const bool whole = act_opts_fault(o) != nullptr; // the options on their own: no unit to name
    set_error(std::string(who) + ": " + f + (whole ? "" : " (unit " + std::to_string(unit) + ")"));
    return unsupported ? JB_ERR_UNSUPPORTED : JB_ERR_INVALID;
}

namespace {

// The energies of one column over the T frames of its unit: the source x[0..n) at `start`, 0 everywhere else
void act_energies(const double *x, uint64_t start, uint64_t n, uint32_t grid, uint64_t T, uint32_t wl, uint32_t hop,
                  std::vector<double> *E)
{
    E->assign(T, 0.0);
    uint64_t f0, nf;
    act_span(grid, T, wl, hop, start, n, &f0, &nf);
    for (uint64_t t = f0; t < f0 + nf; t++) {
        const int64_t s = act_start(grid, t, wl, hop) - (int64_t)start;
        (*E)[t] = frame_sum(wl, [&](uint32_t i) {
            const int64_t k = s + (int64_t)i;
            const double v = k >= 0 && (uint64_t)k < n ? x[k] : 0.0;
            return v * v;
        });
    }
}

// Gate and smoothing of one column: r[T] from E[T]; the report's peak and thr
void act_column(const std::vector<double> &E, const ActOpts &o, uint32_t wl, std::vector<uint8_t> *r, ActReport *rep)
{
    const int64_t T = (int64_t)E.size();
    double peak = 0.0;
    for (int64_t t = 0; t < T; t++)
        if (E[t] > peak)
            peak = E[t];
    const double thr = act_threshold(o.reference == kActRefAbs, act_ratio(o.gate_db), act_abs_threshold(o.gate_db, wl), peak);
    r->assign(T, 0);
    for (int64_t t = 0; t < T; t++)
        (*r)[t] = act_raw(E[t], thr);
    std::vector<uint8_t> &b = *r;
    if (o.min_gap) { // close: between two raw-active frames a < c, c the next one behind a
        int64_t a = -1;
        for (int64_t c = 0; c < T; c++) {
            if (b[c] != 1)
                continue;
            if (a >= 0 && c - a - 1 >= 1 && c - a - 1 <= (int64_t)o.min_gap)
                for (int64_t t = a + 1; t < c; t++)
                    b[t] = 2; // (marked: only raw-active frames bound a gap)
            a = c;
        }
        for (int64_t t = 0; t < T; t++)
            b[t] = b[t] != 0;
    }
    if (o.min_speech > 1) { // open: runs shorter than min_speech go
        for (int64_t t = 0; t < T;) {
            if (!b[t]) {
                t++;
                continue;
            }
            int64_t e = t;
            while (e < T && b[e])
                e++;
            if (e - t < (int64_t)o.min_speech)
                for (int64_t k = t; k < e; k++)
                    b[k] = 0;
            t = e;
        }
    }
    if (o.hang_before || o.hang_after) { // hang: around every surviving frame
        std::vector<uint8_t> h(T, 0);
        int64_t last = -1;
        for (int64_t t = 0; t < T; t++) {
            if (b[t])
                last = t;
            if (last >= 0 && t - last <= (int64_t)o.hang_after)
                h[t] = 1;
        }
        int64_t next = -1;
        for (int64_t t = T - 1; t >= 0; t--) {
            if (b[t])
                next = t;
            if (next >= 0 && next - t <= (int64_t)o.hang_before)
                h[t] = 1;
        }
        b.swap(h);
    }
    if (rep) {
        *rep = ActReport{0, (uint64_t)T, (uint64_t)T, peak, thr};
        for (int64_t t = 0; t < T; t++)
            if (b[t]) {
                if (!rep->active)
                    rep->first = (uint64_t)t;
                rep->last = (uint64_t)t;
                rep->active++;
            }
    }
}

int act_geometry_checked(const ActOpts *o, uint32_t hz, const char *who, uint32_t *wl, uint32_t *hop)
{
    const int rc = act_check_opts(o, who);
    if (rc)
        return rc;
    if (const char *f = act_geometry_fault(*o, hz, wl, hop)) {
        set_error(std::string(who) + ": " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_activity_geometry(const jb_activity_opts *opts, uint32_t hz, size_t n, uint32_t *wl, uint32_t *hop, uint64_t *T)
{
    uint32_t w = 0, h = 0;
    const int rc = act_geometry_checked((const ActOpts *)opts, hz, "jb_activity_geometry", &w, &h);
    if (rc)
        return rc;
    if (wl)
        *wl = w;
    if (hop)
        *hop = h;
    if (T)
        *T = act_frames(opts->grid, n, w, h);
    return JB_OK;
}

int jb_activity_host(const double *x, size_t n, uint32_t hz, const jb_activity_opts *opts, uint8_t *out, size_t cap,
                     jb_activity_report *report)
{
    const char *who = "jb_activity_host";
    const ActOpts *o = (const ActOpts *)opts;
    uint32_t wl = 0, hop = 0;
    const int rc = act_geometry_checked(o, hz, who, &wl, &hop);
    if (rc)
        return rc;
    if (n && !x)
        return JB_ERR_INVALID;
    const uint64_t T = act_frames(o->grid, n, wl, hop);
    if (T > kActMaxCells) {
        set_error(std::string(who) + ": T passes JB_ACTIVITY_MAX_CELLS");
        return JB_ERR_UNSUPPORTED;
    }
    if (cap < T || (T && !out)) {
        set_error(std::string(who) + ": the buffer is too small");
        return JB_ERR_BUFFER;
    }
    std::vector<double> E;
    std::vector<uint8_t> r;
    act_energies(x, 0, n, o->grid, T, wl, hop, &E);
    act_column(E, *o, wl, &r, (ActReport *)report);
    if (T)
        memcpy(out, r.data(), T);
    return JB_OK;
}

int jb_activity_members_host(const double *const *in, const size_t *n_in, const uint64_t *start, const double *gain_db,
                             size_t m, uint64_t n_unit, uint32_t hz, const jb_activity_opts *opts, uint8_t *out,
                             size_t cap, jb_activity_report *cols, jb_activity_unit_report *unit)
{
    const char *who = "jb_activity_members_host";
    const ActOpts *o = (const ActOpts *)opts;
    uint32_t wl = 0, hop = 0;
    const int rc = act_geometry_checked(o, hz, who, &wl, &hop);
    if (rc)
        return rc;
    if (o->columns != kActMembers) {
        set_error(std::string(who) + ": columns must be JB_ACTIVITY_MEMBERS");
        return JB_ERR_INVALID;
    }
    if (m == 0 || !in || !n_in || !start)
        return JB_ERR_INVALID;
    for (size_t j = 0; j < m; j++) {
        if (n_in[j] && !in[j])
            return JB_ERR_INVALID;
        if (start[j] > n_unit || n_in[j] > n_unit - start[j]) {
            set_error(std::string(who) + ": start + samples passes the unit (member " + std::to_string(j) + ")");
            return JB_ERR_INVALID;
        }
    }
    const uint64_t T = act_frames(o->grid, n_unit, wl, hop);
    if (T > kActMaxCells / m) {
        set_error(std::string(who) + ": T * C of a unit passes JB_ACTIVITY_MAX_CELLS (take JB_ACTIVITY_UNIT)");
        return JB_ERR_UNSUPPORTED;
    }
    if (cap < T * m || (T && !out)) {
        set_error(std::string(who) + ": the buffer is too small");
        return JB_ERR_BUFFER;
    }
    std::vector<double> E;
    std::vector<uint8_t> r;
    for (size_t j = 0; j < m; j++) {
        const bool muted = gain_db && gain_db[j] == -INFINITY;
        act_energies(in[j], start[j], muted ? 0 : n_in[j], o->grid, T, wl, hop, &E);
        act_column(E, *o, wl, &r, cols ? (ActReport *)cols + j : nullptr);
        for (uint64_t t = 0; t < T; t++)
            out[t * m + j] = r[t];
    }
    if (unit) {
        *unit = jb_activity_unit_report{T, 0, 0, 0};
        for (uint64_t t = 0; t < T; t++) {
            uint64_t k = 0;
            for (size_t j = 0; j < m; j++)
                k += out[t * m + j];
            (k == 0 ? unit->none : k == 1 ? unit->one : unit->many)++;
        }
    }
    return JB_OK;
}

void jb_activity_free(void *p) { free(p); }

} // extern "C"

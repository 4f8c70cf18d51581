// jb_output_chain.cpp -- OutputChain (jb_host.h): the stages behind the vocoder of one batch.  The setters record a
// request and plan again (plan_output, jb_output.h); prepare() carries the plan out once; enqueue() launches
// k_resample, the filter, the loudness measurement and apply pass, the join, the FLAC encoder and pack, the sample format and IMA
// ADPCM, in that order, on the vocoder's stream.
#include "jb_host.h"

#include <algorithm>
#include <new>
#include <string>

namespace jb {

void OutputChain::init()
{
    slab[(size_t)OutSlab::V64] = b.vd.pcm;
    slab[(size_t)OutSlab::S16] = b.vd.pcm16;
    replan();
}

void OutputChain::replan()
{
    const size_t B = (size_t)b.B;
    std::vector<uint64_t> n(B), off(B);
    for (size_t u = 0; u < B; u++) {
        n[u] = (uint64_t)b.T[u] * b.voice.fperiod;
        off[u] = b.frame_off[u] * b.voice.fperiod;
    }
    OutPlanIn in;
    in.B = B;
    in.n_native = n.data();
    in.off_native = off.data();
    in.voice_hz = b.voice.sampling_frequency;
    in.i16 = (b.flags & JB_BATCH_PCM_I16) != 0;
    in.want_hz = want_hz.empty() ? nullptr : want_hz.data();
    in.loudness = ln_on;
    in.flac = flac_on;
    in.fmt_bytes = fmt_on ? (uint32_t)format_bytes(fmt_p.format) : 0;
    in.adpcm = ad_on;
    in.adpcm_align = ad_align;
    in.join = join_req.empty() ? nullptr : join_req.data();
    in.filter = filt_any.empty() ? nullptr : filt_any.data();
    plan = plan_output(in);
}

// what every setter refuses
int OutputChain::check_settable(const char *after_run) const
{
    if (b.flags & JB_BATCH_MLPG_ONLY) {
        set_error("a JB_BATCH_MLPG_ONLY batch has no PCM");
        return JB_ERR_INVALID;
    }
    if (frozen) {
        set_error(after_run);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

int OutputChain::set_output_rate(const uint32_t *hz, size_t n)
{
    int rc = check_settable("jb_batch_set_output_rate: the output rate is set before the batch's first run");
    if (rc)
        return rc;
    if (!hz || (n != 1 && n != (size_t)b.B)) {
        set_error("jb_batch_set_output_rate: give one rate, or one per utterance");
        return JB_ERR_INVALID;
    }
    const uint32_t in = b.voice.sampling_frequency;
    std::vector<uint32_t> want((size_t)b.B);
    for (size_t u = 0; u < want.size(); u++) {
        const uint32_t h = hz[n == 1 ? 0 : u];
        want[u] = h == in ? 0 : h;
        if (want[u] && (rc = resample_design(in, want[u], nullptr, nullptr)))
            return rc;
    }
    if ((rc = check_groups(ln_group_req, ln_target, ln_ceiling, ln_mode, want, "jb_batch_set_output_rate", nullptr)) ||
        (rc = check_join(join_req, want, "jb_batch_set_output_rate")) ||
        (rc = check_filter(filt_req, want, "jb_batch_set_output_rate")))
        return rc;
    want_hz = std::move(want);
    replan();
    return JB_OK;
}

// The combined request: the groups of `group` under these targets, ceilings, modes and rates (each empty: not set)
int OutputChain::check_groups(const std::vector<uint32_t> &group, const std::vector<double> &target,
                              const std::vector<double> &ceiling, const std::vector<uint32_t> &mode,
                              const std::vector<uint32_t> &want, const char *who, LnGroups *out) const
{
    if (group.empty())
        return JB_OK;
    const size_t B = (size_t)b.B;
    std::vector<uint32_t> hz(B, b.voice.sampling_frequency);
    for (size_t u = 0; u < want.size(); u++)
        if (want[u])
            hz[u] = want[u];
    LnGroupsIn in;
    in.B = B;
    in.group = group.data();
    in.target = target.empty() ? nullptr : target.data();
    in.ceiling = ceiling.empty() ? nullptr : ceiling.data();
    in.mode = mode.empty() ? nullptr : mode.data();
    in.hz = hz.data();
    LnGroups plan;
    uint32_t bad = 0;
    const char *field = "";
    if (!plan_loudness_groups(in, &plan, &bad, &field)) {
        if (std::string(field) == "group id")
            set_error(std::string(who) + ": group id " + std::to_string(bad) +
                      " (an id is below the batch size, or JB_LOUDNESS_NO_GROUP)");
        else
            set_error(std::string(who) + ": the members of loudness group " + std::to_string(bad) +
                      " would disagree on the " + field);
        return JB_ERR_INVALID;
    }
    if (out)
        *out = std::move(plan);
    return JB_OK;
}

int OutputChain::set_loudness_groups(const uint32_t *group, size_t n)
{
    int rc = check_settable("jb_batch_set_loudness_groups: the groups are set before the batch's first run");
    if (rc)
        return rc;
    if (!group && n == 0) {
        ln_group_req.clear();
        ln_groups = LnGroups{};
        return JB_OK;
    }
    if (!group || n != (size_t)b.B) {
        set_error("jb_batch_set_loudness_groups: give one group per utterance");
        return JB_ERR_INVALID;
    }
    std::vector<uint32_t> req(group, group + n);
    LnGroups plan;
    if ((rc = check_groups(req, ln_target, ln_ceiling, ln_mode, want_hz, "jb_batch_set_loudness_groups", &plan)))
        return rc;
    if (req.empty()) // (an empty batch: nothing to group)
        return JB_OK;
    ln_group_req = std::move(req);
    ln_groups = std::move(plan);
    return JB_OK;
}

int OutputChain::set_loudness_report(uint32_t flags)
{
    int rc = check_settable("jb_batch_set_loudness_report: the report is set before the batch's first run");
    if (rc)
        return rc;
    if (flags & ~(uint32_t)JB_LOUDNESS_R128) {
        set_error("jb_batch_set_loudness_report: flags are JB_LOUDNESS_R128 or 0");
        return JB_ERR_INVALID;
    }
    ln_report = flags;
    return JB_OK;
}

int OutputChain::set_loudness(const double *target, const double *ceiling, size_t n)
{
    int rc = check_settable("jb_batch_set_loudness_target: the target is set before the batch's first run");
    if (rc)
        return rc;
    if (!target || !ceiling || (n != 1 && n != (size_t)b.B)) {
        set_error("jb_batch_set_loudness_target: give one target, or one per utterance");
        return JB_ERR_INVALID;
    }
    std::vector<double> t((size_t)b.B, 0.0), c((size_t)b.B, 0.0);
    for (size_t u = 0; u < (size_t)b.B; u++) {
        t[u] = target[n == 1 ? 0 : u];
        c[u] = ceiling[n == 1 ? 0 : u];
    }
    if ((rc = check_groups(ln_group_req, t, c, ln_mode, want_hz, "jb_batch_set_loudness_target", nullptr)))
        return rc;
    ln_target = std::move(t);
    ln_ceiling = std::move(c);
    ln_on = true;
    replan();
    return JB_OK;
}

// The mode is kept with or without a target (either order); it takes effect where a target makes the chain measure
int OutputChain::set_peak_mode(const uint32_t *mode, size_t n)
{
    int rc = check_settable("jb_batch_set_peak_mode: the peak mode is set before the batch's first run");
    if (rc)
        return rc;
    if (!mode || (n != 1 && n != (size_t)b.B)) {
        set_error("jb_batch_set_peak_mode: give one mode, or one per utterance");
        return JB_ERR_INVALID;
    }
    for (size_t u = 0; u < n; u++)
        if (mode[u] != JB_PEAK_SAMPLE && mode[u] != JB_PEAK_TRUE) {
            set_error("jb_batch_set_peak_mode: a mode is JB_PEAK_SAMPLE or JB_PEAK_TRUE");
            return JB_ERR_INVALID;
        }
    std::vector<uint32_t> m((size_t)b.B, JB_PEAK_SAMPLE);
    for (size_t u = 0; u < (size_t)b.B; u++)
        m[u] = mode[n == 1 ? 0 : u];
    if ((rc = check_groups(ln_group_req, ln_target, ln_ceiling, m, want_hz, "jb_batch_set_peak_mode", nullptr)))
        return rc;
    ln_mode = std::move(m);
    return JB_OK;
}

int OutputChain::set_flac(const jb_flac_opts *opts)
{
    FlacParams p{};
    int rc = flac_check_opts(opts, &p);
    if (rc)
        return rc;
    // (a JB_BATCH_MLPG_ONLY batch is told that it has no PCM, not which flag its PCM lacks)
    if (!(b.flags & (JB_BATCH_MLPG_ONLY | JB_BATCH_PCM_I16))) {
        set_error("jb_batch_set_flac: FLAC encodes the 16-bit output (JB_BATCH_PCM_I16)");
        return JB_ERR_INVALID;
    }
    if ((rc = check_settable("jb_batch_set_flac: FLAC is set before the batch's first run")))
        return rc;
    flac_p = p;
    flac_on = true;
    replan();
    return JB_OK;
}

int OutputChain::set_flac_meta(const jb_flac_meta *meta)
{
    FlacMeta m{};
    int rc = flac_check_meta(meta, &m);
    if (rc)
        return rc;
    if (!flac_on) {
        set_error("jb_batch_set_flac_meta: call jb_batch_set_flac first");
        return JB_ERR_INVALID;
    }
    if ((rc = check_settable("jb_batch_set_flac_meta: the metadata is set before the batch's first run")))
        return rc;
    flac_m = m; // (the plan of the slabs does not depend on it: the FLAC slabs are sized at the first run)
    return JB_OK;
}

int OutputChain::set_format(const jb_format_opts *opts)
{
    if (!opts) {
        set_error("jb_batch_set_format: opts is NULL");
        return JB_ERR_INVALID;
    }
    int rc = format_check_opts(opts->format, opts->dither, "jb_batch_set_format");
    if (rc)
        return rc;
    if ((rc = check_settable("jb_batch_set_format: the format is set before the batch's first run")))
        return rc;
    if (b.flags & JB_BATCH_PCM_I16) {
        set_error("jb_batch_set_format: the format stage reads the f64 output (a batch without JB_BATCH_PCM_I16)");
        return JB_ERR_INVALID;
    }
    fmt_p = *opts;
    fmt_on = true;
    replan();
    return JB_OK;
}

int OutputChain::set_adpcm(const jb_adpcm_opts *opts)
{
    int rc = adpcm_check_opts((const AdpcmOpts *)opts, "jb_batch_set_adpcm");
    if (rc)
        return rc;
    if ((rc = check_settable("jb_batch_set_adpcm: IMA ADPCM is set before the batch's first run")))
        return rc;
    ad_align = opts->block_align;
    ad_on = true;
    replan();
    return JB_OK;
}

// The join request `req` ([B], empty: none) under these rates: JB_ERR_INVALID naming what is wrong
int OutputChain::check_join(const std::vector<JoinUtt> &req, const std::vector<uint32_t> &want, const char *who) const
{
    if (req.empty())
        return JB_OK;
    const size_t B = (size_t)b.B;
    std::vector<uint32_t> hz(B, b.voice.sampling_frequency);
    for (size_t u = 0; u < want.size(); u++)
        if (want[u])
            hz[u] = want[u];
    std::vector<uint64_t> n(B, 0); // (the lengths do not bear on the check)
    JoinLayout lay;
    return join_layout_checked(req.data(), n.data(), hz.data(), B, sizeof(double), &lay, who);
}

int OutputChain::set_join(const jb_join_utt *req, size_t n)
{
    int rc = check_settable("jb_batch_set_join: the join is set before the batch's first run");
    if (rc)
        return rc;
    if (!req && n == 0) {
        join_req.clear();
        replan();
        return JB_OK;
    }
    if (!req || n != (size_t)b.B) {
        set_error("jb_batch_set_join: give one request per utterance");
        return JB_ERR_INVALID;
    }
    std::vector<JoinUtt> r((const JoinUtt *)req, (const JoinUtt *)req + n);
    if ((rc = check_join(r, want_hz, "jb_batch_set_join")))
        return rc;
    join_req = std::move(r);
    replan();
    return JB_OK;
}

// The filter request `req` ([B], empty: none) under these rates: JB_ERR_INVALID naming the utterance, the section
// and the field
int OutputChain::check_filter(const std::vector<jb_filter> &req, const std::vector<uint32_t> &want, const char *who) const
{
    int rc;
    for (size_t u = 0; u < req.size(); u++) {
        const uint32_t hz = (u < want.size() && want[u]) ? want[u] : b.voice.sampling_frequency;
        if ((rc = filter_design_checked(&req[u], hz, u, nullptr, who)))
            return rc;
    }
    return JB_OK;
}

int OutputChain::set_filter(const jb_filter *f, size_t n)
{
    int rc = check_settable("jb_batch_set_filter: the filter is set before the batch's first run");
    if (rc)
        return rc;
    if (!f && n == 0) {
        filt_req.clear();
        filt_any.clear();
        replan();
        return JB_OK;
    }
    if (!f || (n != 1 && n != (size_t)b.B)) {
        set_error("jb_batch_set_filter: give one filter, or one per utterance");
        return JB_ERR_INVALID;
    }
    std::vector<jb_filter> r((size_t)b.B);
    for (size_t u = 0; u < r.size(); u++)
        r[u] = f[n == 1 ? 0 : u];
    if ((rc = check_filter(r, want_hz, "jb_batch_set_filter")))
        return rc;
    filt_any.assign(r.size(), 0);
    for (size_t u = 0; u < r.size(); u++)
        filt_any[u] = r[u].n_sections != 0;
    filt_req = std::move(r);
    replan();
    return JB_OK;
}

int OutputChain::filter_coefficients(size_t u, jb_biquad *out, uint32_t *n) const
{
    *n = 0;
    if (!plan.filtered() || u >= filt_req.size())
        return JB_OK;
    double c[kFiltMaxSections * kFiltCoefs] = {};
    int rc = filter_design_checked(&filt_req[u], plan.utt[u].hz, u, c, "jb_batch_filter_coefficients");
    if (rc)
        return rc;
    *n = filt_req[u].n_sections;
    std::copy(c, c + *n * kFiltCoefs, (double *)out);
    return JB_OK;
}

// The classes (one table per distinct filter and rate; utterances without sections share the identity), the
// utterance list sorted by section count and the per-tile state scratch: the f64 of the stage in front in, the
// filter's slab out
int OutputChain::prepare_filter()
{
    if (!plan.filtered())
        return JB_OK;
    const size_t B = (size_t)b.B;
    const double *src = (const double *)slab[(size_t)plan.filter_src];
    char *dst = (char *)slab[(size_t)plan.filter.slab];
    const size_t elem = plan.filter.i16 ? sizeof(int16_t) : sizeof(double);
    std::vector<uint32_t> hz(B), cls_of;
    for (size_t u = 0; u < B; u++)
        hz[u] = plan.utt[u].hz;
    int rc = filter_classes(filt_req.data(), B, hz.data(), B, &fil.classes, &cls_of, "jb_batch_set_filter");
    if (rc)
        return rc;
    fil.utts.assign(B, FilterUtt{});
    uint64_t tiles = 0;
    for (size_t u = 0; u < B; u++) {
        const OutUtt &o = plan.utt[u];
        if (filter_tiles(o.n) > kFiltMaxTiles) {
            set_error("filter: utterance " + std::to_string(u) + " is too long");
            return JB_ERR_UNSUPPORTED;
        }
        fil.utts[u] = {src + o.off, dst + o.off * elem, o.n, tiles, 0, (uint32_t)filter_tiles(o.n), cls_of[u]};
        tiles += fil.utts[u].ntiles;
    }
    if ((rc = filter_launch_list(fil.classes, fil.utts, nullptr, &fil.all)))
        return rc;
    if ((rc = b.dalloc(&fil.classes_dev, fil.classes.size(), false)) || (rc = b.dalloc(&fil.utts_dev, B, false)) ||
        (rc = b.dalloc(&fil.redo_dev, B, false)) || (rc = b.dalloc(&fil.st, (size_t)tiles * kFiltMaxD, false)))
        return rc;
    hipError_t e;
    if ((!fil.classes.empty() && (e = hipMemcpy(fil.classes_dev, fil.classes.data(), sizeof(FilterClass) * fil.classes.size(),
                                               hipMemcpyHostToDevice)) != hipSuccess) ||
        (B > 0 && (e = hipMemcpy(fil.utts_dev, fil.all.utts.data(), sizeof(FilterUtt) * B, hipMemcpyHostToDevice)) !=
                      hipSuccess))
        return hip_fail(e, "filter work list");
    return JB_OK;
}

// At the first run (a second one, or the step done again behind a resident-GV formation timeout, finds it done).
// The vocoder is pointed at its slab last: a failure leaves the batch as it was created, its blocks the batch's own
int OutputChain::prepare()
{
    if (ready)
        return JB_OK;
    frozen = true;
    int rc;
    for (size_t s = 0; s < (size_t)OutSlab::Count; s++)
        if (plan.alloc[s] && (rc = b.dalloc_bytes(&slab[s], (size_t)plan.alloc[s] * out_slab_elem((OutSlab)s), false)))
            return rc;
    if ((rc = prepare_resample()) || (rc = prepare_filter()) || (rc = prepare_loudness()) || (rc = prepare_join()) || (rc = prepare_flac()) ||
        (rc = prepare_format()) || (rc = prepare_adpcm()))
        return rc;
    if (plan.active()) {
        void *voc = slab[(size_t)plan.vocoder.slab];
        b.vd.pcm = plan.vocoder.i16 ? nullptr : (double *)voc;
        b.vd.pcm16 = plan.vocoder.i16 ? (int16_t *)voc : nullptr;
    }
    ready = true;
    return JB_OK;
}

// One table per distinct rate (native utterances go through the identity table: a copy, or the 16-bit conversion
// alone) and the tiles, reading the vocoder's f64 and writing the converter's slab
int OutputChain::prepare_resample()
{
    if (!plan.convert)
        return JB_OK;
    const size_t B = (size_t)b.B;
    const uint32_t in = b.voice.sampling_frequency;
    const double *src = (const double *)slab[(size_t)plan.vocoder.slab];
    char *dst = (char *)slab[(size_t)plan.converter.slab];
    const size_t elem = plan.converter.i16 ? sizeof(int16_t) : sizeof(double);
    std::vector<ResampleTable> tables;
    std::vector<uint32_t> rate_of_table;
    int rc;
    rs.tiles.clear();
    rs.tile_lo.assign(B + 1, 0);
    for (size_t u = 0; u < B; u++) {
        const OutUtt &w = plan.utt[u];
        const size_t t = std::find(rate_of_table.begin(), rate_of_table.end(), w.hz) - rate_of_table.begin();
        if (t == rate_of_table.size()) {
            ResampleTable tb{};
            if ((rc = resample_table(b.device, in, w.hz, &tb)))
                return rc;
            rate_of_table.push_back(w.hz);
            tables.push_back(tb);
            rs.lds = std::max<size_t>(rs.lds, tb.lds_bytes);
        }
        rs.tile_lo[u] = (uint32_t)rs.tiles.size();
        resample_tiles(tables[t], (uint32_t)t, src + (size_t)b.frame_off[u] * b.voice.fperiod,
                       (uint64_t)b.T[u] * b.voice.fperiod, dst + w.off * elem, w.n, rs.tiles);
    }
    rs.tile_lo[B] = (uint32_t)rs.tiles.size();
    const size_t nt = std::max<size_t>(rs.tiles.size(), 1);
    if ((rc = b.dalloc(&rs.tables_dev, tables.size(), false)) || (rc = b.dalloc(&rs.tiles_dev, nt, false)) ||
        (rc = b.dalloc(&rs.redo_dev, nt, false)))
        return rc;
    hipError_t e;
    if ((e = hipMemcpy(rs.tables_dev, tables.data(), sizeof(ResampleTable) * tables.size(), hipMemcpyHostToDevice)) !=
            hipSuccess ||
        (!rs.tiles.empty() && (e = hipMemcpy(rs.tiles_dev, rs.tiles.data(), sizeof(ResampleTile) * rs.tiles.size(),
                                             hipMemcpyHostToDevice)) != hipSuccess))
        return hip_fail(e, "resample work list");
    return JB_OK;
}

// The per-rate tables and the utterance list: the measurement reads the f64 of the stage in front, the apply pass
// writes x * g to its own slab
int OutputChain::prepare_loudness()
{
    if (!plan.normalize())
        return JB_OK;
    const size_t B = (size_t)b.B;
    const double *src = (const double *)slab[(size_t)plan.measure];
    char *dst = (char *)slab[(size_t)plan.apply.slab];
    const size_t elem = plan.apply.i16 ? sizeof(int16_t) : sizeof(double);
    std::vector<LoudnessRate> rates;
    ln.utts.assign(B, LoudnessUtt{});
    uint64_t tiles = 0, atiles = 0;
    int rc;
    for (size_t u = 0; u < B; u++) {
        const OutUtt &o = plan.utt[u];
        size_t r = 0;
        while (r < rates.size() && rates[r].hz != o.hz)
            r++;
        if (r == rates.size()) {
            LoudnessRate lr{};
            if ((rc = loudness_rate(o.hz, &lr)))
                return rc;
            rates.push_back(lr);
        }
        LoudnessUtt &w = ln.utts[u];
        w.x = src + o.off;
        w.y = dst + o.off * elem;
        w.n = o.n;
        w.ntiles = loudness_tiles(rates[r], w.n);
        w.tile0 = w.lt0 = tiles;
        w.at0 = atiles;
        w.rate = (uint32_t)r;
        w.slot = (uint32_t)u;
        w.target = ln_target[u];
        w.ceiling = ln_ceiling[u];
        w.mode = peak_mode(u);
        ln.true_peak = ln.true_peak || w.mode == JB_PEAK_TRUE;
        tiles += w.ntiles;
        atiles += (w.n + kLnApplyTile - 1) / kLnApplyTile;
    }
    const size_t nt = (size_t)std::max<uint64_t>(tiles, 1);
    if ((rc = b.dalloc(&ln.rates_dev, rates.size(), false)) || (rc = b.dalloc(&ln.utts_dev, B, false)) ||
        (rc = b.dalloc(&ln.redo_dev, B, false)) || (rc = b.dalloc(&ln.st, 4 * nt, false)) ||
        (rc = b.dalloc(&ln.pk, nt, false)) || (rc = b.dalloc(&ln.z, nt, false)) ||
        (rc = b.dalloc(&ln.res, B, false)) || (ln.true_peak && (rc = b.dalloc(&ln.tp, nt, false))))
        return rc;
    hipError_t e;
    if ((e = hipMemcpy(ln.rates_dev, rates.data(), sizeof(LoudnessRate) * rates.size(), hipMemcpyHostToDevice)) !=
            hipSuccess ||
        (B > 0 && (e = hipMemcpy(ln.utts_dev, ln.utts.data(), sizeof(LoudnessUtt) * B, hipMemcpyHostToDevice)) !=
                      hipSuccess))
        return hip_fail(e, "loudness work list");
    ln.tiles = tiles;
    ln.atiles = atiles;
    // with a group or a report request: the sets (every utterance, then every group) and what their kernels write
    const bool grouped = !ln_group_req.empty();
    if ((!grouped && !ln_report) || B == 0)
        return JB_OK;
    const size_t G = ln_groups.size();
    ln.sets.assign(B + G, LoudnessSet{});
    std::vector<uint32_t> members(grouped ? 2 * B : B);
    for (size_t u = 0; u < B; u++) {
        ln.sets[u] = LoudnessSet{(uint32_t)u, 1, (uint32_t)u, (uint32_t)u};
        members[u] = (uint32_t)u;
        if (grouped)
            members[B + u] = ln_groups.members[u];
    }
    for (size_t g = 0; g < G; g++)
        ln.sets[B + g] = LoudnessSet{(uint32_t)B + ln_groups.first[g], ln_groups.first[g + 1] - ln_groups.first[g],
                                     (uint32_t)g, (uint32_t)(B + g)};
    if ((rc = b.dalloc(&ln.sets_dev, B + G, false)) || (rc = b.dalloc(&ln.sets_redo_dev, B + G, false)) ||
        (rc = b.dalloc(&ln.members_dev, members.size(), false)) ||
        (grouped && ((rc = b.dalloc(&ln.gres, G, false)) || (rc = b.dalloc(&ln.apply_redo_dev, B, false)))) ||
        (ln_report && ((rc = b.dalloc(&ln.sw, nt, false)) || (rc = b.dalloc(&ln.mm, B, false)) ||
                       (rc = b.dalloc(&ln.r128, B + G, false)))))
        return rc;
    if ((e = hipMemcpy(ln.sets_dev, ln.sets.data(), sizeof(LoudnessSet) * (B + G), hipMemcpyHostToDevice)) !=
            hipSuccess ||
        (e = hipMemcpy(ln.members_dev, members.data(), sizeof(uint32_t) * members.size(), hipMemcpyHostToDevice)) !=
            hipSuccess)
        return hip_fail(e, "loudness group list");
    return JB_OK;
}

// The units the encoders take, in the slab each of them reads: the programmes behind a join, else the utterances
std::vector<OutputChain::EncUnit> OutputChain::enc_units() const
{
    std::vector<EncUnit> units;
    if (joined())
        for (const OutUnit &w : plan.units)
            units.push_back({w.off, w.n, w.hz});
    else
        for (const OutUtt &w : plan.utt)
            units.push_back({w.off, w.n, w.hz});
    return units;
}

// The members in programme order and one span per programme: the final PCM of the plan in, the join slab out
int OutputChain::prepare_join()
{
    if (!joined())
        return JB_OK;
    const size_t B = (size_t)b.B, P = plan.units.size();
    const size_t elem = plan.join.i16 ? sizeof(int16_t) : sizeof(double);
    const char *src = (const char *)slab[(size_t)plan.join_src.slab];
    char *dst = (char *)slab[(size_t)plan.join.slab];
    jn.members.assign(B, JoinMember{});
    jn.member_at.assign(B, 0);
    jn.spans.assign(P, JoinSpan{});
    jn.tiles = 0;
    for (size_t p = 0; p < P; p++) {
        const uint32_t m0 = plan.prog_first[p], m1 = plan.prog_first[p + 1];
        for (uint32_t i = m0; i < m1; i++) {
            const uint32_t u = plan.prog_members[i];
            jn.member_at[u] = i;
            jn.members[i] = {src + plan.utt[u].off * elem, plan.prog_start[u], plan.utt[u].n, join_req[u].fade_in,
                             join_req[u].fade_out};
        }
        jn.spans[p] = {dst + plan.units[p].off * elem, plan.units[p].n, 0, plan.units[p].n, jn.tiles, m0, m1 - m0};
        jn.tiles += join_tiles(0, plan.units[p].n, plan.join.i16);
    }
    int rc;
    // (a redo lists at most one span per member)
    if ((rc = b.dalloc(&jn.members_dev, B, false)) || (rc = b.dalloc(&jn.spans_dev, P, false)) ||
        (rc = b.dalloc(&jn.redo_dev, B, false)))
        return rc;
    hipError_t e;
    if (B > 0 && ((e = hipMemcpy(jn.members_dev, jn.members.data(), sizeof(JoinMember) * B, hipMemcpyHostToDevice)) !=
                      hipSuccess ||
                  (e = hipMemcpy(jn.spans_dev, jn.spans.data(), sizeof(JoinSpan) * P, hipMemcpyHostToDevice)) !=
                      hipSuccess))
        return hip_fail(e, "join work list");
    return JB_OK;
}

// The streams' lists and slabs: one stream per unit (an utterance; behind a join a programme) of the 16-bit slab
// FLAC reads, at its output rate
int OutputChain::prepare_flac()
{
    if (!flac_on)
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t B = units.size();
    std::vector<const int16_t *> xs(B);
    std::vector<uint64_t> ns(B);
    std::vector<uint32_t> hz(B);
    for (size_t u = 0; u < B; u++) {
        xs[u] = (const int16_t *)slab[(size_t)plan.flac] + units[u].off;
        ns[u] = units[u].n;
        hz[u] = units[u].hz;
    }
    std::vector<FlacUtt> utts;
    uint64_t slot_bytes = 0, bound = 0;
    int rc = flac_plan(flac_p, flac_m, xs.data(), ns.data(), hz.data(), B, &utts, &fl.work, &slot_bytes, &bound);
    if (rc)
        return rc;
    const bool md5 = (flac_m.flags & kFlacMetaMd5) != 0;
    std::vector<uint32_t> order;
    if (md5)
        flac_md5_order(utts, nullptr, &order);
    fl.n_md5 = (uint32_t)order.size();
    fl.max_points = 0;
    for (const FlacUtt &w : utts)
        fl.max_points = std::max(fl.max_points, w.n_points);
    const size_t nf = std::max<size_t>(fl.work.size(), 1);
    uint8_t *slots = nullptr;
    if ((rc = b.dalloc(&slots, std::max<uint64_t>(slot_bytes, 4), false)) ||
        (rc = b.dalloc(&fl.out, std::max<uint64_t>(bound, 4), false)) || (rc = b.dalloc(&fl.utts_dev, B, false)) ||
        (rc = b.dalloc(&fl.work_dev, nf, false)) || (rc = b.dalloc(&fl.redo_dev, nf, false)) ||
        (rc = b.dalloc(&fl.fsize, nf, false)) || (rc = b.dalloc(&fl.foff, nf, false)) ||
        (rc = b.dalloc(&fl.res, B, false)) || (rc = b.dalloc(&fl.total, 1, false)) ||
        (md5 && ((rc = b.dalloc(&fl.md5_order_dev, std::max<size_t>(B, 1), false)) ||
                 (rc = b.dalloc(&fl.md5_redo_dev, std::max<size_t>(B, 1), false)) ||
                 (rc = b.dalloc(&fl.digests, 4 * std::max<size_t>(B, 1), false)))))
        return rc;
    flac_bind(&utts, slots);
    hipError_t e = hipSuccess;
    if ((B > 0 && (e = hipMemcpy(fl.utts_dev, utts.data(), sizeof(FlacUtt) * B, hipMemcpyHostToDevice)) != hipSuccess) ||
        (!fl.work.empty() && (e = hipMemcpy(fl.work_dev, fl.work.data(), sizeof(FlacWork) * fl.work.size(),
                                            hipMemcpyHostToDevice)) != hipSuccess) ||
        (!order.empty() && (e = hipMemcpy(fl.md5_order_dev, order.data(), sizeof(uint32_t) * order.size(),
                                          hipMemcpyHostToDevice)) != hipSuccess))
        return hip_fail(e, "FLAC work list");
    if (md5)
        fl.utts = std::move(utts);
    return JB_OK;
}

// The utterance list: the final f64 of the plan in, each utterance's bytes at its 16-byte aligned place out
int OutputChain::prepare_format()
{
    if (plan.fmt_src == OutSlab::None)
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t B = units.size();
    const double *src = (const double *)slab[(size_t)plan.fmt_src];
    uint8_t *dst = (uint8_t *)slab[(size_t)OutSlab::Fmt];
    fm.utts.assign(B, FormatUtt{});
    fm.tiles = 0;
    for (size_t u = 0; u < B; u++) {
        FormatUtt &w = fm.utts[u];
        w.x = src + units[u].off;
        w.y = dst + plan.fmt[u].off;
        w.n = units[u].n;
        w.ft0 = fm.tiles;
        fm.tiles += (w.n + kFmtTile - 1) / kFmtTile;
    }
    int rc;
    if ((rc = b.dalloc(&fm.utts_dev, B, false)) || (rc = b.dalloc(&fm.redo_dev, B, false)))
        return rc;
    hipError_t e;
    if (B > 0 && (e = hipMemcpy(fm.utts_dev, fm.utts.data(), sizeof(FormatUtt) * B, hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(e, "format work list");
    return JB_OK;
}

// The utterance list: the final PCM of the plan in (f64 or 16-bit), each utterance's blocks at their 16-byte aligned
// place out
int OutputChain::prepare_adpcm()
{
    if (plan.adpcm_src.slab == OutSlab::None)
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t B = units.size();
    const char *src = (const char *)slab[(size_t)plan.adpcm_src.slab];
    const size_t elem = plan.adpcm_src.i16 ? sizeof(int16_t) : sizeof(double);
    uint8_t *dst = (uint8_t *)slab[(size_t)OutSlab::Adpcm];
    ad.utts.assign(B, AdpcmUtt{});
    ad.groups = 0;
    for (size_t u = 0; u < B; u++) {
        AdpcmUtt &w = ad.utts[u];
        w.x = src + units[u].off * elem;
        w.y = dst + plan.adpcm[u].off;
        w.n = units[u].n;
        w.g0 = ad.groups;
        w.A = plan.adpcm[u].A;
        w.spb = adpcm_spb(w.A);
        ad.groups += (adpcm_blocks(w.n, w.A) + kAdpcmLanes - 1) / kAdpcmLanes;
    }
    int rc;
    if ((rc = b.dalloc(&ad.utts_dev, B, false)) || (rc = b.dalloc(&ad.redo_dev, B, false)))
        return rc;
    hipError_t e;
    if (B > 0 && (e = hipMemcpy(ad.utts_dev, ad.utts.data(), sizeof(AdpcmUtt) * B, hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(e, "ADPCM work list");
    return JB_OK;
}

int OutputChain::enqueue(const std::vector<uint8_t> *only)
{
    const bool fmt = plan.fmt_src != OutSlab::None;
    const bool adp = plan.adpcm_src.slab != OutSlab::None;
    if (!ready || !(plan.active() || flac_on || fmt || adp || joined()))
        return JB_OK;
    const uint32_t B = (uint32_t)b.B;
    const uint32_t U = (uint32_t)num_outputs(); // the encoders' units: the programmes behind a join, else B
    hipStream_t st = b.stream_voc;
    // the lists of a run: the batch's own
    const ResampleTile *tiles = rs.tiles_dev;
    const LoudnessUtt *utts = ln.utts_dev;
    const FlacWork *work = fl.work_dev;
    const uint32_t *md5_order = fl.md5_order_dev;
    uint32_t n_md5 = fl.n_md5;
    const FormatUtt *futts = fm.utts_dev;
    uint32_t n_futts = fmt ? U : 0;
    uint64_t ft = fm.tiles;
    const AdpcmUtt *autts = ad.utts_dev;
    uint32_t n_autts = adp ? U : 0;
    uint64_t ag = ad.groups;
    const uint32_t n_all_work = (uint32_t)fl.work.size();
    uint32_t n_tiles = (uint32_t)rs.tiles.size(), n_utts = B, n_work = n_all_work;
    uint64_t lt = ln.tiles, at = ln.atiles;
    // loudness groups and the R128 report (with a target only): the utterances the apply pass takes, the groups, the
    // report's sets
    const bool grouped = plan.normalize() && ln.gres, report = plan.normalize() && ln.r128;
    const size_t G = grouped ? ln_groups.size() : 0;
    const LoudnessUtt *apply_utts = ln.utts_dev;
    uint32_t n_apply = B, n_gsets = (uint32_t)G, n_rsets = report ? (uint32_t)(B + G) : 0;
    const LoudnessSet *gsets = grouped ? ln.sets_dev + B : nullptr, *rsets = ln.sets_dev;
    // behind the apply pass a group's gain reaches every member: the stages there run again for all of them
    std::vector<uint8_t> touched_groups, group_members;
    const std::vector<uint8_t> *post = only;
    // behind the join a member's samples reach its programme: the encoders run again for every programme of `post`
    std::vector<uint8_t> touched_units;
    const std::vector<uint8_t> *upost = only; // [U]
    const JoinSpan *jspans = jn.spans_dev;
    uint32_t n_jspans = joined() ? U : 0;
    uint64_t jt = jn.tiles;
    const bool filt = plan.filtered();
    FilterLaunch flt_sub;
    const FilterLaunch *flt = &fil.all;
    const FilterUtt *flt_utts = fil.utts_dev;
    hipError_t e = hipSuccess;
    if (only && grouped) {
        loudness_groups_closure(ln_groups, *only, &touched_groups, &group_members);
        post = &group_members;
    }
    upost = post;
    if (only && joined()) {
        join_closure(plan.prog_of, U, *post, &touched_units);
        upost = &touched_units;
    }
    if (only) {
        // of a redo: the tiles, the utterances (renumbered: their scratch stays where it is) and the FLAC blocks of
        // the utterances it rewrote, uploaded before the first launch
        std::vector<ResampleTile> rs_sub;
        std::vector<LoudnessUtt> ln_sub;
        std::vector<FlacWork> fl_sub;
        std::vector<uint32_t> md5_sub;
        std::vector<FormatUtt> fm_sub;
        std::vector<AdpcmUtt> ad_sub;
        std::vector<LoudnessUtt> ap_sub; // grouped: the apply pass's own list
        std::vector<LoudnessSet> set_sub;
        std::vector<JoinSpan> jn_sub;
        // a recursive filter carries a changed sample to the utterance's end: every touched utterance whole
        if (filt) {
            int rc = filter_launch_list(fil.classes, fil.utts, only, &flt_sub);
            if (rc)
                return rc;
            flt = &flt_sub;
            flt_utts = fil.redo_dev;
        }
        lt = at = ft = ag = jt = 0;
        uint64_t mat = 0; // apply tiles of the measured list (its at0 is not read when the apply pass has its own)
        for (size_t u = 0; u < B; u++) {
            if ((*only)[u]) {
                if (plan.convert)
                    rs_sub.insert(rs_sub.end(), rs.tiles.begin() + rs.tile_lo[u],
                                  rs.tiles.begin() + rs.tile_lo[u + 1]);
                if (plan.normalize()) {
                    LoudnessUtt w = ln.utts[u];
                    w.lt0 = lt;
                    w.at0 = mat;
                    lt += w.ntiles;
                    mat += (w.n + kLnApplyTile - 1) / kLnApplyTile;
                    ln_sub.push_back(w);
                    if (report)
                        set_sub.push_back(ln.sets[u]);
                }
            }
            if (!(*post)[u])
                continue;
            if (grouped) {
                LoudnessUtt w = ln.utts[u];
                w.at0 = at;
                at += (w.n + kLnApplyTile - 1) / kLnApplyTile;
                ap_sub.push_back(w);
            }
            if (joined() && plan.utt[u].n) {
                // the member's span alone, widened to whole groups (the samples around it are what they were: its
                // neighbours' current ones, and pads)
                const uint64_t gs = kJoinGroupBytes / (plan.join.i16 ? sizeof(int16_t) : sizeof(double));
                JoinSpan w = jn.spans[plan.prog_of[u]];
                const JoinMember &m = jn.members[jn.member_at[u]];
                w.k0 = m.start / gs * gs;
                w.k1 = std::min<uint64_t>((m.start + m.n + gs - 1) / gs * gs, w.n);
                w.t0 = jt;
                jt += join_tiles(w.k0, w.k1, plan.join.i16);
                jn_sub.push_back(w);
            }
        }
        for (size_t u = 0; u < U; u++) {
            if (!(*upost)[u])
                continue;
            if (fmt) {
                FormatUtt w = fm.utts[u];
                w.ft0 = ft;
                ft += (w.n + kFmtTile - 1) / kFmtTile;
                fm_sub.push_back(w);
            }
            if (adp) {
                AdpcmUtt w = ad.utts[u];
                w.g0 = ag;
                ag += (adpcm_blocks(w.n, w.A) + kAdpcmLanes - 1) / kAdpcmLanes;
                ad_sub.push_back(w);
            }
        }
        if (!grouped)
            at = mat;
        const uint32_t n_usets = (uint32_t)set_sub.size();
        for (size_t g = 0; g < G; g++)
            if (touched_groups[g])
                set_sub.push_back(ln.sets[B + g]);
        n_gsets = (uint32_t)set_sub.size() - n_usets;
        n_rsets = report ? (uint32_t)set_sub.size() : 0;
        rsets = ln.sets_redo_dev;
        gsets = ln.sets_redo_dev + n_usets;
        n_apply = grouped ? (uint32_t)ap_sub.size() : (uint32_t)ln_sub.size();
        apply_utts = grouped ? ln.apply_redo_dev : ln.redo_dev;
        for (const FlacWork &w : fl.work)
            if ((*upost)[w.utt])
                fl_sub.push_back(w);
        if (fl.digests)
            flac_md5_order(fl.utts, upost, &md5_sub); // (an utterance without frames keeps its digest of no samples)
        tiles = rs.redo_dev;
        utts = ln.redo_dev;
        work = fl.redo_dev;
        md5_order = fl.md5_redo_dev;
        n_md5 = (uint32_t)md5_sub.size();
        futts = fm.redo_dev;
        n_futts = (uint32_t)fm_sub.size();
        autts = ad.redo_dev;
        n_autts = (uint32_t)ad_sub.size();
        n_tiles = (uint32_t)rs_sub.size();
        n_utts = (uint32_t)ln_sub.size();
        n_work = (uint32_t)fl_sub.size();
        jspans = jn.redo_dev;
        n_jspans = (uint32_t)jn_sub.size();
        if (!n_tiles && !n_utts && !n_work && !n_futts && !n_autts && !n_apply && !n_jspans && flt_sub.utts.empty())
            return JB_OK;
        if ((!flt_sub.utts.empty() && (e = hipMemcpy(fil.redo_dev, flt_sub.utts.data(),
                                                     sizeof(FilterUtt) * flt_sub.utts.size(), hipMemcpyHostToDevice)) !=
                                          hipSuccess) ||
            (n_tiles && (e = hipMemcpy(rs.redo_dev, rs_sub.data(), sizeof(ResampleTile) * n_tiles,
                                       hipMemcpyHostToDevice)) != hipSuccess) ||
            (n_utts && (e = hipMemcpy(ln.redo_dev, ln_sub.data(), sizeof(LoudnessUtt) * n_utts,
                                      hipMemcpyHostToDevice)) != hipSuccess) ||
            (!ap_sub.empty() && (e = hipMemcpy(ln.apply_redo_dev, ap_sub.data(), sizeof(LoudnessUtt) * ap_sub.size(),
                                               hipMemcpyHostToDevice)) != hipSuccess) ||
            (!set_sub.empty() && (e = hipMemcpy(ln.sets_redo_dev, set_sub.data(), sizeof(LoudnessSet) * set_sub.size(),
                                                hipMemcpyHostToDevice)) != hipSuccess) ||
            (n_jspans && (e = hipMemcpy(jn.redo_dev, jn_sub.data(), sizeof(JoinSpan) * n_jspans,
                                        hipMemcpyHostToDevice)) != hipSuccess) ||
            (n_work && (e = hipMemcpy(fl.redo_dev, fl_sub.data(), sizeof(FlacWork) * n_work, hipMemcpyHostToDevice)) !=
                           hipSuccess) ||
            (n_md5 && (e = hipMemcpy(fl.md5_redo_dev, md5_sub.data(), sizeof(uint32_t) * n_md5,
                                     hipMemcpyHostToDevice)) != hipSuccess) ||
            (n_futts && (e = hipMemcpy(fm.redo_dev, fm_sub.data(), sizeof(FormatUtt) * n_futts,
                                       hipMemcpyHostToDevice)) != hipSuccess) ||
            (n_autts && (e = hipMemcpy(ad.redo_dev, ad_sub.data(), sizeof(AdpcmUtt) * n_autts,
                                       hipMemcpyHostToDevice)) != hipSuccess))
            return hip_fail(e, "output chain(redo lists)");
    }
    // a run launches every stage of the plan; a redo those that have something to do again
    if (plan.convert && (!only || n_tiles) &&
        (e = launch_resample(rs.tables_dev, tiles, n_tiles, plan.converter.i16, rs.lds, st)) != hipSuccess)
        return hip_fail(e, only ? "k_resample(redo)" : "k_resample");
    // the filter: behind the converter (its second pass too), in front of the measurement
    if (filt && (!only || !flt->utts.empty()) &&
        (e = launch_filter(fil.classes_dev, flt_utts, *flt, fil.st, plan.filter.i16, st)) != hipSuccess)
        return hip_fail(e, only ? "filter(redo)" : "filter");
    if (plan.normalize() && (!only || n_utts) &&
        ((e = launch_loudness_measure(ln.rates_dev, utts, n_utts, lt, ln.st, ln.pk, ln.tp, ln.z, ln.res, ln.true_peak,
                                      st)) != hipSuccess ||
         // the groups' gate over the measured members' scratch, the report, then one gain for every member
         (grouped && (e = launch_loudness_groups(ln.rates_dev, ln.utts_dev, gsets, n_gsets, ln.members_dev, ln.z,
                                                 ln.res, ln.gres, st)) != hipSuccess) ||
         (report && (e = launch_loudness_range(ln.rates_dev, utts, n_utts, ln.utts_dev, rsets, n_rsets, ln.members_dev,
                                               ln.z, ln.sw, ln.mm, ln.r128, st)) != hipSuccess) ||
         (e = launch_loudness_apply(apply_utts, n_apply, at, ln.res, plan.apply.i16, st)) != hipSuccess))
        return hip_fail(e, only ? "loudness(redo)" : "loudness");
    // the join: behind everything that writes the final PCM, in front of everything that encodes it
    if (joined() && (!only || n_jspans) &&
        (e = launch_join(plan.join.i16, jspans, n_jspans, jt, jn.members_dev, st)) != hipSuccess)
        return hip_fail(e, only ? "k_join(redo)" : "k_join");
    // FLAC: the blocks of the list, the digests of its utterances' now final PCM (on request), then every stream's
    // offsets, place and header (all of fl.work_dev, redo or not): the pack never sees a digest of replaced PCM
    if (flac_on && (!only || n_work) &&
        ((e = launch_flac_encode(flac_p, fl.utts_dev, work, n_work, fl.fsize, st)) != hipSuccess ||
         (fl.digests && (e = launch_flac_md5(fl.utts_dev, md5_order, n_md5, fl.digests, st)) != hipSuccess) ||
         (e = launch_flac_pack(flac_p, fl.utts_dev, U, fl.work_dev, n_all_work, fl.fsize, fl.foff, fl.res, fl.total,
                               fl.out, st, fl.digests, fl.max_points)) != hipSuccess))
        return hip_fail(e, only ? "FLAC(redo)" : "FLAC");
    // the sample format last: behind the apply pass, the converter or the hand-off check, whichever wrote last
    if (fmt && (!only || n_futts) &&
        (e = launch_format(fmt_p.format, fmt_p.dither, fmt_p.seed, futts, n_futts, ft, st)) != hipSuccess)
        return hip_fail(e, only ? "k_format(redo)" : "k_format");
    // IMA ADPCM beside it, of the same final PCM
    if (adp && (!only || n_autts) &&
        (e = launch_adpcm(plan.adpcm_src.i16, autts, n_autts, ag, st)) != hipSuccess)
        return hip_fail(e, only ? "k_adpcm(redo)" : "k_adpcm");
    if (only && (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(e, "output chain(redo)");
    return JB_OK;
}

int OutputChain::check_ready(bool requested, const char *not_run, const char *not_set) const
{
    if (requested && ready)
        return JB_OK;
    set_error(requested ? not_run : not_set);
    return JB_ERR_INVALID;
}

int OutputChain::read_loudness(size_t u, LoudnessResult *r)
{
    int rc = check_ready(plan.normalize(), "jb_batch_loudness: the batch has not run",
                         "jb_batch_loudness: no loudness target is set");
    return rc ? rc : b.read(ln.res + u, r, sizeof *r);
}

uint32_t OutputChain::group_members(size_t u) const
{
    const uint32_t g = ln_groups.group_of[u];
    return ln_groups.first[g + 1] - ln_groups.first[g];
}

int OutputChain::read_loudness_group(size_t u, LoudnessGroupResult *r)
{
    int rc = check_ready(plan.normalize() && !ln_group_req.empty(), "jb_batch_loudness_group: the batch has not run",
                         "jb_batch_loudness_group: needs a loudness target and jb_batch_set_loudness_groups");
    return rc ? rc : b.read(ln.gres + ln_groups.group_of[u], r, sizeof *r);
}

int OutputChain::read_loudness_range(size_t u, bool of_group, LoudnessRange *r)
{
    int rc = check_ready(plan.normalize() && ln_report && (!of_group || !ln_group_req.empty()),
                         "loudness report: the batch has not run",
                         "loudness report: needs a loudness target and jb_batch_set_loudness_report");
    return rc ? rc : b.read(ln.r128 + (of_group ? (size_t)b.B + ln_groups.group_of[u] : u), r, sizeof *r);
}

int OutputChain::flac_ready() const
{
    return check_ready(flac_on, "FLAC: the batch has not run", "FLAC: jb_batch_set_flac was not called");
}

int OutputChain::read_flac_index(size_t u, FlacOut *o)
{
    int rc = flac_ready();
    return rc ? rc : b.read(fl.res + u, o, sizeof *o);
}

int OutputChain::read_flac(const FlacOut &o, uint8_t *dst) { return b.read(fl.out + o.off, dst, (size_t)o.bytes, false); }

int OutputChain::read_flac_all(std::vector<FlacOut> *res, std::unique_ptr<uint8_t[]> *host)
{
    int rc = flac_ready();
    if (rc)
        return rc;
    const size_t B = num_outputs();
    res->assign(B, FlacOut{});
    if ((rc = B > 0 ? b.read(fl.res, res->data(), sizeof(FlacOut) * B) : b.sync()))
        return rc;
    uint64_t total = 0;
    for (const FlacOut &o : *res)
        total = std::max<uint64_t>(total, o.off + o.bytes);
    // one copy of the used bytes (not zero-filled first)
    host->reset(new (std::nothrow) uint8_t[std::max<uint64_t>(total, 1)]);
    if (!*host) {
        set_error("out of host memory");
        return JB_ERR_INVALID;
    }
    return total ? b.read(fl.out, host->get(), (size_t)total, false) : JB_OK;
}

int OutputChain::read_programme(size_t p, bool i16, void *dst)
{
    int rc = check_ready(joined(), "join: the batch has not run", "join: jb_batch_set_join was not called");
    if (rc)
        return rc;
    if (i16 != plan.join.i16) {
        set_error(i16 ? "batch was created without JB_BATCH_PCM_I16"
                      : "batch was created with JB_BATCH_PCM_I16: use jb_batch_read_programme_pcm_i16");
        return JB_ERR_INVALID;
    }
    const OutUnit &w = plan.units[p];
    const size_t elem = i16 ? sizeof(int16_t) : sizeof(double);
    return w.n ? b.read((const char *)slab[(size_t)plan.join.slab] + w.off * elem, dst, (size_t)w.n * elem) : b.sync();
}

const OutAdpcmUtt *OutputChain::adpcm_place(size_t u) const
{
    if (!ad_on) {
        set_error("ADPCM: jb_batch_set_adpcm was not called");
        return nullptr;
    }
    return &plan.adpcm[u];
}

int OutputChain::read_adpcm(size_t u, uint8_t *dst)
{
    int rc = check_ready(ad_on, "ADPCM: the batch has not run", "ADPCM: jb_batch_set_adpcm was not called");
    if (rc)
        return rc;
    const OutAdpcmUtt &w = plan.adpcm[u];
    return w.bytes ? b.read((const uint8_t *)slab[(size_t)OutSlab::Adpcm] + w.off, dst, (size_t)w.bytes) : b.sync();
}

int OutputChain::read_adpcm_all(std::unique_ptr<uint8_t[]> *host)
{
    int rc = check_ready(ad_on, "ADPCM: the batch has not run", "ADPCM: jb_batch_set_adpcm was not called");
    if (rc)
        return rc;
    uint64_t total = 0;
    for (const OutAdpcmUtt &w : plan.adpcm)
        total = std::max<uint64_t>(total, w.off + w.bytes);
    // one copy of the used bytes (not zero-filled first)
    host->reset(new (std::nothrow) uint8_t[std::max<uint64_t>(total, 1)]);
    if (!*host) {
        set_error("out of host memory");
        return JB_ERR_INVALID;
    }
    return total ? b.read(slab[(size_t)OutSlab::Adpcm], host->get(), (size_t)total) : b.sync();
}

int OutputChain::format_ready() const
{
    return check_ready(fmt_on, "format: the batch has not run", "format: jb_batch_set_format was not called");
}

int OutputChain::format_size(size_t u, size_t *n_bytes) const
{
    if (!fmt_on) {
        set_error("format: jb_batch_set_format was not called");
        return JB_ERR_INVALID;
    }
    *n_bytes = (size_t)plan.fmt[u].bytes;
    return JB_OK;
}

int OutputChain::read_formatted(size_t u, uint8_t *dst)
{
    int rc = format_ready();
    if (rc)
        return rc;
    const OutFmtUtt &w = plan.fmt[u];
    return w.bytes ? b.read((const uint8_t *)slab[(size_t)OutSlab::Fmt] + w.off, dst, (size_t)w.bytes) : b.sync();
}

int OutputChain::read_formatted_all(std::unique_ptr<uint8_t[]> *host)
{
    int rc = format_ready();
    if (rc)
        return rc;
    uint64_t total = 0;
    for (const OutFmtUtt &w : plan.fmt)
        total = std::max<uint64_t>(total, w.off + w.bytes);
    // one copy of the used bytes (not zero-filled first)
    host->reset(new (std::nothrow) uint8_t[std::max<uint64_t>(total, 1)]);
    if (!*host) {
        set_error("out of host memory");
        return JB_ERR_INVALID;
    }
    return total ? b.read(slab[(size_t)OutSlab::Fmt], host->get(), (size_t)total) : b.sync();
}

} // namespace jb

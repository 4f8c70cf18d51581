// jb_output_chain.cpp -- OutputChain (jb_host.h): the stages behind the vocoder of one batch.  The setters record a
// request and plan again (plan_output, jb_output.h); prepare() carries the plan out once; enqueue() selects what each
// stage takes (everything, or a redo's part: redo_scope, jb_output.h) and launches, in this order and on the
// vocoder's stream: the converter (k_resample), the filter, loudness (measurement, groups, report, apply pass; with a
// limiter request the limiter in the apply pass's place), the join (or the mix in its place), then the encoders of the final PCM: FLAC (blocks, MD5, pack), the sample format, IMA ADPCM and
// the filterbank features.
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
    in.mix = prog_req.empty() ? nullptr : prog_req.data();
    in.chained = prog_chained;
    in.stem_of = stem_req.empty() || prog_req.empty() || prog_chained ? nullptr : stem_req.data();
    flag_stage();
    in.filter = stage_any.empty() ? nullptr : stage_any.data();
    in.fbank = fb_on ? &fb_p : nullptr;
    in.mfcc_fbank = mf_on ? &mf_fb : nullptr;
    in.mfcc = mf_on ? &mf_p : nullptr;
    in.frame = fr_on ? &fr_p : nullptr;
    in.melspec = ml_on ? &ml_p : nullptr;
    in.pitch = pt_on ? &pt_p : nullptr;
    in.activity = act_on ? &act_p : nullptr;
    plan = plan_output(in);
}

// The plan's filter flag: an utterance has a section, a response or a noise request (without the latter two:
// filt_any itself)
void OutputChain::flag_stage()
{
    std::vector<uint8_t> noise_of(noise_req.size());
    for (size_t u = 0; u < noise_req.size(); u++)
        noise_of[u] = noise_req[u].on;
    stage_any = noise_stage_flags(fir_stage_flags(filt_any, fir_of), noise_of);
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

template <class T> bool OutputChain::broadcast(const T *v, size_t n, std::vector<T> *out, const char *err) const
{
    const size_t B = (size_t)b.B;
    if (!v || (n != 1 && n != B)) {
        set_error(err);
        return false;
    }
    out->resize(B);
    for (size_t u = 0; u < B; u++)
        (*out)[u] = v[n == 1 ? 0 : u];
    return true;
}

std::vector<uint32_t> OutputChain::rates_under(const std::vector<uint32_t> &want) const
{
    std::vector<uint32_t> hz((size_t)b.B, b.voice.sampling_frequency);
    for (size_t u = 0; u < want.size(); u++)
        if (want[u])
            hz[u] = want[u];
    return hz;
}

int OutputChain::set_output_rate(const uint32_t *hz, size_t n)
{
    int rc = check_settable("jb_batch_set_output_rate: the output rate is set before the batch's first run");
    if (rc)
        return rc;
    std::vector<uint32_t> want;
    if (!broadcast(hz, n, &want, "jb_batch_set_output_rate: give one rate, or one per utterance"))
        return JB_ERR_INVALID;
    const uint32_t in = b.voice.sampling_frequency;
    for (uint32_t &w : want) {
        w = w == in ? 0 : w;
        if (w && (rc = resample_design(in, w, nullptr, nullptr)))
            return rc;
    }
    if ((rc = check_groups(ln_group_req, ln_target, ln_ceiling, ln_mode, want, "jb_batch_set_output_rate", nullptr)) ||
        (rc = check_programme(prog_req, prog_chained, mix_opts, want, "jb_batch_set_output_rate")) ||
        (rc = check_filter(filt_req, want, "jb_batch_set_output_rate")) ||
        (rc = check_fir(want, "jb_batch_set_output_rate")) ||
        (rc = check_noise(want, "jb_batch_set_output_rate")) ||
        (fb_on && (rc = check_rates(fb_p, want, "jb_batch_set_output_rate"))) ||
        (mf_on && (rc = check_mfcc(mf_fb, want, "jb_batch_set_output_rate"))) ||
        (ml_on && (rc = check_rates(ml_p, want, "jb_batch_set_output_rate"))) ||
        (pt_on && (rc = check_pitch(want, "jb_batch_set_output_rate"))))
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
    const std::vector<uint32_t> hz = rates_under(want);
    LnGroupsIn in;
    in.B = hz.size();
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
    if ((rc = check_groups(req, ln_target, ln_ceiling, ln_mode, want_hz, "jb_batch_set_loudness_groups", &plan)) ||
        (rc = check_limiter_groups(req, lim_req, "jb_batch_set_loudness_groups")))
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
    const char *err = "jb_batch_set_loudness_target: give one target, or one per utterance";
    std::vector<double> t, c;
    if (!broadcast(target, n, &t, err) || !broadcast(ceiling, n, &c, err))
        return JB_ERR_INVALID;
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
    std::vector<uint32_t> m;
    if (!broadcast(mode, n, &m, "jb_batch_set_peak_mode: give one mode, or one per utterance"))
        return JB_ERR_INVALID;
    for (uint32_t v : m)
        if (v != JB_PEAK_SAMPLE && v != JB_PEAK_TRUE) {
            set_error("jb_batch_set_peak_mode: a mode is JB_PEAK_SAMPLE or JB_PEAK_TRUE");
            return JB_ERR_INVALID;
        }
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

template <class Opts>
int OutputChain::check_rates(const Opts &opts, const std::vector<uint32_t> &want, const char *who) const
{
    int rc;
    for (uint32_t hz : rates_under(want))
        if ((rc = rate_geometry(&opts, hz, who, nullptr)))
            return rc;
    return JB_OK;
}

int OutputChain::check_feature_settable(const char *entry, const char *noun) const
{
    if (b.flags & JB_BATCH_MLPG_ONLY) {
        set_error("a JB_BATCH_MLPG_ONLY batch has no PCM");
        return JB_ERR_UNSUPPORTED;
    }
    if (b.flags & JB_BATCH_PCM_I16) {
        set_error(std::string(entry) + ": the " + noun +
                  " stage reads the f64 output (a batch without JB_BATCH_PCM_I16)");
        return JB_ERR_UNSUPPORTED;
    }
    return check_settable((std::string(entry) + ": the features are set before the batch's first run").c_str());
}

int OutputChain::set_fbank(const jb_fbank_opts *opts)
{
    int rc;
    if (opts && (rc = fbank_check_opts((const FbankOpts *)opts, "jb_batch_set_fbank")))
        return rc;
    if ((rc = check_feature_settable("jb_batch_set_fbank", "fbank")))
        return rc;
    if (opts && ((rc = check_rates(*(const FbankOpts *)opts, want_hz, "jb_batch_set_fbank")) ||
                 (rc = check_frame(fr_on ? &fr_p : nullptr, (const FbankOpts *)opts, nullptr, nullptr,
                                   "jb_batch_set_fbank"))))
        return rc;
    fb_on = opts != nullptr;
    if (opts)
        fb_p = *(const FbankOpts *)opts;
    replan();
    return JB_OK;
}

// The cepstral request's filterbank under these rates, as the stage runs it (f64 logarithms)
int OutputChain::check_mfcc(const FbankOpts &fopts, const std::vector<uint32_t> &want, const char *who) const
{
    return check_rates(mfcc_fbank_opts(fopts), want, who);
}

int OutputChain::set_mfcc(const jb_fbank_opts *fopts, const jb_mfcc_opts *opts)
{
    int rc;
    const bool on = fopts || opts;
    if (on && ((rc = mfcc_check_fbank((const FbankOpts *)fopts, "jb_batch_set_mfcc")) ||
               (rc = mfcc_check_opts((const MfccOpts *)opts, fopts->n_mels, "jb_batch_set_mfcc"))))
        return rc;
    if ((rc = check_feature_settable("jb_batch_set_mfcc", "cepstral")))
        return rc;
    if (on && ((rc = check_mfcc(*(const FbankOpts *)fopts, want_hz, "jb_batch_set_mfcc")) ||
               (rc = check_frame(fr_on ? &fr_p : nullptr, nullptr, (const FbankOpts *)fopts, (const MfccOpts *)opts,
                                 "jb_batch_set_mfcc"))))
        return rc;
    mf_on = on;
    if (on) {
        mf_fb = *(const FbankOpts *)fopts;
        mf_p = *(const MfccOpts *)opts;
    }
    replan();
    return JB_OK;
}

// The frame request beside the feature requests it conditions: JB_ERR_INVALID naming the field
int OutputChain::check_frame(const FrameOpts *fr, const FbankOpts *fb, const FbankOpts *mfb, const MfccOpts *mp,
                             const char *who) const
{
    if (!fr)
        return JB_OK;
    const char *f = fb ? frame_pair_fault(*fb, *fr, false) : nullptr;
    if (!f && mfb)
        f = frame_pair_fault(*mfb, *fr, mp->n_ceps >= 1);
    if (f) {
        set_error(std::string(who) + ": jb_frame_opts: " + f);
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

int OutputChain::set_frame_opts(const jb_frame_opts *fr)
{
    const FrameOpts *q = (const FrameOpts *)fr;
    int rc;
    if (q)
        if (const char *f = frame_opts_fault(*q)) {
            set_error(std::string("jb_batch_set_frame_opts: ") + f);
            return JB_ERR_INVALID;
        }
    if ((rc = check_settable("jb_batch_set_frame_opts: the frame request is set before the batch's first run")) ||
        (rc = check_frame(q, fb_on ? &fb_p : nullptr, mf_on ? &mf_fb : nullptr, &mf_p, "jb_batch_set_frame_opts")))
        return rc;
    fr_on = q != nullptr;
    if (q)
        fr_p = *q;
    replan();
    return JB_OK;
}

int OutputChain::set_melspec(const jb_melspec_opts *opts)
{
    int rc;
    if (opts && (rc = mel_check_opts((const MelOpts *)opts, "jb_batch_set_melspec")))
        return rc;
    if ((rc = check_feature_settable("jb_batch_set_melspec", "mel")))
        return rc;
    if (opts && (rc = check_rates(*(const MelOpts *)opts, want_hz, "jb_batch_set_melspec")))
        return rc;
    ml_on = opts != nullptr;
    if (opts)
        ml_p = *(const MelOpts *)opts;
    replan();
    return JB_OK;
}

int OutputChain::check_pitch(const std::vector<uint32_t> &want, const char *who) const
{
    int rc;
    size_t u = 0;
    for (uint32_t hz : rates_under(want))
        if ((rc = pitch_check_rate(hz, u++, who, nullptr)))
            return rc;
    return JB_OK;
}

int OutputChain::set_pitch(const jb_pitch_opts *opts)
{
    int rc;
    if (opts && (rc = pitch_check_opts((const PitchOpts *)opts, "jb_batch_set_pitch", nullptr)))
        return rc;
    if ((rc = check_feature_settable("jb_batch_set_pitch", "pitch")))
        return rc;
    if (opts && (rc = check_pitch(want_hz, "jb_batch_set_pitch")))
        return rc;
    pt_on = opts != nullptr;
    if (opts)
        pt_p = *(const PitchOpts *)opts;
    replan();
    return JB_OK;
}

// The speech-activity request: tried on the plan of the present requests, and put back where some unit refuses it
int OutputChain::set_activity(const jb_activity_opts *opts)
{
    int rc;
    if (opts && (rc = act_check_opts((const ActOpts *)opts, "jb_batch_set_activity")))
        return rc;
    if ((rc = check_settable("jb_batch_set_activity: the activity request is set before the batch's first run")))
        return rc;
    const bool was_on = act_on;
    const ActOpts was = act_p;
    act_on = opts != nullptr;
    if (opts)
        act_p = *(const ActOpts *)opts;
    replan();
    if (act_on && !activity()) {
        rc = activity_fault("jb_batch_set_activity");
        act_on = was_on;
        act_p = was;
        replan();
        return rc;
    }
    return JB_OK;
}

int OutputChain::activity_fault(const char *who) const
{
    const bool whole = act_opts_fault(act_p) != nullptr; // the options on their own: no unit to name
    set_error(std::string(who) + ": " + (plan.act_fault ? plan.act_fault : "the request was not planned") +
              (whole ? "" : " (unit " + std::to_string(plan.act_fault_unit) + ")"));
    return plan.act_unsupported ? JB_ERR_UNSUPPORTED : JB_ERR_INVALID;
}

// The programme request `req` ([B], empty: none), a join's (`chained`) or a mix's, under these rates: JB_ERR_INVALID
// naming what is wrong
int OutputChain::check_programme(const std::vector<MixUtt> &req, bool chained, const MixOpts &opts,
                                 const std::vector<uint32_t> &want, const char *who,
                                 const std::vector<uint32_t> *stems) const
{
    if (req.empty())
        return JB_OK;
    if (!stems)
        stems = &stem_req;
    const std::vector<uint32_t> hz = rates_under(want);
    // (the lengths at these rates, as plan_output forms them: they decide who lies over whom, so the lists' size)
    std::vector<uint64_t> n(hz.size(), 0);
    for (size_t u = 0; u < n.size(); u++) {
        uint64_t L = 1, M = 1;
        if (hz[u] != b.voice.sampling_frequency)
            resample_ratio(b.voice.sampling_frequency, hz[u], &L, &M);
        n[u] = resample_out_len((uint64_t)b.T[u] * b.voice.fperiod, L, M);
    }
    MixLayout lay;
    return mix_layout_checked(req.data(), chained, n.data(), hz.data(), hz.size(), sizeof(double),
                              chained ? nullptr : &opts, &lay, who, stems->empty() ? nullptr : stems->data());
}

// The one slot for a programme request, a join's (`chained`) or a mix's: what either setter checks before it reads its
// request.  *store: a request of one entry per utterance is given and the slot is free for it; else the call is over
// (refused, or a withdrawal, which leaves a request of the other kind alone)
int OutputChain::open_programme(bool chained, bool given, size_t n, bool *store)
{
    *store = false;
    const std::string kind = chained ? "join" : "mix", who = "jb_batch_set_" + kind;
    int rc = check_settable((who + ": the " + kind + " is set before the batch's first run").c_str());
    if (rc)
        return rc;
    const bool taken = !prog_req.empty() && prog_chained != chained; // the slot holds a request of the other kind
    if (!given && n == 0) {
        if (!taken) {
            prog_req.clear();
            mix_opts = MixOpts{};
            stem_req.clear(); // (the stems stand behind a mix: they leave with it)
            stem_flags = 0;
            replan();
        }
        return JB_OK;
    }
    if (!given || n != (size_t)b.B) {
        set_error(who + ": give one request per utterance");
        return JB_ERR_INVALID;
    }
    if (taken) {
        set_error(who + ": the batch holds a " + (chained ? "mix" : "join") +
                  " request (a batch holds a join or a mix request; withdraw the one first)");
        return JB_ERR_INVALID;
    }
    *store = true;
    return JB_OK;
}

// The request in the mix's words into the slot, checked under the present rates
int OutputChain::store_programme(bool chained, std::vector<MixUtt> req, const MixOpts &opts)
{
    int rc = check_programme(req, chained, opts, want_hz, chained ? "jb_batch_set_join" : "jb_batch_set_mix");
    if (rc)
        return rc;
    prog_req = std::move(req);
    prog_chained = chained;
    mix_opts = opts;
    replan();
    return JB_OK;
}

int OutputChain::set_join(const jb_join_utt *req, size_t n)
{
    bool store;
    const int rc = open_programme(true, req != nullptr, n, &store);
    return rc || !store ? rc : store_programme(true, join_as_mix((const JoinUtt *)req, n), MixOpts{});
}

int OutputChain::set_mix(const jb_mix_utt *req, size_t n, const jb_mix_opts *opts)
{
    bool store;
    const int rc = open_programme(false, req != nullptr, n, &store);
    if (rc || !store)
        return rc;
    const MixUtt *r = (const MixUtt *)req;
    return store_programme(false, std::vector<MixUtt>(r, r + n), opts ? *(const MixOpts *)opts : MixOpts{});
}

int OutputChain::set_mix_stems(const uint32_t *stem_of, size_t n, uint32_t flags)
{
    const char *who = "jb_batch_set_mix_stems";
    int rc = check_settable("jb_batch_set_mix_stems: the stems are set before the batch's first run");
    if (rc)
        return rc;
    if (!stem_of && n == 0 && flags == 0) {
        stem_req.clear();
        stem_flags = 0;
        replan();
        return JB_OK;
    }
    auto refuse = [&](const std::string &what) {
        set_error(std::string(who) + ": " + what);
        return JB_ERR_INVALID;
    };
    if (!stem_of || n != (size_t)b.B)
        return refuse("give one stem id per utterance");
    if (flags & ~kMixStemLevels)
        return refuse("flags holds an unknown flag");
    if (prog_req.empty() || prog_chained)
        return refuse(prog_req.empty() ? "the batch holds no mix request (jb_batch_set_mix comes first)"
                                       : "the batch holds a join request: stems stand behind a mix");
    const std::vector<uint32_t> req(stem_of, stem_of + n);
    if ((rc = check_programme(prog_req, false, mix_opts, want_hz, who, &req)))
        return rc;
    stem_req = req;
    stem_flags = flags;
    replan();
    return JB_OK;
}

// The filter request `req` ([B], empty: none) under these rates: JB_ERR_INVALID naming the utterance, the section
// and the field
int OutputChain::check_filter(const std::vector<jb_filter> &req, const std::vector<uint32_t> &want, const char *who) const
{
    const std::vector<uint32_t> hz = rates_under(want);
    int rc;
    for (size_t u = 0; u < req.size(); u++)
        if ((rc = filter_design_checked(&req[u], hz[u], u, nullptr, who)))
            return rc;
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
    std::vector<jb_filter> r;
    if (!broadcast(f, n, &r, "jb_batch_set_filter: give one filter, or one per utterance"))
        return JB_ERR_INVALID;
    if ((rc = check_filter(r, want_hz, "jb_batch_set_filter")))
        return rc;
    filt_any.assign(r.size(), 0);
    for (size_t u = 0; u < r.size(); u++)
        filt_any[u] = r[u].n_sections != 0;
    filt_req = std::move(r);
    replan();
    return JB_OK;
}

// The convolution request under these rates: a response's rate is its utterance's output rate
int OutputChain::check_fir(const std::vector<uint32_t> &want, const char *who) const
{
    const std::vector<uint32_t> hz = rates_under(want);
    for (size_t u = 0; u < fir_of.size(); u++)
        if (fir_of[u] >= 0 && fir_cls.resp[(size_t)fir_of[u]].hz != hz[u]) {
            set_error(std::string(who) + ": utterance " + std::to_string(u) +
                      ": hz of its impulse response differs from the utterance's output rate (a response is never "
                      "resampled): " + std::to_string(fir_cls.resp[(size_t)fir_of[u]].hz) + " Hz against " +
                      std::to_string(hz[u]) + " Hz");
            return JB_ERR_INVALID;
        }
    return JB_OK;
}

int OutputChain::set_fir(const jb_fir *f, size_t n)
{
    int rc = check_settable("jb_batch_set_fir: the impulse response is set before the batch's first run");
    if (rc)
        return rc;
    if (!f && n == 0) {
        fir_cls = FirClasses{};
        fir_of.clear();
        room_rep.clear();
        replan();
        return JB_OK;
    }
    const size_t B = (size_t)b.B;
    if (!f || (n != 1 && n != B)) {
        set_error("jb_batch_set_fir: give one response, or one per utterance");
        return JB_ERR_INVALID;
    }
    if ((rc = install_fir(f, n, "jb_batch_set_fir")))
        return rc;
    room_rep.clear(); // (the slot now holds a response that no room made)
    return JB_OK;
}

// The convolution slot filled from f[0..n), n == 1 or B: checked at every utterance's output rate, the taps copied
int OutputChain::install_fir(const jb_fir *f, size_t n, const char *who)
{
    int rc;
    const size_t B = (size_t)b.B;
    const std::vector<uint32_t> hz = rates_under(want_hz);
    for (size_t u = 0; u < B; u++)
        if ((rc = fir_check(&f[n == 1 ? 0 : u], hz[u], u, who)))
            return rc;
    FirClasses cls; // (the taps are copied here: the caller's buffers are not read again)
    std::vector<int32_t> of(B, -1);
    bool any = false;
    for (size_t u = 0; u < B; u++) {
        const jb_fir &fu = f[n == 1 ? 0 : u];
        if (!fu.taps)
            continue;
        of[u] = (int32_t)cls.find(*(const FirSpec *)&fu);
        any = true;
    }
    if (!any)
        of.clear();
    fir_cls = std::move(cls);
    fir_of = std::move(of);
    replan();
    return JB_OK;
}

int OutputChain::fir_geometry_of(size_t u, FirGeom *g) const
{
    if (u >= fir_of.size() || fir_of[u] < 0) {
        set_error("jb_batch_fir_geometry: utterance " + std::to_string(u) + " has no impulse response");
        return JB_ERR_INVALID;
    }
    *g = fir_cls.resp[(size_t)fir_of[u]].g;
    return JB_OK;
}

int OutputChain::set_room(const jb_room *r, size_t n, const jb_fir *others)
{
    int rc = check_settable("jb_batch_set_room: the room is set before the batch's first run");
    if (rc)
        return rc;
    if (!r && n == 0)
        return set_fir(nullptr, 0);
    const size_t B = (size_t)b.B;
    if (!r || (n != 1 && n != B)) {
        set_error("jb_batch_set_room: give one room, or one per utterance");
        return JB_ERR_INVALID;
    }
    // every room and its rate first: a refused request has touched no device
    const std::vector<uint32_t> hz = rates_under(want_hz);
    std::vector<jb_room> rooms(B);
    for (size_t u = 0; u < B; u++) {
        rooms[u] = r[n == 1 ? 0 : u];
        if (room_none(*(const RoomSpec *)&rooms[u]))
            continue;
        if ((rc = room_check(&rooms[u], u, "jb_batch_set_room", nullptr)))
            return rc;
        if (rooms[u].hz != hz[u]) {
            set_error("jb_batch_set_room: utterance " + std::to_string(u) +
                      ": hz differs from the utterance's output rate (a response is never resampled): " +
                      std::to_string(rooms[u].hz) + " Hz against " + std::to_string(hz[u]) + " Hz");
            return JB_ERR_INVALID;
        }
    }
    std::vector<std::vector<double>> taps;
    std::vector<RoomTables> tabs;
    if ((rc = room_rirs(rooms.data(), B, b.device, &taps, &tabs, "jb_batch_set_room")))
        return rc;
    std::vector<jb_fir> firs(B, jb_fir{});
    std::vector<jb_room_report> rep(B, jb_room_report{});
    std::vector<uint8_t> has(B, 0);
    for (size_t u = 0; u < B; u++) {
        if (taps[u].empty()) {
            if (others)
                firs[u] = others[u];
            continue;
        }
        const uint32_t delay = (rooms[u].flags & kRoomKeepLatency) ? 0u : tabs[u].direct;
        firs[u] = jb_fir{taps[u].data(), (uint32_t)taps[u].size(), rooms[u].hz, delay, 0};
        rep[u] = room_report_of(taps[u].data(), tabs[u].K, tabs[u].direct, delay);
        has[u] = 1;
    }
    if ((rc = install_fir(firs.data(), B, "jb_batch_set_room")))
        return rc;
    room_rep = std::move(rep);
    room_has = std::move(has);
    return JB_OK;
}

int OutputChain::read_room(size_t u, jb_room_report *out) const
{
    if (u >= room_rep.size() || !room_has[u]) {
        set_error("jb_batch_room_report: utterance " + std::to_string(u) + " has no room");
        return JB_ERR_INVALID;
    }
    *out = room_rep[u];
    return JB_OK;
}

// The noise request under these rates: a bed's rate is its utterance's output rate
int OutputChain::check_noise(const std::vector<uint32_t> &want, const char *who) const
{
    const std::vector<uint32_t> hz = rates_under(want);
    for (size_t u = 0; u < noise_req.size(); u++)
        if (noise_req[u].on && noise_req[u].bed >= 0 && noise_beds.rate[(size_t)noise_req[u].bed] != hz[u]) {
            set_error(std::string(who) + ": utterance " + std::to_string(u) +
                      ": hz of its noise bed differs from the utterance's output rate (a bed is never resampled): " +
                      std::to_string(noise_beds.rate[(size_t)noise_req[u].bed]) + " Hz against " +
                      std::to_string(hz[u]) + " Hz");
            return JB_ERR_INVALID;
        }
    return JB_OK;
}

int OutputChain::set_noise(const jb_noise *req, size_t n, const uint64_t *call_k)
{
    int rc = check_settable("jb_batch_set_noise: the noise is set before the batch's first run");
    if (rc)
        return rc;
    if (!req && n == 0) {
        noise_beds = NoiseBeds{};
        noise_req.clear();
        replan();
        return JB_OK;
    }
    const size_t B = (size_t)b.B;
    if (!req || (n != 1 && n != B)) {
        set_error("jb_batch_set_noise: give one request, or one per utterance");
        return JB_ERR_INVALID;
    }
    const std::vector<uint32_t> hz = rates_under(want_hz);
    for (size_t u = 0; u < B; u++) {
        const jb_noise &r = req[n == 1 ? 0 : u];
        if ((rc = noise_check(&r, hz[u], u, "jb_batch_set_noise")))
            return rc;
        if (n != 1 && !call_k && (r.flags & kNoiseVary)) {
            set_error("jb_batch_set_noise: utterance " + std::to_string(u) +
                      ": flags: JB_NOISE_VARY needs one request over many utterances");
            return JB_ERR_INVALID;
        }
    }
    NoiseBeds beds; // (the beds are copied here: the caller's buffers are not read again)
    std::vector<NoiseItem> items(B);
    bool any = false;
    for (size_t u = 0; u < B; u++) {
        const jb_noise &r = req[n == 1 ? 0 : u];
        if (noise_none(*(const NoiseSpec *)&r))
            continue;
        items[u] = noise_resolve(r, r.flags & kNoiseVary, call_k ? call_k[u] : u,
                                 r.kind == kNoiseBed ? beds.find(r.bed, r.bed_len, r.hz) : -1);
        any = true;
    }
    if (beds.words() > kNoiseMaxBeds) {
        set_error("jb_batch_set_noise: the distinct beds hold more than 2^26 samples");
        return JB_ERR_UNSUPPORTED;
    }
    if (!any)
        items.clear();
    noise_beds = std::move(beds);
    noise_req = std::move(items);
    replan();
    return JB_OK;
}

// The limiter request `req` ([B], empty: none) under the groups `group` ([B], empty: none): the members of a group
// agree on the options, else JB_ERR_INVALID naming the group and the field
int OutputChain::check_limiter_groups(const std::vector<uint32_t> &group, const std::vector<LimOpts> &req,
                                      const char *who) const
{
    if (group.empty() || req.empty())
        return JB_OK;
    std::map<uint32_t, size_t> first;
    for (size_t u = 0; u < group.size(); u++) {
        if (group[u] == kLnNoGroup)
            continue;
        const auto it = first.emplace(group[u], u).first;
        const LimOpts &a = req[it->second], &c = req[u];
        const char *field = a.flags != c.flags                         ? "limiter's flags"
                            : a.lookahead_ms != c.lookahead_ms         ? "limiter's lookahead_ms"
                            : a.hold_ms != c.hold_ms                   ? "limiter's hold_ms"
                            : a.max_reduction_db != c.max_reduction_db ? "limiter's max_reduction_db"
                                                                       : nullptr;
        if (field) {
            set_error(std::string(who) + ": the members of loudness group " + std::to_string(group[u]) +
                      " would disagree on the " + field);
            return JB_ERR_INVALID;
        }
    }
    return JB_OK;
}

int OutputChain::set_limiter(const jb_limiter_opts *opts, size_t n)
{
    // (the values first: a refused request has touched nothing)
    const size_t B = (size_t)b.B;
    std::vector<LimOpts> req;
    int rc;
    if (opts || n) {
        if (!opts || (n != 1 && n != B)) {
            set_error("jb_batch_set_limiter: give one request, or one per utterance");
            return JB_ERR_INVALID;
        }
        req.resize(B);
        for (size_t u = 0; u < B; u++)
            if ((rc = limiter_check(&opts[n == 1 ? 0 : u], u, "jb_batch_set_limiter", &req[u])))
                return rc;
    }
    if ((rc = check_settable("jb_batch_set_limiter: the limiter is set before the batch's first run")) ||
        (rc = check_limiter_groups(ln_group_req, req, "jb_batch_set_limiter")))
        return rc;
    lim_req = std::move(req);
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

// At the first run (a second one, or the step done again behind a resident-GV formation timeout, finds it done).
// The vocoder is pointed at its slab last: a failure leaves the batch as it was created, its blocks the batch's own
int OutputChain::prepare()
{
    if (ready)
        return JB_OK;
    int rc;
    if (fr_on && !fb_on && !mf_on) {
        set_error("jb_batch_set_frame_opts: the frame request stands beside jb_batch_set_fbank or jb_batch_set_mfcc");
        return JB_ERR_INVALID;
    }
    if ((rc = check_frame(fr_on ? &fr_p : nullptr, fb_on ? &fb_p : nullptr, mf_on ? &mf_fb : nullptr, &mf_p,
                          "jb_batch_set_frame_opts")))
        return rc;
    if (act_on && !activity()) // (a rate or a programme request set behind the activity request)
        return activity_fault("jb_batch_set_activity");
    frozen = true;
    for (size_t s = 0; s < (size_t)OutSlab::Count; s++)
        if (plan.alloc[s] && (rc = b.dalloc_bytes(&slab[s], (size_t)plan.alloc[s] * out_slab_elem((OutSlab)s), false)))
            return rc;
    if ((rc = prepare_resample()) || (rc = prepare_fir()) || (rc = prepare_noise()) || (rc = prepare_filter()) || (rc = prepare_loudness()) || (rc = prepare_limiter()) ||
        (rc = prepare_programme()) ||
        (rc = prepare_flac()) || (rc = prepare_format()) || (rc = prepare_adpcm()) ||
        (rc = prepare_fbank()) || (rc = prepare_mfcc()) || (rc = prepare_melspec()) || (rc = prepare_pitch()) || (rc = prepare_activity()))
        return rc;
    if (plan.active()) {
        void *voc = slab[(size_t)plan.vocoder.slab];
        b.vd.pcm = plan.vocoder.i16 ? nullptr : (double *)voc;
        b.vd.pcm16 = plan.vocoder.i16 ? (int16_t *)voc : nullptr;
    }
    ready = true;
    return JB_OK;
}

// A run launches every stage of the plan, a redo those that have something to do again: every list of a redo is
// uploaded (select_X) before its first launch, and one wait ends it
int OutputChain::enqueue(const std::vector<uint8_t> *only)
{
    if (!ready || !(plan.active() || flac_on || formatted() || adpcm() || fbank() || mfcc() || melspec() || pitch() || joined() || activity()))
        return JB_OK;
    const bool redo = only != nullptr;
    static const LnGroups no_groups;
    const RedoScope of_redo =
        redo ? redo_scope(plan.prog_of, plan.n_progs, grouped() ? ln_groups : no_groups, *only, plan.unit_parent)
             : RedoScope{};
    const RedoScope *scope = redo ? &of_redo : nullptr;
    int rc;
    if ((rc = select_resample(scope)) || (rc = select_fir(scope)) || (rc = select_noise(scope)) || (rc = select_filter(scope)) || (rc = select_loudness(scope)) ||
        (rc = select_limiter(scope)) || (rc = select_programme(scope)) || (rc = select_activity(scope)) || (rc = select_flac(scope)) || (rc = select_format(scope)) ||
        (rc = select_adpcm(scope)) || (rc = select_fbank(scope)) || (rc = select_mfcc(scope)) ||
        (rc = select_melspec(scope)) || (rc = select_pitch(scope)))
        return rc;
    // (an empty list is not uploaded: a redo that selects nothing has not touched the device)
    if (redo && !(rs.tiles.n || fir.direct.n || fir.part.n || noi.utts.n || fil.utts.n || ln.utts.n || ln.apply.n || lim.utts.n || pg.spans.n || act.cols.n || fl.work.n || fm.utts.n || ad.utts.n || fb.list.n || mf.utts.n || ml.pass.list.n || pt.utts.n))
        return JB_OK;
    if ((rc = launch_resample(redo)) || (rc = launch_fir(redo)) || (rc = launch_noise(redo)) || (rc = launch_filter(redo)) || (rc = launch_loudness(redo)) ||
        (rc = launch_limiter(redo)) || (rc = launch_programme(redo)) || (rc = launch_activity(redo)) || (rc = launch_flac(redo)) || (rc = launch_format(redo)) ||
        (rc = launch_adpcm(redo)) || (rc = launch_fbank(redo)) || (rc = launch_mfcc(redo)) ||
        (rc = launch_melspec(redo)) || (rc = launch_pitch(redo)))
        return rc;
    hipError_t e;
    if (redo && (e = hipStreamSynchronize(b.stream_voc)) != hipSuccess)
        return hip_fail(e, "output chain(redo)");
    return JB_OK;
}

static const char *const kRedoLists = "output chain(redo lists)";

// The picked entries of a run's list, each numbered (its field `base`) from the picked ones in front of it
template <class T> static std::vector<T> renumbered(const std::vector<T> &all, const Picked &p, uint64_t T::*base)
{
    std::vector<T> sub;
    for (size_t i = 0; i < p.index.size(); i++) {
        sub.push_back(all[p.index[i]]);
        sub.back().*base = p.base[i];
    }
    return sub;
}

// ---- the converter.  One table per distinct rate (native utterances go through the identity table: a copy, or the
// 16-bit conversion alone) and the tiles, reading the vocoder's f64 and writing the converter's slab
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
    std::vector<ResampleTile> &tiles = rs.tiles.host;
    int rc;
    tiles.clear();
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
        rs.tile_lo[u] = (uint32_t)tiles.size();
        resample_tiles(tables[t], (uint32_t)t, src + (size_t)b.frame_off[u] * b.voice.fperiod,
                       (uint64_t)b.T[u] * b.voice.fperiod, dst + w.off * elem, w.n, tiles);
    }
    rs.tile_lo[B] = (uint32_t)tiles.size();
    const size_t nt = std::max<size_t>(tiles.size(), 1);
    if ((rc = b.dalloc(&rs.tables_dev, tables.size(), false)) || (rc = rs.tiles.alloc(b, nt, nt)) ||
        (rc = upload_list(rs.tables_dev, tables, "resample work list")))
        return rc;
    return rs.tiles.upload("resample work list");
}

int OutputChain::select_resample(const RedoScope *scope)
{
    if (!plan.convert || !scope)
        return rs.tiles.take_all();
    const std::vector<uint8_t> &mask = scope->measured; // a tile reads the vocoder's PCM of its own utterance alone
    std::vector<ResampleTile> sub; // (a tile says where it reads and writes: nothing to renumber)
    for (size_t u = 0; u < mask.size(); u++)
        if (mask[u])
            sub.insert(sub.end(), rs.tiles.host.begin() + rs.tile_lo[u], rs.tiles.host.begin() + rs.tile_lo[u + 1]);
    return rs.tiles.upload_redo(sub, kRedoLists);
}

int OutputChain::launch_resample(bool redo)
{
    if (!plan.convert || (redo && !rs.tiles.n))
        return JB_OK;
    const hipError_t e =
        jb::launch_resample(rs.tables_dev, rs.tiles.list, rs.tiles.n, plan.converter.i16, rs.lds, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "k_resample(redo)" : "k_resample");
}

// ---- the filter: behind the converter (its second pass too), in front of the measurement.  The classes (one table
// per distinct filter and rate; utterances without sections share the identity), the utterance list sorted by
// section count and the per-tile state scratch: the f64 of the stage in front in, the filter's slab out
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
    // (with a convolution or a noise request alone every utterance is in the identity class)
    const std::vector<jb_filter> none(filt_req.empty() ? B : 0, jb_filter{});
    int rc = filter_classes(filt_req.empty() ? none.data() : filt_req.data(), B, hz.data(), B, &fil.classes, &cls_of,
                            "jb_batch_set_filter");
    if (rc)
        return rc;
    // behind a response or a noise request the sections read the f64 of the sub-stage in front (fir.mid); an utterance
    // with one of the two and no section is theirs alone
    auto fronted = [&](size_t u) { return (!fir.has.empty() && fir.has[u]) || (!noi.has.empty() && noi.has[u]); };
    if (!fir.has.empty() || !noi.has.empty()) {
        fil.mine.assign(B, 1);
        for (size_t u = 0; u < B; u++)
            fil.mine[u] = !(fronted(u) && fil.classes[cls_of[u]].ns == 0);
    }
    fil.utts.host.assign(B, FilterUtt{});
    uint64_t tiles = 0;
    for (size_t u = 0; u < B; u++) {
        const OutUtt &o = plan.utt[u];
        const uint64_t nt = filter_tiles(o.n);
        if (nt > kFiltMaxTiles) {
            set_error("filter: utterance " + std::to_string(u) + " is too long");
            return JB_ERR_UNSUPPORTED;
        }
        const double *x = fronted(u) && fil.mine[u] ? fir.mid : src;
        fil.utts.host[u] = {x + o.off, dst + o.off * elem, o.n, tiles, 0, (uint32_t)nt, cls_of[u]};
        tiles += nt;
    }
    if ((rc = filter_launch_list(fil.classes, fil.utts.host, fil.mine.empty() ? nullptr : &fil.mine, &fil.all)) ||
        (rc = b.dalloc(&fil.classes_dev, fil.classes.size(), false)) || (rc = fil.utts.alloc(b, B, B)) ||
        (rc = b.dalloc(&fil.st, (size_t)tiles * kFiltMaxD, false)) ||
        (rc = upload_list(fil.classes_dev, fil.classes, "filter work list")))
        return rc;
    return upload_list(fil.utts.dev, fil.all.utts, "filter work list");
}

int OutputChain::select_filter(const RedoScope *scope)
{
    fil.take = &fil.all;
    if (!plan.filtered() || !scope)
        return fil.utts.take_all();
    // by filter_launch_list, which also sorts and renumbers: a recursive filter carries a changed sample to the
    // utterance's end, so every touched utterance whole
    std::vector<uint8_t> mask = scope->measured;
    for (size_t u = 0; u < fil.mine.size(); u++)
        mask[u] = mask[u] && fil.mine[u];
    const int rc = filter_launch_list(fil.classes, fil.utts.host, &mask, &fil.sub);
    fil.take = &fil.sub;
    return rc ? rc : fil.utts.upload_redo(fil.sub.utts, kRedoLists);
}

int OutputChain::launch_filter(bool redo)
{
    if (!plan.filtered() || (redo && !fil.utts.n))
        return JB_OK;
    const hipError_t e =
        jb::launch_filter(fil.classes_dev, fil.utts.list, *fil.take, fil.st, plan.filter.i16, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "filter(redo)" : "filter");
}

// ---- the convolution: in the filter stage's place, in front of its sections.  An utterance with a response and no
// section: the stage's input in, the stage's slab out; with both: out to an f64 slab of the chain's own, which the
// sections then read.  The distinct responses' tables, the two launch lists and the spectrum scratch (16 bytes per bin,
// Bk + 1 bins per block of Bk samples of every partitioned utterance)
int OutputChain::prepare_fir()
{
    if (fir_of.empty() || !plan.filtered())
        return JB_OK;
    const size_t B = (size_t)b.B;
    const double *src = (const double *)slab[(size_t)plan.filter_src];
    char *dst = (char *)slab[(size_t)plan.filter.slab];
    const size_t elem = plan.filter.i16 ? sizeof(int16_t) : sizeof(double);
    fir.host.assign(B, FirUtt{});
    fir.has.assign(B, 0);
    // (something follows the convolution: the noise or a section)
    auto followed = [&](size_t u) {
        return (!filt_any.empty() && filt_any[u]) || (!noise_req.empty() && noise_req[u].on);
    };
    bool both = false;
    for (size_t u = 0; u < B; u++) {
        fir.has[u] = fir_of[u] >= 0;
        both = both || (fir.has[u] && followed(u));
    }
    int rc;
    if (both && (rc = b.dalloc(&fir.mid, (size_t)plan.total, false)))
        return rc;
    uint64_t bins = 0;
    for (size_t u = 0; u < B; u++) {
        if (!fir.has[u])
            continue;
        const OutUtt &o = plan.utt[u];
        const FirGeom &g = fir_cls.resp[(size_t)fir_of[u]].g;
        const bool mid = followed(u);
        fir.host[u] = {src + o.off, mid ? (void *)(fir.mid + o.off) : (void *)(dst + o.off * elem), o.n, 0, 0, bins,
                       (uint32_t)fir_of[u], mid ? 0u : (uint32_t)plan.filter.i16};
        if (g.mode == kFirPartitioned)
            bins += fir_frames(o.n, fir_cls.resp[(size_t)fir_of[u]].delay, g.block) * (g.block + 1);
    }
    fir_launch_lists(fir_cls.resp, fir.host, fir.has, nullptr, &fir.all);
    if (fir.all.tiles > 0x7fffffffull || fir.all.frames > 0x7fffffffull) {
        set_error("convolution: too many blocks for one launch");
        return JB_ERR_UNSUPPORTED;
    }
    fir.direct.host = fir.all.direct;
    fir.part.host = fir.all.part;
    if ((rc = b.dalloc(&fir.classes_dev, fir_cls.resp.size(), false)) ||
        (rc = b.dalloc(&fir.tables, fir_cls.words(), false)) || (bins && (rc = b.dalloc(&fir.spec, (size_t)(2 * bins), false))) ||
        (rc = fir.direct.alloc(b, fir.direct.host.size(), fir.direct.host.size())) ||
        (rc = fir.part.alloc(b, fir.part.host.size(), fir.part.host.size())))
        return rc;
    std::vector<double> image;
    std::vector<FirClass> classes;
    fir_cls.bind(fir.tables, &image, &classes);
    if ((rc = upload_list(fir.tables, image, "convolution tables")) ||
        (rc = upload_list(fir.classes_dev, classes, "convolution tables")) ||
        (rc = fir.direct.upload("convolution work list")))
        return rc;
    return fir.part.upload("convolution work list");
}

int OutputChain::select_fir(const RedoScope *scope)
{
    if (fir.has.empty())
        return JB_OK;
    if (!scope) {
        fir.frames = fir.all.frames;
        fir.direct.take_all(fir.all.tiles);
        return fir.part.take_all(fir.all.blocks);
    }
    // every touched utterance whole: a changed sample reaches K - 1 samples on, and the blocks behind it
    fir_launch_lists(fir_cls.resp, fir.host, fir.has, &scope->measured, &fir.sub);
    fir.frames = fir.sub.frames;
    const int rc = fir.direct.upload_redo(fir.sub.direct, kRedoLists, fir.sub.tiles);
    return rc ? rc : fir.part.upload_redo(fir.sub.part, kRedoLists, fir.sub.blocks);
}

int OutputChain::launch_fir(bool redo)
{
    if (fir.has.empty() || !(fir.direct.n || fir.part.n))
        return JB_OK;
    const hipError_t e = jb::launch_fir(fir.classes_dev, fir.direct.list, fir.direct.n, fir.direct.total, fir.part.list,
                                        fir.part.n, fir.part.total, fir.frames, fir.spec, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "convolution(redo)" : "convolution");
}

// ---- the noise: behind the convolution, in front of the sections.  Of an utterance's three sub-stages (response,
// noise, sections) the last writes the stage's slab, the ones in front write f64 to fir.mid: the noise reads the
// stage's input, or fir.mid behind a response; it writes the stage's slab, or fir.mid in front of a section -- behind a
// response and in front of a section the apply pass rewrites fir.mid in place (a sample depends on its own index
// alone; the sums pass only reads).  The beds' image, the launch list, the sum scratch (16 bytes per 1,024 samples,
// where the full run's numbering put it) and the records
int OutputChain::prepare_noise()
{
    if (noise_req.empty() || !plan.filtered())
        return JB_OK;
    const size_t B = (size_t)b.B;
    const double *src = (const double *)slab[(size_t)plan.filter_src];
    char *dst = (char *)slab[(size_t)plan.filter.slab];
    const size_t elem = plan.filter.i16 ? sizeof(int16_t) : sizeof(double);
    noi.host.assign(B, NoiseUtt{});
    noi.has.assign(B, 0);
    auto followed = [&](size_t u) { return !filt_any.empty() && filt_any[u]; };
    bool mid_needed = false;
    for (size_t u = 0; u < B; u++) {
        noi.has[u] = noise_req[u].on;
        mid_needed = mid_needed || (noi.has[u] && followed(u));
    }
    int rc;
    if (mid_needed && !fir.mid && (rc = b.dalloc(&fir.mid, (size_t)plan.total, false)))
        return rc;
    if ((rc = b.dalloc(&noi.beds, (size_t)noise_beds.words(), false)) || (rc = b.dalloc(&noi.rec, B, false)))
        return rc;
    std::vector<double> image;
    std::vector<NoiseBed> beds;
    noise_beds.bind(noi.beds, &image, &beds);
    uint64_t tiles = 0;
    for (size_t u = 0; u < B; u++) {
        if (!noi.has[u])
            continue;
        const OutUtt &o = plan.utt[u];
        const NoiseItem &it = noise_req[u];
        const bool behind = !fir.has.empty() && fir.has[u], mid = followed(u);
        NoiseUtt w{};
        w.x = (behind ? fir.mid : src) + o.off;
        w.y = mid ? (void *)(fir.mid + o.off) : (void *)(dst + o.off * elem);
        w.bed = it.bed >= 0 ? beds[(size_t)it.bed].w : nullptr;
        w.n = o.n;
        w.s0 = tiles;
        w.mseed = fmt_mix(it.seed);
        w.r = it.r;
        w.q = it.q;
        w.lb = it.bed >= 0 ? beds[(size_t)it.bed].len : 0;
        w.offset = it.offset;
        w.active = it.active;
        w.i16 = mid ? 0u : (uint32_t)plan.filter.i16;
        w.rep = (uint32_t)u;
        noi.host[u] = w;
        tiles += noise_tiles(o.n);
    }
    noise_launch_list(noi.host, noi.has, nullptr, &noi.all);
    if (noi.all.tiles > 0x7fffffffull) {
        set_error("noise: too many tiles for one launch");
        return JB_ERR_UNSUPPORTED;
    }
    noi.utts.host = noi.all.utts;
    if ((rc = b.dalloc(&noi.sums, (size_t)(2 * tiles), false)) ||
        (rc = noi.utts.alloc(b, noi.utts.host.size(), noi.utts.host.size())) ||
        (rc = upload_list(noi.beds, image, "noise beds")))
        return rc;
    return noi.utts.upload("noise work list");
}

int OutputChain::select_noise(const RedoScope *scope)
{
    if (noi.has.empty())
        return JB_OK;
    if (!scope) {
        noi.tiles = noi.all.tiles;
        noi.apply = noi.all.apply;
        return noi.utts.take_all();
    }
    // every touched utterance whole: one changed sample changes the power, the gain and so every sample
    noise_launch_list(noi.host, noi.has, &scope->measured, &noi.sub);
    noi.tiles = noi.sub.tiles;
    noi.apply = noi.sub.apply;
    return noi.utts.upload_redo(noi.sub.utts, kRedoLists);
}

int OutputChain::launch_noise(bool redo)
{
    if (noi.has.empty() || !noi.utts.n)
        return JB_OK;
    const hipError_t e =
        jb::launch_noise(noi.utts.list, noi.utts.n, noi.tiles, noi.apply, noi.sums, noi.rec, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "noise(redo)" : "noise");
}

// ---- loudness.  The per-rate tables and the utterance list: the measurement reads the f64 of the stage in front,
// the apply pass writes x * g to its own slab
int OutputChain::prepare_loudness()
{
    if (!plan.normalize())
        return JB_OK;
    const size_t B = (size_t)b.B;
    const double *src = (const double *)slab[(size_t)plan.measure];
    char *dst = (char *)slab[(size_t)plan.apply.slab];
    const size_t elem = plan.apply.i16 ? sizeof(int16_t) : sizeof(double);
    std::vector<LoudnessRate> rates;
    ln.utts.host.assign(B, LoudnessUtt{});
    ln.ntiles.assign(B, 0);
    ln.natiles.assign(B, 0);
    ln.tiles = ln.atiles = 0;
    int rc;
    for (size_t u = 0; u < B; u++) {
        const OutUtt &o = plan.utt[u];
        size_t r = 0;
        while (r < rates.size() && rates[r].hz != o.hz)
            r++;
        if (r == rates.size()) {
            LoudnessRate lr{};
            if ((rc = loudness_measurable(o.hz)) || (rc = loudness_rate(o.hz, &lr)))
                return rc;
            rates.push_back(lr);
        }
        LoudnessUtt &w = ln.utts.host[u];
        w.x = src + o.off;
        w.y = dst + o.off * elem;
        w.n = o.n;
        ln.ntiles[u] = w.ntiles = loudness_tiles(rates[r], w.n);
        ln.natiles[u] = (w.n + kLnApplyTile - 1) / kLnApplyTile;
        w.tile0 = w.lt0 = ln.tiles;
        w.at0 = ln.atiles;
        w.rate = (uint32_t)r;
        w.slot = (uint32_t)u;
        w.target = ln_target[u];
        // (with a limiter the static gain may put the highest peak max_reduction_db over the ceiling: the gates read
        // that as their ceiling, the limiter's own list carries the real one)
        w.ceiling = limits(u) ? ln_ceiling[u] + lim_req[u].max_reduction_db : ln_ceiling[u];
        w.mode = peak_mode(u);
        ln.true_peak = ln.true_peak || w.mode == JB_PEAK_TRUE;
        ln.tiles += ln.ntiles[u];
        ln.atiles += ln.natiles[u];
    }
    const size_t nt = (size_t)std::max<uint64_t>(ln.tiles, 1);
    if ((rc = b.dalloc(&ln.rates_dev, rates.size(), false)) || (rc = ln.utts.alloc(b, B, B)) ||
        (rc = b.dalloc(&ln.st, 4 * nt, false)) || (rc = b.dalloc(&ln.pk, nt, false)) ||
        (rc = b.dalloc(&ln.z, nt, false)) || (rc = b.dalloc(&ln.res, B, false)) ||
        (ln.true_peak && (rc = b.dalloc(&ln.tp, nt, false))) ||
        (rc = upload_list(ln.rates_dev, rates, "loudness work list")) || (rc = ln.utts.upload("loudness work list")))
        return rc;
    // with a group or a report request: the sets (every utterance, then every group) and what their kernels write
    const size_t G = ln_groups.size();
    const bool with_groups = !ln_group_req.empty();
    if ((!with_groups && !ln_report) || B == 0)
        return JB_OK;
    ln.sets.host.assign(B + G, LoudnessSet{});
    std::vector<uint32_t> members(with_groups ? 2 * B : B);
    for (size_t u = 0; u < B; u++) {
        ln.sets.host[u] = LoudnessSet{(uint32_t)u, 1, (uint32_t)u, (uint32_t)u};
        members[u] = (uint32_t)u;
        if (with_groups)
            members[B + u] = ln_groups.members[u];
    }
    for (size_t g = 0; g < G; g++)
        ln.sets.host[B + g] = LoudnessSet{(uint32_t)B + ln_groups.first[g], ln_groups.first[g + 1] - ln_groups.first[g],
                                          (uint32_t)g, (uint32_t)(B + g)};
    if ((rc = ln.sets.alloc(b, B + G, B + G)) || (rc = b.dalloc(&ln.members_dev, members.size(), false)) ||
        (with_groups && ((rc = b.dalloc(&ln.gres, G, false)) || (rc = b.dalloc(&ln.apply.redo, B, false)))) ||
        (ln_report && ((rc = b.dalloc(&ln.sw, nt, false)) || (rc = b.dalloc(&ln.mm, B, false)) ||
                       (rc = b.dalloc(&ln.r128, B + G, false)))) ||
        (rc = ln.sets.upload("loudness group list")))
        return rc;
    return upload_list(ln.members_dev, members, "loudness group list");
}

int OutputChain::select_loudness(const RedoScope *scope)
{
    const bool report = plan.normalize() && ln.r128;
    if (!plan.normalize() || !scope) {
        ln.utts.take_all(ln.tiles);
        ln.apply.list = ln.utts.dev, ln.apply.n = ln.utts.n, ln.apply.total = ln.atiles;
        ln.sets.take_all();
        ln.n_usets = ln.utts.n;
        return JB_OK;
    }
    // The measurement and the utterances' report sets: an utterance's samples in front of the apply pass depend on
    // nothing but its own.  An utterance of zero samples stays in the list: its result is written like any other.
    // (This list's at0 is read only where the apply pass takes it too: without groups)
    const std::vector<uint8_t> &mask = scope->measured;
    const Picked m = pick_renumbered(mask, ln.ntiles), ma = pick_renumbered(mask, ln.natiles);
    std::vector<LoudnessUtt> sub = renumbered(ln.utts.host, m, &LoudnessUtt::lt0); // (the scratch, tile0, stays)
    std::vector<LoudnessSet> set_sub;
    for (size_t i = 0; i < sub.size(); i++) {
        sub[i].at0 = ma.base[i];
        if (report)
            set_sub.push_back(ln.sets.host[m.index[i]]);
    }
    ln.n_usets = (uint32_t)set_sub.size();
    int rc = ln.utts.upload_redo(sub, kRedoLists, m.total);
    if (rc)
        return rc;
    ln.apply.list = ln.utts.redo, ln.apply.n = ln.utts.n, ln.apply.total = ma.total;
    if (grouped()) {
        // the apply pass: a group's gain reaches every member; the groups' sets: those with a measured member
        const std::vector<uint8_t> &apply_mask = scope->post, &group_mask = scope->touched_groups;
        const Picked a = pick_renumbered(apply_mask, ln.natiles);
        for (size_t g = 0; g < group_mask.size(); g++)
            if (group_mask[g])
                set_sub.push_back(ln.sets.host[(size_t)b.B + g]);
        if ((rc = ln.apply.upload_redo(renumbered(ln.utts.host, a, &LoudnessUtt::at0), kRedoLists, a.total)))
            return rc;
    }
    return ln.sets.upload_redo(set_sub, kRedoLists);
}

// The measurement, the groups' gate over the measured members' scratch, the report, then one gain for every member
int OutputChain::launch_loudness(bool redo)
{
    if (!plan.normalize() || (redo && !ln.utts.n))
        return JB_OK;
    hipStream_t st = b.stream_voc;
    const bool report = ln.r128 != nullptr;
    hipError_t e;
    if ((e = launch_loudness_measure(ln.rates_dev, ln.utts.list, ln.utts.n, ln.utts.total, ln.st, ln.pk, ln.tp, ln.z,
                                     ln.res, ln.true_peak, st)) != hipSuccess ||
        (grouped() && (e = launch_loudness_groups(ln.rates_dev, ln.utts.dev, ln.sets.list + ln.n_usets,
                                                  ln.sets.n - ln.n_usets, ln.members_dev, ln.z, ln.res, ln.gres, st)) !=
                          hipSuccess) ||
        (report && (e = launch_loudness_range(ln.rates_dev, ln.utts.list, ln.utts.n, ln.utts.dev, ln.sets.list,
                                              ln.sets.n, ln.members_dev, ln.z, ln.sw, ln.mm, ln.r128, st)) !=
                       hipSuccess) ||
        (!limited() &&
         (e = launch_loudness_apply(ln.apply.list, ln.apply.n, ln.apply.total, ln.res, plan.apply.i16, st)) != hipSuccess))
        return hip_fail(e, redo ? "loudness(redo)" : "loudness");
    return JB_OK;
}

// ---- the limiter: with a request, in the place of the apply pass (same input, same slab out, the gain read from the
// loudness results).  The classes, the utterance list and the per-tile scratch; an utterance without a finite ceiling
// is listed as the plain apply pass
int OutputChain::prepare_limiter()
{
    if (!limited())
        return JB_OK;
    const size_t B = (size_t)b.B;
    LimiterClasses classes;
    lim.utts.host.assign(B, LimiterUtt{});
    lim.ntiles.assign(B, 0);
    lim.L.assign(B, 0);
    lim.H.assign(B, 0);
    lim.tiles = 0;
    int rc;
    for (size_t u = 0; u < B; u++) {
        const LoudnessUtt &m = ln.utts.host[u];
        uint32_t cls = kLimNoSlot;
        if (limits(u) && ((rc = limiter_geometry(lim_req[u], plan.utt[u].hz, u, "limiter", &lim.L[u], &lim.H[u])) ||
                          (rc = classes.find(plan.utt[u].hz, lim.L[u], lim.H[u], m.mode, &cls))))
            return rc;
        lim.ntiles[u] = limiter_tiles(m.n);
        lim.utts.host[u] = LimiterUtt{m.x, m.y, m.n, lim.tiles, lim.tiles, limits(u) ? lim_ceiling(ln_ceiling[u]) : 0.0,
                                      1.0, m.slot, cls, (uint32_t)u, 0};
        lim.tiles += lim.ntiles[u];
    }
    if ((rc = b.dalloc(&lim.classes_dev, classes.tables.size(), false)) || (rc = lim.utts.alloc(b, B, B)) ||
        (rc = b.dalloc(&lim.scratch, (size_t)lim.tiles, false)) || (rc = b.dalloc(&lim.res, B, false)) ||
        (rc = upload_list(lim.classes_dev, classes.tables, "limiter work list")))
        return rc;
    return lim.utts.upload("limiter work list");
}

int OutputChain::select_limiter(const RedoScope *scope)
{
    if (!limited() || !scope)
        return lim.utts.take_all(lim.tiles);
    // `post`: every utterance whose gain or samples changed (the scratch place, s0, stays)
    const Picked p = pick_renumbered(scope->post, lim.ntiles);
    return lim.utts.upload_redo(renumbered(lim.utts.host, p, &LimiterUtt::t0), kRedoLists, p.total);
}

int OutputChain::launch_limiter(bool redo)
{
    if (!limited() || (redo && !lim.utts.n))
        return JB_OK;
    const hipError_t e = jb::launch_limiter(lim.classes_dev, lim.utts.list, lim.utts.n, lim.utts.total, ln.res,
                                            lim.scratch, lim.res, plan.apply.i16, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "k_ln_limit(redo)" : "k_ln_limit");
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

// ---- the programmes, a join's or a mix's: behind everything that writes the final PCM, in front of everything that
// encodes it.  The members, the segments and their lists from the layout (mix_layout, as the plan formed it) and one
// span per programme; with a mix the peak scratch and the results
int OutputChain::prepare_programme()
{
    if (!joined())
        return JB_OK;
    const size_t B = (size_t)b.B, U = plan.units.size(); // the units: the programmes, and a mix's stems behind them
    const size_t elem = plan.join.i16 ? sizeof(int16_t) : sizeof(double);
    std::vector<uint64_t> n(B), xoff(B);
    for (size_t u = 0; u < B; u++) {
        n[u] = plan.utt[u].n;
        xoff[u] = plan.utt[u].off;
    }
    MixLayout lay;
    const bool stems = mixed() && !stem_req.empty();
    int rc = mix_layout_checked(prog_req.data(), prog_chained, n.data(), nullptr, B, elem, mixed() ? &mix_opts : nullptr,
                                &lay, mixed() ? "jb_batch_set_mix" : "jb_batch_set_join",
                                stems ? stem_req.data() : nullptr);
    if (rc)
        return rc;
    if (lay.units.size() != U) {
        set_error("programmes: the plan and the layout disagree");
        return JB_ERR_INVALID;
    }
    mix_lists(lay, prog_req.data(), n.data(), xoff.data(), slab[(size_t)plan.join_src.slab], slab[(size_t)plan.join.slab],
              elem, &pg.members, &pg.spans.host, &pg.tiles);
    pg.member_at.assign(B, 0);
    for (size_t i = 0; i < B; i++)
        pg.member_at[lay.progs.members[i]] = (uint32_t)i;
    ProgMember *md = nullptr;
    // (a join's redo lists at most one span per member, a mix's one per programme)
    if ((rc = b.dalloc(&md, B, false)) || (rc = pg.spans.alloc(b, U, mixed() ? U : B)) ||
        (rc = upload_list(md, pg.members, mixed() ? "mix work list" : "join work list")))
        return rc;
    pg.L.members = md;
    if (mixed()) { // (the join's kernel reads the members alone)
        MixSeg *sd = nullptr;
        uint32_t *ld = nullptr;
        if ((rc = b.dalloc(&sd, lay.segs.size(), false)) || (rc = b.dalloc(&ld, lay.lists.size(), false)) ||
            (rc = b.dalloc(&pg.L.tile_peak, pg.tiles * kMixWaves, false)) || (rc = b.dalloc(&pg.L.res, U, false)) ||
            (rc = upload_list(sd, lay.segs, "mix work list")) || (rc = upload_list(ld, lay.lists, "mix work list")))
            return rc;
        pg.L.segs = sd;
        pg.L.lists = ld;
        pg.L.fit = (mix_opts.flags & kMixFit) != 0;
        pg.L.ceiling = pg.L.fit ? mix_ceiling(mix_opts.ceiling_db) : 0.0;
    }
    if (stems && (stem_flags & kMixStemLevels)) {
        uint64_t scratch = 0;
        // (what a redo's items are built from: the units, the stems and the programmes' count; the segments and their
        // lists are on the device and not kept)
        pg.lay = MixLayout{};
        pg.lay.progs.first = lay.progs.first;
        pg.lay.units = lay.units;
        pg.lay.stems = lay.stems;
        mix_level_items(lay, slab[(size_t)plan.join.slab], elem, {}, &pg.items.host, &pg.level_tiles, &scratch);
        if ((rc = pg.items.alloc(b, U, U)) || (rc = b.dalloc(&pg.tile_sums, 2 * scratch, false)) ||
            (rc = b.dalloc(&pg.sums, U, false)) || (rc = pg.items.upload("mix level list")))
            return rc;
    }
    return pg.spans.upload(mixed() ? "mix work list" : "join work list");
}

// A redo of a mix runs every programme with a member whose final PCM changed again, whole: the sum, the peak and the
// fit.  A redo of a join runs each changed member's own range alone, widened to whole groups of kProgGroupBytes (the
// samples around it are what they were: its neighbours' current ones, and pads)
int OutputChain::select_programme(const RedoScope *scope)
{
    // (the stems stand behind the programmes in every list, a redo's too: the launch counts them from its end)
    const size_t NP = plan.n_progs;
    auto count_stems = [&](const std::vector<ProgSpan> &list) {
        pg.L.stems = 0;
        pg.L.stem_tiles = 0;
        for (const ProgSpan &w : list)
            if (w.prog >= NP) {
                pg.L.stems++;
                pg.L.stem_tiles += prog_tiles(w.k0, w.k1, plan.join.i16);
            }
    };
    if (!joined() || !scope) {
        if (joined() && mixed()) {
            count_stems(pg.spans.host);
            pg.items.take_all(pg.level_tiles);
        }
        return pg.spans.take_all(pg.tiles);
    }
    std::vector<ProgSpan> sub;
    uint64_t tiles = 0;
    auto take = [&](size_t p, uint64_t k0, uint64_t k1) {
        sub.push_back(pg.spans.host[p]);
        sub.back().k0 = k0;
        sub.back().k1 = k1;
        sub.back().t0 = tiles; // (pk0 stays: the programme's tiles in the peak scratch)
        tiles += prog_tiles(k0, k1, plan.join.i16);
    };
    if (mixed()) {
        for (size_t p = 0; p < scope->units.size(); p++)
            if (scope->units[p])
                take(p, 0, plan.units[p].n);
        count_stems(sub);
        if (pg.sums) { // the levels of the touched programmes and of their stems, again
            std::vector<LevelItem> items;
            uint64_t lt = 0;
            mix_level_items(pg.lay, slab[(size_t)plan.join.slab], plan.join.i16 ? sizeof(int16_t) : sizeof(double),
                            scope->units, &items, &lt, nullptr);
            const int rc = pg.items.upload_redo(items, kRedoLists, lt);
            if (rc)
                return rc;
        }
    } else {
        const std::vector<uint8_t> &mask = scope->post; // every utterance whose final PCM changed
        const uint64_t gs = kProgGroupBytes / (plan.join.i16 ? sizeof(int16_t) : sizeof(double));
        for (size_t u = 0; u < mask.size(); u++) {
            if (!mask[u] || !plan.utt[u].n) // a member of zero samples wrote nothing into its programme: no span
                continue;
            const ProgMember &m = pg.members[pg.member_at[u]];
            take(plan.prog_of[u], m.start / gs * gs,
                 std::min<uint64_t>((m.start + m.n + gs - 1) / gs * gs, plan.units[plan.prog_of[u]].n));
        }
    }
    return pg.spans.upload_redo(sub, kRedoLists, tiles);
}

int OutputChain::launch_programme(bool redo)
{
    if (!joined() || (redo && !pg.spans.n))
        return JB_OK;
    const hipError_t e =
        mixed() ? jb::launch_mix(plan.join.i16, pg.spans.list, pg.spans.n, pg.spans.total, pg.L, b.stream_voc)
                : jb::launch_join(plan.join.i16, pg.spans.list, pg.spans.n, pg.spans.total, pg.L.members, b.stream_voc);
    if (e == hipSuccess && mixed() && pg.sums) {
        const hipError_t el = jb::launch_mix_levels(plan.join.i16, pg.items.list, pg.items.n, pg.items.total,
                                                    pg.tile_sums, pg.sums, b.stream_voc);
        if (el != hipSuccess)
            return hip_fail(el, redo ? "k_mix_levels(redo)" : "k_mix_levels");
    }
    if (e == hipSuccess)
        return JB_OK;
    return mixed() ? hip_fail(e, redo ? "k_mix(redo)" : "k_mix") : hip_fail(e, redo ? "k_join(redo)" : "k_join");
}

// ---- the speech-activity labels: behind the programmes, beside the encoders.  One column per member on the member's
// own final PCM (what the join reads), or one per unit on the unit's PCM (what the encoders read); the places from the
// plan (act_layout)
int OutputChain::prepare_activity()
{
    if (!activity())
        return JB_OK;
    const ActLayout &lay = plan.act;
    const size_t U = lay.units.size(), NC = lay.cols.size();
    const size_t elem = plan.act_src.i16 ? sizeof(int16_t) : sizeof(double);
    const bool whole = act_p.columns == kActUnit;
    const char *src = (const char *)slab[(size_t)plan.act_src.slab];
    int rc;
    if ((rc = b.dalloc(&act.lab, std::max<uint64_t>(lay.bytes, 16), false)) ||
        (rc = b.dalloc(&act.en, std::max<uint64_t>(lay.energies, 1), false)) ||
        (lay.words && (rc = b.dalloc(&act.wd, lay.words, false))))
        return rc;
    uint8_t *lab = act.lab;
    double *en = act.en;
    uint64_t *wd = act.wd;
    const std::vector<EncUnit> units = enc_units();
    act.L = ActLaunch{act_p.grid, act_p.reference == kActRefAbs, act_p.min_speech, act_p.min_gap, act_p.hang_before,
                      act_p.hang_after};
    const double q = act_ratio(act_p.gate_db);
    act.cols.host.assign(NC, ActCol{});
    act.units.host.assign(U, ActUnit{});
    uint64_t energy_wgs = 0, unit_wgs = 0;
    for (size_t p = 0; p < U; p++) {
        const ActLayUnit &W = lay.units[p];
        act.units.host[p] = ActUnit{lab + W.off, W.T, unit_wgs, W.C, (uint32_t)p};
        unit_wgs += act_unit_wgs(W.T);
        for (uint32_t j = 0; j < W.C; j++) {
            const ActLayCol &a = lay.cols[W.col0 + j];
            ActCol &c = act.cols.host[W.col0 + j];
            c.x = src + (whole ? units[p].off : plan.utt[a.utt].off) * elem;
            c.y = lab + W.off + j;
            c.e = en + a.e0;
            c.words = act.L.smooth() ? wd + a.w0 : nullptr;
            c.start = a.start;
            c.n = a.n;
            c.T = W.T;
            c.f0 = a.f0;
            c.nf = a.nf;
            c.g0 = energy_wgs;
            c.nw = (W.T + 63) / 64;
            c.q = q;
            c.thr_abs = act_abs_threshold(act_p.gate_db, W.wl);
            c.C = W.C;
            c.wl = W.wl;
            c.hop = W.hop;
            c.col = j;
            c.slot = W.col0 + j;
            c.unit = (uint32_t)p;
            energy_wgs += act_energy_wgs(a.nf, W.wl, W.hop);
        }
    }
    act.cols.total = energy_wgs;
    act.units.total = unit_wgs;
    if ((rc = b.dalloc(&act.col_max, NC, false)) || (rc = b.dalloc(&act.rep, NC, false)) ||
        (rc = b.dalloc(&act.urep, U, false)) || (rc = act.cols.alloc(b, NC, NC)) || (rc = act.units.alloc(b, U, U)) ||
        (rc = act.cols.upload("activity work list")))
        return rc;
    return act.units.upload("activity work list");
}

// A redo measures every unit with a member whose final PCM changed again, whole: the energies, the maxima, the labels
// and the reports of all its columns
int OutputChain::select_activity(const RedoScope *scope)
{
    if (!activity() || !scope) {
        uint64_t energy_wgs = 0, unit_wgs = 0;
        for (const ActCol &c : act.cols.host)
            energy_wgs += act_energy_wgs(c.nf, c.wl, c.hop);
        for (const ActUnit &w : act.units.host)
            unit_wgs += act_unit_wgs(w.T);
        act.units.take_all(unit_wgs);
        return act.cols.take_all(energy_wgs);
    }
    std::vector<ActCol> cols;
    std::vector<ActUnit> us;
    uint64_t energy_wgs = 0, unit_wgs = 0;
    for (size_t p = 0; p < act.units.host.size() && p < scope->units.size(); p++) {
        if (!scope->units[p])
            continue;
        us.push_back(act.units.host[p]);
        us.back().g0 = unit_wgs;
        unit_wgs += act_unit_wgs(us.back().T);
        const ActLayUnit &W = plan.act.units[p];
        for (uint32_t j = 0; j < W.C; j++) {
            cols.push_back(act.cols.host[W.col0 + j]);
            cols.back().g0 = energy_wgs;
            energy_wgs += act_energy_wgs(cols.back().nf, W.wl, W.hop);
        }
    }
    const int rc = act.units.upload_redo(us, kRedoLists, unit_wgs);
    return rc ? rc : act.cols.upload_redo(cols, kRedoLists, energy_wgs);
}

int OutputChain::launch_activity(bool redo)
{
    if (!activity() || (redo && !act.cols.n))
        return JB_OK;
    const hipError_t e =
        jb::launch_activity(plan.act_src.i16, act.cols.list, act.cols.n, act.cols.total, act.units.list, act.units.n,
                            act.units.total, act.col_max, act.rep, act.urep, act.L, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "k_act(redo)" : "k_act");
}

// ---- FLAC.  The streams' lists and slabs: one stream per unit (an utterance; behind a join a programme) of the
// 16-bit slab FLAC reads, at its output rate
int OutputChain::prepare_flac()
{
    if (!flac_on)
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t U = units.size();
    std::vector<const int16_t *> xs(U);
    std::vector<uint64_t> ns(U);
    std::vector<uint32_t> hz(U);
    for (size_t u = 0; u < U; u++) {
        xs[u] = (const int16_t *)slab[(size_t)plan.flac] + units[u].off;
        ns[u] = units[u].n;
        hz[u] = units[u].hz;
    }
    std::vector<FlacUtt> utts;
    uint64_t slot_bytes = 0, bound = 0;
    int rc = flac_plan(flac_p, flac_m, xs.data(), ns.data(), hz.data(), U, &utts, &fl.work.host, &slot_bytes, &bound);
    if (rc)
        return rc;
    const bool md5 = (flac_m.flags & kFlacMetaMd5) != 0;
    if (md5)
        flac_md5_order(utts, nullptr, &fl.md5.host);
    fl.max_points = 0;
    for (const FlacUtt &w : utts)
        fl.max_points = std::max(fl.max_points, w.n_points);
    const size_t nf = std::max<size_t>(fl.work.host.size(), 1), nu = std::max<size_t>(U, 1);
    uint8_t *slots = nullptr;
    if ((rc = b.dalloc(&slots, std::max<uint64_t>(slot_bytes, 4), false)) ||
        (rc = b.dalloc(&fl.out, std::max<uint64_t>(bound, 4), false)) || (rc = b.dalloc(&fl.utts_dev, U, false)) ||
        (rc = fl.work.alloc(b, nf, nf)) || (rc = b.dalloc(&fl.fsize, nf, false)) ||
        (rc = b.dalloc(&fl.foff, nf, false)) || (rc = b.dalloc(&fl.res, U, false)) ||
        (rc = b.dalloc(&fl.total, 1, false)) ||
        (md5 && ((rc = fl.md5.alloc(b, nu, nu)) || (rc = b.dalloc(&fl.digests, 4 * nu, false)))))
        return rc;
    flac_bind(&utts, slots);
    if ((rc = upload_list(fl.utts_dev, utts, "FLAC work list")) || (rc = fl.work.upload("FLAC work list")) ||
        (rc = fl.md5.upload("FLAC work list")))
        return rc;
    if (md5)
        fl.utts = std::move(utts);
    return JB_OK;
}

int OutputChain::select_flac(const RedoScope *scope)
{
    if (!flac_on || !scope) {
        fl.md5.take_all();
        return fl.work.take_all();
    }
    const std::vector<uint8_t> &mask = scope->units; // every unit whose final PCM changed
    // by work item (a block says which frame of which stream it is: nothing to renumber); the digests of the same
    // units where a block is encoded again (a unit without frames keeps its digest of no samples)
    std::vector<FlacWork> sub;
    std::vector<uint32_t> md5_sub;
    for (const FlacWork &w : fl.work.host)
        if (mask[w.utt])
            sub.push_back(w);
    if (fl.digests && !sub.empty())
        flac_md5_order(fl.utts, &mask, &md5_sub);
    const int rc = fl.work.upload_redo(sub, kRedoLists);
    return rc ? rc : fl.md5.upload_redo(md5_sub, kRedoLists);
}

// The blocks of the list, the digests of its units' now final PCM (on request), then every stream's offsets, place
// and header (all of fl.work.dev, redo or not): the pack never sees a digest of replaced PCM
int OutputChain::launch_flac(bool redo)
{
    if (!flac_on || (redo && !fl.work.n))
        return JB_OK;
    hipStream_t st = b.stream_voc;
    hipError_t e;
    if ((e = launch_flac_encode(flac_p, fl.utts_dev, fl.work.list, fl.work.n, fl.fsize, st)) != hipSuccess ||
        (fl.digests && (e = launch_flac_md5(fl.utts_dev, fl.md5.list, fl.md5.n, fl.digests, st)) != hipSuccess) ||
        (e = launch_flac_pack(flac_p, fl.utts_dev, (uint32_t)num_outputs(), fl.work.dev, (uint32_t)fl.work.host.size(),
                              fl.fsize, fl.foff, fl.res, fl.total, fl.out, st, fl.digests, fl.max_points)) != hipSuccess)
        return hip_fail(e, redo ? "FLAC(redo)" : "FLAC");
    return JB_OK;
}

// ---- the sample format: behind the apply pass, the converter or the hand-off check, whichever wrote last.
// The unit list: the final f64 of the plan in, each unit's bytes at its 16-byte aligned place out
int OutputChain::prepare_format()
{
    if (!formatted())
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t U = units.size();
    const double *src = (const double *)slab[(size_t)plan.fmt_src];
    uint8_t *dst = (uint8_t *)slab[(size_t)OutSlab::Fmt];
    fm.utts.host.assign(U, FormatUtt{});
    fm.ntiles.assign(U, 0);
    fm.tiles = 0;
    for (size_t u = 0; u < U; u++) {
        FormatUtt &w = fm.utts.host[u];
        w.x = src + units[u].off;
        w.y = dst + plan.fmt[u].off;
        w.n = units[u].n;
        w.ft0 = fm.tiles;
        fm.ntiles[u] = (w.n + kFmtTile - 1) / kFmtTile;
        fm.tiles += fm.ntiles[u];
    }
    const int rc = fm.utts.alloc(b, U, U);
    return rc ? rc : fm.utts.upload("format work list");
}

int OutputChain::select_format(const RedoScope *scope)
{
    if (!formatted() || !scope)
        return fm.utts.take_all(fm.tiles);
    // `units`: every unit whose final PCM changed (one of zero samples stays in the list: it has no tile)
    const Picked p = pick_renumbered(scope->units, fm.ntiles);
    return fm.utts.upload_redo(renumbered(fm.utts.host, p, &FormatUtt::ft0), kRedoLists, p.total);
}

int OutputChain::launch_format(bool redo)
{
    if (!formatted() || (redo && !fm.utts.n))
        return JB_OK;
    const hipError_t e = jb::launch_format(fmt_p.format, fmt_p.dither, fmt_p.seed, fm.utts.list, fm.utts.n,
                                           fm.utts.total, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "k_format(redo)" : "k_format");
}

// ---- IMA ADPCM beside it, of the same final PCM.  The unit list: the final PCM of the plan in (f64 or 16-bit), each
// unit's blocks at their 16-byte aligned place out
int OutputChain::prepare_adpcm()
{
    if (!adpcm())
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t U = units.size();
    const char *src = (const char *)slab[(size_t)plan.adpcm_src.slab];
    const size_t elem = plan.adpcm_src.i16 ? sizeof(int16_t) : sizeof(double);
    uint8_t *dst = (uint8_t *)slab[(size_t)OutSlab::Adpcm];
    ad.utts.host.assign(U, AdpcmUtt{});
    ad.ngroups.assign(U, 0);
    ad.groups = 0;
    for (size_t u = 0; u < U; u++) {
        AdpcmUtt &w = ad.utts.host[u];
        w.x = src + units[u].off * elem;
        w.y = dst + plan.adpcm[u].off;
        w.n = units[u].n;
        w.g0 = ad.groups;
        w.A = plan.adpcm[u].A;
        w.spb = adpcm_spb(w.A);
        ad.ngroups[u] = (adpcm_blocks(w.n, w.A) + kAdpcmLanes - 1) / kAdpcmLanes;
        ad.groups += ad.ngroups[u];
    }
    const int rc = ad.utts.alloc(b, U, U);
    return rc ? rc : ad.utts.upload("ADPCM work list");
}

int OutputChain::select_adpcm(const RedoScope *scope)
{
    if (!adpcm() || !scope)
        return ad.utts.take_all(ad.groups);
    // `units`: every unit whose final PCM changed (one of zero samples stays in the list: it has no block)
    const Picked p = pick_renumbered(scope->units, ad.ngroups);
    return ad.utts.upload_redo(renumbered(ad.utts.host, p, &AdpcmUtt::g0), kRedoLists, p.total);
}

int OutputChain::launch_adpcm(bool redo)
{
    if (!adpcm() || (redo && !ad.utts.n))
        return JB_OK;
    const hipError_t e = jb::launch_adpcm(plan.adpcm_src.i16, ad.utts.list, ad.utts.n, ad.utts.total, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "k_adpcm(redo)" : "k_adpcm");
}

// ---- the filterbank features beside them, of the same final f64: a RatePass (jb_host.h) over the units, with the
// plan's frames.  The final PCM of the plan in, each unit's frames at their 16-byte aligned place out
int OutputChain::prepare_fbank()
{
    if (!fbank())
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t U = units.size();
    const double *src = (const double *)slab[(size_t)plan.fbank_src];
    uint8_t *dst = (uint8_t *)slab[(size_t)OutSlab::Feat];
    fb.start(fb_p, fr_on ? fr_p : FrameOpts{});
    int rc;
    for (size_t u = 0; u < U; u++) {
        if ((rc = fb.add(units[u].hz, units[u].n, "jb_batch_set_fbank", plan.fbank[u].T)))
            return rc;
        fb.list.host[u].x = src + units[u].off;
        fb.list.host[u].y = dst + plan.fbank[u].off;
    }
    if ((rc = fb.bind(b, "fbank")))
        return rc;
    return b.dalloc(&fb.list.redo, U, false);
}

// A pass's lists of a redo.  `units`: every unit whose final PCM changed, each recomputed whole (one without a frame
// stays in the list: it has no workgroup); the list is renumbered, what a unit points at stays where the full
// numbering put it
template <class Pass> static int select_pass(Pass &p, const RedoScope *scope)
{
    if (!scope)
        return p.list.take_all(p.groups);
    const Picked k = pick_renumbered(scope->units, p.ngroups);
    return p.list.upload_redo(renumbered(p.list.host, k, &Pass::Unit::g0), kRedoLists, k.total);
}

int OutputChain::select_fbank(const RedoScope *scope) { return select_pass(fb, fbank() ? scope : nullptr); }

int OutputChain::launch_fbank(bool redo)
{
    if (!fbank() || (redo && !fb.list.n))
        return JB_OK;
    const hipError_t e = fb.launch(b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "k_fbank(redo)" : "k_fbank");
}

// ---- the cepstral features beside them, of the same final f64, behind a filterbank pass of their own: k_fbank with
// f64 logarithms forced into the log-mel scratch, then the cepstral kernels on the same stream.  The statics, the
// block sums and the statistics are blocks of the stage's own, laid out by the full numbering
int OutputChain::prepare_mfcc()
{
    if (!mfcc())
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t U = units.size();
    const double *src = (const double *)slab[(size_t)plan.mfcc_src];
    double *logmel = (double *)slab[(size_t)OutSlab::MfccL];
    uint8_t *dst = (uint8_t *)slab[(size_t)OutSlab::Mfcc];
    const FbankOpts fo = mfcc_fbank_opts(mf_fb);
    MfccTables tab;
    mfcc_tables(mf_p, fo.n_mels, &tab);
    mf.P = mfcc_params(mf_p, fo.n_mels, tab);
    const uint32_t d = mf.P.d;
    const bool energy = fr_on && (fr_p.flags & kFrEnergy);
    mf.fbank.start(fo, fr_on ? fr_p : FrameOpts{});
    mf.utts.host.assign(U, MfccUtt{});
    mf.ntiles.assign(U, 0);
    mf.nblocks.assign(U, 0);
    mf.tiles = mf.blocks = 0;
    uint64_t frames = 0;
    int rc;
    for (size_t u = 0; u < U; u++) {
        const OutMfccUtt &pl = plan.mfcc[u];
        if ((rc = mf.fbank.add(units[u].hz, units[u].n, "jb_batch_set_mfcc", pl.T)))
            return rc;
        mf.fbank.list.host[u].x = src + units[u].off;
        mf.fbank.list.host[u].y = (uint8_t *)(logmel + pl.loff);
        MfccUtt &w = mf.utts.host[u];
        w.L = logmel + pl.loff;
        w.y = dst + pl.off;
        w.T = pl.T;
        w.g0 = mf.tiles;
        w.b0 = mf.blocks;
        w.r_T = mfcc_r(pl.T);
        mf.ntiles[u] = mfcc_tiles(pl.T);
        mf.nblocks[u] = mfcc_blocks(pl.T);
        mf.tiles += mf.ntiles[u];
        mf.blocks += mf.nblocks[u];
        frames += pl.T;
    }
    double *statics = nullptr, *bs = nullptr, *stat = nullptr, *dct = nullptr, *lift = nullptr, *en = nullptr;
    if ((energy && (rc = b.dalloc(&en, std::max<uint64_t>(frames, 1), false))) ||
        (rc = b.dalloc(&bs, mf.blocks * d, false)) ||
        (rc = b.dalloc(&stat, 2 * U * d, false)) || (rc = b.dalloc(&dct, tab.Dt.size(), false)) ||
        (rc = b.dalloc(&lift, tab.lift.size(), false)) ||
        (mf_p.n_ceps && (rc = b.dalloc(&statics, frames * d, false))))
        return rc;
    uint64_t at = 0;
    for (size_t u = 0; u < U; u++) {
        MfccUtt &w = mf.utts.host[u];
        w.c = mf_p.n_ceps ? statics + at * d : const_cast<double *>(w.L);
        w.bs = bs + w.b0 * d;
        w.stat = stat + 2 * u * d;
        // (the frames' energies of JB_FRAME_ENERGY: k_fbank writes them, k_ceps reads them, numbered as the statics)
        w.e = mf.fbank.list.host[u].e = energy ? en + at : nullptr;
        at += w.T;
    }
    if (energy && !mf.fbank.cls.geom.empty())
        mf.P.e_floor = mf.fbank.cls.geom[0].log_floor, mf.P.e_ln_floor = mf.fbank.cls.geom[0].ln_floor;
    mf.P.Dt = dct;
    mf.P.lift = lift;
    if ((rc = mf.fbank.bind(b, "mfcc filterbank")) ||
        (rc = b.dalloc(&mf.fbank.list.redo, U, false)) || (rc = upload_list(dct, tab.Dt, "mfcc DCT")) ||
        (rc = upload_list(lift, tab.lift, "mfcc lifter")) || (rc = mf.utts.alloc(b, U, U)))
        return rc;
    return mf.utts.upload("mfcc work list");
}

int OutputChain::select_mfcc(const RedoScope *scope)
{
    if (!mfcc() || !scope) {
        mf.take_blocks = mf.blocks;
        mf.fbank.list.take_all(mf.fbank.groups);
        return mf.utts.take_all(mf.tiles);
    }
    // `units`: every unit whose final PCM changed, recomputed whole -- its statistics run over all its frames; the
    // lists are renumbered, the scratch stays where the full numbering put it (the units' pointers)
    const Picked pt = pick_renumbered(scope->units, mf.ntiles), pb = pick_renumbered(scope->units, mf.nblocks);
    std::vector<MfccUtt> sub = renumbered(mf.utts.host, pt, &MfccUtt::g0);
    for (size_t i = 0; i < sub.size(); i++)
        sub[i].b0 = pb.base[i];
    mf.take_blocks = pb.total;
    const int rc = select_pass(mf.fbank, scope);
    return rc ? rc : mf.utts.upload_redo(sub, kRedoLists, pt.total);
}

int OutputChain::launch_mfcc(bool redo)
{
    if (!mfcc() || (redo && !mf.utts.n))
        return JB_OK;
    hipError_t e = mf.fbank.launch(b.stream_voc);
    if (e == hipSuccess)
        e = jb::launch_mfcc(mf.P, mf.utts.list, mf.utts.n, mf.utts.total, mf.take_blocks, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "mfcc(redo)" : "mfcc");
}

// ---- the mel spectrograms beside them, of the same final f64: k_melspec, and with a range the fold of each unit's
// maxima and the finish pass on the same stream.  The f64 values in front of the clamp lie in the MelY slab at the
// plan's places; the workgroups' maxima are numbered by the launch list, the units' by their place in it
int OutputChain::prepare_melspec()
{
    if (!melspec())
        return JB_OK;
    const std::vector<EncUnit> units = enc_units();
    const size_t U = units.size();
    const double *src = (const double *)slab[(size_t)plan.melspec_src];
    uint8_t *dst = (uint8_t *)slab[(size_t)OutSlab::Mel];
    double *vals = (double *)slab[(size_t)OutSlab::MelY];
    const bool ranged = ml_p.range > 0.0;
    ml.pass.start(ml_p);
    int rc;
    for (size_t u = 0; u < U; u++) {
        const OutMelUtt &pl = plan.melspec[u];
        if ((rc = ml.pass.add(units[u].hz, units[u].n, "jb_batch_set_melspec", pl.T)))
            return rc;
        MelUtt &w = ml.pass.list.host[u];
        w.x = src + units[u].off;
        w.y = dst + pl.off;
        w.s = ranged ? vals + pl.yoff : nullptr;
    }
    if ((ranged && ((rc = b.dalloc(&ml.gmax, ml.pass.groups, false)) || (rc = b.dalloc(&ml.umax, U, false)))) ||
        (rc = ml.pass.bind(b, "melspec")))
        return rc;
    return b.dalloc(&ml.pass.list.redo, U, false);
}

// (a redone unit's maximum runs over all its frames)
int OutputChain::select_melspec(const RedoScope *scope) { return select_pass(ml.pass, melspec() ? scope : nullptr); }

int OutputChain::launch_melspec(bool redo)
{
    if (!melspec() || (redo && !ml.pass.list.n))
        return JB_OK;
    const hipError_t e = ml.pass.launch(b.stream_voc, ml.gmax, ml.umax);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "k_melspec(redo)" : "k_melspec");
}

// ---- the pitch features beside them, of the same final f64: the decimator into the stage's f64 block, the tracker (one
// workgroup per listed unit), the post pass and the columns on the same stream.  The tracker's choices, 2 S bytes a
// frame, and the frames' lags, p and pi are blocks of the stage's own, allocated here: at the first run
int OutputChain::prepare_pitch()
{
    if (!pitch())
        return JB_OK;
    const char *who = "jb_batch_set_pitch";
    PitchGrid g;
    int rc = pitch_check_opts(&pt_p, who, &g);
    if (rc)
        return rc;
    const std::vector<EncUnit> units = enc_units();
    const size_t U = units.size();
    const double *src = (const double *)slab[(size_t)plan.pitch_src];
    if ((rc = b.dalloc(&pt.out, plan.pitch_bytes, false)) || (rc = b.dalloc(&pt.y4, plan.pitch_words, false)))
        return rc;
    uint8_t *dst = pt.out;
    double *y4 = pt.y4;
    std::vector<uint64_t> fr0(U + 1, 0), tl0(U + 1, 0);
    for (size_t u = 0; u < U; u++) {
        fr0[u + 1] = fr0[u] + plan.pitch[u].T;
        tl0[u + 1] = tl0[u] + pitch_tiles(plan.pitch[u].n4);
    }
    if (fr0[U] > kPitchMaxScratch / pitch_choice_bytes(g.S)) {
        set_error(std::string(who) + ": the tracker's choices (" + std::to_string(pitch_choice_bytes(g.S)) +
                  " bytes per frame) pass JB_PITCH_MAX_SCRATCH");
        return JB_ERR_UNSUPPORTED;
    }
    // the grid's tables in one block (G, soft, 1 / lag, ln(1 / lag)), and the distinct rates' phase tables in another
    std::vector<double> tab(g.G);
    const size_t o_soft = tab.size();
    tab.insert(tab.end(), g.soft.begin(), g.soft.end());
    const size_t o_inv = tab.size();
    tab.insert(tab.end(), g.inv_lag.begin(), g.inv_lag.end());
    const size_t o_log = tab.size();
    tab.insert(tab.end(), g.log_pitch.begin(), g.log_pitch.end());
    std::vector<double> downs;
    std::vector<uint32_t> seen;
    std::vector<size_t> first;
    std::vector<PitchDown> dn(U);
    std::vector<size_t> w_of(U);
    for (size_t u = 0; u < U; u++) {
        if ((rc = pitch_check_rate(units[u].hz, u, who, &dn[u])))
            return rc;
        size_t k = 0;
        while (k < seen.size() && seen[k] != units[u].hz)
            k++;
        if (k == seen.size()) {
            seen.push_back(units[u].hz);
            first.push_back(downs.size());
            downs.insert(downs.end(), dn[u].W.begin(), dn[u].W.end());
        }
        w_of[u] = first[k];
    }
    if ((rc = b.dalloc(&pt.tables, tab.size(), false)) || (rc = upload_list(pt.tables, tab, "pitch tables")) ||
        (rc = b.dalloc(&pt.down, downs.size(), false)) || (rc = upload_list(pt.down, downs, "pitch phase tables")) ||
        (rc = b.dalloc(&pt.tap, g.tap.size(), false)) || (rc = upload_list(pt.tap, g.tap, "pitch taps")) ||
        (rc = b.dalloc(&pt.tile, std::max<uint64_t>(2 * tl0[U], 2), false)) ||
        (rc = b.dalloc(&pt.choice, std::max<uint64_t>(fr0[U] * g.S, 1), false)) ||
        (rc = b.dalloc(&pt.idx, std::max<uint64_t>(fr0[U], 1), false)) ||
        (rc = b.dalloc(&pt.pv, std::max<uint64_t>(fr0[U], 1), false)) ||
        (rc = b.dalloc(&pt.pw, std::max<uint64_t>(fr0[U], 1), false)))
        return rc;
    PitchClass &C = pt.cls;
    C = PitchClass{};
    C.G = pt.tables;
    C.soft = pt.tables + o_soft;
    C.inv_lag = pt.tables + o_inv;
    C.log_pitch = pt.tables + o_log;
    C.tap = pt.tap;
    C.kappa = g.kappa;
    C.ballast = pt_p.nccf_ballast;
    C.pov_scale = pt_p.pov_scale;
    C.pitch_scale = pt_p.pitch_scale;
    C.delta_scale = pt_p.delta_scale;
    C.S = g.S;
    C.a = g.a;
    C.b = g.b;
    C.wl4 = g.wl4;
    C.sh4 = g.sh4;
    C.grid = pt_p.grid;
    C.flags = pt_p.flags;
    C.left = pt_p.norm_left;
    C.right = pt_p.norm_right;
    pt.utts.host.assign(U, PitchUtt{});
    for (size_t u = 0; u < U; u++) {
        const OutPitchUtt &pl = plan.pitch[u];
        PitchUtt &w = pt.utts.host[u];
        w.x = src + units[u].off;
        w.W = pt.down + w_of[u];
        w.y4 = y4 + pl.yoff;
        w.tile = pt.tile + 2 * tl0[u];
        w.choice = pt.choice + fr0[u] * g.S;
        w.idx = pt.idx + fr0[u];
        w.pv = pt.pv + fr0[u];
        w.pw = pt.pw + fr0[u];
        w.out = dst + pl.off;
        w.n = units[u].n;
        w.n4 = pl.n4;
        w.T = pl.T;
        w.hzp = dn[u].hzp;
        w.P = dn[u].P;
        w.D = dn[u].D;
    }
    pitch_number(&pt.utts.host, &pt.tiles, &pt.post, &pt.cols);
    if ((rc = pt.utts.alloc(b, U, U)))
        return rc;
    return pt.utts.upload("pitch work list");
}

// `units`: every unit whose final PCM changed, numbered among themselves
int OutputChain::select_pitch(const RedoScope *scope)
{
    if (!pitch() || !scope) {
        pitch_number(&pt.utts.host, &pt.tiles, &pt.post, &pt.cols);
        return pt.utts.take_all();
    }
    std::vector<PitchUtt> sub;
    for (size_t u = 0; u < pt.utts.host.size(); u++)
        if (scope->units[u])
            sub.push_back(pt.utts.host[u]);
    pitch_number(&sub, &pt.tiles, &pt.post, &pt.cols);
    return pt.utts.upload_redo(sub, kRedoLists);
}

int OutputChain::launch_pitch(bool redo)
{
    if (!pitch() || (redo && !pt.utts.n))
        return JB_OK;
    const hipError_t e = jb::launch_pitch(pt.utts.list, pt.utts.n, pt.tiles, pt.post, pt.cols, pt.cls, b.stream_voc);
    return e == hipSuccess ? JB_OK : hip_fail(e, redo ? "pitch(redo)" : "pitch");
}

int OutputChain::check_ready(bool requested, const char *not_run, const char *not_set) const
{
    if (requested && ready)
        return JB_OK;
    set_error(requested ? not_run : not_set);
    return JB_ERR_INVALID;
}

// The end of the last of `places` (each with a byte offset `off` and `bytes`) in their slab
template <class T> static uint64_t used_bytes(const std::vector<T> &places)
{
    uint64_t total = 0;
    for (const T &w : places)
        total = std::max<uint64_t>(total, w.off + w.bytes);
    return total;
}

// one copy of the used bytes (not zero-filled first)
int OutputChain::read_used(const void *src, uint64_t bytes, bool wait, std::unique_ptr<uint8_t[]> *host)
{
    host->reset(new (std::nothrow) uint8_t[std::max<uint64_t>(bytes, 1)]);
    if (!*host) {
        set_error("out of host memory");
        return JB_ERR_INVALID;
    }
    return bytes ? b.read(src, host->get(), (size_t)bytes, wait) : wait ? b.sync() : JB_OK;
}

int OutputChain::activity_place(size_t u, bool run, const char *who, ActLayUnit *out) const
{
    if (!act_on || !activity() || (run && !ready) || u >= plan.act.units.size()) {
        set_error(std::string(who) + (!act_on || !activity() ? ": jb_batch_set_activity was not called"
                                      : run && !ready        ? ": the batch has not run"
                                                             : ": no such unit"));
        return JB_ERR_INVALID;
    }
    *out = plan.act.units[u];
    return JB_OK;
}

int OutputChain::read_activity(size_t u, uint8_t *dst)
{
    ActLayUnit w{};
    const int rc = activity_place(u, true, "jb_batch_read_activity", &w);
    if (rc)
        return rc;
    const uint64_t bytes = w.T * w.C;
    return bytes ? b.read(act.lab + w.off, dst, (size_t)bytes) : b.sync();
}

int OutputChain::read_activity_all(std::vector<ByteSpan> *places, std::unique_ptr<uint8_t[]> *host)
{
    ActLayUnit w{};
    int rc = activity_place(0, true, "jb_batch_read_activity_all", &w);
    if (rc)
        return rc;
    places->clear();
    for (const ActLayUnit &v : plan.act.units)
        places->push_back(ByteSpan{v.off, v.T * v.C});
    return read_used(act.lab, used_bytes(*places), true, host);
}

int OutputChain::read_activity_report(size_t u, size_t col, jb_activity_report *out)
{
    ActLayUnit w{};
    const int rc = activity_place(u, true, "jb_batch_activity_report", &w);
    if (rc)
        return rc;
    if (col >= w.C) {
        set_error("jb_batch_activity_report: no such column");
        return JB_ERR_INVALID;
    }
    return b.read(act.rep + w.col0 + col, out, sizeof *out);
}

int OutputChain::read_activity_unit_report(size_t u, jb_activity_unit_report *out)
{
    ActLayUnit w{};
    const int rc = activity_place(u, true, "jb_batch_activity_unit_report", &w);
    return rc ? rc : b.read(act.urep + u, out, sizeof *out);
}

int OutputChain::read_loudness(size_t u, LoudnessResult *r)
{
    int rc = check_ready(plan.normalize(), "jb_batch_loudness: the batch has not run",
                         "jb_batch_loudness: no loudness target is set");
    return rc ? rc : b.read(ln.res + u, r, sizeof *r);
}

int OutputChain::read_noise(size_t u, jb_noise_report *out)
{
    int rc = check_ready(!noi.has.empty() || !noise_req.empty(), "jb_batch_noise_report: the batch has not run",
                         "jb_batch_noise_report: jb_batch_set_noise was not called");
    if (rc)
        return rc;
    if (u >= noise_req.size() || !noise_req[u].on) {
        set_error("jb_batch_noise_report: utterance " + std::to_string(u) + " has no noise request");
        return JB_ERR_INVALID;
    }
    NoiseRecord r{};
    if ((rc = b.read(noi.rec + u, &r, sizeof r)))
        return rc;
    *out = noise_report_of(noise_req[u], r, plan.utt[u].n);
    return JB_OK;
}

int OutputChain::read_mix(size_t p, jb_mix_report *out)
{
    int rc = check_ready(mixed(), "jb_batch_mix_report: the batch has not run",
                         "jb_batch_mix_report: jb_batch_set_mix was not called");
    if (rc)
        return rc;
    if (p >= plan.n_progs) {
        set_error("jb_batch_mix_report: no such programme");
        return JB_ERR_INVALID;
    }
    MixResult r{};
    if ((rc = b.read(pg.L.res + p, &r, sizeof r)))
        return rc;
    *out = jb_mix_report{r.peak, r.scale, plan.mix_depth[p], 0, plan.mix_overlap[p]};
    return JB_OK;
}

int OutputChain::read_stem(size_t unit, jb_stem_report *out)
{
    int rc = check_ready(mixed() && !plan.stems.empty(), "jb_batch_stem_report: the batch has not run",
                         "jb_batch_stem_report: jb_batch_set_mix_stems was not called");
    if (rc)
        return rc;
    const MixStem *st = stem(unit);
    if (!st) {
        set_error("jb_batch_stem_report: no such stem (unit " + std::to_string(unit) + ")");
        return JB_ERR_INVALID;
    }
    MixResult own{}, par{};
    MixSums so{}, sp{};
    if ((rc = b.read(pg.L.res + unit, &own, sizeof own)) || (rc = b.read(pg.L.res + st->programme, &par, sizeof par)))
        return rc;
    if (pg.sums && ((rc = b.read(pg.sums + unit, &so, sizeof so)) || (rc = b.read(pg.sums + st->programme, &sp, sizeof sp))))
        return rc;
    *out = stem_report_of(own.peak, par.scale, pg.sums != nullptr, so, sp.e);
    return JB_OK;
}

int OutputChain::read_limiter(size_t u, jb_limiter_report *out)
{
    int rc = check_ready(plan.normalize() && !lim_req.empty(), "jb_batch_limiter_report: the batch has not run",
                         "jb_batch_limiter_report: needs a loudness target and jb_batch_set_limiter");
    if (rc)
        return rc;
    if (!limited()) { // a request that limits no utterance ran the apply pass
        *out = jb_limiter_report{0.0, 0, 0, 0};
        return b.sync();
    }
    LimiterResult r{};
    if ((rc = b.read(lim.res + u, &r, sizeof r)))
        return rc;
    *out = jb_limiter_report{lim_reduction_db(r.min_a), r.count, lim.L[u], lim.H[u]};
    return JB_OK;
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

// Output u's place among `places` (each with a byte offset `off` and `bytes`); none before the request has planned it
template <class T> static ByteSpan span_of(const std::vector<T> &places, size_t u)
{
    return u < places.size() ? ByteSpan{places[u].off, places[u].bytes} : ByteSpan{};
}

OutputChain::ByteSink OutputChain::byte_sink(SynthSink sink, size_t u) const
{
    switch (sink) {
    case SynthSink::Flac:
        return {flac_on, "FLAC: the batch has not run", "FLAC: jb_batch_set_flac was not called", fl.out, false, {}};
    case SynthSink::Formatted:
        return {fmt_on, "format: the batch has not run", "format: jb_batch_set_format was not called",
                slab[(size_t)OutSlab::Fmt], true, span_of(plan.fmt, u)};
    case SynthSink::Adpcm:
        return {ad_on, "ADPCM: the batch has not run", "ADPCM: jb_batch_set_adpcm was not called",
                slab[(size_t)OutSlab::Adpcm], true, span_of(plan.adpcm, u)};
    case SynthSink::Fbank:
        return {fb_on, "fbank: the batch has not run", "fbank: jb_batch_set_fbank was not called",
                slab[(size_t)OutSlab::Feat], true, span_of(plan.fbank, u)};
    case SynthSink::Mfcc:
        return {mf_on, "mfcc: the batch has not run", "mfcc: jb_batch_set_mfcc was not called",
                slab[(size_t)OutSlab::Mfcc], true, span_of(plan.mfcc, u)};
    case SynthSink::Melspec:
        return {ml_on, "melspec: the batch has not run", "melspec: jb_batch_set_melspec was not called",
                slab[(size_t)OutSlab::Mel], true, span_of(plan.melspec, u)};
    case SynthSink::Pitch:
        return {pt_on, "pitch: the batch has not run", "pitch: jb_batch_set_pitch was not called",
                pt.out, true, span_of(plan.pitch, u)};
    case SynthSink::Pcm:
        break;
    }
    return {false, "", "PCM is no byte sink", nullptr, true, {}};
}

int OutputChain::sink_ready(SynthSink sink, bool run) const
{
    const ByteSink s = byte_sink(sink);
    if (s.on && (ready || !run))
        return JB_OK;
    set_error(s.on ? s.not_run : s.not_set);
    return JB_ERR_INVALID;
}

int OutputChain::sink_spans(SynthSink sink, size_t u0, size_t n, ByteSpan *w)
{
    const bool planned = byte_sink(sink).planned;
    int rc = sink_ready(sink, !planned);
    if (rc)
        return rc;
    if (planned) {
        for (size_t i = 0; i < n; i++)
            w[i] = byte_sink(sink, u0 + i).span;
        return JB_OK;
    }
    // the streams' sizes and places: the device's index, in one copy
    FlacOut one{};
    std::vector<FlacOut> many(n > 1 ? n : 0);
    FlacOut *res = n > 1 ? many.data() : &one;
    if ((rc = n ? b.read(fl.res + u0, res, sizeof(FlacOut) * n) : b.sync()))
        return rc;
    for (size_t i = 0; i < n; i++)
        w[i] = ByteSpan{res[i].off, res[i].bytes};
    return JB_OK;
}

// (the read of a planned sink waits for the batch, an output of no bytes too; FLAC's index read has waited already)
int OutputChain::sink_read(SynthSink sink, const ByteSpan &w, uint8_t *dst)
{
    const ByteSink s = byte_sink(sink);
    const int rc = sink_ready(sink, true);
    if (rc)
        return rc;
    if (w.bytes)
        return b.read((const uint8_t *)s.slab + w.off, dst, (size_t)w.bytes, s.planned);
    return s.planned ? b.sync() : JB_OK;
}

int OutputChain::read_bytes_all(SynthSink sink, std::vector<ByteSpan> *places, std::unique_ptr<uint8_t[]> *host)
{
    int rc = sink_ready(sink, true);
    if (rc)
        return rc;
    places->assign(num_outputs(), ByteSpan{});
    if ((rc = sink_spans(sink, 0, places->size(), places->data())))
        return rc;
    const ByteSink s = byte_sink(sink);
    return read_used(s.slab, used_bytes(*places), s.planned, host);
}

} // namespace jb

// jb_output.cpp -- plan_output: the routing table of the output stages (jb_output.h).
#include "jb_output.h"
#include "jb_adpcm.h"

#include <algorithm>
#include <numeric>

namespace jb {

void resample_ratio(uint32_t in_hz, uint32_t out_hz, uint64_t *L, uint64_t *M)
{
    const uint64_t g = std::gcd((uint64_t)in_hz, (uint64_t)out_hz);
    *L = out_hz / g;
    *M = in_hz / g;
}

uint64_t resample_out_len(uint64_t n_in, uint64_t L, uint64_t M) { return (n_in * L + M - 1) / M; }

OutPlan plan_output(const OutPlanIn &in)
{
    OutPlan p;
    p.utt.resize(in.B);
    for (size_t u = 0; u < in.B; u++) {
        OutUtt &w = p.utt[u];
        w.hz = (in.want_hz && in.want_hz[u]) ? in.want_hz[u] : in.voice_hz;
        uint64_t L = 1, M = 1;
        if (w.hz != in.voice_hz) {
            resample_ratio(in.voice_hz, w.hz, &L, &M);
            p.convert = true;
        }
        w.L = (uint32_t)L;
        w.M = (uint32_t)M;
        p.native_total += in.n_native[u];
    }
    // a converting batch packs its output utterance after utterance; without conversion the native slab is the output
    for (size_t u = 0; u < in.B; u++) {
        OutUtt &w = p.utt[u];
        w.n = p.convert ? resample_out_len(in.n_native[u], w.L, w.M) : in.n_native[u];
        w.off = p.convert ? p.total : in.off_native[u];
        p.total += w.n;
    }
    // Every stage but the last writes f64 (the converter and the measurement read f64); the last one writes what the
    // flags asked for.  A 16-bit output goes to the slab the batch was created with where it fits
    const OutSlab out16 = p.total <= p.native_total ? OutSlab::S16 : OutSlab::New16;
    // (a request whose utterances all have no section is no request: every field as without one)
    bool filt = false;
    for (size_t u = 0; in.filter && u < in.B; u++)
        filt = filt || in.filter[u];
    if (in.i16 && !p.convert && !in.loudness && !filt)
        p.vocoder = {OutSlab::S16, true};
    else
        p.vocoder = {in.i16 ? OutSlab::Voc64 : OutSlab::V64, false};
    p.final = p.vocoder;
    if (p.convert) {
        p.converter = (in.i16 && !in.loudness && !filt) ? OutWrite{out16, true} : OutWrite{OutSlab::Conv64, false};
        p.final = p.converter;
    }
    // the filter behind the converter and in front of the measurement: f64 in; the last stage's rule out
    if (filt) {
        p.filter_src = p.final.slab;
        p.filter = (in.i16 && !in.loudness) ? OutWrite{out16, true} : OutWrite{OutSlab::Filt64, false};
        p.final = p.filter;
    }
    if (in.loudness) {
        p.measure = p.final.slab;
        p.apply = in.i16 ? OutWrite{out16, true} : OutWrite{OutSlab::Apply64, false};
        p.final = p.apply;
    }
    p.native64 = p.vocoder.i16 ? OutSlab::None : p.vocoder.slab;
    p.flac = (in.flac && p.final.i16) ? p.final.slab : OutSlab::None;
    for (const OutWrite &w : {p.vocoder, p.converter, p.filter, p.apply})
        if (w.slab != OutSlab::None && w.slab != OutSlab::V64 && w.slab != OutSlab::S16)
            p.alloc[(size_t)w.slab] = std::max<uint64_t>(w.slab == OutSlab::Voc64 ? p.native_total : p.total, 1);
    // the join behind all of them: the final PCM gathered into programmes in a slab of its own, which the encoders
    // then read; their units are the programmes (a request the chain has checked; one that does not lay out: no join)
    std::vector<OutUnit> units;
    OutWrite enc = p.final; // what the encoders read
    // (a join's request and a mix's go the same way: the same slab, the same fields; only what the report and the redo
    // rule read tells them apart; a join given in its own words is worded as the mix it means first, in front of `mix`)
    std::vector<MixUtt> worded;
    if (in.join)
        worded = join_as_mix(in.join, in.B);
    const MixUtt *request = in.join ? worded.data() : in.mix;
    const bool chained = in.join || in.chained;
    if (request) {
        std::vector<uint64_t> n(in.B);
        for (size_t u = 0; u < in.B; u++)
            n[u] = p.utt[u].n;
        MixLayout lay;
        if (mix_layout(request, n.data(), nullptr, in.B, p.final.i16 ? 2 : 8, &lay, nullptr, nullptr, chained,
                       chained ? nullptr : in.stem_of)) {
            p.join_src = p.final;
            p.join = {p.final.i16 ? OutSlab::Join16 : OutSlab::Join64, p.final.i16};
            p.mixed = !chained;
            p.n_progs = lay.programmes();
            for (size_t g = 0; g < p.n_progs; g++)
                lay.units[g].hz = p.utt[lay.progs.members[lay.progs.first[g]]].hz;
            for (size_t s = 0; s < lay.stems.size(); s++) { // a stem has its programme's rate
                lay.units[p.n_progs + s].hz = lay.units[lay.stems[s].programme].hz;
                p.unit_parent.push_back(lay.stems[s].programme);
            }
            p.stems = std::move(lay.stems);
            p.stem_unit = std::move(lay.stem_unit);
            p.units = lay.units;
            p.prog_of = std::move(lay.progs.group_of);
            p.prog_first = std::move(lay.progs.first);
            p.prog_members = std::move(lay.progs.members);
            p.prog_start = std::move(lay.start);
            if (p.mixed) {
                p.prog_gain = std::move(lay.gain);
                p.mix_depth = std::move(lay.depth);
                p.mix_overlap = std::move(lay.overlap);
            }
            p.alloc[(size_t)p.join.slab] = std::max<uint64_t>(lay.total, 1);
            enc = p.join;
            if (p.flac != OutSlab::None)
                p.flac = p.join.slab;
        }
    }
    const bool joined = p.join.slab != OutSlab::None;
    if (joined)
        units = p.units;
    else
        for (size_t u = 0; u < in.B; u++)
            units.push_back({p.utt[u].hz, p.utt[u].n, p.utt[u].off});
    // the format stage behind all of them: the final f64 to bytes, unit after unit (an utterance; with a join a
    // programme) on 16-byte boundaries
    if (in.fmt_bytes && !p.final.i16) {
        p.fmt_src = enc.slab;
        p.fmt.resize(units.size());
        uint64_t bytes = 0;
        for (size_t u = 0; u < units.size(); u++) {
            p.fmt[u] = {bytes, units[u].n * in.fmt_bytes};
            bytes += (p.fmt[u].bytes + 15) & ~(uint64_t)15;
        }
        p.alloc[(size_t)OutSlab::Fmt] = std::max<uint64_t>(bytes, 16);
    }
    // IMA ADPCM beside it: the final PCM, f64 or 16-bit, to blocks of each unit's own size
    if (in.adpcm) {
        p.adpcm_src = enc;
        p.adpcm.resize(units.size());
        uint64_t bytes = 0;
        for (size_t u = 0; u < units.size(); u++) {
            const uint32_t A = adpcm_block_align(units[u].hz, in.adpcm_align);
            p.adpcm[u] = {bytes, adpcm_bytes(units[u].n, A), A};
            bytes += (p.adpcm[u].bytes + 15) & ~(uint64_t)15;
        }
        p.alloc[(size_t)OutSlab::Adpcm] = std::max<uint64_t>(bytes, 16);
    }
    // the filterbank features beside them: the final f64 to frames of each unit's own geometry (a request that some
    // rate refuses is no request: the chain has checked it)
    const bool reflect = in.frame && (in.frame->flags & kFrReflect); // (the frame request: T of both feature stages)
    if (in.fbank && !p.final.i16) {
        std::vector<OutFbankUtt> f(units.size());
        uint64_t bytes = 0;
        bool ok = true;
        for (size_t u = 0; u < units.size() && ok; u++) {
            FbankGeom g{};
            if (!(ok = fbank_geometry_quiet(*in.fbank, units[u].hz, &g)))
                break;
            const uint64_t T = frame_count(units[u].n, g.wl, g.hop, (in.fbank->flags & kFbCenter) != 0, reflect);
            f[u] = {bytes, T * g.n_mels * fbank_elem(in.fbank->flags), T, g.wl, g.hop, g.n_fft};
            bytes += (f[u].bytes + 15) & ~(uint64_t)15;
        }
        if (ok) {
            p.fbank_src = enc.slab;
            p.fbank = std::move(f);
            p.alloc[(size_t)OutSlab::Feat] = std::max<uint64_t>(bytes, 16);
        }
    }
    // the cepstral features beside them, independent of a plain fbank request: the same final f64 through a filterbank
    // pass of the stage's own into the f64 log-mel scratch, then rows of each unit's own length
    if (in.mfcc && in.mfcc_fbank && !p.final.i16 && !mfcc_fbank_fault(*in.mfcc_fbank) &&
        !mfcc_opts_fault(*in.mfcc, in.mfcc_fbank->n_mels)) {
        const FbankOpts fo = mfcc_fbank_opts(*in.mfcc_fbank);
        std::vector<OutMfccUtt> f(units.size());
        uint64_t bytes = 0, words = 0;
        bool ok = true;
        for (size_t u = 0; u < units.size() && ok; u++) {
            FbankGeom g{};
            if (!(ok = fbank_geometry_quiet(fo, units[u].hz, &g)))
                break;
            const uint64_t T = frame_count(units[u].n, g.wl, g.hop, (fo.flags & kFbCenter) != 0, reflect);
            const uint32_t width = mfcc_width(*in.mfcc, g.n_mels);
            f[u] = {bytes, T * width * mfcc_elem(in.mfcc->flags), T, width, g.n_fft, words};
            bytes += (f[u].bytes + 15) & ~(uint64_t)15;
            words += (T * g.n_mels + 1) & ~(uint64_t)1;
        }
        if (ok) {
            p.mfcc_src = enc.slab;
            p.mfcc = std::move(f);
            p.alloc[(size_t)OutSlab::MfccL] = std::max<uint64_t>(words, 2);
            p.alloc[(size_t)OutSlab::Mfcc] = std::max<uint64_t>(bytes, 16);
        }
    }
    // the mel spectrograms beside them, independent of both: the same final f64 to frames of each unit's own length;
    // with a range the f64 values in front of the clamp in a scratch of the stage
    if (in.melspec && !p.final.i16) {
        const MelOpts &mo = *in.melspec;
        std::vector<OutMelUtt> f(units.size());
        uint64_t bytes = 0, words = 0;
        bool ok = true;
        for (size_t u = 0; u < units.size() && ok; u++) {
            MelGeom g{};
            if (!(ok = mel_geometry_quiet(mo, units[u].hz, &g)))
                break;
            const uint64_t T = mel_frames(units[u].n, g.n_fft, g.hop, mo.pad, mo.flags);
            f[u] = {bytes, T * g.n_mels * mel_elem(mo.flags), T, g.n_fft, g.hop, mo.range > 0.0 ? words : 0};
            bytes += (f[u].bytes + 15) & ~(uint64_t)15;
            words += (T * g.n_mels + 1) & ~(uint64_t)1;
        }
        if (ok) {
            p.melspec_src = enc.slab;
            p.melspec = std::move(f);
            p.alloc[(size_t)OutSlab::Mel] = std::max<uint64_t>(bytes, 16);
            if (mo.range > 0.0)
                p.alloc[(size_t)OutSlab::MelY] = std::max<uint64_t>(words, 2);
        }
    }
    // the pitch features beside them, independent of the three: the same final f64 to a 4 kHz signal of the stage's
    // own, then rows of each unit's own length (a request that some rate refuses is no request: the chain has checked it)
    if (in.pitch && !p.final.i16 && !pitch_opts_fault(*in.pitch)) {
        const PitchOpts &po = *in.pitch;
        std::vector<OutPitchUtt> f(units.size());
        uint64_t bytes = 0, words = 0;
        bool ok = true;
        for (size_t u = 0; u < units.size() && ok; u++) {
            const uint32_t hz = units[u].hz;
            PitchDown down;
            bool cap = false;
            if (!(ok = !pitch_down_fault(hz, &down, &cap)))
                break;
            const uint64_t T = pitch_frames(po.grid, units[u].n, (uint32_t)fbank_round_us(hz, po.win_us),
                                            (uint32_t)fbank_round_us(hz, po.hop_us));
            const uint32_t width = pitch_width(po.flags), elem = (uint32_t)pitch_elem(po.flags);
            f[u] = {bytes, T * width * elem, T, width, elem, pitch_n4(units[u].n, hz), words};
            bytes += (f[u].bytes + 15) & ~(uint64_t)15;
            words += (f[u].n4 + 1) & ~(uint64_t)1;
        }
        if (ok) {
            p.pitch_src = enc.slab;
            p.pitch = std::move(f);
            p.pitch_bytes = std::max<uint64_t>(bytes, 16);
            p.pitch_words = std::max<uint64_t>(words, 2);
        }
    }
    // the speech-activity labels, a side output beside all of them: a column per member of each unit measured on the
    // member's own final PCM at its start, or one column on the unit's PCM (a request that some unit refuses is no
    // request: the chain has checked it)
    if (in.activity) {
        const size_t U = joined ? p.n_progs : units.size(); // (a mix's stems are no units of this stage: it reads members)
        std::vector<uint64_t> unit_n(U), n(in.B), start(in.B, 0);
        std::vector<uint32_t> unit_hz(U), first(U + 1), members(in.B);
        std::vector<double> gain(in.B, 1.0);
        for (size_t u = 0; u < U; u++) {
            unit_n[u] = units[u].n;
            unit_hz[u] = units[u].hz;
        }
        for (size_t u = 0; u < in.B; u++) {
            n[u] = p.utt[u].n;
            members[u] = (uint32_t)u;
        }
        for (size_t u = 0; u <= U; u++)
            first[u] = (uint32_t)u;
        if (joined) {
            first = p.prog_first;
            members = p.prog_members;
            start = p.prog_start;
            if (p.mixed)
                gain = p.prog_gain;
        }
        ActLayout lay;
        p.act_fault = act_layout(*in.activity, U, unit_n.data(), unit_hz.data(), first.data(), members.data(),
                                 start.data(), n.data(), gain.data(), &lay, &p.act_fault_unit, &p.act_unsupported);
        if (!p.act_fault) {
            p.act_src = in.activity->columns == kActUnit ? enc : p.final;
            p.act = std::move(lay);
        }
    }
    return p;
}

std::vector<MixUtt> join_as_mix(const JoinUtt *req, size_t B)
{
    std::vector<MixUtt> m(B, MixUtt{});
    for (size_t u = 0; u < B; u++) {
        m[u].programme = req[u].programme;
        m[u].fade_in = req[u].fade_in;
        m[u].fade_out = req[u].fade_out;
        m[u].reserved = req[u].reserved;
        m[u].start = req[u].pad_before;
        m[u].pad_after = req[u].pad_after;
    }
    return m;
}

bool join_layout(const JoinUtt *req, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem, JoinLayout *out,
                 uint32_t *bad, const char **field)
{
    return mix_layout(join_as_mix(req, B).data(), n, hz, B, elem, out, bad, field, true);
}

bool mix_layout(const MixUtt *req, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem, MixLayout *out,
                uint32_t *bad, const char **field, bool chained, const uint32_t *stem_of)
{
    // the numbering and the agreement on the rate are the loudness groups'
    static_assert(kMixNone == kLnNoGroup && kJoinNone == kLnNoGroup, "one numbering for groups and programmes");
    auto refuse = [&](uint32_t id, const char *f) {
        if (bad)
            *bad = id;
        if (field)
            *field = f;
        return false;
    };
    std::vector<uint32_t> ids(B);
    for (size_t u = 0; u < B; u++)
        ids[u] = req[u].programme;
    LnGroupsIn gi;
    gi.B = B;
    gi.group = ids.data();
    gi.hz = hz;
    MixLayout lay;
    uint32_t id = 0;
    const char *f = "";
    if (!plan_loudness_groups(gi, &lay.progs, &id, &f))
        return refuse(id, f[0] == 'g' ? "programme id" : f); // ("group id")
    const size_t P = lay.progs.size();
    const uint64_t align = kProgGroupBytes / elem;
    constexpr uint64_t kMaxLen = 1ull << 63;
    lay.units.assign(P, OutUnit{});
    lay.start.assign(B, 0);
    lay.gain.assign(B, 0.0);
    lay.seg_first.assign(P + 1, 0);
    lay.depth.assign(P, 0);
    lay.overlap.assign(P, 0);
    struct Event {
        uint64_t k;
        uint32_t at; // the member's place in progs.members
        bool add;
    };
    std::vector<Event> ev;
    std::vector<uint32_t> cover; // ascending places: ascending utterance indices
    // the sweep over the events of unit g of `len` samples: a segment ends at every event; between two the cover stands
    auto sweep = [&](size_t g, uint64_t len) {
        std::stable_sort(ev.begin(), ev.end(), [](const Event &a, const Event &b) { return a.k < b.k; });
        cover.clear();
        uint64_t k = 0;
        auto emit = [&](uint64_t to) {
            if (to <= k)
                return true;
            if (lay.lists.size() + cover.size() > kMixMaxList)
                return false;
            lay.segs.push_back({k, to, (uint32_t)lay.lists.size(), (uint32_t)cover.size()});
            lay.lists.insert(lay.lists.end(), cover.begin(), cover.end());
            lay.depth[g] = std::max<uint32_t>(lay.depth[g], (uint32_t)cover.size());
            if (cover.size() >= 2)
                lay.overlap[g] += to - k;
            k = to;
            return true;
        };
        for (const Event &e : ev) {
            if (!emit(e.k))
                return false;
            const auto it = std::lower_bound(cover.begin(), cover.end(), e.at);
            if (e.add)
                cover.insert(it, e.at);
            else
                cover.erase(it);
        }
        if (!emit(len)) // (the pads behind the last member's end: silence)
            return false;
        lay.seg_first[g + 1] = (uint32_t)lay.segs.size();
        return true;
    };
    for (size_t g = 0; g < P; g++) {
        OutUnit &w = lay.units[g];
        w.off = lay.total;
        ev.clear();
        for (uint32_t i = lay.progs.first[g]; i < lay.progs.first[g + 1]; i++) {
            const uint32_t u = lay.progs.members[i];
            // (each term below 2^63 and each partial sum checked: no sum wraps)
            if (req[u].start >= kMaxLen || n[u] >= kMaxLen || req[u].pad_after >= kMaxLen)
                return refuse(u, "length");
            const uint64_t start = chained ? w.n + req[u].start : req[u].start; // (w.n: where the member in front ends)
            if (start >= kMaxLen || start + n[u] >= kMaxLen || start + n[u] + req[u].pad_after >= kMaxLen)
                return refuse(u, "length");
            lay.start[u] = start;
            lay.gain[u] = mix_gain(req[u].gain_db);
            w.n = std::max(w.n, start + n[u] + req[u].pad_after);
            if (lay.gain[u] != 0.0 && n[u]) {
                ev.push_back({start, i, true});
                ev.push_back({start + n[u], i, false});
            }
        }
        w.hz = hz ? hz[lay.progs.members[lay.progs.first[g]]] : 0;
        if (lay.total >= kMaxLen || w.n + align >= kMaxLen - lay.total)
            return refuse((uint32_t)g, "slab length");
        lay.total = (w.off + w.n + align - 1) / align * align;
        if (!sweep(g, w.n))
            return refuse((uint32_t)g, "work lists");
    }
    // the stems behind the programmes: by programme, within one by each stem's first member
    if (stem_of) {
        for (size_t u = 0; u < B; u++)
            if (stem_of[u] != kMixNoStem && stem_of[u] >= B)
                return refuse((uint32_t)u, "stem id");
        lay.stem_unit.assign(B, -1);
        std::vector<uint32_t> stem_at(B, kMixNoStem); // caller's id -> the stem, within the programme at hand
        for (size_t g = 0; g < P; g++) {
            const size_t s0 = lay.stems.size();
            for (uint32_t i = lay.progs.first[g]; i < lay.progs.first[g + 1]; i++) {
                const uint32_t u = lay.progs.members[i], id = stem_of[u];
                if (id == kMixNoStem)
                    continue;
                if (stem_at[id] == kMixNoStem) {
                    stem_at[id] = (uint32_t)lay.stems.size();
                    lay.stems.push_back(MixStem{(uint32_t)g, id, 0, 0, 0, 0});
                }
                const size_t s = stem_at[id];
                lay.stems[s].n_members++;
                lay.stem_unit[u] = (int32_t)(P + s);
            }
            for (size_t s = s0; s < lay.stems.size(); s++) {
                const size_t unit = P + s;
                stem_at[lay.stems[s].id] = kMixNoStem; // (the next programme counts its ids anew)
                lay.units.push_back(OutUnit{lay.units[g].hz, lay.units[g].n, lay.total});
                lay.seg_first.push_back(lay.seg_first.back());
                lay.depth.push_back(0);
                lay.overlap.push_back(0);
                const OutUnit &w = lay.units[unit];
                if (lay.total >= kMaxLen || w.n + align >= kMaxLen - lay.total)
                    return refuse((uint32_t)unit, "slab length");
                lay.total = (w.off + w.n + align - 1) / align * align;
                ev.clear();
                MixStem &st = lay.stems[s];
                bool any = false;
                for (uint32_t i = lay.progs.first[g]; i < lay.progs.first[g + 1]; i++) {
                    const uint32_t u = lay.progs.members[i];
                    if (stem_of[u] != st.id || lay.gain[u] == 0.0 || !n[u])
                        continue;
                    ev.push_back({lay.start[u], i, true});
                    ev.push_back({lay.start[u] + n[u], i, false});
                    st.first = any ? std::min(st.first, lay.start[u]) : lay.start[u];
                    st.end = any ? std::max(st.end, lay.start[u] + n[u]) : lay.start[u] + n[u];
                    any = true;
                }
                if (!sweep(unit, w.n))
                    return refuse((uint32_t)unit, "work lists");
            }
        }
    }
    *out = std::move(lay);
    return true;
}

void join_closure(const std::vector<uint32_t> &prog_of, size_t P, const std::vector<uint8_t> &post,
                  std::vector<uint8_t> *programmes, const std::vector<uint32_t> &unit_parent)
{
    programmes->assign(P + unit_parent.size(), 0);
    for (size_t u = 0; u < prog_of.size(); u++)
        if (post[u])
            (*programmes)[prog_of[u]] = 1;
    for (size_t s = 0; s < unit_parent.size(); s++)
        (*programmes)[P + s] = (*programmes)[unit_parent[s]];
}

bool plan_loudness_groups(const LnGroupsIn &in, LnGroups *out, uint32_t *bad_group, const char **bad_field)
{
    const size_t B = in.B;
    auto refuse = [&](uint32_t id, const char *field) {
        if (bad_group)
            *bad_group = id;
        if (bad_field)
            *bad_field = field;
        return false;
    };
    LnGroups g;
    g.group_of.assign(B, 0);
    std::vector<uint32_t> dense_of(B, kLnNoGroup); // caller's id -> dense id
    std::vector<uint32_t> first_member;            // dense id -> its first member
    for (size_t u = 0; u < B; u++) {
        const uint32_t id = in.group[u];
        if (id != kLnNoGroup && id >= B)
            return refuse(id, "group id");
        uint32_t d = id == kLnNoGroup ? kLnNoGroup : dense_of[id];
        if (d == kLnNoGroup) {
            d = (uint32_t)first_member.size();
            first_member.push_back((uint32_t)u);
            if (id != kLnNoGroup)
                dense_of[id] = d;
        }
        g.group_of[u] = d;
        // a member agrees with its group's first member
        const size_t f = first_member[d];
        if (f == u)
            continue;
        if (in.target) {
            const double a = in.target[f], b = in.target[u];
            if (!(a == b || (a != a && b != b)))
                return refuse(id, "target");
            if (in.ceiling && in.ceiling[f] != in.ceiling[u])
                return refuse(id, "ceiling");
        }
        if (in.mode && in.mode[f] != in.mode[u])
            return refuse(id, "peak mode");
        if (in.hz && in.hz[f] != in.hz[u])
            return refuse(id, "output rate");
    }
    const size_t G = first_member.size();
    g.first.assign(G + 1, 0);
    for (size_t u = 0; u < B; u++)
        g.first[g.group_of[u] + 1]++;
    for (size_t d = 0; d < G; d++)
        g.first[d + 1] += g.first[d];
    g.members.assign(B, 0);
    std::vector<uint32_t> fill(g.first.begin(), g.first.end() - 1);
    for (size_t u = 0; u < B; u++)
        g.members[fill[g.group_of[u]]++] = (uint32_t)u;
    *out = std::move(g);
    return true;
}

void loudness_groups_closure(const LnGroups &g, const std::vector<uint8_t> &touched, std::vector<uint8_t> *groups,
                             std::vector<uint8_t> *members)
{
    const size_t B = g.group_of.size();
    groups->assign(g.size(), 0);
    members->assign(B, 0);
    for (size_t u = 0; u < B; u++)
        if (touched[u])
            (*groups)[g.group_of[u]] = 1;
    for (size_t u = 0; u < B; u++)
        (*members)[u] = (*groups)[g.group_of[u]];
}

RedoScope redo_scope(const std::vector<uint32_t> &prog_of, size_t P, const LnGroups &groups,
                     const std::vector<uint8_t> &only, const std::vector<uint32_t> &unit_parent)
{
    RedoScope s;
    s.measured = s.post = only;
    if (groups.size())
        loudness_groups_closure(groups, only, &s.touched_groups, &s.post);
    s.units = s.post;
    if (!prog_of.empty())
        join_closure(prog_of, P, s.post, &s.units, unit_parent);
    return s;
}

Picked pick_renumbered(const std::vector<uint8_t> &mask, const std::vector<uint64_t> &count)
{
    Picked p;
    for (size_t i = 0; i < count.size(); i++)
        if (mask[i]) {
            p.index.push_back((uint32_t)i);
            p.base.push_back(p.total);
            p.total += count[i];
        }
    return p;
}

} // namespace jb

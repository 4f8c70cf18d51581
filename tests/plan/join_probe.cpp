// Prints what the output plan (jbonsai_amd/csrc/jb_output.h) makes of a join request as JSON; host-only.
// stdin, whitespace-separated, the first word the mode:
//   plan     voice_hz i16 loudness flac fmt_bytes adpcm adpcm_align  B n_native[0..B) off_native[0..B)
//            nw want_hz[0..nw)  nj request[0..nj)          (nw, nj: 0 = not requested, or B)
//            the fields of tests/plan/adpcm_probe.cpp under the same names, then join_src, join, units (hz, n, off),
//            prog_of, prog_start, prog_first, prog_members
//   layout   elem B request[0..B) n[0..B) nh hz[0..nh)        (nh: 0 = rates not compared, or B)
//            ok, bad, field, prog_of, start, units, total of the one layout (mix_layout over join_as_mix), the mix
//            request the join means as `converted` (programme, start, gain_db, pad_after, fade_in, fade_out), and the
//            work lists: seg_first, segs (k0, k1, l0, nl), lists (as utterance indices), depth, overlap
//   closure  B request[0..B) ng group[0..ng) touched[0..B)   (ng: 0 = no loudness groups, or B; -1 = no group)
//            post (the touched set behind loudness_groups_closure) and programmes (join_closure of it)
// A request entry is: programme (-1 = none) pad_before pad_after fade_in fade_out.
#include "jb_output.h"

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

static const char *name(jb::OutSlab s)
{
    static const char *const names[] = {"none",    "V64",   "S16", "Voc64", "Conv64",
                                        "Apply64", "New16", "Fmt", "Adpcm", "Join64", "Join16"};
    return names[(size_t)s];
}

static void write_of(const char *key, const jb::OutWrite &w)
{
    printf(" \"%s\": [\"%s\", \"%s\"],", key, name(w.slab), w.slab == jb::OutSlab::None ? "-" : w.i16 ? "i16" : "f64");
}

template <class T> static void list_of(const char *key, const std::vector<T> &v, const char *end)
{
    printf(" \"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++)
        printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    printf("]%s", end);
}

static void units_of(const std::vector<jb::OutUnit> &units, const char *end)
{
    printf(" \"units\": [");
    for (size_t g = 0; g < units.size(); g++)
        printf("%s[%u, %llu, %llu]", g ? ", " : "", units[g].hz, (unsigned long long)units[g].n,
               (unsigned long long)units[g].off);
    printf("]%s", end);
}

static std::vector<jb::JoinUtt> read_request(size_t n)
{
    std::vector<jb::JoinUtt> req(n, jb::JoinUtt{});
    for (auto &r : req) {
        long long id = 0;
        std::cin >> id >> r.pad_before >> r.pad_after >> r.fade_in >> r.fade_out;
        r.programme = id < 0 ? jb::kJoinNone : (uint32_t)id;
    }
    return req;
}

static int plan()
{
    jb::OutPlanIn in;
    int i16 = 0, loudness = 0, flac = 0, adpcm = 0;
    size_t nw = 0, nj = 0;
    std::cin >> in.voice_hz >> i16 >> loudness >> flac >> in.fmt_bytes >> adpcm >> in.adpcm_align >> in.B;
    std::vector<uint64_t> n(in.B), off(in.B);
    for (auto &x : n)
        std::cin >> x;
    for (auto &x : off)
        std::cin >> x;
    std::cin >> nw;
    std::vector<uint32_t> want(nw);
    for (auto &x : want)
        std::cin >> x;
    std::cin >> nj;
    const std::vector<jb::JoinUtt> req = read_request(nj);
    if (!std::cin || (nw && nw != in.B) || (nj && nj != in.B)) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    in.n_native = n.data();
    in.off_native = off.data();
    in.i16 = i16 != 0;
    in.loudness = loudness != 0;
    in.flac = flac != 0;
    in.adpcm = adpcm != 0;
    in.want_hz = nw ? want.data() : nullptr;
    in.join = nj ? req.data() : nullptr;
    const jb::OutPlan p = jb::plan_output(in);
    printf("{\"convert\": %s, \"active\": %s, \"total\": %llu, \"native_total\": %llu,", p.convert ? "true" : "false",
           p.active() ? "true" : "false", (unsigned long long)p.total, (unsigned long long)p.native_total);
    write_of("vocoder", p.vocoder);
    write_of("converter", p.converter);
    write_of("apply", p.apply);
    write_of("final", p.final);
    printf(" \"measure\": \"%s\", \"flac\": \"%s\", \"native64\": \"%s\",\n \"alloc\": {", name(p.measure), name(p.flac),
           name(p.native64));
    bool first = true;
    for (size_t s = 0; s < (size_t)jb::OutSlab::Count; s++)
        if (p.alloc[s]) {
            printf("%s\"%s\": [%llu, %zu]", first ? "" : ", ", name((jb::OutSlab)s), (unsigned long long)p.alloc[s],
                   jb::out_slab_elem((jb::OutSlab)s));
            first = false;
        }
    printf("},\n \"utt\": [");
    for (size_t u = 0; u < p.utt.size(); u++) {
        const jb::OutUtt &w = p.utt[u];
        printf("%s[%u, %u, %u, %llu, %llu]", u ? ", " : "", w.hz, w.L, w.M, (unsigned long long)w.n,
               (unsigned long long)w.off);
    }
    printf("],\n \"fmt_src\": \"%s\", \"fmt\": [", name(p.fmt_src));
    for (size_t u = 0; u < p.fmt.size(); u++)
        printf("%s[%llu, %llu]", u ? ", " : "", (unsigned long long)p.fmt[u].off, (unsigned long long)p.fmt[u].bytes);
    printf("],\n");
    write_of("adpcm_src", p.adpcm_src);
    printf(" \"adpcm\": [");
    for (size_t u = 0; u < p.adpcm.size(); u++)
        printf("%s[%llu, %llu, %u]", u ? ", " : "", (unsigned long long)p.adpcm[u].off,
               (unsigned long long)p.adpcm[u].bytes, p.adpcm[u].A);
    printf("],\n");
    write_of("join_src", p.join_src);
    write_of("join", p.join);
    units_of(p.units, ",");
    list_of("prog_of", p.prog_of, ",");
    list_of("prog_start", p.prog_start, ",");
    list_of("prog_first", p.prog_first, ",");
    list_of("prog_members", p.prog_members, "}\n");
    return 0;
}

static int layout()
{
    size_t elem = 0, B = 0, nh = 0;
    std::cin >> elem >> B;
    const std::vector<jb::JoinUtt> req = read_request(B);
    std::vector<uint64_t> n(B);
    for (auto &x : n)
        std::cin >> x;
    std::cin >> nh;
    std::vector<uint32_t> hz(nh);
    for (auto &x : hz)
        std::cin >> x;
    if (!std::cin || (elem != 2 && elem != 8) || (nh && nh != B)) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    // the join in the mix's words, through the one layout; `converted` is the mix request it means: the layout's starts
    // in the place of the pads in front
    std::vector<jb::MixUtt> mix = jb::join_as_mix(req.data(), B);
    jb::MixLayout lay;
    uint32_t bad = 0;
    const char *field = "";
    const bool ok = jb::mix_layout(mix.data(), n.data(), nh ? hz.data() : nullptr, B, elem, &lay, &bad, &field, true);
    printf("{\"ok\": %s, \"bad\": %lld, \"field\": \"%s\",", ok ? "true" : "false",
           bad == jb::kJoinNone ? -1ll : (long long)bad, field);
    list_of("prog_of", lay.progs.group_of, ",");
    list_of("start", lay.start, ",");
    units_of(lay.units, ",");
    printf(" \"converted\": [");
    for (size_t u = 0; ok && u < B; u++)
        printf("%s[%lld, %llu, %.17g, %llu, %u, %u]", u ? ", " : "",
               mix[u].programme == jb::kMixNone ? -1ll : (long long)mix[u].programme, (unsigned long long)lay.start[u],
               mix[u].gain_db, (unsigned long long)mix[u].pad_after, mix[u].fade_in, mix[u].fade_out);
    printf("],");
    list_of("seg_first", lay.seg_first, ",");
    printf(" \"segs\": [");
    for (size_t i = 0; i < lay.segs.size(); i++)
        printf("%s[%llu, %llu, %u, %u]", i ? ", " : "", (unsigned long long)lay.segs[i].k0,
               (unsigned long long)lay.segs[i].k1, lay.segs[i].l0, lay.segs[i].nl);
    printf("],");
    std::vector<uint32_t> who;
    for (uint32_t at : lay.lists)
        who.push_back(lay.progs.members[at]);
    list_of("lists", who, ",");
    list_of("depth", lay.depth, ",");
    list_of("overlap", lay.overlap, ",");
    printf(" \"total\": %llu}\n", (unsigned long long)lay.total);
    return 0;
}

static int closure()
{
    size_t B = 0, ng = 0;
    std::cin >> B;
    const std::vector<jb::JoinUtt> req = read_request(B);
    std::cin >> ng;
    std::vector<uint32_t> group(ng);
    for (auto &g : group) {
        long long id = 0;
        std::cin >> id;
        g = id < 0 ? jb::kLnNoGroup : (uint32_t)id;
    }
    std::vector<uint8_t> touched(B);
    for (auto &t : touched) {
        int v = 0;
        std::cin >> v;
        t = v != 0;
    }
    if (!std::cin || (ng && ng != B)) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    std::vector<uint8_t> post = touched, groups, programmes;
    if (ng) {
        jb::LnGroupsIn gi;
        gi.B = B;
        gi.group = group.data();
        jb::LnGroups g;
        if (!jb::plan_loudness_groups(gi, &g, nullptr, nullptr)) {
            fprintf(stderr, "bad groups\n");
            return 2;
        }
        jb::loudness_groups_closure(g, touched, &groups, &post);
    }
    std::vector<uint64_t> n(B, 1);
    jb::JoinLayout lay;
    if (!jb::join_layout(req.data(), n.data(), nullptr, B, 8, &lay, nullptr, nullptr)) {
        fprintf(stderr, "bad request\n");
        return 2;
    }
    jb::join_closure(lay.progs.group_of, lay.units.size(), post, &programmes);
    printf("{");
    list_of("post", post, ",");
    list_of("programmes", programmes, "}\n");
    return 0;
}

int main()
{
    std::string mode;
    std::cin >> mode;
    if (mode == "plan")
        return plan();
    if (mode == "layout")
        return layout();
    if (mode == "closure")
        return closure();
    fprintf(stderr, "bad mode\n");
    return 2;
}

// Prints what the output plan (jbonsai_amd/csrc/jb_output.h) makes of a mix request as JSON; host-only.
// stdin, whitespace-separated, the first word the mode:
//   layout   elem B request[0..B) n[0..B) nh hz[0..nh)        (nh: 0 = rates not compared, or B)
//            ok, bad, field, prog_of, start, units (hz, n, off), total, gain, seg_first, segs (k0, k1, l0, nl), lists
//            (as utterance indices), depth, overlap
//   plan     kind voice_hz i16 loudness flac fmt_bytes adpcm  B n_native[0..B) off_native[0..B) nw want_hz[0..nw)
//            request[0..B)                                    (kind: "mix", "join" or "both"; nw: 0 or B)
//            final, join_src, join, mixed, flac, fmt_src, adpcm_src, the join slab's elements, units, prog_of,
//            prog_start, prog_first, prog_members, mix_depth, mix_overlap, and each programme's place in fmt and adpcm
// A mix request entry is: programme (-1 = none) start gain_db (the word ninf: muted) pad_after fade_in fade_out; as a
// join request ("join", and the join half of "both") the same six words are read as programme pad_before (gain_db
// skipped) pad_after fade_in fade_out.
#include "jb_output.h"

#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

static const char *name(jb::OutSlab s)
{
    static const char *const names[] = {"none",  "V64",   "S16",    "Voc64",  "Conv64", "Apply64",
                                        "New16", "Fmt",   "Adpcm",  "Join64", "Join16", "Filt64"};
    return (size_t)s < sizeof names / sizeof *names ? names[(size_t)s] : "other";
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

static std::vector<jb::MixUtt> read_request(size_t n)
{
    std::vector<jb::MixUtt> req(n, jb::MixUtt{});
    for (auto &r : req) {
        long long id = 0;
        std::string db;
        std::cin >> id >> r.start >> db >> r.pad_after >> r.fade_in >> r.fade_out;
        r.programme = id < 0 ? jb::kMixNone : (uint32_t)id;
        r.gain_db = db == "ninf" ? -INFINITY : std::stod(db);
    }
    return req;
}

static int layout()
{
    size_t elem = 0, B = 0, nh = 0;
    std::cin >> elem >> B;
    const std::vector<jb::MixUtt> req = read_request(B);
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
    jb::MixLayout lay;
    uint32_t bad = 0;
    const char *field = "";
    const bool ok = jb::mix_layout(req.data(), n.data(), nh ? hz.data() : nullptr, B, elem, &lay, &bad, &field);
    printf("{\"ok\": %s, \"bad\": %lld, \"field\": \"%s\",", ok ? "true" : "false",
           bad == jb::kMixNone ? -1ll : (long long)bad, field);
    list_of("prog_of", lay.progs.group_of, ",");
    list_of("start", lay.start, ",");
    units_of(lay.units, ",");
    printf(" \"total\": %llu, \"gain\": [", (unsigned long long)lay.total);
    for (size_t u = 0; u < lay.gain.size(); u++)
        printf("%s%.17g", u ? ", " : "", lay.gain[u]);
    printf("],");
    list_of("seg_first", lay.seg_first, ",");
    printf(" \"segs\": [");
    for (size_t s = 0; s < lay.segs.size(); s++)
        printf("%s[%llu, %llu, %u, %u]", s ? ", " : "", (unsigned long long)lay.segs[s].k0,
               (unsigned long long)lay.segs[s].k1, lay.segs[s].l0, lay.segs[s].nl);
    printf("],");
    std::vector<uint32_t> who;
    for (uint32_t at : lay.lists)
        who.push_back(lay.progs.members[at]);
    list_of("lists", who, ",");
    list_of("depth", lay.depth, ",");
    list_of("overlap", lay.overlap, "}\n");
    return 0;
}

static int plan()
{
    jb::OutPlanIn in;
    std::string kind;
    int i16 = 0, loudness = 0, flac = 0, adpcm = 0;
    size_t nw = 0;
    std::cin >> kind >> in.voice_hz >> i16 >> loudness >> flac >> in.fmt_bytes >> adpcm >> in.B;
    std::vector<uint64_t> n(in.B), off(in.B);
    for (auto &x : n)
        std::cin >> x;
    for (auto &x : off)
        std::cin >> x;
    std::cin >> nw;
    std::vector<uint32_t> want(nw);
    for (auto &x : want)
        std::cin >> x;
    const std::vector<jb::MixUtt> req = read_request(in.B);
    if (!std::cin || (nw && nw != in.B) || (kind != "mix" && kind != "join" && kind != "both")) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    std::vector<jb::JoinUtt> jreq(in.B, jb::JoinUtt{});
    for (size_t u = 0; u < in.B; u++)
        jreq[u] = {req[u].programme, req[u].fade_in, req[u].fade_out, 0, req[u].start, req[u].pad_after};
    in.n_native = n.data();
    in.off_native = off.data();
    in.i16 = i16 != 0;
    in.loudness = loudness != 0;
    in.flac = flac != 0;
    in.adpcm = adpcm != 0;
    in.want_hz = nw ? want.data() : nullptr;
    in.mix = kind != "join" ? req.data() : nullptr;
    in.join = kind != "mix" ? jreq.data() : nullptr;
    const jb::OutPlan p = jb::plan_output(in);
    printf("{\"final\": \"%s\", \"join_src\": \"%s\", \"join\": \"%s\", \"join_i16\": %s, \"mixed\": %s, \"flac\": \"%s\","
           " \"fmt_src\": \"%s\", \"adpcm_src\": \"%s\", \"join_alloc\": %llu,",
           name(p.final.slab), name(p.join_src.slab), name(p.join.slab), p.join.i16 ? "true" : "false",
           p.mixed ? "true" : "false", name(p.flac), name(p.fmt_src), name(p.adpcm_src.slab),
           (unsigned long long)(p.join.slab == jb::OutSlab::None ? 0 : p.alloc[(size_t)p.join.slab]));
    units_of(p.units, ",");
    list_of("prog_of", p.prog_of, ",");
    list_of("prog_start", p.prog_start, ",");
    list_of("prog_first", p.prog_first, ",");
    list_of("prog_members", p.prog_members, ",");
    list_of("mix_depth", p.mix_depth, ",");
    list_of("mix_overlap", p.mix_overlap, ",");
    printf(" \"fmt\": [");
    for (size_t u = 0; u < p.fmt.size(); u++)
        printf("%s[%llu, %llu]", u ? ", " : "", (unsigned long long)p.fmt[u].off, (unsigned long long)p.fmt[u].bytes);
    printf("], \"adpcm\": [");
    for (size_t u = 0; u < p.adpcm.size(); u++)
        printf("%s[%llu, %llu, %u]", u ? ", " : "", (unsigned long long)p.adpcm[u].off,
               (unsigned long long)p.adpcm[u].bytes, p.adpcm[u].A);
    printf("]}\n");
    return 0;
}

int main()
{
    std::string mode;
    std::cin >> mode;
    if (mode == "layout")
        return layout();
    if (mode == "plan")
        return plan();
    fprintf(stderr, "bad mode\n");
    return 2;
}

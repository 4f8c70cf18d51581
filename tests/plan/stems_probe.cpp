// Prints what the output plan (jbonsai_amd/csrc/jb_output.h) makes of a mix request with a stems request as JSON;
// host-only.  stdin, whitespace-separated, the first word the mode:
//   layout   elem B request[0..B) stems stem_of[0..B) n[0..B)      (stems: 0 = no stems request, the ids are then read
//            and dropped; an id of -1: JB_MIX_NO_STEM)
//            ok, bad, field, P, prog_of, start, units (hz, n, off), total, seg_first, segs (k0, k1, l0, nl), lists (as
//            utterance indices), depth, overlap, stems (programme, id, n_members, first, end), stem_unit
//   plan     i16 fmt_bytes act B n[0..B) request[0..B) stems stem_of[0..B) only[0..B)
//            n_progs, units, stem_unit, unit_parent, the join slab's elements, each unit's place in fmt, the number of
//            the activity layout's units and columns (act: 1 = with an activity request per member), and the redo
//            scope of `only`: post and units
// A mix request entry is: programme (-1 = none) start gain_db (the word ninf: muted) pad_after fade_in fade_out.
#include "jb_output.h"

#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

template <class T> static void list_of(const char *key, const std::vector<T> &v, const char *end)
{
    printf(" \"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++)
        printf("%s%lld", i ? ", " : "", (long long)v[i]);
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

static void stems_of(const std::vector<jb::MixStem> &stems, const char *end)
{
    printf(" \"stems\": [");
    for (size_t s = 0; s < stems.size(); s++)
        printf("%s[%u, %u, %u, %llu, %llu]", s ? ", " : "", stems[s].programme, stems[s].id, stems[s].n_members,
               (unsigned long long)stems[s].first, (unsigned long long)stems[s].end);
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

static std::vector<uint32_t> read_stems(size_t n, int *given)
{
    std::vector<uint32_t> ids(n);
    std::cin >> *given;
    for (auto &x : ids) {
        long long id = 0;
        std::cin >> id;
        x = id < 0 ? jb::kMixNoStem : (uint32_t)id;
    }
    return ids;
}

static int layout()
{
    size_t elem = 0, B = 0;
    int given = 0;
    std::cin >> elem >> B;
    const std::vector<jb::MixUtt> req = read_request(B);
    const std::vector<uint32_t> ids = read_stems(B, &given);
    std::vector<uint64_t> n(B);
    for (auto &x : n)
        std::cin >> x;
    if (!std::cin || (elem != 2 && elem != 8)) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    jb::MixLayout lay;
    uint32_t bad = 0;
    const char *field = "";
    const bool ok =
        jb::mix_layout(req.data(), n.data(), nullptr, B, elem, &lay, &bad, &field, false, given ? ids.data() : nullptr);
    printf("{\"ok\": %s, \"bad\": %lld, \"field\": \"%s\", \"P\": %llu,", ok ? "true" : "false",
           bad == jb::kMixNone ? -1ll : (long long)bad, field, (unsigned long long)lay.programmes());
    list_of("prog_of", lay.progs.group_of, ",");
    list_of("start", lay.start, ",");
    units_of(lay.units, ",");
    printf(" \"total\": %llu,", (unsigned long long)lay.total);
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
    list_of("overlap", lay.overlap, ",");
    stems_of(lay.stems, ",");
    list_of("stem_unit", lay.stem_unit, "}\n");
    return 0;
}

static int plan()
{
    jb::OutPlanIn in;
    int i16 = 0, act = 0, given = 0;
    std::cin >> i16 >> in.fmt_bytes >> act >> in.B;
    std::vector<uint64_t> n(in.B), off(in.B, 0);
    for (auto &x : n)
        std::cin >> x;
    for (size_t u = 1; u < in.B; u++)
        off[u] = off[u - 1] + n[u - 1];
    const std::vector<jb::MixUtt> req = read_request(in.B);
    const std::vector<uint32_t> ids = read_stems(in.B, &given);
    std::vector<uint8_t> only(in.B);
    for (auto &x : only) {
        int v = 0;
        std::cin >> v;
        x = (uint8_t)v;
    }
    if (!std::cin) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    jb::ActOpts o{};
    o.win_us = 400, o.hop_us = 160, o.gate_db = 40.0, o.flags = jb::kActSamples;
    in.voice_hz = 48000;
    in.n_native = n.data();
    in.off_native = off.data();
    in.i16 = i16 != 0;
    in.mix = req.data();
    in.stem_of = given ? ids.data() : nullptr;
    in.activity = act ? &o : nullptr;
    const jb::OutPlan p = jb::plan_output(in);
    printf("{\"n_progs\": %llu, \"mixed\": %s, \"join_alloc\": %llu,", (unsigned long long)p.n_progs,
           p.mixed ? "true" : "false",
           (unsigned long long)(p.join.slab == jb::OutSlab::None ? 0 : p.alloc[(size_t)p.join.slab]));
    units_of(p.units, ",");
    stems_of(p.stems, ",");
    list_of("stem_unit", p.stem_unit, ",");
    list_of("unit_parent", p.unit_parent, ",");
    list_of("mix_depth", p.mix_depth, ",");
    list_of("prog_first", p.prog_first, ",");
    printf(" \"fmt\": [");
    for (size_t u = 0; u < p.fmt.size(); u++)
        printf("%s[%llu, %llu]", u ? ", " : "", (unsigned long long)p.fmt[u].off, (unsigned long long)p.fmt[u].bytes);
    printf("], \"act_fault\": \"%s\", \"act_units\": %llu, \"act_cols\": %llu,", p.act_fault ? p.act_fault : "",
           (unsigned long long)p.act.units.size(), (unsigned long long)p.act.cols.size());
    const jb::RedoScope s = jb::redo_scope(p.prog_of, p.n_progs, jb::LnGroups{}, only, p.unit_parent);
    list_of("redo_post", s.post, ",");
    list_of("redo_units", s.units, "}\n");
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

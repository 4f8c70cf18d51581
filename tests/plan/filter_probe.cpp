// Prints what the output plan (jbonsai_amd/csrc/jb_output.h) makes of a filter request as JSON; host-only.
// stdin, whitespace-separated:
//   voice_hz i16 loudness flac fmt_bytes adpcm adpcm_align  B n_native[0..B) off_native[0..B)
//   nw want_hz[0..nw)  nj request[0..nj)  nf filter[0..nf)     (nw, nj, nf: 0 = not requested, or B)
// the fields of tests/plan/join_probe.cpp's plan mode under the same names, then filter and filter_src.
// A join request entry is: programme (-1 = none) pad_before pad_after fade_in fade_out; a filter entry is 1 where the
// utterance's filter has at least one section, else 0.
#include "jb_output.h"

#include <cstdio>
#include <iostream>
#include <vector>

static const char *name(jb::OutSlab s)
{
    static const char *const names[] = {"none",    "V64",   "S16", "Voc64", "Conv64",
                                        "Apply64", "New16", "Fmt", "Adpcm", "Join64", "Join16", "Filt64"};
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

int main()
{
    jb::OutPlanIn in;
    int i16 = 0, loudness = 0, flac = 0, adpcm = 0;
    size_t nw = 0, nj = 0, nf = 0;
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
    std::cin >> nf;
    std::vector<uint8_t> filt(nf);
    for (auto &x : filt) {
        int v = 0;
        std::cin >> v;
        x = v != 0;
    }
    if (!std::cin || (nw && nw != in.B) || (nj && nj != in.B) || (nf && nf != in.B)) {
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
    in.filter = nf ? filt.data() : nullptr;
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
    list_of("prog_members", p.prog_members, ",");
    write_of("filter", p.filter);
    printf(" \"filter_src\": \"%s\"}\n", name(p.filter_src));
    return 0;
}


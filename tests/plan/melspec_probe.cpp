// Prints the output plan (jbonsai_amd/csrc/jb_output.h) of one batch with a mel spectrogram request as JSON; host-only.
// stdin, whitespace-separated: voice_hz i16 loudness flac fmt_bytes adpcm adpcm_align
//                              melspec n_fft win_length hop_length n_mels pad flags range  B n_native[0..B)
//                              off_native[0..B)  nw want_hz[0..nw)  nj (programme pad_before pad_after)[0..nj)
// (nw, nj: 0 = no rate / no join requested, or B; programme -1 = an utterance of its own)
// The fields of tests/plan/fbank_probe.cpp under the same names (fbank_src and fbank: of no fbank request), then
// melspec_src and melspec (each unit's byte offset, byte count, frames, n_fft, hop and its place in the f64 scratch).
#include "jb_output.h"

#include <cstdio>
#include <iostream>
#include <vector>

static const char *name(jb::OutSlab s)
{
    static const char *const names[] = {"none",   "V64",    "S16",    "Voc64", "Conv64", "Apply64", "New16", "Fmt", "Adpcm",
                                        "Join64", "Join16", "Filt64", "Feat",  "MfccL",  "Mfcc",    "Mel",   "MelY"};
    static_assert(sizeof names / sizeof names[0] == (size_t)jb::OutSlab::Count, "one name per slab");
    return names[(size_t)s];
}

static void write_of(const char *key, const jb::OutWrite &w)
{
    printf(" \"%s\": [\"%s\", \"%s\"],", key, name(w.slab), w.slab == jb::OutSlab::None ? "-" : w.i16 ? "i16" : "f64");
}

int main()
{
    jb::OutPlanIn in;
    jb::MelOpts mo{};
    int i16 = 0, loudness = 0, flac = 0, adpcm = 0, melspec = 0;
    size_t nw = 0, nj = 0;
    std::cin >> in.voice_hz >> i16 >> loudness >> flac >> in.fmt_bytes >> adpcm >> in.adpcm_align;
    std::cin >> melspec >> mo.n_fft >> mo.win_length >> mo.hop_length >> mo.n_mels >> mo.pad >> mo.flags >> mo.range >>
        in.B;
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
    std::vector<jb::JoinUtt> join(nj, jb::JoinUtt{});
    for (auto &j : join) {
        long long prog = 0;
        std::cin >> prog >> j.pad_before >> j.pad_after;
        j.programme = prog < 0 ? jb::kJoinNone : (uint32_t)prog;
    }
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
    in.join = nj ? join.data() : nullptr;
    in.melspec = melspec ? &mo : nullptr;
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
    write_of("join", p.join);
    printf(" \"units\": [");
    for (size_t u = 0; u < p.units.size(); u++)
        printf("%s[%u, %llu, %llu]", u ? ", " : "", p.units[u].hz, (unsigned long long)p.units[u].n,
               (unsigned long long)p.units[u].off);
    printf("],\n \"fbank_src\": \"%s\", \"fbank\": [],\n \"melspec_src\": \"%s\", \"melspec\": [", name(p.fbank_src),
           name(p.melspec_src));
    for (size_t u = 0; u < p.melspec.size(); u++) {
        const jb::OutMelUtt &w = p.melspec[u];
        printf("%s[%llu, %llu, %llu, %u, %u, %llu]", u ? ", " : "", (unsigned long long)w.off,
               (unsigned long long)w.bytes, (unsigned long long)w.T, w.n_fft, w.hop, (unsigned long long)w.yoff);
    }
    printf("]}\n");
    return 0;
}

// mfcc_probe.cpp -- plan_output with a cepstral request (and, beside it, a plain filterbank request) as JSON, for
// tests/test_mfcc_plan.py.  Input: fbank_probe's numbers, then "mfcc win_us hop_us n_fft n_mels flags n_ceps
// delta_order delta_window cmvn mfcc_flags" in front of B.  Plain C++17 without HIP.
#include "jb_output.h"

#include <cstdio>
#include <iostream>
#include <vector>

static const char *name(jb::OutSlab s)
{
    static const char *const names[] = {"none",  "V64", "S16",   "Voc64",  "Conv64", "Apply64", "New16",
                                        "Fmt",   "Adpcm", "Join64", "Join16", "Filt64", "Feat", "MfccL", "Mfcc"};
    return names[(size_t)s];
}

static void write_of(const char *key, const jb::OutWrite &w)
{
    printf(" \"%s\": [\"%s\", \"%s\"],", key, name(w.slab), w.slab == jb::OutSlab::None ? "-" : w.i16 ? "i16" : "f64");
}

int main()
{
    jb::OutPlanIn in;
    jb::FbankOpts fb{}, mfb{};
    jb::MfccOpts mo{};
    int i16 = 0, loudness = 0, flac = 0, adpcm = 0, fbank = 0, mfcc = 0;
    size_t nw = 0, nj = 0;
    std::cin >> in.voice_hz >> i16 >> loudness >> flac >> in.fmt_bytes >> adpcm >> in.adpcm_align;
    std::cin >> fbank >> fb.win_us >> fb.hop_us >> fb.n_fft >> fb.n_mels >> fb.flags;
    std::cin >> mfcc >> mfb.win_us >> mfb.hop_us >> mfb.n_fft >> mfb.n_mels >> mfb.flags;
    std::cin >> mo.n_ceps >> mo.delta_order >> mo.delta_window >> mo.cmvn >> mo.flags >> in.B;
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
    in.fbank = fbank ? &fb : nullptr;
    in.mfcc_fbank = mfcc ? &mfb : nullptr;
    in.mfcc = mfcc ? &mo : nullptr;
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
    printf("],\n \"fbank_src\": \"%s\", \"fbank\": [", name(p.fbank_src));
    for (size_t u = 0; u < p.fbank.size(); u++) {
        const jb::OutFbankUtt &w = p.fbank[u];
        printf("%s[%llu, %llu, %llu, %u, %u, %u]", u ? ", " : "", (unsigned long long)w.off, (unsigned long long)w.bytes,
               (unsigned long long)w.T, w.wl, w.hop, w.n_fft);
    }
    printf("],\n \"mfcc_src\": \"%s\", \"mfcc\": [", name(p.mfcc_src));
    for (size_t u = 0; u < p.mfcc.size(); u++) {
        const jb::OutMfccUtt &w = p.mfcc[u];
        printf("%s[%llu, %llu, %llu, %u, %u, %llu]", u ? ", " : "", (unsigned long long)w.off, (unsigned long long)w.bytes,
               (unsigned long long)w.T, w.width, w.n_fft, (unsigned long long)w.loff);
    }
    printf("]}\n");
    return 0;
}

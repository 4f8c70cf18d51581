// Prints the output plan (jbonsai_amd/csrc/jb_output.h) of one batch with a pitch request as JSON; host-only.
// stdin, whitespace-separated: voice_hz i16 loudness  pitch win_us hop_us grid flags  B n_native[0..B) off_native[0..B)
//                              nw want_hz[0..nw)  mode  then with mode 1 (join) B x (programme pad_before pad_after),
//                              with mode 2 (mix) B x (programme start pad_after stem)
// (nw: 0 = no rate requested, or B; mode 0: neither; programme -1 = an utterance of its own; stem -1 = none, and no
// stems request where every stem is -1)
// Every field of the plan that a request could move: the routing, every slab's elements, the utterances, the units,
// the other sinks' sources; then pitch_src, the two blocks' sizes and each unit's place (byte offset, bytes, T, width,
// element bytes, n4, place in the f64 block).
#include "jb_output.h"

#include <cstdio>
#include <iostream>
#include <vector>

static void write_of(const char *key, const jb::OutWrite &w)
{
    printf(" \"%s\": [%d, %d],", key, (int)w.slab, (int)w.i16);
}

int main()
{
    jb::OutPlanIn in;
    jb::PitchOpts po{};
    int i16 = 0, loudness = 0, pitch = 0, mode = 0;
    size_t nw = 0;
    std::cin >> in.voice_hz >> i16 >> loudness >> pitch >> po.win_us >> po.hop_us >> po.grid >> po.flags >> in.B;
    po.min_f0 = 50.0, po.max_f0 = 400.0, po.delta_pitch = 0.005, po.penalty_factor = 0.1, po.soft_min_f0 = 10.0;
    po.nccf_ballast = 7000.0, po.pov_scale = 2.0, po.pitch_scale = 2.0, po.delta_scale = 10.0;
    po.norm_left = po.norm_right = 75;
    std::vector<uint64_t> n(in.B), off(in.B);
    for (auto &x : n)
        std::cin >> x;
    for (auto &x : off)
        std::cin >> x;
    std::cin >> nw;
    std::vector<uint32_t> want(nw);
    for (auto &x : want)
        std::cin >> x;
    std::cin >> mode;
    std::vector<jb::JoinUtt> join(mode == 1 ? in.B : 0, jb::JoinUtt{});
    std::vector<jb::MixUtt> mix(mode == 2 ? in.B : 0, jb::MixUtt{});
    std::vector<uint32_t> stem(mode == 2 ? in.B : 0);
    bool stems = false;
    for (auto &j : join) {
        long long prog = 0;
        std::cin >> prog >> j.pad_before >> j.pad_after;
        j.programme = prog < 0 ? jb::kJoinNone : (uint32_t)prog;
    }
    for (size_t u = 0; u < mix.size(); u++) {
        long long prog = 0, st = 0;
        std::cin >> prog >> mix[u].start >> mix[u].pad_after >> st;
        mix[u].programme = prog < 0 ? jb::kMixNone : (uint32_t)prog;
        stem[u] = st < 0 ? jb::kMixNoStem : (uint32_t)st;
        stems = stems || st >= 0;
    }
    if (!std::cin || (nw && nw != in.B)) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    in.n_native = n.data();
    in.off_native = off.data();
    in.i16 = i16 != 0;
    in.loudness = loudness != 0;
    in.want_hz = nw ? want.data() : nullptr;
    in.join = mode == 1 ? join.data() : nullptr;
    in.mix = mode == 2 ? mix.data() : nullptr;
    in.stem_of = stems ? stem.data() : nullptr;
    in.pitch = pitch ? &po : nullptr;
    const jb::OutPlan p = jb::plan_output(in);
    printf("{\"convert\": %d, \"active\": %d, \"total\": %llu, \"native_total\": %llu, \"mixed\": %d, \"n_progs\": %zu,",
           (int)p.convert, (int)p.active(), (unsigned long long)p.total, (unsigned long long)p.native_total, (int)p.mixed,
           p.n_progs);
    write_of("vocoder", p.vocoder);
    write_of("converter", p.converter);
    write_of("apply", p.apply);
    write_of("filter", p.filter);
    write_of("final", p.final);
    write_of("join_src", p.join_src);
    write_of("join", p.join);
    write_of("adpcm_src", p.adpcm_src);
    write_of("act_src", p.act_src);
    printf(" \"others\": [%d, %d, %d, %d, %d, %d, %d, %d],\n \"alloc\": [", (int)p.filter_src, (int)p.measure, (int)p.flac,
           (int)p.native64, (int)p.fmt_src, (int)p.fbank_src, (int)p.mfcc_src, (int)p.melspec_src);
    for (size_t s = 0; s < (size_t)jb::OutSlab::Count; s++)
        printf("%s%llu", s ? ", " : "", (unsigned long long)p.alloc[s]);
    printf("],\n \"utt\": [");
    for (size_t u = 0; u < p.utt.size(); u++) {
        const jb::OutUtt &w = p.utt[u];
        printf("%s[%u, %u, %u, %llu, %llu]", u ? ", " : "", w.hz, w.L, w.M, (unsigned long long)w.n,
               (unsigned long long)w.off);
    }
    printf("],\n \"units\": [");
    for (size_t u = 0; u < p.units.size(); u++)
        printf("%s[%u, %llu, %llu]", u ? ", " : "", p.units[u].hz, (unsigned long long)p.units[u].n,
               (unsigned long long)p.units[u].off);
    printf("],\n \"pitch_src\": %d, \"final_slab\": %d, \"join_slab\": %d, \"pitch_bytes\": %llu, \"pitch_words\": %llu, \"pitch\": [",
           (int)p.pitch_src, (int)p.final.slab, (int)p.join.slab, (unsigned long long)p.pitch_bytes,
           (unsigned long long)p.pitch_words);
    for (size_t u = 0; u < p.pitch.size(); u++) {
        const jb::OutPitchUtt &w = p.pitch[u];
        printf("%s[%llu, %llu, %llu, %u, %u, %llu, %llu]", u ? ", " : "", (unsigned long long)w.off,
               (unsigned long long)w.bytes, (unsigned long long)w.T, w.width, w.elem, (unsigned long long)w.n4,
               (unsigned long long)w.yoff);
    }
    printf("]}\n");
    return 0;
}

// Prints what the output plan (jbonsai_amd/csrc/jb_output.h) makes of a speech-activity request as JSON, and runs the
// packed smoothing steps of jbonsai_amd/csrc/jb_activity.h on the host; host-only.
// stdin, whitespace-separated, the first word the mode:
//   plan     kind voice_hz i16 B n_native[0..B) nw want_hz[0..nw) act win hop gate_db grid columns flags min_gap
//            only[0..B) request[0..B)
//            (kind: "mix", "join" or "none"; nw: 0 or B; act: 0 = no activity request; only: the utterances a redo round
//            rewrote; a request entry as tests/plan/mix_probe.cpp reads it)
//            final, join, act_src, act_i16, alloc (every slab's elements), units (off, T, C, wl, hop, col0), cols (unit,
//            utt, start, n, f0, nf, e0, w0), bytes, energies, words, fault, fault_unit, unsupported, and redo_units: the
//            mask of redo_scope the stage follows
//   words    T min_gap min_speech hang_before hang_after bits[0..T)
//            the bits behind close, open and hang as the kernel forms them: word by word from the word's own bits and
//            the nearest set bits carried in from the words in front and behind
#include "jb_output.h"

#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

static const char *name(jb::OutSlab s)
{
    static const char *const names[] = {"none",   "V64",    "S16",    "Voc64", "Conv64", "Apply64", "New16",
                                        "Fmt",    "Adpcm",  "Join64", "Join16", "Filt64", "Feat",    "MfccL",
                                        "Mfcc",   "Mel",    "MelY"};
    return (size_t)s < sizeof names / sizeof *names ? names[(size_t)s] : "other";
}

static int plan()
{
    jb::OutPlanIn in;
    std::string kind;
    int i16 = 0, act = 0;
    size_t nw = 0;
    std::cin >> kind >> in.voice_hz >> i16 >> in.B;
    std::vector<uint64_t> n(in.B), off(in.B);
    for (auto &x : n)
        std::cin >> x;
    for (size_t u = 1; u < in.B; u++)
        off[u] = off[u - 1] + n[u - 1];
    std::cin >> nw;
    std::vector<uint32_t> want(nw);
    for (auto &x : want)
        std::cin >> x;
    jb::ActOpts o{};
    std::cin >> act >> o.win_us >> o.hop_us >> o.gate_db >> o.grid >> o.columns >> o.flags >> o.min_gap;
    std::vector<uint8_t> only(in.B);
    for (auto &x : only) {
        int v = 0;
        std::cin >> v;
        x = (uint8_t)v;
    }
    std::vector<jb::MixUtt> req(in.B, jb::MixUtt{});
    for (auto &r : req) {
        long long id = 0;
        std::string db;
        std::cin >> id >> r.start >> db >> r.pad_after >> r.fade_in >> r.fade_out;
        r.programme = id < 0 ? jb::kMixNone : (uint32_t)id;
        r.gain_db = db == "ninf" ? -INFINITY : std::stod(db);
    }
    if (!std::cin || (nw && nw != in.B) || (kind != "mix" && kind != "join" && kind != "none")) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    std::vector<jb::JoinUtt> jreq(in.B, jb::JoinUtt{});
    for (size_t u = 0; u < in.B; u++)
        jreq[u] = {req[u].programme, req[u].fade_in, req[u].fade_out, 0, req[u].start, req[u].pad_after};
    in.n_native = n.data();
    in.off_native = off.data();
    in.i16 = i16 != 0;
    in.want_hz = nw ? want.data() : nullptr;
    in.mix = kind == "mix" ? req.data() : nullptr;
    in.join = kind == "join" ? jreq.data() : nullptr;
    in.activity = act ? &o : nullptr;
    const jb::OutPlan p = jb::plan_output(in);
    printf("{\"final\": \"%s\", \"join\": \"%s\", \"act_src\": \"%s\", \"act_i16\": %s, \"alloc\": {", name(p.final.slab),
           name(p.join.slab), name(p.act_src.slab), p.act_src.i16 ? "true" : "false");
    for (size_t s = 1; s < (size_t)jb::OutSlab::Count; s++)
        printf("%s\"%s\": %llu", s > 1 ? ", " : "", name((jb::OutSlab)s), (unsigned long long)p.alloc[s]);
    printf("}, \"units\": [");
    for (size_t u = 0; u < p.act.units.size(); u++) {
        const jb::ActLayUnit &w = p.act.units[u];
        printf("%s[%llu, %llu, %u, %u, %u, %u]", u ? ", " : "", (unsigned long long)w.off, (unsigned long long)w.T, w.C,
               w.wl, w.hop, w.col0);
    }
    printf("], \"cols\": [");
    for (size_t c = 0; c < p.act.cols.size(); c++) {
        const jb::ActLayCol &w = p.act.cols[c];
        printf("%s[%u, %u, %llu, %llu, %llu, %llu, %llu, %llu]", c ? ", " : "", w.unit, w.utt,
               (unsigned long long)w.start, (unsigned long long)w.n, (unsigned long long)w.f0, (unsigned long long)w.nf,
               (unsigned long long)w.e0, (unsigned long long)w.w0);
    }
    printf("], \"bytes\": %llu, \"energies\": %llu, \"words\": %llu, \"fault\": \"%s\", \"fault_unit\": %llu,"
           " \"unsupported\": %s, \"redo_units\": [",
           (unsigned long long)p.act.bytes, (unsigned long long)p.act.energies, (unsigned long long)p.act.words,
           p.act_fault ? p.act_fault : "", (unsigned long long)p.act_fault_unit, p.act_unsupported ? "true" : "false");
    const jb::RedoScope scope = jb::redo_scope(p.prog_of, p.units.size(), jb::LnGroups{}, only);
    for (size_t u = 0; u < scope.units.size(); u++)
        printf("%s%d", u ? ", " : "", (int)scope.units[u]);
    printf("]}\n");
    return 0;
}

// One step over the words, as k_act_label's lanes do it: the carried frames by a walk forward and a walk backward
template <class F> static std::vector<uint64_t> step(const std::vector<uint64_t> &src, bool complement, F f)
{
    const size_t nw = src.size();
    std::vector<uint64_t> in(src), out(nw);
    if (complement)
        for (auto &w : in)
            w = ~w;
    std::vector<int64_t> before(nw, -1), behind(nw, (int64_t)1 << 62);
    int64_t carry = -1;
    for (size_t i = 0; i < nw; i++) {
        before[i] = carry;
        if (in[i])
            carry = (int64_t)(i * 64) + 63 - __builtin_clzll(in[i]);
    }
    carry = (int64_t)1 << 62;
    for (size_t i = nw; i-- > 0;) {
        behind[i] = carry;
        if (in[i])
            carry = (int64_t)(i * 64) + __builtin_ctzll(in[i]);
    }
    for (size_t i = 0; i < nw; i++)
        out[i] = f(in[i], (int64_t)(i * 64), before[i], behind[i]);
    return out;
}

static int words()
{
    long long T = 0;
    uint32_t min_gap = 0, min_speech = 0, hang_before = 0, hang_after = 0;
    std::cin >> T >> min_gap >> min_speech >> hang_before >> hang_after;
    std::vector<uint64_t> w((size_t)(T + 63) / 64, 0);
    for (long long t = 0; t < T; t++) {
        int bit = 0;
        std::cin >> bit;
        if (bit)
            w[(size_t)t / 64] |= 1ull << (t % 64);
    }
    if (!std::cin || T < 0) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    if (min_gap)
        w = step(w, false, [&](uint64_t x, int64_t b, int64_t a, int64_t c) {
            return jb::act_close_word(x, b, a, c, T, min_gap);
        });
    if (min_speech > 1)
        w = step(w, true, [&](uint64_t x, int64_t b, int64_t a, int64_t c) {
            return jb::act_open_word(x, b, a, c, T, min_speech);
        });
    if (hang_before || hang_after)
        w = step(w, false, [&](uint64_t x, int64_t b, int64_t a, int64_t c) {
            return jb::act_hang_word(x, b, a, c, T, hang_before, hang_after);
        });
    printf("[");
    for (long long t = 0; t < T; t++)
        printf("%s%d", t ? ", " : "", (int)((w[(size_t)t / 64] >> (t % 64)) & 1));
    printf("]\n");
    return 0;
}

int main()
{
    std::string mode;
    std::cin >> mode;
    if (mode == "plan")
        return plan();
    if (mode == "words")
        return words();
    fprintf(stderr, "bad mode\n");
    return 2;
}

// What the output plan (jbonsai_amd/csrc/jb_output.h) makes of a noise request; host-only.
// stdin, whitespace-separated: the input of tests/plan/fir_probe.cpp (the filter probe's input, then the responses),
// then  nn noise[0..nn)  (nn: 0 = no noise request, or B; an entry is 1 where the utterance has a request -- one at
// snr_db = +INFINITY included: the stage copies it -- else 0).
// stdout: one line {"flags": [...]} -- the plan's filter flag of every utterance (jb_noise.h: noise_stage_flags over
// jb_fir.h: fir_stage_flags) -- then what filter_probe.cpp prints for these flags in the filter entries' place: its
// own main, under another name, fed the rewritten input.
// With "request" as the first word:  snr_db gate_db reference  follow (snr_db may be "inf"); one line
// {"fault": "..." or null, "none": 0|1, "r": 10^(snr_db / 10) or "inf", "gain": the gain of A = 4, C = 2, Bs = 8, N = 4}.
#include "jb_fir.h"
#include "jb_noise.h"

#include <sstream>
#include <string>

#define main filter_probe_main
#include "filter_probe.cpp"
#undef main

int main()
{
    std::string first;
    std::cin >> first;
    if (first == "request") {
        std::string snr;
        double gate = 0.0;
        uint32_t ref = 0;
        std::cin >> snr >> gate >> ref;
        static const double bed[2] = {1.0, -1.0};
        jb::NoiseSpec s{};
        s.bed = bed;
        s.bed_len = 2;
        s.hz = 16000;
        s.snr_db = snr == "inf" ? (double)INFINITY : std::stod(snr);
        s.gate_db = gate;
        s.reference = ref;
        const char *fault = jb::noise_fault(s, 16000);
        const double r = jb::noise_ratio(s.snr_db);
        printf("{\"fault\": %s%s%s, \"none\": %d, \"r\": ", fault ? "\"" : "", fault ? fault : "null", fault ? "\"" : "",
               (int)jb::noise_none(s));
        if (fault) { // (a refused request has no ratio)
            printf("null, \"gain\": null}\n");
            return 0;
        }
        if (std::isinf(r))
            printf("\"inf\"");
        else
            printf("%.17g", r);
        printf(", \"gain\": %.17g}\n", jb::noise_gain(4.0, 2, 8.0, 4, r));
        return 0;
    }
    // the filter probe's input, word for word up to its filter entries
    std::vector<std::string> head{first};
    std::string w;
    for (int i = 0; i < 7 && std::cin >> w; i++) // i16 loudness flac fmt_bytes adpcm adpcm_align B
        head.push_back(w);
    const size_t B = std::stoull(head.back());
    auto take = [&](size_t n) {
        for (size_t i = 0; i < n && std::cin >> w; i++)
            head.push_back(w);
    };
    take(2 * B);
    for (int list = 0; list < 2; list++) { // want_hz, then the join request (five words an entry)
        std::cin >> w;
        head.push_back(w);
        take(std::stoull(w) * (list ? 5 : 1));
    }
    auto flags_in = [&](std::vector<uint8_t> *out) {
        size_t n = 0;
        std::cin >> n;
        out->resize(n);
        for (auto &x : *out) {
            int v = 0;
            std::cin >> v;
            x = v != 0;
        }
    };
    std::vector<uint8_t> sections, resp, noise;
    flags_in(&sections);
    flags_in(&resp);
    flags_in(&noise);
    if (!std::cin || (!sections.empty() && sections.size() != B) || (!resp.empty() && resp.size() != B) ||
        (!noise.empty() && noise.size() != B)) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    std::vector<int32_t> fir_of(resp.size());
    for (size_t u = 0; u < resp.size(); u++)
        fir_of[u] = resp[u] ? 0 : -1;
    const std::vector<uint8_t> flags = jb::noise_stage_flags(jb::fir_stage_flags(sections, fir_of), noise);
    printf("{\"flags\": [");
    for (size_t u = 0; u < flags.size(); u++)
        printf("%s%d", u ? ", " : "", (int)flags[u]);
    printf("]}\n");
    fflush(stdout);
    std::ostringstream in;
    for (const std::string &s : head)
        in << s << ' ';
    in << flags.size();
    for (uint8_t f : flags)
        in << ' ' << (int)f;
    in << '\n';
    std::istringstream fed(in.str());
    std::cin.rdbuf(fed.rdbuf());
    return filter_probe_main();
}

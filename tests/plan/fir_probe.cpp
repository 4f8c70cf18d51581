// What the output plan (jbonsai_amd/csrc/jb_output.h) makes of a convolution request; host-only.
// stdin, whitespace-separated: the input of tests/plan/filter_probe.cpp (its filter entries: 1 where the utterance's
// filter has a section), then  nr resp[0..nr)  (nr: 0 = no convolution request, or B; an entry is 1 where the
// utterance has a response, else 0).
// stdout: one line {"flags": [...]} -- the plan's filter flag of every utterance (jb_fir.h: fir_stage_flags) -- then
// what filter_probe.cpp prints for these flags in the filter entries' place: its own main, under another name, fed
// the rewritten input.
// With "geometry" as the first word: K values follow, one line [mode, block, partitions, n_fft] each.
#include "jb_fir.h"

#include <sstream>
#include <string>

#define main filter_probe_main
#include "filter_probe.cpp"
#undef main

int main()
{
    std::string first;
    std::cin >> first;
    if (first == "geometry") {
        uint32_t K = 0;
        while (std::cin >> K) {
            const jb::FirGeom g = jb::fir_geometry(K);
            printf("[%u, %u, %u, %u]\n", g.mode, g.block, g.partitions, g.n_fft);
        }
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
    size_t nf = 0, nr = 0;
    std::cin >> nf;
    std::vector<uint8_t> sections(nf);
    for (auto &x : sections) {
        int v = 0;
        std::cin >> v;
        x = v != 0;
    }
    std::cin >> nr;
    std::vector<int32_t> fir_of(nr);
    for (auto &x : fir_of) {
        int v = 0;
        std::cin >> v;
        x = v ? 0 : -1;
    }
    if (!std::cin || (nf && nf != B) || (nr && nr != B)) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    const std::vector<uint8_t> flags = jb::fir_stage_flags(sections, fir_of);
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

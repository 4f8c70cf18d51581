// Prints what the shape rules of Batch::create and the group split of an engine request (jbonsai_amd/csrc/jb_plan.h)
// decide, as JSON; host-only, no GPU.
// stdin, whitespace-separated, one request:
//   blocks  f_lo f_hi n_lo n_hi                        -> [[bs, nblk] for fperiod in f_lo..f_hi for nlpf in n_lo..n_hi]
//   runs    n lf0[0..n)                                -> {"durations": [...], "msd": [...]}
//   cond    alpha beta volume nmcp stage  nv (alpha beta volume)[0..nv)         (nv: -1 = no per-utterance entries)
//   stream  L W is_msd use_gv width[0..W) si flags stage from_tracks mt_max_dim
//   groups  cases (n_utts forced one_batch labels[0..n_utts))[0..cases)   -> [glo of each case]; labels: each
//           utterance's label lines (line_off starts at 3: the rule reads differences only)
#include "jb_plan.h"

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

static int fail()
{
    fprintf(stderr, "bad input\n");
    return 2;
}

static void print_voc(const jb::VocUtt &u)
{
    printf("{\"alpha\": %.17g, \"volume\": %.17g, \"beta\": %.17g, \"beta_stage\": %.17g, \"pf\": %u}", u.alpha, u.volume,
           u.beta, u.beta_stage, u.pf);
}

int main()
{
    std::string what;
    std::cin >> what;
    if (what == "blocks") {
        int f_lo = 0, f_hi = 0, n_lo = 0, n_hi = 0;
        std::cin >> f_lo >> f_hi >> n_lo >> n_hi;
        if (!std::cin || f_lo < 1)
            return fail();
        printf("[");
        for (int f = f_lo; f <= f_hi; f++)
            for (int nl = n_lo; nl <= n_hi; nl++) {
                const jb::FrameBlocks fb = jb::plan_frame_blocks(f, nl);
                printf("%s[%d, %d]", (f == f_lo && nl == n_lo) ? "" : ", ", fb.bs, fb.nblk);
            }
        printf("]\n");
    } else if (what == "runs") {
        size_t n = 0;
        std::cin >> n;
        std::vector<double> lf0(n);
        for (auto &x : lf0)
            std::cin >> x;
        if (!std::cin)
            return fail();
        std::vector<uint32_t> dur;
        std::vector<double> msd;
        jb::plan_voiced_runs(lf0.data(), n, dur, msd);
        printf("{\"durations\": [");
        for (size_t k = 0; k < dur.size(); k++)
            printf("%s%u", k ? ", " : "", dur[k]);
        printf("], \"msd\": [");
        for (size_t k = 0; k < msd.size(); k++)
            printf("%s%.17g", k ? ", " : "", msd[k]);
        printf("]}\n");
    } else if (what == "cond") {
        jb_utt_voc voice{};
        uint32_t nmcp = 0, stage = 0;
        long nv = -1;
        std::cin >> voice.alpha >> voice.beta >> voice.volume >> nmcp >> stage >> nv;
        std::vector<jb_utt_voc> utt(nv > 0 ? (size_t)nv : 0);
        for (auto &u : utt)
            std::cin >> u.alpha >> u.beta >> u.volume;
        if (!std::cin)
            return fail();
        const jb::VocCondPlan p =
            jb::plan_voc_conditions(voice, nmcp, stage, nv < 0 ? nullptr : utt.data(), nv < 0 ? 0 : (size_t)nv);
        printf("{\"mixed\": %s, \"n_classes\": %u, \"batch\": ", p.mixed ? "true" : "false", p.n_classes);
        print_voc(p.batch);
        printf(",\n \"utt\": [");
        for (size_t i = 0; i < p.utt.size(); i++) {
            printf("%s", i ? ", " : "");
            print_voc(p.utt[i]);
        }
        printf("],\n \"cls\": [");
        for (size_t i = 0; i < p.cls.size(); i++)
            printf("%s%u", i ? ", " : "", p.cls[i]);
        printf("], \"pf_alphas\": [");
        for (size_t i = 0; i < p.pf_alphas.size(); i++)
            printf("%s%.17g", i ? ", " : "", p.pf_alphas[i]);
        printf("]}\n");
    } else if (what == "stream") {
        jb_stream_desc s{};
        uint32_t si = 0, flags = 0, stage = 0;
        int from_tracks = 0, mt_max_dim = 0;
        std::cin >> s.vector_length >> s.num_windows >> s.is_msd >> s.use_gv;
        if (!std::cin || s.num_windows > JB_MAX_WINDOW)
            return fail();
        for (uint32_t w = 0; w < s.num_windows; w++)
            std::cin >> s.win_width[w];
        std::cin >> si >> flags >> stage >> from_tracks >> mt_max_dim;
        if (!std::cin)
            return fail();
        const jb::StreamMode m = jb::plan_stream_mode(s, si, flags, stage, from_tracks != 0, mt_max_dim);
        printf("{\"W\": %d, \"BW\": %d, \"is_msd\": %d, \"use_gv\": %d, \"mt\": %d, \"defer_out\": %d, \"is_static\": %s}\n",
               m.W, m.BW, m.is_msd, m.use_gv, m.mt, m.defer_out, m.is_static ? "true" : "false");
    } else if (what == "groups") {
        size_t cases = 0;
        std::cin >> cases;
        printf("[");
        for (size_t c = 0; c < cases; c++) {
            size_t n = 0;
            int forced = 0, one_batch = 0;
            std::cin >> n >> forced >> one_batch;
            if (!std::cin || n > 4096)
                return fail();
            std::vector<size_t> off(n + 1, 3);
            for (size_t u = 0; u < n; u++) {
                size_t labels = 0;
                std::cin >> labels;
                off[u + 1] = off[u] + labels;
            }
            if (!std::cin)
                return fail();
            // (no utterance: line_off is not read)
            const std::vector<size_t> glo = jb::plan_synth_groups(n ? off.data() : nullptr, n, forced, one_batch != 0);
            printf("%s[", c ? ",\n " : "");
            for (size_t g = 0; g < glo.size(); g++)
                printf("%s%zu", g ? ", " : "", glo[g]);
            printf("]");
        }
        printf("]\n");
    } else
        return fail();
    return 0;
}

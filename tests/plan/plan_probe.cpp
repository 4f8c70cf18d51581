// Prints the vocoder's work plan (jbonsai_amd/csrc/jb_plan.h) of one batch shape as JSON; host-only, no GPU.
// stdin, whitespace-separated: nmcp fperiod stage flags chunk_frames warmup_frames
//                              B T[0..B)  nk first_of_kind[0..nk)  nc voc_class[0..nc)   (nk, nc: 0 = absent, or B)
#include "jb_plan.h"

#include <cstdio>
#include <iostream>
#include <vector>

int main()
{
    jb::VocPlanIn in;
    size_t B = 0, nk = 0, nc = 0;
    std::cin >> in.nmcp >> in.fperiod >> in.stage >> in.flags >> in.chunk_frames >> in.warmup_frames >> B;
    std::vector<uint32_t> T(B), cls;
    for (auto &t : T)
        std::cin >> t;
    std::cin >> nk;
    std::vector<unsigned> kind(nk);
    for (auto &k : kind)
        std::cin >> k;
    std::cin >> nc;
    cls.resize(nc);
    for (auto &c : cls)
        std::cin >> c;
    if (!std::cin || (nk && nk != B) || (nc && nc != B)) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    std::vector<uint8_t> first(kind.begin(), kind.end());
    in.T = T.data();
    in.B = B;
    in.first_of_kind = nk ? first.data() : nullptr;
    in.voc_class = nc ? cls.data() : nullptr;
    const jb::VocPlan p = jb::plan_vocoder_work(in);
    printf("{\"lane_kernel\": %s, \"waves_per_simd\": %d, \"chunk_frames\": %u, \"warmup_frames\": %u, "
           "\"ckpt_frames\": %u, \"ckpt2_frames\": %u,\n \"items\": [",
           p.lane_kernel ? "true" : "false", p.waves_per_simd, p.chunk_frames, p.warmup_frames, p.ckpt_frames,
           p.ckpt2_frames);
    for (size_t k = 0; k < p.items.size(); k++) {
        const jb::VocPlanItem &w = p.items[k];
        printf("%s[%u, %u, %u, %u, %u]", k ? ", " : "", w.utt, w.t_start, w.t_out, w.t_end, (unsigned)w.saves);
    }
    printf("],\n \"order\": [");
    for (size_t k = 0; k < p.order.size(); k++)
        printf("%s%u", k ? ", " : "", p.order[k]);
    printf("]}\n");
    return 0;
}

// Prints what the host half of a jb_*_pcm_batch call does (jbonsai_amd/csrc/jb_pcm_call.h: pcm_check, pcm_pack,
// pcm_hand_out) as JSON; host-only.  stdin, whitespace-separated, one of:
//   check n  lists (0: the lists are NULL)  null_in (the index of a NULL in[u], or -1)  n_in[0..min(n, 8))
//   pack  n  n_in[0..n)
//   hand  n  fail (the 1-based allocation that fails, 0: none)  elem  {off n}[0..n)   over a slab of bytes 0, 1, 2, ...
#include "jb_pcm_call.h"

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

static int g_fail = 0, g_allocs = 0, g_frees = 0;

static void *counting_alloc(size_t bytes)
{
    if (bytes == 0 || ++g_allocs == g_fail)
        return nullptr;
    return malloc(bytes);
}

static void counting_free(void *p)
{
    g_frees++;
    free(p);
}

int main()
{
    std::string what;
    unsigned long long n = 0;
    std::cin >> what >> n;
    if (what == "check") {
        // (a refused n is refused before a list is walked: the lists here hold 8 entries at the most)
        int lists = 0;
        long long null_in = -1;
        std::cin >> lists >> null_in;
        const size_t held = (size_t)(n < 8 ? n : 8);
        std::vector<size_t> n_in(held + 1, 0);
        for (size_t u = 0; u < held; u++)
            std::cin >> n_in[u];
        if (!std::cin)
            return 2;
        static const double sample = 0.0;
        std::vector<const void *> in(held + 1, &sample);
        if (null_in >= 0 && (size_t)null_in < held)
            in[(size_t)null_in] = nullptr;
        std::vector<void *> out(held + 1, (void *)&in);
        std::vector<size_t> n_out(held + 1, 7);
        const int rc = lists ? jb::pcm_check(in.data(), n_in.data(), (size_t)n, true, out.data(), n_out.data())
                             : jb::pcm_check(nullptr, nullptr, (size_t)n);
        size_t cleared = 0;
        for (size_t u = 0; u < held; u++)
            cleared += !out[u] && !n_out[u];
        printf("{\"rc\": %d, \"cleared\": %zu}\n", rc, cleared);
        return 0;
    }
    if (what == "pack") {
        std::vector<size_t> n_in((size_t)n);
        for (size_t &x : n_in)
            std::cin >> x;
        if (!std::cin)
            return 2;
        const std::vector<uint64_t> off = jb::pcm_pack(n_in.data(), n_in.size());
        printf("{\"off\": [");
        for (size_t i = 0; i < off.size(); i++)
            printf("%s%llu", i ? ", " : "", (unsigned long long)off[i]);
        printf("]}\n");
        return 0;
    }
    if (what != "hand")
        return 2;
    size_t elem = 0;
    std::cin >> g_fail >> elem;
    std::vector<jb::PcmShare> shares((size_t)n);
    uint64_t end = 0;
    for (jb::PcmShare &s : shares) {
        std::cin >> s.off >> s.n;
        end = s.off + s.n > end ? s.off + s.n : end;
    }
    if (!std::cin || !elem)
        return 2;
    std::vector<uint8_t> slab((size_t)end * elem);
    for (size_t i = 0; i < slab.size(); i++)
        slab[i] = (uint8_t)i;
    std::vector<void *> out(shares.size(), nullptr);
    std::vector<size_t> n_out(shares.size(), 0);
    const char *err = "";
    const int rc = jb::pcm_hand_out(slab.data(), elem, shares, out.data(), n_out.data(), &err,
                                    jb::PcmAlloc{counting_alloc, counting_free});
    printf("{\"rc\": %d, \"err\": \"%s\", \"allocs\": %d, \"frees\": %d, \"out\": [", rc, err,
           g_allocs - (g_fail && g_allocs >= g_fail), g_frees);
    for (size_t u = 0; u < out.size(); u++) {
        // null, or the share's bytes
        if (!out[u]) {
            printf("%snull", u ? ", " : "");
            continue;
        }
        printf("%s[", u ? ", " : "");
        for (size_t i = 0; i < n_out[u] * elem; i++)
            printf("%s%u", i ? ", " : "", (unsigned)((const uint8_t *)out[u])[i]);
        printf("]");
        free(out[u]);
    }
    printf("], \"n_out\": [");
    for (size_t u = 0; u < n_out.size(); u++)
        printf("%s%zu", u ? ", " : "", n_out[u]);
    printf("]}\n");
    return 0;
}

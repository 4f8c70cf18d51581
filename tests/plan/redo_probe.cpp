// Prints what a redo round runs again (jbonsai_amd/csrc/jb_output.h: redo_scope, pick_renumbered) as JSON; host-only.
// stdin, whitespace-separated, one of:
//   scope B  n_groups group[0..n_groups) (0 or B entries; 4294967295 = no group)
//            n_prog prog_of[0..n_prog) (0 or B entries: each utterance's programme)  P  only[0..B)
//   pick  N  mask[0..N)  count[0..N)
#include "jb_output.h"

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

template <class T> static void list(const char *key, const std::vector<T> &v, const char *end)
{
    printf(" \"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++)
        printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    printf("]%s", end);
}

template <class T> static std::vector<T> read(size_t n)
{
    std::vector<T> v(n);
    for (T &x : v) {
        unsigned long long t = 0;
        std::cin >> t;
        x = (T)t;
    }
    return v;
}

int main()
{
    std::string what;
    size_t n = 0;
    std::cin >> what >> n;
    if (what == "pick") {
        const std::vector<uint8_t> mask = read<uint8_t>(n);
        const std::vector<uint64_t> count = read<uint64_t>(n);
        if (!std::cin)
            return 2;
        const jb::Picked p = jb::pick_renumbered(mask, count);
        printf("{");
        list("index", p.index, ",");
        list("base", p.base, ",");
        printf(" \"total\": %llu}\n", (unsigned long long)p.total);
        return 0;
    }
    size_t n_groups = 0, n_prog = 0, P = 0;
    std::cin >> n_groups;
    const std::vector<uint32_t> group = read<uint32_t>(n_groups);
    std::cin >> n_prog;
    const std::vector<uint32_t> prog_of = read<uint32_t>(n_prog);
    std::cin >> P;
    const std::vector<uint8_t> only = read<uint8_t>(n);
    if (!std::cin || what != "scope" || (n_groups && n_groups != n) || (n_prog && n_prog != n))
        return 2;
    jb::LnGroups g;
    if (n_groups) {
        jb::LnGroupsIn in;
        in.B = n;
        in.group = group.data();
        if (!jb::plan_loudness_groups(in, &g, nullptr, nullptr))
            return 3;
    }
    const jb::RedoScope s = jb::redo_scope(prog_of, P, g, only);
    printf("{");
    list("measured", s.measured, ",");
    list("post", s.post, ",");
    list("units", s.units, ",");
    list("touched_groups", s.touched_groups, ",");
    list("group_of", g.group_of, "}\n");
    return 0;
}

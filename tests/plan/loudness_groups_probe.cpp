// Prints the loudness group bookkeeping (jbonsai_amd/csrc/jb_output.h: plan_loudness_groups and
// loudness_groups_closure) of one request as JSON; host-only.
// stdin, whitespace-separated: B  group[0..B) (4294967295 = no group)  has_target  target[0..B) ceiling[0..B)
//                              mode[0..B)  hz[0..B)  touched[0..B)      (targets and ceilings as strtod reads them)
#include "jb_output.h"

#include <cstdio>
#include <cstdlib>
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

int main()
{
    jb::LnGroupsIn in;
    int has_target = 0;
    std::cin >> in.B;
    std::vector<uint32_t> group(in.B), mode(in.B), hz(in.B);
    std::vector<double> target(in.B), ceiling(in.B);
    std::vector<uint8_t> touched(in.B);
    for (auto &x : group)
        std::cin >> x;
    std::cin >> has_target;
    for (std::vector<double> *v : {&target, &ceiling})
        for (auto &x : *v) {
            std::string tok;
            std::cin >> tok;
            x = strtod(tok.c_str(), nullptr);
        }
    for (auto &x : mode)
        std::cin >> x;
    for (auto &x : hz)
        std::cin >> x;
    for (auto &x : touched) {
        unsigned t = 0;
        std::cin >> t;
        x = (uint8_t)t;
    }
    if (!std::cin) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    in.group = group.data();
    in.target = has_target ? target.data() : nullptr;
    in.ceiling = has_target ? ceiling.data() : nullptr;
    in.mode = mode.data();
    in.hz = hz.data();
    jb::LnGroups g;
    uint32_t bad = 0;
    const char *field = "";
    if (!jb::plan_loudness_groups(in, &g, &bad, &field)) {
        printf("{\"ok\": false, \"bad_group\": %u, \"bad_field\": \"%s\"}\n", bad, field);
        return 0;
    }
    std::vector<uint8_t> cg, cm;
    jb::loudness_groups_closure(g, touched, &cg, &cm);
    printf("{\"ok\": true,");
    list("group_of", g.group_of, ",");
    list("first", g.first, ",");
    list("members", g.members, ",");
    list("closure_groups", cg, ",");
    list("closure_members", cm, "}\n");
    return 0;
}

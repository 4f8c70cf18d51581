// Drives the rules of the vocoder's redo rounds (jbonsai_amd/csrc/jb_plan.h: redo_pick_round .. redo_recertify) to
// completion, in the order Batch::finish_verify calls them, with the comparisons' outcomes supplied; host-only.
// Prints every round as JSON.
// stdin, whitespace-separated:
//   ckpt2 (0 / 1: the plan has second checkpoints)  n  A
//   utt saves                 n times: the items (saves: kSave* bits)
//   pending[0..n)             the hand-offs that failed the first check
//   code[0..n)[0..A)          the outcomes of chunk k at its attempt a (the last column for every later one).  Bit 1:
//                             its first comparison of a round (checkpoint or speculative end) fails; 2: the one at the
//                             second checkpoint fails; 4: its re-certification fails.  The attempt counts the rounds
//                             that held the chunk before (bits 1, 2), the earlier re-certifications of it (bit 4)
#include "jb_plan.h"

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <vector>

using namespace jb;

static void list(const char *key, const std::vector<uint32_t> &v, const char *end = ",")
{
    printf(" \"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++)
        printf("%s%u", i ? ", " : "", v[i]);
    printf("]%s", end);
}

static std::vector<uint32_t> where(const std::vector<uint8_t> &flags)
{
    std::vector<uint32_t> v;
    for (size_t k = 0; k < flags.size(); k++)
        if (flags[k])
            v.push_back((uint32_t)k);
    return v;
}

int main()
{
    unsigned ckpt2 = 0;
    size_t n = 0, A = 0;
    std::cin >> ckpt2 >> n >> A;
    if (!std::cin || n == 0 || A == 0 || n > (1u << 20) || A > 64)
        return 2;
    std::vector<VocPlanItem> items(n);
    for (VocPlanItem &it : items) {
        unsigned saves = 0;
        std::cin >> it.utt >> saves;
        it.t_start = it.t_out = it.t_end = 0;
        it.saves = (uint8_t)saves;
    }
    std::vector<uint8_t> pending(n);
    std::vector<unsigned> code(n * A);
    for (uint8_t &p : pending) {
        unsigned v = 0;
        std::cin >> v;
        p = v != 0;
    }
    for (unsigned &c : code)
        std::cin >> c;
    if (!std::cin || pending[0])
        return 2;
    std::vector<size_t> tries(n, 0), recerts(n, 0);
    auto outcome = [&](uint32_t k, size_t attempt, unsigned bit) { return (code[k * A + std::min(attempt, A - 1)] & bit) != 0; };

    uint32_t n_redo = 0, n_partial = 0, n_full = 0, n_recert_failed = 0;
    for (uint8_t p : pending)
        n_redo += p;
    printf("{\"rounds\": [");
    for (size_t round = 0;; round++) {
        const RedoPick pick = redo_pick_round(items, pending);
        if (pick.ids.empty())
            break;
        if (round >= n) { // (every round makes the lowest pending chunk final: there are fewer than n)
            fprintf(stderr, "no end after %zu rounds\n", round);
            return 3;
        }
        const RedoStageA a = redo_stage_a(items, pick);
        std::vector<uint8_t> unsettled(n, 0), at2(n, 0);
        for (uint32_t j : a.part)
            unsettled[pick.ids[j]] = outcome(pick.ids[j], tries[pick.ids[j]], 1);
        const std::vector<uint32_t> mid = redo_second_checkpoint(items, pick.ids, unsettled, ckpt2 != 0);
        for (uint32_t k : mid) {
            at2[k] = 1;
            unsettled[k] = outcome(k, tries[k], 2);
        }
        const RedoSettled s = redo_settle(items, pick, pending, a.spec_end, unsettled);
        n_partial += s.n_partial;
        n_full += s.n_full;
        for (uint32_t k : pick.ids) {
            tries[k]++;
            if (s.final_now[k])
                pending[k] = 0;
        }
        const std::vector<uint32_t> succ = redo_recertify(items, s.full_ids, pick.in_round, pending);
        std::vector<uint32_t> failed;
        for (uint32_t k : succ)
            if (outcome(k, recerts[k]++, 4)) {
                pending[k] = 1;
                n_redo++;
                n_recert_failed++;
                failed.push_back(k);
            }
        std::vector<uint32_t> part;
        for (uint32_t j : a.part)
            part.push_back(pick.ids[j]);
        printf("%s\n {", round ? "," : "");
        list("ids", pick.ids);
        list("part", part);
        list("spec_end", where(a.spec_end));
        list("unsettled", where(unsettled));
        list("mid", mid);
        list("final", where(s.final_now));
        list("rest", s.rest);
        list("full_ids", s.full_ids);
        list("succ", succ);
        list("recert_failed", failed);
        printf(" \"n_partial\": %u, \"n_full\": %u,", s.n_partial, s.n_full);
        list("pending", where(pending), "}");
    }
    printf("],\n \"n_redo\": %u, \"n_redo_partial\": %u, \"n_redo_full\": %u, \"n_recert_failed\": %u}\n", n_redo, n_partial,
           n_full, n_recert_failed);
    return 0;
}

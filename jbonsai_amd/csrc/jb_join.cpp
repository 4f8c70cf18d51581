// jb_join.cpp -- the host half of the join stage: the request check and the geometry (both the one layout's) and
// the rules of jb_join.h over PCM the caller holds without a GPU (jb_join_host, what the kernel is checked against).
#include "jb_host.h"

#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(JoinUtt) == sizeof(jb_join_utt) && offsetof(JoinUtt, programme) == offsetof(jb_join_utt, programme) &&
                  offsetof(JoinUtt, fade_in) == offsetof(jb_join_utt, fade_in) &&
                  offsetof(JoinUtt, fade_out) == offsetof(jb_join_utt, fade_out) &&
                  offsetof(JoinUtt, reserved) == offsetof(jb_join_utt, reserved) &&
                  offsetof(JoinUtt, pad_before) == offsetof(jb_join_utt, pad_before) &&
                  offsetof(JoinUtt, pad_after) == offsetof(jb_join_utt, pad_after) && kJoinNone == JB_JOIN_NONE,
              "jb_join.h restates the header's request");

int join_layout_checked(const JoinUtt *req, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem,
                        MixLayout *out, const char *who)
{
    return mix_layout_checked(join_as_mix(req, B).data(), true, n, hz, B, elem, nullptr, out, who);
}

namespace {

template <class T>
int join_host(const T *const *in, const size_t *n_in, size_t n, const jb_join_utt *req, T *const *out, const size_t *cap,
              const char *who)
{
    if (n && (!in || !n_in || !req || !out || !cap))
        return JB_ERR_INVALID;
    for (size_t u = 0; u < n; u++)
        if (n_in[u] && !in[u])
            return JB_ERR_INVALID;
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    int rc = join_layout_checked((const JoinUtt *)req, ns.data(), nullptr, n, sizeof(T), &lay, who);
    if (rc)
        return rc;
    for (size_t p = 0; p < lay.units.size(); p++) {
        if (cap[p] < lay.units[p].n) {
            set_error(std::string(who) + ": the buffer is too small");
            return JB_ERR_BUFFER;
        }
        if (lay.units[p].n && !out[p])
            return JB_ERR_INVALID;
    }
    for (size_t p = 0; p < lay.units.size(); p++) {
        T *y = out[p];
        uint64_t k = 0; // written so far
        for (uint32_t i = lay.progs.first[p]; i < lay.progs.first[p + 1]; i++) {
            const uint32_t u = lay.progs.members[i];
            for (; k < lay.start[u]; k++)
                y[k] = (T)0;
            for (uint64_t j = 0; j < n_in[u]; j++)
                y[k++] = join_sample(in[u][j], j, n_in[u], req[u].fade_in, req[u].fade_out);
        }
        for (; k < lay.units[p].n; k++)
            y[k] = (T)0;
    }
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

uint64_t jb_join_ms_to_samples(double ms, uint32_t hz) { return join_ms_to_samples(ms, hz); }

int jb_join_geometry(const jb_join_utt *req, const size_t *n_in, const uint32_t *hz, size_t n, uint32_t *programme_of,
                     uint64_t *member_start, size_t *n_programmes, uint64_t *programme_samples)
{
    if (n && (!req || !n_in))
        return JB_ERR_INVALID;
    std::vector<uint64_t> ns(n_in, n_in + n);
    MixLayout lay;
    int rc = join_layout_checked((const JoinUtt *)req, ns.data(), hz, n, sizeof(double), &lay, "jb_join_geometry");
    if (rc)
        return rc;
    for (size_t u = 0; u < n; u++) {
        if (programme_of)
            programme_of[u] = lay.progs.group_of[u];
        if (member_start)
            member_start[u] = lay.start[u];
    }
    if (n_programmes)
        *n_programmes = lay.units.size();
    if (programme_samples)
        for (size_t p = 0; p < lay.units.size(); p++)
            programme_samples[p] = lay.units[p].n;
    return JB_OK;
}

int jb_join_host(const double *const *in, const size_t *n_in, size_t n, const jb_join_utt *req, double *const *out,
                 const size_t *cap)
{
    return join_host(in, n_in, n, req, out, cap, "jb_join_host");
}

int jb_join_i16_host(const int16_t *const *in, const size_t *n_in, size_t n, const jb_join_utt *req,
                     int16_t *const *out, const size_t *cap)
{
    return join_host(in, n_in, n, req, out, cap, "jb_join_i16_host");
}

void jb_join_free(void *p) { free(p); }

} // extern "C"

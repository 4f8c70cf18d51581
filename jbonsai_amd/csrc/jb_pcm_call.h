#pragma once
// jb_pcm_call.h -- what every stand-alone entry on PCM the caller holds (jb_*_pcm_batch) does around its stage: the
// check of the input lists, the packing of the inputs one after the other, and the hand-out of each output's share of
// one host slab in a malloc'ed buffer of its own.  Plain C++17 without HIP: made and tested on any host
// (tests/plan/pcm_call_probe.cpp); DeviceScratch (jb_host.h) is the device half of the same call.
#include "../../include/jbonsai_amd.h"

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace jb {

// The lists of a call of n utterances: JB_ERR_INVALID for a missing list (lists: the entry's other lists are all
// there), n above 2^31 - 1, or a NULL in[u] of n_in[u] != 0 samples; out (with n_out, either may be null) is cleared
// before the inputs are looked at
inline int pcm_check(const void *const *in, const size_t *n_in, size_t n, bool lists = true, void **out = nullptr,
                     size_t *n_out = nullptr)
{
    if (n && (!in || !n_in || !lists))
        return JB_ERR_INVALID;
    if (n > 0x7fffffffu)
        return JB_ERR_INVALID;
    for (size_t u = 0; u < n; u++) {
        if (out)
            out[u] = nullptr;
        if (n_out)
            n_out[u] = 0;
    }
    for (size_t u = 0; u < n; u++)
        if (n_in[u] && !in[u])
            return JB_ERR_INVALID;
    return JB_OK;
}

// off[n + 1]: the inputs laid one after the other (as a batch's slab has them), in elements
inline std::vector<uint64_t> pcm_pack(const size_t *n_in, size_t n)
{
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t u = 0; u < n; u++)
        off[u + 1] = off[u] + n_in[u];
    return off;
}

struct PcmShare { // an output's place in the host copy of a slab, in elements
    uint64_t off, n;
};
struct PcmAlloc { // where the outputs come from (a host test makes the k-th allocation fail)
    void *(*alloc)(size_t) = malloc;
    void (*release)(void *) = free;
};
// out[u]: a buffer of max(bytes, 1) with shares[u] of `host` (elements of `elem` bytes); n_out[u] (may be null): its
// elements.  A failed allocation frees and clears what was handed out, names itself in *err and is JB_ERR_INVALID
inline int pcm_hand_out(const void *host, size_t elem, const std::vector<PcmShare> &shares, void **out, size_t *n_out,
                        const char **err, PcmAlloc a = PcmAlloc{})
{
    for (size_t u = 0; u < shares.size(); u++) {
        const size_t bytes = (size_t)shares[u].n * elem;
        if (!(out[u] = a.alloc(bytes ? bytes : 1))) {
            for (size_t k = 0; k < u; k++) {
                a.release(out[k]);
                out[k] = nullptr;
                if (n_out)
                    n_out[k] = 0;
            }
            *err = "out of host memory";
            return JB_ERR_INVALID;
        }
        if (bytes)
            memcpy(out[u], (const uint8_t *)host + (size_t)shares[u].off * elem, bytes);
        if (n_out)
            n_out[u] = (size_t)shares[u].n;
    }
    return JB_OK;
}

} // namespace jb

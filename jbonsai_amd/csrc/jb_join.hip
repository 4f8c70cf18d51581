// jb_join.hip -- the join stage on the device: the chain's final PCM, f64 or 16-bit, gathered into programmes (members
// one after the other between their pads, under their fades) by the rules of jb_join.h, from the members and the spans
// the mix is launched with too (the stand-alone entries: jb_mix.hip, beside the mix's).
//
//   k_join<T>   one workgroup per tile of kProgTileBytes of one span of one programme (tiles never cross spans; every
//               programme starts on a 16-byte boundary of the join slab).  A lane takes groups of 16 destination bytes
//               -- 2 f64 or 8 16-bit samples -- and stores each as one dwordx4.  A group inside one member is one
//               load of the member's samples at whatever alignment they have (the f64 slab is 8-byte aligned, the
//               16-bit one 2-byte aligned: global memory takes the under-aligned dwordx4, and nothing in front of a
//               member's first sample or behind its last one is read), with the fade weights only where the group
//               touches a fade; a group inside a pad is zeros; a group across a boundary is put together sample by
//               sample in registers.  Only a programme's last partial group goes out sample by sample.  The tile's
//               first and last member are found once per workgroup (uniform), so a lane bisects only in tiles that
//               hold a boundary.  A pure streaming pass, no LDS: a member's samples in the programme depend on its own
//               samples and its two fade lengths alone.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

typedef double JoinD2 __attribute__((ext_vector_type(2)));
typedef double JoinD2u __attribute__((ext_vector_type(2), aligned(8)));
typedef int16_t JoinS8 __attribute__((ext_vector_type(8)));
typedef int16_t JoinS8u __attribute__((ext_vector_type(8), aligned(2)));
// (a pointer read from the work list is generic to the compiler: named global, the accesses are global_ ones)
#define JB_JOIN_GLOBAL __attribute__((address_space(1)))

template <class T> struct JoinVec;
template <> struct JoinVec<double> {
    typedef JoinD2 V;
    typedef JoinD2u U;
};
template <> struct JoinVec<int16_t> {
    typedef JoinS8 V;
    typedef JoinS8u U;
};

__device__ __forceinline__ uint32_t join_span_of(const ProgSpan *spans, uint32_t n, uint64_t idx)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (spans[mid].t0 <= idx)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

template <class T>
__global__ __launch_bounds__(kProgLanes) void k_join(const ProgSpan *__restrict__ spans, uint32_t n_spans,
                                                     const ProgMember *__restrict__ members_all)
{
    constexpr uint32_t G = kProgGroupBytes / sizeof(T);
    constexpr uint32_t kTile = kProgTileBytes / sizeof(T);
    static_assert(kTile % (kProgLanes * G) == 0, "a tile is whole groups of every lane");
    typedef typename JoinVec<T>::V V;
    typedef typename JoinVec<T>::U U;
    const ProgSpan S = spans[join_span_of(spans, n_spans, blockIdx.x)];
    const uint64_t k0 = S.k0 + (blockIdx.x - S.t0) * (uint64_t)kTile;
    if (k0 >= S.k1)
        return;
    const uint64_t k1 = std::min<uint64_t>(k0 + kTile, S.k1);
    const ProgMember *mem = members_all + S.m0;
    const int32_t last = (int32_t)S.nm - 1;
    // the members of the tile's first and last sample (uniform): a lane's search stays between them
    bool in0, in1;
    const int32_t jlo = std::max(join_find(mem, 0, last, k0, &in0), 0);
    const int32_t jhi = std::max(join_find(mem, jlo, last, k1 - 1, &in1), 0);
    JB_JOIN_GLOBAL T *gy = (JB_JOIN_GLOBAL T *)S.y;
#pragma unroll
    for (uint32_t i = 0; i < kTile / (kProgLanes * G); i++) {
        const uint64_t ks = k0 + (uint64_t)(i * kProgLanes + threadIdx.x) * G;
        if (ks + G <= k1) {
            bool inside;
            const int32_t j = join_find(mem, jlo, jhi, ks, &inside);
            const ProgMember m = mem[std::max(j, 0)];
            const uint64_t next = j < last ? mem[j + 1].start : S.n; // where the pad behind member j ends
            V v;
            if (j >= 0 && inside && ks + G <= m.start + m.n) {
                // inside one member
                const uint64_t ka = ks - m.start;
                v = *(const JB_JOIN_GLOBAL U *)((const JB_JOIN_GLOBAL T *)m.x + ka);
                if (!join_plain(ka, ka + G - 1, m.n, m.fade_in, m.fade_out)) {
#pragma unroll
                    for (uint32_t q = 0; q < G; q++)
                        v[q] = join_sample((T)v[q], ka + q, m.n, m.fade_in, m.fade_out);
                }
            } else if (!inside && ks + G <= next) {
                // inside one pad
                v = (V)(T)0;
            } else {
                // across a boundary
#pragma unroll
                for (uint32_t q = 0; q < G; q++)
                    v[q] = join_value<T>(mem, jlo, jhi, ks + q);
            }
            *(JB_JOIN_GLOBAL V *)(gy + ks) = v;
        } else if (ks < k1) {
            // the programme's last partial group
            for (uint64_t k = ks; k < k1; k++)
                gy[k] = join_value<T>(mem, jlo, jhi, k);
        }
    }
}

} // namespace

hipError_t launch_join(bool i16, const ProgSpan *spans_dev, uint32_t n, uint64_t tiles, const ProgMember *members_dev,
                       hipStream_t stream)
{
    if (n == 0 || tiles == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (i16)
        hipLaunchKernelGGL((k_join<int16_t>), dim3((uint32_t)tiles), dim3(kProgLanes), 0, stream, spans_dev, n,
                           members_dev);
    else
        hipLaunchKernelGGL((k_join<double>), dim3((uint32_t)tiles), dim3(kProgLanes), 0, stream, spans_dev, n,
                           members_dev);
    return hipGetLastError();
}

} // namespace jb

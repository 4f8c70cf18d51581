// jb_join.hip -- the join stage on the device: the chain's final PCM, f64 or 16-bit, gathered into programmes (members
// one after the other between their pads, under their fades) by the rules of jb_join.h.
//
//   k_join<T>   one workgroup per tile of kJoinTileBytes of one span of one programme (tiles never cross spans; every
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

__device__ __forceinline__ uint32_t join_span_of(const JoinSpan *spans, uint32_t n, uint64_t idx)
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
__global__ __launch_bounds__(kJoinLanes) void k_join(const JoinSpan *__restrict__ spans, uint32_t n_spans,
                                                     const JoinMember *__restrict__ members_all)
{
    constexpr uint32_t G = kJoinGroupBytes / sizeof(T);
    constexpr uint32_t kTile = kJoinTileBytes / sizeof(T);
    static_assert(kTile % (kJoinLanes * G) == 0, "a tile is whole groups of every lane");
    typedef typename JoinVec<T>::V V;
    typedef typename JoinVec<T>::U U;
    const JoinSpan S = spans[join_span_of(spans, n_spans, blockIdx.x)];
    const uint64_t k0 = S.k0 + (blockIdx.x - S.t0) * (uint64_t)kTile;
    if (k0 >= S.k1)
        return;
    const uint64_t k1 = std::min<uint64_t>(k0 + kTile, S.k1);
    const JoinMember *mem = members_all + S.m0;
    const int32_t last = (int32_t)S.nm - 1;
    // the members of the tile's first and last sample (uniform): a lane's search stays between them
    bool in0, in1;
    const int32_t jlo = std::max(join_find(mem, 0, last, k0, &in0), 0);
    const int32_t jhi = std::max(join_find(mem, jlo, last, k1 - 1, &in1), 0);
    JB_JOIN_GLOBAL T *gy = (JB_JOIN_GLOBAL T *)S.y;
#pragma unroll
    for (uint32_t i = 0; i < kTile / (kJoinLanes * G); i++) {
        const uint64_t ks = k0 + (uint64_t)(i * kJoinLanes + threadIdx.x) * G;
        if (ks + G <= k1) {
            bool inside;
            const int32_t j = join_find(mem, jlo, jhi, ks, &inside);
            const JoinMember m = mem[std::max(j, 0)];
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

hipError_t launch_join(bool i16, const JoinSpan *spans_dev, uint32_t n, uint64_t tiles, const JoinMember *members_dev,
                       hipStream_t stream)
{
    if (n == 0 || tiles == 0)
        return hipSuccess;
    if (tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    if (i16)
        hipLaunchKernelGGL((k_join<int16_t>), dim3((uint32_t)tiles), dim3(kJoinLanes), 0, stream, spans_dev, n,
                           members_dev);
    else
        hipLaunchKernelGGL((k_join<double>), dim3((uint32_t)tiles), dim3(kJoinLanes), 0, stream, spans_dev, n,
                           members_dev);
    return hipGetLastError();
}

namespace {

// jb_join_pcm_batch / _i16: the inputs packed one after the other on the device (as a batch's slab has them), the
// programmes of the geometry each on a 16-byte boundary
template <class T>
int join_pcm_batch(const T *const *in, const size_t *n_in, size_t n, const jb_join_utt *req, int32_t device, T **out,
                   size_t *n_out, size_t *n_programmes, const char *who)
{
    if (n_programmes)
        *n_programmes = 0;
    int rc = pcm_check((const void *const *)in, n_in, n, req && out && n_out, (void **)out, n_out);
    if (rc)
        return rc;
    std::vector<uint64_t> ns(n_in, n_in + n);
    JoinLayout lay;
    if ((rc = join_layout_checked((const JoinUtt *)req, ns.data(), nullptr, n, sizeof(T), &lay, who)))
        return rc;
    const size_t P = lay.progs.size();
    DeviceScratch ds;
    if ((rc = ds.open(device, who)))
        return rc;
    std::vector<uint64_t> xoff;
    const T *dx = ds.pack(in, n_in, n, &xoff);
    T *dy = ds.alloc<T>(lay.total);
    std::vector<JoinMember> members;
    std::vector<JoinSpan> spans;
    join_lists(lay, (const JoinUtt *)req, ns.data(), xoff.data(), dx, dy, sizeof(T), &members, &spans);
    uint64_t tiles = 0;
    for (const JoinSpan &w : spans)
        tiles += join_tiles(w.k0, w.k1, sizeof(T) == 2);
    const JoinMember *dm = ds.upload(members);
    const JoinSpan *dsp = ds.upload(spans);
    if (ds.ok())
        ds.err = launch_join(sizeof(T) == 2, dsp, (uint32_t)P, tiles, dm, ds.stream);
    std::vector<T> host;
    ds.read_back(&host, dy, lay.total);
    if ((rc = ds.status()))
        return rc;
    std::vector<PcmShare> shares(P);
    for (size_t p = 0; p < P; p++)
        shares[p] = {lay.units[p].off, lay.units[p].n};
    if ((rc = hand_out(host.data(), sizeof(T), shares, (void **)out, n_out)))
        return rc;
    if (n_programmes)
        *n_programmes = P;
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_join_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_join_utt *req, int32_t device,
                      double **out, size_t *n_out, size_t *n_programmes)
{
    return join_pcm_batch(in, n_in, n, req, device, out, n_out, n_programmes, "jb_join_pcm_batch");
}

int jb_join_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_join_utt *req,
                          int32_t device, int16_t **out, size_t *n_out, size_t *n_programmes)
{
    return join_pcm_batch(in, n_in, n, req, device, out, n_out, n_programmes, "jb_join_pcm_batch_i16");
}

} // extern "C"

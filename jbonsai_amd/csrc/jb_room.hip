// jb_room.hip -- room responses on the device (jb_room.h): the impulse response of a shoebox room by the image-source
// method, one lane per tap.
//
//   k_room   one workgroup of 256 lanes per 256 consecutive taps of one room; the grid is (tap tiles, distinct rooms).
//            The room's three axis tables (D2, g) and the low-pass table F are staged in LDS (sized by the launch's largest
//            room: at most 80 KiB).  Lane l forms tap k0 + l by the rule of jb_room.h: i ascends over the x table, j over
//            the y table, m over the z table, every term through room_term in that order.  What the workgroup's taps
//            can reach is a band of squared distances (room_reach, widened by 2^-30): the tables are sorted, so the i
//            and j loops end at the first entry beyond the band, and per (i, j) the window of z entries is found once
//            by bisection on D2z and widened by one entry on either side (room_window) -- the same for every lane;
//            inside the window every lane applies the exact test.  A skipped term is one the test refuses, so a tap
//            has the bits of the full triple loop.  Arithmetic-bound: a square root and a division in f64 per term;
//            no atomics, nothing whose order the scheduling sets.  An even lane stores its tap and its neighbour's as
//            one 16-byte store (a room's taps start at an even index of the slab); a last single tap goes out alone.
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

namespace {

#define JB_ROOM_GLOBAL __attribute__((address_space(1)))
typedef double RoomD2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(kRoomLanes) void k_room(const RoomDev *__restrict__ rooms,
                                                     const double *__restrict__ image,
                                                     const double *__restrict__ Fg, double *__restrict__ out)
{
    extern __shared__ double s_room[]; // F (kRoomTable + 1 doubles: the tables start at an even index), then the tables
    double *s_F = s_room, *s_tab = s_room + kRoomTable + 1;
    const RoomDev R = rooms[blockIdx.y];
    const uint32_t K = R.c.K, k0 = blockIdx.x * kRoomLanes, l = threadIdx.x;
    if (k0 >= K)
        return;
    const uint32_t nx = R.n[0], ny = R.n[1], nz = R.n[2], words = 2 * (nx + ny + nz);
    const JB_ROOM_GLOBAL double *gt = (const JB_ROOM_GLOBAL double *)image + R.tab;
    const JB_ROOM_GLOBAL double *gf = (const JB_ROOM_GLOBAL double *)Fg;
    for (uint32_t w = l; w < words; w += kRoomLanes)
        s_tab[w] = gt[w];
    for (uint32_t w = l; w < kRoomTable; w += kRoomLanes)
        s_F[w] = gf[w];
    __syncthreads();
    const double *D2x = s_tab, *gx = D2x + nx, *D2y = gx + nx, *gy = D2y + ny, *D2z = gy + ny, *gz = D2z + nz;
    double lo2, hi2;
    room_reach(k0, std::min(k0 + kRoomLanes - 1, K - 1), R.c.kappa, &lo2, &hi2);
    const uint32_t k = k0 + l;
    const double kd = (double)k;
    double acc = 0.0;
    for (uint32_t i = 0; i < nx; i++) {
        const double dx = D2x[i], wx = gx[i];
        if (dx > hi2)
            break;
        for (uint32_t j = 0; j < ny; j++) {
            const double dy = D2y[j], wy = gy[j], sxy = dx + dy;
            if (sxy > hi2)
                break;
            uint32_t m0, m1;
            room_window(D2z, nz, sxy, lo2, hi2, &m0, &m1);
            for (uint32_t m = m0; m < m1; m++)
                acc = room_term(acc, dx, dy, D2z[m], wx, wy, gz[m], kd, R.c, s_F);
        }
    }
    const double next = __shfl_down(acc, 1, 64);
    if (l & 1u)
        return;
    JB_ROOM_GLOBAL double *o = (JB_ROOM_GLOBAL double *)out + R.out + k;
    if (k + 1 < K)
        *(JB_ROOM_GLOBAL RoomD2 *)o = RoomD2{acc, next};
    else if (k < K)
        *o = acc;
}

} // namespace

hipError_t launch_room(const RoomDev *rooms_dev, uint32_t n, uint32_t tiles, uint32_t table_words, const double *image,
                       const double *F, double *out, hipStream_t stream)
{
    if (n == 0 || tiles == 0)
        return hipSuccess;
    if (n > 65535u || table_words > 6 * kRoomMaxAxis)
        return hipErrorInvalidValue;
    const uint32_t lds = room_lds(table_words);
    if (lds > 64 * 1024) { // above the default limit of a launch's dynamic LDS
        const hipError_t attr =
            hipFuncSetAttribute((const void *)k_room, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRoomLds + 8);
        if (attr != hipSuccess)
            return attr;
    }
    hipLaunchKernelGGL(k_room, dim3(tiles, n), dim3(kRoomLanes), lds, stream, rooms_dev, image, F, out);
    return hipGetLastError();
}

int room_rirs(const jb_room *r, size_t n, int device, std::vector<std::vector<double>> *h,
              std::vector<RoomTables> *tabs, const char *who)
{
    h->assign(n, std::vector<double>());
    if (tabs)
        tabs->assign(n, RoomTables{});
    // the distinct rooms, by content (JB_ROOM_KEEP_LATENCY does not enter the taps)
    std::vector<jb_room> keys;
    std::vector<RoomTables> T;
    std::vector<int32_t> of(n, -1);
    for (size_t u = 0; u < n; u++) {
        if (room_none(*(const RoomSpec *)&r[u]))
            continue;
        jb_room key = r[u];
        key.flags &= ~kRoomKeepLatency;
        for (size_t i = 0; i < keys.size() && of[u] < 0; i++)
            if (!memcmp(&keys[i], &key, sizeof(jb_room)))
                of[u] = (int32_t)i;
        if (of[u] >= 0)
            continue;
        RoomTables t;
        const int rc = room_check(&r[u], u, who, &t);
        if (rc)
            return rc;
        of[u] = (int32_t)keys.size();
        keys.push_back(key);
        T.push_back(std::move(t));
    }
    if (keys.empty())
        return JB_OK;
    std::vector<double> image;
    std::vector<RoomDev> rooms(T.size());
    uint64_t total = 0;
    for (size_t i = 0; i < T.size(); i++) {
        RoomDev &d = rooms[i];
        d = RoomDev{};
        d.tab = image.size();
        d.out = total;
        for (int a = 0; a < 3; a++) {
            d.n[a] = (uint32_t)T[i].D2[a].size();
            image.insert(image.end(), T[i].D2[a].begin(), T[i].D2[a].end());
            image.insert(image.end(), T[i].g[a].begin(), T[i].g[a].end());
        }
        d.c = RoomConst{T[i].kappa, T[i].fourpi, T[i].d0, T[i].unit, T[i].K};
        total += ((uint64_t)T[i].K + 1) & ~1ull;
    }
    DeviceScratch ds;
    int rc = ds.open(device, who);
    if (rc)
        return rc;
    const double *dF = ds.upload(room_lowpass());
    const double *dimg = ds.upload(image);
    const RoomDev *drooms = ds.upload(rooms);
    double *dout = ds.alloc<double>((size_t)total);
    // launches of at most kRoomLaunchVisits pair visits (a room above the budget alone: a launch of its own)
    for (size_t a = 0; a < T.size() && ds.ok();) {
        size_t b = a;
        uint64_t visits = 0;
        uint32_t tiles = 0, words = 0;
        while (b < T.size() && b - a < 65535 && (b == a || visits + T[b].visits() <= kRoomLaunchVisits)) {
            visits += T[b].visits();
            tiles = std::max(tiles, (uint32_t)T[b].workgroups());
            words = std::max(words, 2 * (rooms[b].n[0] + rooms[b].n[1] + rooms[b].n[2]));
            b++;
        }
        ds.err = launch_room(drooms + a, (uint32_t)(b - a), tiles, words, dimg, dF, dout, ds.stream);
        a = b;
    }
    std::vector<double> host;
    ds.read_back(&host, dout, (size_t)total);
    if ((rc = ds.status()))
        return rc;
    for (size_t u = 0; u < n; u++) {
        if (of[u] < 0)
            continue;
        const size_t i = (size_t)of[u];
        (*h)[u].assign(host.begin() + (ptrdiff_t)rooms[i].out, host.begin() + (ptrdiff_t)(rooms[i].out + T[i].K));
        if (tabs)
            (*tabs)[u] = T[i];
    }
    return JB_OK;
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_room_rir_batch(const jb_room *r, size_t n, int32_t device, double **h, size_t *n_h)
{
    if (n && (!r || !h || !n_h))
        return JB_ERR_INVALID;
    if (n > 0x7fffffffu)
        return JB_ERR_INVALID;
    for (size_t u = 0; u < n; u++) {
        h[u] = nullptr;
        n_h[u] = 0;
    }
    // (every room first: a refused call has touched no device)
    for (size_t u = 0; u < n; u++) {
        const int rc = room_check(&r[u], u, "jb_room_rir_batch", nullptr);
        if (rc)
            return rc;
    }
    std::vector<std::vector<double>> taps;
    int rc = room_rirs(r, n, device, &taps, nullptr, "jb_room_rir_batch");
    if (rc)
        return rc;
    std::vector<double> host;
    std::vector<PcmShare> shares(n);
    for (size_t u = 0; u < n; u++) {
        shares[u] = {host.size(), taps[u].size()};
        host.insert(host.end(), taps[u].begin(), taps[u].end());
    }
    return hand_out(host.data(), sizeof(double), shares, (void **)h, n_h);
}

} // extern "C"

#pragma once
// jb_room.h -- room responses (include/jbonsai_amd.h "Room responses"): the impulse response of a shoebox room by the
// image-source method of Allen and Berkley, made on the device and handed to the convolution stage.  The rule, stated
// once for the kernel (jb_room.hip) and for the host rule (jb_room.cpp): the low-pass interpolator's table and its
// lookup, the axis tables (host, long double, rounded once), one term of a tap and the order of a tap's terms; the
// request check; the kernel's device items.
// Plain C++17; under hipcc the rule compiles for the host and the device alike.
#include "jb_format.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define JB_ROOM_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define JB_ROOM_HD inline
#endif

namespace jb {

constexpr uint32_t kRoomUnitDirect = 1, kRoomKeepLatency = 2; // JB_ROOM_UNIT_DIRECT, JB_ROOM_KEEP_LATENCY
constexpr uint32_t kRoomVary = 1;                             // JB_ROOM_VARY
constexpr uint32_t kRoomWh = 32, kRoomQ = 128;                // JB_ROOM_WH, JB_ROOM_Q
constexpr uint32_t kRoomTable = kRoomQ * kRoomWh + 3;         // F[0 .. Q Wh] and the two zeros above
constexpr uint32_t kRoomMaxAxis = 1024;                       // JB_ROOM_MAX_AXIS
constexpr uint32_t kRoomMaxTaps = 131072;                     // JB_FIR_MAX_TAPS
constexpr uint32_t kRoomLanes = 256;                          // taps of a workgroup of k_room
constexpr uint64_t kRoomMaxVisits = 1ull << 32;               // entries_x entries_y K of one room
constexpr double kRoomSound = 343.0;                          // c == 0
constexpr double kRoomMinApart = 0.01;                        // metres between source and microphone
// LDS of a workgroup at the bound: three axis tables of (D2, g), 48 KiB, and F, 32 KiB, of a CU's 160 KiB (48 bytes
// too many for two workgroups per CU).  A launch takes what its largest room needs (room_lds): the tables of a room
// of a few metres take a few hundred bytes beside F, and four workgroups share a CU
constexpr uint32_t kRoomLds = 3 * 2 * 8 * kRoomMaxAxis + 8 * kRoomTable;
static_assert(kRoomLds <= 160 * 1024, "three axis tables and F fit in LDS together");
constexpr uint32_t room_lds(uint32_t table_words) { return 8 * (kRoomTable + 1 + table_words); }
// The reach of a workgroup's taps is widened by this much (relative, on squared distances) before an entry is
// skipped: 2^-30, against the 2^-52 of the roundings between a squared distance and the exact test
constexpr double kRoomSlack = 1.0 / (double)(1u << 30);
// The launch budget, in pair visits (entries_x entries_y K, summed over a launch's rooms): a call's rooms are cut
// into launches of at most this many, so that no launch runs long.  profiles/r25_room.txt (tools/room_cost.py): whole
// calls of 256 rooms (tables, upload and read-back included) run at 3.3e10 to 9.0e10 pair visits a second, so a launch
// of 2^35 = 3.4e10 takes 0.4 to 1.05 s at the most (a room of many z entries per pair may take a few times that)
constexpr uint64_t kRoomLaunchVisits = 1ull << 35;

// jb_room of the public header, restated (this header stands without it; jb_room.cpp asserts the two agree)
struct RoomSpec {
    double size[3], source[3], mic[3], beta[6], c;
    uint32_t hz, n_taps, flags, reserved;
};

// "no room for this utterance": every byte zero
inline bool room_none(const RoomSpec &r)
{
    static const RoomSpec z{};
    return !memcmp(&r, &z, sizeof(RoomSpec));
}

inline double room_sound(const RoomSpec &r) { return r.c == 0.0 ? kRoomSound : r.c; }

// What is wrong with the fields of a room, naming the field; empty: nothing.  (The direct index, the tables' sizes
// and the work bound need the tables: room_check, jb_room.cpp.)
inline std::string room_fault(const RoomSpec &r)
{
    static const char *axis[3] = {"0", "1", "2"};
    if (r.reserved)
        return "reserved must be 0";
    if (r.flags & ~(kRoomUnitDirect | kRoomKeepLatency))
        return "flags holds an unknown flag";
    for (int a = 0; a < 3; a++)
        if (!(r.size[a] >= 0.5 && r.size[a] <= 1000.0))
            return std::string("size[") + axis[a] + "] is outside [0.5, 1000] m";
    for (int a = 0; a < 3; a++) {
        if (!(r.source[a] > 0.0 && r.source[a] < r.size[a]))
            return std::string("source[") + axis[a] + "] is not strictly inside the room";
        if (!(r.mic[a] > 0.0 && r.mic[a] < r.size[a]))
            return std::string("mic[") + axis[a] + "] is not strictly inside the room";
    }
    for (int w = 0; w < 6; w++)
        if (!(fabs(r.beta[w]) < 1.0))
            return std::string("beta[") + std::to_string(w) + "] is not in (-1, 1)";
    if (!(r.c == 0.0 || (r.c >= 50.0 && r.c <= 5000.0)))
        return "c is neither 0 nor in [50, 5000] m/s";
    if (r.hz < 1000 || r.hz > 768000)
        return "hz is outside 1000..768000";
    if (r.n_taps == 0 || r.n_taps > kRoomMaxTaps)
        return "n_taps is outside 1..JB_FIR_MAX_TAPS (131072)";
    const double dx = r.source[0] - r.mic[0], dy = r.source[1] - r.mic[1], dz = r.source[2] - r.mic[2];
    if (!(sqrt((dx * dx + dy * dy) + dz * dz) >= kRoomMinApart))
        return "source and mic are closer than 1 cm";
    return std::string();
}

// The tables of one room: per axis the entries (D2 = D^2, g) sorted by |D|, ties by (n, p); kappa = hz / c, 4 pi,
// the direct distance and index
struct RoomTables {
    std::vector<double> D2[3], g[3];
    double kappa = 0.0, fourpi = 0.0, d0 = 0.0;
    uint32_t direct = 0, K = 0, unit = 0;
    uint64_t visits() const { return (uint64_t)D2[0].size() * D2[1].size() * K; }
    uint64_t workgroups() const { return (K + kRoomLanes - 1) / kRoomLanes; }
};

// What a term needs beside its table entries
struct RoomConst {
    double kappa, fourpi, d0;
    uint32_t unit, K;
};

// lp(t), |t| < Wh
JB_ROOM_HD double room_lp(const double *F, double t)
{
    const double u = fabs(t) * (double)kRoomQ;
    const uint32_t i0 = (uint32_t)u; // floor: u >= 0
    const double f = u - (double)i0;
    return __builtin_fma(f, F[i0 + 1] - F[i0], F[i0]);
}

// One term of tap k onto acc
JB_ROOM_HD double room_term(double acc, double D2x, double D2y, double D2z, double gx, double gy, double gz, double k,
                            const RoomConst &c, const double *F)
{
    const double s2 = (D2x + D2y) + D2z;
    const double d = __builtin_sqrt(s2);
    const double tau = d * c.kappa;
    const double t = k - tau;
    if (fabs(t) < (double)kRoomWh) {
        const double div = c.unit ? d / c.d0 : c.fourpi * d;
        const double A = ((gx * gy) * gz) / div;
        acc = __builtin_fma(A, room_lp(F, t), acc);
    }
    return acc;
}

// What the terms of the taps [k0, k1] can reach, as squared distances [lo2, hi2], widened by kRoomSlack: a term of
// s2 outside fails the exact test for every one of those taps
JB_ROOM_HD void room_reach(uint32_t k0, uint32_t k1, double kappa, double *lo2, double *hi2)
{
    const double hi = ((double)k1 + (double)kRoomWh) / kappa;
    *hi2 = hi * hi * (1.0 + kRoomSlack);
    const double lo = k0 > kRoomWh ? ((double)k0 - (double)kRoomWh) / kappa : 0.0;
    *lo2 = lo * lo * (1.0 - kRoomSlack);
}

// The z entries [m0, m1) that a pair of sxy = D2x + D2y can put inside [lo2, hi2]: by bisection on the sorted D2z,
// widened by one entry on either side
JB_ROOM_HD void room_window(const double *D2z, uint32_t nz, double sxy, double lo2, double hi2, uint32_t *m0,
                            uint32_t *m1)
{
    const double a = lo2 - sxy, b = hi2 - sxy;
    uint32_t l = 0, h = nz;
    while (l < h) { // the first entry not below a
        const uint32_t mid = (l + h) >> 1;
        if (D2z[mid] < a)
            l = mid + 1;
        else
            h = mid;
    }
    *m0 = l ? l - 1 : 0;
    h = nz;
    while (l < h) { // the first entry above b
        const uint32_t mid = (l + h) >> 1;
        if (D2z[mid] <= b)
            l = mid + 1;
        else
            h = mid;
    }
    *m1 = l < nz ? l + 1 : nz;
}

// One distinct room of a launch on the device: its tables in the launch's image (doubles from `tab`: D2x, gx, D2y,
// gy, D2z, gz one after the other), its taps in the output slab (out, a multiple of two doubles)
struct RoomDev {
    uint64_t tab, out;
    uint32_t n[3], pad;
    RoomConst c;
};

} // namespace jb

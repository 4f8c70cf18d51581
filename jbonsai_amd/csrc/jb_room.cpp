// jb_room.cpp -- the host half of the room responses: the request check, the low-pass table and the axis tables (long
// double, rounded once), Eyring's design, the varied positions, the report of a response, and the rule of jb_room.h
// without a GPU (jb_room_host, what the kernel is checked against).
#include "jb_host.h"

#include <algorithm>
#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(RoomSpec) == sizeof(jb_room) && offsetof(RoomSpec, size) == offsetof(jb_room, size) &&
                  offsetof(RoomSpec, source) == offsetof(jb_room, source) &&
                  offsetof(RoomSpec, mic) == offsetof(jb_room, mic) && offsetof(RoomSpec, beta) == offsetof(jb_room, beta) &&
                  offsetof(RoomSpec, c) == offsetof(jb_room, c) && offsetof(RoomSpec, hz) == offsetof(jb_room, hz) &&
                  offsetof(RoomSpec, n_taps) == offsetof(jb_room, n_taps) &&
                  offsetof(RoomSpec, flags) == offsetof(jb_room, flags) &&
                  offsetof(RoomSpec, reserved) == offsetof(jb_room, reserved),
              "jb_room.h restates the header's request");
static_assert(kRoomUnitDirect == JB_ROOM_UNIT_DIRECT && kRoomKeepLatency == JB_ROOM_KEEP_LATENCY &&
                  kRoomVary == JB_ROOM_VARY && kRoomWh == JB_ROOM_WH && kRoomQ == JB_ROOM_Q &&
                  kRoomMaxAxis == JB_ROOM_MAX_AXIS && kRoomMaxTaps == JB_FIR_MAX_TAPS,
              "jb_room.h restates the header's constants");
static_assert(sizeof(jb_room) == 144 && sizeof(jb_room_info) == 40 && sizeof(jb_room_report) == 24,
              "the layouts the bindings restate");

const std::vector<double> &room_lowpass()
{
    static const std::vector<double> F = [] {
        std::vector<double> f(kRoomTable, 0.0);
        const long double pi = acosl(-1.0L);
        const uint32_t top = kRoomQ * kRoomWh;
        for (uint32_t q = 0; q <= top; q++) {
            const uint32_t n = q / kRoomQ, rq = q % kRoomQ;
            long double sinc;
            if (rq == 0)
                sinc = n == 0 ? 1.0L : 0.0L;
            else
                sinc = ((n & 1u) ? -1.0L : 1.0L) * sinl(pi * ((long double)rq / kRoomQ)) /
                       (pi * ((long double)q / kRoomQ));
            const long double s = sinl(pi * (long double)(top - q) / (2.0L * top));
            f[q] = (double)(sinc * (s * s));
        }
        return f;
    }();
    return F;
}

namespace {

struct AxisEntry {
    long double a; // |D|
    int32_t n, p;
    double D2, g;
};

long double ipow(long double b, uint32_t e)
{
    long double r = 1.0L;
    for (; e; e >>= 1, b *= b)
        if (e & 1u)
            r *= b;
    return r;
}

// false: more than kRoomMaxAxis entries
bool axis_table(long double L, long double s, long double r, long double b0, long double b1, long double Rmax,
                std::vector<double> *D2, std::vector<double> *g)
{
    const int32_t Na = (int32_t)ceill(Rmax / (2.0L * L)) + 1;
    std::vector<AxisEntry> e;
    for (int32_t n = -Na; n <= Na; n++)
        for (int32_t p = 0; p < 2; p++) {
            AxisEntry x;
            const long double D = ((long double)(1 - 2 * p) * s + 2.0L * (long double)n * L) - r;
            x.g = (double)(ipow(b0, (uint32_t)abs(n - p)) * ipow(b1, (uint32_t)abs(n)));
            if (x.g == 0.0)
                continue;
            x.a = fabsl(D);
            x.n = n;
            x.p = p;
            x.D2 = (double)(D * D);
            e.push_back(x);
            if (e.size() > kRoomMaxAxis)
                return false;
        }
    std::sort(e.begin(), e.end(), [](const AxisEntry &x, const AxisEntry &y) {
        return x.a != y.a ? x.a < y.a : x.n != y.n ? x.n < y.n : x.p < y.p;
    });
    D2->clear();
    g->clear();
    for (const AxisEntry &x : e) {
        D2->push_back(x.D2);
        g->push_back(x.g);
    }
    return true;
}

int fail(int rc, const char *who, size_t idx, const std::string &what)
{
    set_error(std::string(who) + ": room " + std::to_string(idx) + ": " + what);
    return rc;
}

} // namespace

int room_check(const jb_room *r, size_t idx, const char *who, RoomTables *out)
{
    if (!r)
        return fail(JB_ERR_INVALID, who, idx, "the room is NULL");
    const RoomSpec &s = *(const RoomSpec *)r;
    const std::string fault = room_fault(s);
    if (!fault.empty())
        return fail(JB_ERR_INVALID, who, idx, fault);
    RoomTables t;
    const long double c = (long double)room_sound(s);
    t.kappa = (double)((long double)s.hz / c);
    t.fourpi = (double)(4.0L * acosl(-1.0L));
    t.K = s.n_taps;
    t.unit = (s.flags & kRoomUnitDirect) ? 1u : 0u;
    // d0: the rule's expression for the three (n = 0, p = 0) entries
    double D2o[3];
    for (int a = 0; a < 3; a++) {
        const long double D = (long double)s.source[a] - (long double)s.mic[a];
        D2o[a] = (double)(D * D);
    }
    t.d0 = sqrt((D2o[0] + D2o[1]) + D2o[2]);
    const double di = floor(t.d0 * t.kappa + 0.5);
    if (!(di < (double)s.n_taps))
        return fail(JB_ERR_INVALID, who, idx,
                    "n_taps: the direct index " + std::to_string((uint64_t)di) + " is not below n_taps " +
                        std::to_string(s.n_taps));
    t.direct = (uint32_t)di;
    const long double Rmax = c * (long double)(s.n_taps + kRoomWh) / (long double)s.hz;
    for (int a = 0; a < 3; a++)
        if (!axis_table(s.size[a], s.source[a], s.mic[a], s.beta[2 * a], s.beta[2 * a + 1], Rmax, &t.D2[a], &t.g[a]))
            return fail(JB_ERR_UNSUPPORTED, who, idx,
                        "axis " + std::to_string(a) + " has more than JB_ROOM_MAX_AXIS (1024) entries");
    if (t.visits() > kRoomMaxVisits)
        return fail(JB_ERR_UNSUPPORTED, who, idx, "entries_x entries_y n_taps is above 2^32");
    if (out)
        *out = std::move(t);
    return JB_OK;
}

void room_host_taps(const RoomTables &t, double *h)
{
    const double *F = room_lowpass().data();
    const RoomConst c{t.kappa, t.fourpi, t.d0, t.unit, t.K};
    const size_t nx = t.D2[0].size(), ny = t.D2[1].size(), nz = t.D2[2].size();
    const double *D2x = t.D2[0].data(), *D2y = t.D2[1].data(), *D2z = t.D2[2].data();
    // (the reach of the one tap: the kernel's skipping with a workgroup of one)
    for (uint32_t k = 0; k < t.K; k++) {
        double lo2, hi2, acc = 0.0;
        room_reach(k, k, t.kappa, &lo2, &hi2);
        for (size_t i = 0; i < nx && !(D2x[i] > hi2); i++)
            for (size_t j = 0; j < ny; j++) {
                const double sxy = D2x[i] + D2y[j];
                if (sxy > hi2)
                    break;
                uint32_t m0, m1;
                room_window(D2z, (uint32_t)nz, sxy, lo2, hi2, &m0, &m1);
                for (uint32_t m = m0; m < m1; m++)
                    acc = room_term(acc, D2x[i], D2y[j], D2z[m], t.g[0][i], t.g[1][j], t.g[2][m], (double)k, c, F);
            }
        h[k] = acc;
    }
}

jb_room_report room_report_of(const double *h, uint32_t K, uint32_t direct, uint32_t delay)
{
    jb_room_report o{};
    double all = 0.0, near = 0.0, rest = 0.0;
    for (uint32_t k = 0; k < K; k++) {
        all = __builtin_fma(h[k], h[k], all);
        const bool in = k + kRoomWh >= direct && k <= direct + kRoomWh;
        (in ? near : rest) = __builtin_fma(h[k], h[k], in ? near : rest);
    }
    o.energy = all;
    o.drr_db = rest == 0.0 ? (double)INFINITY : 10.0 * log10(near / rest);
    o.direct_index = direct;
    o.delay = delay;
    return o;
}

int room_vary(uint64_t seed, uint64_t k, const double size[3], double margin, double source[3], double mic[3],
              const char *who)
{
    if (!size || !source || !mic)
        return JB_ERR_INVALID;
    for (int a = 0; a < 3; a++)
        if (!(size[a] >= 0.5 && size[a] <= 1000.0)) {
            set_error(std::string(who) + ": size[" + std::to_string(a) + "] is outside [0.5, 1000] m");
            return JB_ERR_INVALID;
        }
    if (!(margin > 0.0) || !(2.0 * margin < std::min(size[0], std::min(size[1], size[2])))) {
        set_error(std::string(who) + ": margin is not above 0 with 2 margin below every edge");
        return JB_ERR_INVALID;
    }
    const uint64_t z = fmt_mix(fmt_mix(seed) ^ k);
    for (uint64_t a = 0; a < 64; a++) {
        double v[6];
        for (uint64_t j = 0; j < 6; j++) {
            const double u = (double)(fmt_mix(z + 6 * a + j + 1) >> 11) * (1.0 / 9007199254740992.0);
            const double w = u * (size[j % 3] - 2.0 * margin);
            v[j] = margin + w;
        }
        const double dx = v[0] - v[3], dy = v[1] - v[4], dz = v[2] - v[5];
        if (!(sqrt((dx * dx + dy * dy) + dz * dz) >= kRoomMinApart))
            continue;
        for (int j = 0; j < 3; j++) {
            source[j] = v[j];
            mic[j] = v[3 + j];
        }
        return JB_OK;
    }
    set_error(std::string(who) + ": no attempt put source and mic 1 cm apart");
    return JB_ERR_INVALID;
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_room_host(const jb_room *r, double *h, size_t cap)
{
    RoomTables t;
    const int rc = room_check(r, 0, "jb_room_host", &t);
    if (rc)
        return rc;
    if (!h)
        return JB_ERR_INVALID;
    if (cap < t.K) {
        set_error("jb_room_host: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    room_host_taps(t, h);
    return JB_OK;
}

int jb_room_geometry(const jb_room *r, jb_room_info *out)
{
    RoomTables t;
    const int rc = room_check(r, 0, "jb_room_geometry", &t);
    if (rc)
        return rc;
    if (!out)
        return JB_ERR_INVALID;
    *out = jb_room_info{};
    out->direct_distance = t.d0;
    out->pair_visits = t.visits();
    out->workgroups = t.workgroups();
    for (int a = 0; a < 3; a++)
        out->entries[a] = (uint32_t)t.D2[a].size();
    out->direct_index = t.direct;
    return JB_OK;
}

int jb_room_lowpass(double *F, size_t cap, uint32_t *Wh, uint32_t *Q)
{
    if (Wh)
        *Wh = kRoomWh;
    if (Q)
        *Q = kRoomQ;
    if (F) {
        if (cap < kRoomTable) {
            set_error("jb_room_lowpass: the buffer is too small");
            return JB_ERR_BUFFER;
        }
        memcpy(F, room_lowpass().data(), sizeof(double) * kRoomTable);
    }
    return JB_OK;
}

int jb_room_design(const double size[3], double rt60, double c, double beta[6])
{
    if (!size || !beta)
        return JB_ERR_INVALID;
    for (int a = 0; a < 3; a++)
        if (!(size[a] >= 0.5 && size[a] <= 1000.0)) {
            set_error("jb_room_design: size[" + std::to_string(a) + "] is outside [0.5, 1000] m");
            return JB_ERR_INVALID;
        }
    if (!(rt60 > 0.0) || !std::isfinite(rt60)) {
        set_error("jb_room_design: rt60 is not above 0 and finite");
        return JB_ERR_INVALID;
    }
    if (!(c == 0.0 || (c >= 50.0 && c <= 5000.0))) {
        set_error("jb_room_design: c is neither 0 nor in [50, 5000] m/s");
        return JB_ERR_INVALID;
    }
    const long double cs = c == 0.0 ? (long double)kRoomSound : (long double)c;
    const long double lx = size[0], ly = size[1], lz = size[2];
    const long double V = lx * ly * lz, S = 2.0L * (lx * ly + ly * lz + lx * lz);
    const long double alpha = 1.0L - expl(-(24.0L * logl(10.0L) / cs) * V / (S * (long double)rt60));
    const double b = (double)sqrtl(1.0L - alpha);
    for (int w = 0; w < 6; w++)
        beta[w] = b;
    return JB_OK;
}

int jb_room_vary(uint64_t seed, uint64_t k, const double size[3], double margin, double source[3], double mic[3])
{
    return room_vary(seed, k, size, margin, source, mic, "jb_room_vary");
}

void jb_room_free(void *p) { free(p); }

} // extern "C"

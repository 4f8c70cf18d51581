#pragma once
// jb_activity.h -- the speech-activity stage (include/jbonsai_amd.h "Speech activity"): per-frame 0/1 labels of a unit,
// one column per member of a programme (or one for the unit), on the frame grid of the feature stages.  The grid, the
// energy of a frame, the gate and the three smoothing steps are stated once here for the kernels (jb_activity.hip) and
// for the host rule (jb_activity.cpp), with the work lists' entries.  The frame grids are jb_fbank.h's frame_count /
// frame_start and jb_melspec.h's mel_frames, called and not restated; the sum of a frame is jb_fbank.h's frame_sum.
// Plain C++17; under hipcc the rules compile for the host and the device alike.
#include <math.h>

#include "jb_fbank.h"
#include "jb_melspec.h"

namespace jb {

// jb_activity_opts, jb_activity_report and jb_activity_unit_report of the public header, restated (this header stands
// without it; jb_activity.cpp asserts that the two agree)
struct ActOpts {
    uint32_t win_us, hop_us; // with kActSamples: samples
    double gate_db;
    uint32_t grid, reference, columns, flags;
    uint32_t min_speech, min_gap, hang_before, hang_after; // frames, each in 0..65535
    uint32_t reserved[4];
};
static_assert(sizeof(ActOpts) == 64 && offsetof(ActOpts, gate_db) == 8 && offsetof(ActOpts, grid) == 16 &&
                  offsetof(ActOpts, min_speech) == 32 && offsetof(ActOpts, reserved) == 48,
              "jb_activity_opts is 64 bytes");
struct ActReport {
    uint64_t active, first, last; // first == last == T where no frame is active
    double peak, thr;             // the largest energy of the column, and the threshold its frames met
};
struct ActUnitReport {
    uint64_t frames, none, one, many; // T, and the frames under 0, exactly 1, and 2 or more active columns
};

constexpr uint32_t kActSnip = 0, kActCenter = 1, kActKaldi = 2, kActStft = 3; // JB_ACTIVITY_SNIP, _CENTER, _KALDI, _STFT
constexpr uint32_t kActRefPeak = 0, kActRefAbs = 1;                          // JB_ACTIVITY_REF_PEAK, _REF_ABS
constexpr uint32_t kActMembers = 0, kActUnit = 1;                            // JB_ACTIVITY_MEMBERS, _UNIT
constexpr uint32_t kActSamples = 1;                                          // JB_ACTIVITY_SAMPLES
constexpr uint32_t kActMinWin = 2, kActMaxWin = 4096, kActMaxLen = 65535;
constexpr double kActMinGateDb = 1.0, kActMaxGateDb = 120.0;
// JB_ACTIVITY_MAX_CELLS: T * C of a unit, and the label bytes of a batch (256 members by 3.27 million frames pass)
constexpr uint64_t kActMaxCells = 1ull << 30;

// The launch shape.  A workgroup of the energy kernel stages kActLds samples and takes as many consecutive frames of
// one column as they hold, at most kActMaxFrames; the label kernel walks a column in blocks of kActBlockWords words of
// 64 frames
constexpr uint32_t kActLanes = 256, kActLds = 6144, kActMaxFrames = 32;
constexpr uint32_t kActEnergyLanes = 256; // of the energy kernel (1024 measured 1.2 to 1.4 times the time of 256)
constexpr uint32_t kActBlockWords = 64, kActBlockFrames = 64 * kActBlockWords;
constexpr uint32_t act_wg_frames(uint32_t wl, uint32_t hop)
{
    const uint64_t f = (uint64_t)(kActLds - wl) / hop + 1;
    return (uint32_t)(f < kActMaxFrames ? f : kActMaxFrames);
}

// What is wrong with the options whatever the rate, naming the field; null: nothing
inline const char *act_opts_fault(const ActOpts &o)
{
    if (o.grid > kActStft)
        return "grid is JB_ACTIVITY_SNIP, _CENTER, _KALDI or _STFT";
    if (o.reference > kActRefAbs)
        return "reference is JB_ACTIVITY_REF_PEAK or JB_ACTIVITY_REF_ABS";
    if (o.columns > kActUnit)
        return "columns is JB_ACTIVITY_MEMBERS or JB_ACTIVITY_UNIT";
    if (o.flags & ~kActSamples)
        return "flags has an unknown bit";
    if (o.reserved[0] || o.reserved[1] || o.reserved[2] || o.reserved[3])
        return "reserved must be 0";
    if (!(o.gate_db >= kActMinGateDb && o.gate_db <= kActMaxGateDb))
        return "gate_db is in [1, 120]";
    if (o.min_speech > kActMaxLen)
        return "min_speech is in 0..65535 frames";
    if (o.min_gap > kActMaxLen)
        return "min_gap is in 0..65535 frames";
    if (o.hang_before > kActMaxLen)
        return "hang_before is in 0..65535 frames";
    if (o.hang_after > kActMaxLen)
        return "hang_after is in 0..65535 frames";
    return nullptr;
}
// What is out of its limits at hz, naming the field; null: nothing, and the window and the hop are in *wl and *hop
inline const char *act_geometry_fault(const ActOpts &o, uint32_t hz, uint32_t *wl, uint32_t *hop)
{
    const bool samples = (o.flags & kActSamples) != 0;
    if (!samples && hz == 0)
        return "the rate is 0";
    const uint64_t w = samples ? o.win_us : fbank_round_us(hz, o.win_us);
    const uint64_t h = samples ? o.hop_us : fbank_round_us(hz, o.hop_us);
    if (w < kActMinWin || w > kActMaxWin)
        return "win_us gives a window of 2..4096 samples";
    if (h < 1 || h > 0xffffffffull)
        return "hop_us gives a hop of at least 1 sample";
    *wl = (uint32_t)w;
    *hop = (uint32_t)h;
    return nullptr;
}

// T of a unit of n samples, and the first sample of frame t (below 0 or behind n: outside the unit, read as 0)
constexpr uint64_t act_frames(uint32_t grid, uint64_t n, uint32_t wl, uint32_t hop)
{
    return n == 0             ? 0
           : grid == kActStft ? mel_frames(n, wl, hop, kMelPadZero, 0)
                              : frame_count(n, wl, hop, grid == kActCenter, grid == kActKaldi);
}
JB_RFFT_HD constexpr int64_t act_start(uint32_t grid, uint64_t t, uint32_t wl, uint32_t hop)
{
    return frame_start(t, wl, hop, grid == kActCenter || grid == kActStft, grid == kActKaldi);
}

// The frames of a unit of T that touch a sample of [start, start + n): [*f0, *f0 + *nf), none where n == 0.  Every
// other frame of the column has the energy +0.0
inline void act_span(uint32_t grid, uint64_t T, uint32_t wl, uint32_t hop, uint64_t start, uint64_t n, uint64_t *f0,
                     uint64_t *nf)
{
    *f0 = *nf = 0;
    if (n == 0 || T == 0)
        return;
    const int64_t off = act_start(grid, 0, wl, hop); // s_t = t hop + off
    // the first t with s_t + wl > start, and the first with s_t >= start + n
    const int64_t a = (int64_t)start - off - (int64_t)wl, b = (int64_t)(start + n) - off;
    uint64_t lo = a < 0 ? 0 : (uint64_t)a / hop + 1;
    uint64_t hi = b <= 0 ? 0 : ((uint64_t)b + hop - 1) / hop;
    lo = lo < T ? lo : T;
    hi = hi < T ? hi : T;
    if (hi > lo) {
        *f0 = lo;
        *nf = hi - lo;
    }
}

// The gate.  q = 10^(-gate_db / 10) and the absolute threshold wl 32768^2 q, each formed in long double and rounded
// once (host functions: the device reads them from its work list)
inline double act_ratio(double gate_db) { return (double)powl(10.0L, -(long double)gate_db / 10.0L); }
inline double act_abs_threshold(double gate_db, uint32_t wl)
{
    return (double)((long double)wl * 1073741824.0L * powl(10.0L, -(long double)gate_db / 10.0L));
}
// thr of a column from its largest energy, and whether a frame of energy E is raw-active
JB_RFFT_HD double act_threshold(bool ref_abs, double q, double thr_abs, double peak) { return ref_abs ? thr_abs : q * peak; }
JB_RFFT_HD bool act_raw(double E, double thr) { return E > 0.0 && E >= thr; }

// The smoothing steps on packed words (the kernel's form; the host rule walks the bytes).  Frame t is bit t & 63 of
// word t >> 6; `word` is the word of frame b + i, i < 64, b a multiple of 64.  prev / next: the nearest set bit in front
// of frame b + i and behind it; in the word where it has one, else what the scan across the words carried in (before:
// the nearest in front of the word, or -1; behind: the nearest behind it, or a value of at least T)
JB_RFFT_HD int64_t act_prev(uint64_t word, uint32_t i, int64_t b, int64_t before)
{
    const uint64_t m = i ? word & (~0ull >> (64 - i)) : 0;
    return m ? b + 63 - (int64_t)__builtin_clzll(m) : before;
}
JB_RFFT_HD int64_t act_next(uint64_t word, uint32_t i, int64_t b, int64_t behind)
{
    const uint64_t m = i < 63 ? word >> (i + 1) : 0;
    return m ? b + i + 1 + (int64_t)__builtin_ctzll(m) : behind;
}
// Close: a clear frame between raw-active frames a < t < c, the nearest ones, with c - a - 1 <= min_gap is set
JB_RFFT_HD uint64_t act_close_word(uint64_t word, int64_t b, int64_t before, int64_t behind, int64_t T, uint32_t min_gap)
{
    uint64_t out = word;
    for (uint32_t i = 0; i < 64; i++) {
        if ((word >> i) & 1)
            continue;
        const int64_t a = act_prev(word, i, b, before), c = act_next(word, i, b, behind);
        if (a >= 0 && c < T && c - a - 1 <= (int64_t)min_gap)
            out |= 1ull << i;
    }
    return out;
}
// Open: a set frame in a run shorter than min_speech is cleared.  clear_word is the complement of the frames' word
// (frames at T and behind read as clear); before / behind were carried over the complements
JB_RFFT_HD uint64_t act_open_word(uint64_t clear_word, int64_t b, int64_t before, int64_t behind, int64_t T,
                                  uint32_t min_speech)
{
    uint64_t out = ~clear_word;
    for (uint32_t i = 0; i < 64; i++) {
        if ((clear_word >> i) & 1)
            continue;
        const int64_t a = act_prev(clear_word, i, b, before);
        int64_t c = act_next(clear_word, i, b, behind);
        c = c < T ? c : T;
        if (c - a - 1 < (int64_t)min_speech)
            out &= ~(1ull << i);
    }
    return out;
}
// Hang: frame t is set iff a set frame s has s - hang_before <= t <= s + hang_after
JB_RFFT_HD uint64_t act_hang_word(uint64_t word, int64_t b, int64_t before, int64_t behind, int64_t T,
                                  uint32_t hang_before, uint32_t hang_after)
{
    uint64_t out = word;
    for (uint32_t i = 0; i < 64 && b + i < T; i++) {
        if ((word >> i) & 1)
            continue;
        const int64_t t = b + i, a = act_prev(word, i, b, before), c = act_next(word, i, b, behind);
        if ((a >= 0 && t - a <= (int64_t)hang_after) || (c < T && c - t <= (int64_t)hang_before))
            out |= 1ull << i;
    }
    return out;
}

// One column of a launch.  Launch lists are in unit order, a unit's columns in column order; g0 is the prefix sum of
// the list's energy workgroups (act_wg_frames frames each; workgroups never cross columns).  slot and unit number the
// column and its unit in the full run's lists: the reports' places, which a redo keeps
struct ActCol {
    const void *x;     // the source's first sample: f64 or 16-bit (by the launch); not read where n == 0
    uint8_t *y;        // the column's first byte: the unit's [T][C] matrix + its column
    double *e;         // its compact energies: frame f0 + i at e[i], i < nf
    uint64_t *words;   // three runs of `nw` words of scratch (only with a smoothing step; else null)
    uint64_t start, n; // the source's place within the unit (n == 0: a muted or empty member, a column of zeros)
    uint64_t T, f0, nf, g0;
    uint64_t nw;       // ceil(T / 64)
    double q, thr_abs;
    uint32_t C, wl, hop;
    uint32_t col, slot, unit; // its place in the unit's row, its report's and its unit's report's
};

// One unit of a launch: its matrix, the prefix sum of the counting kernel's workgroups (kActLanes frames each) and its
// report's place
struct ActUnit {
    const uint8_t *y;
    uint64_t T, g0;
    uint32_t C, unit;
};
constexpr uint64_t act_energy_wgs(uint64_t nf, uint32_t wl, uint32_t hop)
{
    return (nf + act_wg_frames(wl, hop) - 1) / act_wg_frames(wl, hop);
}
constexpr uint64_t act_unit_wgs(uint64_t T) { return (T + kActLanes - 1) / kActLanes; }

// The request laid out over the units of a batch or a call.  Unit p owns cols[units[p].col0 .. + C); with kActMembers a
// column per member in ascending utterance index, with kActUnit one column that spans the unit.  The label slab holds
// every unit's [T][C] bytes from a 16-byte boundary; the energy scratch holds per column only the frames that touch its
// source, so it grows with the members' samples and not with T * C; the word scratch (with a smoothing step) holds
// three runs of ceil(T / 64) words per column
struct ActLayUnit {
    uint64_t off, T; // its first byte in the label slab, and its frames
    uint32_t C, wl, hop, col0;
};
struct ActLayCol {
    uint64_t start, n;   // the source's place within the unit; n == 0: a column of zeros
    uint64_t f0, nf, e0; // the frames that touch it, and the first one's place in the energy scratch
    uint64_t w0;         // its first word in the word scratch
    uint32_t unit, utt;  // utt: the member's utterance index (kActUnit: the unit's first member)
};
struct ActLayout {
    std::vector<ActLayUnit> units;
    std::vector<ActLayCol> cols;
    uint64_t bytes = 0, energies = 0, words = 0;
};
// Pure.  unit_n, unit_hz: [P] each unit's samples and rate; unit p's members are members[first[p] .. first[p + 1]) with
// start[u], n[u] and gain[u] (0: muted) by utterance index.  null: laid out into *out; else what is refused, naming the
// field, *unit the offending unit and *unsupported whether a cap was passed (JB_ERR_UNSUPPORTED) or a limit
inline const char *act_layout(const ActOpts &o, size_t P, const uint64_t *unit_n, const uint32_t *unit_hz,
                              const uint32_t *first, const uint32_t *members, const uint64_t *start, const uint64_t *n,
                              const double *gain, ActLayout *out, size_t *unit, bool *unsupported)
{
    *unsupported = false;
    *unit = 0;
    if (const char *f = act_opts_fault(o))
        return f;
    const bool smooth = o.min_gap || o.min_speech > 1 || o.hang_before || o.hang_after;
    ActLayout L;
    L.units.resize(P);
    for (size_t p = 0; p < P; p++) {
        *unit = p;
        ActLayUnit &U = L.units[p];
        if (const char *f = act_geometry_fault(o, unit_hz ? unit_hz[p] : 0, &U.wl, &U.hop))
            return f;
        U.T = act_frames(o.grid, unit_n[p], U.wl, U.hop);
        U.C = o.columns == kActUnit ? 1 : first[p + 1] - first[p];
        U.col0 = (uint32_t)L.cols.size();
        U.off = L.bytes;
        *unsupported = true;
        if (U.C && U.T > kActMaxCells / U.C)
            return "T * C of a unit passes JB_ACTIVITY_MAX_CELLS (take JB_ACTIVITY_UNIT)";
        L.bytes += (U.T * U.C + 15) & ~15ull;
        if (L.bytes > kActMaxCells)
            return "the label bytes of the units together pass JB_ACTIVITY_MAX_CELLS";
        *unsupported = false;
        for (uint32_t j = 0; j < U.C; j++) {
            ActLayCol c{};
            c.unit = (uint32_t)p;
            c.utt = members[first[p] + j];
            if (o.columns == kActUnit) {
                c.start = 0;
                c.n = unit_n[p];
            } else {
                c.start = start[c.utt];
                c.n = gain[c.utt] == 0.0 ? 0 : n[c.utt];
            }
            act_span(o.grid, U.T, U.wl, U.hop, c.start, c.n, &c.f0, &c.nf);
            c.e0 = L.energies;
            L.energies += c.nf;
            c.w0 = L.words;
            if (smooth)
                L.words += 3 * ((U.T + 63) / 64);
            L.cols.push_back(c);
        }
    }
    *out = std::move(L);
    return nullptr;
}

// The request's share of every launch
struct ActLaunch {
    uint32_t grid, ref_abs;
    uint32_t min_speech, min_gap, hang_before, hang_after;
    JB_RFFT_HD bool smooth() const { return min_gap || min_speech > 1 || hang_before || hang_after; }
};

} // namespace jb

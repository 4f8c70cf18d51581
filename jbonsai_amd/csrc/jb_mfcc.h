#pragma once
// jb_mfcc.h -- cepstral features (include/jbonsai_amd.h "Cepstral features"): the option check, the widths, the order
// of every sum (the cepstrum of a frame, the statistics of a unit, the delta rows), stated once for the kernels
// (jb_mfcc.hip), for the host half (jb_mfcc.cpp) and for whoever plans the stage's memory, and the stage's work list.
// Plain C++17; under hipcc the rules compile for the host and the device alike.
#include "jb_fbank.h"

namespace jb {

// jb_mfcc_opts of the public header, restated (this header stands without it; jb_mfcc.cpp asserts the two agree)
struct MfccOpts {
    uint32_t n_ceps, delta_order, delta_window, cmvn;
    double lifter, var_floor;
    uint32_t flags;
    uint32_t reserved[3];
};
static_assert(sizeof(MfccOpts) == 48 && offsetof(MfccOpts, lifter) == 16 && offsetof(MfccOpts, flags) == 32 &&
                  offsetof(MfccOpts, reserved) == 36,
              "jb_mfcc_opts is 48 bytes");

constexpr uint32_t kMfCmvnNone = 0, kMfCmvnMean = 1, kMfCmvnMeanVar = 2; // JB_CMVN_NONE, _MEAN, _MEAN_VAR
constexpr uint32_t kMfF64 = 1;                                            // JB_MFCC_F64
constexpr uint32_t kMfMaxOrder = 2, kMfMaxWindow = 5;
constexpr uint32_t kMfMaxS1 = 2 * kMfMaxWindow + 1, kMfMaxS2 = 4 * kMfMaxWindow + 1; // the longest s_1 and s_2
constexpr uint32_t kMfBlock = 64;  // frames of one block sum of the statistics
constexpr uint32_t kMfLanes = 256; // threads of a workgroup
constexpr uint32_t kMfTile = 32;   // frames a workgroup of k_ceps and of k_delta takes
constexpr uint32_t kMfCols = 64;   // columns of the statics a workgroup of k_delta takes

// What is wrong with the options, naming the field; null: nothing.  n_mels: of the filterbank they stand behind
inline const char *mfcc_opts_fault(const MfccOpts &o, uint32_t n_mels)
{
    if (o.n_ceps > n_mels)
        return "n_ceps is at most n_mels (0: the log-mel energies themselves)";
    if (o.delta_order > kMfMaxOrder)
        return "delta_order is in 0..2";
    if (o.delta_window < 1 || o.delta_window > kMfMaxWindow)
        return "delta_window is in 1..5";
    if (o.cmvn > kMfCmvnMeanVar)
        return "cmvn is JB_CMVN_NONE, JB_CMVN_MEAN or JB_CMVN_MEAN_VAR";
    if (!(o.lifter >= 0.0) || !std::isfinite(o.lifter))
        return "lifter is 0 (none) or a positive number";
    if (!(o.var_floor >= 0.0) || !std::isfinite(o.var_floor))
        return "var_floor is a positive number, or 0 for 2^-52";
    if (o.flags & ~kMfF64)
        return "flags has an unknown bit";
    if (o.reserved[0] || o.reserved[1] || o.reserved[2])
        return "reserved must be 0";
    return nullptr;
}
// What the stage refuses in the filterbank options it stands behind (it makes the f64 logarithms itself)
inline const char *mfcc_fbank_fault(const FbankOpts &f)
{
    if (f.flags & (kFbLinear | kFbF64))
        return "the filterbank's flags must not hold JB_FBANK_LINEAR or JB_FBANK_F64 (the stage reads f64 logarithms)";
    return nullptr;
}
// The filterbank options as the stage runs them: f64 logarithms
inline FbankOpts mfcc_fbank_opts(FbankOpts f)
{
    f.flags = (f.flags & ~kFbLinear) | kFbF64;
    return f;
}

constexpr uint32_t mfcc_static_width(uint32_t n_ceps, uint32_t n_mels) { return n_ceps ? n_ceps : n_mels; }
constexpr uint32_t mfcc_width(const MfccOpts &o, uint32_t n_mels)
{
    return mfcc_static_width(o.n_ceps, n_mels) * (o.delta_order + 1);
}
constexpr uint64_t mfcc_elem(uint32_t flags) { return (flags & kMfF64) ? 8 : 4; }
constexpr uint64_t mfcc_blocks(uint64_t T) { return (T + kMfBlock - 1) / kMfBlock; }
constexpr uint64_t mfcc_tiles(uint64_t T) { return (T + kMfTile - 1) / kMfTile; }

// JB_OK, or JB_ERR_INVALID with set_error naming the field (jb_mfcc.cpp)
int mfcc_check_opts(const MfccOpts *opts, uint32_t n_mels, const char *who);
int mfcc_check_fbank(const FbankOpts *fopts, const char *who);

// The tables of one (n_mels, options) pair, built in long double and rounded once (jb_mfcc.cpp)
struct MfccTables {
    std::vector<double> D;      // [n_ceps][n_mels] the orthonormal DCT-II (empty with n_ceps = 0)
    std::vector<double> Dt;     // [n_mels][n_ceps] the same, transposed: what the kernel reads
    std::vector<double> lift;   // [n_ceps]
    double s1[kMfMaxS1] = {};   // s_1[-N..N]
    double s2[kMfMaxS2] = {};   // s_2[-2N..2N]
};
void mfcc_dct(uint32_t n_mels, uint32_t n_ceps, double lifter, double *D, double *lift);
void mfcc_delta_kernel(uint32_t q, uint32_t N, double *s); // s_q[-qN..qN], 2 q N + 1 values
void mfcc_tables(const MfccOpts &o, uint32_t n_mels, MfccTables *t);
inline double mfcc_r(uint64_t T) { return T ? (double)(1.0L / (long double)T) : 0.0; } // r_T

// What every kernel of a launch is told (by value)
struct MfccParams {
    const double *Dt, *lift; // device tables (null with n_ceps = 0)
    uint32_t n_mels, n_ceps, d, order, N, cmvn, flags, pad;
    double floor; // var_floor, or 2^-52
    double s1[kMfMaxS1], s2[kMfMaxS2];
    double e_floor, e_ln_floor; // the filterbank's log_floor and its logarithm: what c0 of JB_FRAME_ENERGY is held to
};
inline MfccParams mfcc_params(const MfccOpts &o, uint32_t n_mels, const MfccTables &t)
{
    MfccParams p{};
    p.n_mels = n_mels;
    p.n_ceps = o.n_ceps;
    p.d = mfcc_static_width(o.n_ceps, n_mels);
    p.order = o.delta_order;
    p.N = o.delta_window;
    p.cmvn = o.cmvn;
    p.flags = o.flags;
    p.floor = o.var_floor == 0.0 ? 0x1p-52 : o.var_floor;
    for (uint32_t i = 0; i < kMfMaxS1; i++)
        p.s1[i] = t.s1[i];
    for (uint32_t i = 0; i < kMfMaxS2; i++)
        p.s2[i] = t.s2[i];
    return p;
}

// One unit of a launch.  Launch lists are in unit order; g0 is the prefix sum of the list's frame tiles (kMfTile frames
// each; workgroups never cross units), b0 that of its blocks of kMfBlock frames
struct MfccUtt {
    const double *L; // [T][n_mels] the f64 log-mel frames
    double *c;       // [T][d] the f64 statics (n_ceps = 0: L itself, never written)
    double *bs;      // [blocks][d] the block sums of the statistics' pass at hand
    double *stat;    // [2][d]: mu, then sqrt(max(var, floor))
    uint8_t *y;      // [T][d (order + 1)] elements, 16-byte aligned
    uint64_t T, g0, b0;
    double r_T;
    const double *e; // [T] the frames' energies (JB_FRAME_ENERGY: c[t][0] is their logarithm); null: none
};

// ---- the rule, operation for operation (every product and sum on its own: the build has -ffp-contract=off) ----

// c[t][i]: the cepstrum i of one frame.  Lrow: the frame's n_mels logarithms; Dcol: D[i][0], stride ds to D[i][1]
JB_RFFT_HD double mfcc_cep(const double *Lrow, const double *Dcol, uint32_t ds, uint32_t n_mels, double lift)
{
    double acc = 0.0;
    for (uint32_t m = 0; m < n_mels; m++)
        acc = acc + Dcol[(size_t)m * ds] * Lrow[m];
    return lift * acc;
}
// c[t][0] under JB_FRAME_ENERGY: ln(max(e, log_floor)), the floor's logarithm from the host; the lifter's l_0 is 1
JB_RFFT_HD double mfcc_c0(double e, double floor, double ln_floor) { return e > floor ? log(e) : ln_floor; }
// One value of the statistics' passes: c (the mean's pass), or (c - mu)^2 (the variance's)
JB_RFFT_HD double mfcc_stat_term(double c, double mu, bool var)
{
    const double dv = c - mu;
    return var ? dv * dv : c;
}
// The normalised static
JB_RFFT_HD double mfcc_norm(double c, double mu, double sd, uint32_t cmvn)
{
    return cmvn == kMfCmvnNone ? c : cmvn == kMfCmvnMean ? c - mu : (c - mu) / sd;
}
JB_RFFT_HD double mfcc_sd(double var, double floor) { return sqrt(var > floor ? var : floor); }
// out_q of one element: v(j) is c'[clamp(t + j)][i] for j in -qN..qN; s: s_q[-qN..qN]
template <class V> JB_RFFT_HD double mfcc_delta(const double *s, int32_t qN, V v)
{
    double acc = 0.0;
    for (int32_t j = -qN; j <= qN; j++)
        acc = acc + s[j + qN] * v(j);
    return acc;
}

} // namespace jb

// jb_host.h -- host-side internals shared by the C-ABI translation units.
#pragma once
#include "../../include/jbonsai_amd.h"
#include "jb_device.h"
#include "jb_activity.h"
#include "jb_adpcm.h"
#include "jb_fbank.h"
#include "jb_filter.h"
#include "jb_fir.h"
#include "jb_format.h"
#include "jb_limiter.h"
#include "jb_loudness_rules.h"
#include "jb_md5.h"
#include "jb_melspec.h"
#include "jb_mfcc.h"
#include "jb_noise.h"
#include "jb_output.h"
#include "jb_pcm_call.h"
#include "jb_pitch.h"
#include "jb_room.h"

#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace jb {

extern thread_local std::string g_err;
void set_error(const std::string &s);
int hip_fail(hipError_t e, const char *what);
// JB_BATCH_INVARIANT fixes the geometry itself: with an explicit chunk_frames / warmup_frames or a forced vocoder
// kernel, JB_ERR_INVALID (set_error names the conflict); touches no device
int check_invariant_opts(const jb_batch_opts *opts);
// Device copy of the shared Gaussian noise stream; a Batch keeps the table it was created with alive
struct NoiseDev {
    int device = -1;
    double *ptr = nullptr;
    size_t len = 0;
    ~NoiseDev();
};
int noise_table(int device, size_t need, std::shared_ptr<NoiseDev> *out);
void release_cached_memory(); // empties the per-device pools of finished batches' memory
void set_cached_memory_limit(size_t bytes); // cap of a device's pool (JB_DEVICE_POOL_MB at start)
// What an engine-level call hands out per utterance (or per programme): PCM, or the bytes of one of the encoders
enum class SynthSink { Pcm, Flac, Formatted, Adpcm, Fbank, Mfcc, Melspec, Pitch };
struct ByteSpan { // an output's place in the host copy of a byte sink's slab (OutputChain::read_bytes_all)
    uint64_t off, bytes;
};
// One engine request on one device: what the jb_synthesize* entries (jb_engine.cpp, jb_multi.cpp) ask of
// synthesize_batch_impl.  Exactly one sink; the options of the others stay null
struct SynthRequest {
    const jb_engine *e = nullptr;            // the engine; with `each`, each[0]: what the engines share
    const jb_engine *const *each = nullptr;  // jb_synthesize_batch_each*: utterance u under each[u]'s Condition (the
                                             // engines checked by the caller); null: e for all
    const char *const *lines = nullptr;      // utterance u is lines[line_off[u] .. line_off[u + 1])
    const size_t *line_off = nullptr;
    size_t n_utts = 0;
    int32_t device = -1;
    unsigned host_threads = 0;               // 0: the default front-half thread count
    SynthSink sink = SynthSink::Pcm;
    bool i16 = false;                        // the batch's PCM in 16 bits (Pcm: what is handed out; Flac and Adpcm
                                             // encode it) or in f64 (Formatted, Fbank, Mfcc and Melspec read f64)
    const jb_flac_opts *flac = nullptr;      // Flac: both may be null (the defaults; no MD5 / SEEKTABLE request)
    const jb_flac_meta *flac_meta = nullptr;
    const jb_format_opts *fmt = nullptr;     // Formatted
    const jb_adpcm_opts *adpcm = nullptr;    // Adpcm
    const jb_fbank_opts *fbank = nullptr;    // Fbank
    const jb_mfcc_opts *mfcc = nullptr;      // Mfcc: behind the filterbank options of `fbank`
    const jb_melspec_opts *melspec = nullptr; // Melspec
    const jb_pitch_opts *pitch = nullptr;     // Pitch
    size_t *counts = nullptr;                // counts[u] (may be null), by the sink: the samples output u's blocks
                                             // encode (Adpcm), or its frames (Fbank, Mfcc, Melspec)
    const jb_join_opts *join = nullptr;      // jb_synthesize_programme*: all utterances are one programme, the one
    uint64_t *join_starts = nullptr;         // output; join_starts[u] (may be null): each member's first sample
    const jb_activity_opts *activity = nullptr; // beside a Pcm sink with a join: the programme's speech-activity labels
    uint8_t **act_out = nullptr;             // into act_out[0] (malloc'ed), their frames and columns into act_T[0]
    uint64_t *act_T = nullptr;               // and act_C[0]
    uint32_t *act_C = nullptr;
    const uint32_t *stem_of = nullptr;       // jb_synthesize_programme_stems*: [n_utts] the stems request behind the
    uint32_t stem_flags = 0;                 // engine's mix (JB_MIX_STEM_LEVELS); the outputs are then the mixture and
    size_t *n_outputs = nullptr;             // the S stems behind it, *n_outputs = 1 + S, and stem_reports[0 .. S)
    jb_stem_report *stem_reports = nullptr;  // ([n_utts], may be null) each stem's report
    void **out = nullptr;                    // [n_utts], or [1] with a join ([1 + n_utts] with stems): malloc'ed PCM or
                                             // bytes of each output
    size_t *n_out = nullptr;                 // its samples (Pcm) or bytes
};
int synthesize_batch_impl(const SynthRequest &rq);
// A stream / a device block from the per-device pools that batches draw from (jb_batch.cpp), for work outside a
// batch; *got is the block's pooled size, which pooled_block_free takes back
hipError_t pooled_stream_acquire(int device, hipStream_t *st);
void pooled_stream_release(int device, hipStream_t st);
hipError_t pooled_block_alloc(int device, size_t bytes, void **out, size_t *got);
void pooled_block_free(int device, void *p, size_t got);
// Decision-tree search of the front half on the device (jb_treesearch.hip): labels are slab[off[i] .. off[i + 1]),
// each at most kTsMaxLabel bytes; outputs as ts_walk_label's, [n_labels][entries] and [n_labels] (tree_pos may be
// null: a tree's position does not depend on the label)
struct TsDev;
uint32_t tree_search_memo_words(size_t n_questions); // TsDev::memo_words for that many questions (0: no memo fits)
hipError_t launch_tree_search(const TsDev &d, const uint8_t *slab, const uint32_t *off, uint32_t n_labels,
                              int32_t *tree_pos, int32_t *pdf_index, uint8_t *gv_on, hipStream_t stream);
// static LPT partition (jb_multi.cpp): part_of[i] = bin of item i
void lpt_partition(const uint64_t *weights, size_t n, size_t n_parts, uint32_t *part_of);

// Output-rate conversion (jb_resample.hip): the polyphase filter of one (in_hz, out_hz) pair
constexpr uint64_t kResampleMaxLM = 2048;
struct ResampleSpec {
    uint32_t L, M, C, ntaps;
};
// in_hz -> out_hz reduced to L/M; taps ([L][ntaps], may be null) by the definition in jb_resample.hip.
// JB_ERR_UNSUPPORTED (set_error says why) for L or M above 2048
int resample_design(uint32_t in_hz, uint32_t out_hz, ResampleSpec *spec, std::vector<double> *taps);
// A pair's device table and its launch geometry, built once per (device, in_hz, out_hz) and kept for the process;
// in_hz == out_hz gives the identity (one tap 1.0: a copy, or the 16-bit conversion alone)
struct ResampleTable {
    const double *h;    // [L][ntaps] device
    uint32_t L, M, C, ntaps;
    uint32_t rows;      // output rows (of L outputs each) per tile
    uint32_t row_waves; // waves a tile's rows are spread over (1, 2, 4); the others split the phases
    uint32_t lds;       // 1: the tile's input window is staged in LDS; 0: read from global memory
    uint32_t pad;       // > 0: the LDS window carries one pad double per 2^pad (bank spread for even M)
    uint32_t lds_bytes; // LDS of a full tile's window (0 without LDS): a launch allocates its tables' largest
    uint32_t identity;  // 1: in == out, a copy; a tile is `rows` outputs (L = 1)
};
// One workgroup's work: rows [m0, m0 + rows) of one utterance (tiles never cross utterances)
struct ResampleTile {
    const double *x; // the utterance's input (f64)
    void *y;         // its output (f64 or i16, by the launch)
    uint64_t n_in, n_out;
    uint64_t m0;
    uint32_t rows;
    uint32_t table;  // index into the launch's table list
};
// The path of a pair, by (L, M, ntaps) alone -- no device is touched (jb_resample_geometry hands it out): the fields of
// ResampleTable of the same names, and the two figures they follow from
struct ResampleGeom {
    uint32_t L, M, C, ntaps;
    uint32_t cap;       // LDS slots left for a window's samples once the pad doubles of shift `pad` are set aside
    uint32_t fit;       // rows whose window (rows M + ntaps samples) fits cap; 0: the global-memory path
    uint32_t rows, row_waves, lds, pad, lds_bytes, identity;
};
// taps (may be null): the pair's table, [L][ntaps], or the identity's one tap 1.0
int resample_geometry(uint32_t in_hz, uint32_t out_hz, ResampleGeom *out, std::vector<double> *taps);
int resample_table(int device, uint32_t in_hz, uint32_t out_hz, ResampleTable *out);
void resample_tiles(const ResampleTable &t, uint32_t table, const double *x, uint64_t n_in, void *y, uint64_t n_out,
                    std::vector<ResampleTile> &tiles);
// lds_bytes: the largest lds_bytes of the launch's tables
hipError_t launch_resample(const ResampleTable *tables_dev, const ResampleTile *tiles_dev, uint32_t n_tiles, bool i16,
                           size_t lds_bytes, hipStream_t stream);

// Loudness normalization (jb_loudness.hip): BS.1770-4 K-weighting, measured per utterance in tiles of at most
// 256 segments of S samples; tiles never cross a hop (H samples), a hop has tph of them
// (kLnLanes, the threads of a loudness workgroup: jb_loudness_rules.h)
constexpr uint32_t kTpMaxF = 64, kTpTaps = 12; // true peak: oversampling factor at most, taps per phase
struct LoudnessRate {
    double b[6], a[6];     // stage 1 (shelf) then stage 2 (high-pass): b0 b1 b2 / 1 a1 a2
    double P[8][16];       // A^(S 2^k), k = 0..7: the state transition over 2^k segments (4x4, row-major)
    double Pt[16], Pr[16]; // A^G (a hop's tiles but its last), A^(H - (tph - 1) G) (a hop's last tile)
    double Ph[16];         // A^H (a hop).  A is in the coordinates states are carried in (jb_loudness.hip ln_to_scan)
    uint32_t hz, H, S, G, tph;
    uint32_t F;                                  // true-peak oversampling factor, 1..64 (true_peak_table)
    double tp[(kTpMaxF - 1) * kTpTaps];          // its phases 1..F-1, [F - 1][12]
};
// One utterance of a loudness launch.  Launch lists are in utterance order; lt0 / at0 are prefix sums over the
// list (measure tiles / apply tiles), tile0 the utterance's place in the per-tile scratch (fixed per batch)
struct LoudnessUtt {
    const double *x; // f64 PCM measured
    void *y;         // output (f64 or i16, by the launch); null: measure only
    uint64_t n, tile0, lt0, at0;
    uint32_t ntiles, rate, slot;
    uint32_t mode; // JB_PEAK_SAMPLE / JB_PEAK_TRUE: what the ceiling bounds
    double target, ceiling;
};
struct LoudnessResult {
    double lufs, peak_dbfs, gain_db, g;
    double true_peak_dbtp; // NaN in sample mode
};
constexpr uint32_t kLnApplyTile = 8192; // samples per workgroup of the apply pass
// K-weighting coefficients and the hop of `hz`; JB_ERR_INVALID for hz == 0
int loudness_filter(uint32_t hz, double b[6], double a[6], uint32_t *hop);
// The true-peak interpolator of `hz` (pure): *F = min(64, ceil(192000 / hz)) and, when taps is not null, the
// [F - 1][12] taps of phases 1..F-1 (room for (kTpMaxF - 1) * kTpTaps always suffices); JB_ERR_INVALID for hz == 0
int true_peak_table(uint32_t hz, uint32_t *F, double *taps);
// The device table of one rate (host-built); JB_ERR_UNSUPPORTED where the tiling does not reach (H == 0, H > 61439)
int loudness_rate(uint32_t hz, LoudnessRate *out);
// Whether a loudness value (L, the momentary and short-term maxima, LRA) is defined at `hz`: JB_ERR_UNSUPPORTED at
// 3363 Hz and below, where the shelf's centre is not below Nyquist and the K-weighting diverges.  Asked wherever such
// a value is produced; the true peak reads no hop energy and is measured at any rate the tiling reaches
int loudness_measurable(uint32_t hz);
uint32_t loudness_tiles(const LoudnessRate &r, uint64_t n); // measure tiles of an utterance of n samples
// measure: utts_dev[0..n) of total tiles; st: 4 doubles per tile, pk / tp / z: one; res[slot] of each utterance.
// true_peak: some utterance of the list is in JB_PEAK_TRUE mode (without one the oversampled pass is not launched)
hipError_t launch_loudness_measure(const LoudnessRate *rates_dev, const LoudnessUtt *utts_dev, uint32_t n,
                                   uint64_t tiles, double *st, double *pk, double *tp, double *z, LoudnessResult *res,
                                   bool true_peak, hipStream_t stream);
// y = x * res[slot].g for every utterance of the list (apply tiles in all)
hipError_t launch_loudness_apply(const LoudnessUtt *utts_dev, uint32_t n, uint64_t atiles, const LoudnessResult *res,
                                 bool i16, hipStream_t stream);
// Loudness groups and the R128 report (jb_output.h: LnGroups; the rules: jb_loudness_rules.h).  A set is what one
// workgroup walks: the members of a group, or one utterance; members[m0 .. m0 + nm) index the batch's utterance list
struct LoudnessSet {
    uint32_t m0, nm;
    uint32_t slot;  // its place in the group results (a group) or the utterance's slot (an utterance)
    uint32_t rslot; // its place in the R128 results
};
struct LoudnessGroupResult {
    double lufs, peak_dbfs, true_peak_dbtp, gain_db, g;
};
using LoudnessRange = LnRangeOut;
// k_ln_gate_group behind the measure passes: sets_dev[0..n) are groups; utts_all is the batch's list by utterance
// index (its res entries hold what k_ln_gate left); gres[slot] gets the group's result and every member's gain_db and
// g in res are overwritten with the group's
hipError_t launch_loudness_groups(const LoudnessRate *rates_dev, const LoudnessUtt *utts_all, const LoudnessSet *sets_dev,
                                  uint32_t n, const uint32_t *members, const double *z, LoudnessResult *res,
                                  LoudnessGroupResult *gres, hipStream_t stream);
// The R128 report: k_ln_windows over utts_dev[0..n_utts) (each utterance's short-term windows into sw, at its tile0,
// and its largest momentary loudness into mm[slot]), then k_ln_range over sets_dev[0..n_sets) into r128[rslot]
hipError_t launch_loudness_range(const LoudnessRate *rates_dev, const LoudnessUtt *utts_dev, uint32_t n_utts,
                                 const LoudnessUtt *utts_all, const LoudnessSet *sets_dev, uint32_t n_sets,
                                 const uint32_t *members, const double *z, double *sw, double *mm,
                                 LoudnessRange *r128, hipStream_t stream);
// the public structs of a result
inline void loudness_r128_out(const LoudnessRange &r, jb_loudness_r128 *out)
{
    out->max_momentary_lufs = r.max_momentary;
    out->max_short_term_lufs = r.max_short_term;
    out->lra_lu = r.lra;
    out->lra_low_lufs = r.lra_low;
    out->lra_high_lufs = r.lra_high;
    out->n_windows = r.n;
}
// oversampling: the factor of the group's rate in true-peak mode (0: not known); range: null without a report
inline void loudness_group_report(const LoudnessGroupResult &g, uint32_t mode, uint32_t oversampling, uint32_t members,
                                  const LoudnessRange *range, jb_loudness_group_report *out)
{
    *out = jb_loudness_group_report{};
    out->lufs = g.lufs;
    out->sample_peak_dbfs = g.peak_dbfs;
    out->true_peak_dbtp = g.true_peak_dbtp;
    out->gain_db = g.gain_db;
    out->peak_mode = mode;
    out->oversampling = mode == JB_PEAK_TRUE ? oversampling : 1;
    out->members = members;
    if (range) {
        out->flags = JB_LOUDNESS_R128;
        loudness_r128_out(*range, &out->r128);
    }
}
// The host statement of the same rules (jb_loudness.cpp; no GPU): z[m][0..nh[m]) the hop energies of member m, peak /
// true_peak (null: sample mode) their largest magnitudes in 16-bit units; *group the set's result, *range its R128
// fields, member_range (null or [n]) each member's own
void loudness_gate_host(const double *const *z, const size_t *nh, size_t n, uint32_t hop, const double *peak,
                        const double *true_peak, double target, double ceiling, LoudnessGroupResult *group,
                        LoudnessRange *range, LoudnessRange *member_range);

// FLAC encoding of the 16-bit output (jb_flac.hip; the host half: jb_flac.cpp).  One stream per utterance: its header
// (42 bytes: fLaC + STREAMINFO; with a SEEKTABLE request that block behind it, jb_md5.h), then frames of
// block_size samples (the last may be shorter), each encoded into its block's slot (the VERBATIM bound apart), then
// packed at byte offsets into one compact slab, utterance after utterance
constexpr uint32_t kFlacMaxBlock = 4608, kFlacMaxLpc = 12, kFlacDefaultBlock = 4096, kFlacDefaultLpc = 8;
struct FlacParams {
    uint32_t block_size, max_order, slot_bytes, pad_;
};
struct FlacUtt {
    const int16_t *x; // the utterance's 16-bit PCM
    uint8_t *slots;   // frame f at slots + f * slot_bytes
    uint64_t n, frame0; // samples; first frame's index in the per-frame arrays
    uint32_t nframes, hz, rate_code, rate_bits, rate_val;
    uint32_t header_bytes;        // bytes in front of the first frame: 42, or 46 + 18 n_points
    uint32_t seek_step, n_points; // SEEKTABLE: frames between two points, points (0: no table)
};
struct FlacWork { // one block of an encode launch (a pack launch: every frame of the batch, in order)
    uint32_t utt, frame;
};
struct FlacOut { // per utterance: the stream's size and offset in the compact slab, min / max frame size
    uint64_t bytes, off;
    uint32_t min_frame, max_frame;
};
// opts (NULL: defaults) -> p; JB_ERR_INVALID (set_error says why) for values outside the contract
int flac_check_opts(const jb_flac_opts *opts, FlacParams *p);
// meta (NULL: no request) -> m; JB_ERR_INVALID for unknown flag bits or non-zero reserved words
int flac_check_meta(const jb_flac_meta *meta, FlacMeta *m);
uint32_t flac_slot_bytes(uint32_t block_size);
// The frame-header rate code of hz (and its 8- or 16-bit extra field); JB_ERR_UNSUPPORTED where none exists
int flac_rate_code(uint32_t hz, uint32_t *code, uint32_t *bits, uint32_t *val);
// The lists of a batch of n_utts streams; slots are offsets (total *slot_bytes) until flac_bind adds the slab's
// base; *out_bound bounds the compact slab; meta fills each utterance's seek step, points and header bytes
int flac_plan(const FlacParams &p, const FlacMeta &meta, const int16_t *const *x, const uint64_t *n,
              const uint32_t *hz, size_t n_utts, std::vector<FlacUtt> *utts, std::vector<FlacWork> *work,
              uint64_t *slot_bytes, uint64_t *out_bound);
void flac_bind(std::vector<FlacUtt> *utts, uint8_t *slots);
// The MD5 launch list of the utterances `only` marks (null: all): their indices, longest first, so that the 64
// lanes of a wave walk chains of similar length
void flac_md5_order(const std::vector<FlacUtt> &utts, const std::vector<uint8_t> *only, std::vector<uint32_t> *order);
hipError_t launch_flac_encode(const FlacParams &p, const FlacUtt *utts, const FlacWork *work, uint32_t n_work,
                              uint32_t *fsize, hipStream_t stream);
// digests[4 u ..] = MD5 of utterance u = order[i]'s samples, one lane per utterance
hipError_t launch_flac_md5(const FlacUtt *utts, const uint32_t *order, uint32_t n_order, uint32_t *digests,
                           hipStream_t stream);
// every utterance: frame offsets, sizes, places, headers, and every frame (work: all of them) into dst; digests
// (null: zeros) go into STREAMINFO; the SEEKTABLE of every utterance that has points (max_points: the most of one)
hipError_t launch_flac_pack(const FlacParams &p, const FlacUtt *utts, uint32_t n_utts, const FlacWork *work,
                            uint32_t n_frames, const uint32_t *fsize, uint64_t *foff, FlacOut *out, uint64_t *total,
                            uint8_t *dst, hipStream_t stream, const uint32_t *digests = nullptr,
                            uint32_t max_points = 0);

// Output sample formats (jb_format.hip; the rules and FormatUtt: jb_format.h): utts_dev[0..n) of `tiles` tiles in all
hipError_t launch_format(uint32_t format, uint32_t dither, uint64_t seed, const FormatUtt *utts_dev, uint32_t n,
                         uint64_t tiles, hipStream_t stream);

// IMA ADPCM (jb_adpcm.hip; the rules and AdpcmUtt: jb_adpcm.h): utts_dev[0..n) of `groups` workgroups in all, their
// x f64 or 16-bit samples by i16
hipError_t launch_adpcm(bool i16, const AdpcmUtt *utts_dev, uint32_t n, uint64_t groups, hipStream_t stream);

// The distinct geometries of a launch of the filterbank features or the mel spectrograms, one per rate: their tables
// on the host.  A stage states its geometry and its tables (rate_geometry, rate_tables), the body of bind and, for the
// pass that RatePass below puts together, a unit's frames, the frames of a workgroup and the launch (rate_frames,
// rate_wg_frames, rate_launch)
struct RateNoCond {};
template <class Opts, class Geom, class Tables, class Class, class Cond = RateNoCond> struct RateClasses {
    typedef Opts opts_type;
    typedef Class class_type;
    typedef Cond cond_type;
    Cond cond{}; // what conditions every class of the launch beside the options (RatePass::start sets it)
    std::vector<uint32_t> key_hz;
    std::vector<Geom> geom;
    std::vector<Tables> tables;
    // the class of `hz` (made at its first use), or JB_ERR_INVALID naming the field that is out of its limits there
    int find(const Opts &opts, uint32_t hz, const char *who, uint32_t *cls)
    {
        for (size_t i = 0; i < key_hz.size(); i++)
            if (key_hz[i] == hz) {
                *cls = (uint32_t)i;
                return JB_OK;
            }
        Geom g{};
        const int rc = rate_geometry(&opts, hz, who, &g);
        if (rc)
            return rc;
        Tables t; // (a class is listed once its tables stand)
        if (!rate_tables(g, hz, opts, cond, &t)) {
            set_error(std::string(who) + ": the filterbank at " + std::to_string(hz) + " Hz has no by-bin form");
            return JB_ERR_INVALID;
        }
        *cls = (uint32_t)key_hz.size();
        key_hz.push_back(hz);
        geom.push_back(g);
        tables.push_back(std::move(t));
        return JB_OK;
    }
    // the image (to be copied to `dev`) and the classes that point into it
    void bind(const Opts &opts, const double *dev, std::vector<double> *image, std::vector<Class> *out) const;
    size_t words() const // doubles of the image: of the one bind makes
    {
        std::vector<double> image;
        std::vector<Class> classes;
        bind(Opts{}, nullptr, &image, &classes);
        return image.size();
    }
};

// Filterbank features (jb_fbank.hip; the rule, FbankClass and FbankUtt: jb_fbank.h; the host half: jb_fbank.cpp)
inline int rate_geometry(const FbankOpts *o, uint32_t hz, const char *who, FbankGeom *g)
{
    return fbank_geometry(o, hz, who, g);
}
inline bool rate_tables(const FbankGeom &g, uint32_t hz, const FbankOpts &o, const FrameOpts &fr, FbankTables *t)
{
    if (!fbank_tables(g, hz, o.window, t))
        return false;
    frame_window(o.window, fr.window, g.wl, t->win.data());
    return true;
}
// (the class key: the rate, under the one FrameOpts of the launch)
typedef RateClasses<FbankOpts, FbankGeom, FbankTables, FbankClass, FrameOpts> FbankClasses;
template <>
void FbankClasses::bind(const FbankOpts &opts, const double *dev, std::vector<double> *image,
                        std::vector<FbankClass> *out) const;
// utts_dev[0..n) of `groups` workgroups in all; framed: the classes carry a frame request (the conditioned loader)
hipError_t launch_fbank(const FbankClass *classes_dev, const FbankUtt *utts_dev, uint32_t n, uint64_t groups,
                        hipStream_t stream, bool framed);
inline uint64_t rate_frames(const FbankOpts &o, const FrameOpts &fr, const FbankGeom &g, uint64_t n)
{
    return frame_count(n, g, o, fr);
}
inline uint32_t rate_wg_frames(const FbankGeom &g) { return fbank_wg_frames(g.n_fft); }
// (the one place that decides between k_fbank<false> and k_fbank<true>: jb_fbank.h "Frame conditioning")
inline hipError_t rate_launch(const FbankOpts &, const FrameOpts &fr, const FbankClass *classes_dev,
                              const FbankUtt *utts_dev, uint32_t n, uint64_t groups, hipStream_t stream)
{
    return launch_fbank(classes_dev, utts_dev, n, groups, stream, !frame_is_identity(fr));
}

// Mel spectrograms (jb_melspec.hip; the rule, MelClass and MelUtt: jb_melspec.h; the host half: jb_melspec.cpp)
inline int rate_geometry(const MelOpts *o, uint32_t hz, const char *who, MelGeom *g)
{
    return mel_geometry(o, hz, who, g);
}
inline bool rate_tables(const MelGeom &g, uint32_t hz, const MelOpts &o, const RateNoCond &, MelTables *t)
{
    return mel_tables(g, hz, o, t);
}
typedef RateClasses<MelOpts, MelGeom, MelTables, MelClass> MelClasses;
template <>
void MelClasses::bind(const MelOpts &opts, const double *dev, std::vector<double> *image,
                      std::vector<MelClass> *out) const;
// utts_dev[0..n) of `groups` workgroups in all; with `ranged` (the options' range above 0) k_melspec_max and
// k_melspec_finish behind k_melspec: gmax one double per workgroup, umax one per unit (scratch; else unused)
hipError_t launch_melspec(const MelClass *classes_dev, const MelUtt *utts_dev, uint32_t n, uint64_t groups, bool ranged,
                          double *gmax, double *umax, hipStream_t stream);
inline uint64_t rate_frames(const MelOpts &o, const RateNoCond &, const MelGeom &g, uint64_t n)
{
    return mel_frames(n, g.n_fft, g.hop, o.pad, o.flags);
}
inline uint32_t rate_wg_frames(const MelGeom &g) { return mel_wg_frames(g.n_fft); }
inline hipError_t rate_launch(const MelOpts &o, const RateNoCond &, const MelClass *classes_dev, const MelUtt *utts_dev,
                              uint32_t n, uint64_t groups, hipStream_t stream, double *gmax, double *umax)
{
    return launch_melspec(classes_dev, utts_dev, n, groups, o.range > 0.0, gmax, umax, stream);
}

// Cepstral features (jb_mfcc.hip; the rule, MfccParams and MfccUtt: jb_mfcc.h; the host half: jb_mfcc.cpp):
// utts_dev[0..n) of `tiles` frame tiles and `blocks` statistics blocks in all; k_ceps (with n_ceps), the statistics'
// passes (with CMVN) and k_delta, in that order on `stream`
hipError_t launch_mfcc(const MfccParams &P, const MfccUtt *utts_dev, uint32_t n, uint64_t tiles, uint64_t blocks,
                       hipStream_t stream);

// The programme stage: the join (jb_join.hip; the rules, ProgMember and ProgSpan: jb_join.h) and the mix (jb_mix.hip;
// the rules and MixSeg: jb_mix.h; the host half: jb_mix.cpp) over one layout (jb_output.h mix_layout).
// mix_layout with the request's and the options' fields checked and set_error naming what is wrong (JB_ERR_INVALID;
// lists past kMixMaxList entries: JB_ERR_UNSUPPORTED).  opts may be null.  `chained`: req is a join's (join_as_mix),
// and the refusals are worded for the join
// stem_of: [B] the stems request behind a mix's (jb_mix.h "Stems"; with `chained`: refused), nullptr: none
int mix_layout_checked(const MixUtt *req, bool chained, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem,
                       const MixOpts *opts, MixLayout *out, const char *who, const uint32_t *stem_of = nullptr);
// The same from the join's own request
int join_layout_checked(const JoinUtt *req, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem,
                        MixLayout *out, const char *who);
// The lists of a run: members[i] for the layout's members[i] (utterance u's samples at x + xoff[u] elements) and one
// span per unit, whole (unit p at y + units[p].off elements; the stems behind the programmes); *tiles their tiles, the
// peak scratch's slots / kMixWaves
void mix_lists(const MixLayout &lay, const MixUtt *req, const uint64_t *n, const uint64_t *xoff, const void *x, void *y,
               size_t elem, std::vector<ProgMember> *members, std::vector<ProgSpan> *spans, uint64_t *tiles);
// The join's launch over the same members and spans (k_join reads neither the segments nor the gains): spans_dev[0..n)
// of `tiles` tiles in all, their samples f64 or 16-bit by i16
hipError_t launch_join(bool i16, const ProgSpan *spans_dev, uint32_t n, uint64_t tiles, const ProgMember *members_dev,
                       hipStream_t stream);
// What a launch reads on the device beside its spans
struct MixLaunch {
    const ProgMember *members;
    const MixSeg *segs;
    const uint32_t *lists;
    double *tile_peak; // kMixWaves per tile, by the spans' pk0
    MixResult *res;    // by the spans' prog
    bool fit;          // kMixFit: the second pass follows
    double ceiling;    // in sample units, with fit
    uint32_t stems;      // the last `stems` spans of the list are stems (they stand behind the programmes), of
    uint64_t stem_tiles; // `stem_tiles` tiles: with fit they take their programme's scale and are not clamped
};
// spans_dev[0..n) of `tiles` tiles in all: k_mix, k_mix_peak and with fit k_mix again over the programmes of s != 1
// and the stems of such programmes
hipError_t launch_mix(bool i16, const ProgSpan *spans_dev, uint32_t n, uint64_t tiles, const MixLaunch &L,
                      hipStream_t stream);
// The level items of the units picked by mask ([P + S]; empty: all): one per stem over the tiles of its extent, one
// per programme that has a stem over all of its tiles (unit p at y + units[p].off elements); t0 counted from 0 over
// the list, s0 the full numbering's (a redo keeps it); *tiles: the list's tiles.  scratch (may be null): the full
// numbering's tiles
void mix_level_items(const MixLayout &lay, const void *y, size_t elem, const std::vector<uint8_t> &mask,
                     std::vector<LevelItem> *items, uint64_t *tiles, uint64_t *scratch);
// A stem's report from what the device left: its peak, its programme's scale and, with levels, the sums (its own pair
// and its programme's E_p) and the dB values the host derives from them
inline jb_stem_report stem_report_of(double peak, double scale, bool levels, MixSums own, double e_p)
{
    jb_stem_report r{};
    r.peak = peak;
    r.scale = scale;
    r.level_db = r.sir_db = r.si_sdr_db = NAN;
    if (levels) {
        r.e_s = own.e;
        r.d = own.d;
        r.e_p = e_p;
        level_db_of(r.e_s, r.d, r.e_p, &r.level_db, &r.sir_db, &r.si_sdr_db);
    }
    return r;
}
// k_mix_levels over the `tiles` tiles of items_dev[0..n) and the fold: tile_sums two doubles per tile by the items'
// s0, sums by the items' unit
hipError_t launch_mix_levels(bool i16, const LevelItem *items_dev, uint32_t n, uint64_t tiles, double *tile_sums,
                             MixSums *sums, hipStream_t stream);

// The speech-activity stage (jb_activity.hip; the rules, ActCol and ActUnit: jb_activity.h; the host half:
// jb_activity.cpp).  opts checked with set_error naming the field under the entry `who` (null: refused)
int act_check_opts(const ActOpts *opts, const char *who);
// act_layout with set_error naming the unit and the field: JB_ERR_INVALID, or JB_ERR_UNSUPPORTED past a cap
int act_layout_checked(const ActOpts &o, size_t P, const uint64_t *unit_n, const uint32_t *unit_hz, const uint32_t *first,
                       const uint32_t *members, const uint64_t *start, const uint64_t *n, const double *gain,
                       ActLayout *out, const char *who);
// cols_dev[0..n_cols) of `energy_wgs` workgroups in all, their sources f64 or 16-bit by i16: the columns' maxima
// (col_max[n_cols], scratch by list position) cleared, k_act_energy, k_act_label (reports[slot] of each column; a
// unit's first column clears unit_reports[unit]), then units_dev[0..n_units) of `unit_wgs` workgroups: k_act_unit.
// A list holds every column of each of its units
hipError_t launch_activity(bool i16, const ActCol *cols_dev, uint32_t n_cols, uint64_t energy_wgs,
                           const ActUnit *units_dev, uint32_t n_units, uint64_t unit_wgs, uint64_t *col_max,
                           ActReport *reports, ActUnitReport *unit_reports, const ActLaunch &L, hipStream_t stream);

// The pitch stage (jb_pitch.hip; the rules, PitchClass and PitchUtt: jb_pitch.h; the host half: jb_pitch.cpp).  opts
// checked with set_error naming the field under the entry `who` (null: refused), the lag grid into *grid (may be null);
// a unit's rate checked (JB_ERR_UNSUPPORTED past the phase table's cap), its phase table into *down (may be null)
int pitch_check_opts(const PitchOpts *opts, const char *who, PitchGrid *grid);
int pitch_check_rate(uint32_t hz, size_t unit, const char *who, PitchDown *down);
jb_pitch_geometry_t pitch_geometry_of(const PitchOpts &o, const PitchGrid &g, uint32_t hz, uint64_t n);
// utts_dev[0..n_utts) in unit order with `tiles`, `post_wgs` and `cols_wgs` workgroups in all: k_pitch_down,
// k_pitch_track (a workgroup per unit), k_pitch_post and, without JB_PITCH_RAW, k_pitch_cols
hipError_t launch_pitch(const PitchUtt *utts_dev, uint32_t n_utts, uint64_t tiles, uint64_t post_wgs, uint64_t cols_wgs,
                        const PitchClass &cls, hipStream_t stream);

// The filter stage (jb_filter.hip; the rules, FilterClass and FilterUtt: jb_filter.h; the host half: jb_filter.cpp)
// f at `hz`: its coefficients into c ([n_sections][5], may be null), or JB_ERR_INVALID with set_error naming the
// utterance `utt`, the section and the field
int filter_design_checked(const jb_filter *f, uint32_t hz, size_t utt, double *c, const char *who);
void filter_class_build(const double *c, uint32_t ns, FilterClass *out); // the device table of designed coefficients
// The distinct (filter, rate) pairs of f[0..nf) (nf == 1: one filter for all) over hz[0..B): their tables and each
// utterance's class; every utterance without sections shares one identity class
int filter_classes(const jb_filter *f, size_t nf, const uint32_t *hz, size_t B, std::vector<FilterClass> *classes,
                   std::vector<uint32_t> *cls_of, const char *who);
// A launch list: the utterances `only` marks (null: all) sorted by their classes' section count, t0 filled in;
// count[ns] / tiles[ns]: the utterances and tiles of each count
struct FilterLaunch {
    std::vector<FilterUtt> utts;
    uint32_t count[kFiltMaxSections + 1] = {};
    uint64_t tiles[kFiltMaxSections + 1] = {};
};
int filter_launch_list(const std::vector<FilterClass> &classes, const std::vector<FilterUtt> &utts,
                       const std::vector<uint8_t> *only, FilterLaunch *out);
// utts_dev: a launch list on the device; st: kFiltMaxD doubles per tile of the batch; per section count present the
// three launches (zero-state tiles, the utterance scan, the tiles again from their start states), a copy for count 0
hipError_t launch_filter(const FilterClass *classes_dev, const FilterUtt *utts_dev, const FilterLaunch &l, double *st,
                         bool i16, hipStream_t stream);

// The convolution stage (jb_fir.hip; the rule, FirClass and FirUtt: jb_fir.h; the host half: jb_fir.cpp).
// f at the output rate `hz`: JB_OK, or JB_ERR_INVALID with set_error naming the utterance `utt` and the field
int fir_check(const jb_fir *f, uint32_t hz, size_t utt, const char *who);
// The distinct responses of a launch, by content (taps, delay, rate): their host copies
struct FirClasses {
    std::vector<FirResponse> resp;
    uint32_t find(const FirSpec &f); // the class of an accepted request with taps (made at its first use)
    // the image (to be copied to `dev`) and the classes that point into it
    void bind(const double *dev, std::vector<double> *image, std::vector<FirClass> *out) const;
    size_t words() const // doubles of the image: of the one bind makes
    {
        std::vector<double> image;
        std::vector<FirClass> classes;
        bind(nullptr, &image, &classes);
        return image.size();
    }
};
// The partitions' spectra ([P][M + 1][2], scaled by 1 / M) and the twiddles ([M + 1][2]) of a partitioned response
void fir_spectra(const FirResponse &r, std::vector<double> *H, std::vector<double> *tw);
// The launch lists of the utterances `has` marks (and `only`, where not null): the direct ones and the partitioned
// ones, each in utterance order with g0 filled in; tiles / blocks: their workgroups
struct FirLaunch {
    std::vector<FirUtt> direct, part;
    uint64_t tiles = 0, blocks = 0, frames = 0; // frames: the partitioned list's spectra (jb_fir.h: fir_frames)
};
void fir_launch_lists(const std::vector<FirResponse> &resp, const std::vector<FirUtt> &utts,
                      const std::vector<uint8_t> &has, const std::vector<uint8_t> *only, FirLaunch *out);
// k_fir_direct over direct_dev[0..n_direct), k_fir_spectrum and k_fir_mac over part_dev[0..n_part); spec: the
// spectrum scratch, 16 bytes per bin
hipError_t launch_fir(const FirClass *classes_dev, const FirUtt *direct_dev, uint32_t n_direct, uint64_t tiles,
                      const FirUtt *part_dev, uint32_t n_part, uint64_t blocks, uint64_t frames, double *spec,
                      hipStream_t stream);

// Room responses (jb_room.hip; the rule, RoomTables and RoomDev: jb_room.h; the host half: jb_room.cpp).
// The room `idx` of a call checked and its tables made (t may be null): JB_OK, JB_ERR_INVALID (set_error names the
// room and the field) or JB_ERR_UNSUPPORTED (an axis table or the work above its bound); touches no device
int room_check(const jb_room *r, size_t idx, const char *who, RoomTables *t);
const std::vector<double> &room_lowpass(); // F: kRoomTable entries, made at the first call
void room_host_taps(const RoomTables &t, double *h); // the rule on the host: h[0..K)
jb_room_report room_report_of(const double *h, uint32_t K, uint32_t direct, uint32_t delay);
// JB_ROOM_VARY's positions of the utterance of index k (JB_ERR_INVALID names what is wrong)
int room_vary(uint64_t seed, uint64_t k, const double size[3], double margin, double source[3], double mic[3],
              const char *who);
// The responses of r[0..n) (room_none entries: left empty) generated on `device` (< 0: the current one): h[u] and,
// where not null, tabs[u]; rooms equal by content are generated once
int room_rirs(const jb_room *r, size_t n, int device, std::vector<std::vector<double>> *h,
              std::vector<RoomTables> *tabs, const char *who);
// k_room over rooms_dev[0..n) (their tables in `image`), `tiles` workgroups of taps per room at most; table_words:
// the doubles of the largest room's three tables
hipError_t launch_room(const RoomDev *rooms_dev, uint32_t n, uint32_t tiles, uint32_t table_words, const double *image,
                       const double *F, double *out, hipStream_t stream);

// The noise stage (jb_noise.hip; the rule, NoiseUtt and NoiseRecord: jb_noise.h; the host half: jb_noise.cpp).
// req at the output rate `hz`: JB_OK, or JB_ERR_INVALID with set_error naming the utterance `utt` and the field
int noise_check(const jb_noise *req, uint32_t hz, size_t utt, const char *who);
// An accepted request of one utterance, resolved
struct NoiseItem {
    bool on = false;     // the utterance has a request
    bool active = false; // JB_NOISE_REF_ACTIVE
    int32_t bed = -1;    // its bed in NoiseBeds, -1: white
    uint32_t offset = 0;
    uint64_t seed = 0;
    double snr_db = 0.0, r = 0.0, q = 0.0; // r = 10^(snr_db / 10), q = 10^(-gate_db / 10) (0 with _WHOLE)
};
// `vary`: JB_NOISE_VARY's seed and offset of the utterance of index k
NoiseItem noise_resolve(const jb_noise &req, bool vary, uint64_t k, int32_t bed);
// The distinct beds of a launch, by content (samples, rate): their host copies
struct NoiseBeds {
    std::vector<std::vector<double>> beds;
    std::vector<uint32_t> rate;
    int32_t find(const double *w, uint32_t len, uint32_t hz); // made at its first use
    uint64_t words() const;                                   // doubles of the device image
    void bind(const double *dev, std::vector<double> *image, std::vector<NoiseBed> *out) const;
};
jb_noise_report noise_report_of(const NoiseItem &it, const NoiseRecord &r, uint64_t n);
// The launch list of the utterances `has` marks (and `only`, where not null), in utterance order with t0 and a0
// filled in; tiles / apply: the workgroups of the sums and of the apply pass
struct NoiseLaunch {
    std::vector<NoiseUtt> utts;
    uint64_t tiles = 0, apply = 0;
};
void noise_launch_list(const std::vector<NoiseUtt> &utts, const std::vector<uint8_t> &has,
                       const std::vector<uint8_t> *only, NoiseLaunch *out);
// k_noise_sums, k_noise_gain and k_noise_apply over utts_dev[0..n); sums: the scratch, two doubles per tile; rec: the
// records the utterances' `rep` index
hipError_t launch_noise(const NoiseUtt *utts_dev, uint32_t n, uint64_t tiles, uint64_t apply, double *sums,
                        NoiseRecord *rec, hipStream_t stream);

// The limiter stage (jb_limiter.hip; the rules, LimiterClass and LimiterUtt: jb_limiter.h; the host half:
// jb_limiter.cpp).  opts (null: the defaults) checked and resolved into *out (may be null), or JB_ERR_INVALID with
// set_error naming the utterance `utt` and the field
int limiter_check(const jb_limiter_opts *opts, size_t utt, const char *who, LimOpts *out);
// L and H of a resolved request at hz; JB_ERR_UNSUPPORTED for 2 L + H above kLimMaxSpan
int limiter_geometry(const LimOpts &r, uint32_t hz, size_t utt, const char *who, uint32_t *L, uint32_t *H);
void limiter_window(uint32_t L, double *w); // w[0..L]
int limiter_class_build(uint32_t hz, uint32_t L, uint32_t H, uint32_t mode, LimiterClass *out);
// The distinct classes of a launch: one table per (L, H) in sample mode, per (rate, L, H) in true-peak mode
struct LimiterClasses {
    std::vector<LimiterClass> tables;
    std::vector<uint32_t> key_hz;
    int find(uint32_t hz, uint32_t L, uint32_t H, uint32_t mode, uint32_t *cls);
};
// utts_dev[0..n) of `tiles` tiles in all: k_ln_limit, then the fold of each listed utterance's tiles (scratch, at the
// utterance's s0) into out[rslot]; res: the loudness results the gains are read from (null where every g is in the list)
hipError_t launch_limiter(const LimiterClass *classes_dev, const LimiterUtt *utts_dev, uint32_t n, uint64_t tiles,
                          const LoudnessResult *res, LimiterTile *scratch, LimiterResult *out, bool i16,
                          hipStream_t stream);

// Device-resident pdf tables of a voice set (jb_pdf_set) and an indexed batch source
struct PdfSet {
    int device = -1;
    uint32_t nv = 0, ns = 0;
    std::vector<const float *> tab;        // [nv * ns] device
    std::vector<uint32_t> n_rows, row_len; // [nv * ns]
    ~PdfSet();
};
struct IndexSrc {
    const PdfSet *set;
    const jb_index_utt *utts;
};
// Parameter tracks as the batch's source (SpeechGenerator::new, src/speech.rs:25-50): no MLPG
struct TrackSrc {
    const jb_track_utt *utts;
    // Vocoder::new + Vocoder::synthesize per frame (vocoder/mod.rs:45-72) instead of SpeechGenerator::new:
    // no check of the LPF length, so nlpf == 0 (the ring-buffer-less branch of Excitation::get,
    // excitation.rs:87-100) is reachable, as it is in the reference through this seam alone
    bool vocoder_level = false;
};

// What an entry that works on PCM the caller holds needs on the device for the length of the call: makes a device
// current and gives the caller its own back, owns a non-blocking stream and the device blocks it hands out.  The
// jb_*_pcm_batch entries (their host half: jb_pcm_call.h) open it, then allocate, pack, upload and read back through it:
// it carries the first HIP error of these calls (`err`; every later call is then skipped and returns null), and the
// entry asks once, with status(), before it hands anything out
struct DeviceScratch {
    int prev = -1, device = -1;
    bool changed = false;
    hipStream_t stream = nullptr;
    std::vector<void *> blocks;
    hipError_t err = hipSuccess;
    const char *who = "";
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    hipError_t enter(int dev) // dev < 0: the caller's current one
    {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess)
            prev = -1;
        device = dev < 0 ? prev : dev;
        if (e == hipSuccess && prev != device) {
            e = hipSetDevice(device);
            changed = e == hipSuccess;
        }
        return e;
    }
    // The device of an entry `name` (dev < 0: the caller's current one) made current, and the stream: JB_ERR_DEVICE
    // (set_error says which) without a device
    int open(int dev, const char *name)
    {
        who = name;
        const hipError_t e = enter(dev);
        if (prev < 0) {
            set_error("no HIP device");
            return JB_ERR_DEVICE;
        }
        if (e != hipSuccess) {
            set_error("hipSetDevice failed");
            return JB_ERR_DEVICE;
        }
        err = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        return JB_OK;
    }
    bool ok() const { return err == hipSuccess; }
    int status() const { return ok() ? JB_OK : hip_fail(err, who); }
    template <class T> T *alloc(size_t n) // max(n, 1) elements
    {
        T *p = nullptr;
        if (ok() && (err = hipMalloc((void **)&p, sizeof(T) * (n ? n : 1))) == hipSuccess)
            blocks.push_back((void *)p);
        return p;
    }
    // A block of max(v.size(), 1) elements and v on its way into it (an empty list: nothing is copied); v lives to the
    // wait of read_back
    template <class T> T *upload(const std::vector<T> &v)
    {
        T *p = alloc<T>(v.size());
        put(p, v, who);
        return p;
    }
    // alloc and the copy of upload as a Batch spells them (dalloc, put): what RatePass::bind stores through.  JB_OK
    // always: the error waits in `err`
    template <class T> int dalloc(T **p, size_t n, bool)
    {
        *p = alloc<T>(n);
        return JB_OK;
    }
    template <class T> int put(T *dst, const std::vector<T> &v, const char *)
    {
        if (ok() && !v.empty())
            err = hipMemcpyAsync(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, stream);
        return JB_OK;
    }
    // The inputs one after the other in one slab (*off: pcm_pack), each on its way into it
    template <class T> T *pack(const T *const *in, const size_t *n_in, size_t n, std::vector<uint64_t> *off)
    {
        *off = pcm_pack(n_in, n);
        T *p = alloc<T>((*off)[n]);
        for (size_t u = 0; u < n && ok(); u++)
            if (n_in[u])
                err = hipMemcpyAsync(p + (*off)[u], in[u], sizeof(T) * n_in[u], hipMemcpyHostToDevice, stream);
        return p;
    }
    // Waits for the stream, then host[0..n) = src[0..n)
    template <class T> void read_back(std::vector<T> *host, const T *src, size_t n)
    {
        if (ok())
            err = hipStreamSynchronize(stream);
        if (ok() && n) {
            host->resize(n);
            err = hipMemcpy(host->data(), src, sizeof(T) * n, hipMemcpyDeviceToHost);
        }
    }
    ~DeviceScratch()
    {
        if (stream)
            (void)hipStreamSynchronize(stream); // nothing of the call stays in flight into the blocks
        for (void *p : blocks)
            (void)hipFree(p);
        if (stream)
            (void)hipStreamDestroy(stream);
        if (changed)
            (void)hipSetDevice(prev);
    }
};
// pcm_hand_out with the text of a failed allocation in jb_last_error
inline int hand_out(const void *host, size_t elem, const std::vector<PcmShare> &shares, void **out, size_t *n_out)
{
    const char *err = "";
    const int rc = pcm_hand_out(host, elem, shares, out, n_out, &err);
    if (rc)
        set_error(err);
    return rc;
}

struct Batch;

// n elements to the device, synchronously (an empty list: nothing)
template <class T> int upload_list(T *dst, const std::vector<T> &v, const char *what)
{
    const hipError_t e =
        v.empty() ? hipSuccess : hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    return e == hipSuccess ? JB_OK : hip_fail(e, what);
}

// A work list of an output stage: the list of a full run on the host and on the device, a second device block for
// the list of a redo, and what the next launch takes of the two (take_all / upload_redo)
template <class T> struct DevList {
    std::vector<T> host;
    T *dev = nullptr, *redo = nullptr;
    const T *list = nullptr; // of the next launch
    uint32_t n = 0;          // its entries
    uint64_t total = 0;      // its tiles (or groups of blocks), where the entries number them
    template <class Alloc> int alloc(Alloc &b, size_t n_dev, size_t n_redo) // (Batch is declared below)
    {
        const int rc = b.dalloc(&dev, n_dev, false);
        return rc ? rc : b.dalloc(&redo, n_redo, false);
    }
    int upload(const char *what) { return upload_list(dev, host, what); }
    int take_all(uint64_t all = 0) // JB_OK
    {
        list = dev, n = (uint32_t)host.size(), total = all;
        return JB_OK;
    }
    int upload_redo(const std::vector<T> &v, const char *what, uint64_t of_v = 0)
    {
        list = redo, n = (uint32_t)v.size(), total = of_v;
        return upload_list(redo, v, what);
    }
};

// One pass of a rate-classed stage (the filterbank features, the mel spectrograms) put together on the host, for the
// entries on caller-held PCM and for a batch's output chain alike: the classes under the launch's condition, the unit
// list (class, n, T and g0, the prefix sum of the workgroups), each unit's workgroups -- what a redo renumbers from --
// and their sum.  start, add per unit, attach the units' pointers (list.host[u]), bind, launch
template <class Classes, class Utt> struct RatePass {
    typedef typename Classes::opts_type Opts;
    typedef typename Classes::class_type Class;
    typedef Utt Unit;
    static constexpr uint64_t kByRule = ~0ull;
    Opts opts{};
    Classes cls;
    DevList<Utt> list;             // host: the units in their order
    std::vector<uint64_t> ngroups; // each unit's workgroups
    uint64_t groups = 0;
    const Class *classes_dev = nullptr;
    std::vector<double> image; // the tables and the classes as bind sent them: they live to the wait of a store
    std::vector<Class> classes; // that copies behind the call
    void start(const Opts &o, const typename Classes::cond_type &cond = {})
    {
        *this = RatePass{};
        opts = o;
        cls.cond = cond;
    }
    // A unit of n samples at hz behind those added so far; T: its frames where the caller's plan holds them.
    // JB_ERR_INVALID naming the field that is out of its limits at hz; touches no device
    int add(uint32_t hz, uint64_t n, const char *who, uint64_t T = kByRule)
    {
        Utt w{};
        const int rc = cls.find(opts, hz, who, &w.cls);
        if (rc)
            return rc;
        const auto &g = cls.geom[w.cls];
        w.n = n;
        w.T = T == kByRule ? rate_frames(opts, cls.cond, g, n) : T;
        w.g0 = groups;
        ngroups.push_back((w.T + rate_wg_frames(g) - 1) / rate_wg_frames(g));
        groups += ngroups.back();
        list.host.push_back(w);
        return JB_OK;
    }
    // The classes' tables in a block of their own, the classes that point into it and the unit list, through `st` (a
    // DeviceScratch or a Batch: dalloc and put; what: the stage's name in a failure's text); the next launch takes the
    // whole list
    template <class Store> int bind(Store &st, const std::string &what)
    {
        double *tables = nullptr;
        Class *cd = nullptr;
        int rc = st.dalloc(&tables, cls.words(), false);
        if (rc)
            return rc;
        cls.bind(opts, tables, &image, &classes);
        if ((rc = st.put(tables, image, (what + " tables").c_str())) ||
            (rc = st.dalloc(&cd, classes.size(), false)) || (rc = st.put(cd, classes, (what + " classes").c_str())) ||
            (rc = st.dalloc(&list.dev, list.host.size(), false)) ||
            (rc = st.put(list.dev, list.host, (what + " work list").c_str())))
            return rc;
        classes_dev = cd;
        return list.take_all(groups);
    }
    // what list.take_all or list.upload_redo chose; extra: what the stage's launch takes beside the lists
    template <class... Extra> hipError_t launch(hipStream_t stream, Extra... extra) const
    {
        return rate_launch(opts, cls.cond, classes_dev, list.list, list.n, list.total, stream, extra...);
    }
};
typedef RatePass<FbankClasses, FbankUtt> FbankPass;
typedef RatePass<MelClasses, MelUtt> MelPass;

// The stages behind the vocoder of one batch, in their order -- the converter (jb_batch_set_output_rate), the filter
// (jb_batch_set_filter), loudness (jb_batch_set_loudness_target, with peak mode, groups and the R128 report), the
// join (jb_batch_set_join), then the encoders of the final PCM side by side: FLAC (jb_batch_set_flac, _flac_meta),
// the sample format (jb_batch_set_format), IMA ADPCM (jb_batch_set_adpcm) and the filterbank features
// (jb_batch_set_fbank), the cepstral features (jb_batch_set_mfcc) and the mel spectrograms (jb_batch_set_melspec) --
// and all their device state.
// The setters record a request and plan again (jb_output.h); the first run carries the plan out (prepare); every run
// enqueues the chain once behind the hand-off check, and finish_verify once more for the utterances its redo rounds
// rewrote.  Each stage has the same three steps: prepare_X (its lists and scratch), select_X (what the next launch
// takes: the run's lists, or those of a redo by the one mask of the RedoScope the stage follows) and launch_X.
// Without a request the chain holds no device memory and enqueues nothing
struct OutputChain {
    explicit OutputChain(Batch &batch) : b(batch) {}
    // Each setter refuses after the first run; the last request before it wins
    int set_output_rate(const uint32_t *hz, size_t n); // n == 1 or B entries, 0 = native
    int set_loudness(const double *target, const double *ceiling, size_t n); // n == 1 or B entries each
    int set_peak_mode(const uint32_t *mode, size_t n);                       // n == 1 or B entries; needs no target
    // group[u]: a group id below B or kLnNoGroup, n == B (nullptr, 0: the request is withdrawn); every setter that
    // could leave a group's members disagreeing (this one, target, peak mode, output rate) checks the combined request
    int set_loudness_groups(const uint32_t *group, size_t n);
    int set_loudness_report(uint32_t flags); // JB_LOUDNESS_R128 or 0
    int set_flac(const jb_flac_opts *opts);
    int set_flac_meta(const jb_flac_meta *meta); // behind set_flac
    int set_format(const jb_format_opts *opts); // an f64 batch only
    int set_adpcm(const jb_adpcm_opts *opts);   // an f64 or a 16-bit batch
    // an f64 batch only; checked at every utterance's output rate (NULL: the request is withdrawn); set_output_rate
    // checks the combined request again
    int set_fbank(const jb_fbank_opts *opts);
    // req[u]: utterance u's programme, pads and fades, n == B (nullptr, 0: the request is withdrawn); this setter and
    // set_output_rate check that a programme's members agree on the rate
    int set_join(const jb_join_utt *req, size_t n);
    // req[u]: utterance u's programme, start, pad, fades and gain, n == B, under opts (may be null); nullptr, 0: the
    // request is withdrawn.  Checked as set_join's; a batch holds a join or a mix request, the second setter is refused
    int set_mix(const jb_mix_utt *req, size_t n, const jb_mix_opts *opts);
    int read_mix(size_t p, jb_mix_report *out); // after sync
    // The stems request behind a mix's (jb_mix.h "Stems"): one id per utterance, or JB_MIX_NO_STEM; flags:
    // JB_MIX_STEM_LEVELS.  Null and 0 withdraw it, and so does withdrawing the mix.  Checked with the mix under the
    // present rates; refused without a mix request (or over a join)
    int set_mix_stems(const uint32_t *stem_of, size_t n, uint32_t flags);
    int read_stem(size_t unit, jb_stem_report *out); // after sync
    size_t num_programmes() const { return joined() ? plan.n_progs : plan.utt.size(); }
    int64_t stem_unit(size_t u) const { return plan.stem_unit.empty() ? -1 : plan.stem_unit[u]; }
    const MixStem *stem(size_t unit) const // null: the unit is no stem
    {
        return joined() && unit >= plan.n_progs && unit - plan.n_progs < plan.stems.size()
                   ? &plan.stems[unit - plan.n_progs]
                   : nullptr;
    }
    // the cepstral features behind a filterbank pass of their own (jb_mfcc.h): an f64 batch only; the filterbank
    // options checked at every utterance's output rate (both NULL: the request is withdrawn); set_output_rate checks
    // the combined request again.  Independent of set_fbank
    int set_mfcc(const jb_fbank_opts *fopts, const jb_mfcc_opts *opts);
    // the mel spectrograms (jb_melspec.h): an f64 batch only; checked at every utterance's output rate (NULL: the
    // request is withdrawn); set_output_rate checks the combined request again.  Independent of set_fbank and set_mfcc
    int set_melspec(const jb_melspec_opts *opts);
    // the pitch features (jb_pitch.h): an f64 batch only; checked at every utterance's output rate and against
    // JB_PITCH_MAX_SCRATCH at the first run (NULL: the request is withdrawn)
    int set_pitch(const jb_pitch_opts *opts);
    // the speech-activity labels (jb_activity.h), a side output beside whatever sinks the batch has, f64 or 16-bit:
    // checked at every unit's rate and against the caps under the present requests (NULL: the request is withdrawn),
    // and again at the first run, since the rates and the programmes may be set behind it
    int set_activity(const jb_activity_opts *opts);
    // unit u's place (JB_ERR_INVALID without a request or for no such unit; `run`: or before the run), its labels, the
    // labels of every unit in one copy (unit u at host + places[u].off), and the reports (after sync)
    int activity_place(size_t u, bool run, const char *who, ActLayUnit *out) const;
    int read_activity(size_t u, uint8_t *dst);
    int read_activity_all(std::vector<ByteSpan> *places, std::unique_ptr<uint8_t[]> *host);
    int read_activity_report(size_t u, size_t col, jb_activity_report *out);
    int read_activity_unit_report(size_t u, jb_activity_unit_report *out);
    // the frame request beside set_fbank's and set_mfcc's (jb_fbank.h "Frame conditioning"; NULL: withdrawn), in either
    // order with them: the pair is checked when both are present and again at the first run, where a request without
    // either is an error
    int set_frame_opts(const jb_frame_opts *fr);
    // f[0..n): n == 1 or B filters (nullptr, 0: the request is withdrawn), each checked at its utterance's output
    // rate; set_output_rate checks the combined request again
    int set_filter(const jb_filter *f, size_t n);
    // f[0..n): n == 1 or B responses (nullptr, 0: the request is withdrawn; taps == NULL: none for that utterance),
    // each checked at its utterance's output rate and its taps copied; set_output_rate checks the rates again
    int set_fir(const jb_fir *f, size_t n);
    // r[0..n): n == 1 or B rooms (nullptr, 0: the request is withdrawn; all bytes zero: none for that utterance, which
    // then takes others[u] where `others` ([B], the engine entries) is given): generated on the batch's device here
    // and installed in set_fir's slot, the later of the two calls replacing the earlier
    int set_room(const jb_room *r, size_t n, const jb_fir *others = nullptr);
    int read_room(size_t u, jb_room_report *out) const;
    // the geometry of utterance u's response (JB_ERR_INVALID: it has none)
    int fir_geometry_of(size_t u, FirGeom *g) const;
    // req[0..n): n == 1 or B requests (nullptr, 0: the request is withdrawn; no bed with JB_NOISE_BED: none for that
    // utterance), each checked at its utterance's output rate and its bed copied; set_output_rate checks the rates again
    // call_k (the engine entries; [B] or null): one request per utterance may carry JB_NOISE_VARY, and utterance u
    // varies by its index call_k[u] in the call
    int set_noise(const jb_noise *req, size_t n, const uint64_t *call_k = nullptr);
    int read_noise(size_t u, jb_noise_report *out); // after sync
    // opts[0..n): n == 1 or B requests (nullptr, 0: the request is withdrawn); with groups, the members must agree
    int set_limiter(const jb_limiter_opts *opts, size_t n);
    int read_limiter(size_t u, jb_limiter_report *out); // after sync
    // the coefficients the device runs for utterance u at its output rate (*n = 0 without a filter)
    int filter_coefficients(size_t u, jb_biquad *out, uint32_t *n) const;
    void init();   // Batch::create: the slabs the batch was made with, the plan of no request
    int prepare(); // at the first run: every slab, table and list of the plan; points the vocoder at its slab
    // only: [B] 1 = the utterances a redo rewrote: their part of every stage again (the FLAC pack: every stream),
    // then one wait
    int enqueue(const std::vector<uint8_t> *only = nullptr);

    bool active() const { return plan.active(); } // the PCM is converted or normalized behind the vocoder
    // what the PCM read entries hand out: utterance u's samples, rate and place in the slab, the slab by type
    size_t samples(size_t u) const { return (size_t)plan.utt[u].n; }
    size_t offset(size_t u) const { return u < plan.utt.size() ? (size_t)plan.utt[u].off : (size_t)plan.total; }
    size_t total() const { return (size_t)plan.total; }
    const OutUtt &utt(size_t u) const { return plan.utt[u]; }
    const double *pcm64() const { return plan.final.i16 ? nullptr : (const double *)slab[(size_t)plan.final.slab]; }
    const int16_t *pcm16() const { return plan.final.i16 ? (const int16_t *)slab[(size_t)plan.final.slab] : nullptr; }
    const void *pcm() const { return slab[(size_t)plan.final.slab]; }
    const double *native64() const { return (const double *)slab[(size_t)plan.native64]; } // null: there is none
    // after sync (each reports a stage that was not set, or a batch that has not run, as JB_ERR_INVALID)
    int read_loudness(size_t u, LoudnessResult *r);
    uint32_t peak_mode(size_t u) const { return u < ln_mode.size() ? ln_mode[u] : 0u; }
    // the dense group of utterance u (-1 without a group request), its members, its result and the R128 fields of an
    // utterance or of utterance u's group
    int32_t group_of(size_t u) const { return ln_groups.group_of.empty() ? -1 : (int32_t)ln_groups.group_of[u]; }
    uint32_t group_members(size_t u) const;
    int read_loudness_group(size_t u, LoudnessGroupResult *r);
    bool report_on() const { return ln_report != 0; }
    int read_loudness_range(size_t u, bool of_group, LoudnessRange *r);
    // The byte sinks (every SynthSink but Pcm) through one path; byte_sink() holds what they differ in.
    // sink_ready: JB_ERR_INVALID with the sink's message when it was not requested or, with `run`, has not run.
    // sink_spans: the places of the outputs [u0, u0 + n) in the sink's slab -- from the plan, known once the request
    // is made; FLAC's from the device's index in one small copy, so after the run only.
    // sink_read: the bytes of an output at the span sink_spans gave (after the run)
    int sink_ready(SynthSink sink, bool run) const;
    int sink_spans(SynthSink sink, size_t u0, size_t n, ByteSpan *w);
    int sink_read(SynthSink sink, const ByteSpan &w, uint8_t *dst);
    // every output of a byte sink: the used part of its slab in one copy, output u at host + places[u].off
    int read_bytes_all(SynthSink sink, std::vector<ByteSpan> *places, std::unique_ptr<uint8_t[]> *host);
    // the plan's entry of output u, behind sink_ready(sink, false): the ADPCM block size, the features' frames and
    // width, and the rate and filters the features are computed at
    const OutAdpcmUtt &adpcm_place(size_t u) const { return plan.adpcm[u]; }
    const OutFbankUtt &fbank_place(size_t u) const { return plan.fbank[u]; }
    const OutMfccUtt &mfcc_place(size_t u) const { return plan.mfcc[u]; }
    const OutMelUtt &melspec_place(size_t u) const { return plan.melspec[u]; }
    uint32_t melspec_mels() const { return ml_p.n_mels; }
    const OutPitchUtt &pitch_place(size_t u) const { return plan.pitch[u]; }
    uint32_t fbank_mels() const { return fb_p.n_mels; }
    uint32_t fbank_hz(size_t u) const { return joined() ? plan.units[u].hz : plan.utt[u].hz; }
    // the join: what the encoders' entries index (the programmes, or the utterances without a request), an
    // utterance's programme (-1 without a request) and start, a programme's place, members and PCM
    bool joined() const { return plan.join.slab != OutSlab::None; } // a join or a mix request
    bool mixed() const { return plan.mixed; }                        // the programmes are a mix request's
    size_t num_outputs() const { return joined() ? plan.units.size() : plan.utt.size(); }
    int32_t programme_of(size_t u) const { return joined() ? (int32_t)plan.prog_of[u] : -1; }
    uint64_t member_start(size_t u) const { return plan.prog_start[u]; }
    const OutUnit &programme(size_t p) const { return plan.units[p]; }
    size_t programme_members(size_t p) const // (a stem's unit: the members under its id)
    {
        return p < plan.n_progs ? plan.prog_first[p + 1] - plan.prog_first[p] : plan.stems[p - plan.n_progs].n_members;
    }
    int read_programme(size_t p, bool i16, void *dst);

private:
    Batch &b;
    OutPlan plan;
    std::vector<uint32_t> want_hz;             // [B] 0 = native; empty: no rate requested
    bool ln_on = false, flac_on = false;       // a loudness target / FLAC is requested
    bool fmt_on = false;                       // a sample format is requested
    jb_format_opts fmt_p{};
    bool ad_on = false;                        // IMA ADPCM is requested
    uint32_t ad_align = 0;                     // its block_align (0: by the rate)
    bool fb_on = false;                        // filterbank features are requested
    FbankOpts fb_p{};
    bool mf_on = false;                        // cepstral features are requested
    FbankOpts mf_fb{};                         // their filterbank options, as the caller gave them
    MfccOpts mf_p{};
    bool fr_on = false;                        // a frame request stands beside the two above
    FrameOpts fr_p{};
    bool ml_on = false;                        // mel spectrograms are requested
    MelOpts ml_p{};
    bool pt_on = false;                        // pitch features are requested
    PitchOpts pt_p{};
    bool act_on = false;                       // speech-activity labels are requested
    ActOpts act_p{};
    std::vector<MixUtt> prog_req;              // [B] the programme request, a join's (join_as_mix) or a mix's; empty: none
    bool prog_chained = false;                 // it is a join's: its starts count from the member in front
    MixOpts mix_opts{};                        // a mix's options
    std::vector<uint32_t> stem_req;            // [B] the stems request behind a mix's; empty: none
    uint32_t stem_flags = 0;                   // kMixStemLevels
    std::vector<jb_filter> filt_req;           // [B] the filter request; empty: none
    std::vector<uint8_t> filt_any;             // [B] 1 = that utterance's filter has a section
    FirClasses fir_cls;                        // the distinct responses of the convolution request (its copies)
    std::vector<int32_t> fir_of;               // [B] an utterance's response in fir_cls, -1: none; empty: no request
    std::vector<jb_room_report> room_rep;      // [B] what set_room read back; empty: no room made the slot's responses
    std::vector<uint8_t> room_has;             // [B] 1 = that utterance's response is a room's
    NoiseBeds noise_beds;                      // the distinct beds of the noise request (its copies)
    std::vector<NoiseItem> noise_req;          // [B] the noise request, resolved; empty: none
    std::vector<uint8_t> stage_any;            // [B] 1 = a section, a response or a noise request: the plan's filter flag
    std::vector<double> ln_target, ln_ceiling; // [B]
    std::vector<LimOpts> lim_req;              // [B] the limiter request, resolved; empty: none
    std::vector<uint32_t> ln_mode;             // [B] JB_PEAK_*; empty: sample peak everywhere
    std::vector<uint32_t> ln_group_req;        // [B] the caller's ids; empty: no group request
    LnGroups ln_groups;                        // the request planned (empty without one)
    uint32_t ln_report = 0;                    // JB_LOUDNESS_R128: the report is requested
    FlacParams flac_p{};
    FlacMeta flac_m{}; // MD5 / SEEKTABLE request (zeros: none)
    bool frozen = false, ready = false; // the first run has begun: no more requests / its prepare() succeeded
    void *slab[(size_t)OutSlab::Count] = {};
    struct Converter { // follows `measured`
        ResampleTable *tables_dev = nullptr;
        DevList<ResampleTile> tiles; // sorted by utterance: utterance u owns [tile_lo[u], tile_lo[u + 1])
        std::vector<uint32_t> tile_lo;
        size_t lds = 0;              // dynamic LDS of its launches
    } rs;
    struct Filter { // follows `measured`
        std::vector<FilterClass> classes;
        DevList<FilterUtt> utts;             // host: [B] by utterance index; on the device: a launch list
        FilterLaunch all, sub;               // the launch list of a run, of the last redo
        const FilterLaunch *take = nullptr;  // of the next launch
        FilterClass *classes_dev = nullptr;
        double *st = nullptr;                // kFiltMaxD doubles per tile
        std::vector<uint8_t> mine;           // [B] 0 = the convolution or the noise writes the stage's output; empty: all 1
    } fil;
    struct Fir { // follows `measured`; in front of the filter's kernels
        std::vector<FirUtt> host;            // [B] by utterance index
        std::vector<uint8_t> has;            // [B] 1 = the utterance has a response
        DevList<FirUtt> direct, part;        // the launch lists
        FirLaunch all, sub;                  // of a run, of the last redo
        uint64_t frames = 0;                 // the spectra of the next launch's partitioned list
        FirClass *classes_dev = nullptr;
        double *tables = nullptr;            // the classes' image
        double *spec = nullptr;              // the spectrum scratch of the partitioned utterances
        double *mid = nullptr;               // f64, the plan's geometry: what a sub-stage with another behind it writes
    } fir;
    struct Noise { // follows `measured`; behind the convolution's kernels, in front of the filter's
        std::vector<NoiseUtt> host;          // [B] by utterance index
        std::vector<uint8_t> has;            // [B] 1 = the utterance has a request
        DevList<NoiseUtt> utts;              // the launch list
        NoiseLaunch all, sub;                // of a run, of the last redo
        uint64_t tiles = 0, apply = 0;       // of the next launch
        double *beds = nullptr;              // the beds' image
        double *sums = nullptr;              // two doubles per tile of 1,024 samples, by the full run's numbering
        NoiseRecord *rec = nullptr;          // [B]
    } noi;
    struct Loudness { // measurement and an utterance's report set: `measured`; the apply pass with groups: `post`
        DevList<LoudnessUtt> utts;             // [B]; total: the measurement's tiles
        DevList<LoudnessUtt> apply;            // what the apply pass takes: `utts`, or on a redo with groups a list
                                               // of its own (only `redo` is a block of its own); total: its tiles
        std::vector<uint64_t> ntiles, natiles; // [B] each utterance's measurement and apply tiles
        LoudnessRate *rates_dev = nullptr;
        double *st = nullptr, *pk = nullptr, *tp = nullptr, *z = nullptr;
        LoudnessResult *res = nullptr;
        uint64_t tiles = 0, atiles = 0; // of the batch
        bool true_peak = false;         // some utterance is in JB_PEAK_TRUE mode
        // with a group or a report request only
        DevList<LoudnessSet> sets;       // [B] the utterances, then [G] the groups (a redo: the measured, the touched)
        uint32_t n_usets = 0;            // the utterances' sets of the next launch: the groups' follow them
        uint32_t *members_dev = nullptr; // [B] the identity, then [B] the groups' members
        LoudnessGroupResult *gres = nullptr; // [G]
        double *sw = nullptr, *mm = nullptr; // the report's windows (per tile slot) and momentary maxima (per utterance)
        LoudnessRange *r128 = nullptr;       // [B + G]
    } ln;
    struct Limiter { // follows `post`, in the place of the apply pass
        DevList<LimiterUtt> utts;     // [B]; total: the tiles
        std::vector<uint64_t> ntiles; // [B]
        std::vector<uint32_t> L, H;   // [B] (0, 0: that utterance is not limited)
        LimiterClass *classes_dev = nullptr;
        LimiterTile *scratch = nullptr; // per tile
        LimiterResult *res = nullptr;   // [B]
        uint64_t tiles = 0;
    } lim;
    struct Programme { // the join or the mix.  A join follows `post`: each changed member's own range runs again;
                       // a mix follows `units`: a touched programme runs again whole
        std::vector<ProgMember> members; // in programme order: programme p owns [prog_first[p], prog_first[p + 1])
        std::vector<uint32_t> member_at; // [B] utterance -> its place in `members`
        DevList<ProgSpan> spans;         // [P] every programme whole (a join's redo: one span per member)
        MixLaunch L{};                   // the members; with a mix the segments and their lists, the peak scratch, the results
        uint64_t tiles = 0;
        // with a stems request and its levels: the items of a full run (a redo: those of the touched units), the
        // tile sums by the full numbering and the sums per unit; lay: the layout's units, stems and programme count
        // alone (what mix_level_items reads), empty without levels
        MixLayout lay;
        DevList<LevelItem> items;
        uint64_t level_tiles = 0;
        double *tile_sums = nullptr;
        MixSums *sums = nullptr;
    } pg;
    struct Flac { // follows `units`, by work item; the pack takes every stream
        DevList<FlacWork> work;
        DevList<uint32_t> md5;     // with an MD5 request: the units in launch order
        std::vector<FlacUtt> utts; // (kept with an MD5 request: the redo's launch list is ordered by their lengths)
        FlacUtt *utts_dev = nullptr;
        uint32_t *digests = nullptr; // with an MD5 request
        uint32_t max_points = 0;
        uint8_t *out = nullptr;
        uint32_t *fsize = nullptr;
        uint64_t *foff = nullptr, *total = nullptr;
        FlacOut *res = nullptr;
    } fl;
    struct Format { // follows `units`
        DevList<FormatUtt> utts;
        std::vector<uint64_t> ntiles; // [U]
        uint64_t tiles = 0;
    } fm;
    struct Adpcm { // follows `units`
        DevList<AdpcmUtt> utts;
        std::vector<uint64_t> ngroups; // [U] each unit's groups of kAdpcmLanes blocks
        uint64_t groups = 0;
    } ad;
    FbankPass fb; // follows `units`
    struct Mfcc { // follows `units`: the filterbank pass into the log-mel scratch, then the cepstral kernels
        FbankPass fbank;
        DevList<MfccUtt> utts;                  // total: the frame tiles
        std::vector<uint64_t> ntiles, nblocks;  // [U] each unit's frame tiles, blocks
        uint64_t tiles = 0, blocks = 0;
        uint64_t take_blocks = 0;               // the blocks of the next launch's list
        MfccParams P{};
    } mf;
    struct Melspec { // follows `units`: k_melspec, and with a range the fold of the maxima and the finish pass
        MelPass pass;
        double *gmax = nullptr, *umax = nullptr; // with a range: one double per workgroup, one per unit
    } ml;
    struct Pitch { // follows `units`: a unit whose final PCM changed is tracked again, whole
        DevList<PitchUtt> utts;        // [U]; a launch's entries carry its own three prefix sums
        PitchClass cls{};              // the tables of the request on the device
        uint8_t *out = nullptr;        // the rows' bytes, unit after unit on 16-byte boundaries (plan.pitch_bytes)
        double *y4 = nullptr;          // the 4 kHz signals (plan.pitch_words)
        double *tables = nullptr, *down = nullptr; // the grid's tables, and the distinct rates' phase tables
        uint32_t *tap = nullptr;
        double *tile = nullptr, *pv = nullptr, *pw = nullptr; // the tiles' sums; p and pi of every frame
        uint16_t *choice = nullptr;    // 2 S bytes a frame: allocated at the first run that needs it
        uint32_t *idx = nullptr;       // the chosen lag of every frame
        uint64_t tiles = 0, post = 0, cols = 0; // of the next launch
    } pt;
    struct Activity { // follows `units`: a unit with a rewritten member is measured again, whole
        DevList<ActCol> cols;        // every column, unit after unit; total: the energy kernel's workgroups
        DevList<ActUnit> units;      // [U]; total: the counting kernel's workgroups
        uint8_t *lab = nullptr;      // the label bytes, unit after unit on 16-byte boundaries (plan.act.bytes)
        double *en = nullptr;        // the compact energies (plan.act.energies)
        uint64_t *wd = nullptr;      // the word scratch (plan.act.words; with a smoothing length only)
        uint64_t *col_max = nullptr; // one per column of a launch list
        ActReport *rep = nullptr;    // one per column
        ActUnitReport *urep = nullptr; // [U]
        ActLaunch L{};
    } act;
    // the units the encoders take: the programmes in the join slab, or the utterances
    struct EncUnit {
        uint64_t off, n;
        uint32_t hz;
    };
    std::vector<EncUnit> enc_units() const;
    bool grouped() const { return plan.normalize() && ln.gres; } // the chain runs loudness groups
    // the limiter takes the apply pass's place: some utterance is limited (a request that limits none is no request)
    bool limited() const
    {
        if (!plan.normalize())
            return false;
        for (size_t u = 0; u < lim_req.size(); u++)
            if (limits(u))
                return true;
        return false;
    }
    // utterance u is limited: a request that is not JB_LIMITER_OFF with some depth, a target and a finite ceiling
    bool limits(size_t u) const
    {
        return !lim_req.empty() && !(lim_req[u].flags & kLimOff) && lim_req[u].max_reduction_db > 0.0 &&
               std::isfinite(ln_ceiling[u]);
    }
    int check_limiter_groups(const std::vector<uint32_t> &group, const std::vector<LimOpts> &req, const char *who) const;
    bool formatted() const { return plan.fmt_src != OutSlab::None; }
    bool adpcm() const { return plan.adpcm_src.slab != OutSlab::None; }
    bool fbank() const { return plan.fbank_src != OutSlab::None; }
    bool mfcc() const { return plan.mfcc_src != OutSlab::None; }
    bool melspec() const { return plan.melspec_src != OutSlab::None; }
    bool pitch() const { return plan.pitch_src != OutSlab::None; }
    bool activity() const { return plan.act_src.slab != OutSlab::None; }
    // why the plan holds no activity stage for the request (JB_ERR_INVALID naming the unit and the field, or
    // JB_ERR_UNSUPPORTED past a cap)
    int activity_fault(const char *who) const;
    // a feature request (FbankOpts, MelOpts) under these rates: JB_ERR_INVALID naming the field that is out of its
    // limits at some rate
    template <class Opts> int check_rates(const Opts &opts, const std::vector<uint32_t> &want, const char *who) const;
    int check_mfcc(const FbankOpts &fopts, const std::vector<uint32_t> &want, const char *who) const;
    int check_pitch(const std::vector<uint32_t> &want, const char *who) const; // every rate's phase table under `want`
    // what the three feature setters refuse alike: a batch without PCM, a 16-bit one (`noun` stage reads the f64
    // output), a batch that has run
    int check_feature_settable(const char *entry, const char *noun) const;
    // the frame request fr (null: none) beside an fbank request fb and an mfcc request (mfb, mp), each null: none
    int check_frame(const FrameOpts *fr, const FbankOpts *fb, const FbankOpts *mfb, const MfccOpts *mp,
                    const char *who) const;
    void replan(); // host geometry and routing of the present requests
    // v[0..n), n == 1 or B, as [B] values; false (set_error(err)) for anything else
    template <class T> bool broadcast(const T *v, size_t n, std::vector<T> *out, const char *err) const;
    std::vector<uint32_t> rates_under(const std::vector<uint32_t> &want) const; // [B] the output rates a request gives
    // the group request `group` ([B], empty: none) against these targets, modes and rates: JB_ERR_INVALID naming the
    // group and the field where members would disagree; *out (may be null) gets the plan
    int check_groups(const std::vector<uint32_t> &group, const std::vector<double> &target,
                     const std::vector<double> &ceiling, const std::vector<uint32_t> &mode,
                     const std::vector<uint32_t> &want, const char *who, LnGroups *out) const;
    // (stems: the stems request to check with it; null: the one the chain holds)
    int check_programme(const std::vector<MixUtt> &req, bool chained, const MixOpts &opts,
                        const std::vector<uint32_t> &want, const char *who,
                        const std::vector<uint32_t> *stems = nullptr) const;
    // the one slot of set_join and set_mix: the checks in front of the request, and the request stored
    int open_programme(bool chained, bool given, size_t n, bool *store);
    int store_programme(bool chained, std::vector<MixUtt> req, const MixOpts &opts);
    int check_filter(const std::vector<jb_filter> &req, const std::vector<uint32_t> &want, const char *who) const;
    int check_fir(const std::vector<uint32_t> &want, const char *who) const; // the responses' rates under `want`
    int install_fir(const jb_fir *f, size_t n, const char *who);             // set_fir's and set_room's common half
    int check_noise(const std::vector<uint32_t> &want, const char *who) const; // the beds' rates under `want`
    void flag_stage(); // stage_any of the three requests
    int check_settable(const char *after_run) const;
    // the stages, in the order enqueue() runs them.  scope null: a full run
    int prepare_resample(), select_resample(const RedoScope *scope), launch_resample(bool redo);
    int prepare_filter(), select_filter(const RedoScope *scope), launch_filter(bool redo);
    int prepare_fir(), select_fir(const RedoScope *scope), launch_fir(bool redo);
    int prepare_noise(), select_noise(const RedoScope *scope), launch_noise(bool redo);
    int prepare_loudness(), select_loudness(const RedoScope *scope), launch_loudness(bool redo);
    int prepare_limiter(), select_limiter(const RedoScope *scope), launch_limiter(bool redo);
    int prepare_programme(), select_programme(const RedoScope *scope), launch_programme(bool redo);
    int prepare_flac(), select_flac(const RedoScope *scope), launch_flac(bool redo);
    int prepare_format(), select_format(const RedoScope *scope), launch_format(bool redo);
    int prepare_adpcm(), select_adpcm(const RedoScope *scope), launch_adpcm(bool redo);
    int prepare_fbank(), select_fbank(const RedoScope *scope), launch_fbank(bool redo);
    int prepare_mfcc(), select_mfcc(const RedoScope *scope), launch_mfcc(bool redo);
    int prepare_melspec(), select_melspec(const RedoScope *scope), launch_melspec(bool redo);
    int prepare_pitch(), select_pitch(const RedoScope *scope), launch_pitch(bool redo);
    int prepare_activity(), select_activity(const RedoScope *scope), launch_activity(bool redo);
    int check_ready(bool requested, const char *not_run, const char *not_set) const;
    struct ByteSink {
        bool on;                       // the sink is requested
        const char *not_run, *not_set; // sink_ready's messages
        const void *slab;              // its outputs on the device
        bool planned;                  // the outputs' places come from the plan (FLAC: from the device's index)
        ByteSpan span;                 // planned: output u's place
    };
    ByteSink byte_sink(SynthSink sink, size_t u = 0) const;
    // the used bytes of a byte slab in one copy (wait: for the batch first, as Batch::read does)
    int read_used(const void *src, uint64_t bytes, bool wait, std::unique_ptr<uint8_t[]> *host);
};

struct Batch {
    int device = -1;
    uint32_t flags = 0;
    int B = 0;
    jb_voice_desc voice{};
    hipStream_t stream = nullptr;            // main: MCP chain (and the vocoder unless CUs are partitioned)
    hipStream_t stream_voc = nullptr;        // vocoder + hand-off check (== stream)
    hipEvent_t ev_mlpg_done = nullptr, ev_voc_done = nullptr;
    hipStream_t stream_lf0 = nullptr, stream_lpf = nullptr; // concurrent parameter-generation chains
    hipEvent_t ev_fork = nullptr, ev_lf0 = nullptr, ev_lpf = nullptr, ev_prep = nullptr, ev_build = nullptr, ev_mcpbuild = nullptr, ev_ivar = nullptr, ev_fb = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    std::vector<uint32_t> T;
    std::vector<uint64_t> frame_off;
    uint64_t sumT = 0;
    uint32_t maxT = 0;
    size_t total_samples = 0;
    size_t bytes_alloc = 0, bytes_input = 0;
    BatchDev bd{};
    StreamDev sd[kMaxStream]{};
    VocDev vd{};
    std::shared_ptr<NoiseDev> noise;         // vd.noise points into it
    // vocoder work items
    std::vector<VocWork> work;       // host copy
    VocWork *work_dev = nullptr;
    uint32_t n_items = 0, chunk_frames = 0, warmup_frames = 0, n_redo = 0;
    double verify_tol = 1e-9;
    double *end_state = nullptr, *warm_state = nullptr;
    double *ckpt_state = nullptr, *tmp_state = nullptr; // partial redo: checkpoints / recomputed states
    double *ckpt2_state = nullptr, *tmp2_state = nullptr; // the same for the second checkpoint of long chunks
    const double **pairs_dev = nullptr;
    uint32_t n_redo_partial = 0, n_redo_full = 0;   // of the last run: settled at the checkpoint / redone to the end
    uint32_t n_recert_failed = 0;                   // successors of fully redone chunks that failed re-certification
    size_t state_stride = 0;
    uint8_t *bad_dev = nullptr;
    uint32_t *nbad_dev = nullptr;
    bool verify_pending = false;
    std::vector<uint8_t> first_of_kind; // [B] 1: no earlier utterance of the batch was made from the same arrays
    bool invariant = false;          // JB_BATCH_INVARIANT without JB_BATCH_SERIAL: geometry from each utterance alone
    bool lp_mode = false;            // lane-triple throughput kernel
    int lt_waves_per_simd = 2;       // its waves per SIMD: 2 (eight-wave workgroups) or 1 (build_work)
    uint32_t *order_dev = nullptr;   // its launch permutation
    uint32_t n_slots = 0;            // ... and its length: n_items, plus the padding of condition classes (build_work)
    // per-utterance vocoder conditions (jb_batch_create_voc): the host copy of vd.uvoc -- empty when every utterance
    // has the same, which then stands in vd.alpha / volume / beta / beta_stage -- and each utterance's condition
    // class: utterances with equal (alpha, volume), numbered in order of first appearance
    std::vector<VocUtt> uvoc;
    std::vector<uint32_t> voc_class;
    uint32_t n_classes = 1;
    VocWork *redo_dev = nullptr;
    VocWork *gen_work_dev = nullptr; // one item per frame of utterance 0 (streaming generator)
    std::vector<std::pair<void *, size_t>> allocs; // device blocks (pointer, pooled size)
    std::map<std::pair<const void *, size_t>, const void *> uploaded;
    // PINNED staging chunks of the upload arena, kept in a process-wide list between batches (a chunk allocated
    // with new[] for every batch made the arena's H2D copy a pageable one of fresh pages: 14 ms of a 28 ms
    // creation when sub-batches of a job are created one after the other)
    struct PinnedChunk { // staging buffer of an upload arena: pinned if the host grants it, else pageable
        uint8_t *p = nullptr;
        bool pageable = false;
        PinnedChunk() = default;
        PinnedChunk(const PinnedChunk &) = delete;
        PinnedChunk &operator=(const PinnedChunk &) = delete;
        PinnedChunk(PinnedChunk &&o) noexcept : p(o.p), pageable(o.pageable) { o.p = nullptr; }
        PinnedChunk &operator=(PinnedChunk &&o) noexcept
        {
            reset();
            p = o.p;
            pageable = o.pageable;
            o.p = nullptr;
            return *this;
        }
        ~PinnedChunk() { reset(); }
        bool acquire(size_t bytes);
        void reset();
        uint8_t *get() const { return p; }
    };
    struct UploadChunk { // arena for small input arrays: one H2D copy per chunk
        uint8_t *dev = nullptr;
        PinnedChunk host;
        size_t used = 0, sent = 0;
    };
    std::vector<UploadChunk> up_chunks;
    int flush_uploads();

    ~Batch();
    int dalloc_bytes(void **p, size_t bytes, bool zero); // a pool block the batch owns until it is destroyed
    template <class T> int dalloc(T **p, size_t n, bool zero) // n elements (0: one)
    {
        void *v = nullptr;
        const int rc = dalloc_bytes(&v, (n ? n : 1) * sizeof(T), zero);
        *p = (T *)v;
        return rc;
    }
    // v into a block of the batch, synchronously (beside dalloc: what RatePass::bind stores through)
    template <class T> int put(T *dst, const std::vector<T> &v, const char *what) { return upload_list(dst, v, what); }
    // blocks that must start out zeroed: cleared by ONE launch when the batch has been put together (flush_zero),
    // not by a fill of its own each -- two dozen 5 us launches were 0.13 ms of the 2.4 ms of a one-sentence request
    std::vector<std::pair<void *, size_t>> zero_list;
    int flush_zero();
    int upload(const void *host, size_t bytes, const void **dev);
    // the same arena without the de-duplication: for descriptor arrays put together in temporaries of create() (a
    // synchronous hipMemcpy of its own each -- nine of them -- was 0.2 ms of a one-sentence request); the bytes reach
    // the device with the next flush_uploads()
    template <class T> int stage(const T *host, size_t n, T **dev);
    bool from_tracks = false;        // created from parameter tracks: run() starts at the frame prologue
    bool gang_check_pending = false; // a resident GV kernel has been enqueued since its error flag was last read
    // the resident GV kernel of the pending run gave up in formation (flag read, not cleared: sync() acts on it);
    // the caller has waited for ev_mlpg_done
    int gang_timeout_seen(bool *seen);
    double *gen_pcm = nullptr;       // PCM of the streaming generator's serially served frames (its own buffer)
    OutputChain out{*this};          // the stages behind the vocoder: rate, filter, loudness, join, the encoders
    bool last_run_timed = false;
    uint32_t gang_fallbacks = 0;     // times the resident GV kernel timed out in formation and the sweeps took over
    static int create(const jb_voice_desc *voice, const jb_state_utt *utts, size_t n,
                      const jb_batch_opts *opts, Batch **out, const IndexSrc *idx = nullptr,
                      const TrackSrc *trk = nullptr, const jb_utt_voc *voc = nullptr);
    int enqueue_mlpg_only();
    int enqueue_from_tracks();
    int gather_states(const jb_voice_desc *voice, const IndexSrc &idx, size_t n,
                      std::vector<StreamStatesDev> &out); // [n * nstream]: mean/var/msd filled
    int build_work(const jb_batch_opts *opts);
    int build_generator_work();
    int enqueue_paramgen();
    int enqueue_vocoder();
    int finish_verify();
    int run(bool timed);
    int sync();
    int read(const void *dev, void *dst, size_t bytes, bool do_sync = true); // do_sync: wait for the batch's streams + certification first
    // whole PCM slab -> one host buffer per utterance (dst[u] may be null for empty utterances);
    // elem = 8 (f64) or 2 (JB_BATCH_PCM_I16)
    int read_pcm_split(void *const *dst, size_t elem);
};

} // namespace jb

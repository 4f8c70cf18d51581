#pragma once
// jb_output.h -- the routing of the stages behind the vocoder, in their order: converter (output rate), filter,
// loudness (measurement, groups, report, apply pass), join, then the encoders side by side: FLAC, sample format, IMA
// ADPCM, filterbank features, cepstral features, mel spectrograms.  plan_output (jb_output.cpp) decides from the batch's shape and the requests alone which slab each stage
// reads and writes, in f64 or in 16 bits, which slab the read entries hand out, each utterance's output geometry and
// its place in the encoders' byte slabs, and with a join request (jb_join.h) or a mix request (jb_mix.h) the programmes:
// their numbering, each one's place in the join slab, each member's start, and the encoders' geometry by programme
// instead of by utterance.
// The loudness groups' bookkeeping is here too, and what a redo round runs again: the three masks the stages follow
// (redo_scope) and the renumbering of the items a mask picks (pick_renumbered).
// Plain C++17 without HIP: all of it is made and tested on any host; OutputChain (jb_host.h) carries it out.
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "jb_activity.h"
#include "jb_fbank.h"
#include "jb_mfcc.h"
#include "jb_melspec.h"
#include "jb_pitch.h"
#include "jb_join.h"
#include "jb_mix.h"

namespace jb {

// The PCM slabs of a batch, by name.  The first two are made with the batch (one of them: by JB_BATCH_PCM_I16);
// the others are allocated at the first run where the plan lists them
enum class OutSlab : uint8_t {
    None,
    V64,     // the vocoder's f64 slab of the batch as created
    S16,     // the 16-bit slab of the batch as created
    Voc64,   // f64 the vocoder of a 16-bit batch writes for a stage that reads f64
    Conv64,  // f64 the converter writes
    Apply64, // f64 the loudness apply pass writes
    New16,   // 16-bit output longer than S16
    Fmt,     // bytes the format stage writes
    Adpcm,   // IMA ADPCM blocks
    Join64,  // f64 the join stage writes: the programmes
    Join16,  // the same in 16 bits
    Filt64,  // f64 the filter stage writes
    Feat,    // bytes of the filterbank features
    MfccL,   // f64 log-mel frames the cepstral stage makes for itself
    Mfcc,    // bytes of the cepstral features
    Mel,     // bytes of the mel spectrograms
    MelY,    // f64 values the mel stage holds in front of its range clamp (with a range only)
    Count
};
constexpr size_t out_slab_elem(OutSlab s) // bytes
{
    return s == OutSlab::Fmt || s == OutSlab::Adpcm || s == OutSlab::Feat || s == OutSlab::Mfcc || s == OutSlab::Mel ? 1
           : s == OutSlab::S16 || s == OutSlab::New16 || s == OutSlab::Join16 ? 2
                                                                               : 8;
}

// in_hz -> out_hz reduced by their gcd (rates above 0)
void resample_ratio(uint32_t in_hz, uint32_t out_hz, uint64_t *L, uint64_t *M);
uint64_t resample_out_len(uint64_t n_in, uint64_t L, uint64_t M); // ceil(n_in L / M)

// What the plan reads, as plain values
struct OutPlanIn {
    size_t B = 0;
    const uint64_t *n_native = nullptr;   // [B] samples of each utterance at the voice's rate
    const uint64_t *off_native = nullptr; // [B] its first sample in the native slab
    uint32_t voice_hz = 0;
    bool i16 = false;                     // JB_BATCH_PCM_I16
    const uint32_t *want_hz = nullptr;    // [B] requested rate, 0 or voice_hz = native; nullptr: none requested
    bool loudness = false, flac = false;
    uint32_t fmt_bytes = 0;               // bytes per sample of the requested sample format; 0: none requested
    bool adpcm = false;                   // IMA ADPCM is requested
    uint32_t adpcm_align = 0;             // its block_align: 0 = by each utterance's output rate (jb_adpcm.h)
    const uint32_t *stem_of = nullptr;    // [B] the stems request behind a mix's (jb_mix.h "Stems"); nullptr: none
    const MixUtt *mix = nullptr;          // [B] the programme request in the mix's words (jb_mix.h): a mix's, or with
    bool chained = false;                 // `chained` a join's as join_as_mix words it; nullptr: none
    const JoinUtt *join = nullptr;        // [B] a join request in its own words (jb_join.h), as the host probes give
                                          // it: the plan words it with join_as_mix itself, in front of `mix`
    const uint8_t *filter = nullptr;      // [B] 1 = the utterance's filter has at least one section; nullptr: no request
    const FbankOpts *fbank = nullptr;     // the filterbank request (jb_fbank.h), checked at every output rate; nullptr: none
    const FbankOpts *mfcc_fbank = nullptr; // the cepstral request (jb_mfcc.h): its filterbank's geometry (the stage forces
    const MfccOpts *mfcc = nullptr;        // f64 logarithms itself) and its options; both or neither
    const FrameOpts *frame = nullptr;      // the frame request beside the fbank and mfcc ones (JB_FRAME_REFLECT: their T); nullptr: none
    const MelOpts *melspec = nullptr;      // the mel spectrogram request (jb_melspec.h), checked at every output rate; nullptr: none
    const PitchOpts *pitch = nullptr;      // the pitch request (jb_pitch.h), checked at every output rate; nullptr: none
    const ActOpts *activity = nullptr;     // the speech-activity request (jb_activity.h), checked at every unit's rate; nullptr: none
};

struct OutUtt {
    uint32_t hz, L, M; // output rate = voice_hz L / M
    uint64_t n, off;   // samples and first sample in the slabs behind the converter (the native ones without it)
};

struct OutFmtUtt { // an utterance's place in the format slab
    uint64_t off, bytes; // byte offset (16-byte aligned) and n * bytes per sample
};

struct OutAdpcmUtt { // an utterance's blocks in the ADPCM slab
    uint64_t off, bytes; // byte offset (16-byte aligned) and blocks * A
    uint32_t A;          // its block size
};

struct OutFbankUtt { // a unit's features in the feature slab
    uint64_t off, bytes;     // byte offset (16-byte aligned) and T * n_mels * bytes per element
    uint64_t T;              // its frames
    uint32_t wl, hop, n_fft; // its geometry, by its rate
};

struct OutMfccUtt { // a unit's cepstral rows in the Mfcc slab and its log-mel frames in the MfccL slab
    uint64_t off, bytes; // byte offset (16-byte aligned) and T * width * bytes per element
    uint64_t T;          // its frames
    uint32_t width;      // elements of a row: d (delta_order + 1)
    uint32_t n_fft;      // of its filterbank geometry, by its rate
    uint64_t loff;       // its first log-mel value in the MfccL slab, in doubles (a 16-byte boundary)
};

struct OutMelUtt { // a unit's mel spectrogram in the Mel slab and, with a range, its f64 values in the MelY slab
    uint64_t off, bytes; // byte offset (16-byte aligned) and T * n_mels * bytes per element
    uint64_t T;          // its frames
    uint32_t n_fft, hop; // its geometry (in samples: the same at every rate)
    uint64_t yoff;       // its first value in the MelY slab, in doubles (a 16-byte boundary); 0 without a range
};

struct OutPitchUtt { // a unit's pitch rows in the stage's byte block and its 4 kHz signal in its f64 block
    uint64_t off, bytes; // byte offset (16-byte aligned) and T * width * bytes per element
    uint64_t T;          // its frames: the fbank stage's under the same window, hop and grid
    uint32_t width, elem; // elements of a row and bytes of an element
    uint64_t n4, yoff;   // its samples at 4 kHz and the first one's place in the f64 block, in doubles (a 16-byte boundary)
};

struct OutUnit { // a programme in the join slab: what the encoders behind a join take for an utterance
    uint32_t hz;
    uint64_t n, off; // samples and first sample in the join slab (a 16-byte boundary)
};

struct OutWrite { // what a stage writes; slab None: the stage does not run
    OutSlab slab = OutSlab::None;
    bool i16 = false;
};

struct OutPlan {
    std::vector<OutUtt> utt;  // [B]
    uint64_t total = 0;       // samples of the slabs behind the converter
    uint64_t native_total = 0;
    bool convert = false;     // some utterance is not native; the native ones then go through the identity table
    OutWrite vocoder, converter, apply;
    // The filter stage (jb_filter.h): behind the converter (or the vocoder), in front of the measurement; it reads the
    // f64 of the stage in front (filter_src) and every stage behind it reads what it writes.  None: no utterance of
    // the request has a section
    OutWrite filter;
    OutSlab filter_src = OutSlab::None;
    OutSlab measure = OutSlab::None;  // f64 the loudness measurement reads (never scaled in place)
    OutSlab flac = OutSlab::None;     // 16 bits FLAC encodes: the slab handed out
    OutWrite final;                   // what the PCM read entries hand out
    OutSlab native64 = OutSlab::None; // f64 at the voice's rate (jb_batch_read_pcm_native)
    OutSlab fmt_src = OutSlab::None;  // f64 the format stage reads: what `final` names (None: no format, or no f64)
    std::vector<OutFmtUtt> fmt;       // [B] with a format stage, else empty
    OutWrite adpcm_src;               // what the ADPCM stage reads: what `final` names, f64 or 16-bit (None: no ADPCM)
    std::vector<OutAdpcmUtt> adpcm;   // [B] with an ADPCM stage, else empty
    OutSlab fbank_src = OutSlab::None; // f64 the fbank stage reads: what `final` names (None: no request, or no f64)
    std::vector<OutFbankUtt> fbank;    // [B] with an fbank stage, else empty
    OutSlab mfcc_src = OutSlab::None;  // f64 the cepstral stage reads: what fbank_src would name (None: no request)
    std::vector<OutMfccUtt> mfcc;      // [B] with a cepstral stage, else empty
    OutSlab melspec_src = OutSlab::None; // f64 the mel stage reads: what fbank_src would name (None: no request)
    std::vector<OutMelUtt> melspec;      // [B] with a mel stage, else empty
    OutSlab pitch_src = OutSlab::None;   // f64 the pitch stage reads: what fbank_src would name (None: no request)
    std::vector<OutPitchUtt> pitch;      // [B] with a pitch stage, else empty ([P], or [P + S] with stems, behind a join or mix)
    uint64_t pitch_bytes = 0, pitch_words = 0; // the stage's two blocks: the rows' bytes and the 4 kHz signals' doubles
                                         // (blocks of the stage's own, as the activity stage's are: not slabs of `alloc`)
    // With a join request: the stage reads what `final` names and writes the programmes to a slab of its own; flac,
    // fmt_src, adpcm_src, fbank_src, mfcc_src and melspec_src then name that slab, and fmt, adpcm, fbank, mfcc and melspec have [P] entries laid
    // out from `units`
    OutWrite join_src, join;          // None: neither a join nor a mix
    bool mixed = false;               // the programmes are a mix request's: sums of their members (jb_mix.h)
    std::vector<uint32_t> mix_depth;  // [P] with a mix: the largest number of unmuted members over one sample
    std::vector<uint64_t> mix_overlap; // [P] with a mix: the samples under two or more unmuted members
    std::vector<OutUnit> units;       // [P] the programmes; with a stems request [P + S]: the stems behind them, units
                                      // like any other to the encoders (mix_depth and mix_overlap run over them too)
    size_t n_progs = 0;               // P
    std::vector<MixStem> stems;       // [S] with a stems request
    std::vector<int32_t> stem_unit;   // [B] with a stems request: the unit of each utterance's stem, or -1
    std::vector<uint32_t> unit_parent; // [S] the programme of each stem (redo_scope's)
    std::vector<uint32_t> prog_of;    // [B] each utterance's programme
    std::vector<uint64_t> prog_start; // [B] its first sample within it
    std::vector<uint32_t> prog_first, prog_members; // programme p owns prog_members[prog_first[p] .. prog_first[p + 1])
    // With a speech-activity request (jb_activity.h), a side output beside the encoders: with JB_ACTIVITY_MEMBERS the
    // stage reads the members where the join reads them (join_src: what `final` names), with JB_ACTIVITY_UNIT the
    // units where the encoders read them (the join slab, or `final`); f64 or 16 bits.  act: each unit's place in the
    // label bytes with its T, C, wl and hop, each column's source, frames and place in the compact energy scratch, and
    // the three blocks' sizes (act.bytes, act.energies, act.words: the stage's own blocks, not slabs of `alloc`)
    OutWrite act_src;                 // None: no request (or one that some unit refuses: the chain has checked it)
    ActLayout act;
    const char *act_fault = nullptr;  // what act_layout refused of the request, its unit and whether a cap was passed
    size_t act_fault_unit = 0;
    bool act_unsupported = false;
    std::vector<double> prog_gain;    // [B] with a mix: mix_gain of each member (0: muted)
    uint64_t alloc[(size_t)OutSlab::Count] = {}; // elements to allocate of each slab, at least 1 (0: none; V64 / S16 exist)
    bool normalize() const { return apply.slab != OutSlab::None; }
    bool filtered() const { return filter.slab != OutSlab::None; }
    bool active() const { return convert || normalize() || filtered(); } // a stage rewrites the PCM behind the vocoder
};

// Pure: no globals, no environment.
OutPlan plan_output(const OutPlanIn &in);

// Loudness groups (jb_batch_set_loudness_groups): one measurement and one gain for the members of a group.
constexpr uint32_t kLnNoGroup = 0xffffffffu; // JB_LOUDNESS_NO_GROUP: the utterance is a group of its own

// What the group bookkeeping reads.  An entry of `group` is a caller's id below B or kLnNoGroup
struct LnGroupsIn {
    size_t B = 0;
    const uint32_t *group = nullptr;  // [B]
    const double *target = nullptr;   // [B] (NaN: measured only); nullptr: no target set yet, nothing to compare
    const double *ceiling = nullptr;  // [B], with target
    const uint32_t *mode = nullptr;   // [B] JB_PEAK_*; nullptr: the sample peak everywhere
    const uint32_t *hz = nullptr;     // [B] output rate
};

// Groups numbered densely in the order of their first member (an ungrouped utterance: a group of one, numbered the
// same way); group g owns members[first[g] .. first[g + 1]), ascending utterance indices
struct LnGroups {
    std::vector<uint32_t> group_of; // [B]
    std::vector<uint32_t> first;    // [G + 1]
    std::vector<uint32_t> members;  // [B]
    size_t size() const { return first.empty() ? 0 : first.size() - 1; }
};

// Pure.  false: the request is refused; *bad_group is the caller's id of the first offending group (kLnNoGroup for
// an entry that is no id) and *bad_field names what its members disagree on ("target", "ceiling", "peak mode",
// "output rate") or says "group id" for an id of B or above.  Two NaN targets agree
bool plan_loudness_groups(const LnGroupsIn &in, LnGroups *out, uint32_t *bad_group, const char **bad_field);

// The redo closure.  touched: [B] 1 = an utterance a redo round rewrote.  groups: [G] 1 = a group with a touched
// member; members: [B] 1 = a member of such a group (a superset of touched)
void loudness_groups_closure(const LnGroups &g, const std::vector<uint8_t> &touched, std::vector<uint8_t> *groups,
                             std::vector<uint8_t> *members);

// A join request (jb_join.h) in the mix's words, all but the starts: 0 dB, the fades, pad_after and the reserved word
// carried over, and `start` holding pad_before -- counted from where the member in front ends with its pad_after,
// which the layout alone knows.  mix_layout takes it with `chained` and leaves in `start` the starts the request means:
// a join is the mix whose members follow each other, so its depth is at most 1 and its overlap 0
std::vector<MixUtt> join_as_mix(const JoinUtt *req, size_t B);

// The programme request laid out, a mix's (jb_mix.h) or a join's (join_as_mix, `chained`): programmes numbered densely
// in the order of their first member, as the loudness groups are (an utterance of kMixNone: a programme of one), their
// members in ascending utterance index; a member starts where its request says (`chained`: that far behind the end of
// the member in front), a programme's length is the largest start + n + pad_after of its members, and each programme
// starts on a 16-byte boundary of a slab of `elem`-byte samples.  The work lists follow from the geometry alone: each
// programme cut at every start and end of an unmuted member (gain[u] != 0) of at least one sample into segments under
// a constant set of members, each segment's set listed once in ascending utterance index
struct MixLayout {
    LnGroups progs;              // group_of: [B] the programme of each utterance; first / members: [P + 1] / [B]
    std::vector<OutUnit> units;  // [P]
    std::vector<uint64_t> start; // [B] each member's first sample within its programme
    uint64_t total = 0;          // samples of the slab
    std::vector<double> gain;    // [B] mix_gain of each request
    std::vector<uint32_t> seg_first; // [P + 1] programme p owns segs[seg_first[p] .. seg_first[p + 1])
    std::vector<MixSeg> segs;        // (a programme of no samples: none)
    std::vector<uint32_t> lists;     // the segments' members: places in progs.members
    std::vector<uint32_t> depth;     // [P] the longest list of the programme
    std::vector<uint64_t> overlap;   // [P] its samples in segments of two or more
    // With a stems request (stem_of; jb_mix.h "Stems"): the stems are units P .. P + S - 1 behind the programmes, by
    // programme in dense order and within one by the ascending utterance index of each stem's first member; a stem is
    // laid out as what it is, a unit of its programme's length and rate on a 16-byte boundary of the same slab with
    // segments and lists of its own over its subset (places in progs.members, as the programmes').  units, seg_first,
    // depth and overlap then run over the P + S units; progs stays the programmes'.  Without a request: all empty
    std::vector<MixStem> stems;     // [S]
    std::vector<int32_t> stem_unit; // [B] the unit of each utterance's stem, -1: none; empty without a request
    size_t programmes() const { return progs.size(); }
};
// Pure.  n: [B] each utterance's samples; hz: [B] its output rate (nullptr: not compared, the units' rate is 0).
// false: the request is refused; *bad is the caller's id of the offending programme (for "length" and "work lists":
// the utterance or the dense programme) and *field says "programme id" for an id of B or above, "output rate" where
// its members disagree, "length" where an utterance's start + n + pad_after passes 2^63, "slab length" where the
// programmes up to the dense programme *bad pass it together, or "work lists" where the lists pass kMixMaxList entries.
// stem_of: [B] each utterance's stem id within its programme, or kMixNoStem; nullptr: no stems.  "stem id": the
// utterance *bad carries an id of B or above; "slab length" and "work lists" then name a unit, programme or stem
bool mix_layout(const MixUtt *req, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem, MixLayout *out,
                uint32_t *bad, const char **field, bool chained = false, const uint32_t *stem_of = nullptr);
// The same from a join request in its own words (the host probes' way in): mix_layout of join_as_mix, chained
using JoinLayout = MixLayout;
bool join_layout(const JoinUtt *req, const uint64_t *n, const uint32_t *hz, size_t B, size_t elem, JoinLayout *out,
                 uint32_t *bad, const char **field);

// The redo closure behind the join.  post: [B] 1 = an utterance whose final PCM changed (behind
// loudness_groups_closure); programmes: [P] 1 = a programme with such a member.  unit_parent: the programme of every
// unit behind the P programmes (a mix's stems; empty: none): programmes then has P + S entries, and a touched
// programme touches its stems (they and their levels run again whole)
void join_closure(const std::vector<uint32_t> &prog_of, size_t P, const std::vector<uint8_t> &post,
                  std::vector<uint8_t> *programmes, const std::vector<uint32_t> &unit_parent = {});

// What a redo round runs again, from the utterances it rewrote.  Each stage of the chain follows one of the masks
struct RedoScope {
    std::vector<uint8_t> measured;       // [B] = only: converter, filter, measurement, per-utterance report sets
    std::vector<uint8_t> post;           // [B] the members of every touched group (= only without groups): behind the
                                         // apply pass a group's gain reaches every member; the join spans
    std::vector<uint8_t> units;          // [P] the programmes of `post` (= post, [B], without a join): the encoders
    std::vector<uint8_t> touched_groups; // [G] a group with a member in `only` (empty without groups)
};
// Pure: loudness_groups_closure, then join_closure.  prog_of: [B] each utterance's programme of P (empty: no join);
// groups: the loudness groups the chain runs (empty: none); only: [B] 1 = an utterance the round rewrote
RedoScope redo_scope(const std::vector<uint32_t> &prog_of, size_t P, const LnGroups &groups,
                     const std::vector<uint8_t> &only, const std::vector<uint32_t> &unit_parent = {});

// The items a mask picks, renumbered: a redo launch packs their tiles (or groups, or blocks) from 0, while their
// scratch stays where the full run's numbering put it.  An item of count 0 is picked like any other
struct Picked {
    std::vector<uint32_t> index; // the picked items, ascending
    std::vector<uint64_t> base;  // the sum of the counts of the picked items in front of each
    uint64_t total = 0;
};
// Pure.  mask, count: one entry per item
Picked pick_renumbered(const std::vector<uint8_t> &mask, const std::vector<uint64_t> &count);

} // namespace jb

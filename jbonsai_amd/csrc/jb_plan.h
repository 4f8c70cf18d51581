#pragma once
// jb_plan.h -- the vocoder's work geometry: chunk length, warm-up, checkpoints, kernel and waves per SIMD, the work
// items and the lane kernel's launch order, decided from the batch's shape alone (plan_vocoder_work, jb_plan.cpp).
// Below it, the rules of the redo rounds that follow a failed hand-off check (Batch::finish_verify) and the shape
// rules of Batch::create: frame blocks, the voiced runs of an LF0 track, the vocoder conditions and
// each stream's MLPG mode.  Plain C++17 without HIP: the planners run and are tested on any host; the kernels read the
// constants below too.
#include "../../include/jbonsai_amd.h"

#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace jb {

// The code an order runs on: its own for nitech's two (35, 25: the EXACT instantiations), else the next of
// {25, 31, 35} as lane triples or of {41, 51, 61} with one stage per lane, the taps above the voice's own at coefficient
// zero (an order-39 voice pays for 40 taps, an order-49 voice for 50).  Orders below 6 stay with the wave kernels.
constexpr int lt_code_nm(int nmcp)
{
    return nmcp <= 25 ? 25 : nmcp <= 31 ? 31 : nmcp <= 35 ? 35
         : nmcp <= 41 ? 41 : nmcp <= 51 ? 51 : nmcp <= 61 ? 61 : 0;
}
constexpr int lt_chunks(int lpc) { return lpc == 3 ? 21 : 12; } // chunks per wave
constexpr bool vocoder_ls_supported(int nmcp) { return nmcp >= 7 && lt_code_nm(nmcp) != 0; }
// 21 (lane triples: orders up to 34) or 12 (one stage per lane)
constexpr int vocoder_ls_chunks_per_wave(int nmcp) { return lt_chunks(lt_code_nm(nmcp) <= 35 ? 3 : 5); }
constexpr uint32_t kLtNoItem = 0xffffffffu; // a slot of the launch permutation without a chunk (class padding)

// A failing chunk is first recomputed only up to VocDev::ckpt_frames frames past its start; if the
// recomputed state meets the checkpoint the original chunk left there, the rest of the chunk stands.
// 48 frames into chunks of 96 frames and more, 24 into chunks of 36 to 95, 16 into chunks of 24 to 35, none below
// (plan_vocoder_work).  A redo round lasts as long as the frames to the checkpoint (0.06 ms per frame, one wave per
// chunk) and ALL of a round's chunks wait for the one that goes furthest.  A hand-off that failed behind 18 frames
// of warm-up settles at the checkpoint if 18 + 48 frames from zero state are enough.  Tried in round 4: 32 frames
// (-1 ms per round) -- but about 1 % of the failing hand-offs have not converged there, and a batch of 512 or 1024
// distinct utterances (BASELINE configs 3 to 5: ~300 failing hand-offs) then nearly always has one and pays the
// second stage: 2.0 + 3.0 ms instead of 2.9 (profiles/r04_ckpt_sweep.txt: 1024 x 6,386 frames 86.6 / 86.3 / 83.9 /
// 84.6 ms per step with the first checkpoint at 32 / 40 / 48 / 56).
// Chunks of 144 frames and more leave a SECOND checkpoint 96 frames in: the rare chunk that has not converged at
// the first one is recomputed 48 frames further and compared again, instead of to its end (105 frames = 6.4 ms).
constexpr uint32_t kVocCkptFrames = 48, kVocCkptFramesShort = 24, kVocCkptFramesTiny = 16, kVocCkpt2Frames = 96;

// What the plan reads: the batch's shape and the caller's options, as plain values.
struct VocPlanIn {
    const uint32_t *T = nullptr;            // [B] frames of each utterance (zeros allowed)
    size_t B = 0;
    const uint8_t *first_of_kind = nullptr; // [B] 1: no earlier utterance is a copy of this one; nullptr: all distinct
    const uint32_t *voc_class = nullptr;    // [B] condition class of each utterance; nullptr: one class
    int nmcp = 0, fperiod = 0, stage = 0;   // the voice's vocoder
    uint32_t flags = 0;                     // JB_BATCH_* of the batch
    uint32_t chunk_frames = 0, warmup_frames = 0; // jb_batch_opts: 0 = the library's choice
};

// VocPlanItem::saves: the states a chunk leaves for the hand-off check and the partial redo
enum : uint8_t { kSaveEnd = 1, kSaveWarm = 2, kSaveCkpt = 4, kSaveCkpt2 = 8 };

struct VocPlanItem {
    uint32_t utt, t_start, t_out, t_end; // as VocWork: warm-up from t_start, output [t_out, t_end)
    uint8_t saves;                       // kSave* bits
};

struct VocPlan {
    bool lane_kernel = false;    // k_vocoder_lt (else the wave kernel k_vocoder)
    int waves_per_simd = 2;      // the lane kernel's: 1 (four-wave workgroups) or 2 (eight-wave)
    uint32_t chunk_frames = 0;   // 0: serial (one item per utterance); JB_BATCH_INVARIANT: the longest of the batch
    uint32_t warmup_frames = 0;
    uint32_t ckpt_frames = 0, ckpt2_frames = 0; // VocDev::ckpt_frames / ckpt2_frames
    std::vector<VocPlanItem> items;
    std::vector<uint32_t> order; // the lane kernel's launch permutation of items, kLtNoItem slots included
};

// Pure: no globals, no environment.
VocPlan plan_vocoder_work(const VocPlanIn &in);

// ---- the redo rounds of the hand-off check (Batch::finish_verify) ----
// Which failing chunks a round recomputes, how far, and what the recomputations are worth once their states have been
// compared: rules over chunk indices alone.  They read each item's utt and kSave* bits, the flags below ([n items]
// each, 0 / 1) and nothing else; the driver does the device round trips between them.  Each pure.

// This round: `ids` (increasing) and the same as flags.  pending[0] must be 0: chunk 0 has no hand-off
struct RedoPick {
    std::vector<uint32_t> ids;
    std::vector<uint8_t> in_round;
};
RedoPick redo_pick_round(const std::vector<VocPlanItem> &items, const std::vector<uint8_t> &pending);

// Stage A: a chunk with a checkpoint goes up to it, every other one to its end -- speculatively (spec_end) where its
// successor is in the round too, of the same utterance, and starts from the end state this chunk leaves
struct RedoStageA {
    std::vector<uint32_t> part;    // positions in ids whose recomputed state is compared: with a checkpoint, or spec_end
    std::vector<uint8_t> spec_end; // recomputed to the end into a scratch dump, compared with the first pass's end state
};
RedoStageA redo_stage_a(const std::vector<VocPlanItem> &items, const RedoPick &pick);

// Second checkpoint: the chunks of the round that had not converged at the first one and have a second to go on to
std::vector<uint32_t> redo_second_checkpoint(const std::vector<VocPlanItem> &items, const std::vector<uint32_t> &ids,
                                             const std::vector<uint8_t> &unsettled, bool ckpt2);

// In chunk order: what the round's recomputations are worth.  unsettled: the chunk's last comparison failed (at the
// second checkpoint for those that went on to it); pending: as the round was picked from
struct RedoSettled {
    std::vector<uint8_t> final_now; // valid recomputations: no longer pending after this round
    std::vector<uint32_t> rest;     // stage B: final chunks that go on to their end from the checkpoint they were last
                                    // compared at
    std::vector<uint32_t> full_ids; // final chunks recomputed to their end in this round
    uint32_t n_partial = 0, n_full = 0; // final chunks settled at a checkpoint / recomputed to the end
};
RedoSettled redo_settle(const std::vector<VocPlanItem> &items, const RedoPick &pick, const std::vector<uint8_t> &pending,
                        const std::vector<uint8_t> &spec_end, const std::vector<uint8_t> &unsettled);

// Re-certification: the successors of full_ids whose hand-off is compared again.  pending: after the round
std::vector<uint32_t> redo_recertify(const std::vector<VocPlanItem> &items, const std::vector<uint32_t> &full_ids,
                                     const std::vector<uint8_t> &in_round, const std::vector<uint8_t> &pending);

// ---- the shape rules of Batch::create (each pure: plain values in, no globals, no environment) ----

constexpr double kNoData = -1e10; // src/constants.rs:13

// A frame's samples in blocks of bs <= 64 (one pulse-mask word and one wave pass of lane = sample per block).
// The largest divisor of the frame period that is <= 64 where there is a useful one (every BASELINE shape: 240 ->
// 4 x 60; the split excitation kernels and the lane-triple vocoder are built on equal blocks); otherwise -- a
// prime frame period, 75 = 3 x 25 under a 31-tap filter -- blocks of ceil(fperiod / nblk) samples with a shorter
// LAST block (block q = samples [q bs, min(fperiod, (q + 1) bs)): sample i is bit i % bs of word i / bs either way).
struct FrameBlocks {
    int bs, nblk;
};
FrameBlocks plan_frame_blocks(int fperiod, int nlpf);

// Parameter tracks as the source: the runs of voiced / unvoiced frames of an LF0 track (a frame is voiced where
// lf0 != NODATA, vocoder/mod.rs:73-77) as the pseudo-states of the LF0 stream's state walk: durations[k] frames of
// msd[k] = 1 (voiced) or 0, alternating.
void plan_voiced_runs(const double *lf0, size_t n, std::vector<uint32_t> &durations, std::vector<double> &msd);

// Vocoder condition of one utterance (jb_utt_voc after the beta rule below): what VocDev::alpha / volume / beta /
// beta_stage hold for a batch with one condition.  pf: which freqt operator of VocDev::pf_table (beta > 0).
struct VocUtt {
    double alpha, volume, beta, beta_stage;
    uint32_t pf, pad;
};

// The vocoder conditions of a batch.  One for the whole batch -- no jb_utt_voc, or every entry the same -- stands in
// `batch`, and the kernels run as they always have.  Otherwise `utt` holds each utterance's; batch.beta / beta_stage
// are then the maxima over the utterances: they say only whether SOME utterance has a post-filter (what is allocated
// and launched), and the lane kernel's launch permutation keeps the condition classes apart (plan_vocoder_work).
struct VocCondPlan {
    VocUtt batch{};
    bool mixed = false;
    std::vector<VocUtt> utt;        // [n], mixed only (VocDev::uvoc)
    std::vector<uint32_t> cls;      // [n], mixed only: utterances with equal (alpha, volume), by first appearance
    uint32_t n_classes = 1;
    std::vector<double> pf_alphas;  // the alpha of each post-filter operator (VocDev::pf_table): the batch-wide
                                    // condition's first where its beta > 0, then by first appearance among the
                                    // utterances with beta > 0
};
// voice: the voice's own alpha / beta / volume; utt: [n] per-utterance triples, or nullptr.  The beta rule:
// postfilter_mcp acts only for beta > 0, more than two coefficients and stage 0 (cepstrum.rs:24); with stage > 0 beta
// goes to postfilter_lsp (lsp.rs:113-139).
VocCondPlan plan_voc_conditions(const jb_utt_voc &voice, uint32_t nmcp, uint32_t stage, const jb_utt_voc *utt, size_t n);

// "The one-window case": a width-1 window alone, no GV -- the track is the state means (k_mlpg_static), and no MLPG
// workspace is allocated for the stream
constexpr bool mlpg_is_static(int BW, int W, int use_gv, int generic_solver)
{
    return BW == 1 && W == 1 && !use_gv && !generic_solver;
}

// How stream si of a batch is generated: what StreamDev's fields of the same names hold.
struct StreamMode {
    int W, BW;      // windows read; band width = Windows::max_width() * 2 + 1 (window.rs:19-21, mlpg.rs:27)
    int is_msd, use_gv;
    int mt;         // [dim][frame] workspace with the fused kernels
    int defer_out;  // the MCP stream's transpose is fused with mc2b (enqueue_paramgen)
    bool is_static; // mlpg_is_static
};
// flags: JB_BATCH_* of the batch; from_tracks: parameter tracks are the source (no MLPG: the window description is not
// read and may be absent); mt_max_dim: mlpg_mt_max_dim()
StreamMode plan_stream_mode(const jb_stream_desc &s, uint32_t si, uint32_t flags, uint32_t stage, bool from_tracks,
                            int mt_max_dim);

// ---- the groups of an engine request (synthesize_batch_impl, jb_engine.cpp) ----

// The boundaries glo[0 .. ngroups] of the groups a request of n_utts utterances is pipelined in: group g is the
// utterances [glo[g], glo[g + 1]).  Two groups from 8 utterances and 16,000 label lines on, else one; `forced`
// (JB_SYNTH_GROUPS; 0: none) overrides the count, one_batch (a programme, or one gain for the request: both live in one
// batch) makes it one, and there are never more groups than utterances.  The groups split the utterances by label
// count: boundary g is the first utterance whose line_off reaches g / ngroups of the request's lines.
// line_off: [n_utts + 1], not read for n_utts == 0.  Pure
std::vector<size_t> plan_synth_groups(const size_t *line_off, size_t n_utts, int forced, bool one_batch);

} // namespace jb

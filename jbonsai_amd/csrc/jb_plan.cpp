// jb_plan.cpp -- the vocoder's work list (jb_plan.h): serial = one item per utterance; chunked = items of
// chunk_frames output frames that start warmup_frames early from zero state.  Batch::build_work allocates and
// uploads what this decides.  Behind it, the rules of the redo rounds and the shape rules of Batch::create.
#include "jb_plan.h"

#include <algorithm>
#include <numeric>
#include <utility>

namespace jb {
namespace {

// JB_BATCH_INVARIANT: each utterance's own chunk length (the rule is explained in plan_vocoder_work)
uint32_t inv_chunk(uint32_t Ti)
{
    constexpr uint32_t kInvChunks = 96, kInvMin = 16, kInvMax = 153;
    return std::min(std::max((Ti + kInvChunks - 1) / kInvChunks, kInvMin), kInvMax);
}

} // namespace

VocPlan plan_vocoder_work(const VocPlanIn &in)
{
    VocPlan p;
    const bool serial = (in.flags & JB_BATCH_SERIAL) != 0;
    const bool invariant = (in.flags & JB_BATCH_INVARIANT) && !serial;
    uint64_t sumT = 0;
    for (size_t i = 0; i < in.B; i++)
        sumT += in.T[i];
    // chunks of c frames over the batch, and the hand-off positions among them (one per chunk of each DISTINCT
    // utterance: copies pass or fail their hand-offs together)
    auto chunks_at = [&](uint64_t c) {
        uint64_t n = 0;
        for (size_t i = 0; i < in.B; i++)
            n += (in.T[i] + c - 1) / c;
        return n;
    };
    auto positions_at = [&](uint64_t c) {
        uint64_t n = 0;
        for (size_t i = 0; i < in.B; i++)
            if (!in.first_of_kind || in.first_of_kind[i])
                n += (in.T[i] + c - 1) / c;
        return n;
    };
    // 18 frames.  Every frame of warm-up is 0.6 % of the vocoder kernel (0.35 ms on config 2); a failing
    // hand-off costs a redo round (~2.5 ms whatever their number).  Same box, config 2 (copies of one utterance
    // / 64 distinct utterances), ms per step: 20 frames 92.2 / 94.1, 19: 91.2 / 93.3, 18: 90.5 / 93.6,
    // 17: 93.0 / 92.6 (at 17 a hand-off of config 2's own utterance fails in all 256 copies; with distinct
    // utterances a few hundred fail at every length and settle at their checkpoint).  24 -> 20 earlier in the
    // round: vocoder 67.8 -> 66.3 ms, 136 -> 220 failing hand-offs with distinct utterances.
    // Round 4, the other side of that trade: wherever a redo round is certain anyway -- any batch with more than a
    // few hundred DISTINCT hand-off positions has failing ones at every length up to ~40 frames -- a shorter warm-up
    // is cheaper as long as the failing chunks still get a SIMD each in the redo launch (<= 1024): same box, ms per
    // step at 18 / 16 / 14 / 12 frames: 512 mixed lengths 84.5 / 83.8 / 83.2 / 84.7, 1024 x 6,386 distinct 83.5 /
    // 82.6 / 82.3 / 83.5, 64 distinct x 4 copies 82.4 / 81.3 / 80.5 / 82.2, 64 x 2,000 10.9 / 9.6 / 9.2 (at 14:
    // 1.7 % of the hand-offs fail, 720-810 chunks; at 12: 1,400-1,470, two to a SIMD).  Copies of ONE utterance
    // keep 18: their 167 positions fail for all copies or for none, and over the FAMILY of such batches 18 is the
    // cheaper length -- round 5, BASELINE config 2 for the utterances of seeds 0..3, ms per step at 18 / 14 frames, same
    // box: 76.6 / 78.4, 79.5 / 80.5 (three positions fail at 18, seven at 14), 79.3 / 78.3, 76.2 / 78.1; mean 77.9
    // against 78.8 (profiles/r05_seed_sweep_before.txt; two of the four have no failing position at 18, all have at
    // 14).  Decided below, once the chunk length is known: 14 frames from 1000 distinct hand-off positions (the chance
    // that none of them fails at 18 frames is then under 0.1 %), else 18 -- small requests keep the geometry they had.
    auto warmup_at = [&](uint64_t c) -> uint32_t { return positions_at(c) >= 1000 ? 14 : 18; };
    const bool warmup_given = in.warmup_frames != 0;
    p.warmup_frames = warmup_given ? in.warmup_frames : 18;
    uint32_t ch = in.chunk_frames;
    // chunks the lane kernel holds with one wave on every SIMD
    const uint64_t slots1 = 64ull * 16 * (uint64_t)vocoder_ls_chunks_per_wave(in.nmcp);
    // lane-triple throughput kernel: worth it once the batch holds enough frames to give every SIMD two
    // waves of 21 chunks that are long against the warm-up (measured crossover against the wave kernel at
    // one item per SIMD: between 6 and 8 utterances of 25.5 k frames -- 22.4 vs 26.7 ms at 6, 28.5 vs 26.9
    // at 8)
    constexpr uint64_t lp_min = 100000;
    // (the lane-triple kernel walks the samples of a frame two at a time)
    const bool lane_ok = in.stage == 0 && vocoder_ls_supported(in.nmcp) && (in.fperiod & 1) == 0;
    p.lane_kernel = !serial && !(in.flags & JB_BATCH_WAVE_KERNEL) && lane_ok &&
                    (sumT >= lp_min || (in.flags & JB_BATCH_LANE_KERNEL));
    // JB_BATCH_INVARIANT: every choice below that the default makes from the whole batch -- chunk length, warm-up,
    // kernel, its waves per SIMD, checkpoints -- is made from the utterance (and the voice) alone.  Chunks of
    // clamp(ceil(T / 96), 16, 153) frames behind 18 of warm-up: 153 is what config 2 (256 x 25,546 frames) gets by
    // default, so that an utterance of more than 14,592 frames keeps the default's chunk-with-warm-up of 171 frames
    // (12 % of the frames computed twice) and config 2 its work list; shorter utterances get ~96 chunks each, which
    // keeps a batch of a few of them spread over the chip (64 x 2,000 frames: 21-frame chunks, 6,144 items; the
    // default gives that batch 16-frame chunks) at the price of more warm-up where many of them fill it anyway
    // (1024 x 6,386 frames: 67-frame chunks, 27 % of the frames twice against 12 %).  18 frames of warm-up: the
    // default's for batches with few hand-off positions (14 pays only where a redo round is certain anyway, which
    // is a property of the batch).  The lane-triple kernel wherever the voice supports it, in its eight-wave form.
    if (invariant) {
        p.warmup_frames = 18;
        p.lane_kernel = lane_ok;
        p.waves_per_simd = 2;
        ch = 0;
        for (size_t i = 0; i < in.B; i++)
            ch = std::max(ch, inv_chunk(in.T[i])); // (what jb_batch_info reports: the longest of the batch)
    } else if (serial) {
        ch = 0;
    } else if (ch == 0 && p.lane_kernel) {
        // two waves on every SIMD: 8 XCDs x 32 CUs x 4 SIMDs x 2 -- or ONE, while the batch is too small to give
        // every SIMD two waves of chunks that are long against their warm-up.  The launch takes as long as one
        // chunk-with-warm-up at the rate a wave gets: a lone wave issues an instruction every 6-6.7 cycles, one of a
        // pair every 8.9-9.7 (tools/lt_clocks.sh); compare the two at the chunk length each would get (floor below).
        constexpr uint64_t cfloor = 16;
        auto launch_cost = [&](uint64_t slots, double us_per_sample) {
            return (double)(std::max<uint64_t>((sumT + slots - 1) / slots, cfloor) + p.warmup_frames) * us_per_sample;
        };
        // (per sample and wave, measured: 0.90 us alone on a SIMD, 1.39-1.46 us beside a second wave -- 64 x 11,000
        // frames 18.1 ms per step with one wave per SIMD and 33-frame chunks, 19.8 with two and 17-frame chunks)
        // (the warm-up the chunks will get -- 14 frames from 1000 distinct hand-off positions, decided for good
        // below -- enters the comparison: estimated here from the chunk length two waves per SIMD would give)
        if (!warmup_given)
            p.warmup_frames = warmup_at(std::max<uint64_t>((sumT + 2 * slots1 - 1) / (2 * slots1), cfloor));
        p.waves_per_simd = launch_cost(slots1, 0.90) < launch_cost(2 * slots1, 1.42) ? 1 : 2;
        const uint64_t target = slots1 * (uint64_t)p.waves_per_simd;
        uint64_t c = (sumT + target - 1) / target;
        // while the batch cannot fill the chip the time of the launch is that of ONE chunk (chunk +
        // warm-up frames): chunks down to 16 frames.  Shorter chunks mean more hand-off positions and
        // more of them failing the check, but a failed 16-frame chunk is also redone in a third of the
        // time of a 48-frame one; with DISTINCT utterances (bench.py --distinct 32) 16 beats the earlier
        // floor of twice the warm-up on every shape tried -- 32 x 25,546 frames 59.0 -> 43.0 ms per
        // step, 64 x 4,600 32.7 -> 23.0, 256 x 2,000 33.4 -> 23.5, 1024 x 500 22.8 -> 21.0 -- and 12 or
        // 8 gain nothing more.  (The earlier floor had been tuned on copies of one utterance, whose
        // hand-offs all pass.)
        constexpr uint64_t cmin = cfloor;
        ch = (uint32_t)std::max<uint64_t>(c, cmin);
        // (no rounding of the chunk length: 153 frames instead of 156 on config 2 is 1.7 % fewer frames per
        // chunk-with-warm-up and still fits the chip -- 42,752 items for 43,008 slots)
        // every utterance rounds its chunk count up: with ragged lengths the items can exceed the two
        // waves per SIMD the target stands for, and the waves over the limit run as a tail after the
        // others -- lengthen the chunks until the items fit
        for (int guard = 0; guard < 256 && c >= cmin && chunks_at(ch) > target; guard++)
            ch += 1;
        // (still more items than one wave per SIMD holds: the second wave takes them rather than a tail launch)
        if (p.waves_per_simd == 1 && chunks_at(ch) > slots1)
            p.waves_per_simd = 2;
    } else if (ch == 0) {
        // auto (wave kernel): one item per SIMD, two once the batch is large.  The launch takes as long
        // as ONE item (warm-up + chunk frames at 0.25 us per sample; 0.47 with two items on a SIMD), so a
        // small batch wants short chunks -- down to 16 frames (one 1.4 s sentence: 24.7 -> 17.5 ms per
        // call; below 16 the extra hand-off positions and their occasional redo round cost more than
        // they save) -- but never more items than SIMDs: the kernel's four-wave workgroups are what puts
        // exactly one on each.  (64 x 2000 frames: 16.0 ms with 1344 items of 96 frames, 11.6 with 1000 of 128.)
        // Round 5: a request of ONE or a few sentences fills a fraction of the SIMDs whatever its chunk length, and its
        // time is that of one item = (chunk + 18 warm-up frames) x 240 samples x 0.25 us: shorter chunks down to 6-8
        // frames, while the hand-off positions stay few enough for a redo round to be rare (same box, chunk 16 / 8 /
        // 6 / 4 frames at 18 of warm-up, ms per run: the reference's three benchmark sentences -- 277, 420, 742 frames
        // -- 2.38 / 1.88 / 1.75 / 1.62, 2.47 / 1.97 / 1.85 / 1.73, 3.66 / 2.68 / 2.47 / 2.54; 8 x 400 frames 2.59 /
        // 2.68 / 2.43 / 2.20; one utterance of 2,000 frames 3.86 / 2.89 / 3.12 / 3.12: tools/small_geometry_sweep.py,
        // profiles/r05_small_geometry_sweep.txt).  A shorter warm-up does not pay there: at 10 frames and below the
        // failing hand-offs cost a redo round more often than the frames saved.
        const uint64_t target = sumT >= 400000 ? 2048 : 1024;
        const uint64_t floor_w = sumT < 1024 ? 6 : sumT < 8192 ? 8 : 16;
        ch = (uint32_t)std::max<uint64_t>((sumT + target - 1) / target, floor_w);
        if (ch >= 16)
            ch = (ch + 7) / 8 * 8;
    }
    p.chunk_frames = ch;
    if (!warmup_given && ch != 0 && !invariant)
        p.warmup_frames = warmup_at(ch);
    // (a chunk length given by the caller: one wave per SIMD if the items fit)
    if (p.lane_kernel && ch != 0 && in.chunk_frames)
        p.waves_per_simd = chunks_at(ch) <= slots1 ? 1 : 2;
    // the checkpoint a failed chunk is first recomputed to (finish_verify): 48 frames into chunks of 96 and more, 24 into
    // chunks of 36 and more, 16 into chunks of 24 and more (a single 128 s utterance, 799 chunks of 32 frames: all six
    // failing hand-offs settle there and the redo is one round of 16 frames, 10.2 -> 9.2 ms per call; 8 frames into
    // 16-frame chunks settle three in four but the rest still take their rounds: same time, not done)
    // (JB_BATCH_INVARIANT: the positions are constants, and each chunk has them or not by its own length -- a chunk of
    // 60 frames and more the first, of 108 and more the second; shorter chunks are recomputed to their end)
    p.ckpt_frames = invariant ? kVocCkptFrames
                    : ch >= 2 * kVocCkptFrames ? kVocCkptFrames
                    : ch >= kVocCkptFramesShort + 12 ? kVocCkptFramesShort
                    : ch >= kVocCkptFramesTiny + 8 ? kVocCkptFramesTiny : 0;
    p.ckpt2_frames = invariant || (p.ckpt_frames == kVocCkptFrames && ch >= kVocCkpt2Frames + 48) ? kVocCkpt2Frames : 0;
    // checkpoint for the partial redo, wherever the chunk goes on for at least 12 frames behind it.  (A
    // redo round lasts as long as its longest item: when only chunks of twice the checkpoint had one, the
    // short last chunk of an utterance -- up to 95 frames recomputed to their end -- made the round of a
    // batch of distinct utterances 5.7 ms instead of the 2.9 ms of 48 frames.)
    const uint32_t need = p.ckpt_frames + (p.ckpt_frames < kVocCkptFramesShort ? 8u : 12u);
    for (size_t i = 0; i < in.B; i++) {
        const uint32_t Ti = in.T[i];
        if (Ti == 0)
            continue;
        const uint32_t ci = invariant ? inv_chunk(Ti) : ch;
        if (ci == 0 || Ti <= ci + p.warmup_frames) {
            p.items.push_back(VocPlanItem{(uint32_t)i, 0, 0, Ti, 0}); // a single item leaves no state
            continue;
        }
        for (uint32_t t0 = 0; t0 < Ti; t0 += ci) {
            VocPlanItem w{(uint32_t)i, t0 > p.warmup_frames ? t0 - p.warmup_frames : 0, t0, std::min(Ti, t0 + ci), 0};
            const bool first = t0 == 0;
            w.saves = kSaveEnd;
            if (!first)
                w.saves |= kSaveWarm;
            if (!first && p.ckpt_frames && w.t_end - w.t_out >= need)
                w.saves |= kSaveCkpt;
            if ((w.saves & kSaveCkpt) && p.ckpt2_frames && w.t_end - w.t_out >= p.ckpt2_frames + 12u)
                w.saves |= kSaveCkpt2;
            p.items.push_back(w);
        }
    }
    // longest utterances first for the serial case; chunk items are uniform
    if (ch == 0)
        std::stable_sort(p.items.begin(), p.items.end(), [](const VocPlanItem &a, const VocPlanItem &c) {
            return (a.t_end - a.t_start) > (c.t_end - c.t_start);
        });
    if (p.lane_kernel) {
        // launch permutation: equal-length chunks share a wave (lanes run in lock step).  With several condition
        // classes (per-utterance alpha / volume) the chunks go by class first, and each class is padded to whole
        // waves with slots that hold no chunk: a wave's chunks then share the alpha and volume it keeps in scalar
        // registers.  One class: the plain permutation.
        const uint32_t n = (uint32_t)p.items.size();
        auto len = [&](uint32_t k) { return p.items[k].t_end - p.items[k].t_start; };
        std::vector<uint32_t> ord(n);
        std::iota(ord.begin(), ord.end(), 0u);
        if (!in.voc_class) {
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return len(x) > len(y); });
            p.order = std::move(ord);
        } else {
            auto cls = [&](uint32_t k) { return in.voc_class[p.items[k].utt]; };
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
                return cls(x) != cls(y) ? cls(x) < cls(y) : len(x) > len(y);
            });
            const uint32_t per_wave = (uint32_t)vocoder_ls_chunks_per_wave(in.nmcp);
            for (uint32_t k = 0; k < n; k++) {
                p.order.push_back(ord[k]);
                const bool class_ends = k + 1 == n || cls(ord[k + 1]) != cls(ord[k]);
                while (class_ends && p.order.size() % per_wave)
                    p.order.push_back(kLtNoItem);
            }
        }
    }
    return p;
}

RedoPick redo_pick_round(const std::vector<VocPlanItem> &items, const std::vector<uint8_t> &pending)
{
    // This round: every failing chunk whose predecessor is final, AND -- speculatively -- a failing chunk
    // behind a failing chunk: it starts from the end state its predecessor left in the FIRST pass.  That state
    // stands if the predecessor settles at its checkpoint (295 of 297 do; stage A of a chunk with a checkpoint
    // does not touch the dump), or, for a chunk without a checkpoint, if the end state of its recomputation
    // -- written to a scratch dump, compared after the launch, then copied over -- meets it to the hand-off
    // tolerance (the trajectory that started wrong has had warm-up + chunk frames to converge: every one of
    // 156 did in a batch of 16 x 25,546 frames).  Where it does not stand, the successor's recomputation
    // started from a state that is being replaced: it stays pending for the next round.  (Before, a run of
    // consecutive failures cost one round per chunk: 3 ms each with checkpoints, 1.2 ms each for 20-frame
    // chunks, two or three rounds per step in small batches.)
    const uint32_t n = (uint32_t)items.size();
    RedoPick p;
    p.in_round.assign(n, 0);
    for (uint32_t k = 1; k < n; k++) {
        if (!pending[k])
            continue;
        if (!pending[k - 1] || (p.in_round[k - 1] && (items[k - 1].saves & kSaveEnd) && items[k - 1].utt == items[k].utt)) {
            p.ids.push_back(k);
            p.in_round[k] = 1;
        }
    }
    return p;
}

RedoStageA redo_stage_a(const std::vector<VocPlanItem> &items, const RedoPick &pick)
{
    const uint32_t n = (uint32_t)items.size();
    RedoStageA a;
    a.spec_end.assign(n, 0);
    for (size_t j = 0; j < pick.ids.size(); j++) {
        const uint32_t k = pick.ids[j];
        if (items[k].saves & kSaveCkpt) {
            a.part.push_back((uint32_t)j);
        } else if (k + 1 < n && pick.in_round[k + 1] && items[k + 1].utt == items[k].utt && (items[k].saves & kSaveEnd)) {
            a.spec_end[k] = 1;
            a.part.push_back((uint32_t)j);
        }
    }
    return a;
}

std::vector<uint32_t> redo_second_checkpoint(const std::vector<VocPlanItem> &items, const std::vector<uint32_t> &ids,
                                             const std::vector<uint8_t> &unsettled, bool ckpt2)
{
    std::vector<uint32_t> mid_ids;
    for (uint32_t k : ids)
        if (ckpt2 && (items[k].saves & kSaveCkpt) && (items[k].saves & kSaveCkpt2) && unsettled[k])
            mid_ids.push_back(k);
    return mid_ids;
}

RedoSettled redo_settle(const std::vector<VocPlanItem> &items, const RedoPick &pick, const std::vector<uint8_t> &pending,
                        const std::vector<uint8_t> &spec_end, const std::vector<uint8_t> &unsettled)
{
    RedoSettled s;
    s.final_now.assign(items.size(), 0);
    for (uint32_t k : pick.ids) {
        // valid: started from a final state -- the predecessor was final before the round, or it was in the
        // round, valid itself, and its first-pass end state stands (settled at its checkpoint / met by the end
        // state of its recomputation)
        const bool pred_in = pick.in_round[k - 1] && pending[k - 1];
        const bool valid = !pred_in || (s.final_now[k - 1] && ((items[k - 1].saves & kSaveCkpt) || spec_end[k - 1]) && !unsettled[k - 1]);
        if (!valid)
            continue; // stays pending: next round, from the state its predecessor is getting now
        s.final_now[k] = 1;
        if (!(items[k].saves & kSaveCkpt)) {
            s.n_full++;
            s.full_ids.push_back(k);
        } else if (!unsettled[k]) {
            s.n_partial++;
        } else {
            s.n_full++;
            s.full_ids.push_back(k);
            s.rest.push_back(k);
        }
    }
    return s;
}

std::vector<uint32_t> redo_recertify(const std::vector<VocPlanItem> &items, const std::vector<uint32_t> &full_ids,
                                     const std::vector<uint8_t> &in_round, const std::vector<uint8_t> &pending)
{
    // Re-certification.  Chunk k+1 was checked against the end state chunk k left in the first
    // pass -- the end of a trajectory now known to have started wrong.  Where chunk k has been
    // recomputed to its end, that dump now holds the exact state: compare it with the warm state of
    // chunk k+1 again and put k+1 on the list if it fails.  (A chunk settled at its checkpoint kept
    // its first-pass end state, whose trajectory was certified at the checkpoint: nothing to re-check.)
    std::vector<uint32_t> succ;
    for (uint32_t k : full_ids)
        // (a successor that was recomputed in this round started from this chunk's end state: nothing to re-check
        // if that was valid, and it is still pending if not)
        if (k + 1 < items.size() && items[k + 1].utt == items[k].utt && (items[k + 1].saves & kSaveWarm) && !pending[k + 1] &&
            !in_round[k + 1] && (items[k].saves & kSaveEnd))
            succ.push_back(k + 1);
    return succ;
}

FrameBlocks plan_frame_blocks(int fperiod, int nlpf)
{
    int bs = std::min(64, fperiod);
    while (fperiod % bs)
        bs--;
    if ((bs < nlpf - 1 || bs < 16) && bs < std::min(64, fperiod)) {
        const int nblk = (fperiod + 63) / 64;
        bs = (fperiod + nblk - 1) / nblk;
    }
    return FrameBlocks{bs, (fperiod + bs - 1) / bs};
}

void plan_voiced_runs(const double *lf0, size_t n, std::vector<uint32_t> &durations, std::vector<double> &msd)
{
    for (size_t f = 0; f < n; f++) {
        const double v = lf0[f] != kNoData ? 1.0 : 0.0;
        if (msd.empty() || msd.back() != v) {
            msd.push_back(v);
            durations.push_back(0);
        }
        durations.back()++;
    }
}

VocCondPlan plan_voc_conditions(const jb_utt_voc &voice, uint32_t nmcp, uint32_t stage, const jb_utt_voc *utt, size_t n)
{
    auto cond = [&](const jb_utt_voc &c) {
        VocUtt u{};
        u.alpha = c.alpha;
        u.volume = c.volume;
        u.beta = (c.beta > 0.0 && nmcp > 2 && stage == 0) ? c.beta : 0.0;
        u.beta_stage = stage ? c.beta : 0.0;
        return u;
    };
    auto same = [](const VocUtt &a, const VocUtt &b) {
        return a.alpha == b.alpha && a.volume == b.volume && a.beta == b.beta && a.beta_stage == b.beta_stage;
    };
    VocCondPlan p;
    p.batch = cond((utt && n) ? utt[0] : voice);
    for (size_t i = 1; utt && i < n && !p.mixed; i++)
        p.mixed = !same(cond(utt[i]), p.batch);
    if (p.batch.beta > 0.0)
        p.pf_alphas.push_back(p.batch.alpha);
    if (!p.mixed)
        return p;
    p.utt.resize(n);
    p.cls.resize(n);
    std::vector<std::pair<double, double>> cls; // (alpha, volume) of each class
    for (size_t i = 0; i < n; i++) {
        VocUtt &u = p.utt[i];
        u = cond(utt[i]);
        const auto key = std::make_pair(u.alpha, u.volume);
        const size_t c = std::find(cls.begin(), cls.end(), key) - cls.begin();
        if (c == cls.size())
            cls.push_back(key);
        p.cls[i] = (uint32_t)c;
        if (u.beta > 0.0) {
            const size_t k = std::find(p.pf_alphas.begin(), p.pf_alphas.end(), u.alpha) - p.pf_alphas.begin();
            if (k == p.pf_alphas.size())
                p.pf_alphas.push_back(u.alpha);
            u.pf = (uint32_t)k;
        }
        p.batch.beta = std::max(p.batch.beta, u.beta);
        p.batch.beta_stage = std::max(p.batch.beta_stage, u.beta_stage);
    }
    p.n_classes = (uint32_t)cls.size();
    return p;
}

StreamMode plan_stream_mode(const jb_stream_desc &s, uint32_t si, uint32_t flags, uint32_t stage, bool from_tracks,
                            int mt_max_dim)
{
    StreamMode m{};
    const int L = (int)s.vector_length;
    const int generic = (flags & JB_BATCH_GENERIC_MLPG) ? 1 : 0;
    m.W = from_tracks ? 1 : (int)s.num_windows;
    m.is_msd = from_tracks ? (si == 1) : (int)s.is_msd;
    m.use_gv = from_tracks ? 0 : (int)s.use_gv;
    int maxw = from_tracks ? 1 : 0;
    for (int w = 0; !from_tracks && w < m.W; w++)
        maxw = std::max(maxw, (int)s.win_width[w]);
    m.BW = (maxw / 2) * 2 + 1;
    // [dim][frame] workspace with the fused kernels: band width 3, up to three windows (the sliding-window
    // build), 3..60 dims; everything else takes the generic reference-shaped kernels
    m.mt = (m.BW == 3 && m.W <= 3 && !generic && L > 2 && L <= mt_max_dim) ? 1 : 0;
    // MCP, non-MSD, [dim][frame]: its transpose is fused with mc2b (enqueue_paramgen)
    // (Stage::NonZero reads the [frame][dim] track itself: k_stage_coef)
    m.defer_out = (si == 0 && m.mt && !m.is_msd && stage == 0 && !from_tracks) ? 1 : 0;
    m.is_static = mlpg_is_static(m.BW, m.W, m.use_gv, generic);
    return m;
}

std::vector<size_t> plan_synth_groups(const size_t *line_off, size_t n_utts, int forced, bool one_batch)
{
    size_t ngroups = 1;
    const size_t total_lines = n_utts ? line_off[n_utts] - line_off[0] : 0;
    if (n_utts >= 8 && total_lines >= 16000)
        ngroups = 2;
    if (forced)
        ngroups = (size_t)std::max(1, forced);
    if (one_batch)
        ngroups = 1;
    ngroups = std::max<size_t>(1, std::min(ngroups, n_utts));
    std::vector<size_t> glo(ngroups + 1, n_utts);
    glo[0] = 0;
    for (size_t g = 1, u = 0; g < ngroups; g++) {
        const size_t want = line_off[0] + total_lines * g / ngroups;
        while (u < n_utts && line_off[u] < want)
            u++;
        glo[g] = std::max(u, glo[g - 1]);
    }
    return glo;
}

} // namespace jb

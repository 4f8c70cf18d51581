/*
 * jbonsai_amd.h -- C ABI of libjbonsai_amd.so: an MI355X (gfx950) drop-in for the
 * parameter-generation + MLSA-vocoder hot path of the `jbonsai` crate (v0.4.2).
 *
 * The reference exposes a Rust library API, not an FFI; each entry point below
 * names the reference item it stands in for (file:line under /root/reference).
 * A Rust shim re-exporting `Engine` / `SpeechGenerator` over these symbols is in
 * INTEGRATION.md.  All functions return 0 (JB_OK) or a negative jb_status; no
 * exception or unwinding crosses this boundary; jb_last_error() gives the text
 * for the calling thread.  No torch / HIP types appear in any signature.
 *
 * Two levels:
 *   (1) state level  -- `jb_batch_*`, `jb_paramgen_vocode_batch`: the exact image
 *       of `ModelStream` + `durations` (src/model/model_stream.rs:6-15,
 *       src/engine.rs:321-357), batched over independent utterances.  This is
 *       the seam the HIP kernels sit behind: MlpgAdjust::create x3
 *       (src/mlpg_adjust/mod.rs:51-95) -> SpeechGenerator::generate_all
 *       (src/speech.rs:87-96) -> Vocoder::synthesize (src/vocoder/mod.rs:72-141).
 *   (2) engine level -- `jb_engine_*`, `jb_synthesize*`, `jb_generator_*`: mirrors
 *       Engine::{load, load_from_bytes, synthesize, generator} (src/engine.rs:257-366)
 *       and SpeechGenerator::{fperiod, synthesized_frames, generate_step}
 *       (src/speech.rs:53-82); label parsing / tree search / durations run on
 *       the host, everything from the state level down runs on the GPU.
 */
#ifndef JBONSAI_AMD_H
#define JBONSAI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JB_MAX_STREAM 3
#define JB_MAX_WINDOW 8
#define JB_NODATA (-1e10) /* src/constants.rs:13 */

typedef enum jb_status {
    JB_OK = 0,
    JB_ERR_INVALID = -1,     /* bad argument / shape (reference: panics in src/speech.rs:32-40) */
    JB_ERR_UNSUPPORTED = -2, /* shapes no kernel is built for: nmcp > 64, window widths above 9, stages above 256, nlpf > 2047, other
                                than three streams (frame periods, stages and low-pass orders are otherwise free: rounds 1-4 refused
                                stages above 8, nlpf > 63 and frame periods without a divisor <= 64 that is >= nlpf - 1) */
    JB_ERR_DEVICE = -3,      /* HIP error or no gfx950 device: the product never falls back to CPU */
    JB_ERR_MODEL = -4,       /* ModelError (src/model/mod.rs:31-46) */
    JB_ERR_LABEL = -5,       /* LabelError (src/label.rs:8-23) */
    JB_ERR_PARSE_OPTION = -6,/* EngineError::ParseOptionError (src/engine.rs:21-23) */
    JB_ERR_WEIGHT = -7,      /* WeightError (src/model/interporation_weight.rs:7-14) */
    JB_ERR_BUFFER = -8       /* output buffer too small (reference: panic, src/speech.rs:69-71) */
} jb_status;

/* ------------------------------------------------------------------------ */
/* (1) state level                                                          */
/* ------------------------------------------------------------------------ */

/* Per-stream static description: StreamModelMetadata + Windows
 * (src/model/voice/mod.rs, src/model/voice/window.rs:4-22). */
typedef struct jb_stream_desc {
    uint32_t vector_length;              /* L */
    uint32_t num_windows;                /* W */
    uint32_t is_msd;
    uint32_t use_gv;
    uint32_t win_width[JB_MAX_WINDOW];   /* odd widths */
    const double *win_coef;              /* concatenated coefficients, sum(win_width) */
} jb_stream_desc;

/* Vocoder::new arguments (src/vocoder/mod.rs:45-55) + stream layout. */
typedef struct jb_voice_desc {
    uint32_t sampling_frequency;  /* rate */
    uint32_t fperiod;
    uint32_t nstream;             /* 3: MCP, LF0, LPF (src/engine.rs:303-313 needs stream 2) */
    uint32_t stage;               /* 0: MLSA (mel-cepstra); 1..256: Stage::NonZero, gamma = -1/stage, spectrum = [gain, LSP...],
                                     MGLSA filter (vocoder/mod.rs:90-107,142-176; parity unpinned: no reference test reaches it) */
    uint32_t use_log_gain;        /* ignored when stage==0 */
    double alpha, beta, volume;   /* beta > 0: post-filter per frame (stage 0: cepstrum.rs:23-37; stage > 0: lsp.rs:113-139) */
    jb_stream_desc stream[JB_MAX_STREAM];
} jb_voice_desc;

/* State-level parameters of one stream of one utterance: StreamParameter +
 * GvParameter (src/model/stream_parameter.rs:11, src/model/mod.rs:49). */
typedef struct jb_stream_states {
    const double *mean;        /* [S][W*L]; element L*w+m (src/mlpg_adjust/mod.rs:62) */
    const double *var;         /* [S][W*L] */
    const double *msd;         /* [S]; NULL => f64::MAX (non-MSD, src/model/mod.rs:113) */
    const double *gv_mean;     /* [L] or NULL (no GV) */
    const double *gv_var;      /* [L] */
    const uint8_t *gv_switch;  /* [S] */
    double gv_weight;          /* Condition::gv_weight[i]   (src/engine.rs:93) */
    double msd_threshold;      /* Condition::msd_threshold[i] (src/engine.rs:92) */
} jb_stream_states;

typedef struct jb_state_utt {
    uint32_t num_states;        /* S = labels * nstate */
    const uint32_t *durations;  /* [S] frames per state (src/duration.rs) */
    jb_stream_states stream[JB_MAX_STREAM];
} jb_state_utt;

/* FLAC options (jb_batch_set_flac, jb_flac_encode_pcm_batch, jb_synthesize*_flac).  All zero (or a NULL pointer) =
 * the defaults: block_size 4096, max_lpc_order 8 (what `flac -5` uses for mono).  block_size 16..4608 (0: 4096);
 * max_lpc_order 0..12, 0 with a nonzero block_size = CONSTANT, VERBATIM and FIXED subframes only; reserved 0.
 * Anything else: JB_ERR_INVALID before any device is touched. */
typedef struct jb_flac_opts {
    uint32_t block_size;
    uint32_t max_lpc_order;
    uint32_t reserved[2];
} jb_flac_opts;
/* New.  FLAC metadata that needs the samples or the frame offsets (jb_batch_set_flac_meta, the *_flac_meta entries;
 * see "FLAC" below).  All zero (or a NULL pointer) = neither: the stream of jb_flac_opts alone, byte for byte.
 * flags: JB_FLAC_MD5 puts the MD5 of the samples into STREAMINFO; any other bit is JB_ERR_INVALID.
 * seek_interval_ms > 0 adds a SEEKTABLE with one point about every seek_interval_ms of audio.  reserved must be 0. */
#define JB_FLAC_MD5 1u
typedef struct jb_flac_meta {
    uint32_t flags;
    uint32_t seek_interval_ms;
    uint32_t reserved[2];
} jb_flac_meta;

/* Output sample format (jb_batch_set_format, jb_format_pcm_batch, jb_format_pcm_host, jb_synthesize*_formatted; see
 * "Output sample formats" below).  dither: JB_DITHER_TPDF with JB_FMT_S16 and JB_FMT_S24 only; seed: the dither's,
 * one per batch.  An unknown format or dither, or dither with another format: JB_ERR_INVALID before any device is
 * touched. */
#define JB_FMT_F32 1u  /* float32 in +-1.0, 4 bytes little-endian */
#define JB_FMT_S16 2u  /* 16-bit PCM, 2 bytes */
#define JB_FMT_S24 3u  /* 24-bit PCM, 3 bytes packed, little-endian */
#define JB_FMT_ULAW 4u /* G.711 mu-law, 1 byte */
#define JB_FMT_ALAW 5u /* G.711 A-law, 1 byte */
#define JB_DITHER_NONE 0u
#define JB_DITHER_TPDF 1u
typedef struct jb_format_opts {
    uint32_t format; /* JB_FMT_* */
    uint32_t dither; /* JB_DITHER_* */
    uint64_t seed;
} jb_format_opts;

/* IMA ADPCM options (jb_batch_set_adpcm, jb_adpcm_encode_pcm_batch, jb_adpcm_encode_host, jb_synthesize*_adpcm; see
 * "IMA ADPCM" below).  block_align 0 = by each utterance's output rate (256 below 22,050 Hz, 512 below 44,100 Hz, 1024
 * otherwise: the Microsoft convention); otherwise a multiple of 4 in 32..8192; reserved 0.  Anything else:
 * JB_ERR_INVALID before any device is touched. */
typedef struct jb_adpcm_opts {
    uint32_t block_align;
    uint32_t reserved[3];
} jb_adpcm_opts;
/* New.  Filterbank options (jb_batch_set_fbank, jb_fbank_pcm_batch, jb_fbank_host, jb_synthesize*_fbank; see "Filterbank features" below).
 * win_us, hop_us: window and hop in microseconds (25000 and 10000 are the usual values); n_fft 0 = the smallest power
 * of two that holds the window; f_max_hz 0 = half the rate; log_floor 0 = 2^-52; reserved 0.  Anything outside the
 * limits of that section: JB_ERR_INVALID, naming the field, before any device is touched. */
#define JB_FBANK_HANN 0u    /* periodic: 0.5 - 0.5 cos(2 pi j / wl) */
#define JB_FBANK_HAMMING 1u /* symmetric: 0.54 - 0.46 cos(2 pi j / (wl - 1)) */
#define JB_FBANK_CENTER 1u  /* frame t is centred on sample t hop; samples outside the unit read as 0 */
#define JB_FBANK_LINEAR 2u  /* the filters' energies themselves, not their logarithms */
#define JB_FBANK_UNIT 4u    /* samples scaled by 2^-15 (full scale 1.0) instead of the 16-bit scale */
#define JB_FBANK_F64 8u     /* f64 elements instead of f32 */
typedef struct jb_fbank_opts {
    uint32_t win_us, hop_us;
    uint32_t n_fft, n_mels;
    double f_min_hz, f_max_hz;
    double log_floor;
    uint32_t window; /* JB_FBANK_HANN, JB_FBANK_HAMMING */
    uint32_t flags;  /* JB_FBANK_CENTER | _LINEAR | _UNIT | _F64 */
    uint32_t reserved[4];
} jb_fbank_opts;
/* New.  Cepstral options (jb_batch_set_mfcc, jb_mfcc_host, jb_mfcc_pcm_host, jb_mfcc_frames_batch, jb_mfcc_pcm_batch,
 * jb_synthesize*_mfcc; see "Cepstral features" below).  n_ceps 0 = no DCT and no lifter (the log-mel energies themselves); lifter 0 = none; var_floor 0 =
 * 2^-52; reserved 0.  Anything outside the limits of that section: JB_ERR_INVALID, naming the field, before any device
 * is touched. */
#define JB_CMVN_NONE 0u     /* the statics as they are */
#define JB_CMVN_MEAN 1u     /* c - mu, per unit and dimension */
#define JB_CMVN_MEAN_VAR 2u /* (c - mu) / sqrt(max(var, var_floor)) */
#define JB_MFCC_F64 1u      /* f64 elements instead of f32 */
typedef struct jb_mfcc_opts {
    uint32_t n_ceps;       /* 0..n_mels */
    uint32_t delta_order;  /* 0..2 */
    uint32_t delta_window; /* N, 1..5 (at every order) */
    uint32_t cmvn;         /* JB_CMVN_* */
    double lifter;         /* Q */
    double var_floor;
    uint32_t flags;        /* JB_MFCC_F64 */
    uint32_t reserved[3];
} jb_mfcc_opts;
/* New.  Frame conditioning (jb_batch_set_frame_opts, jb_engine_set_frame_opts, the _framed entries; see "Frame
 * conditioning" below): what makes a frame of the filterbank and cepstral stages Kaldi's.  It stands beside a
 * jb_fbank_opts (and a jb_mfcc_opts), as the cepstral options stand beside the filterbank's.  All zero = the identity;
 * reserved 0.  Anything outside the limits of that section: JB_ERR_INVALID, naming the field, before any device is
 * touched.  jb_frame_kaldi fills in compute-fbank-feats' defaults. */
#define JB_FRAME_WINDOW_OPTS 0u /* the window of the jb_fbank_opts, unchanged */
#define JB_FRAME_POVEY 1u       /* (0.5 - 0.5 cos(a j))^0.85,  a = 2 pi / (wl - 1) */
#define JB_FRAME_HANN_SYM 2u    /* 0.5 - 0.5 cos(a j)   (Kaldi's "hanning") */
#define JB_FRAME_RECT 3u        /* 1 */
#define JB_FRAME_BLACKMAN 4u    /* 0.42 - 0.5 cos(a j) + 0.08 cos(2 a j) */
#define JB_FRAME_REMOVE_DC 1u   /* flags */
#define JB_FRAME_REFLECT 2u     /* flags: Kaldi's snip_edges = false */
#define JB_FRAME_ENERGY 4u      /* flags: behind an mfcc request with n_ceps >= 1, c0 is the frame's log energy */
typedef struct jb_frame_opts {
    double preemph; /* c in [0, 1]; 0: none */
    uint32_t window, flags;
    uint32_t reserved[4]; /* 0 */
} jb_frame_opts;
/* New.  Mel spectrogram options (jb_batch_set_melspec, jb_melspec_pcm_batch, jb_melspec_host, jb_synthesize*_melspec;
 * see "Mel spectrograms" below).  Window and hop in samples at the unit's own rate; win_length 0 = n_fft; f_max_hz 0 =
 * half the rate; floor 0 = 1e-10; range 0 = no clamp; scale 0 = 1.0; reserved 0.  Anything outside the limits of that
 * section: JB_ERR_INVALID, naming the field, before any device is touched.  jb_melspec_whisper fills in Whisper's. */
#define JB_MEL_HTK 0u         /* mel(f) = 2595 log10(1 + f / 700) */
#define JB_MEL_SLANEY 1u      /* 3 f / 200 below 1 kHz, 15 + ln(f / 1000) / (ln 6.4 / 27) above */
#define JB_MEL_NORM_NONE 0u   /* triangles of height 1 */
#define JB_MEL_NORM_SLANEY 1u /* each filter times 2 / (f_{m+2} - f_m): unit area */
#define JB_MEL_PAD_REFLECT 0u /* frame t centred on sample t hop, the unit reflected about its edge samples */
#define JB_MEL_PAD_ZERO 1u    /* centred, zeros outside the unit */
#define JB_MEL_PAD_NONE 2u    /* frame t starts at sample t hop; whole frames only */
#define JB_MEL_LOG_NONE 0u    /* the filters' sums themselves */
#define JB_MEL_LOG_LN 1u      /* ln(max(E, floor)) */
#define JB_MEL_LOG_LOG10 2u   /* log10(max(E, floor)) */
#define JB_MEL_LOG_DB 3u      /* 10 log10(max(E, floor)) */
#define JB_MEL_MAGNITUDE 1u   /* |X_k| instead of |X_k|^2 */
#define JB_MEL_DROP_LAST 2u   /* without the last frame (reflect and zero padding only) */
#define JB_MEL_F64 4u         /* f64 elements instead of f32 */
typedef struct jb_melspec_opts {
    uint32_t n_fft, win_length, hop_length, n_mels;
    double f_min_hz, f_max_hz; /* f_max 0: half the rate */
    double floor;              /* clamp in front of the logarithm; 0: 1e-10 */
    double range;              /* 0: none; else y = max(y, Ymax - range), Ymax over the unit */
    double offset, scale;      /* out = (y + offset) * scale; scale 0: 1.0 */
    uint32_t mel_scale;        /* JB_MEL_HTK, JB_MEL_SLANEY */
    uint32_t norm;             /* JB_MEL_NORM_NONE, JB_MEL_NORM_SLANEY */
    uint32_t pad;              /* JB_MEL_PAD_REFLECT, _ZERO, _NONE */
    uint32_t log;              /* JB_MEL_LOG_NONE, _LN, _LOG10, _DB */
    uint32_t flags;            /* JB_MEL_MAGNITUDE | _DROP_LAST | _F64 */
    uint32_t reserved[3];      /* 0 */
} jb_melspec_opts;
/* The join request of one utterance (see "Join" below): the programme it belongs to, the zero samples before and
 * after it and the lengths of its edge fades.  reserved must be 0. */
#define JB_JOIN_NONE 0xffffffffu
typedef struct jb_join_utt {
    uint32_t programme;             /* id below jb_batch_size(b), or JB_JOIN_NONE: a programme of its own */
    uint32_t fade_in, fade_out;     /* samples at the output rate; 0: none */
    uint32_t reserved;              /* 0 */
    uint64_t pad_before, pad_after; /* zero samples at the output rate */
} jb_join_utt;
/* The join of a jb_synthesize_programme* call: all its utterances are one programme.  lead_ms of zeros in front of the
 * first, gap_ms between neighbours, trail_ms behind the last, a fade of fade_ms at both edges of every utterance; each
 * in samples at the output rate by jb_join_ms_to_samples.  Finite and not negative; reserved 0. */
typedef struct jb_join_opts {
    double lead_ms, gap_ms, trail_ms, fade_ms;
    uint32_t reserved[2];
} jb_join_opts;
/* The mix request of one utterance (see "Mix" below): the programme it belongs to, where it starts within it, the zero
 * samples it claims behind its end, its edge fades (the join's) and its gain.  reserved and reserved2 must be 0. */
#define JB_MIX_NONE 0xffffffffu
typedef struct jb_mix_utt {
    uint32_t programme;         /* id below jb_batch_size(b), or JB_MIX_NONE: a programme of its own */
    uint32_t fade_in, fade_out; /* samples at the output rate; 0: none */
    uint32_t reserved;          /* 0 */
    uint64_t start;             /* the member's first sample within the programme, at the output rate */
    uint64_t pad_after;         /* zero samples behind its last one that count for the programme's length */
    double gain_db;             /* finite in [-120, 40], or -INFINITY: muted, the member counts for the length alone */
    uint64_t reserved2;         /* 0 */
} jb_mix_utt;
/* The options of a whole mix request.  JB_MIX_FIT: a programme whose peak lies above the ceiling is scaled down to
 * it; ceiling_db in dBFS (finite, in [-120, 0]; 0 dBFS = 32768), read with the flag only.  reserved 0. */
#define JB_MIX_FIT 1u
typedef struct jb_mix_opts {
    uint32_t flags;
    uint32_t reserved;
    double ceiling_db;
} jb_mix_opts;
/* What the mix stage did to one programme. */
typedef struct jb_mix_report {
    double peak;       /* M_p: the largest |sum| in f64 in front of the fit and the sink (a NaN sample is passed over) */
    double scale;      /* s_p: what JB_MIX_FIT multiplied the sum by; 1 without the flag or under the ceiling */
    uint32_t depth;    /* the largest number of unmuted members over one sample */
    uint32_t reserved; /* 0 */
    uint64_t overlap;  /* samples under two or more unmuted members */
} jb_mix_report;
/* A member's place in jb_engine_set_programme_mix: its start behind the lead, and its gain. */
typedef struct jb_mix_place {
    double start_ms, gain_db;
} jb_mix_place;

/* The output filter (see "Filter" below): a cascade of up to JB_FILTER_MAX_SECTIONS second-order sections at the
 * output rate, applied in order.  A section is a kind with f0_hz, q and gain_db (gain_db: peaking and the shelves
 * only, but finite everywhere), or JB_FILTER_RAW with b0 b1 b2 a1 a2 (a0 = 1), used as given at any rate.  reserved 0.
 * n_sections 0: no filter. */
#define JB_FILTER_MAX_SECTIONS 4
#define JB_FILTER_HIGHPASS 1u
#define JB_FILTER_LOWPASS 2u
#define JB_FILTER_PEAKING 3u
#define JB_FILTER_LOWSHELF 4u
#define JB_FILTER_HIGHSHELF 5u
#define JB_FILTER_NOTCH 6u
#define JB_FILTER_RAW 7u
typedef struct jb_filter_section {
    uint32_t kind; /* JB_FILTER_* */
    uint32_t reserved;
    double f0_hz, q, gain_db;
    double b0, b1, b2, a1, a2; /* JB_FILTER_RAW only */
} jb_filter_section;
typedef struct jb_filter {
    jb_filter_section section[JB_FILTER_MAX_SECTIONS];
    uint32_t n_sections;
    uint32_t reserved;
} jb_filter;
/* One designed section: y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2]. */
typedef struct jb_biquad {
    double b0, b1, b2, a1, a2;
} jb_biquad;

typedef struct jb_batch_opts {
    int32_t device;         /* HIP device ordinal; -1 = current */
    uint32_t flags;         /* JB_BATCH_* */
    uint32_t chunk_frames;  /* vocoder time-chunk length in frames; 0 = auto */
    uint32_t warmup_frames; /* frames each chunk starts early from zero state; 0 = default (18; 14 for batches with 1000 and more distinct hand-off positions) */
    double verify_tol;      /* chunk hand-off check: max|state diff| <= tol*max|state|; 0 = default (1e-9) */
    uint32_t reserved0;     /* must be 0 (rounds 1-3: mlpg_cus_per_xcd, a CU partition that lost at every split; removed) */
    uint32_t reserved;
} jb_batch_opts;

#define JB_BATCH_KEEP_TRACKS 1u  /* keep MLPG parameter tracks readable (tests) */
#define JB_BATCH_GENERIC_MLPG 2u /* un-fused, reference-shaped MLPG kernels (A/B parity tests) */
#define JB_BATCH_SERIAL 4u       /* one wave per utterance, no time-chunking (reference-shaped recursion): an utterance's
                                    audio is then bitwise independent of the rest of the batch */
#define JB_BATCH_WAVE_KERNEL 8u  /* always the wave-per-chunk vocoder kernel (A/B tests) */
#define JB_BATCH_LANE_KERNEL 16u /* always the lane-triple throughput kernel, whatever the batch size (A/B tests) */
#define JB_BATCH_PCM_I16 64u     /* fused 16-bit sink: the vocoder writes clamped i16 PCM (value.min(32767).max(-32768)
                                    as i16, examples/is-bonsai/main.rs:44-48) instead of f64: 2 B/sample leave
                                    the GPU instead of 8.  jb_batch_read_pcm / device_pcm then fail; use the
                                    _i16 forms */
#define JB_BATCH_SERIAL_GV 32u   /* GV sums in the reference's serial order: parameter tracks bit-exact
                                    against src/mlpg_adjust/mlpg.rs:145-292, slower.  The default runs the
                                    GV sweeps time-parallel with fixed-shape tree reductions (deterministic;
                                    tracks agree to ~1e-14 relative) */

#define JB_BATCH_MLPG_ONLY 128u  /* MlpgAdjust::create only (src/mlpg_adjust/mod.rs:31-51): the run ends with the
                                    three parameter tracks (implies KEEP_TRACKS); no excitation, no PCM, and
                                    no device memory for them.  What jb_mlpg_batch sets */

#define JB_BATCH_NO_EXC_TABLE 512u /* A/B tests: the pulse-free excitation of EVERY frame is computed per utterance
                                    (what a voice whose LPF taps differ from frame to frame gets anyway) instead of
                                    read from the table all utterances share where their taps are the batch's
                                    canonical ones; same bits either way */

#define JB_BATCH_INVARIANT 1024u /* fast batch-invariant mode: every choice the default mode makes from the whole batch
                                    is made from the utterance and the voice alone, with the throughput kernels.
                                    The output bits are a function of the voice, the utterance's inputs (states or
                                    tracks, its jb_utt_voc), verify_tol, the library build and the GPU architecture;
                                    they do not depend on the other utterances of the batch, the utterance's position
                                    in it, the device list of a _multi entry, the entry point, the number of batches
                                    in flight, or whether the resident GV kernel formed.  They differ from the default
                                    mode's and from JB_BATCH_SERIAL's (both stay within the hand-off tolerance of the
                                    serial recursion).  Combined with chunk_frames, warmup_frames,
                                    JB_BATCH_WAVE_KERNEL or JB_BATCH_LANE_KERNEL: JB_ERR_INVALID before any device is
                                    touched.  With JB_BATCH_SERIAL (already invariant) the serial mode runs and this
                                    flag has no effect.  How: per utterance of T frames, chunks of
                                    clamp(ceil(T / 96), 16, 153) frames behind 18 frames of warm-up, checkpoints at
                                    48 / 96 frames into chunks long enough for them, the lane-triple kernel wherever
                                    the voice supports it (else one fixed wave-kernel form), redo rounds on one fixed
                                    wave-kernel form, the GV by the resident kernel or, wherever it does not run (rows
                                    of more than 64 of its tiles, too few CUs, a formation timeout), by its
                                    multi-launch form k_mlpg_gv_gsweep with the same sums bit for bit, and no
                                    serially served head in the generator */

#define JB_BATCH_TEST_GANG_TIMEOUT 256u /* test aid: the first run behaves as if the resident GV kernel had timed
                                    out in formation (possible without a fault when several such launches share a
                                    device), which makes jb_batch_sync redo the step with the multi-launch GV
                                    sweeps; jb_batch_gang_fallbacks counts these.  (JB_GENERATOR_TEST_GANG_TIMEOUT=1
                                    in the environment does the same to the batch behind jb_generator_new.) */

/* Time-chunked vocoder (default).  The MLSA recursion is time-serial per utterance
 * (src/vocoder/mlsa.rs), but it forgets its initial state within ~16 frames (measured:
 * <=2e-11 relative after 16, rounding floor after 24; tools/warmup_study.py).  Each
 * utterance is cut into chunks that start `warmup_frames` early from zero state; a
 * device-side check then requires every chunk's warmed-up filter state to match its
 * predecessor's end state within verify_tol, and any chunk that fails is recomputed
 * serially from that end state, so the result is certified against the serial one. */

/* ---- indexed state level --------------------------------------------------
 * The per-state Gaussians of an utterance are rows of the voice's pdf tables, selected by the
 * decision trees (src/model/voice/model.rs:51-82) and, with several voices, blended with the
 * interpolation weights (VoiceSet weighted sum, src/model/voice_set.rs:80-95).  Here the tables
 * live on the device and an utterance is given by its row indices: the gather and the blend
 * (first*w0, then += w_i*param_i in voice order, as the reference) run on the GPU, and 12 bytes
 * per state and voice cross PCIe instead of 2.2 kB per state. */
#define JB_MAX_VOICES 8
typedef struct jb_pdf_table {
    const float *rows;  /* [n_rows][row_len] f32 as stored in the voice: means | variances | (msd weight) */
    uint32_t n_rows;    /* all trees of the stream concatenated */
    uint32_t row_len;   /* 2*L*W (+1 for MSD streams) */
} jb_pdf_table;
typedef struct jb_pdf_set jb_pdf_set;
/* tables[v * nstream + s] = stream s of voice v.  The rows are copied to `device` (-1 = current). */
int jb_pdf_set_create(const jb_pdf_table *tables, uint32_t n_voices, uint32_t nstream, int32_t device,
                      jb_pdf_set **out);
void jb_pdf_set_free(jb_pdf_set *set);

typedef struct jb_index_stream {
    const uint32_t *row[JB_MAX_VOICES]; /* [S] row of the state's pdf in voice v's table */
    const double *weight;               /* [n_voices] interpolation weights (Condition, engine.rs:211-243) */
    const double *gv_mean, *gv_var;     /* as jb_stream_states (already blended: one pdf per utterance) */
    const uint8_t *gv_switch;
    double gv_weight, msd_threshold;
} jb_index_stream;
typedef struct jb_index_utt {
    uint32_t num_states;
    const uint32_t *durations;
    jb_index_stream stream[JB_MAX_STREAM];
    double lf0_offset; /* additional_half_tone * ln2/12 added to the static LF0 mean and clamped to
                          [ln 20, ln 20000] (stream_parameter.rs:29-37); 0 = none */
} jb_index_utt;

typedef struct jb_batch jb_batch;

/* Upload a batch of utterances to HBM and allocate outputs/workspace.
 * Utterances may alias each other's input arrays. */
int jb_batch_create(const jb_voice_desc *voice, const jb_state_utt *utts, size_t n_utts,
                    const jb_batch_opts *opts, jb_batch **out);
/* Same from row indices into device-resident pdf tables (gather + blend on the GPU). */
int jb_batch_create_indexed(const jb_voice_desc *voice, const jb_pdf_set *set, const jb_index_utt *utts,
                            size_t n_utts, const jb_batch_opts *opts, jb_batch **out);
/* Vocoder condition of one utterance: the Vocoder::new arguments alpha, beta and volume (src/vocoder/mod.rs:45-55;
 * Condition::alpha / beta / volume, src/engine.rs:46-80) that jb_voice_desc otherwise holds for the whole batch.
 * volume is linear, as jb_voice_desc.volume.  The beta rule is the batch's: stage 0 filters with beta only where
 * nmcp > 2 (cepstrum.rs:24), stage > 0 hands it to postfilter_lsp (lsp.rs:113-139). */
typedef struct jb_utt_voc {
    double alpha, beta, volume;
} jb_utt_voc;
/* jb_batch_create / jb_batch_create_indexed with one jb_utt_voc per utterance (voc[n_utts]): utterance u is vocoded
 * as Vocoder::new(..., voc[u].alpha, voc[u].beta, voc[u].volume) would (new entry: the reference has no batch).
 * voc == NULL: every utterance takes voice->alpha / beta / volume, i.e. jb_batch_create[_indexed].  Entries are
 * checked like jb_voice_desc's (beta >= 0; alpha, beta, volume finite): JB_ERR_INVALID naming the entry. */
int jb_batch_create_voc(const jb_voice_desc *voice, const jb_state_utt *utts, size_t n_utts, const jb_utt_voc *voc,
                        const jb_batch_opts *opts, jb_batch **out);
int jb_batch_create_indexed_voc(const jb_voice_desc *voice, const jb_pdf_set *set, const jb_index_utt *utts,
                                size_t n_utts, const jb_utt_voc *voc, const jb_batch_opts *opts, jb_batch **out);
/* Enqueue the whole hot path (MLPG+GV x3 -> frame prologue -> pulse schedule ->
 * excitation + MLSA) on the batch's HIP stream.  Inputs are already resident. */
int jb_batch_run(jb_batch *b);
int jb_batch_sync(jb_batch *b);
/* run + sync, returning device time of the launch sequence in ms (HIP events on
 * the batch's own stream); vocoder_ms = the MLSA kernel alone. */
int jb_batch_run_timed(jb_batch *b, float *total_ms, float *vocoder_ms);
/* Device times of the last completed run (call after jb_batch_sync): whole launch
 * sequence and the vocoder kernel alone, from HIP events on the batch's stream. */
int jb_batch_last_timing(jb_batch *b, float *total_ms, float *vocoder_ms);
size_t jb_batch_size(const jb_batch *b);
size_t jb_batch_num_frames(const jb_batch *b, size_t utt);
size_t jb_batch_num_samples(const jb_batch *b, size_t utt);
size_t jb_batch_total_samples(const jb_batch *b);
/* The read entries below (and jb_batch_device_pcm) wait for the batch's pending run and for the
 * hand-off certification + redo first, as jb_batch_sync does: what they return is the finished result.
 * Copy utterance `utt`'s PCM (f64, un-clipped, as Vec<f64> of src/engine.rs:294). */
int jb_batch_read_pcm(jb_batch *b, size_t utt, double *dst, size_t cap);
/* Same for a batch created with JB_BATCH_PCM_I16 (16-bit PCM as written to WAV by the reference's
 * examples, examples/is-bonsai/main.rs:37-49). */
int jb_batch_read_pcm_i16(jb_batch *b, size_t utt, int16_t *dst, size_t cap);
/* Whole batch at once: dst[u] must hold jb_batch_num_samples(b, u) samples (may be NULL for empty
 * utterances).  The slab streams through a ring of pinned slots at link rate while worker threads
 * scatter finished slots into the caller's buffers (what jb_synthesize_batch uses): several times the
 * rate of one pageable copy per utterance. */
int jb_batch_read_pcm_all(jb_batch *b, double *const *dst);
int jb_batch_read_pcm_i16_all(jb_batch *b, int16_t *const *dst);
/* Parameter track of stream s ([T][L], NODATA in unvoiced frames); needs KEEP_TRACKS. */
int jb_batch_read_track(jb_batch *b, size_t utt, uint32_t stream, double *dst, size_t cap);
/* Device memory and HIP streams of freed batches are kept per device for the next batch
 * (hipMalloc/hipFree of a config-2 batch cost more than its GPU work, stream creation more than a
 * one-sentence synthesis); this hands them back to the driver.  The memory cap is
 * JB_DEVICE_POOL_MB (environment, default 65536; 0 disables the memory pool). */
int jb_release_cached_memory(void);
/* Changes the cap of each device's memory pool (megabytes; 0 disables the pool) and trims what is cached
 * beyond it.  A caller that keeps several large batches alive in turn (bench.py's config-3 job) raises it. */
int jb_set_cached_memory_limit(size_t megabytes);
/* Parity tap: the MLSA filter coefficients the vocoder interpolates between, [T][nmcp] =
 * mc2b(postfilter_mcp(spectrum)) per frame (src/vocoder/mod.rs:116-118). */
int jb_batch_read_coefficients(jb_batch *b, size_t utt, double *dst, size_t cap);
/* The coefficients frame 0 STARTS from, [nmcp]: equal to frame 0's row above unless a post-filter or
 * Stage::NonZero is on (then: of the un-filtered spectrum, vocoder/mod.rs:80-106). */
int jb_batch_read_first_coefficients(jb_batch *b, size_t utt, double *dst, size_t cap);
/* Debug/parity taps: excitation before gain [N]; needs KEEP_TRACKS. */
int jb_batch_read_excitation(jb_batch *b, size_t utt, double *dst, size_t cap);
/* Device pointer + sample count of the batch's contiguous PCM slab (for an RCCL gather
 * by the caller); utterance i starts at sample jb_batch_pcm_offset(b,i).  f64 samples, or
 * i16 for a JB_BATCH_PCM_I16 batch. */
void *jb_batch_device_pcm(jb_batch *b, size_t *n_samples);
size_t jb_batch_pcm_offset(const jb_batch *b, size_t utt);
/* Execution facts of the last run: chunk length / warm-up actually used, number of
 * vocoder work items, and how many chunks failed the hand-off check and were redone.
 * (JB_BATCH_INVARIANT: every utterance has a chunk length of its own; this is the longest.) */
int jb_batch_info(const jb_batch *b, uint32_t *chunk_frames, uint32_t *warmup_frames,
                  uint32_t *n_items, uint32_t *n_redo);
/* Of the chunks that failed the hand-off check in the last run: how many were settled by
 * recomputing only up to their checkpoint (48 frames) and how many had to be recomputed to the end. */
int jb_batch_redo_stats(const jb_batch *b, uint32_t *n_partial, uint32_t *n_full);
/* Which vocoder kernel the last run's work list was built for: *lane_triple = 1 the throughput kernel
 * (k_vocoder_lt: one time-chunk per lane triple), 0 the wave kernel (k_vocoder: one chunk per wave);
 * *waves_per_simd = 1 or 2 (four- / eight-wave workgroups of the throughput kernel; 0 for the wave kernel). */
int jb_batch_kernel_info(const jb_batch *b, uint32_t *lane_triple, uint32_t *waves_per_simd);
/* Times the resident GV kernel of this batch gave up in formation and the step was redone with the
 * multi-launch sweeps (0 in normal operation; see jb_gv_gang.hip "Liveness"). */
uint32_t jb_batch_gang_fallbacks(const jb_batch *b);
/* New (the reference only emits the voice's own rate; Condition::set_sampling_frequency changes the rate the vocoder
 * converts pitch with, not the rate of the audio).  Output rate of the batch's PCM: out_hz[0] for every utterance
 * (n == 1) or out_hz[u] for utterance u (n == jb_batch_size(b)); 0, or the voice's rate, = native.  Only before the
 * batch's first run, and not on a JB_BATCH_MLPG_ONLY batch: JB_ERR_INVALID.  A pair whose ratio reduces to L/M with
 * L or M above 2048: JB_ERR_UNSUPPORTED (jb_last_error says why).  With some utterance at another rate, the run
 * converts the certified PCM on the device (jb_resample_filter's table) and jb_batch_num_samples / total_samples /
 * pcm_offset, jb_batch_read_pcm[_all], jb_batch_read_pcm_i16[_all], jb_batch_device_pcm and so jb_gather_pcm all
 * report the output: ceil(N L / M) samples for N at the voice's rate, f64 or 16-bit by the batch's flags (the 16-bit
 * conversion then follows the conversion of the rate; native utterances of such a batch are copied, values
 * unchanged).  Excitation, coefficient and track reads stay at the voice's rate.  With every entry native nothing
 * runs and nothing is allocated: the batch is the one created.  The call records the request and answers the
 * geometry at once; the converter's slabs and tables are allocated by the first jb_batch_run, as the loudness and
 * FLAC ones are, so a device allocation failure for them surfaces there and not from this call. */
int jb_batch_set_output_rate(jb_batch *b, const uint32_t *out_hz, size_t n);
/* Rate of utterance utt's PCM as the read entries hand it out (the voice's rate when native); 0 for no such utterance. */
uint32_t jb_batch_output_rate(const jb_batch *b, size_t utt);
/* The vocoder's f64 PCM of utterance utt at the voice's rate, jb_batch_num_frames * fperiod samples (what
 * jb_batch_read_pcm reads without an output rate or a loudness target: never normalized).  Readable whenever an
 * output rate or a loudness target is set, with JB_BATCH_PCM_I16 as well; a JB_BATCH_PCM_I16 batch without either has
 * no f64 PCM: JB_ERR_INVALID. */
int jb_batch_read_pcm_native(jb_batch *b, size_t utt, double *dst, size_t cap);
/* New (the reference's only level control is the fixed `volume` gain).  Loudness normalization ("loudness" below):
 * target_lufs[0] for every utterance (n == 1) or target_lufs[u] for utterance u (n == jb_batch_size(b)), and one peak
 * ceiling (dBFS; +INFINITY: none).  A NaN target: the utterance is measured and gets gain 0 dB unless its peak is above
 * the ceiling.  Only before the batch's first run, and not on a JB_BATCH_MLPG_ONLY batch: JB_ERR_INVALID.  Together
 * with an output rate, in either order: the measurement is taken at the output rate.  The run measures the output
 * f64 on the device and writes x * g to a slab of its own, f64 or 16-bit by the flags: jb_batch_read_pcm[_all],
 * jb_batch_read_pcm_i16[_all], jb_batch_device_pcm and so jb_gather_pcm hand that out (lengths and offsets
 * unchanged); jb_batch_read_pcm_native does not.  Without a call nothing runs and nothing is allocated.  An output
 * rate whose hop is outside 1..61439 samples fails at the run with JB_ERR_UNSUPPORTED. */
int jb_batch_set_loudness_target(jb_batch *b, const double *target_lufs, size_t n, double ceiling_dbfs);
/* What the last run measured and applied for utterance utt (each pointer may be NULL): L (LUFS, -INFINITY when no
 * block survives the gates), P (dBFS, -INFINITY for silence) and gain_dB.  Waits for the run like the read entries;
 * a batch without a target or not yet run: JB_ERR_INVALID. */
int jb_batch_loudness(jb_batch *b, size_t utt, double *lufs, double *peak_dbfs, double *gain_db);
/* New.  What the ceiling of jb_batch_set_loudness_target bounds ("loudness" below, step 5): the sample peak
 * (JB_PEAK_SAMPLE, the default) or the true peak (JB_PEAK_TRUE, dBTP).  mode[0] for every utterance (n == 1) or
 * mode[u] for utterance u (n == jb_batch_size(b)); any other value, or another n: JB_ERR_INVALID.  Only before the
 * batch's first run, and not on a JB_BATCH_MLPG_ONLY batch: JB_ERR_INVALID.  In either order with the target; without
 * a target it has no effect.  A batch with every utterance in sample mode launches and allocates nothing more. */
#define JB_PEAK_SAMPLE 0
#define JB_PEAK_TRUE 1
int jb_batch_set_peak_mode(jb_batch *b, const uint32_t *mode, size_t n);
/* jb_batch_loudness with the true peak: TP (NaN for an utterance in sample mode), the utterance's mode and the
 * oversampling factor F its TP was taken with (1 in sample mode).  gain_db is the gain applied, by the rule of the
 * utterance's mode.  Readiness rules of jb_batch_loudness. */
typedef struct jb_loudness_report {
    double lufs, sample_peak_dbfs, true_peak_dbtp, gain_db;
    uint32_t peak_mode, oversampling;
} jb_loudness_report;
int jb_batch_loudness_report(jb_batch *b, size_t utt, jb_loudness_report *out);
/* New.  Programme loudness ("loudness" below, step 6): one measurement, one peak and one gain for a group of
 * utterances, so that their relative levels survive -- libebur128's ebur128_loudness_global_multiple, ReplayGain's
 * album gain.  group[u] is a group id below jb_batch_size(b), or JB_LOUDNESS_NO_GROUP for an utterance of its own;
 * n == jb_batch_size(b).  group == NULL with n == 0 withdraws the request.  The members of one group must agree on
 * target, ceiling, peak mode and output rate (two NaN targets agree): this call, jb_batch_set_loudness_target,
 * jb_batch_set_peak_mode and jb_batch_set_output_rate each check the combined request, and a call that would leave a
 * group mixed is refused with JB_ERR_INVALID (jb_last_error names the group and the field) and changes nothing.
 * Only before the batch's first run.  In either order with the target; without a target it has no effect.  The
 * per-utterance entries (jb_batch_loudness, jb_batch_loudness_report) keep reporting each utterance's own L, P and
 * TP; their gain_db is the gain applied, the group's.  Without a call nothing more runs and nothing is allocated. */
#define JB_LOUDNESS_NO_GROUP 0xffffffffu
int jb_batch_set_loudness_groups(jb_batch *b, const uint32_t *group, size_t n);
/* The group of utterance utt, numbered densely in the order of the groups' first members (an utterance of its own
 * counts as a group of one); -1 without a group request or for no such utterance. */
int32_t jb_batch_loudness_group_of(const jb_batch *b, size_t utt);
/* New.  The R128 report ("loudness" below, steps 7 and 8): with JB_LOUDNESS_R128 the run also takes the largest
 * momentary and short-term loudness and the loudness range of every utterance and of every group; 0 withdraws the
 * request.  Only before the batch's first run; without a target it has no effect.  Changes no sample. */
#define JB_LOUDNESS_R128 1u
int jb_batch_set_loudness_report(jb_batch *b, uint32_t flags);
typedef struct jb_loudness_r128 {
    double max_momentary_lufs;  /* over every 400 ms block, no gate; -INFINITY without a block */
    double max_short_term_lufs; /* over every 3 s window; -INFINITY without a window */
    double lra_lu;              /* loudness range; 0 when n_windows == 0 */
    double lra_low_lufs, lra_high_lufs; /* the 10 % and 95 % windows; NaN when n_windows == 0 */
    uint64_t n_windows;         /* windows above both gates of step 8 */
} jb_loudness_r128;
/* What the last run measured for utterance utt; needs JB_LOUDNESS_R128 and a target.  Readiness rules of
 * jb_batch_loudness. */
int jb_batch_loudness_r128(jb_batch *b, size_t utt, jb_loudness_r128 *out);
/* What the last run measured and applied for the group of utterance utt: L_G, P_G, TP_G (NaN in sample mode), the
 * one gain, the group's peak mode and oversampling factor, its member count, and, when flags has JB_LOUDNESS_R128,
 * the group's R128 fields (zeros otherwise).  Needs a group request and a target.  Readiness rules of
 * jb_batch_loudness. */
typedef struct jb_loudness_group_report {
    double lufs, sample_peak_dbfs, true_peak_dbtp, gain_db;
    uint32_t peak_mode, oversampling; /* oversampling: 1 in sample mode, 0 where the rate is not known */
    uint32_t members, flags;
    jb_loudness_r128 r128;
} jb_loudness_group_report;
int jb_batch_loudness_group(jb_batch *b, size_t utt, jb_loudness_group_report *out);
/* New.  FLAC output (see "FLAC" below): the run encodes each utterance's 16-bit PCM as the read entries hand it out
 * (after the output rate and the loudness target) into one FLAC stream per utterance, on the device.  opts: NULL or
 * zeros = the defaults.  Only before the batch's first run, on a JB_BATCH_PCM_I16 batch that is not
 * JB_BATCH_MLPG_ONLY; otherwise JB_ERR_INVALID.  An output rate with no frame-header code fails at the run with
 * JB_ERR_UNSUPPORTED.  The PCM read entries keep working.  Without a call nothing runs and nothing is allocated. */
int jb_batch_set_flac(jb_batch *b, const jb_flac_opts *opts);
/* New.  The streams' MD5 and SEEKTABLE (jb_flac_meta): after jb_batch_set_flac and before the batch's first run;
 * otherwise, or with unknown flag bits or non-zero reserved words, JB_ERR_INVALID.  NULL or zeros withdraw the
 * request.  jb_batch_flac_size and the read entries work as before (a table adds its bytes to the size). */
int jb_batch_set_flac_meta(jb_batch *b, const jb_flac_meta *m);
/* Bytes of utterance utt's stream; waits for the run like the read entries.  No FLAC or no such utterance:
 * JB_ERR_INVALID. */
int jb_batch_flac_size(jb_batch *b, size_t utt, size_t *n_bytes);
/* The stream of utterance utt into dst; cap below jb_batch_flac_size: JB_ERR_BUFFER. */
int jb_batch_read_flac(jb_batch *b, size_t utt, uint8_t *dst, size_t cap);
/* Every stream: dst[u] must hold jb_batch_flac_size(b, u) bytes (one device-to-host copy for the batch). */
int jb_batch_read_flac_all(jb_batch *b, uint8_t *const *dst);
/* New.  Output sample format (see "Output sample formats" below): the run also writes each utterance's final f64
 * PCM -- what jb_batch_read_pcm hands out, after the output rate and the loudness target -- as bytes of opts->format,
 * on the device.  Only before the batch's first run, on a batch that is neither JB_BATCH_PCM_I16 (the stage reads
 * f64; FLAC, which needs the 16-bit batch, is therefore never in the same batch) nor JB_BATCH_MLPG_ONLY; otherwise
 * JB_ERR_INVALID.  The f64 read entries keep working.  Without a call nothing runs and nothing is allocated. */
int jb_batch_set_format(jb_batch *b, const jb_format_opts *opts);
/* Bytes of utterance utt in the format: jb_batch_num_samples x jb_format_bytes_per_sample.  No format or no such
 * utterance: JB_ERR_INVALID. */
int jb_batch_formatted_size(jb_batch *b, size_t utt, size_t *n_bytes);
/* The bytes of utterance utt into dst; waits for the run like the read entries; cap below jb_batch_formatted_size:
 * JB_ERR_BUFFER. */
int jb_batch_read_formatted(jb_batch *b, size_t utt, uint8_t *dst, size_t cap);
/* Every utterance: dst[u] must hold jb_batch_formatted_size(b, u) bytes (one device-to-host copy for the batch). */
int jb_batch_read_formatted_all(jb_batch *b, uint8_t *const *dst);
/* New.  IMA ADPCM output (see "IMA ADPCM" below): the run also encodes each utterance's final PCM -- what the PCM read
 * entries hand out, after the output rate and the loudness target; the f64 of an f64 batch quantised by the 16-bit
 * sink's rule, the 16-bit samples of a JB_BATCH_PCM_I16 batch -- as 4-bit WAV blocks, on the device.  Only before the
 * batch's first run, on a batch that is not JB_BATCH_MLPG_ONLY; otherwise JB_ERR_INVALID.  Independent of FLAC and of
 * the sample format: it may be requested with either.  The PCM read entries keep working.  Without a call nothing runs
 * and nothing is allocated. */
int jb_batch_set_adpcm(jb_batch *b, const jb_adpcm_opts *opts);
/* Bytes of utterance utt's blocks (known from the geometry once the request is made) and its block size A.  No
 * request or no such utterance: JB_ERR_INVALID. */
int jb_batch_adpcm_size(jb_batch *b, size_t utt, size_t *n_bytes);
int jb_batch_adpcm_block_align(jb_batch *b, size_t utt, uint32_t *block_align);
/* The blocks of utterance utt into dst; waits for the run like the read entries; cap below jb_batch_adpcm_size:
 * JB_ERR_BUFFER. */
int jb_batch_read_adpcm(jb_batch *b, size_t utt, uint8_t *dst, size_t cap);
/* Every utterance: dst[u] must hold jb_batch_adpcm_size(b, u) bytes (one device-to-host copy for the batch). */
int jb_batch_read_adpcm_all(jb_batch *b, uint8_t *const *dst);
/* New (none: no reference counterpart).  Filterbank features (see "Filterbank features" below): the run also turns
 * each utterance's final f64 PCM -- what jb_batch_read_pcm hands out, after the output rate, the filter and the
 * loudness target; behind a join each programme -- into [T][n_mels] log-mel frames, on the device.  The options are
 * checked at every utterance's output rate, here and again by jb_batch_set_output_rate (JB_ERR_INVALID naming the
 * field).  Only before the batch's first run ("... is set before the batch's first run"), on a batch that is neither
 * JB_BATCH_PCM_I16 nor JB_BATCH_MLPG_ONLY (JB_ERR_UNSUPPORTED).  opts == NULL withdraws the request.  Independent of
 * the sample format and IMA ADPCM; the PCM read entries keep working and their bytes do not change.  Without a call
 * nothing runs and nothing is allocated. */
int jb_batch_set_fbank(jb_batch *b, const jb_fbank_opts *opts);
/* Frames, filters and rate of unit `unit` (an utterance; behind a join a programme), known once the request is made;
 * any out pointer may be NULL.  No request or no such unit: JB_ERR_INVALID. */
int jb_batch_fbank_shape(jb_batch *b, size_t unit, size_t *T, uint32_t *n_mels, uint32_t *hz);
/* Its bytes: T x n_mels x 4 (8 with JB_FBANK_F64). */
int jb_batch_fbank_size(jb_batch *b, size_t unit, size_t *n_bytes);
/* The frames of unit `unit` into dst, row-major; waits for the run like the read entries; cap below
 * jb_batch_fbank_size: JB_ERR_BUFFER. */
int jb_batch_read_fbank(jb_batch *b, size_t unit, uint8_t *dst, size_t cap);
/* Every unit: dst[u] must hold jb_batch_fbank_size(b, u) bytes (one device-to-host copy for the batch). */
int jb_batch_read_fbank_all(jb_batch *b, uint8_t *const *dst);
/* New.  Cepstral features of every unit's final PCM (see "Cepstral features" below): cepstra, deltas and CMVN behind a
 * filterbank pass of the stage's own with the geometry of fopts (its JB_FBANK_LINEAR or JB_FBANK_F64: JB_ERR_INVALID).
 * Preconditions as jb_batch_set_fbank's: an f64 batch (JB_BATCH_PCM_I16, JB_BATCH_MLPG_ONLY: JB_ERR_UNSUPPORTED), before
 * the first run; checked at every unit's output rate, and again by jb_batch_set_output_rate.  Both NULL withdraws the
 * request.  Independent of jb_batch_set_fbank, which keeps its own slab and bytes; behind a join the units are the
 * programmes, and the CMVN runs over the whole programme. */
int jb_batch_set_mfcc(jb_batch *b, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts);
/* New.  The frame request beside jb_batch_set_fbank's and jb_batch_set_mfcc's (see "Frame conditioning" below): both
 * stages condition their frames by it.  Before the first run, in either order with the two; the pair is checked when
 * both are present and again at the first run, where a request without an fbank or mfcc request is JB_ERR_INVALID.
 * NULL withdraws the request.  jb_batch_fbank_shape, jb_batch_mfcc_shape and the byte sinks' sizes report the reflected
 * T under JB_FRAME_REFLECT. */
int jb_batch_set_frame_opts(jb_batch *b, const jb_frame_opts *fr);
/* Unit `unit`'s frames, row width d (delta_order + 1) and rate, known once the request is made; any out pointer may be
 * NULL. */
int jb_batch_mfcc_shape(jb_batch *b, size_t unit, size_t *T, uint32_t *width, uint32_t *hz);
/* Its bytes: T x width x 4 (8 with JB_MFCC_F64). */
int jb_batch_mfcc_size(jb_batch *b, size_t unit, size_t *n_bytes);
/* Its rows after a run (waits for the batch); cap below jb_batch_mfcc_size: JB_ERR_BUFFER. */
int jb_batch_read_mfcc(jb_batch *b, size_t unit, uint8_t *dst, size_t cap);
/* Every unit: dst[u] must hold jb_batch_mfcc_size(b, u) bytes (one device-to-host copy for the batch). */
int jb_batch_read_mfcc_all(jb_batch *b, uint8_t *const *dst);
/* New.  Mel spectrograms of every unit's final PCM (see "Mel spectrograms" below), on the device.  Preconditions as
 * jb_batch_set_fbank's: an f64 batch (JB_BATCH_PCM_I16, JB_BATCH_MLPG_ONLY: JB_ERR_UNSUPPORTED), before the first run;
 * checked at every unit's output rate, and again by jb_batch_set_output_rate.  opts == NULL withdraws the request.
 * Independent of jb_batch_set_fbank and jb_batch_set_mfcc, which keep their slabs and bytes; behind a join the units
 * are the programmes, and the range clamp runs under the whole programme's maximum.  Without a call nothing runs and
 * nothing is allocated. */
int jb_batch_set_melspec(jb_batch *b, const jb_melspec_opts *opts);
/* Unit `unit`'s frames, filters and rate, known once the request is made; any out pointer may be NULL. */
int jb_batch_melspec_shape(jb_batch *b, size_t unit, size_t *T, uint32_t *n_mels, uint32_t *hz);
/* Its bytes: T x n_mels x 4 (8 with JB_MEL_F64). */
int jb_batch_melspec_size(jb_batch *b, size_t unit, size_t *n_bytes);
/* Its frames after a run, row-major (waits for the batch); cap below jb_batch_melspec_size: JB_ERR_BUFFER. */
int jb_batch_read_melspec(jb_batch *b, size_t unit, uint8_t *dst, size_t cap);
/* Every unit: dst[u] must hold jb_batch_melspec_size(b, u) bytes (one device-to-host copy for the batch). */
int jb_batch_read_melspec_all(jb_batch *b, uint8_t *const *dst);
/* New (none: no reference counterpart).  Join (see "Join" below): the run also gathers the utterances' final PCM --
 * what the PCM read entries hand out, after the output rate and the loudness target -- into programmes, on the
 * device: each programme its members in ascending utterance index, each between its pads and under its fades.  FLAC,
 * the sample format and IMA ADPCM then encode programmes instead of utterances: the index `utt` of
 * jb_batch_flac_size / _read_flac, jb_batch_formatted_size / _read_formatted and jb_batch_adpcm_size /
 * _adpcm_block_align / _read_adpcm is then a programme (jb_batch_num_outputs of them; one of that number or above:
 * JB_ERR_INVALID), and their _all forms take jb_batch_num_outputs pointers.  n == jb_batch_size(b); req == NULL with
 * n == 0 withdraws the request.  The members of one programme must agree on the output rate: this call and
 * jb_batch_set_output_rate each check the combined request, and a call that would leave a programme mixed is refused
 * with JB_ERR_INVALID (jb_last_error names the programme and the field) and changes nothing.  Only before the batch's
 * first run, on a batch that is not JB_BATCH_MLPG_ONLY; an id of jb_batch_size or above (JB_JOIN_NONE apart) or a
 * non-zero reserved word: JB_ERR_INVALID.  The per-utterance PCM entries, jb_batch_device_pcm and jb_gather_pcm keep
 * handing out utterances.  Without a call nothing more runs, nothing is allocated and no output byte changes. */
int jb_batch_set_join(jb_batch *b, const jb_join_utt *req, size_t n);
/* New (none).  What the encoders' entries index: the programmes with a join request, else the utterances. */
size_t jb_batch_num_outputs(const jb_batch *b);
/* New (none).  The programme of utterance utt, numbered densely in the order of the programmes' first members (a
 * JB_JOIN_NONE utterance counts as a programme of one); -1 without a join request or for no such utterance. */
int32_t jb_batch_programme_of(const jb_batch *b, size_t utt);
/* New (none).  Members, samples and rate of programme p, known from the geometry once the request is made (any out
 * pointer may be NULL).  No request or no such programme: JB_ERR_INVALID. */
int jb_batch_programme_layout(const jb_batch *b, size_t p, size_t *n_members, uint64_t *n_samples, uint32_t *hz);
/* New (none).  The first sample of utterance utt within its programme, behind its pad_before: the cue list that maps
 * sentences to times.  No request or no such utterance: JB_ERR_INVALID. */
int jb_batch_member_start(const jb_batch *b, size_t utt, uint64_t *start_sample);
/* New (none).  The PCM of programme p, f64 or 16-bit by the batch's flags as jb_batch_read_pcm / _i16; waits for the
 * run like the read entries; cap below the programme's samples: JB_ERR_BUFFER. */
int jb_batch_read_programme_pcm(jb_batch *b, size_t p, double *dst, size_t cap);
int jb_batch_read_programme_pcm_i16(jb_batch *b, size_t p, int16_t *dst, size_t cap);
/* New (none: no reference counterpart).  Mix (see "Mix" below), the join's sibling in the join's place: the run also
 * sums the utterances' final PCM into programmes, on the device, each member at its start and under its gain.  All
 * that jb_batch_set_join says of the encoders' indices, of jb_batch_num_outputs, _programme_of, _programme_layout,
 * _member_start and _read_programme_pcm / _i16, of the output rate and of when the call is allowed holds here too.
 * n == jb_batch_size(b); opts may be NULL (no flags); req == NULL with n == 0 withdraws the request.  A batch holds a
 * join request or a mix request, never both: the second setter is refused with JB_ERR_INVALID and changes nothing;
 * withdrawing the one frees the way for the other.  Refused with JB_ERR_INVALID (jb_last_error names the utterance or
 * programme and the field): a bad programme id, members of mixed rates, a gain_db outside [-120, 40] that is not
 * -INFINITY, non-zero reserved words, an unknown flag, a ceiling_db outside [-120, 0] with JB_MIX_FIT.  Work lists of
 * more than 2^24 entries: JB_ERR_UNSUPPORTED. */
int jb_batch_set_mix(jb_batch *b, const jb_mix_utt *req, size_t n, const jb_mix_opts *opts);
/* New (none).  What the stage did to programme p, after a run (peak and scale are the device's).  JB_ERR_INVALID
 * without a mix request, before a run or for no such programme. */
int jb_batch_mix_report(jb_batch *b, size_t p, jb_mix_report *out);
void jb_batch_free(jb_batch *b);

/* One-shot convenience: create + run + read + free.  pcm[i] must hold
 * n_samples[i] doubles; call with pcm==NULL to get n_samples only. */
int jb_paramgen_vocode_batch(const jb_voice_desc *voice, const jb_state_utt *utts, size_t n_utts,
                             const jb_batch_opts *opts, double *const *pcm, size_t *n_samples);

/* ---- the two inner seams of the reference -----------------------------------------
 * MlpgAdjust::new(gv_weight, msd_threshold, model_stream).create(&durations) -> Vec<Vec<f64>>
 * (src/mlpg_adjust/mod.rs:31-51; called once per stream, src/engine.rs:333-357): for every utterance the
 * tracks of all streams.  tracks[u * nstream + s] receives T_u x L_s doubles ([frame][dim], JB_NODATA in
 * unvoiced frames of an MSD stream) or is NULL (that track is not wanted); n_frames[u] = T_u.  Call with
 * tracks == NULL for the frame counts only. */
int jb_mlpg_batch(const jb_voice_desc *voice, const jb_state_utt *utts, size_t n_utts, const jb_batch_opts *opts,
                  double *const *tracks, size_t *n_frames);

/* SpeechGenerator::new(fperiod, vocoder, spectrum, lf0, lpf) (src/speech.rs:25-50) for one utterance: the
 * three parameter tracks as Vec<Vec<f64>> flattened row-major, with their outer and inner lengths so that
 * the reference's three panics can be mirrored as JB_ERR_INVALID with the same messages:
 * outer lengths differ; lf0 inner length != 1; lpf inner length even. */
typedef struct jb_track_utt {
    size_t n_spectrum, n_lf0, n_lpf;                /* outer lengths (frames) */
    uint32_t spectrum_width, lf0_width, lpf_width;  /* inner lengths: nmcp, 1, nlpf (odd) */
    uint32_t reserved;
    const double *spectrum; /* [n_spectrum][spectrum_width]: mel-cepstra (stage 0) or [gain, LSP...] */
    const double *lf0;      /* [n_lf0][1]; JB_NODATA = unvoiced frame (vocoder/mod.rs:73-77) */
    const double *lpf;      /* [n_lpf][lpf_width] */
} jb_track_utt;
/* A batch whose source is parameter tracks: jb_batch_run starts at the frame prologue
 * (Vocoder::synthesize per frame, src/vocoder/mod.rs:72-178).  Of `voice` the Vocoder::new arguments are
 * read (sampling_frequency, fperiod, stage, use_log_gain, alpha, beta, volume, and the vector lengths of
 * streams 0 and 2 = nmcp, nlpf); the window descriptions are not. */
int jb_batch_create_from_tracks(const jb_voice_desc *voice, const jb_track_utt *utts, size_t n_utts,
                                const jb_batch_opts *opts, jb_batch **out);
/* SpeechGenerator::new + generate_all (src/speech.rs:25-50,87-96) for a batch: create + run + read + free.
 * pcm[i] must hold n_samples[i] = n_lf0 * fperiod doubles; pcm == NULL: n_samples only. */
int jb_vocode_tracks_batch(const jb_voice_desc *voice, const jb_track_utt *utts, size_t n_utts,
                           const jb_batch_opts *opts, double *const *pcm, size_t *n_samples);
/* Vocoder::new(nmcp, nlpf, stage, use_log_gain, rate, alpha, beta, volume, fperiod) followed by
 * Vocoder::synthesize(lf0, spectrum, lpf, rawdata) frame after frame over the given tracks
 * (src/vocoder/mod.rs:45-72,72-178): the Vocoder seam itself, WITHOUT SpeechGenerator::new's checks of the LPF
 * length.  This is the one way to the ring-buffer-less branch of Excitation::get (nlpf == 0,
 * src/vocoder/excitation.rs:87-100: bare pulses on voiced samples, the noise stream drawn on unvoiced samples
 * only, no delay): voice->stream[2].vector_length == 0, lpf_width == 0, lpf may be NULL.  An even non-zero
 * count is JB_ERR_UNSUPPORTED (the reference's ring buffer takes it; the kernels here do not).  Outer-length
 * and lf0-width mismatches stay JB_ERR_INVALID.  Same buffers as jb_vocode_tracks_batch. */
int jb_vocoder_synthesize_batch(const jb_voice_desc *voice, const jb_track_utt *utts, size_t n_utts,
                                const jb_batch_opts *opts, double *const *pcm, size_t *n_samples);

/* ---- output rate (new: no reference counterpart) -----------------------------------------------------------------
 * Rational polyphase resampling with a Kaiser-windowed sinc, in f64: g = gcd(in_hz, out_hz), L = out_hz / g,
 * M = in_hz / g, r = min(1, L/M), cutoff fc = 0.45 r cycles per input sample, half-width H = 32 / (2 fc) input
 * samples, C = ceil(H), ntaps = 2 C; h(t) = 2 fc sinc(2 fc t) I0(10 sqrt(1 - (t/H)^2)) / I0(10) for |t| < H, else 0.
 * Output k of N input samples: q = floor(k M / L), p = k M mod L, y[k] = sum_{j=0}^{ntaps-1} h[p][j] x[q - C + 1 + j]
 * with h[p][j] = h(p/L + C - 1 - j), x = 0 outside [0, N) (every utterance alone), n_out = ceil(N L / M).  The device
 * sums in ascending j with explicit FMAs: each output is a function of x and h alone.  L and M up to 2048 (every pair
 * of 8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000 Hz); else JB_ERR_UNSUPPORTED. */
/* The library's phase table, host only (no GPU needed): *L, *M, *ntaps (each may be NULL) and, when taps is not NULL,
 * the [L][ntaps] taps h[p][j] (JB_ERR_BUFFER if cap < L * ntaps).  in_hz == out_hz is the pair L = M = 1 of the
 * formula; the batch entries never filter it. */
int jb_resample_filter(uint32_t in_hz, uint32_t out_hz, uint32_t *L, uint32_t *M, uint32_t *ntaps, double *taps,
                       size_t cap);
/* The path k_resample takes for a pair, by (L, M, ntaps) alone; pure, no GPU is touched.  A workgroup of four waves
 * computes a tile of `rows` output rows (row m holds outputs m L .. m L + L - 1) of one utterance.  pad: the shift s
 * that spreads a half-wave's LDS reads, rows M apart, over the most bank pairs -- one pad double per 2^s window slots,
 * s in {4, 5, 6, 7}, or 0 for none.  cap: the window samples that 8,192 LDS doubles (64 KiB) hold beside the pad
 * doubles of that shift; fit = floor((cap - ntaps) / M), or 0 where ntaps + M > cap.  By fit:
 *   fit >= 256          lds 1, rows 256, row_waves 4: a wave holds 64 rows and walks all L phases
 *   128 <= fit < 256    lds 1, rows 128, row_waves 2: two waves hold the rows, the two pairs split the phases
 *   1 <= fit < 128      lds 1, rows min(fit, 64), row_waves 1: one wave's lanes hold the rows, the four waves split
 *                       the phases (with L < 4 the waves beyond L idle)
 *   fit == 0            lds 0, pad 0, rows 256, row_waves 4: every lane reads the utterance from global memory behind a
 *                       bounds predicate (cap and fit keep the figures of the shift that was picked)
 * lds_bytes is the window of a full tile, rows M + ntaps samples and their pad doubles (0 without LDS; never above
 * 65,536).  in_hz == out_hz is the identity table of the batch entries, not the pair L = M = 1 of the formula:
 * identity 1, ntaps 1, lds 0, pad 0, tiles of rows = 16,384 samples copied.  Every path sums in the order above, so
 * the path changes the speed of a pair and never its bits (tests/test_gpu_resample_paths.py holds each to a host
 * evaluation with std::fma, bit for bit).  Errors as jb_resample_filter's; out NULL: JB_ERR_INVALID. */
typedef struct jb_resample_geometry_t {
    uint32_t L, M, ntaps;
    uint32_t pad, cap, fit;
    uint32_t lds, rows, row_waves, lds_bytes;
    uint32_t identity;
    uint32_t reserved; /* 0 */
} jb_resample_geometry_t;
int jb_resample_geometry(uint32_t in_hz, uint32_t out_hz, jb_resample_geometry_t *out);
/* The converter on PCM the caller holds (the seam of jb_vocoder_synthesize_batch's kind): in[u] of n_in[u] samples at
 * in_hz -> out[u] of n_out[u] = ceil(n_in[u] L / M) samples at out_hz, library-owned (jb_pcm_free each), on `device`
 * (-1 = current). */
int jb_resample_pcm_batch(const double *const *in, const size_t *n_in, size_t n, uint32_t in_hz, uint32_t out_hz,
                          int32_t device, double **out, size_t *n_out);

/* ---- loudness (new: no reference counterpart; ITU-R BS.1770-4 / EBU R128 integrated loudness) -------------------
 * PCM in the library's 16-bit units (full scale 32768); x = an utterance's output as the read entries hand it out
 * before any 16-bit conversion (the vocoder's certified f64, or the converter's f64 with an output rate), N samples
 * at its output rate fs.
 * 1. K-weighting: y = HP(SHELF(x / 32768)), two biquads (transposed direct form II), each utterance alone from zero
 *    state.  K = tan(pi fc / fs), a0 = 1 + K/Q + K^2, a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0];
 *    shelf: fc = 1681.974450955533, Q = 0.7071752369554196, Vh = 10^(3.999843853973347 / 20),
 *    Vb = Vh^0.4996667741545416, b = [(Vh + Vb K/Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K/Q + K^2) / a0];
 *    high-pass: fc = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1].
 *    The shelf's centre has to lie below Nyquist: at fs <= 3363 Hz K is not positive and the shelf's poles leave the
 *    unit circle (a2 = 1.00125 at 3363 Hz, 0.99993 at 3364 Hz).  No loudness value (L, the momentary and short-term
 *    maxima, LRA) is defined there: jb_loudness_pcm_batch, jb_loudness_groups_pcm_batch and a batch with a loudness
 *    target or an R128 report at such an output rate return JB_ERR_UNSUPPORTED, naming the rate; 3364 Hz and up are
 *    measured.  jb_loudness_filter stays the formula at any rate, and the true peak (step 5), which reads no
 *    K-weighted sample, is measured below the limit as well.
 * 2. Hop H = (fs + 5) / 10 (integer division); z_j = sum of y^2 over [jH, (j + 1)H); block i (hops i..i+3, counted
 *    only when (i + 4)H <= N) has l_i = -0.691 + 10 log10((z_i + ... + z_(i+3)) / 4H).
 * 3. Gates: keep l_i > -70; G = -0.691 + 10 log10(mean of their block mean squares) - 10; keep l_i > G as well;
 *    L = -0.691 + 10 log10(mean of the block mean squares left); -INFINITY if none is left (or N < 4H).
 * 4. P = 20 log10(max |x| / 32768) (sample peak; -INFINITY for silence).  gain_dB = min(T - L, C - P) over the terms
 *    that are finite (0 if neither is), T the target, C the ceiling; output x * 10^(gain_dB / 20), one f64 product
 *    per sample, then the 16-bit sink's clamp and truncation on a 16-bit batch.  A quiet or silent utterance is never
 *    amplified past C.
 * 5. True peak (BS.1770-4 Annex 2), on the same f64 x, x = 0 outside [0, N).  Oversampling factor
 *    F = min(64, ceil(192000 / fs)): 48 k -> 4, 44.1 k -> 5, 96 k -> 2, 192 k and above -> 1, 32 k -> 6, 24 k -> 8,
 *    22.05 k -> 9, 16 k -> 12, 11.025 k -> 18, 8 k -> 24.  Interpolator h(t) = sinc(t) I0(8 sqrt(1 - (t/6)^2)) / I0(8)
 *    for |t| < 6, else 0, sinc(t) = sin(pi t) / (pi t); 12 taps per phase, h[p][j] = h(p/F + 5 - j), j = 0..11 (the size
 *    of the Annex 2 example filter); phases p = 1..F-1 are tabled, phase 0 is the samples themselves.
 *    y_p[n] = sum_{j=0}^{11} h[p][j] x[n - 5 + j] for n = 0..N-1, summed as h[p][0] x[n-5] and then FMAs in ascending
 *    j (the resampler's rule): each y is a function of x and h alone.  TPlin = max(max |x[n]|, max_{p,n} |y_p[n]|),
 *    TP = 20 log10(TPlin / 32768) dBTP, -INFINITY for silence; TP >= P by construction, and with F = 1 TP = P and
 *    nothing extra runs.  In true-peak mode (JB_PEAK_TRUE) the gain rule is step 4 with TP in place of P:
 *    gain_dB = min(T - L, C - TP) over the finite terms; the reported P stays the sample peak.  Sample mode is the
 *    default.  TP is measured on the f64 before any 16-bit conversion: what the 16-bit sink's clamp and truncation
 *    do to the waveform is not measured again.  One gain per utterance: no look-ahead limiting.
 * 6. Groups (jb_batch_set_loudness_groups).  The blocks of a group are the union of its members' own blocks (a
 *    block never straddles two members: this is libebur128's ebur128_loudness_global_multiple, not the loudness of
 *    the concatenated file).  With l_i of step 2: keep l_i > -70; G_G = the loudness of the mean of their mean
 *    squares, minus 10; keep l_i > G_G as well; L_G = the loudness of the mean of the mean squares left, -INFINITY
 *    when none is.  P_G (TP_G in true-peak mode) is the largest of the members' peaks.  gain_dB is step 4's rule,
 *    min(T - L_G, C - P_G) over the finite terms, and every member is multiplied by the same g, the identical f64.
 *    Fixed order: a member's partial (sum, count) of each gate pass is formed as for an utterance alone (256 lanes,
 *    lane t adding blocks t, t + 256, ...; then a tree, lane t taking lane t + w for w = 128, 64, ..., 1), and the
 *    members' partials are added one after the other in ascending utterance index.  So a group of one member gives
 *    the ungrouped result bit for bit, and a group's result depends on its members' samples, rate and relative order
 *    only -- not on the batch, the members' positions or what else runs: JB_BATCH_INVARIANT output stays invariant for
 *    a whole group.
 * 7. Momentary maximum: max_i l_i over all blocks of step 2, no gate; -INFINITY without a block.  Short-term:
 *    s_i = (z_i + ... + z_(i+29)) / (30 H) for i = 0 .. nh - 30 (nh = N / H full hops), added in ascending hop order:
 *    a 3 s window at every 100 ms hop, none for nh < 30; the maximum is reported as loudness, -0.691 + 10 log10(s).
 * 8. Loudness range (EBU Tech 3342): of the s_i with loudness above -70, G_r = the loudness of their mean, minus 20;
 *    keep those above G_r as well, n values in ascending order; lo = element floor((n - 1) 0.10 + 0.5),
 *    hi = element floor((n - 1) 0.95 + 0.5) (libebur128's nearest-rank rule); LRA = 10 log10(hi / lo), 0.0 for n = 0.
 *    For a group the s_i are the union of the members' windows (none straddles two members) and the mean is taken in
 *    the order of step 6.  The two order statistics are exact for any n.
 * L, P, TP and gain_dB are functions of the utterance's samples alone (not of the batch, its order, the entry or the
 * devices); the device sums in fixed orders, so JB_BATCH_INVARIANT output stays invariant with a target. */
/* Host only (no GPU): the coefficients of step 1 at hz, b[6] = b of the shelf then of the high-pass, a[6] likewise
 * (a[0] = a[3] = 1), and *hop = H; each pointer may be NULL.  hz == 0: JB_ERR_INVALID. */
int jb_loudness_filter(uint32_t hz, double *b, double *a, uint32_t *hop);
/* The measurement on PCM the caller holds (jb_resample_pcm_batch's twin): lufs[u] = L and peak_dbfs[u] = P of in[u]
 * (n_in[u] samples at hz), on `device` (-1 = current).  A hop outside 1..61439 samples (hz >= 614395) or a rate of
 * 3363 Hz or less (step 1): JB_ERR_UNSUPPORTED, before any device is opened. */
int jb_loudness_pcm_batch(const double *const *in, const size_t *n_in, size_t n, uint32_t hz, int32_t device,
                          double *lufs, double *peak_dbfs);
/* The group measurement on PCM the caller holds (jb_loudness_pcm_batch's twin for steps 6 to 8): in[u] (n_in[u]
 * samples at hz) in the groups of group[u] (ids below n or JB_LOUDNESS_NO_GROUP; NULL: every utterance its own),
 * measured on `device` (-1 = current) in peak mode `mode` against target_lufs and ceiling_db.  group_of[u] (may be
 * NULL) = the dense group of utterance u, numbered by first member; groups[g] for g < *n_groups (at most groups_cap
 * are written; JB_ERR_BUFFER if there are more), each with its R128 fields; utt_r128[u] (may be NULL) = each
 * utterance's own R128 fields; utt_lufs[u] (may be NULL) = its own L.  No sample is changed.  The rates of
 * jb_loudness_pcm_batch. */
int jb_loudness_groups_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *group,
                                 uint32_t hz, int32_t device, uint32_t mode, double target_lufs, double ceiling_db,
                                 uint32_t *group_of, jb_loudness_group_report *groups, size_t groups_cap,
                                 size_t *n_groups, jb_loudness_r128 *utt_r128, double *utt_lufs);
/* Host only (no GPU): steps 6 to 8 by the library's rule text, on hop energies the caller holds.  Member m has
 * n_hops[m] full hops of `hop` samples with energies z[m][j] (step 2's z_j), sample peak peak[m] and, in true-peak
 * mode, true_peak[m] (largest magnitudes in 16-bit units; true_peak == NULL: sample mode).  *group = the set's report
 * with its R128 fields (oversampling 0 in true-peak mode: no rate is given); member_r128 (may be NULL) = each
 * member's own R128 fields. */
int jb_loudness_gate_host(const double *const *z, const size_t *n_hops, size_t n, uint32_t hop, const double *peak,
                          const double *true_peak, double target_lufs, double ceiling_db,
                          jb_loudness_group_report *group, jb_loudness_r128 *member_r128);
/* Host only (no GPU): the interpolator of step 5 at hz: *F, *ntaps = 12 (each may be NULL) and, when taps is not NULL,
 * the [F - 1][12] taps h[p][j] of phases p = 1..F-1 (JB_ERR_BUFFER if cap < (F - 1) * 12).  hz == 0: JB_ERR_INVALID. */
int jb_true_peak_filter(uint32_t hz, uint32_t *F, uint32_t *ntaps, double *taps, size_t cap);
/* jb_loudness_pcm_batch's twin for step 5: true_peak_dbtp[u] = TP of in[u] (n_in[u] samples at hz), on `device`
 * (-1 = current).  The tiling is the measurement's: a hop outside 1..61439 samples is JB_ERR_UNSUPPORTED; the lower
 * limit of the loudness values (step 1) does not apply. */
int jb_true_peak_pcm_batch(const double *const *in, const size_t *n_in, size_t n, uint32_t hz, int32_t device,
                           double *true_peak_dbtp);

/* ---- FLAC (new: the reference writes WAV only; RFC 9639) ---------------------------------------------------------
 * Each utterance's 16-bit output (exactly what jb_batch_read_pcm_i16 hands out: after the converter, the loudness
 * apply pass or the fused sink) becomes one complete FLAC stream; decoding it gives those samples bit for bit.
 * - Layout: "fLaC", one STREAMINFO block (marked last unless a SEEKTABLE follows), then frames.  Mono, 16 bits, at
 *   the utterance's output rate (jb_batch_output_rate).  Fixed block size with frame-number headers: every frame has block_size samples but the
 *   last, which may be shorter.
 * - STREAMINFO: min = max block size = block_size; min / max frame size the true values of the stream (0 with no
 *   frames); total samples exact; MD5 all zero ("not computed", which the format allows) unless JB_FLAC_MD5 asks for
 *   it.
 * - MD5 (JB_FLAC_MD5; RFC 1321): of the utterance's 16-bit samples as little-endian bytes, 2 N of them -- FLAC's
 *   definition for mono 16-bit -- in STREAMINFO bytes 18..33 in RFC 1321's output order.  Computed on the device from
 *   the PCM the stream encodes (in FLAC mode the host never holds it), one chain per utterance, the batch in
 *   parallel; a redo round's utterances are hashed again from their final PCM.
 * - SEEKTABLE (seek_interval_ms > 0): with block size bs and rate hz the step in frames is
 *   max(1, (seek_interval_ms hz + 500 bs) / (1000 bs)) in integer division, raised to ceil(frames / 65535) where that
 *   is larger; the points are the frames 0, step, 2 step, ... (ceil(frames / step) of them, ascending, no
 *   placeholders), each 18 bytes big-endian: u64 first sample f bs, u64 byte offset of frame f's header from the first
 *   frame's header, u16 samples of the frame.  The stream is then "fLaC", STREAMINFO (not marked last), one
 *   SEEKTABLE block (type 3, marked last, 18 bytes per point), the frames; a stream without frames has no table.
 *   The header is 42 + (points ? 4 + 18 points : 0) bytes (jb_flac_seek_geometry).  The frames' bytes are the same
 *   with and without either request.
 * - Every stream is in the streamable subset: block size <= 4608, LPC order <= 12, Rice partition order <= 8, and
 *   the sample rate and bit depth coded in every frame header.  A rate without a code of its own uses the kHz,
 *   16-bit-Hz or tens-of-Hz form; a rate none of them can express is JB_ERR_UNSUPPORTED when FLAC is requested
 *   (every rate up to 65,535 Hz has a code, and so do 88.2, 96, 176.4 and 192 kHz).
 * - Subframes: a block of equal samples is CONSTANT; otherwise the cheapest of VERBATIM, FIXED orders 0-4 and LPC
 *   at the orders 2, 4, 8 and max_lpc_order (those <= max_lpc_order and below the block length; Tukey(0.5) window,
 *   autocorrelation, Levinson-Durbin, precision 7..12 bits by block length, shift 0..15) with partitioned Rice
 *   residuals (4- or 5-bit parameters, chosen by libFLAC's estimate; the winner priced exactly).  A frame is never
 *   larger than its VERBATIM encoding.  Wasted-bits flag 0.  An LPC candidate whose residual does not fit in 32
 *   bits is dropped.
 * - Determinism: a stream's bytes depend only on its samples, its rate, the options and the library build (every
 *   f64 step runs in a fixed order and ties break by a fixed rule), not on the batch, the utterance's position, the
 *   entry point or redo rounds; JB_BATCH_INVARIANT output stays invariant.
 * Not covered: the generator (it hands out f64), the _multi entries and jb_gather_pcm, f64 batches, 24-bit or
 * stereo, VORBIS_COMMENT and ReplayGain tags, PADDING and other metadata, variable block size, Ogg encapsulation,
 * lossy codecs. */
/* The encoder on PCM the caller holds (jb_resample_pcm_batch's twin): out[u] = the stream of in[u] (n_in[u] samples
 * at hz), n_out[u] bytes, library-owned (jb_flac_free each), on `device` (-1 = current).  The same samples and
 * options give the same bytes as the batch path. */
int jb_flac_encode_pcm_batch(const int16_t *const *in, const size_t *n_in, size_t n, uint32_t hz,
                             const jb_flac_opts *opts, int32_t device, uint8_t **out, size_t *n_out);
/* New.  The same with a metadata request (meta NULL or zeros: jb_flac_encode_pcm_batch itself). */
int jb_flac_encode_pcm_batch_meta(const int16_t *const *in, const size_t *n_in, size_t n, uint32_t hz,
                                  const jb_flac_opts *opts, const jb_flac_meta *meta, int32_t device, uint8_t **out,
                                  size_t *n_out);
/* New.  The device's MD5 alone: digests[16 u ..] = MD5 of in[u]'s n_in[u] samples as little-endian bytes, on
 * `device` (-1 = current). */
int jb_flac_md5_pcm_batch(const int16_t *const *in, const size_t *n_in, size_t n, int32_t device, uint8_t *digests);
/* New.  The same rules in plain C++ on the host, no GPU touched: MD5 (RFC 1321) of n_bytes bytes, and the SEEKTABLE
 * geometry of a stream of n_samples at block_size (0: 4096) and hz: frames between two points (0 without a table),
 * points, bytes in front of the first frame.  Any output pointer of the geometry may be NULL. */
int jb_md5_host(const void *data, size_t n_bytes, uint8_t digest[16]);
int jb_flac_seek_geometry(uint64_t n_samples, uint32_t block_size, uint32_t hz, uint32_t seek_interval_ms,
                          uint32_t *step_frames, uint32_t *n_points, uint32_t *header_bytes);
void jb_flac_free(uint8_t *p);

/* ---- Output sample formats (new: the reference hands out f64 and its examples clamp and truncate to 16 bits) -------
 * v is the final f64 sample in 16-bit scale (what jb_batch_read_pcm hands out).
 * - JB_FMT_F32: (float)(v * 2^-15); the product is exact, one round-to-nearest-even f64 -> f32; no clamp.
 * - JB_FMT_S16: q(v) in [-32768, 32767].  JB_FMT_S24: q(256 v) in [-8388608, 8388607], little-endian, packed.
 * - JB_FMT_ULAW / JB_FMT_ALAW: G.711 of s = q(v) at 16 bits without dither, with the semantics of the common C
 *   implementation (14-bit mu-law with the clip at 8159 and the bias 33, 13-bit A-law): mu-law never emits 0x7F.
 * - q(x) without dither is the 16-bit sink's rule: fmin to the upper bound, fmax to the lower, truncate toward zero;
 *   JB_FMT_S16 is then bit for bit what a JB_BATCH_PCM_I16 batch hands out, and S24 truncated by 256 equals S16.
 *   With JB_DITHER_TPDF: floor((x + d) + 0.5) (two f64 additions in that order), then the clamp.
 * - d = ((double)(r >> 32) - (double)(r & 0xffffffff)) * 2^-32, triangular in (-1, 1) LSB; r = mix(mix(seed) ^ k),
 *   k the sample's 0-based index within its utterance's output, mix the splitmix64 finaliser (z += 0x9E3779B97F4A7C15;
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31).  An utterance's
 *   bytes depend on its samples, the options and the seed, not on the batch, its position in it or redo rounds.
 * Not covered: the generator (it hands out f64), the _multi entries and jb_gather_pcm, per-utterance formats within
 * one batch, S32, U8 and big-endian, noise shaping (a serial nonlinear recursion), dither on the fused 16-bit sink. */
size_t jb_format_bytes_per_sample(uint32_t format); /* 0 for an unknown format */
/* The stage on PCM the caller holds (jb_resample_pcm_batch's twin): out[u] = the bytes of in[u], n_bytes[u] of them,
 * library-owned (jb_format_free each), on `device` (-1 = current). */
int jb_format_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_format_opts *opts,
                        int32_t device, uint8_t **out, size_t *n_bytes);
void jb_format_free(uint8_t *p);
/* The same rules in plain C++ on the host; no GPU is touched.  out must hold n x jb_format_bytes_per_sample bytes
 * (cap below that: JB_ERR_BUFFER).  The same samples and options give the same bytes from both seams and from the
 * batch path. */
int jb_format_pcm_host(const double *in, size_t n, const jb_format_opts *opts, uint8_t *out, size_t cap);

/* ---- IMA ADPCM (new: the reference writes 16-bit WAV only; WAV format tag 0x0011, mono) --------------------------------
 * Half a byte per sample at any rate.  A WAV ADPCM block carries its own predictor and step index, and here every
 * block picks its start index from its own first samples instead of carrying it from the block before (as the serial
 * encoders do), so blocks are independent: one GPU lane encodes one block.
 * - Geometry: block size A bytes (jb_adpcm_opts); samples per block spb = 2 (A - 4) + 1; ceil(n / spb) blocks of A
 *   bytes for n samples, 0 bytes for n = 0.  The last block is padded by repeating the last sample.
 * - Input: s[k] = the 16-bit sink's rule on the final f64 (fmin to 32767, fmax to -32768, truncate toward zero; no
 *   dither), or the 16-bit sample itself on a JB_BATCH_PCM_I16 batch; the two are equal.
 * - Block header: bytes 0-1 the block's first sample b[0] (little-endian int16), byte 2 the start index i0, byte 3
 *   zero.  i0 is the smallest i with STEP[i] >= d, d = floor((sum_{k=1..8} |b[k] - b[k-1]|) / 8), and 88 if none.
 * - Each further sample b[k], from pred = b[0], idx = i0: step = STEP[idx]; diff = b[k] - pred; sign = diff < 0 ? 8 : 0;
 *   diff = |diff|; delta = 0; vp = step >> 3; three times {if (diff >= step) set the bit (4, 2, 1), diff -= step,
 *   vp += step; step >>= 1}; pred = clamp(pred -/+ vp to int16); idx = clamp(idx + IDX[delta], 0, 88);
 *   code = delta | sign.  IDX = {-1, -1, -1, -1, 2, 4, 6, 8}; STEP is the standard 89-entry IMA table (7 .. 32767).
 *   Byte 4 + j holds the code of sample 2j + 1 in its low nibble and that of sample 2j + 2 in its high nibble.  The
 *   decoder builds the same vp from the code's bits (jb_adpcm_decode_host; any WAV player).
 * - Determinism: a stream's bytes depend only on its samples, its rate and A, not on the batch, the utterance's
 *   position in it, the entry point or redo rounds; JB_BATCH_INVARIANT output stays invariant.
 * - Cost on 256 x 128 s (profiles/r14_adpcm.txt): 0.502 bytes per sample at A = 1024; the encoder takes 1.67 ms of
 *   device time from the 16-bit slab and 4.19 ms from f64 (a 16-bit format pass of the same batch: 2.64 ms); run + read
 *   of everything 292 ms at 48 kHz (16-bit PCM: 151 ms) and 140 ms at 8 kHz (mu-law: 191 ms): the read is one
 *   pageable copy.
 * Not covered: the generator (it hands out f64), the _multi entries and jb_gather_pcm, stereo, Microsoft ADPCM
 * (tag 2), a trial search over start indices, reading through the pinned ring (the read is one pageable copy). */
/* A (block_align 0: by hz), samples per block, blocks and bytes of n samples; any out pointer may be NULL.  A bad
 * block_align: JB_ERR_INVALID. */
int jb_adpcm_geometry(uint32_t hz, uint32_t block_align, size_t n, uint32_t *A, uint32_t *spb, size_t *n_blocks,
                      size_t *n_bytes);
/* The encoder in plain C++ on the host; no GPU is touched.  out must hold the geometry's bytes (cap below that:
 * JB_ERR_BUFFER).  The same samples, rate and options give the same bytes from the host, the seam and the batch. */
int jb_adpcm_encode_host(const double *in, size_t n, uint32_t hz, const jb_adpcm_opts *opts, uint8_t *out, size_t cap);
int jb_adpcm_encode_i16_host(const int16_t *in, size_t n, uint32_t hz, const jb_adpcm_opts *opts, uint8_t *out,
                             size_t cap);
/* The decoder on the host: the first n_samples samples of n_bytes bytes of blocks of A bytes (cap below n_samples:
 * JB_ERR_BUFFER; fewer blocks than n_samples need, or a bad A: JB_ERR_INVALID). */
int jb_adpcm_decode_host(const uint8_t *bytes, size_t n_bytes, uint32_t A, size_t n_samples, int16_t *out, size_t cap);
/* The stage on PCM the caller holds (jb_format_pcm_batch's twin): out[u] = the blocks of in[u] (n_in[u] f64 samples at
 * hz[u]), n_bytes[u] of them, library-owned (jb_adpcm_free each), on `device` (-1 = current). */
int jb_adpcm_encode_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                              const jb_adpcm_opts *opts, int32_t device, uint8_t **out, size_t *n_bytes);
void jb_adpcm_free(uint8_t *p);

/* ---- Filterbank features (new: the reference hands out samples only; none of these entries has a counterpart) ---------
 * A bulk consumer (ASR corpora, distillation, alignment, QA) takes log-mel frames, not samples: n_mels numbers per hop.
 * The stage reads the final f64 PCM on the device and hands out the frames; a programme (jb_batch_set_join) is
 * analysed whole.
 * - Geometry, per unit at its own output rate hz, in 64-bit integers: wl = (hz win_us + 500000) / 1000000, hop the
 *   same from hop_us.  Limits: 2 <= wl <= n_fft, n_fft a power of two in 64..4096 (0: the smallest one >= wl, which
 *   must lie in that range), hop >= 1, 1 <= n_mels <= 128, 0 <= f_min < f_max <= hz / 2.
 * - Frames: without JB_FBANK_CENTER T = n >= wl ? 1 + (n - wl) / hop : 0 and frame t is samples [t hop, t hop + wl);
 *   with it T = ceil(n / hop), frame t starts at t hop - wl / 2 (integer division) and samples outside [0, n) read as
 *   0: zero padding, not reflection.
 * - Samples are in 16-bit scale, as jb_batch_read_pcm hands them out; JB_FBANK_UNIT multiplies each by 2^-15 (exact).
 * - Window: JB_FBANK_HANN is periodic, 0.5 - 0.5 cos(2 pi j / wl); JB_FBANK_HAMMING symmetric, 0.54 - 0.46 cos(2 pi j /
 *   (wl - 1)); computed on the host in long double and rounded to f64 once (jb_fbank_window).
 * - Spectrum: X_k = sum_j w_j x_j e^{-2 pi i j k / n_fft}, k = 0..n_fft / 2; P_k = re^2 + im^2.  f64 throughout; the
 *   twiddles come from a host table (long double, rounded once), never from the device's sincos.
 * - Filterbank: mel(f) = 1127 ln(1 + f / 700) (the HTK form); n_mels + 2 edges equally spaced in mel from mel(f_min) to
 *   mel(f_max): edge i = lo + (hi - lo) i / (n_mels + 1); W[m][k] = max(0, min((mu_k - l) / (c - l), (r - mu_k) /
 *   (r - c))) with mu_k = mel(k hz / n_fft) and l, c, r edges m, m + 1, m + 2; no area normalisation; a filter that
 *   covers no bin is allowed, its energy is 0.  Built on the host in long double, rounded once (jb_fbank_filterbank).
 *   E_m = sum_k W[m][k] P_k, summed in ascending k over the filter's support.
 * - Output: element [t][m], row-major per unit, is E_m under JB_FBANK_LINEAR, else ln(max(E_m, log_floor)); f32 (one
 *   round-to-nearest from the f64 value) unless JB_FBANK_F64.  A unit starts on a 16-byte boundary of the slab.
 * - Determinism: a frame's values depend on its own wl samples, hz and the options only; the order of every operation
 *   is fixed per (n_fft, wl, n_mels).  Hence the seam (jb_fbank_pcm_batch), the batch path, redo rounds and any batch
 *   give the same bits, and JB_BATCH_INVARIANT output stays invariant.  The host form (jb_fbank_host) follows the same
 *   rule to the precision of f64 arithmetic; bit equality with the device is not claimed (the logarithm is each
 *   side's own).
 * - Cost on 256 x 128 s at 25 / 10 ms and 80 filters (profiles/r20_fbank.txt): 0.667 bytes per sample in f32; the
 *   kernel takes 43.7 ms of device time at 48 kHz (3.27 million frames of 2048 points) and 11.4 ms at 16 kHz; run + read
 *   of everything 430 ms (the f64 samples: 353 ms): the read is one pageable copy.  Against the long double model the
 *   device's error is 1.00 to 1.25 times (3.88 with one filter alone) that of a float64 rfft of the same frames.
 * Not covered: the Slaney mel scale, reflection padding and magnitude instead of power (these are the "Mel
 * spectrograms" stage below); dither (pre-emphasis, per-frame DC removal, the symmetric windows and reflected edges are
 * the "Frame conditioning" section below); the generator, the _multi entries and jb_gather_pcm; 16-bit batches; per-utterance options within one batch;
 * reading through the pinned ring (the read is one pageable copy). */
/* wl, hop, n_fft of the options at hz and T and bytes of n samples; any out pointer may be NULL. */
int jb_fbank_geometry(uint32_t hz, const jb_fbank_opts *opts, size_t n, uint32_t *wl, uint32_t *hop, uint32_t *n_fft,
                      size_t *T, size_t *n_bytes);
/* The window (wl doubles) and the filterbank (dense [n_mels][n_fft / 2 + 1]) the options give at hz; cap (in doubles)
 * below that: JB_ERR_BUFFER. */
int jb_fbank_window(uint32_t hz, const jb_fbank_opts *opts, double *w, size_t cap);
int jb_fbank_filterbank(uint32_t hz, const jb_fbank_opts *opts, double *W, size_t cap);
/* The rule in plain C++ on the host; no GPU is touched.  out must hold the geometry's bytes (cap below that:
 * JB_ERR_BUFFER). */
int jb_fbank_host(const double *in, size_t n, uint32_t hz, const jb_fbank_opts *opts, uint8_t *out, size_t cap);
/* The stage on PCM the caller holds (jb_format_pcm_batch's twin): out[u] = the frames of in[u] (n_in[u] f64 samples at
 * hz[u]), n_bytes[u] bytes, library-owned (jb_fbank_free each), on `device` (-1 = current). */
int jb_fbank_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                       const jb_fbank_opts *opts, int32_t device, uint8_t **out, size_t *n_bytes);
void jb_fbank_free(uint8_t *p);

/* ---- Cepstral features (new: the reference hands out samples only; none of these entries has a counterpart) -----------
 * What a Kaldi / HTK / ESPnet-style front end reads behind the filterbank: cepstra (a liftered DCT of the log-mel
 * energies), delta and delta-delta rows, normalised per unit (CMVN); with n_ceps = 0 the same deltas and CMVN on the
 * log-mel itself.  A unit is what the caller hands in as one: an utterance, or a programme.  For a unit of T frames:
 * 1. Log-mel.  L[t][m] is the filterbank stage's f64 logarithms: the jb_fbank_opts of the request with JB_FBANK_F64 and
 *    without JB_FBANK_LINEAR.  A caller's JB_FBANK_LINEAR or JB_FBANK_F64 in it is refused, naming `flags`.  The device
 *    entries run the filterbank kernel unchanged: these are its bits.
 * 2. Cepstra.  With n_ceps in 1..n_mels, for i < n_ceps: c[t][i] = l_i (sum_m D[i][m] L[t][m]), the sum from 0.0 in
 *    ascending m.  D is the orthonormal DCT-II of N = n_mels points: D[0][m] = sqrt(1 / N), D[i][m] = sqrt(2 / N)
 *    cos(pi i (m + 0.5) / N).  l_i = 1 + (Q / 2) sin(pi i / Q) for a lifter Q > 0, 1 for Q = 0.  D and l are made on the
 *    host in long double and rounded once (jb_mfcc_dct).  n_ceps = 0: c = L.  d is the static width: n_ceps, or n_mels.
 * 3. CMVN, per unit and dimension.  JB_CMVN_MEAN: c' = c - mu.  JB_CMVN_MEAN_VAR: c' = (c - mu) / sqrt(max(var,
 *    var_floor)); var is the population variance, the mean of (c - mu)^2 (two passes).  A mean is taken in an order that
 *    is a function of T alone: the sums of consecutive blocks of 64 frames, each from 0.0 in ascending t; the block sums
 *    from 0.0 in ascending order; times r_T = (double)(1.0L / T), which comes from the host.  T = 0 writes nothing;
 *    T = 1 under MEAN_VAR gives zeros.
 * 4. Deltas, as Kaldi's add-deltas has them (not a regression applied twice with two clamps): with N = delta_window,
 *    g[k] = k / sum_{j=-N..N} j^2, s_0 = [1], s_q = s_{q-1} * g (full convolution, 2 q N + 1 values), made on the host
 *    in long double and rounded once (jb_mfcc_delta_kernel).  out_q[t][i] = sum_{j=-qN..qN} s_q[j] c'[clamp(t + j, 0,
 *    T - 1)][i], from 0.0 in ascending j, on the normalised statics.
 * 5. Output.  Row t is [c' | out_1 | out_2], d (delta_order + 1) elements, row-major per unit; f32 (one
 *    round-to-nearest from the f64 value) or f64 with JB_MFCC_F64.
 * 6. Arithmetic.  f64 throughout, every product and sum on its own (no contraction); the device calls no transcendental
 *    but the one sqrt of MEAN_VAR.  Hence jb_mfcc_frames_batch equals jb_mfcc_host bit for bit under JB_CMVN_NONE and
 *    JB_CMVN_MEAN, and a frame's values depend on its unit's frames and the options only, not on the other units of the
 *    call, the place in the slab or the lanes that share the work.
 * Precision (tests/mfcc_ref.py): against a long double model, with each element's error divided by the same pipeline
 * run on absolute values, the host and the device stay within 8 times the error of a plain float64 numpy model.
 * Cost on 256 x 128 s at 25 / 10 ms, 80 filters, 13 cepstra, order 2, MEAN_VAR (profiles/r22_mfcc.txt): 46.7 ms of
 * device time, 43.6 ms of them the filterbank pass and 3.0 ms the cepstral kernels; run + read of everything 286 ms
 * (the f64 samples: 351 ms).
 * In a batch (jb_batch_set_mfcc) the stage runs beside the other encoders on the final f64 PCM: the filterbank kernel
 * into an f64 log-mel scratch slab, then the cepstral kernels; a unit's rows start on a 16-byte boundary of the
 * feature slab.  A redo round recomputes every unit it touched whole, statistics included, so the rows are the seam's
 * on the final PCM, and JB_BATCH_INVARIANT output stays invariant.
 * Not covered: sharing one filterbank pass between an fbank and an mfcc request; 16-bit batches; reading through the
 * pinned ring (the read is one pageable copy); HTK's unnormalised DCT; sliding-window or global (corpus) CMVN; fusing
 * the DCT into the filterbank kernel (frame energy in place of c0, pre-emphasis, DC removal and the Povey window are
 * the "Frame conditioning" section below); the generator, the _multi entries and jb_gather_pcm. */
/* T (the filterbank's), the row width d (delta_order + 1) and the bytes of n samples at hz; any out pointer may be
 * NULL. */
int jb_mfcc_geometry(uint32_t hz, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts, size_t n, size_t *T,
                     uint32_t *width, size_t *n_bytes);
/* D (dense [n_ceps][n_mels], cap_D doubles) and the lifter (n_ceps doubles, cap_l) of the options; either pointer may
 * be NULL; a cap below that: JB_ERR_BUFFER.  n_ceps = 0 writes nothing. */
int jb_mfcc_dct(uint32_t n_mels, const jb_mfcc_opts *opts, double *D, size_t cap_D, double *lifter, size_t cap_l);
/* s_q[-qN..qN] of order q in 0..2 and window N in 1..5: 2 q N + 1 doubles (cap below that: JB_ERR_BUFFER). */
int jb_mfcc_delta_kernel(uint32_t q, uint32_t N, double *s, size_t cap);
/* The rule from step 2 on in plain C++ on the host, from T f64 log-mel frames [T][n_mels]; no GPU is touched.  out must
 * hold T x width x 4 (8) bytes (cap below that: JB_ERR_BUFFER). */
int jb_mfcc_host(const double *L, size_t T, uint32_t n_mels, const jb_mfcc_opts *opts, uint8_t *out, size_t cap);
/* The whole rule on the host, from n samples at hz through jb_fbank_host. */
int jb_mfcc_pcm_host(const double *in, size_t n, uint32_t hz, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts,
                     uint8_t *out, size_t cap);
/* The stage from step 2 on, on log-mel frames the caller holds: out[u] = the rows of L[u] ([T[u]][n_mels] f64),
 * n_bytes[u] bytes, library-owned (jb_mfcc_free each), on `device` (-1 = current). */
int jb_mfcc_frames_batch(const double *const *L, const size_t *T, size_t n, uint32_t n_mels, const jb_mfcc_opts *opts,
                         int32_t device, uint8_t **out, size_t *n_bytes);
/* The whole stage on PCM the caller holds (jb_fbank_pcm_batch's twin): in[u] is n_in[u] f64 samples at hz[u]. */
int jb_mfcc_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                      const jb_fbank_opts *fopts, const jb_mfcc_opts *opts, int32_t device, uint8_t **out,
                      size_t *n_bytes);
void jb_mfcc_free(uint8_t *p);

/* ---- Frame conditioning (new: the reference hands out samples only; none of these entries has a counterpart) ----------
 * What a Kaldi, lhotse or WeNet recipe does to a frame in front of the transform (Kaldi's ExtractWindow / ProcessWindow,
 * without dither), as a request (jb_frame_opts) beside the filterbank and cepstral options.  For one frame of wl values
 * of a unit of n samples, in this order:
 * 1. Samples.  v_i = x[k(i)] * scale; the scale is JB_FBANK_UNIT's, applied first.  Without JB_FRAME_REFLECT the frame
 *    starts, T and the zeros outside the unit are the filterbank stage's (snip, or JB_FBANK_CENTER).  With it T =
 *    (n + hop / 2) / hop, frame t starts at t hop + hop / 2 - wl / 2 (integer divisions), and an index k outside [0, n)
 *    is mapped by k < 0 ? -k - 1 : 2 n - 1 - k, repeated until it lies inside (a unit shorter than half a window
 *    reflects more than once).  JB_FRAME_REFLECT together with JB_FBANK_CENTER is refused, naming `flags`.
 * 2. DC (JB_FRAME_REMOVE_DC).  p_j (j = 0..63) is the sum of v_i over i = j (mod 64), from 0.0 in ascending i; then for
 *    w = 32, 16, .., 1: p_j = p_j + p_{j+w} for j < w; mean = p_0 / (double)wl (a division: a constant integer-valued
 *    frame gives exactly its value); v_i -= mean.  In JB_FBANK_CENTER mode the padded zeros belong to the frame.  The
 *    order is a function of wl alone, not of n_fft or of the lanes that share the frame.
 * 3. Energy (JB_FRAME_ENERGY).  e = sum v_i^2 in the order of step 2, each square rounded on its own: the "raw" energy,
 *    after DC removal, before pre-emphasis and the window.
 * 4. Pre-emphasis (preemph = c > 0).  y_0 = v_0 - c v_0, y_i = v_i - c v_{i-1}, from the values of step 2; the product
 *    is rounded, then the difference (no contraction).
 * 5. Window.  z_i = w_i y_i; the table is made on the host in long double and rounded once (jb_frame_window).
 *    JB_FRAME_WINDOW_OPTS gives the jb_fbank_opts window's table bit for bit.
 * Spectrum, filterbank, floor, logarithm and element type follow unchanged ("Filterbank features").  With
 * JB_FRAME_ENERGY, c[t][0] = ln(max(e, log_floor)) replaces the DCT's row 0 in front of CMVN and the deltas; the
 * lifter's l_0 is 1.
 * Refused, naming the field, before any device is touched: JB_FRAME_ENERGY with an fbank request or with n_ceps = 0
 * (`flags`); an unknown window or flag; a reserved word that is not 0; preemph outside [0, 1] or not finite.
 * An all-zero jb_frame_opts is the identity: every entry that takes one then returns the bytes of its counterpart
 * without it.  Determinism is the filterbank stage's: a frame's values depend on its own samples, hz and the options
 * only, so the seams, the batch path, redo rounds and any batch give the same bits.
 * Cost on 256 x 128 s at 25 / 10 ms and 80 filters (profiles/r27_frame.txt), Povey window, DC removal and pre-emphasis
 * 0.97: k_fbank takes 55.3 ms of device time at 48 kHz against 43.9 ms without the request (3.27 million frames of 2048
 * points, two waves a frame: 16.9 against 13.4 ns a frame, 1.26 times) and 15.1 against 11.4 ms behind the converter at
 * 16 kHz (n_fft 512: 1.32 times); the cepstral stage with the energy 62.3 against 46.5 ms.  What it pays for: two more
 * barriers and one more LDS round trip per frame.  Without a request the kernel is the one it was (43.9 ms; the default
 * step 77.63 ms against the parent's 77.60 ms, medians of three alternating runs, 77.55 .. 77.77 ms in all).  Against the
 * long double model the device's error is 0.59 to 3.04 times that of a float64 numpy model of the same frames (the host
 * form's: at most 3.61; gate 8).
 * Not claimed: bit-compatibility with Kaldi (Kaldi works in f32 and truncates the window length where this stage rounds
 * it); dither (the noise stage adds white noise to the whole signal instead); an energy column on the fbank sink;
 * raw_energy = false; the melspec stage does not read the request. */
/* compute-fbank-feats' defaults with n_mels filters (23 there) into *f and *fr: 25 / 10 ms, the Povey window, DC
 * removal, pre-emphasis 0.97, f_min 20 Hz, floor 2^-23, snip framing, no energy. */
int jb_frame_kaldi(uint32_t n_mels, jb_fbank_opts *f, jb_frame_opts *fr);
/* The request beside the options it conditions: fopts, and mopts for an mfcc request (NULL: an fbank request). */
int jb_frame_check(const jb_fbank_opts *fopts, const jb_mfcc_opts *mopts, const jb_frame_opts *fr);
/* jb_fbank_geometry with the request: T and the bytes are the reflected ones under JB_FRAME_REFLECT. */
int jb_fbank_framed_geometry(uint32_t hz, const jb_fbank_opts *opts, const jb_frame_opts *fr, size_t n, uint32_t *wl,
                             uint32_t *hop, uint32_t *n_fft, size_t *T, size_t *n_bytes);
/* The window of step 5 (wl doubles; cap below that: JB_ERR_BUFFER). */
int jb_frame_window(uint32_t hz, const jb_fbank_opts *opts, const jb_frame_opts *fr, double *w, size_t cap);
/* The rule on the host (jb_fbank_host's and jb_mfcc_pcm_host's twins); no GPU is touched. */
int jb_fbank_framed_host(const double *in, size_t n, uint32_t hz, const jb_fbank_opts *opts, const jb_frame_opts *fr,
                         uint8_t *out, size_t cap);
int jb_mfcc_framed_pcm_host(const double *in, size_t n, uint32_t hz, const jb_fbank_opts *fopts,
                            const jb_mfcc_opts *opts, const jb_frame_opts *fr, uint8_t *out, size_t cap);
/* The stages on PCM the caller holds (jb_fbank_pcm_batch's and jb_mfcc_pcm_batch's twins); out[u] is library-owned
 * (jb_fbank_free, jb_mfcc_free). */
int jb_fbank_framed_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                              const jb_fbank_opts *opts, const jb_frame_opts *fr, int32_t device, uint8_t **out,
                              size_t *n_bytes);
int jb_mfcc_framed_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                             const jb_fbank_opts *fopts, const jb_mfcc_opts *opts, const jb_frame_opts *fr,
                             int32_t device, uint8_t **out, size_t *n_bytes);

/* ---- Mel spectrograms (new: the reference hands out samples only; none of these entries has a counterpart) ------------
 * The filterbank stage above speaks Kaldi / HTK.  Everything neural reads the other dialect -- what librosa's
 * melspectrogram, torchaudio's MelSpectrogram and Whisper's log_mel_spectrogram compute: a centred, reflected
 * short-time transform of any 5-smooth length with window and hop in samples, triangles that are linear in Hz between
 * mel-spaced edges, Slaney's scale and area normalisation, log10 or dB, and a clamp against the unit's own maximum.
 * For a unit of n samples x (16-bit scale, as jb_batch_read_pcm hands them out) at rate hz:
 * 1. Scale.  s[i] = x[i] * 2^-15 (exact); this stage has no 16-bit scale.
 * 2. Sizes.  N = n_fft is even, in 64..4096, without a prime factor above 5 (400, 480, 600, 800, 1024, 1200, 2048,
 *    4000, ...); W = win_length is 0 (N) or in 2..N; H = hop_length >= 1; all in samples at the unit's own rate.
 * 3. Frames.  With p = N / 2: under JB_MEL_PAD_REFLECT and _ZERO T = 1 + n / H (integer division) and frame t is
 *    s~[t H - p + j], j < N; _ZERO: s~ is 0 outside the unit; _REFLECT: s~[-j] = s[j], s~[n - 1 + j] = s[n - 1 - j] (the
 *    edge sample is not repeated), which needs n > p: a shorter unit has T = 0.  Under _NONE frame t is s[t H + j] and
 *    T = n >= N ? 1 + (n - N) / H : 0.  JB_MEL_DROP_LAST drops the last frame under _REFLECT and _ZERO (T one less, not
 *    below 0); with _NONE it is refused.
 * 4. Window.  Periodic Hann of W points, 0.5 - 0.5 cos(2 pi j / W), at (N - W) / 2 inside the frame with zeros around
 *    it (torch.stft's placement); made on the host in long double and rounded once (jb_melspec_window).
 * 5. Spectrum.  X_k, k = 0..N / 2, of the windowed frame; S_k = |X_k|^2, or |X_k| with JB_MEL_MAGNITUDE.  f64
 *    throughout; the twiddles come from host tables (long double, rounded once).
 * 6. Filters.  n_mels + 2 points equally spaced on the mel scale between mel(f_min) and mel(f_max) -- JB_MEL_HTK:
 *    2595 log10(1 + f / 700); JB_MEL_SLANEY: 3 f / 200 below 1 kHz, 15 + ln(f / 1000) / (ln 6.4 / 27) above -- and
 *    converted back to Hz: f_0 .. f_{n_mels+1}.  With nu_k = k hz / N, W[m][k] = max(0, min((nu_k - f_m) / (f_{m+1} -
 *    f_m), (f_{m+2} - nu_k) / (f_{m+2} - f_{m+1}))); JB_MEL_NORM_SLANEY multiplies it by 2 / (f_{m+2} - f_m).  Made on
 *    the host in long double, rounded once (jb_melspec_filterbank).  E[t][m] = sum_k W[m][k] S_k in ascending k; a
 *    filter that covers no bin gives 0.  1 <= n_mels <= 128, 0 <= f_min < f_max <= hz / 2.
 * 7. Logarithm.  _NONE: y = E; _LN: ln(max(E, floor)); _LOG10: log10(max(E, floor)); _DB: 10 log10(max(E, floor)).  An
 *    E at or below the floor gives the floor's logarithm as made on the host in long double and rounded once.
 * 8. Range.  If range > 0: y = max(y, Ymax - range), Ymax the largest y of the whole unit (behind a join: of the whole
 *    programme), in f64.
 * 9. Affine and element.  out = (y + offset) * scale, one f64 add and one f64 multiply without contraction; the
 *    element is f32 by one rounding, or f64 with JB_MEL_F64.  Row-major [T][n_mels] per unit.
 * Whisper's front end (jb_melspec_whisper): 400 / 400 / 160, reflect padding, drop-last, power spectrum, Slaney scale
 * and norm, 0..8000 Hz, log10, floor 1e-10, range 8, offset 4, scale 0.25; the caller sets the output rate to 16 kHz.
 * Determinism: a frame's operations and their order are a function of (N, W, n_mels, options) alone; the maximum of
 * step 8 has no order.  Hence the seam (jb_melspec_pcm_batch), the batch path, redo rounds and any batch give the same
 * bits, and JB_BATCH_INVARIANT output stays invariant.  The host form (jb_melspec_host) follows the same rule with the
 * same butterflies; bit equality with the device is not claimed (the logarithm is each side's own).
 * Cost on 256 x 128 s with 80 filters (profiles/r24_melspec.txt): N = 1200, H = 480 at 48 kHz takes 58.7 ms of device
 * time (3.27 million frames; 63.1 ms with a range), k_fbank's 2048-point pass on the same frames 43.9 ms; Whisper's front
 * end behind the converter at 16 kHz 24.4 ms; 0.667 bytes per sample in f32 at 48 kHz; run + read of everything 444 ms
 * (the f64 samples: 353 ms).  Against the long double model the device's error is 0.66 to 1.92 times that of a float64
 * rfft of the same frames.
 * Not covered: HiFi-GAN's own (N - H) / 2 padding; windows other than Hann; pre-emphasis and dither; Whisper's padding
 * or trimming to 30 s; the generator, the _multi entries and jb_gather_pcm; 16-bit batches; per-utterance options
 * within a batch; reading through the pinned ring (the read is one pageable copy). */
/* Whisper's options with n_mels filters (80 or 128 in its models; any 1..128 is taken) into *opts. */
int jb_melspec_whisper(uint32_t n_mels, jb_melspec_opts *opts);
/* N, W, H of the options at hz and T and bytes of n samples; any out pointer may be NULL. */
int jb_melspec_geometry(uint32_t hz, const jb_melspec_opts *opts, size_t n, uint32_t *n_fft, uint32_t *win_length,
                        uint32_t *hop_length, size_t *T, size_t *n_bytes);
/* The window as the frame sees it (N doubles: the W Hann values at (N - W) / 2, zeros around them) and the filterbank
 * (dense [n_mels][N / 2 + 1]) the options give at hz; cap (in doubles) below that: JB_ERR_BUFFER. */
int jb_melspec_window(uint32_t hz, const jb_melspec_opts *opts, double *w, size_t cap);
int jb_melspec_filterbank(uint32_t hz, const jb_melspec_opts *opts, double *W, size_t cap);
/* The rule in plain C++ on the host; no GPU is touched.  out must hold the geometry's bytes (cap below that:
 * JB_ERR_BUFFER). */
int jb_melspec_host(const double *in, size_t n, uint32_t hz, const jb_melspec_opts *opts, uint8_t *out, size_t cap);
/* The stage on PCM the caller holds (jb_fbank_pcm_batch's twin): out[u] = the frames of in[u] (n_in[u] f64 samples at
 * hz[u]), n_bytes[u] bytes, library-owned (jb_melspec_free each), on `device` (-1 = current). */
int jb_melspec_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                         const jb_melspec_opts *opts, int32_t device, uint8_t **out, size_t *n_bytes);
void jb_melspec_free(uint8_t *p);

/* ---- Join (new: the reference synthesises one utterance into one buffer; none of these entries has a counterpart) ------
 * A programme is "sentence, pause, sentence" as ONE stream: FLAC frame numbers, STREAMINFO, MD5 and SEEKTABLE, ADPCM
 * blocks and the dither index then run over the whole, which the host cannot make from per-utterance outputs.
 * - Numbering: programmes are numbered densely in the order of their first member; an utterance of JB_JOIN_NONE is a
 *   programme of one and still gets its pads and fades.  Members stand in ascending utterance index.
 * - Geometry: a programme's length is the sum over its members of pad_before + n + pad_after; a member starts at the
 *   running sum plus its own pad_before.  All of it is known on the host once the request is made.
 * - Fade weight: sample k < fade_in of a member is multiplied by s(t), t = (double)(2k + 1) / (double)(2 fade_in),
 *   s = (t * t) * (3.0 - 2.0 * t) (a smoothstep, evaluated as written in f64 without contraction: bit-exact on the host
 *   and the device); the fade-out the same with k' = n - 1 - k < fade_out.  Where both reach one sample (fade_in +
 *   fade_out > n is allowed): x * s_in * s_out in that order.  From f64 the product stays f64; from 16 bits it is
 *   truncated toward zero to int16 (the weights are in [0, 1]: no clamp).  Samples outside both fades are copied bit
 *   for bit; pads are zeros.
 * - Independence: a member's samples in the programme depend on its own samples and its two fade lengths alone, not on
 *   the batch, the programme, its position or redo rounds; JB_BATCH_INVARIANT output stays invariant.
 * - Loudness is measured on the members, in front of the pads; with jb_batch_set_loudness_groups over the same
 *   members the programme has one gain.
 * - Cost: not measured yet.
 * Not covered: the generator, the _multi entries and jb_gather_pcm, the _each forms at engine level, a caller-chosen
 * member order, FLAC CUESHEET / VORBIS_COMMENT blocks and seek points at member starts, loudness measured over the
 * joined programme, reading through the pinned ring.  (Overlapping members, a crossfade: "Mix" below.) */
/* New (none).  floor(ms * hz / 1000.0 + 0.5): a duration in samples at hz (0 for a negative or NaN duration). */
uint64_t jb_join_ms_to_samples(double ms, uint32_t hz);
/* New (none).  The geometry of a request over n members of n_in[u] samples at hz[u] (hz NULL: not compared):
 * programme_of[u] and member_start[u] ([n] each), *n_programmes = P and programme_samples[p] ([n], the first P are
 * written); any out pointer may be NULL.  A bad id, a non-zero reserved word or a programme of mixed rates:
 * JB_ERR_INVALID. */
int jb_join_geometry(const jb_join_utt *req, const size_t *n_in, const uint32_t *hz, size_t n, uint32_t *programme_of,
                     uint64_t *member_start, size_t *n_programmes, uint64_t *programme_samples);
/* New (none).  The rules in plain C++ on the host; no GPU is touched.  out[p] must hold programme p's samples
 * (cap[p] below that: JB_ERR_BUFFER); p runs over the geometry's P programmes.  The same samples and request give the
 * same programmes from the host, the seam and the batch. */
int jb_join_host(const double *const *in, const size_t *n_in, size_t n, const jb_join_utt *req, double *const *out,
                 const size_t *cap);
int jb_join_i16_host(const int16_t *const *in, const size_t *n_in, size_t n, const jb_join_utt *req,
                     int16_t *const *out, const size_t *cap);
/* New (none).  The stage on PCM the caller holds (jb_format_pcm_batch's twin), on `device` (-1 = current): the members
 * are packed one after the other on the device, as a batch's slab has them (member u starts n_in[0] + .. + n_in[u-1]
 * samples into it), and joined there.  out and n_out have n entries; the first *n_programmes are written: out[p] =
 * programme p, n_out[p] samples, library-owned (jb_join_free each). */
int jb_join_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_join_utt *req, int32_t device,
                      double **out, size_t *n_out, size_t *n_programmes);
int jb_join_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_join_utt *req,
                          int32_t device, int16_t **out, size_t *n_out, size_t *n_programmes);
void jb_join_free(void *p);

/* ---- Mix (new: the reference synthesises one utterance into one buffer; none of these entries has a counterpart) -------
 * A programme is the SUM of its members, each at a start of its own and under a gain of its own: two talkers at once
 * (the members' PCM stays readable; the stems in programme coordinates: "Stems" below), a crossfade between
 * sentences, a timed event over a sentence.  The stage stands in the join's place and feeds the same encoders and
 * feature stages, which then run over the mixture whole.  The rule (jbonsai_amd/csrc/jb_mix.h states it once for the
 * host, the device and the plan):
 * - Numbering and rate: as the join's.  Length: the largest start + n + pad_after over a programme's members.  Each
 *   programme starts on a 16-byte boundary of its slab.
 * - Gain: g = 10^(gain_db / 20), formed on the host in long double and rounded once (jb_mix_gain); 0 dB is exactly 1,
 *   -INFINITY exactly 0.
 * - Sample k: over the members in ascending utterance index, whatever their starts, each one with g != 0 and
 *   start <= k < start + n gives t = the join's faded sample of x[k - start] in f64 (a 16-bit sample enters as its
 *   (double); nothing is truncated per member), times g where g != 1.  The first term starts the sum, each later one
 *   is acc = acc + t (no fma).  Under no member the sample is +0.0.  An f64 programme stores acc, a 16-bit one the
 *   16-bit sink's rule of acc (clamp, then truncate toward zero).  So a sample under one member at 0 dB outside its
 *   fades keeps its bits, and a mix whose starts are a join's, at 0 dB, is that join's programme bit for bit.
 * - Fit (JB_MIX_FIT): M_p = the largest |acc| of the programme (fmax: a NaN is passed over), c the ceiling in sample
 *   units (32768 * 10^(ceiling_db / 20)), s_p = M_p > c ? c / M_p : 1.  Where s_p != 1 every sample is
 *   fmin(fmax(acc * s_p, -c), c) in front of the sink, so |y| <= c holds exactly; where s_p == 1 no bit changes.
 *   Without the flag nothing is scaled and the 16-bit sink clamps as it always does.  The peak is measured either way.
 * - Report: M_p, s_p, the largest number of unmuted members over one sample, the samples under two or more.
 * - Independence: a programme's bits depend on its members' samples and the request alone, not on the batch, its
 *   position, redo rounds (a touched programme runs again whole, the peak included) or the entry point;
 *   JB_BATCH_INVARIANT output stays invariant.
 * - Loudness, the ceiling and the limiter stay per utterance in front of the mix, as with the join.  The recipe for
 *   talkers at a level difference: per-utterance loudness targets set the difference (BS.1770 gating), JB_MIX_FIT
 *   keeps the sum under the ceiling.
 * - On the device (jb_mix.hip): the host cuts each programme at every member start and end into segments under a
 *   constant set of members; k_mix, one workgroup per 16 KiB destination tile, loads each covering member's 16-byte
 *   group at whatever alignment it has and adds in list order, so the work per sample follows the depth at that
 *   sample; k_mix_peak folds the tiles' maxima per programme; with JB_MIX_FIT k_mix runs again over the programmes
 *   with s_p != 1, from the members.  No LDS, no atomics.
 * - Cost: not measured.
 * Not covered: loudness measured over the mixture, the generator, the _multi entries, a member in two programmes
 * (the stems below are what that was asked for). */
/* New (none).  g of gain_db by the rule above; pure (a NaN or a value outside the setter's range is not refused here). */
double jb_mix_gain(double gain_db);
/* New (none).  The geometry of a request, as jb_join_geometry, plus depth[p] and overlap[p] of the report ([n] each,
 * the first P written); any out pointer may be NULL; opts may be NULL. */
int jb_mix_geometry(const jb_mix_utt *req, const size_t *n_in, const uint32_t *hz, size_t n, const jb_mix_opts *opts,
                    uint32_t *programme_of, uint64_t *member_start, size_t *n_programmes, uint64_t *programme_samples,
                    uint32_t *depth, uint64_t *overlap);
/* New (none).  The rule in plain C++ on the host; no GPU is touched.  out[p] must hold programme p's samples (cap[p]
 * below that: JB_ERR_BUFFER).  scale == NULL: the rule's s_p; otherwise scale[p] is taken as given (as jb_noise_host
 * takes a gain) and reported.  reports (may be NULL): [P]. */
int jb_mix_host(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req, const jb_mix_opts *opts,
                const double *scale, double *const *out, const size_t *cap, jb_mix_report *reports);
int jb_mix_i16_host(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                    const jb_mix_opts *opts, const double *scale, int16_t *const *out, const size_t *cap,
                    jb_mix_report *reports);
/* New (none).  The stage on PCM the caller holds (jb_join_pcm_batch's twin), on `device` (-1 = current).  out and
 * n_out have n entries; the first *n_programmes are written: out[p] = programme p, library-owned (jb_mix_free each).
 * reports (may be NULL): [n], the first P written, peak and scale the device's. */
int jb_mix_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                     const jb_mix_opts *opts, int32_t device, double **out, size_t *n_out, size_t *n_programmes,
                     jb_mix_report *reports);
int jb_mix_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                         const jb_mix_opts *opts, int32_t device, int16_t **out, size_t *n_out, size_t *n_programmes,
                         jb_mix_report *reports);
void jb_mix_free(void *p);

/* ---- Stems of a mix (new: none of these entries has a counterpart) -------------------------------------------------------
 * What a separation or diarisation corpus stores beside the mixture: each source exactly as it entered the sum -- at its
 * start, under its fades, its gain and the fit's scale, zero elsewhere, as long as the mixture -- and its level
 * against the mixture.  The members of one programme that carry the same stem id form one stem (one id per talker:
 * a talker's five sentences are one stem).  The rule (jbonsai_amd/csrc/jb_mix.h states it once):
 * - Stem s of programme p has the programme's length and rate.  Sample k is the mix rule over the stem's own members
 *   alone: ascending utterance index, the first term starts the sum, acc = acc + t behind it (no fma), +0.0 under
 *   none.  With JB_MIX_FIT and s_p != 1 the stored value is acc * s_p, s_p the PROGRAMME's scale: a stem has no scale
 *   of its own and is NOT clamped to the ceiling (a stem may peak above its mixture; a clamp would break additivity).
 *   The 16-bit sink clamps and truncates as it always does.
 * - Numbering: units 0 .. P-1 stay the programmes; the stems follow, by programme in dense order and within one by the
 *   ascending utterance index of each stem's first member.  Each stem starts on a 16-byte boundary of the programmes'
 *   slab, behind them, and is a unit like any other to FLAC, the sample formats, ADPCM, fbank, mfcc and melspec (the
 *   mfcc CMVN and the melspec range clamp are per unit, hence per stem).  The activity stage keeps reading members and
 *   keeps the P programmes as its units.  A muted member may carry an id and contributes nothing; a stem without an
 *   unmuted member of at least one sample exists and is all +0.0.
 * - Additivity: in f64 with s_p == 1 and every unmuted member under an id, at a sample under at most two members the
 *   stems added in unit order equal the mixture (==); under a depth d only the association differs:
 *   |sum - mix| <= (d - 1) 2^-52 sum |t|.  In 16 bits, where no term and no sum leaves [-32768, 32767], the stems' sum
 *   is within d counts of the mixture.  A stem that is one member at 0 dB keeps that member's bits outside its fades.
 * - Independence: a stem's bits depend on its members' samples, the request and s_p alone; a redo round runs a
 *   touched programme again whole, with its stems and their levels.
 * - Levels (JB_MIX_STEM_LEVELS): E_s = sum s[k]^2 and D = sum s[k] m[k] over the programme's 1,024-sample tiles that
 *   touch the stem's extent [first_sample, end_sample), E_p = sum m[k]^2 over all of the programme's tiles, of the
 *   units AS STORED (a 16-bit sample enters as its (double)), so a caller reproduces them from what they read back.
 *   The order is the noise stage's: 256 strided partials per tile, a partial's first term the product and each later
 *   one fused on (fma), the partials folded by the tree h = 128 .. 1, the tile sums added in ascending order.  The
 *   device's three sums are jb_mix_levels_host's bit for bit.  From them, on the host in long double:
 *   level_db = 10 log10(E_s / E_p), sir_db = 10 log10(E_s / (E_p - 2 D + E_s)), si_sdr_db = 10 log10(a / (E_p - a))
 *   with a = D^2 / E_s; +INFINITY where a denominator is not above 0, -INFINITY where E_s == 0.
 * - On the device (jb_mix.hip): the stems go through k_mix as units (the fit pass of a stem reads its programme's
 *   scale and does not clamp); k_mix_levels, one workgroup per tile, and a fold of one wave per unit.  No atomics.
 * - Cost: not measured.
 * - At engine level: jb_synthesize_programme_stems and jb_synthesize_programme_stems_flac_meta, behind
 *   jb_engine_set_programme_mix.
 * Not covered: activity columns per stem, loudness measured per stem, the generator, the _multi entries, a member in
 * two programmes. */
#define JB_MIX_NO_STEM 0xffffffffu
#define JB_MIX_STEM_LEVELS 1u
typedef struct jb_stem_report {
    double peak;  /* the largest |acc| of the stem, in front of the scale */
    double scale; /* s_p of its programme */
    double e_s, d, e_p; /* with JB_MIX_STEM_LEVELS, else 0 */
    double level_db, sir_db, si_sdr_db; /* with JB_MIX_STEM_LEVELS, else NaN */
} jb_stem_report;
/* New (none).  The stems request behind jb_batch_set_mix, before the first run: stem_of[u] is utterance u's stem id
 * within its programme (below jb_batch_size(b)) or JB_MIX_NO_STEM; flags: JB_MIX_STEM_LEVELS or 0.  NULL, 0, 0
 * withdraws it; withdrawing the mix withdraws it too.  JB_ERR_INVALID with jb_last_error naming the utterance and the
 * field: an id of jb_batch_size(b) or above, a request without a mix or over a join, an unknown flag, a slab too long.
 * jb_batch_num_outputs is P + S while it stands, and every encoder index and jb_batch_read_programme_pcm / _i16 take a
 * stem's unit. */
int jb_batch_set_mix_stems(jb_batch *b, const uint32_t *stem_of, size_t n, uint32_t flags);
size_t jb_batch_num_programmes(const jb_batch *b); /* P (without a join or mix request: the batch size) */
int64_t jb_batch_stem_unit(const jb_batch *b, size_t utt); /* the unit of the utterance's stem, or -1 */
/* New (none).  A stem's place: its dense programme, the caller's id, its members (muted ones included) and its extent
 * (0, 0 without an unmuted member of at least one sample); any out pointer may be NULL; unit below P or not below
 * P + S: JB_ERR_INVALID. */
int jb_batch_stem_layout(const jb_batch *b, size_t unit, uint32_t *programme, uint32_t *stem_id, uint32_t *n_members,
                         uint64_t *first_sample, uint64_t *end_sample);
/* New (none).  After a run: the stem's peak, its programme's scale and, with JB_MIX_STEM_LEVELS, the sums and the dB
 * values. */
int jb_batch_stem_report(jb_batch *b, size_t unit, jb_stem_report *out);
/* New (none).  The geometry of a mix request with stems: P, the units P + S, each utterance's stem unit (-1: none) and
 * per unit ([2 n] each, the first P + S written) its samples, its dense programme, the caller's stem id
 * (JB_MIX_NO_STEM for a programme), its members, its extent (a programme: 0 and its length) and its depth.  Any out
 * pointer may be NULL. */
int jb_mix_stems_geometry(const jb_mix_utt *req, const uint32_t *stem_of, const size_t *n_in, const uint32_t *hz, size_t n,
                          const jb_mix_opts *opts, size_t *n_programmes, size_t *n_units, int64_t *stem_unit,
                          uint64_t *unit_samples, uint32_t *unit_programme, uint32_t *unit_stem_id,
                          uint32_t *unit_members, uint64_t *unit_first, uint64_t *unit_end, uint32_t *unit_depth);
/* New (none).  The rule on the host: out and cap have P + S entries, the programmes first; scale as jb_mix_host's
 * ([P]; a stem takes its programme's).  reports (may be NULL): [P]; stem_reports (may be NULL): [S], the levels with
 * JB_MIX_STEM_LEVELS in flags taken from out as stored. */
int jb_mix_stems_host(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                      const uint32_t *stem_of, uint32_t flags, const jb_mix_opts *opts, const double *scale,
                      double *const *out, const size_t *cap, jb_mix_report *reports, jb_stem_report *stem_reports);
int jb_mix_stems_i16_host(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                          const uint32_t *stem_of, uint32_t flags, const jb_mix_opts *opts, const double *scale,
                          int16_t *const *out, const size_t *cap, jb_mix_report *reports, jb_stem_report *stem_reports);
/* New (none).  The three sums of a stem and its mixture of n samples each by the order above, on the host; the extent
 * with first_sample <= end_sample <= n.  Any out pointer may be NULL. */
int jb_mix_levels_host(const double *stem, const double *mix, size_t n, uint64_t first_sample, uint64_t end_sample,
                       double *e_s, double *d, double *e_p);
int jb_mix_levels_i16_host(const int16_t *stem, const int16_t *mix, size_t n, uint64_t first_sample,
                           uint64_t end_sample, double *e_s, double *d, double *e_p);
/* New (none).  The three dB values of a report from its three sums (long double on the host); pure. */
void jb_mix_levels_db(double e_s, double d, double e_p, double *level_db, double *sir_db, double *si_sdr_db);
/* New (none).  The stage with stems on PCM the caller holds, on `device` (-1 = current).  out and n_out have 2 n
 * entries; the first *n_units are written, the *n_programmes programmes first, library-owned (jb_mix_free each).
 * reports (may be NULL): [n], the first P written; stem_reports (may be NULL): [n], the first S written, the sums the
 * device's. */
int jb_mix_stems_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                           const uint32_t *stem_of, uint32_t flags, const jb_mix_opts *opts, int32_t device,
                           double **out, size_t *n_out, size_t *n_programmes, size_t *n_units, jb_mix_report *reports,
                           jb_stem_report *stem_reports);
int jb_mix_stems_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                               const uint32_t *stem_of, uint32_t flags, const jb_mix_opts *opts, int32_t device,
                               int16_t **out, size_t *n_out, size_t *n_programmes, size_t *n_units,
                               jb_mix_report *reports, jb_stem_report *stem_reports);

/* ---- Speech activity (new: the reference has no such output) ---------------------------------------------------------
 * Per-frame 0/1 labels on the frame grid of the feature stages, one column per talker: what an RTTM file or an
 * EEND-style [T][speakers] target holds, measured on the device so that the stems need not cross the link.  The rule
 * (jbonsai_amd/csrc/jb_activity.h states it once for the host and the device):
 * - A unit is an utterance, or a programme of a join or mix request.  Each unit gets a row-major uint8 matrix [T][C].
 * - Columns.  JB_ACTIVITY_MEMBERS: C = the programme's members in ascending utterance index; column j is measured on
 *   member j's own PCM before fade and gain (the gate is relative), placed at its start, reading 0 outside
 *   [start_j, start_j + n_j); a muted member (gain_db == -INFINITY) keeps its column, all zeros.  JB_ACTIVITY_UNIT:
 *   C = 1, measured on the unit's own PCM (the programme, or the utterance).  Without a programme the two are the same.
 * - Grid.  wl and hop are win_us and hop_us rounded at the unit's rate as the filterbank stage rounds them
 *   (floor(hz us / 10^6 + 1/2)); with JB_ACTIVITY_SAMPLES they are samples as given.  wl in 2..4096, hop >= 1.  For a
 *   unit of n >= 1 samples frame t starts at s_t:
 *     JB_ACTIVITY_SNIP    T = n >= wl ? 1 + (n - wl) / hop : 0   s_t = t hop                     (plain fbank)
 *     JB_ACTIVITY_CENTER  T = ceil(n / hop)                      s_t = t hop - wl / 2            (JB_FBANK_CENTER)
 *     JB_ACTIVITY_KALDI   T = (n + hop / 2) / hop                s_t = t hop + hop / 2 - wl / 2  (JB_FRAME_REFLECT)
 *     JB_ACTIVITY_STFT    T = 1 + n / hop                        s_t = t hop - wl / 2            (melspec, no drop-last)
 *   Samples outside the unit read as 0 (no reflection: a mirrored edge would invent energy).  n == 0: T = 0.
 * - Energy.  E[j][t] = sum over i < wl of v_i v_i, v_i column j's sample at s_t + i (16 bits enter as their (double)),
 *   summed as the frame conditioning's step 2 sums: 64 strided partials from 0.0, folded 32, 16, .., 1; products are
 *   rounded, then added (no fma).  A zero term leaves a partial's bits alone, so a frame that touches no sample of the
 *   member is exactly +0.0 and the result does not depend on how samples outside a member are skipped.
 * - Gate.  A frame is raw-active iff E > 0 and E >= thr.  JB_ACTIVITY_REF_PEAK: thr = q max_t E[j][t] with
 *   q = 10^(-gate_db / 10) formed in long double and rounded once.  JB_ACTIVITY_REF_ABS: thr = wl 32768^2
 *   10^(-gate_db / 10), rounded once from long double: a level in dBFS, the mode for stems that carry noise.
 *   gate_db in [1, 120].
 * - Smoothing, three integer steps on a column's raw bits in this order, lengths in frames, each in 0..65535.
 *   Close (min_gap): an inactive frame becomes active iff the nearest raw-active frames a in front and b behind exist
 *   with b - a - 1 <= min_gap (gaps at the head and the tail of the unit are never closed).  Open (min_speech): every
 *   run of active frames shorter than min_speech is cleared (a run cut by the unit's edge counts as long as is
 *   visible).  Hang: frame t is active iff a surviving frame s has s - hang_before <= t <= s + hang_after.  All four
 *   at 0: the raw bits.
 * - On the device (jb_activity.hip): k_act_energy stages a run of frames' samples in LDS once and sums each frame on
 *   one wave, storing per member only the frames that touch it and an integer atomic maximum of the bit patterns per
 *   column; k_act_label, one wave per column, packs the raw bits 64 to a word by ballot, runs the smoothing steps on the
 *   words with a wave scan across them, stores the bytes and the column's report; k_act_unit counts the rows.
 * Not covered: measuring in front of the noise stage (with a noise request the stems carry the noise: take
 * JB_ACTIVITY_REF_ABS or a gate above the floor), trimming, labels from the HMM alignment, packed-bit output, and any
 * claim of equality with Kaldi's or WebRTC's detectors. */
#define JB_ACTIVITY_SNIP 0u
#define JB_ACTIVITY_CENTER 1u
#define JB_ACTIVITY_KALDI 2u
#define JB_ACTIVITY_STFT 3u
#define JB_ACTIVITY_REF_PEAK 0u
#define JB_ACTIVITY_REF_ABS 1u
#define JB_ACTIVITY_MEMBERS 0u
#define JB_ACTIVITY_UNIT 1u
#define JB_ACTIVITY_SAMPLES 1u
/* T * C of a unit and the label bytes of a call may not pass this (JB_ERR_UNSUPPORTED): 256 members by 3.27 million
 * frames pass.  A chapter of hundreds of members takes JB_ACTIVITY_UNIT. */
#define JB_ACTIVITY_MAX_CELLS (1ull << 30)
typedef struct jb_activity_opts {
    uint32_t win_us, hop_us; /* microseconds; samples with JB_ACTIVITY_SAMPLES */
    double gate_db;          /* [1, 120] */
    uint32_t grid;           /* JB_ACTIVITY_SNIP, _CENTER, _KALDI, _STFT */
    uint32_t reference;      /* JB_ACTIVITY_REF_PEAK, _REF_ABS */
    uint32_t columns;        /* JB_ACTIVITY_MEMBERS, _UNIT */
    uint32_t flags;          /* JB_ACTIVITY_SAMPLES or 0 */
    uint32_t min_speech, min_gap, hang_before, hang_after; /* frames, 0..65535 */
    uint32_t reserved[4];
} jb_activity_opts;
/* A column's report. */
typedef struct jb_activity_report {
    uint64_t active;      /* active frames */
    uint64_t first, last; /* the first and the last active frame; T where there is none */
    double peak;          /* the largest energy of the column */
    double thr;           /* the threshold its frames were held to */
} jb_activity_report;
/* A unit's report. */
typedef struct jb_activity_unit_report {
    uint64_t frames;          /* T */
    uint64_t none, one, many; /* frames under 0, exactly 1, and 2 or more active columns */
} jb_activity_unit_report;
/* New (none).  The window, the hop and T of a unit of n samples at hz under opts (each out pointer may be NULL).
 * Refused with JB_ERR_INVALID naming the field: an unknown grid, reference, columns or flag, a non-zero reserved
 * word, a gate_db or a length outside its range, a window or hop outside its limits at hz. */
int jb_activity_geometry(const jb_activity_opts *opts, uint32_t hz, size_t n, uint32_t *wl, uint32_t *hop, uint64_t *T);
/* New (none).  The rule over one column in plain C++ on the host: x[0..n) is the unit, out[T] its labels (cap below T:
 * JB_ERR_BUFFER); report may be NULL.  `columns` is not read. */
int jb_activity_host(const double *x, size_t n, uint32_t hz, const jb_activity_opts *opts, uint8_t *out, size_t cap,
                     jb_activity_report *report);
/* New (none).  The rule over one unit of n_unit samples from its m members, on the host: member j holds in[j][0..n_in[j])
 * at start[j] (start[j] + n_in[j] above n_unit: JB_ERR_INVALID), muted where gain_db (may be NULL) has -INFINITY.
 * out: [T][m] (cap below T m: JB_ERR_BUFFER); cols (may be NULL): [m]; unit may be NULL.  opts->columns must be
 * JB_ACTIVITY_MEMBERS. */
int jb_activity_members_host(const double *const *in, const size_t *n_in, const uint64_t *start, const double *gain_db,
                             size_t m, uint64_t n_unit, uint32_t hz, const jb_activity_opts *opts, uint8_t *out,
                             size_t cap, jb_activity_report *cols, jb_activity_unit_report *unit);
/* New (none).  The stage on PCM the caller holds, on `device` (-1 = current).  Members, starts and programmes are given
 * as for jb_mix_pcm_batch; req == NULL: every utterance is a unit of its own.  hz: [n] each utterance's rate (a
 * programme's members must agree; may be NULL with JB_ACTIVITY_SAMPLES).  With JB_ACTIVITY_UNIT a programme is mixed
 * first (under mix_opts, may be NULL) and its column measured on the mixture.  out, T and C have n entries, the first
 * *n_units written: out[p] = unit p's [T[p]][C[p]] matrix, library-owned (jb_activity_free each).  cols (may be NULL):
 * [n], the columns' reports unit after unit; units (may be NULL): [n], the first *n_units written. */
int jb_activity_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                          const jb_mix_opts *mix_opts, const uint32_t *hz, const jb_activity_opts *opts, int32_t device,
                          uint8_t **out, uint64_t *T, uint32_t *C, size_t *n_units, jb_activity_report *cols,
                          jb_activity_unit_report *units);
int jb_activity_pcm_batch_i16(const int16_t *const *in, const size_t *n_in, size_t n, const jb_mix_utt *req,
                              const jb_mix_opts *mix_opts, const uint32_t *hz, const jb_activity_opts *opts,
                              int32_t device, uint8_t **out, uint64_t *T, uint32_t *C, size_t *n_units,
                              jb_activity_report *cols, jb_activity_unit_report *units);
void jb_activity_free(void *p);
/* New (none).  The stage in a batch: a side output beside whatever sinks the batch has, f64 or JB_BATCH_PCM_I16.  The
 * units are the batch's outputs (jb_batch_num_outputs): the programmes of a join or mix request, or the utterances.
 * Column j of a programme is its j-th member in ascending utterance index, measured on the PCM jb_batch_read_pcm hands
 * out, at jb_batch_member_start; JB_ACTIVITY_UNIT measures what jb_batch_read_programme_pcm hands out.  Checked at
 * every unit's rate and against JB_ACTIVITY_MAX_CELLS under the present requests (JB_ERR_INVALID naming the unit and
 * the field, JB_ERR_UNSUPPORTED past the cap), and again at the first run where a rate or a programme request came
 * behind it.  opts == NULL withdraws the request.  Only before the batch's first run.  A redo round measures every
 * unit with a rewritten member again, whole.  Without the request no kernel, list or allocation is added. */
int jb_batch_set_activity(jb_batch *b, const jb_activity_opts *opts);
/* New (none).  T, C and the rate of unit `unit` (each may be NULL), known once the request is made; its bytes T * C. */
int jb_batch_activity_shape(jb_batch *b, size_t unit, uint64_t *T, uint32_t *C, uint32_t *hz);
int jb_batch_activity_size(jb_batch *b, size_t unit, size_t *n_bytes);
/* New (none).  After the run: unit `unit`'s [T][C] labels into dst[0 .. cap) (JB_ERR_BUFFER if cap is below T * C); and
 * every unit's labels, dst[u] sized by jb_batch_activity_size, in one device-to-host copy for the batch. */
int jb_batch_read_activity(jb_batch *b, size_t unit, uint8_t *dst, size_t cap);
int jb_batch_read_activity_all(jb_batch *b, uint8_t *const *dst);
/* New (none).  After the run: the report of column `col` of unit `unit`, and the unit's. */
int jb_batch_activity_report(jb_batch *b, size_t unit, size_t col, jb_activity_report *out);
int jb_batch_activity_unit_report(jb_batch *b, size_t unit, jb_activity_unit_report *out);

/* ---- Pitch features (new: the reference has no such output) ----------------------------------------------------------
 * The pitch columns that the Kaldi/ESPnet recipes for tonal and pitch-accent languages read beside the filterbank rows
 * (compute-kaldi-pitch-feats | process-kaldi-pitch-feats; Ghahremani et al., ICASSP 2014), tracked on the PCM the
 * caller holds.  The rule (jbonsai_amd/csrc/jb_pitch.h states it once for the host and the device) is f64 throughout;
 * its tables come from the host in long double, rounded once; every sum has a fixed order; products are rounded before
 * they are added (no fma).  hz: the unit's rate, n its samples, r = JB_PITCH_RATE = 4000 Hz.
 * 1. Decimate.  y[m] = (1 / hz) sum_k x[k] f(k / hz - m / r), m < n4 = ceil(n r / hz), with
 *    f(t) = 2c sinc(2ct) (1 + cos(2 pi c t / w)) / 2 inside |t| < w / (2c) and 0 elsewhere, c = 1000 Hz, w = 1; from
 *    +0.0 over ascending k inside [0, n).  The weights come from a table of r / gcd(hz, r) phases (1 at 8, 16 and
 *    48 kHz, 40 at 44.1 kHz) of 2 ceil(hz / 2000) + 1 weights; a table above JB_PITCH_MAX_DOWN weights is
 *    JB_ERR_UNSUPPORTED, hz < r JB_ERR_INVALID.  S1 = sum y and S2 = sum y^2 are taken in the noise stage's order (tiles
 *    of 1,024 samples, 256 strided partials, the tree 128 .. 1, the tiles in ascending order) without its fused
 *    multiply-add; sigma^2 = S2 / n4 - (S1 / n4)^2.
 * 2. Frames.  wl and hop at the unit's rate are win_us and hop_us rounded as the filterbank stage rounds them, and
 *    T = n >= wl ? 1 + (n - wl) / hop : 0 (JB_PITCH_SNIP) or (n + hop / 2) / hop (JB_PITCH_KALDI): the filterbank
 *    stage's T under the same window, hop and grid (plain, or JB_FRAME_REFLECT), so the rows concatenate.  At 4 kHz
 *    wl4 = win_us / 250 (8..512) and sh4 = hop_us / 250, whole numbers: win_us and hop_us are multiples of 250.  Frame t
 *    starts at t sh4 (JB_PITCH_KALDI: t sh4 + sh4 / 2 - wl4 / 2); samples outside [0, n4) read as 0.  A stated
 *    deviation: Kaldi's snip mode drops the last frames whose longest lag runs past the end; they are kept here over
 *    zeros.
 * 3. Lags.  lag_0 = 1 / max_f0 and lag_{i+1} = lag_i (1 + delta_pitch), each one long double operation, while
 *    lag_i <= 1 / min_f0 (S lags, at most 1024; 417 at the defaults).  The integer lags run over a .. b,
 *    a = max(0, floor(r / max_f0 - 5/2)), b = ceil(r / min_f0 + 5/2) (at most 255; 7..83 at the defaults).
 * 4. NCCF.  v: the wl4 + b samples from the frame's start less the mean of the first wl4 (every sum of a frame in the
 *    frame conditioning's order: 64 strided partials from 0.0, folded 32 .. 1).  inner_L = sum_{i<wl4} v_i v_{i+L},
 *    e_L = sum v_{i+L}^2; q_L = inner_L / sqrt(e_0 e_L + B), B = nccf_ballast (sigma^2 wl4)^2, and
 *    p_L = inner_L / sqrt(e_0 e_L); +0.0 where the denominator is 0.  Both go to the lag grid:
 *    Q_i = sum_L q_L g_i[L] from +0.0 over ascending L, g_i[L] = f(L / r - lag_i) / r with c = r / 2 and w = 5.
 * 5. Track.  local_i = (1 - Q_i) + (soft_min_f0 lag_i) Q_i; F_t[i] = min_j (F_{t-1}[j] + kappa (i - j)^2) + local_i,
 *    kappa = penalty_factor ln(1 + delta_pitch)^2, (i - j)^2 an exact integer, the minimum exact over all j with ties
 *    to the smallest j; then F_t -= min_i F_t.  F_{-1} = 0.  The last state is the smallest index of the minimum; the
 *    stored choices are traced back.  The raw pair of a frame is (p at the chosen lag, 1 / lag).
 * 6. Process, the default output [T][3]: pov_scale ((1.0001 - clamp(p, -1, 1))^0.15 - 1); pitch_scale (l_t -
 *    sum pi_j l_j / sum pi_j) over j in [t - norm_left, t + norm_right] within [0, T), ascending, with l = ln(1 / lag)
 *    and pi = 1 / (1 + e^-rho), rho = -5.2 + 5.4 e^{7.5(a-1)} + 4.8 a - 2 e^{-10 a} + 4.2 e^{20(a-1)}, a = min(|p|, 1);
 *    delta_scale sum_{k=-2..2} k l_{clamp(t+k)} / 10.  JB_PITCH_RAW_LOG adds l_t as a fourth column; JB_PITCH_RAW gives
 *    the two columns of step 5 instead.  Elements are f32, or f64 with JB_PITCH_F64.
 * On the device (jb_pitch.hip): k_pitch_down, a workgroup per tile of the sums with the rate's phase table in LDS;
 * k_pitch_track, one workgroup per unit, serial over its frames and parallel over the lags (a call of one long unit
 * runs on one workgroup), storing a 16-bit choice per frame and lag: 2 S bytes per frame of scratch, 834 at the
 * defaults, over a call at most JB_PITCH_MAX_SCRATCH (JB_ERR_UNSUPPORTED); k_pitch_post, a wave per frame, for p at the
 * chosen lag; k_pitch_cols, a lane per frame, for step 6.  Steps 1 to 5 use + - * / sqrt and tables alone.
 * Not claimed: Kaldi's bits (no Kaldi binary was at hand to compare with), its online modes and its random delta
 * noise, a fused fbank + pitch sink (the equal T lets a caller concatenate), the generator, the _multi
 * entries, and the voice's own LF0 as ground truth. */
#define JB_PITCH_SNIP 0u
#define JB_PITCH_KALDI 1u
#define JB_PITCH_F64 1u
#define JB_PITCH_RAW 2u
#define JB_PITCH_RAW_LOG 4u
#define JB_PITCH_RATE 4000u
#define JB_PITCH_MAX_DOWN 4096u
#define JB_PITCH_MAX_SCRATCH (1ull << 32)
typedef struct jb_pitch_opts {
    uint32_t win_us, hop_us;        /* microseconds, multiples of 250 */
    double min_f0, max_f0;          /* Hz */
    double delta_pitch;             /* the lag grid's step, [0.0001, 1] */
    double penalty_factor;
    double soft_min_f0;
    double nccf_ballast;
    double pov_scale, pitch_scale, delta_scale;
    uint32_t norm_left, norm_right; /* frames, 0..4096 */
    uint32_t grid;                  /* JB_PITCH_SNIP, _KALDI */
    uint32_t flags;                 /* JB_PITCH_F64 | JB_PITCH_RAW | JB_PITCH_RAW_LOG */
    uint32_t reserved[4];
} jb_pitch_opts;
typedef struct jb_pitch_geometry_t {
    uint64_t T, n4;               /* frames, and samples at 4 kHz */
    uint32_t wl, hop;             /* at the unit's rate */
    uint32_t wl4, sh4;            /* at 4 kHz */
    uint32_t S, lag_first, lag_last; /* lags of the grid; a and b */
    uint32_t width, elem;         /* columns of a row, bytes of an element */
    uint32_t choice_bytes;        /* the tracker's scratch per frame */
} jb_pitch_geometry_t;
/* New (none).  Kaldi's defaults as PitchExtractionOptions and ProcessPitchOptions have them: 25 / 10 ms, 50..400 Hz,
 * delta_pitch 0.005, penalty_factor 0.1, soft_min_f0 10, nccf_ballast 7000, the three scales 2, 2, 10, 75 frames on
 * either side, JB_PITCH_KALDI (snip_edges = false), f32, three columns. */
int jb_pitch_kaldi(jb_pitch_opts *opts);
/* New (none).  The geometry of a unit of n samples at hz under opts (out may be NULL).  Refused with JB_ERR_INVALID
 * naming the field: an unknown grid or flag, a non-zero reserved word, a window or hop that is no multiple of 250 us
 * or outside its limits, a bound, step or scale outside its range, more than 1024 lags, an integer lag above 255,
 * hz below 4000; JB_ERR_UNSUPPORTED for a rate whose phase table passes JB_PITCH_MAX_DOWN. */
int jb_pitch_geometry(const jb_pitch_opts *opts, uint32_t hz, size_t n, jb_pitch_geometry_t *out);
/* New (none).  The lags of step 3 in seconds: *S (may be NULL) their count, lags (may be NULL) [cap] receives them
 * (JB_ERR_BUFFER if cap is below S). */
int jb_pitch_lags(const jb_pitch_opts *opts, double *lags, size_t cap, size_t *S);
/* New (none).  The rule in plain C++ on the host: x[0..n) is the unit, out its [T][width] elements (cap in bytes;
 * below T width elem: JB_ERR_BUFFER).  Each of lag_index [T] (the chosen lag of every frame), grid_q and grid_p
 * ([T][S]: Q and p over the lag grid) may be NULL. */
int jb_pitch_host(const double *x, size_t n, uint32_t hz, const jb_pitch_opts *opts, void *out, size_t cap,
                  uint32_t *lag_index, double *grid_q, double *grid_p);
/* New (none).  The stage on PCM the caller holds, on `device` (-1 = current): every utterance is a unit, hz[u] its
 * rate.  out[u] = its [T[u]][width] elements, library-owned (jb_pitch_free); lag_index (may be NULL): [n], each the
 * unit's [T[u]] chosen lags, library-owned.  T and width (may be NULL) have n entries. */
int jb_pitch_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                       const jb_pitch_opts *opts, int32_t device, void **out, uint64_t *T, uint32_t *width,
                       uint32_t **lag_index);
void jb_pitch_free(void *p);
/* New (none).  The stage in a batch: a byte sink beside whatever else the batch has, of an f64 batch (with
 * JB_BATCH_PCM_I16: JB_ERR_UNSUPPORTED).  The units are the batch's outputs (jb_batch_num_outputs): the utterances, or
 * behind a join or mix the programmes (and the stems behind them), so that the normalisation of the log-pitch runs over
 * the whole programme.  It reads the final f64 PCM that the filterbank stage would read, at each unit's output rate.
 * Checked at every unit's rate when set and when a rate is set behind it; the tracker's choices are allocated at the
 * first run, and past JB_PITCH_MAX_SCRATCH that run is refused with JB_ERR_UNSUPPORTED.  opts == NULL withdraws the
 * request.  Only before the batch's first run.  A redo round tracks every unit whose PCM changed again, whole.  Without
 * the request no kernel, list or allocation is added. */
int jb_batch_set_pitch(jb_batch *b, const jb_pitch_opts *opts);
/* New (none).  T, the row's width and the rate of unit `unit` (each may be NULL), known once the request is made; its
 * bytes T * width * element bytes. */
int jb_batch_pitch_shape(jb_batch *b, size_t unit, size_t *T, uint32_t *width, uint32_t *hz);
int jb_batch_pitch_size(jb_batch *b, size_t unit, size_t *n_bytes);
/* New (none).  After the run: unit `unit`'s rows into dst[0 .. cap) (JB_ERR_BUFFER if cap is too small); and every
 * unit's rows, dst[u] sized by jb_batch_pitch_size, in one device-to-host copy for the batch. */
int jb_batch_read_pitch(jb_batch *b, size_t unit, uint8_t *dst, size_t cap);
int jb_batch_read_pitch_all(jb_batch *b, uint8_t *const *dst);

/* ---- Filter (new: the reference has no such control) ---------------------------------------------------------------
 * A caller-chosen cascade of up to four second-order sections shapes the PCM on the device, at the output rate: behind
 * the converter (or the vocoder at the native rate) and in front of the loudness measurement, so that the target, the
 * ceiling, the groups, the join and every encoder see the filtered audio.
 * - Design (host only, once per distinct filter and output rate): the Audio EQ Cookbook forms with w0 = 2 pi f0 / fs and
 *   alpha = sin(w0) / (2 q) for every kind, the shelves with the same alpha and A = 10^(gain_db / 40), normalised by a0.
 * - Refused (JB_ERR_INVALID; jb_last_error names the utterance, the section and the field): more than four sections, an
 *   unknown kind, f0 <= 0, f0 >= rate / 2 at that utterance's output rate, q <= 0, a field that is not finite, and any
 *   section, designed or raw, whose poles are not strictly inside the unit circle (|a2| < 1 and |a1| < 1 + a2).
 * - One sample: transposed direct form II, per section y = fma(b0, x, s0); s0 = fma(b1, x, fma(-a1, y, s1));
 *   s1 = fma(b2, x, -a2 * y); the next section's x is y.  States start at zero.  Input and output are f64 in 16-bit
 *   units; a 16-bit batch's output is the 16-bit sink's rule (fmin to 32767, fmax to -32768, truncate) on the same y.
 * - The device filters tiles of 4,096 samples from zero state, carries their states with a scan of the affine maps
 *   s -> A^len s + e and filters the tiles again from their true start states: the serial recursion up to rounding.
 *   The tiling depends on the utterance's length alone: an utterance's output depends on its samples, its filter and
 *   its rate, not on the batch, its position in it or redo rounds; JB_BATCH_INVARIANT output stays invariant.
 * - jb_batch_read_pcm_native stays the unfiltered vocoder PCM.
 * - Cost on 256 x 128 s (profiles/r18_filter.txt): a one-section high-pass takes 6.70 ms of device time (each sample read
 *   twice and written once: 37.7 GB), four sections 12.20 ms; the loudness measurement and apply pass of the same batch:
 *   16.89 ms.  Against a serial cascade in extended precision the device's largest error is 4.4e-12 of the utterance's
 *   largest sample (a serial f64 cascade: 1.4e-12).
 * Not covered: time-varying filters, more than four sections, one-pole sections, a filter in front of
 * the converter, filters on the native-rate reads, serving a generator head early, reading through the pinned
 * ring. */
/* New (none).  f[0..n): one filter for the batch (n == 1) or one per utterance (n == jb_batch_size); NULL, 0 withdraws
 * the request.  Before the first run only.  Checked against each utterance's output rate, here and again by a later
 * jb_batch_set_output_rate. */
int jb_batch_set_filter(jb_batch *b, const jb_filter *f, size_t n);
/* New (none).  What the device runs for utterance utt at its output rate: *n sections (0 without a filter) in out. */
int jb_batch_filter_coefficients(const jb_batch *b, size_t utt, jb_biquad out[JB_FILTER_MAX_SECTIONS], uint32_t *n);
/* New (none).  The host design of f at hz: f->n_sections sections into out (out may be NULL: the check alone). */
int jb_filter_design(const jb_filter *f, uint32_t hz, jb_biquad out[JB_FILTER_MAX_SECTIONS]);
/* New (none).  The serial recursion in plain C++ on the host; no GPU is touched.  out must hold n samples (cap below
 * that: JB_ERR_BUFFER).  A filter without sections returns the input bit for bit. */
int jb_filter_pcm_host(const double *in, size_t n, const jb_filter *f, uint32_t hz, double *out, size_t cap);
/* New (none).  The stage on PCM the caller holds (jb_format_pcm_batch's twin), on `device` (-1 = current): utterance u
 * is n_in[u] f64 samples at hz[u] under f[u]; out[u] = its n_out[u] = n_in[u] filtered samples, f64 or by the 16-bit
 * sink's rule, library-owned (jb_filter_free each).  The same samples, filter and rate give the same bits from this
 * seam and from the batch path. */
int jb_filter_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_filter *f, const uint32_t *hz,
                        int32_t device, double **out, size_t *n_out);
int jb_filter_pcm_batch_i16(const double *const *in, const size_t *n_in, size_t n, const jb_filter *f,
                            const uint32_t *hz, int32_t device, int16_t **out, size_t *n_out);
void jb_filter_free(void *p);

/* ---- Convolution (new: the reference has no such control) ----------------------------------------------------------
 * The PCM convolved with a caller-given impulse response (FIR) on the device, at the output rate: a room or a
 * microphone response, a telephone channel in front of G.711, a linear-phase EQ, a matched or de-emphasis filter.  The
 * stage is part of the filter stage: behind the converter (or the vocoder at the native rate) and in front of the
 * filter's sections -- convolution first, then the cascade -- so that the loudness measurement, the ceiling, the
 * limiter, the groups, the join and every encoder see the convolved audio.
 * - The rule, for one utterance x[0..N) (f64, 16-bit units), taps h[0..K) and a delay d with 0 <= d < K:
 *       y[n] = sum over k of h[k] x[n + d - k],   n in [0, N)
 *   Terms whose index n + d - k lies outside [0, N) are skipped, not multiplied by zero.  The output has the input's
 *   length: the tail beyond N is dropped and d removes a leading latency (the direct path's index of a room response,
 *   (K - 1) / 2 of a linear-phase FIR), so the plan's geometry is that of the batch without the request.
 * - The host rule (jb_fir_host; plain C++, no GPU, O(N K), every K): the in-range terms in ascending k; the first
 *   starts acc = h[k] x[..], every later one is acc = fma(h[k], x[..], acc); no term in range gives +0.0.  So
 *   h = [1.0], d = 0 returns the input bit for bit.  A 16-bit batch's output is the 16-bit sink's rule (fmin to 32767,
 *   fmax to -32768, truncate) on the same y, as the filter's is.
 * - The request: taps (copied at the call: the caller's buffer may be freed afterwards), hz, the rate the response was
 *   sampled at -- it must equal the utterance's output rate; a response is never resampled -- the delay, reserved 0.
 *   taps == NULL with n_taps == 0 is no response for that utterance.
 * - Refused (JB_ERR_INVALID; jb_last_error names the utterance and the field) before any device is touched: n_taps == 0
 *   with taps given, n_taps above JB_FIR_MAX_TAPS, a tap that is not finite, delay >= n_taps, hz different from the
 *   utterance's output rate (at the set call and again at a later jb_batch_set_output_rate), reserved != 0.
 * - On the device, by K alone (jb_fir_geometry).  JB_FIR_DIRECT, K <= JB_FIR_DIRECT_MAX: every output sample's sum in
 *   one lane, over tiles of 2,048 outputs staged in LDS with their K - 1 samples in front, in the host rule's order:
 *   the output equals jb_fir_host bit for bit.  JB_FIR_PARTITIONED above: uniform partitioned overlap-save in f64 with blocks of
 *   Bk = n_fft / 2 samples, n_fft = 2048 up to K = 4096 and 4096 above, P = ceil(K / Bk) partitions; the partitions'
 *   spectra and the twiddles are made on the host in long double, once per distinct response (taps, delay, rate: by
 *   content); block j's spectrum -- of the n_fft samples that end at its end, shifted by d -- is taken once, and
 *   Y_j = sum over p of X[j - p] H[p] with p ascending from 0 to min(P - 1, j + lead), every bin's sum in one lane.  The
 *   d samples in front of block 0 are lead = ceil(d / Bk) blocks -lead .. -1 of their own (with d = 0 there are none
 *   and p stops at min(P - 1, j)).  Blocks are counted from the utterance's own first sample: a sample's
 *   bits depend on its utterance's samples, the taps, the delay and K only, not on the batch, the position, the entry
 *   point or redo rounds; JB_BATCH_INVARIANT output stays invariant.  Against the sum in extended precision the
 *   partitioned mode stays within 8 times the error of a float64 FFT convolution of the whole signal, relative to
 *   ||h||_1 max|x| (tests/test_gpu_fir.py).
 * - The spectrum scratch takes 16 (Bk + 1) bytes per block, lead blocks included: about 16 bytes per sample of every
 *   utterance in partitioned mode.
 * - jb_batch_read_pcm_native stays the vocoder's PCM.
 * - Cost on 256 x 128 s at 48 kHz (profiles/r21_fir.txt, written by tools/fir_cost.py): 64 taps take 11.07 ms of device
 *   time, 4,800 taps 39.24 ms, 24,000 taps 54.12 ms; the loudness measurement and apply pass of the same batch:
 *   17.42 ms.  Partitioned mode's error is at most 1.72 times the float64 FFT convolution's over the test shapes of more
 *   than one sample.
 * Not covered: keeping the tail, resampling a response, time-varying responses, non-uniform partitions, serving a
 * generator head early. */
#define JB_FIR_MAX_TAPS 131072u
#define JB_FIR_DIRECT_MAX 256u
#define JB_FIR_DIRECT 0u
#define JB_FIR_PARTITIONED 1u
typedef struct jb_fir {
    const double *taps; /* h[0..n_taps); NULL with n_taps 0: no response */
    uint32_t n_taps;
    uint32_t hz;        /* the rate the response was sampled at */
    uint32_t delay;     /* d < n_taps */
    uint32_t reserved;  /* 0 */
} jb_fir;
/* New (none).  f[0..n): one response for the batch (n == 1) or one per utterance (n == jb_batch_size); NULL, 0
 * withdraws the request.  Before the first run only. */
int jb_batch_set_fir(jb_batch *b, const jb_fir *f, size_t n);
/* New (none).  The geometry of utterance utt's response: JB_FIR_DIRECT or _PARTITIONED, the outputs of a workgroup
 * (the tile, or Bk) and the partitions (each may be NULL).  JB_ERR_INVALID where the utterance has no response. */
int jb_batch_fir_geometry(const jb_batch *b, size_t utt, uint32_t *mode, uint32_t *block, uint32_t *partitions);
/* New (none).  The same for a tap count in 1..JB_FIR_MAX_TAPS; pure. */
int jb_fir_geometry(uint32_t n_taps, uint32_t *mode, uint32_t *block, uint32_t *partitions);
/* New (none).  The host rule; no GPU is touched.  f->hz is not looked at beyond the request check; out must hold n
 * samples (cap below that: JB_ERR_BUFFER) and must not overlap in.  A request without taps returns the input. */
int jb_fir_host(const double *in, size_t n, const jb_fir *f, double *out, size_t cap);
/* New (none).  The stage on PCM the caller holds (jb_filter_pcm_batch's twin), on `device` (-1 = current): utterance u
 * is n_in[u] f64 samples at hz[u] under f[u] (taps NULL: the samples themselves); out[u] = its n_out[u] = n_in[u]
 * samples, f64 or by the 16-bit sink's rule, library-owned (jb_fir_free each).  The same samples, response and delay
 * give the same bits from this seam and from the batch path. */
int jb_fir_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_fir *f, const uint32_t *hz,
                     int32_t device, double **out, size_t *n_out);
int jb_fir_pcm_batch_i16(const double *const *in, const size_t *n_in, size_t n, const jb_fir *f, const uint32_t *hz,
                         int32_t device, int16_t **out, size_t *n_out);
void jb_fir_free(void *p);

/* ---- Room responses (new: the reference has no such control) -------------------------------------------------------
 * The impulse response of a shoebox room by the image-source method (Allen and Berkley, 1979), made on the device and
 * installed as the convolution stage's request: "a different simulated room per utterance" without a second tool, a
 * directory of responses or a host loop.  Everything behind the generator is the convolution stage, unchanged.
 * - The room: edges size[3] in metres; source[3] and mic[3], strictly inside; reflection coefficients beta[6] in
 *   (-1, 1), in the order x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz; the speed of sound c (0: 343 m/s); the rate hz;
 *   n_taps = K in 1..JB_FIR_MAX_TAPS; flags; reserved 0.  A room whose bytes are all zero is "no room for this
 *   utterance" where one is given per utterance.
 * - Constants: the low-pass interpolator's half-width Wh = JB_ROOM_WH = 32 samples, Q = JB_ROOM_Q = 128 table points
 *   per sample.  The table (jb_room_lowpass) is F[q] = sinc(q / Q) w(q) for q = 0 .. Q Wh, with the Hann window
 *   w(q) = (1 + cos(pi q / (Q Wh))) / 2, and 0 for the two entries above: Q Wh + 3 entries, made on the host in long
 *   double and rounded once.  It is evaluated in the well-conditioned forms sinc(n + r) = (-1)^n sin(pi r) / (pi (n + r))
 *   for q = n Q + r Q (exactly 0 where r = 0 < n, 1 at q = 0) and w(q) = sin^2(pi (Q Wh - q) / (2 Q Wh)).
 * - Axis tables (host, long double, rounded once).  For the axis of length L, source s, microphone r and walls b0, b1:
 *   n runs over -Na .. Na, Na = ceil(Rmax / 2L) + 1, Rmax = c (K + Wh) / hz, and p over {0, 1}; the coordinate is
 *   D = ((1 - 2p) s + 2 n L) - r and the weight g = b0^|n - p| b1^|n| (x^0 = 1).  Entries whose g rounds to 0 are left
 *   out; the rest are sorted by |D| ascending, ties by (n, p), and stored as the doubles D2 = D^2 and g.  More than
 *   JB_ROOM_MAX_AXIS = 1024 entries on an axis: JB_ERR_UNSUPPORTED (three tables and F are staged in LDS together:
 *   80 KiB of a CU's 160 KiB at the bound; a launch takes what its largest room needs).
 * - Lookup: lp(t): u = |t| Q, i0 = floor(u), f = u - i0, lp = fma(f, F[i0 + 1] - F[i0], F[i0]).
 * - Tap k, in one lane, in this order: acc = +0.0; then i ascends over the x table, inside it j over the y table,
 *   inside it m over the z table: s2 = (D2x[i] + D2y[j]) + D2z[m], d = sqrt(s2), tau = d kappa (kappa = hz / c, long
 *   double, rounded once), t = (double)k - tau; if |t| < Wh: A = ((gx[i] gy[j]) gz[m]) / (fourpi d) and
 *   acc = fma(A, lp(t), acc).  With JB_ROOM_UNIT_DIRECT the divisor is d / d0 instead, d0 the same expression for the
 *   three (n = 0, p = 0) entries: the direct path then has amplitude about 1 and a batch without a loudness target
 *   keeps its level.  The direct index is floor(d0 kappa + 0.5).
 * - A response's bits depend on the room alone: not on the call, the other rooms of a call, or the device's
 *   scheduling.  jb_room_host visits every (i, j, m); the kernel skips entries only where the test |t| < Wh fails for
 *   every tap of the workgroup (below).
 * - Refused (JB_ERR_INVALID; jb_last_error names the room and the field) before any device is touched: an edge outside
 *   [0.5, 1000] m, a position not strictly inside, |beta| >= 1 or a value that is not finite, c neither 0 nor in
 *   [50, 5000], source and microphone closer than 1 cm, hz outside 1000..768000, K of 0 or above the cap, a direct
 *   index >= K, an unknown flag, reserved != 0.  entries_x entries_y K above 2^32 for one room: JB_ERR_UNSUPPORTED
 *   (a bound on the work of one room, to protect a shared card).
 * - On the device (jb_room.hip, k_room): one lane per tap, workgroups of 256 consecutive taps of one room, a grid over
 *   (tap tiles, distinct rooms); rooms equal by content are generated once.  The three tables and F are staged in
 *   LDS.  A workgroup's taps k0 .. k0 + 255 reach d in ((k0 - Wh) / kappa, (k0 + 255 + Wh) / kappa); that band, as
 *   squared distances and widened by 2^-30 of itself, ends the i and j loops at the first entry beyond it (the tables
 *   are sorted) and, per (i, j), bounds the window of z entries by bisection on D2z, widened by one entry on either
 *   side; inside the window every lane applies the exact test.  f64 throughout, explicit fma, no atomics.  A call
 *   whose rooms together exceed a launch budget of 2^35 pair visits (entries_x entries_y K) is cut into several
 *   launches by room: at the 3.3e10 to 9.0e10 pair visits a second of whole calls of 256 rooms
 *   (profiles/r25_room.txt, written by tools/room_cost.py) a launch stays around a second at most.
 * - jb_room_vary: the positions of the utterance of index k, uniform at least `margin` from every wall.  With mix the
 *   splitmix64 finaliser of the noise and dither stages: z = mix(mix(seed) ^ k); attempt a = 0, 1, ..: coordinate j
 *   (0..2: the source's x, y, z; 3..5: the microphone's) is margin + u (L - 2 margin) -- the product rounded, then the
 *   sum -- with u = (mix(z + 6 a + j + 1) >> 11) 2^-53 and L its axis' edge; the first attempt whose source and
 *   microphone are at least 1 cm apart is taken (64 attempts without one: JB_ERR_INVALID).  margin > 0 and
 *   2 margin < every edge.
 * Not covered: frequency-dependent absorption, directivity, rooms that are not shoeboxes, randomised image positions
 * (Lehmann's fix of sweeping echoes), responses that stay on the device instead of passing through the host on their
 * way to the convolution's spectra, more than one microphone per room. */
#define JB_ROOM_UNIT_DIRECT 1u  /* flags: amplitudes relative to the direct path's */
#define JB_ROOM_KEEP_LATENCY 2u /* flags: jb_batch_set_room installs the response with delay 0 */
#define JB_ROOM_VARY 1u         /* jb_engine_set_room's flags: positions by jb_room_vary */
#define JB_ROOM_WH 32u
#define JB_ROOM_Q 128u
#define JB_ROOM_MAX_AXIS 1024u
typedef struct jb_room {
    double size[3], source[3], mic[3], beta[6], c;
    uint32_t hz, n_taps, flags, reserved;
} jb_room;
typedef struct jb_room_info {
    double direct_distance; /* d0, metres */
    uint64_t pair_visits;   /* entries_x entries_y K */
    uint64_t workgroups;    /* ceil(K / 256) */
    uint32_t entries[3];    /* of the x, y and z tables */
    uint32_t direct_index;  /* floor(d0 kappa + 0.5) */
} jb_room_info;
typedef struct jb_room_report {
    double energy;         /* sum of h[k]^2, ascending k, fused */
    double drr_db;         /* 10 log10 of the energy within +-Wh of the direct index over the rest (+INFINITY: no rest) */
    uint32_t direct_index;
    uint32_t delay;        /* what the convolution was given: the direct index, or 0 with JB_ROOM_KEEP_LATENCY */
} jb_room_report;
/* New (none).  The rule on the host; no GPU is touched.  h must hold r->n_taps taps (cap below that: JB_ERR_BUFFER). */
int jb_room_host(const jb_room *r, double *h, size_t cap);
/* New (none).  The device seam: the responses of r[0..n) generated on `device` (-1 = current); h[u] = room u's
 * n_h[u] = n_taps taps, library-owned (jb_room_free each).  Rooms equal by content are generated once and give the
 * same bits. */
int jb_room_rir_batch(const jb_room *r, size_t n, int32_t device, double **h, size_t *n_h);
void jb_room_free(void *p);
/* New (none).  Entries per axis, direct distance and index, pair visits and workgroups of a room; pure. */
int jb_room_geometry(const jb_room *r, jb_room_info *out);
/* New (none).  The table F (cap below Q Wh + 3 with F given: JB_ERR_BUFFER) and the two constants; each pointer may be
 * NULL. */
int jb_room_lowpass(double *F, size_t cap, uint32_t *Wh, uint32_t *Q);
/* New (none).  Eyring's formula: alpha = 1 - exp(-(24 ln 10 / c) V / (S rt60)) with the volume V and the surface S,
 * beta = sqrt(1 - alpha) on all six walls (long double, rounded once).  c 0: 343 m/s.  rt60 <= 0 or not finite, or an
 * edge outside [0.5, 1000] m: JB_ERR_INVALID. */
int jb_room_design(const double size[3], double rt60, double c, double beta[6]);
/* New (none).  The positions of the utterance of index k (the rule above); pure. */
int jb_room_vary(uint64_t seed, uint64_t k, const double size[3], double margin, double source[3], double mic[3]);
/* New (none).  r[0..n): one room for the batch (n == 1) or one per utterance (n == jb_batch_size; all bytes zero: none
 * for that utterance); NULL, 0 withdraws the request.  Before the first run only.  Each room's hz must equal its
 * utterance's output rate (the convolution's check, made again by a later jb_batch_set_output_rate).  The distinct
 * rooms are generated on the batch's device in this call and installed as the batch's convolution request with
 * delay = the direct index (0 with JB_ROOM_KEEP_LATENCY).  The room request and jb_batch_set_fir share one slot: the
 * later call replaces the earlier.  The same room gives the bits of jb_batch_set_fir with jb_room_rir_batch's taps. */
int jb_batch_set_room(jb_batch *b, const jb_room *r, size_t n);
/* New (none).  The response of utterance utt, from the taps jb_batch_set_room read back (host).  JB_ERR_INVALID where
 * the utterance has no room. */
int jb_batch_room_report(const jb_batch *b, size_t utt, jb_room_report *out);

/* ---- Noise (new: the reference has no such control) ----------------------------------------------------------------
 * Background noise added to the PCM on the device at a target signal-to-noise ratio: a caller-given noise bed that is
 * looped, or white noise generated on the device, scaled so that speech power over added-noise power is the requested
 * SNR.  The stage is part of the filter stage and runs at the output rate, behind the convolution and in front of the
 * filter's sections -- reverberate, add noise, then the channel filter -- so that the loudness measurement, the
 * ceiling, the limiter, the groups, the join and every encoder and feature stage see the noisy audio.  The output has
 * the input's length.  The rule, for one utterance x[0..N) (f64, 16-bit units: the convolution's output where the
 * utterance has a response, else what the filter stage reads):
 *   1. The noise sequence w[n], n in [0, N).  JB_NOISE_BED: w[n] = bed[(offset + n) mod Lb], offset < Lb.
 *      JB_NOISE_WHITE: r = mix(mix(seed) ^ n), mix the splitmix64 finaliser of the format stage's dither; w[n] is the
 *      sum of the four 16-bit fields of r as integers, minus 131070, as a double: an exact integer in +-131070,
 *      bell-shaped (Irwin-Hall of four), of zero mean and variance (2^32 - 1) / 3.  Its scale does not matter (the gain
 *      normalises it); a sample depends on (seed, n) alone.
 *   2. The power sum S(z) of a sequence z[0..N), in a fixed order that depends on the utterance alone.  Tiles of 1,024
 *      samples are counted from the utterance's first sample.  A tile has 256 partials: p[l] covers the in-range
 *      indices l + 256 j, j = 0..3 ascending; the first term is the product z z, every later one fma(z, z, p); a
 *      partial with no index in range is +0.0.  Then p[l] = p[l] + p[l + h] for l < h, h = 128, 64, .., 1; the tile
 *      sum is t_i = p[0].  S = t_0, then S = S + t_i in ascending i; N == 0 gives +0.0.
 *   3. The reference level.  JB_NOISE_REF_WHOLE: A = S(x), C = N (what Kaldi's wav-reverberate and
 *      torchaudio.functional.add_noise do).  JB_NOISE_REF_ACTIVE (synthesized utterances begin and end with silence,
 *      which makes the whole-signal power understate the speech): with q = 10^(-gate_db / 10) (host, long double,
 *      rounded once), tile i of c_i samples is active iff t_i (double)N >= (S(x) q) (double)c_i; A is the sum of the
 *      active t_i in ascending order (the first starts it), C the sum of their c_i.
 *   4. The noise power is over all N samples: Bs = S(w).
 *   5. The gain: with r = 10^(snr_db / 10) (host, long double, rounded once),
 *      g = sqrt(((A (double)N) / (Bs (double)C)) / r), in that operation order; g = 0 where A == 0, Bs == 0 or
 *      snr_db == +INFINITY.
 *   6. y[n] = fma(g, w[n], x[n]).  With g == 0 the utterance is not mixed: y = x bit for bit, signed zeros included.
 *      A 16-bit output is the 16-bit sink's rule (fmin, fmax, truncate) on that y, as the filter's and the
 *      convolution's are.
 * - The request: kind; the bed (copied at the call), its length (at most JB_NOISE_MAX_BED) and hz, the rate it was
 *   sampled at -- it must equal the utterance's output rate; a bed is never resampled; hz is not read with
 *   JB_NOISE_WHITE -- the offset into the bed; the generator's seed; snr_db, finite in [-40, 100] or +INFINITY;
 *   the reference and its gate_db ([1, 60] with JB_NOISE_REF_ACTIVE, else 0); flags; reserved 0.  kind JB_NOISE_BED
 *   with bed == NULL and bed_len == 0 is no request for that utterance.  The distinct beds of a batch are stored once
 *   each, by content, and hold at most 2^26 samples (above: JB_ERR_UNSUPPORTED).
 * - Refused (JB_ERR_INVALID; jb_last_error names the utterance and the field) before any device is touched: an unknown
 *   kind, reference or flag, a bed sample that is not finite, offset >= bed_len, bed_len == 0 with a bed given, a bed
 *   with JB_NOISE_WHITE, hz different from the output rate (at the set call and again at a later
 *   jb_batch_set_output_rate), snr_db or gate_db out of range or NaN, reserved != 0.
 * - JB_NOISE_VARY, where one request is spread over many utterances (jb_batch_set_noise with n == 1, the engine
 *   entries): the utterance of index k in the batch or call uses z = mix(mix(seed) ^ k), seed_k = z,
 *   offset_k = mix(z) mod Lb (the given offset is ignored), so that the utterances of a corpus do not all get the same
 *   noise (jb_noise_vary).  With one request per utterance the flag is refused.
 * - On the device (jb_noise.hip): k_noise_sums forms the tile sums of x and w in one pass, one workgroup per tile, the
 *   partial tree through LDS in the rule's order; k_noise_gain, one wave per utterance, adds the tile sums in ascending
 *   order, runs the active pass and leaves the gain; k_noise_apply streams y.  No atomics, nothing whose order the
 *   scheduling sets: A, C and Bs equal jb_noise_host's bit for bit, the gain to an ulp of the division and the square
 *   root, and y equals jb_noise_host under the device's gain bit for bit.  A sample's bits depend on its utterance's
 *   samples, the request and the gain alone, not on the batch, the position, the entry point or redo rounds;
 *   JB_BATCH_INVARIANT output stays invariant.  The sum scratch takes 16 bytes per 1,024 samples.
 * - jb_batch_read_pcm_native stays the vocoder's PCM.
 * - Cost on 256 x 128 s at 48 kHz (profiles/r23_noise.txt, written by tools/noise_cost.py): white noise at 15 dB takes
 *   8.05 ms of device time, a 10 s bed 9.68 ms, a 7-sample bed 8.75 ms, a 10 s bed against the active tiles 10.24 ms;
 *   the loudness measurement and apply pass of the same batch: 16.96 ms.  By kernel: k_noise_apply 4.63 ms (5.26 ms
 *   with the long bed) beside k_ln_apply's 4.62 ms on the same samples, k_noise_sums 3.28 to 4.34 ms, k_noise_gain
 *   0.10 ms (0.65 ms with the active reference).  Over the test shapes the device's gain equals the host's bit for
 *   bit (largest |g_dev / g_host - 1|: 0; gate 2^-50).
 * Not covered: noise over a programme's pads (the stage runs per utterance in front of the join), several layers per
 * utterance and timed foreground events, resampling a bed, coloured generated noise (a bed does that), the _multi
 * entries (the convolution does not serve them either). */
#define JB_NOISE_BED 0u
#define JB_NOISE_WHITE 1u
#define JB_NOISE_REF_WHOLE 0u
#define JB_NOISE_REF_ACTIVE 1u
#define JB_NOISE_VARY 1u
#define JB_NOISE_MAX_BED 16777216u
typedef struct jb_noise {
    const double *bed;  /* bed[0..bed_len), 16-bit units; NULL with JB_NOISE_WHITE, or with bed_len 0: no request */
    uint64_t seed;      /* JB_NOISE_WHITE's sequence; with JB_NOISE_VARY what the utterances' seeds and offsets come from */
    double snr_db;      /* [-40, 100], or +INFINITY: the utterance is not mixed */
    double gate_db;     /* [1, 60] with JB_NOISE_REF_ACTIVE, else 0 */
    uint32_t kind;      /* JB_NOISE_BED, JB_NOISE_WHITE */
    uint32_t bed_len;
    uint32_t hz;        /* the rate the bed was sampled at */
    uint32_t offset;    /* < bed_len */
    uint32_t reference; /* JB_NOISE_REF_WHOLE, JB_NOISE_REF_ACTIVE */
    uint32_t flags;     /* JB_NOISE_VARY */
    uint32_t reserved;  /* 0 */
} jb_noise;
typedef struct jb_noise_report {
    double speech_power;     /* A / C (0 where C is 0) */
    double noise_power;      /* Bs / N, of the unscaled noise (0 where N is 0) */
    double gain;             /* g */
    double snr_db;           /* as requested */
    uint64_t active_samples; /* C */
    uint64_t seed;           /* the seed and ... */
    uint32_t offset;         /* ... the offset that were used (JB_NOISE_VARY: the utterance's own) */
    uint32_t reserved;
} jb_noise_report;
/* New (none).  req[0..n): one request for the batch (n == 1) or one per utterance (n == jb_batch_size); NULL, 0
 * withdraws the request.  Before the first run only; not on a JB_BATCH_MLPG_ONLY batch; in either order with the rate,
 * filter, response, loudness and join setters. */
int jb_batch_set_noise(jb_batch *b, const jb_noise *req, size_t n);
/* New (none).  What the stage did to utterance utt, after a run.  JB_ERR_INVALID without a request for that utterance
 * or before a run. */
int jb_batch_noise_report(jb_batch *b, size_t utt, jb_noise_report *out);
/* New (none).  The rule in plain C++; no GPU is touched.  gain == NULL: the rule's gain; otherwise *gain is taken as
 * given (as jb_limiter_host takes its gain).  req->hz is not looked at beyond the request check, JB_NOISE_VARY is
 * ignored; y must hold n samples (cap below that: JB_ERR_BUFFER) and must not overlap x; report may be NULL.  No
 * request returns the input. */
int jb_noise_host(const double *x, size_t n, const jb_noise *req, const double *gain, double *y, size_t cap,
                  jb_noise_report *report);
int jb_noise_host_i16(const double *x, size_t n, const jb_noise *req, const double *gain, int16_t *y, size_t cap,
                      jb_noise_report *report);
/* New (none).  Samples first .. first + count of JB_NOISE_WHITE's sequence of `seed`; pure. */
int jb_noise_white(uint64_t seed, uint64_t first, size_t count, double *out);
/* New (none).  JB_NOISE_VARY's rule for the utterance of index k (bed_len 0: white, *offset_k = 0); pure. */
int jb_noise_vary(uint64_t seed, uint64_t k, uint32_t bed_len, uint64_t *seed_k, uint32_t *offset_k);
/* New (none).  The stage on PCM the caller holds (jb_fir_pcm_batch's twin), on `device` (-1 = current): utterance u is
 * n_in[u] f64 samples at hz[u] under req[u] (no request: the samples themselves; JB_NOISE_VARY is refused);
 * out[u] = its n_out[u] = n_in[u] samples, f64 or by the 16-bit sink's rule, library-owned (jb_noise_free each);
 * reports (may be NULL): [n].  The same samples and request give the same bits from this seam and from the batch
 * path. */
int jb_noise_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const jb_noise *req, const uint32_t *hz,
                       int32_t device, double **out, size_t *n_out, jb_noise_report *reports);
int jb_noise_pcm_batch_i16(const double *const *in, const size_t *n_in, size_t n, const jb_noise *req,
                           const uint32_t *hz, int32_t device, int16_t **out, size_t *n_out, jb_noise_report *reports);
void jb_noise_free(void *p);

/* ---- Limiter (new: the reference has no such control) --------------------------------------------------------------
 * A look-ahead peak limiter in the place of the loudness apply pass: a few peaks are taken down so that the rest can
 * reach the target.  With a request the static gain of an utterance (or of its loudness group) is
 * ln_gain_db(T, L, C + max_reduction_db, P): it may put the highest peak up to max_reduction_db over the ceiling C, and
 * the limiter holds the ceiling.  The rule, for one utterance x[0..N) (f64, 16-bit units) under the gain g, the
 * ceiling c = 32768 10^(C / 20), the look-ahead L = max(1, round(lookahead_ms hz / 1000)) and the hold
 * H = round(hold_ms hz / 1000) samples (round: floor(v + 0.5)), FIR only -- no recursion, no iteration, no delay:
 *   1. u[n] = x[n] g.
 *   2. the detector: JB_PEAK_SAMPLE d[n] = |u[n]|; JB_PEAK_TRUE d[n] = max(|u[n]|, b[n - 1], b[n]), b[n] the largest
 *      magnitude of the F - 1 interpolated phases between samples n and n + 1 (jb_true_peak_filter's taps over
 *      u[n - 5 .. n + 6], u = 0 outside [0, N), one product and eleven FMAs in ascending tap order; b[-1] included).
 *   3. r[n] = c / d[n] where d[n] > c, else 1; r = 1 outside [0, N).
 *   4. m[k] = min r[k - H .. k + L], k = -L .. N - 1.
 *   5. a[n] = w[0] m[n], then fma(w[j], m[n - j], a) for j = 1..L (w: jb_limiter_window); a[n] = 1 where every
 *      m[n - j] is 1; then a[n] = min(a[n], r[n]).
 *   6. y[n] = min(max(u[n] a[n], -c), c); a 16-bit output is the 16-bit sink's rule on that y.
 * Guaranteed: |y[n]| <= c exactly (the sample peak), N samples out, and y[n] = x[n] g bit for bit unless some d[i] > c
 * lies in i = n - L - H .. n + L: an utterance that stays under the ceiling gets the bytes of the plain apply pass.
 * Reported only: the true peak of y (in JB_PEAK_TRUE mode the detector bounds the inter-sample peaks of u; those of y
 * stay near the ceiling, without a guarantee) and the loudness of y, which ends a little under the target (the
 * limiter is not iterated; jb_batch_loudness* keep reporting the static gain_db).
 * The device (jb_limiter.hip) limits tiles of 1,024 samples with a halo of L + H samples in front and L behind; the
 * tiling depends on the utterance alone, every sample follows the rule above exactly, so the output depends on the
 * utterance's samples, gain and options only and JB_BATCH_INVARIANT output stays invariant.
 * Not covered: a recursive release, multiband limiting, iteration to the target, a guaranteed true-peak bound, the
 * _multi entries. */
#define JB_LIMITER_EXACT 1u /* flags: the three values are taken as given (a hold or a reduction of 0 means 0) */
#define JB_LIMITER_OFF 2u   /* flags: this utterance is not limited: the plain apply pass.  The values are not read, so
                               no geometry is formed and no rate is refused for it */
typedef struct jb_limiter_opts {
    double lookahead_ms;     /* (0, 10]; 0 without JB_LIMITER_EXACT: 2 ms */
    double hold_ms;          /* [0, 50]; 0 without JB_LIMITER_EXACT: 8 ms */
    double max_reduction_db; /* [0, 24]: how far the static gain may put the highest peak over the ceiling; 0 without
                                JB_LIMITER_EXACT: 6 dB.  Read by the batch and the engine alone, where it enters the gain
                                rule (there, with JB_LIMITER_EXACT, 0 gives the plain apply pass); jb_limiter_host and
                                jb_limiter_pcm_batch take the gain as given, check the field's range and do not read
                                it further: they limit whatever that gain puts over the ceiling */
    uint32_t flags;          /* JB_LIMITER_EXACT, JB_LIMITER_OFF or 0; any other bit: JB_ERR_INVALID */
    uint32_t reserved;       /* 0 */
} jb_limiter_opts;
typedef struct jb_limiter_report {
    double max_reduction_db;  /* -20 log10 of the smallest a[n] (0: nothing was limited) */
    uint64_t limited_samples; /* samples with a[n] < 1 */
    uint32_t lookahead, hold; /* L and H in samples at the utterance's output rate */
} jb_limiter_report;
/* New (none).  opts[0..n): one request for the batch (n == 1) or one per utterance (n == jb_batch_size); NULL, 0
 * withdraws it.  A value outside its range, a non-finite one, an unknown flag or a non-zero reserved word:
 * JB_ERR_INVALID before any device is touched (jb_last_error names the utterance and the field).  Only before the
 * first run and not on a JB_BATCH_MLPG_ONLY batch; in either order with the target, the peak mode, the output rate and
 * the groups.  The members of one loudness group must agree on the options: this setter and the group setters refuse a
 * mixed group, naming the group and the field.  Without a target the request has no effect; an utterance without a
 * finite ceiling is not limited.  2 L + H above 2048 samples at an utterance's output rate fails at the run with
 * JB_ERR_UNSUPPORTED.  Without the call -- and with a request that limits no utterance (every one JB_LIMITER_OFF,
 * without depth or without a finite ceiling) -- the apply pass runs as before: nothing is added to a run and nothing is
 * allocated. */
int jb_batch_set_limiter(jb_batch *b, const jb_limiter_opts *opts, size_t n);
/* New (none).  What the last run's limiter did to utterance utt (zeros with the L, H of its request where nothing
 * reached the ceiling; all zeros for an utterance that is not limited: JB_LIMITER_OFF, no depth, no finite ceiling).
 * No request, no target or a batch that has not run: JB_ERR_INVALID. */
int jb_batch_limiter_report(jb_batch *b, size_t utt, jb_limiter_report *out);
/* New (none).  L and H of opts (NULL: the defaults) at hz and the smoothing window w[0..L]: the interior of a Hann
 * window of L + 3 points, normalised to sum 1, computed in extended precision and symmetric.  Each pointer may be NULL;
 * cap below L + 1 with w given: JB_ERR_BUFFER.  2 L + H above 2048: JB_ERR_UNSUPPORTED. */
int jb_limiter_window(uint32_t hz, const jb_limiter_opts *opts, uint32_t *L, uint32_t *H, double *w, size_t cap);
/* New (none).  The rule above in plain C++ on the host; no GPU is touched.  x[0..n) at hz under `gain` (linear) and
 * the ceiling (dBFS or dBTP by peak_mode; +INFINITY: none); y must hold n samples; report may be NULL. */
int jb_limiter_host(const double *x, uint64_t n, uint32_t hz, double gain, double ceiling_dbfs, uint32_t peak_mode,
                    const jb_limiter_opts *opts, double *y, jb_limiter_report *report);
int jb_limiter_host_i16(const double *x, uint64_t n, uint32_t hz, double gain, double ceiling_dbfs,
                        uint32_t peak_mode, const jb_limiter_opts *opts, int16_t *y, jb_limiter_report *report);
/* New (none).  The stage on PCM the caller holds, on `device` (-1 = current): the seam of the same kernel.  Utterance
 * u is n_in[u] f64 samples at hz[u] under gain[u], ceiling_dbfs[u], peak_mode[u] and opts[u]; out[u] = its n_in[u]
 * limited samples, f64 or by the 16-bit sink's rule, library-owned (jb_limiter_free each); reports (may be NULL): [n].
 * The same samples and arguments give the same bits from this seam, from jb_limiter_host and from the batch path. */
int jb_limiter_pcm_batch(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz, const double *gain,
                         const double *ceiling_dbfs, const uint32_t *peak_mode, const jb_limiter_opts *opts,
                         int32_t device, double **out, jb_limiter_report *reports);
int jb_limiter_pcm_batch_i16(const double *const *in, const size_t *n_in, size_t n, const uint32_t *hz,
                             const double *gain, const double *ceiling_dbfs, const uint32_t *peak_mode,
                             const jb_limiter_opts *opts, int32_t device, int16_t **out, jb_limiter_report *reports);
void jb_limiter_free(void *p);

/* ---- multi-GPU (SURVEY 8b "device_ids[] / n_devices", 8e) ----------------------------------
 * Utterances are independent, so a batch shards over the GPUs of a node with no data-path
 * collective: static LPT partition by length, one host thread per device, results in the caller's
 * order.  A device may be listed more than once (two shares run side by side on it). */
/* part_of[i] = bin of item i: items heaviest first (ties: lower index), each onto the currently
 * lightest bin (ties: lower bin).  The rule jbonsai_amd/shard.py states for one-process-per-GPU drivers. */
int jb_lpt_partition(const uint64_t *weights, size_t n, size_t n_parts, uint32_t *part_of);
/* jb_paramgen_vocode_batch over a device list (weights = frames per utterance; opts->device is ignored). */
int jb_paramgen_vocode_batch_multi(const jb_voice_desc *voice, const jb_state_utt *utts, size_t n_utts,
                                   const jb_batch_opts *opts, const int32_t *devices, size_t n_devices,
                                   double *const *pcm, size_t *n_samples);

/* ---- PCM gather over RCCL (north_star: "RCCL over xGMI only to gather output PCM") --------
 * One process (or thread) per GPU synthesises its share; nothing is exchanged on the data path.  The one
 * optional exchange is the sink that wants every rank's PCM slab on ONE GPU: variable-length slabs, so
 * point to point -- grouped ncclSend / ncclRecv, one message per peer (over xGMI every peer has its own link
 * into the root).  The reference has no counterpart (single process, single utterance).
 * RCCL is bound at run time (dlopen "librccl.so.1": the copy the process already holds, else ROCm's); a
 * communicator of one rank never loads it.  The unique id travels between the ranks by the caller's own
 * means (a file, an environment variable, the launcher's store): it is control plane. */
#define JB_COMM_ID_BYTES 128 /* ncclUniqueId */
typedef struct jb_comm jb_comm;
typedef struct jb_gathered jb_gathered;
/* rank 0: a fresh id for jb_comm_init on every rank (ncclGetUniqueId). */
int jb_comm_unique_id(uint8_t *id, size_t cap);
/* ncclCommInitRank on `device` (-1 = current); collective over the n_ranks ranks.  n_ranks == 1: id may be NULL. */
int jb_comm_init(const uint8_t *id, int n_ranks, int rank, int32_t device, jb_comm **out);
int jb_comm_rank(const jb_comm *c);
int jb_comm_size(const jb_comm *c);
void jb_comm_free(jb_comm *c);
/* Collective: every rank passes its (finished or running: the call waits) batch.  On `root`, *out holds
 * one device slab per rank (f64 samples, or i16 for JB_BATCH_PCM_I16 batches; utterance i of rank r's batch
 * at its jb_batch_pcm_offset); the root's own entry aliases its batch's slab (no copy: valid while that
 * batch lives).  On the other ranks *out is NULL.  *ms (may be NULL) = wall time of the exchange.
 * Failure is collective: a rank whose local work failed still calls this (b = NULL is allowed for it) and
 * EVERY rank then returns an error instead of blocking; so does every rank when the root cannot allocate its
 * receive slabs or when f64 and 16-bit slabs are mixed.  RCCL is bound at first use with dlopen
 * ("librccl.so.1"; JB_RCCL_LIBRARY = full path of another library to bind, e.g. the test double of
 * tests/fake_rccl that lets several ranks share one device). */
int jb_gather_pcm(jb_comm *c, jb_batch *b, int root, jb_gathered **out, float *ms);
size_t jb_gathered_samples(const jb_gathered *g, int rank);
/* Bytes per sample of the gathered slabs: 8 (f64) or 2 (the 16-bit sink) -- what the SENDING ranks' batches
 * were made with (a root whose own batch is empty takes it from them). */
size_t jb_gathered_sample_bytes(const jb_gathered *g);
void *jb_gathered_device(const jb_gathered *g, int rank);
/* Device-to-host copy of rank r's slab (cap in BYTES). */
int jb_gathered_read(const jb_gathered *g, int rank, void *dst, size_t cap_bytes);
void jb_gathered_free(jb_gathered *g);

/* ------------------------------------------------------------------------ */
/* (2) engine level                                                         */
/* ------------------------------------------------------------------------ */
typedef struct jb_engine jb_engine;
typedef struct jb_generator jb_generator;

/* Engine::load (src/engine.rs:257) / load_from_bytes (:263). */
int jb_engine_load(const char *const *paths, size_t n, jb_engine **out);
int jb_engine_load_from_bytes(const uint8_t *const *bufs, const size_t *lens, size_t n,
                              jb_engine **out);
/* Engine::new(VoiceSet, Condition) (src/engine.rs:289-291): an engine over the voices of `voices_of`
 * (shared, as the reference's Arc<Voice>) with a copy of the Condition of `condition_of`; the same engine
 * for both = Engine::clone.  JB_ERR_WEIGHT if the condition was made for another number of voices. */
int jb_engine_new(const jb_engine *voices_of, const jb_engine *condition_of, jb_engine **out);
void jb_engine_free(jb_engine *e);

/* Condition accessors (src/engine.rs:127-243); setters clamp like the reference. */
int jb_engine_set_sampling_frequency(jb_engine *e, size_t v);
size_t jb_engine_get_sampling_frequency(const jb_engine *e);
int jb_engine_set_fperiod(jb_engine *e, size_t v);
size_t jb_engine_get_fperiod(const jb_engine *e);
int jb_engine_set_volume(jb_engine *e, double db);
double jb_engine_get_volume(const jb_engine *e);
int jb_engine_set_msd_threshold(jb_engine *e, size_t stream, double v);
double jb_engine_get_msd_threshold(const jb_engine *e, size_t stream);
int jb_engine_set_gv_weight(jb_engine *e, size_t stream, double v);
double jb_engine_get_gv_weight(const jb_engine *e, size_t stream);
int jb_engine_set_phoneme_alignment_flag(jb_engine *e, int flag);
int jb_engine_get_phoneme_alignment_flag(const jb_engine *e);
/* New (no reference counterpart; the reference has no batches).  By default an utterance's audio depends,
 * to about 1e-10 relative, on what else is in its batch: the time-chunked vocoder picks its chunk length from
 * the batch's total length and hand-offs are certified to 1e-9 of the filter state, not to the last bit
 * (README.md:124 of the reference advertises bitwise-identical audio between builds).  With this flag every
 * batch of the engine runs with JB_BATCH_SERIAL | JB_BATCH_SERIAL_GV -- one wave per utterance, the
 * reference-shaped recursion from zero state, and the GV sums in the reference's serial order (parameter tracks
 * bit-exact against the CPU path) -- and the same labels give the SAME BITS alone, in any batch, through the
 * generator and on any device count; throughput drops to one SIMD per utterance. */
int jb_engine_set_batch_invariant(jb_engine *e, int flag);
int jb_engine_get_batch_invariant(const jb_engine *e);
/* New.  Fast batch-invariant mode: every batch of the engine carries JB_BATCH_INVARIANT (see there), so the same
 * labels give the SAME BITS alone, in any batch (jb_synthesize_batch[_each|_multi], the 16-bit sink) and through
 * jb_generator_new, at close to the throughput of the default mode.  The bits are a function of the voice set, the
 * Condition, the labels, the library build and the GPU architecture; they differ from the default mode's and from
 * jb_engine_set_batch_invariant's, and stay within the same tolerance of the serial recursion.
 * jb_engine_set_batch_invariant, when also set, takes precedence (its bits, its speed).  jb_engine_new copies the
 * flag with the rest of the Condition; the engines of jb_synthesize_batch_each must agree on it. */
int jb_engine_set_fast_invariant(jb_engine *e, int flag);
int jb_engine_get_fast_invariant(const jb_engine *e);
/* New.  Rate of the audio the engine's entries return: jb_synthesize, jb_synthesize_batch[_i16], _each[_i16] (each
 * engine's own rate for its utterance: it is not among the fields the engines must agree on), _multi and the
 * generator convert the voice-rate PCM on the device before it is copied out (jb_batch_set_output_rate).  0 (the
 * default) or the voice's rate = native: unchanged output.  jb_engine_new copies it with the Condition.  Unlike
 * jb_engine_set_sampling_frequency (Condition::set_sampling_frequency, the rate the vocoder converts pitch with),
 * this resamples.  A pair the converter does not support fails at synthesis with JB_ERR_UNSUPPORTED. */
int jb_engine_set_output_sampling_frequency(jb_engine *e, size_t hz);
size_t jb_engine_get_output_sampling_frequency(const jb_engine *e);
/* New.  Loudness target (LUFS) of the audio the engine's entries return: jb_synthesize, jb_synthesize_batch[_i16],
 * _each[_i16] (each engine's own target and ceiling for its utterance: they are not among the fields the engines
 * must agree on), _multi and the generator normalize on the device (jb_batch_set_loudness_target).  NaN (the
 * default) = off: nothing is measured and the output is unchanged, whatever the ceiling.  jb_engine_new copies both
 * with the Condition. */
int jb_engine_set_loudness_target(jb_engine *e, double lufs);
double jb_engine_get_loudness_target(const jb_engine *e);
/* New.  Peak ceiling (dBFS) that goes with the loudness target: default 0; +INFINITY = none. */
int jb_engine_set_peak_ceiling(jb_engine *e, double dbfs);
double jb_engine_get_peak_ceiling(const jb_engine *e);
/* New.  What that ceiling bounds: JB_PEAK_SAMPLE (the default) or JB_PEAK_TRUE (dBTP, jb_batch_set_peak_mode); any
 * other value: JB_ERR_INVALID.  jb_engine_new copies it with the Condition.  Honoured where the target is: by
 * jb_synthesize, _batch[_i16], _each[_i16] (each utterance's engine's own mode, like its target and ceiling), the
 * _flac and _multi entries and the generator. */
int jb_engine_set_peak_mode(jb_engine *e, uint32_t mode);
uint32_t jb_engine_get_peak_mode(const jb_engine *e);
/* New.  What one gain of the loudness target covers: each utterance (JB_LOUDNESS_PER_UTTERANCE, the default) or the
 * whole request (JB_LOUDNESS_PER_REQUEST): all utterances of one jb_synthesize_batch* call -- the f64, _i16,
 * _flac[_meta], _formatted, _adpcm and _each* forms -- are one loudness group (jb_batch_set_loudness_groups), so
 * their relative levels survive; such a request runs as one batch.  In the _each forms the engines must then agree
 * on scope, target, ceiling, peak mode and output rate: JB_ERR_INVALID naming the field, before any device is
 * touched.  jb_synthesize and the generator are a group of one: their output is unchanged.  The _multi entries
 * refuse an engine with per-request scope (a group does not span devices): JB_ERR_INVALID.  Any other value:
 * JB_ERR_INVALID.  Without a target the scope has no effect. */
#define JB_LOUDNESS_PER_UTTERANCE 0
#define JB_LOUDNESS_PER_REQUEST 1
int jb_engine_set_loudness_scope(jb_engine *e, uint32_t scope);
uint32_t jb_engine_get_loudness_scope(const jb_engine *e);
/* New.  The output filter of the audio the engine's entries return (see "Filter"): jb_synthesize, every
 * jb_synthesize_batch* and jb_synthesize_programme* form, _each* (each engine's own filter for its utterance: it is
 * not among the fields the engines must agree on), _multi and the generator filter on the device
 * (jb_batch_set_filter), behind the output rate and in front of the loudness target.  NULL or a filter without
 * sections (the default) = off: the output is unchanged.  Checked here at the engine's present output rate and again
 * at synthesis.  jb_engine_new copies it with the Condition. */
int jb_engine_set_filter(jb_engine *e, const jb_filter *f);
int jb_engine_get_filter(const jb_engine *e, jb_filter *out);
/* New.  The impulse response of the audio the engine's entries return (see "Convolution"): wherever the engine's
 * filter applies, in front of its sections (jb_batch_set_fir).  The taps are copied.  NULL or a request without taps
 * (the default) = off: the output is unchanged.  Checked here at the engine's present output rate and again at
 * synthesis.  jb_engine_new copies it with the Condition. */
int jb_engine_set_fir(jb_engine *e, const jb_fir *f);
/* New.  The frame request of the features the engine's entries return (see "Frame conditioning"): read by every later
 * *_fbank and *_mfcc synthesis entry, _batch, _each and _programme included (the engines of one _each call must agree).
 * Checked here on its own and beside the entry's options at synthesis.  NULL (the default) = none.  jb_engine_new copies
 * it with the Condition. */
int jb_engine_set_frame_opts(jb_engine *e, const jb_frame_opts *fr);
/* New.  The room of the audio the engine's entries return (see "Room responses"): wherever the engine's impulse
 * response applies, in its place (jb_batch_set_room) -- the room and jb_engine_set_fir share one slot, the later call
 * replaces the earlier.  flags: JB_ROOM_VARY or 0.  With JB_ROOM_VARY the utterance of index k in the call gets the
 * positions jb_room_vary(seed, k, r->size, margin, ..) in the one room (r's own source and mic are not read; the
 * generator's utterance has index 0); without it seed and margin are not read.  NULL (the default) = off: the output
 * is unchanged.  Checked here at the engine's present output rate (with JB_ROOM_VARY: for index 0) and again at
 * synthesis, where the rooms are generated on the batch's device.  jb_engine_new copies it with the Condition. */
int jb_engine_set_room(jb_engine *e, const jb_room *r, uint32_t flags, uint64_t seed, double margin);
/* New.  The noise of the audio the engine's entries return (see "Noise"): wherever the engine's impulse response
 * applies, behind it and in front of the filter's sections (jb_batch_set_noise) -- jb_synthesize, every
 * jb_synthesize_batch* and jb_synthesize_programme* form, the _each* forms (each engine's own request for its
 * utterance) and the generator (whose converted utterance is read whole by the first step).  With JB_NOISE_VARY the
 * utterance of index k in the call uses jb_noise_vary(seed, k, ..).  The bed is copied.  NULL, or no bed with
 * JB_NOISE_BED (the default) = off: the output is unchanged.  Checked here at the engine's present output rate and
 * again at synthesis.  jb_engine_new copies it with the Condition; jb_engine_get_noise's bed points into the engine's
 * copy (valid until the next jb_engine_set_noise). */
int jb_engine_set_noise(jb_engine *e, const jb_noise *req);
/* New (none).  While set, every jb_synthesize_programme* entry called with n utterances MIXES them instead of joining
 * them ("Mix" below), whatever its sink: utterance u starts at jb_join_ms_to_samples(lead_ms + place[u].start_ms) under
 * place[u].gain_db, trail_ms is every member's pad_after, fade_ms every member's fades, and gap_ms must be 0.  starts
 * receives the members' starts as with a join.  A call with another utterance count or a non-zero gap: JB_ERR_INVALID
 * before any device is touched.  Here: a negative or non-finite start_ms, a gain_db or options jb_batch_set_mix would
 * refuse: JB_ERR_INVALID.  opts may be NULL (no flags); NULL, 0 withdraws the setting.  The getter writes *n, *opts and,
 * where place is given, the n places (cap below n: JB_ERR_BUFFER); any out pointer may be NULL. */
int jb_engine_set_programme_mix(jb_engine *e, const jb_mix_place *place, size_t n, const jb_mix_opts *opts);
int jb_engine_get_programme_mix(const jb_engine *e, jb_mix_place *place, size_t cap, size_t *n, jb_mix_opts *opts);
int jb_engine_get_noise(const jb_engine *e, jb_noise *out);
/* New.  The limiter of the audio the engine's entries return (see "Limiter"): jb_synthesize, every
 * jb_synthesize_batch* and jb_synthesize_programme* form and _each* (each engine's own request for its utterance: not
 * among the fields the engines must agree on, except inside a per-request loudness group) ask the batch for it
 * (jb_batch_set_limiter).  It takes effect with a loudness target and a ceiling.  NULL (the default) = off.  Checked
 * here; jb_engine_new copies it with the Condition.  jb_engine_get_limiter returns 1 and the request as it was given
 * in *out, or 0 and zeros where there is none. */
int jb_engine_set_limiter(jb_engine *e, const jb_limiter_opts *opts);
int jb_engine_get_limiter(const jb_engine *e, jb_limiter_opts *out);
/* New.  Where the per-label decision-tree search of the front half runs (Model::get_index for the duration model and
 * every stream model, state and voice, and the GV switch question).  The default is the host, as before: nothing new
 * runs and nothing is allocated.  On the device one wave searches one label (jb_treesearch.hip); label parsing, the
 * duration estimate, the GV pdf of the first label and batch creation stay on the host, and the results are bit for
 * bit the host's, errors included.  A request holding a label above 1023 bytes is searched on the host.  Any other
 * value: JB_ERR_INVALID.  jb_engine_new copies the mode with the Condition; the engines of an _each call must agree
 * on it.  Honoured by jb_synthesize, _batch[_i16], _each[_i16], the _flac and _multi entries (each device thread with
 * its own device's tables), jb_generator_new and jb_engine_states (those two on the current device). */
#define JB_SEARCH_HOST 0   /* default: the host threads search */
#define JB_SEARCH_AUTO 1   /* device when the request has at least the measured number of label lines (1,024), else host */
#define JB_SEARCH_DEVICE 2 /* device for every request with at least one label */
int jb_engine_set_tree_search(jb_engine *e, uint32_t mode);
uint32_t jb_engine_get_tree_search(const jb_engine *e);
/* labels whose trees were searched on a device for this engine so far (0 in host mode); utterance u of an _each call
 * counts for engines[u] */
uint64_t jb_engine_device_searched_labels(const jb_engine *e);
int jb_engine_set_speed(jb_engine *e, double v);
double jb_engine_get_speed(const jb_engine *e);
int jb_engine_set_alpha(jb_engine *e, double v);
double jb_engine_get_alpha(const jb_engine *e);
int jb_engine_set_beta(jb_engine *e, double v);
double jb_engine_get_beta(const jb_engine *e);
int jb_engine_set_additional_half_tone(jb_engine *e, double v);
double jb_engine_get_additional_half_tone(const jb_engine *e);
size_t jb_engine_num_voices(const jb_engine *e);
size_t jb_engine_num_streams(const jb_engine *e);
size_t jb_engine_num_states(const jb_engine *e);
/* InterporationWeight setters (src/model/interporation_weight.rs:48-126);
 * which: 0 duration, 1 parameter[stream], 2 gv[stream]. */
int jb_engine_set_interpolation_weight(jb_engine *e, int which, size_t stream, const double *w,
                                       size_t n);
/* InterporationWeight::{get_duration, get_parameter, get_gv} (interporation_weight.rs:115-125): *n = number
 * of voices; w (may be NULL) receives the weights, JB_ERR_BUFFER if cap is too small. */
int jb_engine_get_interpolation_weight(const jb_engine *e, int which, size_t stream, double *w, size_t cap,
                                       size_t *n);

/* Engine::synthesize (src/engine.rs:294): label lines ("label" or "start end label").
 * *pcm is library-owned; release with jb_pcm_free.  Zero labels => n_samples 0. */
int jb_synthesize(const jb_engine *e, const char *const *label_lines, size_t n_lines,
                  double **pcm, size_t *n_samples);
void jb_pcm_free(double *pcm);
/* 16-bit mono RIFF/WAVE writer for the i16 sink -- what the reference's examples do with hound
 * (examples/is-bonsai/main.rs:37-49: 1 channel, 16 bits, SampleFormat::Int).  JB_ERR_MODEL (Io) if the
 * file cannot be written. */
int jb_write_wav_i16(const char *path, const int16_t *pcm, size_t n_samples, uint32_t sampling_frequency);
/* Same from f64 samples, converting like jb's i16 sink: value.min(32767).max(-32768) as i16. */
int jb_write_wav_f64(const char *path, const double *pcm, size_t n_samples, uint32_t sampling_frequency);
/* Mono RIFF/WAVE of formatted bytes (n_samples x jb_format_bytes_per_sample of them): format tag 1 for JB_FMT_S16 and
 * _S24, 3 for _F32, 7 for _ULAW, 6 for _ALAW; the non-PCM tags carry cbSize = 0 and a fact chunk; a data chunk of odd
 * length is padded. */
int jb_write_wav_formatted(const char *path, const uint8_t *bytes, size_t n_samples, uint32_t sampling_frequency,
                           uint32_t format);

/* Mono RIFF/WAVE of IMA ADPCM blocks: fmt chunk with tag 0x11, 1 channel, nAvgBytesPerSec = floor(hz A / spb),
 * nBlockAlign A, 4 bits, cbSize 2, wSamplesPerBlock spb; a fact chunk holding n_samples; the data chunk. */
int jb_write_wav_adpcm(const char *path, const uint8_t *bytes, size_t n_bytes, size_t n_samples,
                       uint32_t sampling_frequency, uint32_t block_align);

/* Batched synthesize: utterance u has lines [line_off[u], line_off[u+1]).  New
 * entry (the reference is single-utterance); a Rust `Engine::synthesize_batch`
 * would sit on it.  pcm[u] library-owned (jb_pcm_free each). */
int jb_synthesize_batch(const jb_engine *e, const char *const *label_lines,
                        const size_t *line_off, size_t n_utts, int32_t device, double **pcm,
                        size_t *n_samples);
/* Same with the 16-bit sink fused into the vocoder (what the reference's callers do with the
 * result: clamp to i16 and write WAV, examples/is-bonsai/main.rs:37-49): a quarter of the PCIe
 * traffic.  pcm[u] library-owned (jb_pcm_i16_free each). */
int jb_synthesize_batch_i16(const jb_engine *e, const char *const *label_lines,
                            const size_t *line_off, size_t n_utts, int32_t device,
                            int16_t **pcm, size_t *n_samples);
void jb_pcm_i16_free(int16_t *pcm);
/* jb_synthesize_batch with one engine per utterance: utterance u is Engine::synthesize (src/engine.rs:250-266) of
 * engines[u], under engines[u]'s whole Condition (speed, alignment flag, half tone, volume, alpha, beta, GV weights,
 * MSD thresholds, the three kinds of interpolation weight), in one batch.  New entry (the reference has no batch).
 * The engines share one voice set -- engines made from one another with jb_engine_new (Engine::clone) -- and agree
 * on sampling_frequency, fperiod, stage, use_log_gain, the batch-invariant and the fast-invariant flags and the tree-search mode; otherwise JB_ERR_INVALID, with
 * jb_last_error naming what differs, before any device is touched.  pcm[u] library-owned (jb_pcm_free each). */
int jb_synthesize_batch_each(const jb_engine *const *engines, const char *const *label_lines, const size_t *line_off,
                             size_t n_utts, int32_t device, double **pcm, size_t *n_samples);
/* Same with the 16-bit sink (jb_synthesize_batch_i16); pcm[u]: jb_pcm_i16_free each. */
int jb_synthesize_batch_each_i16(const jb_engine *const *engines, const char *const *label_lines,
                                 const size_t *line_off, size_t n_utts, int32_t device, int16_t **pcm,
                                 size_t *n_samples);
/* New.  FLAC forms of jb_synthesize (one utterance, current device), jb_synthesize_batch_i16 and
 * jb_synthesize_batch_each_i16: flac[u] is the stream of what the _i16 entry returns (each engine's output rate and
 * loudness target honoured the same way), n_bytes[u] bytes, library-owned (jb_flac_free each).  opts as
 * jb_batch_set_flac's. */
int jb_synthesize_flac(const jb_engine *e, const char *const *label_lines, size_t n_lines, const jb_flac_opts *opts,
                       uint8_t **flac, size_t *n_bytes);
int jb_synthesize_batch_flac(const jb_engine *e, const char *const *label_lines, const size_t *line_off, size_t n_utts,
                             int32_t device, const jb_flac_opts *opts, uint8_t **flac, size_t *n_bytes);
int jb_synthesize_batch_each_flac(const jb_engine *const *engines, const char *const *label_lines,
                                  const size_t *line_off, size_t n_utts, int32_t device, const jb_flac_opts *opts,
                                  uint8_t **flac, size_t *n_bytes);
/* New.  The same with a metadata request (jb_flac_meta; NULL or zeros: the entries above). */
int jb_synthesize_flac_meta(const jb_engine *e, const char *const *label_lines, size_t n_lines,
                            const jb_flac_opts *opts, const jb_flac_meta *meta, uint8_t **flac, size_t *n_bytes);
int jb_synthesize_batch_flac_meta(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                  size_t n_utts, int32_t device, const jb_flac_opts *opts, const jb_flac_meta *meta,
                                  uint8_t **flac, size_t *n_bytes);
int jb_synthesize_batch_each_flac_meta(const jb_engine *const *engines, const char *const *label_lines,
                                       const size_t *line_off, size_t n_utts, int32_t device, const jb_flac_opts *opts,
                                       const jb_flac_meta *meta, uint8_t **flac, size_t *n_bytes);
/* New.  Formatted forms of jb_synthesize (one utterance, current device), jb_synthesize_batch and
 * jb_synthesize_batch_each: bytes[u] is what the f64 entry returns (each engine's output rate, loudness target,
 * ceiling and peak mode honoured the same way) in opts->format, n_bytes[u] bytes, library-owned (jb_format_free
 * each). */
int jb_synthesize_formatted(const jb_engine *e, const char *const *label_lines, size_t n_lines,
                            const jb_format_opts *opts, uint8_t **bytes, size_t *n_bytes);
int jb_synthesize_batch_formatted(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                  size_t n_utts, int32_t device, const jb_format_opts *opts, uint8_t **bytes,
                                  size_t *n_bytes);
int jb_synthesize_batch_each_formatted(const jb_engine *const *engines, const char *const *label_lines,
                                       const size_t *line_off, size_t n_utts, int32_t device,
                                       const jb_format_opts *opts, uint8_t **bytes, size_t *n_bytes);
/* New.  IMA ADPCM forms of jb_synthesize (one utterance, current device), jb_synthesize_batch_i16 and
 * jb_synthesize_batch_each_i16: bytes[u] holds the blocks of what the PCM entry returns (each engine's output rate,
 * loudness target, ceiling and peak mode honoured the same way; with block_align 0 each utterance's A follows its own
 * rate), n_bytes[u] bytes, library-owned (jb_adpcm_free each); n_samples[u] (may be NULL) the samples they encode. */
int jb_synthesize_adpcm(const jb_engine *e, const char *const *label_lines, size_t n_lines, const jb_adpcm_opts *opts,
                        uint8_t **bytes, size_t *n_bytes, size_t *n_samples);
int jb_synthesize_batch_adpcm(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                              size_t n_utts, int32_t device, const jb_adpcm_opts *opts, uint8_t **bytes,
                              size_t *n_bytes, size_t *n_samples);
int jb_synthesize_batch_each_adpcm(const jb_engine *const *engines, const char *const *label_lines,
                                   const size_t *line_off, size_t n_utts, int32_t device, const jb_adpcm_opts *opts,
                                   uint8_t **bytes, size_t *n_bytes, size_t *n_samples);
/* New (none).  Filterbank forms of jb_synthesize (one utterance, current device), jb_synthesize_batch and
 * jb_synthesize_batch_each (see "Filterbank features"): bytes[u] = the [n_frames[u]][opts->n_mels] frames of utterance
 * u's final f64 PCM at its engine's output rate, n_bytes[u] bytes, library-owned (jb_fbank_free each); n_frames (may
 * be NULL).  Options that some utterance's rate refuses: JB_ERR_INVALID naming the field. */
int jb_synthesize_fbank(const jb_engine *e, const char *const *label_lines, size_t n_lines, const jb_fbank_opts *opts,
                        uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
int jb_synthesize_batch_fbank(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                              size_t n_utts, int32_t device, const jb_fbank_opts *opts, uint8_t **bytes,
                              size_t *n_bytes, size_t *n_frames);
/* New.  The same for the cepstral features (jb_batch_set_mfcc): bytes[u] = the rows of utterance u, library-owned
 * (jb_mfcc_free each); n_frames (may be NULL) gets each output's frames. */
int jb_synthesize_mfcc(const jb_engine *e, const char *const *label_lines, size_t n_lines, const jb_fbank_opts *fopts,
                       const jb_mfcc_opts *opts, uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
int jb_synthesize_batch_mfcc(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                             size_t n_utts, int32_t device, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts,
                             uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
int jb_synthesize_batch_each_mfcc(const jb_engine *const *engines, const char *const *label_lines,
                                  const size_t *line_off, size_t n_utts, int32_t device, const jb_fbank_opts *fopts,
                                  const jb_mfcc_opts *opts, uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
int jb_synthesize_batch_each_fbank(const jb_engine *const *engines, const char *const *label_lines,
                                   const size_t *line_off, size_t n_utts, int32_t device, const jb_fbank_opts *opts,
                                   uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
/* New.  Mel spectrograms (see "Mel spectrograms") straight from the engine, as the _fbank entries above: bytes[u] = the
 * [n_frames[u]][opts->n_mels] frames of utterance u's final f64 PCM at its engine's output rate, n_bytes[u] bytes,
 * library-owned (jb_melspec_free each); n_frames may be NULL.  For Whisper's front end set the engines' output rate
 * to 16 kHz. */
int jb_synthesize_melspec(const jb_engine *e, const char *const *label_lines, size_t n_lines,
                          const jb_melspec_opts *opts, uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
int jb_synthesize_batch_melspec(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                size_t n_utts, int32_t device, const jb_melspec_opts *opts, uint8_t **bytes,
                                size_t *n_bytes, size_t *n_frames);
int jb_synthesize_batch_each_melspec(const jb_engine *const *engines, const char *const *label_lines,
                                     const size_t *line_off, size_t n_utts, int32_t device,
                                     const jb_melspec_opts *opts, uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
/* The same two over a device list: the utterances are split by LPT on their label counts (the frame
 * counts are known only after the front half), one host thread per device runs jb_synthesize_batch's
 * path on its share (front half on that thread's workers, GPU work on that device). */
int jb_synthesize_batch_multi(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                              size_t n_utts, const int32_t *devices, size_t n_devices, double **pcm,
                              size_t *n_samples);
int jb_synthesize_batch_i16_multi(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                  size_t n_utts, const int32_t *devices, size_t n_devices, int16_t **pcm,
                                  size_t *n_samples);

/* Host front half only (tree search + durations): fills a state-level utterance
 * owned by the returned handle; used by tests and by jb_synthesize itself. */
typedef struct jb_states jb_states;
int jb_engine_states(const jb_engine *e, const char *const *label_lines, size_t n_lines,
                     jb_states **out);
const jb_state_utt *jb_states_utt(const jb_states *s);
/* Models::duration() (src/model/mod.rs:80-92): the (mean, variance) pairs the durations were estimated from, blended
 * over the voices with the duration weights -- [num_states][2] doubles owned by the handle (NULL for no states).
 * What the reference's `multiple_models` test pins for two voices (src/model/mod.rs:395-428). */
const double *jb_states_duration_params(const jb_states *s);
const jb_voice_desc *jb_engine_voice_desc(const jb_engine *e);
void jb_states_free(jb_states *s);

/* Model introspection (pub fields of Voice/Model, src/model/voice/model.rs:12-82).
 * kind: 0 duration model, 1+s stream model s, 4+s GV model of stream s. */
int jb_engine_model_shape(const jb_engine *e, size_t voice, int kind, size_t *ntree,
                          size_t *pdf_len);
/* pdf table of one tree: *table -> npdf*pdf_len f32 (means, variances, [msd]); engine-owned. */
int jb_engine_pdf_table(const jb_engine *e, size_t voice, int kind, size_t tree,
                        const float **table, size_t *npdf);
/* Model::get_index (src/model/voice/model.rs:51-68): tree_state = matched tree's state
 * (or -1 when none has that state index), pdf_index 1-based. */
int jb_engine_tree_index(const jb_engine *e, size_t voice, int kind, int state_index,
                         const char *label, int *tree_state, int *pdf_index);

/* New.  The device tree search on labels the caller holds (jb_resample_pcm_batch's kind): bare label strings, no
 * times, no shape check, on `device` (-1 = current).  tree_state / pdf_index: [n_labels][n_voices][1 + nstream][nstate];
 * kind k = 0 is the duration model (entry s = 0 is state_index 2; its entries s > 0 are -1 / 0), kind 1 + si stream
 * si with entry s = state_index 2 + s: exactly the two values jb_engine_tree_index(e, voice, k, state_index, label)
 * returns, out-of-range leaves included (no error is raised for them here).  gv_on[n_labels] = 1 unless the voice's
 * GV_OFF_CONTEXT question matches the label.  Each output may be NULL.  A label above 1023 bytes:
 * JB_ERR_UNSUPPORTED naming it.  Not counted by jb_engine_device_searched_labels. */
int jb_tree_search_batch(const jb_engine *e, const char *const *labels, size_t n_labels, int32_t device,
                         int32_t *tree_state, int32_t *pdf_index, uint8_t *gv_on);
/* Same outputs from the scalar walker over the same flattened tables (any label length); no GPU is touched. */
int jb_tree_search_flat_host(const jb_engine *e, const char *const *labels, size_t n_labels, int32_t *tree_state,
                             int32_t *pdf_index, uint8_t *gv_on);

/* Engine::generator (src/engine.rs:301) + SpeechGenerator (src/speech.rs:25-96). */
int jb_generator_new(const jb_engine *e, const char *const *label_lines, size_t n_lines,
                     jb_generator **out);
/* SpeechGenerator::new(fperiod, vocoder, spectrum, lf0, lpf) on tracks the caller holds (src/speech.rs:25-50),
 * for jb_generator_step = generate_step (:65-82).  Of `voice` the Vocoder::new arguments are read, as in
 * jb_batch_create_from_tracks; the three panics of SpeechGenerator::new come back as JB_ERR_INVALID with the
 * reference's messages.  opts may be NULL (current device, defaults); the 16-bit sink flag is ignored
 * (generate_step hands out f64 samples). */
int jb_generator_new_from_tracks(const jb_voice_desc *voice, const jb_track_utt *utt, const jb_batch_opts *opts,
                                 jb_generator **out);
size_t jb_generator_fperiod(const jb_generator *g);
size_t jb_generator_synthesized_frames(const jb_generator *g);
size_t jb_generator_total_frames(const jb_generator *g);
/* generate_step: writes fperiod samples to buf, returns fperiod, 0 when exhausted,
 * or a negative jb_status (JB_ERR_BUFFER where the reference panics).
 * With an output rate (jb_engine_set_output_sampling_frequency, L/M of the voice's rate): step k writes the output
 * samples [ceil(k F L / M), ceil((k + 1) F L / M)), F = fperiod, and returns their count (at 22.05 kHz from 48 kHz
 * with F = 240: 110 or 111); buf must hold ceil(F L / M) samples, else JB_ERR_BUFFER.  The steps concatenate to
 * jb_synthesize's output at that rate; the first step waits for the whole utterance (no serially served head).
 * With a loudness target (jb_engine_set_loudness_target) the first step waits for the whole utterance as well (the
 * gain needs every sample), and the steps hand out the normalized output. */
long jb_generator_step(jb_generator *g, double *buf, size_t buf_len);
/* Up to max_frames generate_step calls in one: writes n * fperiod samples to buf, n = min(max_frames,
 * frames left, buf_len / fperiod), and returns that sample count (0 when exhausted, JB_ERR_BUFFER if buf
 * cannot hold one frame).  With an output rate: the samples of the n steps by jb_generator_step's rule, n the most
 * frames whose samples fit buf_len (JB_ERR_BUFFER if not one step's ceil(F L / M) fit).  One device-to-host copy for the n frames.
 * How the generator works: the whole utterance is enqueued on the device when the generator is made (the
 * path of jb_synthesize: nothing a SpeechGenerator holds can change between steps) and the call returns
 * without waiting; steps hand out the finished PCM.  While the utterance is still in flight the first 8
 * single-frame steps are served by the serial recursion with persistent state on a side stream, so the
 * first frame does not wait for the last (not with jb_engine_set_fast_invariant: those frames would not have the
 * bits of jb_synthesize, and the first step waits for the whole utterance). */
long jb_generator_step_n(jb_generator *g, double *buf, size_t buf_len, size_t max_frames);
void jb_generator_free(jb_generator *g);

/* New (none: no reference counterpart).  The utterances of one call as ONE programme ("Join" above): the arguments of
 * the jb_synthesize_batch* entry of the same sink plus the join options; one output (*pcm / *bytes, library-owned, freed
 * as the batch entry's outputs are) instead of n_utts.  The engine's output rate, loudness target, ceiling, peak mode
 * and scope hold as in the batch entries: with JB_LOUDNESS_PER_REQUEST the programme has one gain.  The _flac_meta and
 * _adpcm forms join the 16-bit samples (what jb_synthesize_programme_i16 returns), the _formatted form the f64 ones.  starts (NULL or
 * n_utts entries) receives each utterance's first sample within the programme.  n_utts == 0, a NULL join, a negative or
 * non-finite duration or non-zero reserved words: JB_ERR_INVALID before any device is touched. */
int jb_synthesize_programme(const jb_engine *e, const char *const *label_lines, const size_t *line_off, size_t n_utts,
                            int32_t device, const jb_join_opts *join, double **pcm, size_t *n_samples, uint64_t *starts);
int jb_synthesize_programme_i16(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                size_t n_utts, int32_t device, const jb_join_opts *join, int16_t **pcm,
                                size_t *n_samples, uint64_t *starts);
/* New (none).  jb_synthesize_programme with the programme's speech-activity labels ("Speech activity" above) beside its
 * f64 PCM, from the same run: *labels is the [*T][*C] matrix (library-owned: jb_activity_free), with
 * JB_ACTIVITY_MEMBERS one column per utterance of the call, placed at starts[u].  While jb_engine_set_programme_mix is
 * set the programme is a mix, as in every programme entry.  opts is checked before any device is touched. */
int jb_synthesize_programme_activity(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                     size_t n_utts, int32_t device, const jb_join_opts *join,
                                     const jb_activity_opts *opts, double **pcm, size_t *n_samples, uint8_t **labels,
                                     uint64_t *T, uint32_t *C, uint64_t *starts);
int jb_synthesize_programme_flac_meta(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                      size_t n_utts, int32_t device, const jb_flac_opts *opts, const jb_flac_meta *meta,
                                      const jb_join_opts *join, uint8_t **flac, size_t *n_bytes, uint64_t *starts);
/* New (none).  jb_synthesize_programme and jb_synthesize_programme_flac_meta with the stems of the mixture ("Stems of a
 * mix" above) from the same run: stem_of[u] is utterance u's stem id (below n_utts) or JB_MIX_NO_STEM, flags
 * JB_MIX_STEM_LEVELS or 0.  The outputs are the mixture first and the S stems behind it, *n_outputs = 1 + S of them:
 * pcm / flac and n_samples / n_bytes have 1 + n_utts entries, each written output library-owned (jb_join_free /
 * jb_flac_free); reports (may be NULL) has n_utts entries, the first S written, one per stem in output order.  Valid
 * only while jb_engine_set_programme_mix is set: otherwise, and for a NULL stem_of, an unknown flag or an id of n_utts
 * or above, JB_ERR_INVALID before any device is touched.  Any other sink with stems is reached at batch level. */
int jb_synthesize_programme_stems(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                  size_t n_utts, int32_t device, const jb_join_opts *join, const uint32_t *stem_of,
                                  uint32_t flags, double **pcm, size_t *n_samples, size_t *n_outputs,
                                  jb_stem_report *reports, uint64_t *starts);
int jb_synthesize_programme_stems_flac_meta(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                            size_t n_utts, int32_t device, const jb_flac_opts *opts,
                                            const jb_flac_meta *meta, const jb_join_opts *join, const uint32_t *stem_of,
                                            uint32_t flags, uint8_t **flac, size_t *n_bytes, size_t *n_outputs,
                                            jb_stem_report *reports, uint64_t *starts);
int jb_synthesize_programme_formatted(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                      size_t n_utts, int32_t device, const jb_format_opts *opts,
                                      const jb_join_opts *join, uint8_t **bytes, size_t *n_bytes, uint64_t *starts);
int jb_synthesize_programme_adpcm(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                  size_t n_utts, int32_t device, const jb_adpcm_opts *opts, const jb_join_opts *join,
                                  uint8_t **bytes, size_t *n_bytes, size_t *n_samples, uint64_t *starts);
/* New (none).  The programme's filterbank frames: the f64 programme (what jb_synthesize_programme returns) analysed
 * whole; bytes[0], n_bytes[0], n_frames (may be NULL) as jb_synthesize_fbank's. */
int jb_synthesize_programme_fbank(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                  size_t n_utts, int32_t device, const jb_fbank_opts *opts, const jb_join_opts *join,
                                  uint8_t **bytes, size_t *n_bytes, size_t *n_frames, uint64_t *starts);
/* New.  The programme's cepstral features, CMVN over the whole programme; bytes[0], n_bytes[0], n_frames (may be NULL)
 * as jb_synthesize_mfcc's. */
int jb_synthesize_programme_mfcc(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                 size_t n_utts, int32_t device, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts,
                                 const jb_join_opts *join, uint8_t **bytes, size_t *n_bytes, size_t *n_frames,
                                 uint64_t *starts);
/* New.  The programme's mel spectrogram, the range clamp under the whole programme's maximum; bytes[0], n_bytes[0],
 * n_frames (may be NULL) as jb_synthesize_melspec's. */
int jb_synthesize_programme_melspec(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                    size_t n_utts, int32_t device, const jb_melspec_opts *opts,
                                    const jb_join_opts *join, uint8_t **bytes, size_t *n_bytes, size_t *n_frames,
                                    uint64_t *starts);
/* New (none).  The pitch features ("Pitch features" above) of what jb_synthesize, jb_synthesize_batch and
 * jb_synthesize_batch_each return, and of a programme (the normalisation of the log-pitch over the whole programme),
 * tracked on the device from the final f64 PCM of the same run: bytes[u] = output u's [T][width] elements,
 * library-owned (jb_pitch_free), n_bytes[u] their bytes, n_frames[u] (may be NULL) = T; starts as
 * jb_synthesize_programme's.  Options that are refused: JB_ERR_INVALID naming the field, before any device is touched. */
int jb_synthesize_pitch(const jb_engine *e, const char *const *label_lines, size_t n, const jb_pitch_opts *opts,
                        uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
int jb_synthesize_batch_pitch(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                              size_t n_utts, int32_t device, const jb_pitch_opts *opts, uint8_t **bytes,
                              size_t *n_bytes, size_t *n_frames);
int jb_synthesize_batch_each_pitch(const jb_engine *const *engines, const char *const *label_lines,
                                   const size_t *line_off, size_t n_utts, int32_t device, const jb_pitch_opts *opts,
                                   uint8_t **bytes, size_t *n_bytes, size_t *n_frames);
int jb_synthesize_programme_pitch(const jb_engine *e, const char *const *label_lines, const size_t *line_off,
                                  size_t n_utts, int32_t device, const jb_pitch_opts *opts, const jb_join_opts *join,
                                  uint8_t **bytes, size_t *n_bytes, size_t *n_frames, uint64_t *starts);

/* ------------------------------------------------------------------------ */
const char *jb_last_error(void);
int jb_device_count(void);
/* "gfx950" etc. of device `dev` into buf. */
int jb_device_arch(int dev, char *buf, size_t cap);
/* hipDeviceGetPCIBusId of device `dev` ("0000:05:00.0") into buf: which CARD a rank really runs on -- two ranks that
 * report the same id share one GPU, whatever WORLD_SIZE says (bench.py --gpus N puts it into its line). */
int jb_device_pci_bus_id(int dev, char *buf, size_t cap);
const char *jb_version(void);
/* The tolerance of the chunk hand-off check a batch runs with when jb_batch_opts.verify_tol is 0 (1e-9 of the largest
 * state value): the ONE number the PCM gates of the tests and sweeps are derived from (tests/helpers.py). */
double jb_default_verify_tol(void);

#ifdef __cplusplus
}
#endif

/* Layout of every struct that crosses the boundary, as a binding in another language must declare it
 * (LP64, natural alignment: what `#[repr(C)]` and ctypes.Structure give).  Checked here at compile time
 * and against the ctypes mirror in tests/test_abi.py; INTEGRATION.md section 1 carries the same table. */
#if defined(__cplusplus) || (defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L)
#ifdef __cplusplus
#define JB_LAYOUT_ASSERT(c, m) static_assert(c, m)
#else
#define JB_LAYOUT_ASSERT(c, m) _Static_assert(c, m)
#endif
JB_LAYOUT_ASSERT(sizeof(jb_stream_desc) == 56 && offsetof(jb_stream_desc, win_width) == 16 &&
                     offsetof(jb_stream_desc, win_coef) == 48, "jb_stream_desc");
JB_LAYOUT_ASSERT(sizeof(jb_voice_desc) == 216 && offsetof(jb_voice_desc, alpha) == 24 &&
                     offsetof(jb_voice_desc, stream) == 48, "jb_voice_desc");
JB_LAYOUT_ASSERT(sizeof(jb_stream_states) == 64 && offsetof(jb_stream_states, gv_weight) == 48, "jb_stream_states");
JB_LAYOUT_ASSERT(sizeof(jb_state_utt) == 208 && offsetof(jb_state_utt, durations) == 8 &&
                     offsetof(jb_state_utt, stream) == 16, "jb_state_utt");
JB_LAYOUT_ASSERT(sizeof(jb_batch_opts) == 32 && offsetof(jb_batch_opts, verify_tol) == 16 &&
                     offsetof(jb_batch_opts, reserved0) == 24, "jb_batch_opts");
JB_LAYOUT_ASSERT(sizeof(jb_pdf_table) == 16 && offsetof(jb_pdf_table, n_rows) == 8, "jb_pdf_table");
JB_LAYOUT_ASSERT(sizeof(jb_index_stream) == 112 && offsetof(jb_index_stream, weight) == 64 &&
                     offsetof(jb_index_stream, gv_weight) == 96, "jb_index_stream");
JB_LAYOUT_ASSERT(sizeof(jb_index_utt) == 360 && offsetof(jb_index_utt, stream) == 16 &&
                     offsetof(jb_index_utt, lf0_offset) == 352, "jb_index_utt");
JB_LAYOUT_ASSERT(sizeof(jb_track_utt) == 64 && offsetof(jb_track_utt, spectrum_width) == 24 &&
                     offsetof(jb_track_utt, spectrum) == 40, "jb_track_utt");
JB_LAYOUT_ASSERT(sizeof(jb_utt_voc) == 24 && offsetof(jb_utt_voc, beta) == 8 && offsetof(jb_utt_voc, volume) == 16,
                 "jb_utt_voc");
JB_LAYOUT_ASSERT(sizeof(jb_flac_opts) == 16 && offsetof(jb_flac_opts, max_lpc_order) == 4 &&
                     offsetof(jb_flac_opts, reserved) == 8, "jb_flac_opts");
JB_LAYOUT_ASSERT(sizeof(jb_flac_meta) == 16 && offsetof(jb_flac_meta, seek_interval_ms) == 4 &&
                     offsetof(jb_flac_meta, reserved) == 8, "jb_flac_meta");
JB_LAYOUT_ASSERT(sizeof(jb_format_opts) == 16 && offsetof(jb_format_opts, dither) == 4 &&
                     offsetof(jb_format_opts, seed) == 8, "jb_format_opts");
JB_LAYOUT_ASSERT(sizeof(jb_adpcm_opts) == 16 && offsetof(jb_adpcm_opts, reserved) == 4, "jb_adpcm_opts");
JB_LAYOUT_ASSERT(sizeof(jb_mfcc_opts) == 48 && offsetof(jb_mfcc_opts, cmvn) == 12 && offsetof(jb_mfcc_opts, lifter) == 16 &&
                     offsetof(jb_mfcc_opts, var_floor) == 24 && offsetof(jb_mfcc_opts, flags) == 32 &&
                     offsetof(jb_mfcc_opts, reserved) == 36,
                 "jb_mfcc_opts");
JB_LAYOUT_ASSERT(sizeof(jb_fbank_opts) == 64 && offsetof(jb_fbank_opts, n_fft) == 8 &&
                     offsetof(jb_fbank_opts, f_min_hz) == 16 && offsetof(jb_fbank_opts, log_floor) == 32 &&
                     offsetof(jb_fbank_opts, window) == 40 && offsetof(jb_fbank_opts, reserved) == 48,
                 "jb_fbank_opts");
JB_LAYOUT_ASSERT(sizeof(jb_frame_opts) == 32 && offsetof(jb_frame_opts, window) == 8 &&
                     offsetof(jb_frame_opts, flags) == 12 && offsetof(jb_frame_opts, reserved) == 16,
                 "jb_frame_opts");
JB_LAYOUT_ASSERT(sizeof(jb_melspec_opts) == 96 && offsetof(jb_melspec_opts, f_min_hz) == 16 &&
                     offsetof(jb_melspec_opts, floor) == 32 && offsetof(jb_melspec_opts, range) == 40 &&
                     offsetof(jb_melspec_opts, offset) == 48 && offsetof(jb_melspec_opts, mel_scale) == 64 &&
                     offsetof(jb_melspec_opts, flags) == 80 && offsetof(jb_melspec_opts, reserved) == 84,
                 "jb_melspec_opts");
JB_LAYOUT_ASSERT(sizeof(jb_join_utt) == 32 && offsetof(jb_join_utt, fade_out) == 8 &&
                     offsetof(jb_join_utt, pad_before) == 16 && offsetof(jb_join_utt, pad_after) == 24,
                 "jb_join_utt");
JB_LAYOUT_ASSERT(sizeof(jb_mix_utt) == 48 && offsetof(jb_mix_utt, fade_out) == 8 && offsetof(jb_mix_utt, start) == 16 &&
                     offsetof(jb_mix_utt, pad_after) == 24 && offsetof(jb_mix_utt, gain_db) == 32 &&
                     offsetof(jb_mix_utt, reserved2) == 40,
                 "jb_mix_utt");
JB_LAYOUT_ASSERT(sizeof(jb_mix_opts) == 16 && offsetof(jb_mix_opts, ceiling_db) == 8, "jb_mix_opts");
JB_LAYOUT_ASSERT(sizeof(jb_mix_report) == 32 && offsetof(jb_mix_report, scale) == 8 &&
                     offsetof(jb_mix_report, depth) == 16 && offsetof(jb_mix_report, overlap) == 24,
                 "jb_mix_report");
JB_LAYOUT_ASSERT(sizeof(jb_stem_report) == 64 && offsetof(jb_stem_report, e_s) == 16 &&
                     offsetof(jb_stem_report, level_db) == 40,
                 "jb_stem_report");
JB_LAYOUT_ASSERT(sizeof(jb_mix_place) == 16 && offsetof(jb_mix_place, gain_db) == 8, "jb_mix_place");
JB_LAYOUT_ASSERT(sizeof(jb_activity_opts) == 64 && offsetof(jb_activity_opts, gate_db) == 8 &&
                     offsetof(jb_activity_opts, grid) == 16 && offsetof(jb_activity_opts, flags) == 28 &&
                     offsetof(jb_activity_opts, min_speech) == 32 && offsetof(jb_activity_opts, reserved) == 48,
                 "jb_activity_opts");
JB_LAYOUT_ASSERT(sizeof(jb_activity_report) == 40 && offsetof(jb_activity_report, first) == 8 &&
                     offsetof(jb_activity_report, peak) == 24 && offsetof(jb_activity_report, thr) == 32,
                 "jb_activity_report");
JB_LAYOUT_ASSERT(sizeof(jb_activity_unit_report) == 32 && offsetof(jb_activity_unit_report, none) == 8 &&
                     offsetof(jb_activity_unit_report, many) == 24,
                 "jb_activity_unit_report");
JB_LAYOUT_ASSERT(sizeof(jb_pitch_opts) == 112 && offsetof(jb_pitch_opts, min_f0) == 8 &&
                     offsetof(jb_pitch_opts, pov_scale) == 56 && offsetof(jb_pitch_opts, norm_left) == 80 &&
                     offsetof(jb_pitch_opts, grid) == 88 && offsetof(jb_pitch_opts, reserved) == 96,
                 "jb_pitch_opts");
JB_LAYOUT_ASSERT(sizeof(jb_pitch_geometry_t) == 56 && offsetof(jb_pitch_geometry_t, wl) == 16 &&
                     offsetof(jb_pitch_geometry_t, S) == 32 && offsetof(jb_pitch_geometry_t, choice_bytes) == 52,
                 "jb_pitch_geometry_t");
JB_LAYOUT_ASSERT(sizeof(jb_join_opts) == 40 && offsetof(jb_join_opts, fade_ms) == 24 &&
                     offsetof(jb_join_opts, reserved) == 32, "jb_join_opts");
JB_LAYOUT_ASSERT(sizeof(jb_loudness_report) == 40 && offsetof(jb_loudness_report, gain_db) == 24 &&
                     offsetof(jb_loudness_report, peak_mode) == 32 && offsetof(jb_loudness_report, oversampling) == 36,
                 "jb_loudness_report");
JB_LAYOUT_ASSERT(sizeof(jb_loudness_r128) == 48 && offsetof(jb_loudness_r128, lra_lu) == 16 &&
                     offsetof(jb_loudness_r128, n_windows) == 40,
                 "jb_loudness_r128");
JB_LAYOUT_ASSERT(sizeof(jb_loudness_group_report) == 96 && offsetof(jb_loudness_group_report, peak_mode) == 32 &&
                     offsetof(jb_loudness_group_report, members) == 40 && offsetof(jb_loudness_group_report, r128) == 48,
                 "jb_loudness_group_report");
JB_LAYOUT_ASSERT(sizeof(jb_filter_section) == 72 && offsetof(jb_filter_section, f0_hz) == 8 &&
                     offsetof(jb_filter_section, gain_db) == 24 && offsetof(jb_filter_section, b0) == 32,
                 "jb_filter_section");
JB_LAYOUT_ASSERT(sizeof(jb_fir) == 24 && offsetof(jb_fir, n_taps) == 8 && offsetof(jb_fir, hz) == 12 &&
                     offsetof(jb_fir, delay) == 16 && offsetof(jb_fir, reserved) == 20,
                 "jb_fir");
JB_LAYOUT_ASSERT(sizeof(jb_room) == 144 && offsetof(jb_room, source) == 24 && offsetof(jb_room, mic) == 48 &&
                     offsetof(jb_room, beta) == 72 && offsetof(jb_room, c) == 120 && offsetof(jb_room, hz) == 128 &&
                     offsetof(jb_room, n_taps) == 132 && offsetof(jb_room, flags) == 136 &&
                     offsetof(jb_room, reserved) == 140,
                 "jb_room");
JB_LAYOUT_ASSERT(sizeof(jb_room_info) == 40 && offsetof(jb_room_info, pair_visits) == 8 &&
                     offsetof(jb_room_info, entries) == 24 && offsetof(jb_room_info, direct_index) == 36,
                 "jb_room_info");
JB_LAYOUT_ASSERT(sizeof(jb_resample_geometry_t) == 48 && offsetof(jb_resample_geometry_t, pad) == 12 &&
                     offsetof(jb_resample_geometry_t, lds) == 24 && offsetof(jb_resample_geometry_t, identity) == 40,
                 "jb_resample_geometry_t");
JB_LAYOUT_ASSERT(sizeof(jb_room_report) == 24 && offsetof(jb_room_report, drr_db) == 8 &&
                     offsetof(jb_room_report, direct_index) == 16 && offsetof(jb_room_report, delay) == 20,
                 "jb_room_report");
JB_LAYOUT_ASSERT(sizeof(jb_noise) == 64 && offsetof(jb_noise, seed) == 8 && offsetof(jb_noise, snr_db) == 16 &&
                     offsetof(jb_noise, gate_db) == 24 && offsetof(jb_noise, kind) == 32 &&
                     offsetof(jb_noise, bed_len) == 36 && offsetof(jb_noise, hz) == 40 &&
                     offsetof(jb_noise, offset) == 44 && offsetof(jb_noise, reference) == 48 &&
                     offsetof(jb_noise, flags) == 52 && offsetof(jb_noise, reserved) == 56,
                 "jb_noise");
JB_LAYOUT_ASSERT(sizeof(jb_noise_report) == 56 && offsetof(jb_noise_report, gain) == 16 &&
                     offsetof(jb_noise_report, active_samples) == 32 && offsetof(jb_noise_report, seed) == 40 &&
                     offsetof(jb_noise_report, offset) == 48,
                 "jb_noise_report");
JB_LAYOUT_ASSERT(sizeof(jb_filter) == 296 && offsetof(jb_filter, n_sections) == 288, "jb_filter");
JB_LAYOUT_ASSERT(sizeof(jb_biquad) == 40 && offsetof(jb_biquad, a1) == 24, "jb_biquad");
JB_LAYOUT_ASSERT(sizeof(jb_limiter_opts) == 32 && offsetof(jb_limiter_opts, max_reduction_db) == 16 &&
                     offsetof(jb_limiter_opts, flags) == 24, "jb_limiter_opts");
JB_LAYOUT_ASSERT(sizeof(jb_limiter_report) == 24 && offsetof(jb_limiter_report, limited_samples) == 8 &&
                     offsetof(jb_limiter_report, lookahead) == 16 && offsetof(jb_limiter_report, hold) == 20,
                 "jb_limiter_report");
#undef JB_LAYOUT_ASSERT
#endif
#endif /* JBONSAI_AMD_H */

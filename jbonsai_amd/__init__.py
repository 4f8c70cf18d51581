"""jbonsai_amd: MI355X (gfx950) implementation of jbonsai's parameter-generation +
MLSA-vocoder hot path behind a C ABI (include/jbonsai_amd.h).

The HIP shared library `libjbonsai_amd.so` is the product; this package is the
thin host-side mirror of the reference's API used by tests and the benchmark.
"""
from ._ffi import (JbError, LIB_PATH, NODATA, PEAK_SAMPLE, PEAK_TRUE, UttVoc, build, flac_encode, flac_md5, flac_seek_geometry, lib, loudness,  # noqa: F401
                   md5_host,
                   loudness_filter, resample, resample_filter, resample_geometry, ResampleGeometry, true_peak,
                   true_peak_filter, write_wav,
                   format_pcm, format_pcm_host, write_wav_formatted, AdpcmStream, adpcm_decode_host, adpcm_encode,
                   adpcm_encode_host, adpcm_geometry, write_wav_adpcm, loudness_groups, loudness_gate_host,
                   LOUDNESS_NO_GROUP, LOUDNESS_R128, LOUDNESS_PER_UTTERANCE, LOUDNESS_PER_REQUEST,
                   JOIN_NONE, JoinUtt, join_geometry, join_host, join_ms_to_samples, join_pcm,
                   MIX_NONE, MIX_FIT, MixUtt, MixOpts, MixReport, MixPlace, mix_opts, mix_geometry, mix_gain, mix_host,
                   mix_pcm, MIX_NO_STEM, MIX_STEM_LEVELS, StemReport, mix_stems_geometry, mix_stems_host,
                   mix_stems_pcm, mix_levels_host, mix_levels_db,
                   ACTIVITY_SNIP, ACTIVITY_CENTER, ACTIVITY_KALDI, ACTIVITY_STFT, ACTIVITY_REF_PEAK, ACTIVITY_REF_ABS,
                   ACTIVITY_MEMBERS, ACTIVITY_UNIT, ACTIVITY_SAMPLES, ACTIVITY_MAX_CELLS, ActivityOpts, ActivityReport,
                   ActivityUnitReport, activity, activity_geometry, activity_host, activity_members_host, activity_pcm,
                   Filter, FilterSection, Biquad, filter_design, filter_sos, filter_pcm, filter_pcm_host, highpass,
                   lowpass, peaking, lowshelf, highshelf, notch, raw_filter, telephone_band, no_filter,
                   Fir, fir, fir_geometry, fir_host, fir_pcm, FIR_MAX_TAPS, FIR_DIRECT_MAX, FIR_DIRECT, FIR_PARTITIONED,
                   Noise, NoiseReport, noise, noise_host, noise_white, noise_vary, noise_pcm, NOISE_BED, NOISE_WHITE,
                   NOISE_REF_WHOLE, NOISE_REF_ACTIVE, NOISE_VARY, NOISE_MAX_BED,
                   Room, RoomInfo, RoomReport, room, room_host, room_rir, room_geometry, room_lowpass, room_design,
                   room_vary, ROOM_UNIT_DIRECT, ROOM_KEEP_LATENCY, ROOM_VARY, ROOM_WH, ROOM_Q, ROOM_MAX_AXIS,
                   LimiterOpts, LimiterReport, LIMITER_EXACT, LIMITER_OFF, limiter, no_limiter, limiter_window,
                   limiter_host, limiter_pcm,
                   FbankOpts, FBANK_HANN, FBANK_HAMMING, FBANK_CENTER, FBANK_LINEAR, FBANK_UNIT, FBANK_F64, fbank,
                   fbank_geometry, fbank_window, fbank_filterbank, fbank_host, fbank_pcm,
                   MfccOpts, CMVN_NONE, CMVN_MEAN, CMVN_MEAN_VAR, MFCC_F64, mfcc, mfcc_geometry,
                   mfcc_dct, mfcc_delta_kernel, mfcc_host, mfcc_pcm_host, mfcc_frames, mfcc_pcm,
                   FrameOpts, FRAME_WINDOW_OPTS, FRAME_POVEY, FRAME_HANN_SYM, FRAME_RECT, FRAME_BLACKMAN,
                   FRAME_REMOVE_DC, FRAME_REFLECT, FRAME_ENERGY, frame, kaldi_frame, fbank_framed_geometry,
                   frame_window, fbank_framed_host, fbank_framed_pcm, mfcc_framed_pcm_host, mfcc_framed_pcm,
                   MelspecOpts, MEL_HTK, MEL_SLANEY, MEL_NORM_NONE, MEL_NORM_SLANEY, MEL_PAD_REFLECT, MEL_PAD_ZERO,
                   MEL_PAD_NONE, MEL_LOG_NONE, MEL_LOG_LN, MEL_LOG_LOG10, MEL_LOG_DB, MEL_MAGNITUDE, MEL_DROP_LAST,
                   MEL_F64, melspec, whisper_mel, melspec_geometry, melspec_window, melspec_filterbank, melspec_host,
                   melspec_pcm)
from .batch import (Batch, IndexStreamStates, IndexUtterance, PdfSet, StreamInfo, StreamStates, TrackUtterance,  # noqa: F401
                    Utterance, VoiceInfo, generator_from_tracks, mlpg_batch, paramgen_vocode_batch, vocode_tracks_batch,
                    vocoder_synthesize_batch)

from .engine import (Engine, SpeechGenerator, synthesize_batch_each, synthesize_batch_each_flac,  # noqa: F401,E402
                     synthesize_batch_each_adpcm, synthesize_batch_each_formatted, synthesize_batch_each_fbank)
from . import comm  # noqa: F401,E402

__all__ = ["Engine", "SpeechGenerator", "JbError", "LIB_PATH", "NODATA", "build", "lib", "write_wav", "Batch", "StreamInfo", "StreamStates",
           "Utterance", "VoiceInfo", "paramgen_vocode_batch", "mlpg_batch", "vocode_tracks_batch", "vocoder_synthesize_batch", "generator_from_tracks", "TrackUtterance", "PdfSet", "IndexUtterance", "IndexStreamStates",
           "UttVoc", "synthesize_batch_each", "resample", "resample_filter", "resample_geometry", "ResampleGeometry",
           "loudness", "loudness_filter", "flac_encode", "synthesize_batch_each_flac", "flac_md5", "flac_seek_geometry", "md5_host",
           "true_peak", "true_peak_filter", "PEAK_SAMPLE", "PEAK_TRUE",
           "format_pcm", "format_pcm_host", "write_wav_formatted", "synthesize_batch_each_formatted",
           "AdpcmStream", "adpcm_decode_host", "adpcm_encode", "adpcm_encode_host", "adpcm_geometry", "write_wav_adpcm",
           "synthesize_batch_each_adpcm", "loudness_groups", "loudness_gate_host", "LOUDNESS_NO_GROUP", "LOUDNESS_R128", "LOUDNESS_PER_UTTERANCE",
           "LOUDNESS_PER_REQUEST", "JOIN_NONE", "JoinUtt", "join_geometry", "join_host", "join_ms_to_samples",
           "join_pcm", "MIX_NONE", "MIX_FIT", "MixUtt", "MixOpts", "MixReport", "MixPlace", "mix_opts", "mix_geometry",
           "mix_gain", "mix_host", "mix_pcm", "MIX_NO_STEM", "MIX_STEM_LEVELS", "StemReport", "mix_stems_geometry",
           "mix_stems_host", "mix_stems_pcm", "mix_levels_host", "mix_levels_db", "ACTIVITY_SNIP", "ACTIVITY_CENTER",
           "ACTIVITY_KALDI", "ACTIVITY_STFT",
           "ACTIVITY_REF_PEAK", "ACTIVITY_REF_ABS", "ACTIVITY_MEMBERS", "ACTIVITY_UNIT", "ACTIVITY_SAMPLES",
           "ACTIVITY_MAX_CELLS", "ActivityOpts", "ActivityReport", "ActivityUnitReport", "activity", "activity_geometry",
           "activity_host", "activity_members_host", "activity_pcm", "Filter", "FilterSection", "Biquad", "filter_design", "filter_sos", "filter_pcm",
           "filter_pcm_host", "highpass", "lowpass", "peaking", "lowshelf", "highshelf", "notch", "raw_filter",
           "telephone_band", "no_filter", "Fir", "fir", "fir_geometry", "fir_host", "fir_pcm", "FIR_MAX_TAPS",
           "FIR_DIRECT_MAX", "FIR_DIRECT", "FIR_PARTITIONED", "Noise", "NoiseReport", "noise", "noise_host",
           "noise_white", "noise_vary", "noise_pcm", "NOISE_BED", "NOISE_WHITE", "NOISE_REF_WHOLE", "NOISE_REF_ACTIVE",
           "NOISE_VARY", "NOISE_MAX_BED", "Room", "RoomInfo", "RoomReport", "room", "room_host", "room_rir",
           "room_geometry", "room_lowpass", "room_design", "room_vary", "ROOM_UNIT_DIRECT", "ROOM_KEEP_LATENCY",
           "ROOM_VARY", "ROOM_WH", "ROOM_Q", "ROOM_MAX_AXIS", "LimiterOpts", "LimiterReport", "LIMITER_EXACT", "LIMITER_OFF", "limiter",
           "no_limiter", "limiter_window", "limiter_host", "limiter_pcm",
           "FbankOpts", "FBANK_HANN", "FBANK_HAMMING", "FBANK_CENTER", "FBANK_LINEAR", "FBANK_UNIT", "FBANK_F64", "fbank",
           "fbank_geometry", "fbank_window", "fbank_filterbank", "fbank_host", "fbank_pcm",
           "FrameOpts", "FRAME_WINDOW_OPTS", "FRAME_POVEY", "FRAME_HANN_SYM", "FRAME_RECT", "FRAME_BLACKMAN",
           "FRAME_REMOVE_DC", "FRAME_REFLECT", "FRAME_ENERGY", "frame", "kaldi_frame", "fbank_framed_geometry",
           "frame_window", "fbank_framed_host", "fbank_framed_pcm", "mfcc_framed_pcm_host", "mfcc_framed_pcm",
           "synthesize_batch_each_fbank",
           "MfccOpts", "CMVN_NONE", "CMVN_MEAN", "CMVN_MEAN_VAR", "MFCC_F64", "mfcc", "mfcc_geometry",
           "mfcc_dct", "mfcc_delta_kernel", "mfcc_host", "mfcc_pcm_host", "mfcc_frames", "mfcc_pcm",
           "MelspecOpts", "MEL_HTK", "MEL_SLANEY", "MEL_NORM_NONE", "MEL_NORM_SLANEY", "MEL_PAD_REFLECT", "MEL_PAD_ZERO",
           "MEL_PAD_NONE", "MEL_LOG_NONE", "MEL_LOG_LN", "MEL_LOG_LOG10", "MEL_LOG_DB", "MEL_MAGNITUDE", "MEL_DROP_LAST",
           "MEL_F64", "melspec", "whisper_mel", "melspec_geometry", "melspec_window", "melspec_filterbank",
           "melspec_host", "melspec_pcm"]

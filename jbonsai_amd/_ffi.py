"""ctypes binding of libjbonsai_amd.so (include/jbonsai_amd.h).

The shared library is the product; this file only marshals arguments.  It
fails loudly when the HIP library is missing -- there is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
import subprocess
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libjbonsai_amd.so"

MAX_STREAM = 3
MAX_WINDOW = 8
NODATA = -1e10

JB_OK = 0
ERRORS = {
    -1: "JB_ERR_INVALID", -2: "JB_ERR_UNSUPPORTED", -3: "JB_ERR_DEVICE", -4: "JB_ERR_MODEL",
    -5: "JB_ERR_LABEL", -6: "JB_ERR_PARSE_OPTION", -7: "JB_ERR_WEIGHT", -8: "JB_ERR_BUFFER",
}
BATCH_KEEP_TRACKS = 1
BATCH_GENERIC_MLPG = 2
BATCH_SERIAL = 4
BATCH_WAVE_KERNEL = 8
BATCH_LANE_KERNEL = 16
BATCH_SERIAL_GV = 32
BATCH_PCM_I16 = 64
BATCH_MLPG_ONLY = 128
BATCH_TEST_GANG_TIMEOUT = 256
BATCH_NO_EXC_TABLE = 512
BATCH_INVARIANT = 1024
PEAK_SAMPLE = 0
PEAK_TRUE = 1
FMT_F32, FMT_S16, FMT_S24, FMT_ULAW, FMT_ALAW = 1, 2, 3, 4, 5
DITHER_NONE, DITHER_TPDF = 0, 1
FORMATS = {"f32": FMT_F32, "s16": FMT_S16, "s24": FMT_S24, "ulaw": FMT_ULAW, "alaw": FMT_ALAW}
SEARCH_HOST = 0
SEARCH_AUTO = 1
SEARCH_DEVICE = 2


class JbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class StreamDesc(C.Structure):
    _fields_ = [
        ("vector_length", C.c_uint32),
        ("num_windows", C.c_uint32),
        ("is_msd", C.c_uint32),
        ("use_gv", C.c_uint32),
        ("win_width", C.c_uint32 * MAX_WINDOW),
        ("win_coef", C.POINTER(C.c_double)),
    ]


class VoiceDesc(C.Structure):
    _fields_ = [
        ("sampling_frequency", C.c_uint32),
        ("fperiod", C.c_uint32),
        ("nstream", C.c_uint32),
        ("stage", C.c_uint32),
        ("use_log_gain", C.c_uint32),
        ("alpha", C.c_double),
        ("beta", C.c_double),
        ("volume", C.c_double),
        ("stream", StreamDesc * MAX_STREAM),
    ]


class StreamStates(C.Structure):
    _fields_ = [
        ("mean", C.POINTER(C.c_double)),
        ("var", C.POINTER(C.c_double)),
        ("msd", C.POINTER(C.c_double)),
        ("gv_mean", C.POINTER(C.c_double)),
        ("gv_var", C.POINTER(C.c_double)),
        ("gv_switch", C.POINTER(C.c_uint8)),
        ("gv_weight", C.c_double),
        ("msd_threshold", C.c_double),
    ]


class StateUtt(C.Structure):
    _fields_ = [
        ("num_states", C.c_uint32),
        ("durations", C.POINTER(C.c_uint32)),
        ("stream", StreamStates * MAX_STREAM),
    ]


MAX_VOICES = 8


class PdfTable(C.Structure):
    _fields_ = [("rows", C.POINTER(C.c_float)), ("n_rows", C.c_uint32), ("row_len", C.c_uint32)]


class IndexStream(C.Structure):
    _fields_ = [
        ("row", C.POINTER(C.c_uint32) * MAX_VOICES),
        ("weight", C.POINTER(C.c_double)),
        ("gv_mean", C.POINTER(C.c_double)),
        ("gv_var", C.POINTER(C.c_double)),
        ("gv_switch", C.POINTER(C.c_uint8)),
        ("gv_weight", C.c_double),
        ("msd_threshold", C.c_double),
    ]


class IndexUtt(C.Structure):
    _fields_ = [
        ("num_states", C.c_uint32),
        ("durations", C.POINTER(C.c_uint32)),
        ("stream", IndexStream * MAX_STREAM),
        ("lf0_offset", C.c_double),
    ]


class TrackUtt(C.Structure):
    _fields_ = [
        ("n_spectrum", C.c_size_t), ("n_lf0", C.c_size_t), ("n_lpf", C.c_size_t),
        ("spectrum_width", C.c_uint32), ("lf0_width", C.c_uint32), ("lpf_width", C.c_uint32),
        ("reserved", C.c_uint32),
        ("spectrum", C.POINTER(C.c_double)), ("lf0", C.POINTER(C.c_double)), ("lpf", C.POINTER(C.c_double)),
    ]


class UttVoc(C.Structure):
    """jb_utt_voc: one utterance's vocoder condition (volume linear, as VoiceDesc.volume)."""
    _fields_ = [("alpha", C.c_double), ("beta", C.c_double), ("volume", C.c_double)]


class FlacOpts(C.Structure):
    """jb_flac_opts: all zero = the defaults (block size 4096, LPC order up to 8)."""
    _fields_ = [("block_size", C.c_uint32), ("max_lpc_order", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def flac_opts(block_size: int = 0, max_lpc_order=None):
    """FlacOpts for (block_size, max_lpc_order); None / 0 keep the defaults (max_lpc_order=0 with a block size: no
    LPC)."""
    o = FlacOpts()
    o.block_size = int(block_size)
    if max_lpc_order is not None:
        o.max_lpc_order = int(max_lpc_order)
        if not o.block_size and o.max_lpc_order == 0:
            o.block_size = 4096  # "FIXED only" needs a nonzero block size: all zeros are the defaults
    return o


FLAC_MD5 = 1


class FlacMeta(C.Structure):
    """jb_flac_meta: all zero = no MD5 and no SEEKTABLE (the stream of jb_flac_opts alone)."""
    _fields_ = [("flags", C.c_uint32), ("seek_interval_ms", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def flac_meta(md5: bool = False, seek_interval_ms: int = 0):
    """FlacMeta for (md5, seek_interval_ms); None where neither is asked for (the entries without _meta)."""
    if not md5 and not seek_interval_ms:
        return None
    m = FlacMeta()
    m.flags = FLAC_MD5 if md5 else 0
    m.seek_interval_ms = int(seek_interval_ms)
    return m


class FormatOpts(C.Structure):
    """jb_format_opts: the output sample format, its dither and the dither's seed."""
    _fields_ = [("format", C.c_uint32), ("dither", C.c_uint32), ("seed", C.c_uint64)]


def format_opts(fmt, dither=False, seed: int = 0):
    """FormatOpts for a format ("f32", "s16", "s24", "ulaw", "alaw" or a JB_FMT_* value), TPDF dither or none."""
    o = FormatOpts()
    o.format = FORMATS[fmt] if isinstance(fmt, str) else int(fmt)
    o.dither = int(dither)
    o.seed = int(seed) & (2 ** 64 - 1)
    return o


class AdpcmOpts(C.Structure):
    """jb_adpcm_opts: the IMA ADPCM block size (0: by each utterance's output rate)."""
    _fields_ = [("block_align", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def adpcm_opts(block_align: int = 0):
    o = AdpcmOpts()
    o.block_align = int(block_align)
    return o


FBANK_HANN, FBANK_HAMMING = 0, 1
FBANK_CENTER, FBANK_LINEAR, FBANK_UNIT, FBANK_F64 = 1, 2, 4, 8


class FbankOpts(C.Structure):
    """jb_fbank_opts: window and hop in microseconds, n_fft (0: by the window), the mel filters and their band, the
    floor under the logarithm, the window (FBANK_HANN, FBANK_HAMMING) and FBANK_* flags."""
    _fields_ = [("win_us", C.c_uint32), ("hop_us", C.c_uint32), ("n_fft", C.c_uint32), ("n_mels", C.c_uint32),
                ("f_min_hz", C.c_double), ("f_max_hz", C.c_double), ("log_floor", C.c_double),
                ("window", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]

    @property
    def dtype(self):
        import numpy as np

        return np.dtype(np.float64 if self.flags & FBANK_F64 else np.float32)


def fbank(win_ms: float = 25, hop_ms: float = 10, n_mels: int = 80, n_fft: int = 0, f_min: float = 0.0,
          f_max: float = 0.0, log_floor: float = 0.0, window="hann", center: bool = False, linear: bool = False,
          unit: bool = False, f64: bool = False):
    """FbankOpts: log-mel filterbank features of win_ms windows every hop_ms (n_fft 0: the smallest power of two that
    holds the window; f_max 0: half the rate; log_floor 0: 2^-52); window "hann" (periodic) or "hamming" (symmetric);
    center: frame t is centred on sample t * hop, zero-padded; linear: energies, not logarithms; unit: samples in
    +-1.0 instead of the 16-bit scale; f64: float64 elements instead of float32."""
    o = FbankOpts()
    o.win_us, o.hop_us = int(round(win_ms * 1000)), int(round(hop_ms * 1000))
    o.n_fft, o.n_mels = int(n_fft), int(n_mels)
    o.f_min_hz, o.f_max_hz, o.log_floor = float(f_min), float(f_max), float(log_floor)
    o.window = {"hann": FBANK_HANN, "hamming": FBANK_HAMMING}[window] if isinstance(window, str) else int(window)
    o.flags = (FBANK_CENTER * bool(center) | FBANK_LINEAR * bool(linear) | FBANK_UNIT * bool(unit) |
               FBANK_F64 * bool(f64))
    return o


FRAME_WINDOW_OPTS, FRAME_POVEY, FRAME_HANN_SYM, FRAME_RECT, FRAME_BLACKMAN = 0, 1, 2, 3, 4
FRAME_REMOVE_DC, FRAME_REFLECT, FRAME_ENERGY = 1, 2, 4


class FrameOpts(C.Structure):
    """jb_frame_opts: Kaldi-style conditioning of each frame in front of the transform -- the pre-emphasis coefficient,
    the window (FRAME_WINDOW_OPTS: the FbankOpts' own) and FRAME_* flags.  All zero: the identity."""
    _fields_ = [("preemph", C.c_double), ("window", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


def frame(preemph: float = 0.0, window=None, remove_dc: bool = False, reflect: bool = False, energy: bool = False):
    """FrameOpts: per-frame DC removal, pre-emphasis y_i = v_i - preemph * v_{i-1} and the window "povey", "hann_sym",
    "rect" or "blackman" (None: the FbankOpts' own); reflect: Kaldi's snip_edges = false; energy: behind an mfcc
    request, c0 is the frame's log energy."""
    o = FrameOpts()
    o.preemph = float(preemph)
    names = {None: FRAME_WINDOW_OPTS, "povey": FRAME_POVEY, "hann_sym": FRAME_HANN_SYM, "rect": FRAME_RECT,
             "blackman": FRAME_BLACKMAN}
    o.window = names[window] if window is None or isinstance(window, str) else int(window)
    o.flags = FRAME_REMOVE_DC * bool(remove_dc) | FRAME_REFLECT * bool(reflect) | FRAME_ENERGY * bool(energy)
    return o


def kaldi_frame(n_mels: int = 23):
    """jb_frame_kaldi: (FbankOpts, FrameOpts) of compute-fbank-feats' defaults with n_mels filters."""
    f, fr = FbankOpts(), FrameOpts()
    check(lib().jb_frame_kaldi(int(n_mels), C.byref(f), C.byref(fr)))
    return f, fr


CMVN_NONE, CMVN_MEAN, CMVN_MEAN_VAR = 0, 1, 2
MFCC_F64 = 1


class MfccOpts(C.Structure):
    """jb_mfcc_opts: the cepstra kept (0: the log-mel energies themselves), the delta order and window, the CMVN mode
    (CMVN_*), the lifter, the floor under the variance and MFCC_* flags."""
    _fields_ = [("n_ceps", C.c_uint32), ("delta_order", C.c_uint32), ("delta_window", C.c_uint32),
                ("cmvn", C.c_uint32), ("lifter", C.c_double), ("var_floor", C.c_double), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]

    @property
    def dtype(self):
        import numpy as np

        return np.dtype(np.float64 if self.flags & MFCC_F64 else np.float32)

    def width(self, n_mels: int) -> int:
        """Elements of a row behind a filterbank of n_mels filters."""
        return (self.n_ceps or n_mels) * (self.delta_order + 1)


def mfcc(n_ceps: int = 13, lifter: float = 22, delta_order: int = 0, delta_window: int = 2, cmvn="none",
         var_floor: float = 0, f64: bool = False):
    """MfccOpts: n_ceps liftered cepstra of the log-mel energies (0: the energies themselves; lifter 0: none), with
    delta rows up to delta_order over windows of +-delta_window frames, normalised per unit: cmvn "none", "mean" or
    "mean_var" (var_floor 0: 2^-52); f64: float64 elements instead of float32."""
    o = MfccOpts()
    o.n_ceps, o.delta_order, o.delta_window = int(n_ceps), int(delta_order), int(delta_window)
    o.cmvn = ({"none": CMVN_NONE, "mean": CMVN_MEAN, "mean_var": CMVN_MEAN_VAR}[cmvn] if isinstance(cmvn, str)
              else int(cmvn))
    o.lifter, o.var_floor = float(lifter), float(var_floor)
    o.flags = MFCC_F64 * bool(f64)
    return o


MEL_HTK, MEL_SLANEY = 0, 1
MEL_NORM_NONE, MEL_NORM_SLANEY = 0, 1
MEL_PAD_REFLECT, MEL_PAD_ZERO, MEL_PAD_NONE = 0, 1, 2
MEL_LOG_NONE, MEL_LOG_LN, MEL_LOG_LOG10, MEL_LOG_DB = 0, 1, 2, 3
MEL_MAGNITUDE, MEL_DROP_LAST, MEL_F64 = 1, 2, 4


class MelspecOpts(C.Structure):
    """jb_melspec_opts: transform, window and hop in samples, the mel filters, their band, scale (MEL_HTK, MEL_SLANEY)
    and normalisation (MEL_NORM_*), the padding (MEL_PAD_*), the logarithm (MEL_LOG_*) with its floor, the range clamp
    under the unit's maximum, the affine step and MEL_* flags."""
    _fields_ = [("n_fft", C.c_uint32), ("win_length", C.c_uint32), ("hop_length", C.c_uint32), ("n_mels", C.c_uint32),
                ("f_min_hz", C.c_double), ("f_max_hz", C.c_double), ("floor", C.c_double), ("range", C.c_double),
                ("offset", C.c_double), ("scale", C.c_double), ("mel_scale", C.c_uint32), ("norm", C.c_uint32),
                ("pad", C.c_uint32), ("log", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    @property
    def dtype(self):
        import numpy as np

        return np.dtype(np.float64 if self.flags & MEL_F64 else np.float32)


def _choice(value, names):
    return names[value] if isinstance(value, str) else int(value)


def melspec_next_fft(win: int) -> int:
    """The smallest transform length the stage takes that holds a window of `win` samples: even, at least 64, no prime
    factor above 5."""
    n = max(64, win + (win & 1))
    while True:
        r = n
        for p in (2, 3, 5):
            while r % p == 0:
                r //= p
        if r == 1:
            return n
        n += 2


def melspec(n_fft: int = 0, hop: int = 0, win: int = 0, n_mels: int = 80, f_min: float = 0.0, f_max: float = 0.0,
            mel_scale="slaney", norm="slaney", pad="reflect", log="ln", floor: float = 0.0, range: float = 0.0,
            offset: float = 0.0, scale: float = 0.0, magnitude: bool = False, drop_last: bool = False,
            f64: bool = False, win_ms: float = 0.0, hop_ms: float = 0.0, rate: int = 0):
    """MelspecOpts: mel spectrograms in the librosa / Whisper convention: an n_fft-point transform (even, 64..4096, no
    prime factor above 5) every `hop` samples under a periodic Hann window of `win` samples (0: n_fft); win_ms / hop_ms
    with `rate` give win and hop in samples instead (n_fft 0 then: the smallest length the stage takes that holds win).  mel_scale "htk" or "slaney"; norm "none" or
    "slaney"; pad "reflect", "zero" or "none"; log "none", "ln", "log10" or "db" above `floor` (0: 1e-10); range > 0
    clamps at the unit's maximum minus range; then (y + offset) * scale (scale 0: 1.0).  magnitude: |X| instead of
    |X|^2; drop_last: without the last frame; f64: float64 elements instead of float32."""
    if win_ms or hop_ms:
        if not rate:
            raise ValueError("win_ms / hop_ms need the rate")
        win = int(win_ms * rate / 1000.0 + 0.5) if win_ms else win  # (half a sample rounds up, as the fbank stage's)
        hop = int(hop_ms * rate / 1000.0 + 0.5) if hop_ms else hop
    o = MelspecOpts()
    n_fft = n_fft or (melspec_next_fft(int(win)) if win_ms else win)
    o.n_fft, o.win_length, o.hop_length, o.n_mels = int(n_fft), int(win), int(hop), int(n_mels)
    o.f_min_hz, o.f_max_hz = float(f_min), float(f_max)
    o.floor, o.range, o.offset, o.scale = float(floor), float(range), float(offset), float(scale)
    o.mel_scale = _choice(mel_scale, {"htk": MEL_HTK, "slaney": MEL_SLANEY})
    o.norm = _choice("none" if norm is None else norm, {"none": MEL_NORM_NONE, "slaney": MEL_NORM_SLANEY})
    o.pad = _choice(pad, {"reflect": MEL_PAD_REFLECT, "zero": MEL_PAD_ZERO, "none": MEL_PAD_NONE})
    o.log = _choice("none" if log is None else log,
                    {"none": MEL_LOG_NONE, "ln": MEL_LOG_LN, "log10": MEL_LOG_LOG10, "db": MEL_LOG_DB})
    o.flags = MEL_MAGNITUDE * bool(magnitude) | MEL_DROP_LAST * bool(drop_last) | MEL_F64 * bool(f64)
    return o


def whisper_mel(n_mels: int = 80, f64: bool = False):
    """jb_melspec_whisper: Whisper's front end (400 / 400 / 160 at 16 kHz, reflect padding without the last frame, Slaney
    filters, log10 clamped 8 under the maximum, (y + 4) / 4); the caller sets the output rate to 16 kHz."""
    o = MelspecOpts()
    check(lib().jb_melspec_whisper(n_mels, C.byref(o)))
    o.flags |= MEL_F64 * bool(f64)
    return o


JOIN_NONE = 0xFFFFFFFF


class JoinUtt(C.Structure):
    """jb_join_utt: an utterance's programme, its edge fades and its pads of zero samples."""
    _fields_ = [("programme", C.c_uint32), ("fade_in", C.c_uint32), ("fade_out", C.c_uint32), ("reserved", C.c_uint32),
                ("pad_before", C.c_uint64), ("pad_after", C.c_uint64)]


class JoinOpts(C.Structure):
    """jb_join_opts: lead, gap, trail and fade of a jb_synthesize_programme* call, in milliseconds."""
    _fields_ = [("lead_ms", C.c_double), ("gap_ms", C.c_double), ("trail_ms", C.c_double), ("fade_ms", C.c_double),
                ("reserved", C.c_uint32 * 2)]


def join_opts(lead_ms: float = 0.0, gap_ms: float = 0.0, trail_ms: float = 0.0, fade_ms: float = 0.0):
    o = JoinOpts()
    o.lead_ms, o.gap_ms, o.trail_ms, o.fade_ms = float(lead_ms), float(gap_ms), float(trail_ms), float(fade_ms)
    return o


def join_request(req):
    """A (JoinUtt * n) array of `req`: JoinUtt entries, or tuples / dicts of (programme, pad_before, pad_after,
    fade_in, fade_out) with programme None for an utterance of its own and the rest 0 by default."""
    arr = (JoinUtt * max(1, len(req)))()
    for i, r in enumerate(req):
        if isinstance(r, JoinUtt):
            arr[i] = r
            continue
        if isinstance(r, dict):
            r = (r.get("programme"), r.get("pad_before", 0), r.get("pad_after", 0), r.get("fade_in", 0),
                 r.get("fade_out", 0))
        r = tuple(r) + (0,) * (5 - len(r))
        arr[i].programme = JOIN_NONE if r[0] is None else int(r[0])
        arr[i].pad_before, arr[i].pad_after, arr[i].fade_in, arr[i].fade_out = (int(v) for v in r[1:5])
    return arr


MIX_NONE = 0xFFFFFFFF
MIX_FIT = 1


class MixUtt(C.Structure):
    """jb_mix_utt: an utterance's programme, its start within it, its pad behind, its edge fades and its gain."""
    _fields_ = [("programme", C.c_uint32), ("fade_in", C.c_uint32), ("fade_out", C.c_uint32), ("reserved", C.c_uint32),
                ("start", C.c_uint64), ("pad_after", C.c_uint64), ("gain_db", C.c_double), ("reserved2", C.c_uint64)]


class MixOpts(C.Structure):
    """jb_mix_opts: MIX_FIT and its ceiling in dBFS."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("ceiling_db", C.c_double)]


class MixReport(C.Structure):
    """jb_mix_report: a programme's peak, its scale, its depth and its samples under two or more members."""
    _fields_ = [("peak", C.c_double), ("scale", C.c_double), ("depth", C.c_uint32), ("reserved", C.c_uint32),
                ("overlap", C.c_uint64)]


MIX_NO_STEM = 0xFFFFFFFF
MIX_STEM_LEVELS = 1


class StemReport(C.Structure):
    """jb_stem_report: a stem's peak, its programme's scale and, with levels, the three sums and the dB values."""
    _fields_ = [("peak", C.c_double), ("scale", C.c_double), ("e_s", C.c_double), ("d", C.c_double),
                ("e_p", C.c_double), ("level_db", C.c_double), ("sir_db", C.c_double), ("si_sdr_db", C.c_double)]


def stem_ids(stem_of):
    """A (uint32 * n) array of stem ids; None: MIX_NO_STEM."""
    return (C.c_uint32 * max(1, len(stem_of)))(*[MIX_NO_STEM if s is None else int(s) for s in stem_of])


class MixPlace(C.Structure):
    """jb_mix_place: a member's start behind the lead in milliseconds, and its gain."""
    _fields_ = [("start_ms", C.c_double), ("gain_db", C.c_double)]


def mix_opts(fit: bool = False, ceiling_db: float = 0.0):
    o = MixOpts()
    o.flags, o.ceiling_db = MIX_FIT * bool(fit), float(ceiling_db)
    return o


def mix_request(req):
    """A (MixUtt * n) array of `req`: MixUtt entries, or tuples / dicts of (programme, start, gain_db, pad_after,
    fade_in, fade_out) with programme None for an utterance of its own and the rest 0 by default."""
    arr = (MixUtt * max(1, len(req)))()
    for i, r in enumerate(req):
        if isinstance(r, MixUtt):
            arr[i] = r
            continue
        if isinstance(r, dict):
            r = (r.get("programme"), r.get("start", 0), r.get("gain_db", 0.0), r.get("pad_after", 0),
                 r.get("fade_in", 0), r.get("fade_out", 0))
        r = tuple(r) + (0,) * (6 - len(r))
        arr[i].programme = MIX_NONE if r[0] is None else int(r[0])
        arr[i].start, arr[i].gain_db, arr[i].pad_after = int(r[1]), float(r[2]), int(r[3])
        arr[i].fade_in, arr[i].fade_out = int(r[4]), int(r[5])
    return arr


ACTIVITY_SNIP, ACTIVITY_CENTER, ACTIVITY_KALDI, ACTIVITY_STFT = range(4)
ACTIVITY_REF_PEAK, ACTIVITY_REF_ABS = 0, 1
ACTIVITY_MEMBERS, ACTIVITY_UNIT = 0, 1
ACTIVITY_SAMPLES = 1
ACTIVITY_MAX_CELLS = 1 << 30
_ACTIVITY_GRIDS = {"snip": ACTIVITY_SNIP, "center": ACTIVITY_CENTER, "kaldi": ACTIVITY_KALDI, "stft": ACTIVITY_STFT}
_ACTIVITY_REFS = {"peak": ACTIVITY_REF_PEAK, "abs": ACTIVITY_REF_ABS}
_ACTIVITY_COLUMNS = {"members": ACTIVITY_MEMBERS, "unit": ACTIVITY_UNIT}


class ActivityOpts(C.Structure):
    """jb_activity_opts: the frame grid, the gate and the smoothing lengths of a speech-activity request."""
    _fields_ = [("win_us", C.c_uint32), ("hop_us", C.c_uint32), ("gate_db", C.c_double), ("grid", C.c_uint32),
                ("reference", C.c_uint32), ("columns", C.c_uint32), ("flags", C.c_uint32), ("min_speech", C.c_uint32),
                ("min_gap", C.c_uint32), ("hang_before", C.c_uint32), ("hang_after", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class ActivityReport(C.Structure):
    """jb_activity_report: a column's active frames, its first and last one (T: none), its largest energy, its thr."""
    _fields_ = [("active", C.c_uint64), ("first", C.c_uint64), ("last", C.c_uint64), ("peak", C.c_double),
                ("thr", C.c_double)]


class ActivityUnitReport(C.Structure):
    """jb_activity_unit_report: T and the frames under 0, exactly 1, and 2 or more active columns."""
    _fields_ = [("frames", C.c_uint64), ("none", C.c_uint64), ("one", C.c_uint64), ("many", C.c_uint64)]


def activity(win_ms=25, hop_ms=10, gate_db=40, grid="snip", reference="peak", columns="members", min_speech=0, min_gap=0,
             hang_before=0, hang_after=0, samples=False):
    """An ActivityOpts: window and hop in milliseconds (samples=True: in samples, as melspec takes them), the gate in dB
    under the column's largest frame energy (reference="peak") or under full scale (reference="abs"), the grid by name
    ("snip", "center", "kaldi", "stft") or constant, and the smoothing lengths in frames."""
    o = ActivityOpts()
    if samples:
        o.win_us, o.hop_us, o.flags = int(win_ms), int(hop_ms), ACTIVITY_SAMPLES
    else:
        o.win_us, o.hop_us = int(round(win_ms * 1000)), int(round(hop_ms * 1000))
    o.gate_db = float(gate_db)
    o.grid = _ACTIVITY_GRIDS.get(grid, grid)
    o.reference = _ACTIVITY_REFS.get(reference, reference)
    o.columns = _ACTIVITY_COLUMNS.get(columns, columns)
    o.min_speech, o.min_gap, o.hang_before, o.hang_after = int(min_speech), int(min_gap), int(hang_before), int(hang_after)
    return o


PITCH_SNIP, PITCH_KALDI = 0, 1
PITCH_F64, PITCH_RAW, PITCH_RAW_LOG = 1, 2, 4
PITCH_RATE = 4000
PITCH_MAX_DOWN = 4096
PITCH_MAX_SCRATCH = 1 << 32
_PITCH_GRIDS = {"snip": PITCH_SNIP, "kaldi": PITCH_KALDI}


class PitchOpts(C.Structure):
    """jb_pitch_opts: the frame grid, the lag grid, the tracker's costs and the post-processing of a pitch request."""
    _fields_ = [("win_us", C.c_uint32), ("hop_us", C.c_uint32), ("min_f0", C.c_double), ("max_f0", C.c_double),
                ("delta_pitch", C.c_double), ("penalty_factor", C.c_double), ("soft_min_f0", C.c_double),
                ("nccf_ballast", C.c_double), ("pov_scale", C.c_double), ("pitch_scale", C.c_double),
                ("delta_scale", C.c_double), ("norm_left", C.c_uint32), ("norm_right", C.c_uint32),
                ("grid", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class PitchGeometry(C.Structure):
    """jb_pitch_geometry_t: T and n4, the window and hop at the unit's rate and at 4 kHz, the lag grid's size and the
    integer lags' range, a row's columns and element bytes, and the tracker's scratch bytes per frame."""
    _fields_ = [("T", C.c_uint64), ("n4", C.c_uint64), ("wl", C.c_uint32), ("hop", C.c_uint32), ("wl4", C.c_uint32),
                ("sh4", C.c_uint32), ("S", C.c_uint32), ("lag_first", C.c_uint32), ("lag_last", C.c_uint32),
                ("width", C.c_uint32), ("elem", C.c_uint32), ("choice_bytes", C.c_uint32)]


def kaldi_pitch():
    """jb_pitch_kaldi: a PitchOpts with Kaldi's defaults (25 / 10 ms, 50..400 Hz, the Kaldi grid, f32, 3 columns)."""
    o = PitchOpts()
    check(lib().jb_pitch_kaldi(C.byref(o)))
    return o


def pitch(win_ms=25, hop_ms=10, grid="kaldi", raw=False, raw_log=False, f64=False, **fields):
    """A PitchOpts: Kaldi's defaults with the window and hop in milliseconds, the grid by name ("snip", "kaldi") or
    constant, raw=True for the tracker's two columns (p, Hz), raw_log=True for the fourth column, f64=True for float64
    elements, and any other field of jb_pitch_opts by name (min_f0, max_f0, delta_pitch, ...)."""
    o = kaldi_pitch()
    o.win_us, o.hop_us = int(round(win_ms * 1000)), int(round(hop_ms * 1000))
    o.grid = _PITCH_GRIDS.get(grid, grid)
    o.flags = PITCH_F64 * bool(f64) | PITCH_RAW * bool(raw) | PITCH_RAW_LOG * bool(raw_log)
    names = {f[0] for f in PitchOpts._fields_} - {"reserved"}
    for k, v in fields.items():
        if k not in names:
            raise TypeError(f"jb_pitch_opts has no field {k!r}")
        setattr(o, k, v)
    return o


FILTER_MAX_SECTIONS = 4
FILTER_HIGHPASS, FILTER_LOWPASS, FILTER_PEAKING, FILTER_LOWSHELF, FILTER_HIGHSHELF, FILTER_NOTCH, FILTER_RAW = range(1, 8)


class FilterSection(C.Structure):
    """jb_filter_section: a kind with f0_hz, q and gain_db, or FILTER_RAW with b0 b1 b2 a1 a2 (a0 = 1)."""
    _fields_ = [("kind", C.c_uint32), ("reserved", C.c_uint32), ("f0_hz", C.c_double), ("q", C.c_double),
                ("gain_db", C.c_double), ("b0", C.c_double), ("b1", C.c_double), ("b2", C.c_double),
                ("a1", C.c_double), ("a2", C.c_double)]


class Filter(C.Structure):
    """jb_filter: up to four sections applied in order.  `a + b` is the cascade of a's sections, then b's."""
    _fields_ = [("section", FilterSection * FILTER_MAX_SECTIONS), ("n_sections", C.c_uint32), ("reserved", C.c_uint32)]

    def __add__(self, other):
        out = Filter()
        # (a cascade of more than four sections keeps its count: the library refuses it, naming n_sections)
        out.n_sections = self.n_sections + other.n_sections
        secs = [self.section[i] for i in range(min(self.n_sections, FILTER_MAX_SECTIONS))] + \
            [other.section[i] for i in range(min(other.n_sections, FILTER_MAX_SECTIONS))]
        for i, sec in enumerate(secs[:FILTER_MAX_SECTIONS]):
            C.memmove(C.byref(out.section[i]), C.byref(sec), C.sizeof(FilterSection))
        return out


class Biquad(C.Structure):
    """jb_biquad: one designed section."""
    _fields_ = [("b0", C.c_double), ("b1", C.c_double), ("b2", C.c_double), ("a1", C.c_double), ("a2", C.c_double)]


def filter_section(kind: int, f0: float, q: float = 0.7071067811865476, gain_db: float = 0.0):
    """A Filter of one designed section."""
    f = Filter()
    f.n_sections = 1
    f.section[0].kind, f.section[0].f0_hz, f.section[0].q, f.section[0].gain_db = int(kind), float(f0), float(q), \
        float(gain_db)
    return f


def no_filter():
    return Filter()


def highpass(f0, q=0.7071067811865476): return filter_section(FILTER_HIGHPASS, f0, q)
def lowpass(f0, q=0.7071067811865476): return filter_section(FILTER_LOWPASS, f0, q)
def peaking(f0, gain_db, q=0.7071067811865476): return filter_section(FILTER_PEAKING, f0, q, gain_db)
def lowshelf(f0, gain_db, q=0.7071067811865476): return filter_section(FILTER_LOWSHELF, f0, q, gain_db)
def highshelf(f0, gain_db, q=0.7071067811865476): return filter_section(FILTER_HIGHSHELF, f0, q, gain_db)
def notch(f0, q=0.7071067811865476): return filter_section(FILTER_NOTCH, f0, q)


def telephone_band():
    """The G.712 voice band in front of G.711: high-pass 300 Hz, low-pass 3400 Hz."""
    return highpass(300.0) + lowpass(3400.0)


def raw_filter(sos):
    """A Filter of FILTER_RAW sections from rows of b0 b1 b2 a1 a2, or of scipy's b0 b1 b2 1 a1 a2."""
    f = Filter()
    rows = [list(map(float, r)) for r in sos]
    f.n_sections = len(rows)
    for i, r in enumerate(rows[:FILTER_MAX_SECTIONS]):
        if len(r) == 6:
            if r[3] != 1.0:
                raise ValueError("raw_filter: a0 must be 1")
            r = r[:3] + r[4:]
        sec = f.section[i]
        sec.kind = FILTER_RAW
        sec.b0, sec.b1, sec.b2, sec.a1, sec.a2 = r
    return f


FIR_MAX_TAPS, FIR_DIRECT_MAX, FIR_DIRECT, FIR_PARTITIONED = 131072, 256, 0, 1


class Fir(C.Structure):
    """jb_fir: an impulse response of n_taps f64 taps sampled at hz, and the delay d < n_taps its output is advanced by.
    The object keeps its taps alive (`_taps`); the library copies them at every call that takes one."""
    _fields_ = [("taps", C.POINTER(C.c_double)), ("n_taps", C.c_uint32), ("hz", C.c_uint32), ("delay", C.c_uint32),
                ("reserved", C.c_uint32)]


def fir(taps, hz: int, delay: int = 0):
    """A Fir of `taps` (any sequence of floats; None: no response) at `hz`, advanced by `delay` samples."""
    import numpy as np
    f = Fir()
    f.hz, f.delay = int(hz), int(delay)
    if taps is not None:
        f._taps = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
        f.taps = f._taps.ctypes.data_as(C.POINTER(C.c_double))
        f.n_taps = f._taps.size
    return f


def fir_array(firs, n=None):
    """A (Fir * n) array of Fir entries (None: no response); one entry stands for all n.  The array keeps the entries
    (and so their taps) alive."""
    fs = [firs] if isinstance(firs, Fir) or firs is None else list(firs)
    if n is not None and len(fs) == 1:
        fs = fs * n
    arr = (Fir * max(1, len(fs)))()
    for i, f in enumerate(fs):
        if f is not None:
            C.memmove(C.byref(arr[i]), C.byref(f), C.sizeof(Fir))
    arr._keep = fs
    return arr, len(fs)


ROOM_UNIT_DIRECT, ROOM_KEEP_LATENCY, ROOM_VARY, ROOM_WH, ROOM_Q, ROOM_MAX_AXIS = 1, 2, 1, 32, 128, 1024


class Room(C.Structure):
    """jb_room: a shoebox room -- edges, source and microphone in metres, the six walls' reflection coefficients (x = 0,
    x = Lx, y = 0, y = Ly, z = 0, z = Lz), the speed of sound (0: 343 m/s), the rate and the number of taps."""
    _fields_ = [("size", C.c_double * 3), ("source", C.c_double * 3), ("mic", C.c_double * 3),
                ("beta", C.c_double * 6), ("c", C.c_double), ("hz", C.c_uint32), ("n_taps", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class RoomInfo(C.Structure):
    """jb_room_info: the direct distance and index, entries per axis, pair visits and workgroups of a room."""
    _fields_ = [("direct_distance", C.c_double), ("pair_visits", C.c_uint64), ("workgroups", C.c_uint64),
                ("entries", C.c_uint32 * 3), ("direct_index", C.c_uint32)]


class ResampleGeometry(C.Structure):
    """jb_resample_geometry_t: the path k_resample takes for a pair -- L, M, ntaps, the pad shift, the LDS cap and the
    rows that fit it, whether the window is staged in LDS, rows per tile, waves per row block, LDS bytes, identity."""
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("ntaps", C.c_uint32), ("pad", C.c_uint32), ("cap", C.c_uint32),
                ("fit", C.c_uint32), ("lds", C.c_uint32), ("rows", C.c_uint32), ("row_waves", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("identity", C.c_uint32), ("reserved", C.c_uint32)]


class RoomReport(C.Structure):
    """jb_room_report: the taps' energy, the direct-to-reverberant ratio in dB, the direct index and the delay used."""
    _fields_ = [("energy", C.c_double), ("drr_db", C.c_double), ("direct_index", C.c_uint32), ("delay", C.c_uint32)]


def room(size, source, mic, beta=None, rt60=None, hz: int = 0, n_taps: int = 0, c: float = 343.0,
         unit_direct: bool = True, keep_latency: bool = False):
    """A Room of edges `size` with `source` and `mic` inside (metres).  Give exactly one of `beta` (one coefficient
    for all six walls, or six) and `rt60` (seconds: Eyring's formula, room_design)."""
    if (beta is None) == (rt60 is None):
        raise ValueError("room: give exactly one of beta and rt60")
    r = Room()
    r.size[:], r.source[:], r.mic[:] = [float(v) for v in size], [float(v) for v in source], [float(v) for v in mic]
    if rt60 is not None:
        r.beta[:] = room_design(size, rt60, c)
    else:
        try:
            r.beta[:] = [float(v) for v in beta]
        except TypeError:
            r.beta[:] = [float(beta)] * 6
    r.c, r.hz, r.n_taps = float(c), int(hz), int(n_taps)
    r.flags = (ROOM_UNIT_DIRECT if unit_direct else 0) | (ROOM_KEEP_LATENCY if keep_latency else 0)
    return r


def room_array(rooms, n=None):
    """A (Room * n) array of Room entries (None: no room, all bytes zero); one entry stands for all n."""
    rs = [rooms] if isinstance(rooms, Room) or rooms is None else list(rooms)
    if n is not None and len(rs) == 1:
        rs = rs * n
    arr = (Room * max(1, len(rs)))()
    for i, r in enumerate(rs):
        if r is not None:
            C.memmove(C.byref(arr[i]), C.byref(r), C.sizeof(Room))
    return arr, len(rs)


NOISE_BED, NOISE_WHITE, NOISE_REF_WHOLE, NOISE_REF_ACTIVE, NOISE_VARY, NOISE_MAX_BED = 0, 1, 0, 1, 1, 1 << 24


class Noise(C.Structure):
    """jb_noise: a noise request -- a bed of bed_len f64 samples at hz that is looped from `offset`, or white noise of
    `seed`, at snr_db against the whole utterance's power or its active tiles' (gate_db below the mean).  The object
    keeps its bed alive (`_bed`); the library copies it at every call that takes one."""
    _fields_ = [("bed", C.POINTER(C.c_double)), ("seed", C.c_uint64), ("snr_db", C.c_double), ("gate_db", C.c_double),
                ("kind", C.c_uint32), ("bed_len", C.c_uint32), ("hz", C.c_uint32), ("offset", C.c_uint32),
                ("reference", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class NoiseReport(C.Structure):
    """jb_noise_report: speech_power = A / C, noise_power = Bs / N, the gain, and the snr_db, seed and offset used."""
    _fields_ = [("speech_power", C.c_double), ("noise_power", C.c_double), ("gain", C.c_double),
                ("snr_db", C.c_double), ("active_samples", C.c_uint64), ("seed", C.c_uint64),
                ("offset", C.c_uint32), ("reserved", C.c_uint32)]


def noise(bed=None, hz: int = 0, snr_db: float = 20.0, offset: int = 0, seed: int = 0, reference: str = "whole",
          gate_db: float = 20.0, vary: bool = False):
    """A Noise: `bed` (any sequence of floats at `hz`, 16-bit units) looped from `offset`, or white noise of `seed`
    where bed is None, at `snr_db`; reference "whole" or "active" (tiles within gate_db of the mean power); vary: every
    utterance of a batch or call gets a seed and an offset of its own (noise_vary)."""
    import numpy as np
    if reference not in ("whole", "active"):
        raise ValueError('noise: reference is "whole" or "active"')
    r = Noise()
    r.hz, r.snr_db, r.seed, r.offset = int(hz), float(snr_db), int(seed) & (2**64 - 1), int(offset)
    r.reference = NOISE_REF_ACTIVE if reference == "active" else NOISE_REF_WHOLE
    r.gate_db = float(gate_db) if reference == "active" else 0.0
    r.flags = NOISE_VARY if vary else 0
    if bed is None:
        r.kind = NOISE_WHITE
    else:
        r.kind = NOISE_BED
        r._bed = np.ascontiguousarray(bed, dtype=np.float64).reshape(-1)
        r.bed = r._bed.ctypes.data_as(C.POINTER(C.c_double))
        r.bed_len = r._bed.size
    return r


def noise_array(reqs, n=None):
    """A (Noise * n) array of Noise entries (None: no request); one entry stands for all n.  The array keeps the
    entries (and so their beds) alive."""
    rs = [reqs] if isinstance(reqs, Noise) or reqs is None else list(reqs)
    if n is not None and len(rs) == 1:
        rs = rs * n
    arr = (Noise * max(1, len(rs)))()
    for i, r in enumerate(rs):
        if r is not None:
            C.memmove(C.byref(arr[i]), C.byref(r), C.sizeof(Noise))
    arr._keep = rs
    return arr, len(rs)


def filter_array(filters, n=None):
    """A (Filter * n) array of Filter entries (None: no sections); one entry stands for all n."""
    fs = [filters] if isinstance(filters, Filter) or filters is None else list(filters)
    if n is not None and len(fs) == 1:
        fs = fs * n
    arr = (Filter * max(1, len(fs)))()
    for i, f in enumerate(fs):
        if f is not None:
            C.memmove(C.byref(arr[i]), C.byref(f), C.sizeof(Filter))
    return arr, len(fs)


LIMITER_EXACT, LIMITER_OFF = 1, 2


class LimiterOpts(C.Structure):
    """jb_limiter_opts: look-ahead and hold in ms, how far the static gain may put the highest peak over the ceiling."""
    _fields_ = [("lookahead_ms", C.c_double), ("hold_ms", C.c_double), ("max_reduction_db", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class LimiterReport(C.Structure):
    """jb_limiter_report: what the limiter did to one utterance."""
    _fields_ = [("max_reduction_db", C.c_double), ("limited_samples", C.c_uint64), ("lookahead", C.c_uint32),
                ("hold", C.c_uint32)]

    def as_dict(self):
        return {"max_reduction_db": self.max_reduction_db, "limited_samples": int(self.limited_samples),
                "lookahead": int(self.lookahead), "hold": int(self.hold)}


def limiter(lookahead_ms: float = 2.0, hold_ms: float = 8.0, max_reduction_db: float = 6.0):
    """A LimiterOpts with the three values as given (LIMITER_EXACT: a hold or a reduction of 0 means 0)."""
    return LimiterOpts(float(lookahead_ms), float(hold_ms), float(max_reduction_db), LIMITER_EXACT, 0)


def no_limiter():
    """The LimiterOpts of an utterance that is not limited (LIMITER_OFF)."""
    return LimiterOpts(0.0, 0.0, 0.0, LIMITER_OFF, 0)


def limiter_array(opts, n=None):
    """A (LimiterOpts * n) array (None: no_limiter()); one entry stands for all n."""
    os_ = [opts] if isinstance(opts, LimiterOpts) or opts is None else list(opts)
    if n is not None and len(os_) == 1:
        os_ = os_ * n
    arr = (LimiterOpts * max(1, len(os_)))()
    for i, o in enumerate(os_):
        C.memmove(C.byref(arr[i]), C.byref(o if o is not None else no_limiter()), C.sizeof(LimiterOpts))
    return arr, len(os_)


class LoudnessReport(C.Structure):
    """jb_loudness_report: what a run measured and applied for one utterance."""
    _fields_ = [("lufs", C.c_double), ("sample_peak_dbfs", C.c_double), ("true_peak_dbtp", C.c_double),
                ("gain_db", C.c_double), ("peak_mode", C.c_uint32), ("oversampling", C.c_uint32)]


class LoudnessR128(C.Structure):
    """jb_loudness_r128: largest momentary and short-term loudness and the loudness range of an utterance or a group."""
    _fields_ = [("max_momentary_lufs", C.c_double), ("max_short_term_lufs", C.c_double), ("lra_lu", C.c_double),
                ("lra_low_lufs", C.c_double), ("lra_high_lufs", C.c_double), ("n_windows", C.c_uint64)]


class LoudnessGroupReport(C.Structure):
    """jb_loudness_group_report: what a run measured and applied for one loudness group."""
    _fields_ = [("lufs", C.c_double), ("sample_peak_dbfs", C.c_double), ("true_peak_dbtp", C.c_double),
                ("gain_db", C.c_double), ("peak_mode", C.c_uint32), ("oversampling", C.c_uint32),
                ("members", C.c_uint32), ("flags", C.c_uint32), ("r128", LoudnessR128)]


LOUDNESS_PER_UTTERANCE, LOUDNESS_PER_REQUEST = 0, 1
LOUDNESS_NO_GROUP = 0xFFFFFFFF
LOUDNESS_R128 = 1


def _struct_dict(r):
    return {k: (_struct_dict(getattr(r, k)) if isinstance(getattr(r, k), C.Structure) else getattr(r, k))
            for k, _ in r._fields_}


class BatchOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32), ("chunk_frames", C.c_uint32),
                ("warmup_frames", C.c_uint32), ("verify_tol", C.c_double), ("reserved0", C.c_uint32), ("reserved", C.c_uint32)]


# every symbol include/jbonsai_amd.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "jb_batch_create", "jb_batch_run", "jb_batch_sync", "jb_batch_run_timed", "jb_batch_last_timing", "jb_batch_size",
    "jb_batch_num_frames", "jb_batch_num_samples", "jb_batch_total_samples", "jb_batch_read_pcm",
    "jb_batch_read_pcm_i16", "jb_batch_read_pcm_all", "jb_batch_read_pcm_i16_all", "jb_pdf_set_create", "jb_pdf_set_free", "jb_batch_create_indexed", "jb_batch_read_track", "jb_release_cached_memory", "jb_set_cached_memory_limit", "jb_batch_read_coefficients", "jb_batch_read_first_coefficients", "jb_batch_read_excitation", "jb_batch_device_pcm", "jb_batch_pcm_offset",
    "jb_batch_info", "jb_batch_kernel_info", "jb_batch_redo_stats", "jb_batch_gang_fallbacks", "jb_batch_free", "jb_paramgen_vocode_batch",
    "jb_mlpg_batch", "jb_batch_create_from_tracks", "jb_vocode_tracks_batch",
    "jb_engine_load", "jb_engine_load_from_bytes", "jb_engine_new", "jb_engine_free",
    "jb_engine_set_sampling_frequency", "jb_engine_get_sampling_frequency",
    "jb_engine_set_fperiod", "jb_engine_get_fperiod", "jb_engine_set_volume", "jb_engine_get_volume",
    "jb_engine_set_msd_threshold", "jb_engine_get_msd_threshold", "jb_engine_set_gv_weight",
    "jb_engine_get_gv_weight", "jb_engine_set_phoneme_alignment_flag",
    "jb_engine_get_phoneme_alignment_flag", "jb_engine_set_batch_invariant", "jb_engine_get_batch_invariant",
    "jb_engine_set_fast_invariant", "jb_engine_get_fast_invariant",
    "jb_engine_set_speed", "jb_engine_get_speed",
    "jb_engine_set_alpha", "jb_engine_get_alpha", "jb_engine_set_beta", "jb_engine_get_beta",
    "jb_engine_set_additional_half_tone", "jb_engine_get_additional_half_tone",
    "jb_engine_num_voices", "jb_engine_num_streams", "jb_engine_num_states",
    "jb_engine_set_interpolation_weight", "jb_engine_get_interpolation_weight", "jb_synthesize", "jb_pcm_free", "jb_write_wav_i16", "jb_write_wav_f64", "jb_synthesize_batch", "jb_synthesize_batch_i16", "jb_pcm_i16_free",
    "jb_engine_model_shape", "jb_engine_pdf_table", "jb_engine_tree_index",
    "jb_engine_states", "jb_states_utt", "jb_engine_voice_desc", "jb_states_free",
    "jb_generator_new", "jb_generator_new_from_tracks", "jb_vocoder_synthesize_batch", "jb_generator_fperiod", "jb_generator_synthesized_frames",
    "jb_generator_total_frames", "jb_generator_step", "jb_generator_step_n", "jb_generator_free",
    "jb_comm_unique_id", "jb_comm_init", "jb_comm_rank", "jb_comm_size", "jb_comm_free", "jb_gather_pcm",
    "jb_gathered_samples", "jb_gathered_sample_bytes", "jb_gathered_device", "jb_gathered_read", "jb_gathered_free",
    "jb_lpt_partition", "jb_paramgen_vocode_batch_multi", "jb_synthesize_batch_multi", "jb_synthesize_batch_i16_multi",
    "jb_states_duration_params", "jb_last_error", "jb_device_count", "jb_device_arch", "jb_device_pci_bus_id", "jb_version", "jb_default_verify_tol",
    "jb_batch_create_voc", "jb_batch_create_indexed_voc", "jb_synthesize_batch_each", "jb_synthesize_batch_each_i16",
    "jb_batch_set_output_rate", "jb_batch_output_rate", "jb_batch_read_pcm_native", "jb_resample_filter",
    "jb_resample_pcm_batch", "jb_engine_set_output_sampling_frequency", "jb_engine_get_output_sampling_frequency",
    "jb_resample_geometry",
    "jb_batch_set_loudness_target", "jb_batch_loudness", "jb_loudness_filter", "jb_loudness_pcm_batch",
    "jb_engine_set_loudness_target", "jb_engine_get_loudness_target", "jb_engine_set_peak_ceiling",
    "jb_engine_get_peak_ceiling",
    "jb_batch_set_flac", "jb_batch_flac_size", "jb_batch_read_flac", "jb_batch_read_flac_all",
    "jb_flac_encode_pcm_batch", "jb_flac_free", "jb_synthesize_flac", "jb_synthesize_batch_flac",
    "jb_synthesize_batch_each_flac",
    "jb_batch_set_flac_meta", "jb_flac_encode_pcm_batch_meta", "jb_flac_md5_pcm_batch", "jb_md5_host",
    "jb_flac_seek_geometry", "jb_synthesize_flac_meta", "jb_synthesize_batch_flac_meta",
    "jb_synthesize_batch_each_flac_meta",
    "jb_batch_set_peak_mode", "jb_batch_loudness_report", "jb_true_peak_filter", "jb_true_peak_pcm_batch",
    "jb_engine_set_peak_mode", "jb_engine_get_peak_mode",
    "jb_engine_set_tree_search", "jb_engine_get_tree_search", "jb_engine_device_searched_labels",
    "jb_tree_search_batch", "jb_tree_search_flat_host",
    "jb_format_bytes_per_sample", "jb_batch_set_format", "jb_batch_formatted_size", "jb_batch_read_formatted",
    "jb_batch_read_formatted_all", "jb_format_pcm_batch", "jb_format_pcm_host", "jb_format_free",
    "jb_synthesize_formatted", "jb_synthesize_batch_formatted", "jb_synthesize_batch_each_formatted",
    "jb_write_wav_formatted",
    "jb_batch_set_adpcm", "jb_batch_adpcm_size", "jb_batch_adpcm_block_align", "jb_batch_read_adpcm",
    "jb_batch_read_adpcm_all", "jb_adpcm_geometry", "jb_adpcm_encode_host", "jb_adpcm_encode_i16_host",
    "jb_adpcm_decode_host", "jb_adpcm_encode_pcm_batch", "jb_adpcm_free", "jb_write_wav_adpcm",
    "jb_synthesize_adpcm", "jb_synthesize_batch_adpcm", "jb_synthesize_batch_each_adpcm",
    "jb_batch_set_fbank", "jb_batch_fbank_shape", "jb_batch_fbank_size", "jb_batch_read_fbank",
    "jb_batch_read_fbank_all", "jb_fbank_geometry", "jb_fbank_window", "jb_fbank_filterbank", "jb_fbank_host",
    "jb_fbank_pcm_batch", "jb_fbank_free", "jb_synthesize_fbank", "jb_synthesize_batch_fbank",
    "jb_synthesize_batch_each_fbank", "jb_synthesize_programme_fbank",
    "jb_mfcc_geometry", "jb_mfcc_dct", "jb_mfcc_delta_kernel", "jb_mfcc_host", "jb_mfcc_pcm_host",
    "jb_mfcc_frames_batch", "jb_mfcc_pcm_batch", "jb_mfcc_free",
    "jb_frame_kaldi", "jb_frame_check", "jb_fbank_framed_geometry", "jb_frame_window", "jb_fbank_framed_host",
    "jb_mfcc_framed_pcm_host", "jb_fbank_framed_pcm_batch", "jb_mfcc_framed_pcm_batch",
    "jb_batch_set_frame_opts", "jb_engine_set_frame_opts",
    "jb_batch_set_mfcc", "jb_batch_mfcc_shape", "jb_batch_mfcc_size", "jb_batch_read_mfcc", "jb_batch_read_mfcc_all",
    "jb_synthesize_mfcc", "jb_synthesize_batch_mfcc", "jb_synthesize_batch_each_mfcc", "jb_synthesize_programme_mfcc",
    "jb_melspec_whisper", "jb_melspec_geometry", "jb_melspec_window", "jb_melspec_filterbank", "jb_melspec_host",
    "jb_melspec_pcm_batch", "jb_melspec_free",
    "jb_batch_set_melspec", "jb_batch_melspec_shape", "jb_batch_melspec_size", "jb_batch_read_melspec",
    "jb_batch_read_melspec_all", "jb_synthesize_melspec", "jb_synthesize_batch_melspec",
    "jb_synthesize_batch_each_melspec", "jb_synthesize_programme_melspec",
    "jb_batch_set_loudness_groups", "jb_batch_loudness_group_of", "jb_batch_loudness_group",
    "jb_batch_set_loudness_report", "jb_batch_loudness_r128", "jb_loudness_groups_pcm_batch",
    "jb_loudness_gate_host", "jb_engine_set_loudness_scope", "jb_engine_get_loudness_scope",
    "jb_batch_set_join", "jb_batch_num_outputs", "jb_batch_programme_of", "jb_batch_programme_layout",
    "jb_batch_member_start", "jb_batch_read_programme_pcm", "jb_batch_read_programme_pcm_i16",
    "jb_join_ms_to_samples", "jb_join_geometry", "jb_join_host", "jb_join_i16_host", "jb_join_pcm_batch",
    "jb_join_pcm_batch_i16", "jb_join_free",
    "jb_batch_set_mix", "jb_batch_mix_report", "jb_mix_gain", "jb_mix_geometry", "jb_mix_host", "jb_mix_i16_host",
    "jb_mix_pcm_batch", "jb_mix_pcm_batch_i16", "jb_mix_free", "jb_engine_set_programme_mix",
    "jb_engine_get_programme_mix",
    "jb_batch_set_mix_stems", "jb_batch_num_programmes", "jb_batch_stem_unit", "jb_batch_stem_layout",
    "jb_batch_stem_report", "jb_mix_stems_geometry", "jb_mix_stems_host", "jb_mix_stems_i16_host",
    "jb_mix_levels_host", "jb_mix_levels_i16_host", "jb_mix_levels_db", "jb_mix_stems_pcm_batch",
    "jb_mix_stems_pcm_batch_i16", "jb_synthesize_programme_stems", "jb_synthesize_programme_stems_flac_meta",
    "jb_activity_geometry", "jb_activity_host", "jb_activity_members_host", "jb_activity_pcm_batch",
    "jb_activity_pcm_batch_i16", "jb_activity_free", "jb_batch_set_activity", "jb_batch_activity_shape",
    "jb_batch_activity_size", "jb_batch_read_activity", "jb_batch_read_activity_all", "jb_batch_activity_report",
    "jb_batch_activity_unit_report", "jb_synthesize_programme_activity",
    "jb_pitch_kaldi", "jb_pitch_geometry", "jb_pitch_lags", "jb_pitch_host", "jb_pitch_pcm_batch", "jb_pitch_free",
    "jb_batch_set_pitch", "jb_batch_pitch_shape", "jb_batch_pitch_size", "jb_batch_read_pitch", "jb_batch_read_pitch_all",
    "jb_synthesize_pitch", "jb_synthesize_batch_pitch", "jb_synthesize_batch_each_pitch", "jb_synthesize_programme_pitch",
    "jb_batch_set_filter", "jb_batch_filter_coefficients", "jb_filter_design", "jb_filter_pcm_host",
    "jb_filter_pcm_batch", "jb_filter_pcm_batch_i16", "jb_filter_free", "jb_engine_set_filter", "jb_engine_get_filter",
    "jb_batch_set_fir", "jb_batch_fir_geometry", "jb_engine_set_fir", "jb_fir_host", "jb_fir_geometry",
    "jb_fir_pcm_batch", "jb_fir_pcm_batch_i16", "jb_fir_free",
    "jb_room_host", "jb_room_rir_batch", "jb_room_free", "jb_room_geometry", "jb_room_lowpass", "jb_room_design",
    "jb_room_vary", "jb_batch_set_room", "jb_batch_room_report", "jb_engine_set_room",
    "jb_batch_set_noise", "jb_batch_noise_report", "jb_engine_set_noise", "jb_engine_get_noise", "jb_noise_host",
    "jb_noise_host_i16", "jb_noise_white", "jb_noise_vary", "jb_noise_pcm_batch", "jb_noise_pcm_batch_i16",
    "jb_noise_free",
    "jb_batch_set_limiter", "jb_batch_limiter_report", "jb_limiter_window", "jb_limiter_host", "jb_limiter_host_i16",
    "jb_limiter_pcm_batch", "jb_limiter_pcm_batch_i16", "jb_limiter_free", "jb_engine_set_limiter",
    "jb_engine_get_limiter",
    "jb_synthesize_programme", "jb_synthesize_programme_i16", "jb_synthesize_programme_flac_meta",
    "jb_synthesize_programme_formatted", "jb_synthesize_programme_adpcm",
]


def build(force: bool = False) -> Path:
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = list((_HERE / "csrc").glob("*.hip")) + list((_HERE / "csrc").glob("*.cpp")) + \
        list((_HERE / "csrc").glob("*.h")) + [_HERE.parent / "include" / "jbonsai_amd.h"]
    stale = (not LIB_PATH.exists()) or any(p.stat().st_mtime > LIB_PATH.stat().st_mtime for p in srcs)
    if force or stale:
        r = subprocess.run(["bash", str(_HERE / "csrc" / "build.sh")], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc build failed:\n" + r.stdout + r.stderr)
    return LIB_PATH


_lib = None


def lib():
    """Load libjbonsai_amd.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                           " (the HIP library is the product; there is no fallback)")
    L = C.CDLL(str(LIB_PATH))
    vp, sz, dp = C.c_void_p, C.c_size_t, C.POINTER(C.c_double)
    L.jb_last_error.restype = C.c_char_p
    L.jb_version.restype = C.c_char_p
    L.jb_default_verify_tol.restype = C.c_double
    L.jb_device_count.restype = C.c_int
    L.jb_device_arch.argtypes = [C.c_int, C.c_char_p, sz]
    L.jb_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, sz]
    L.jb_batch_create.argtypes = [C.POINTER(VoiceDesc), C.POINTER(StateUtt), sz, C.POINTER(BatchOpts),
                                  C.POINTER(vp)]
    L.jb_pdf_set_create.argtypes = [C.POINTER(PdfTable), C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(vp)]
    L.jb_pdf_set_free.argtypes = [vp]
    L.jb_pdf_set_free.restype = None
    L.jb_batch_create_indexed.argtypes = [C.POINTER(VoiceDesc), vp, C.POINTER(IndexUtt), sz, C.POINTER(BatchOpts),
                                          C.POINTER(vp)]
    L.jb_batch_create_voc.argtypes = [C.POINTER(VoiceDesc), C.POINTER(StateUtt), sz, C.POINTER(UttVoc),
                                      C.POINTER(BatchOpts), C.POINTER(vp)]
    L.jb_batch_create_indexed_voc.argtypes = [C.POINTER(VoiceDesc), vp, C.POINTER(IndexUtt), sz, C.POINTER(UttVoc),
                                              C.POINTER(BatchOpts), C.POINTER(vp)]
    L.jb_batch_run.argtypes = [vp]
    L.jb_batch_sync.argtypes = [vp]
    L.jb_batch_run_timed.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.jb_batch_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    for n in ("jb_batch_size", "jb_batch_total_samples"):
        getattr(L, n).restype = sz
        getattr(L, n).argtypes = [vp]
    for n in ("jb_batch_num_frames", "jb_batch_num_samples", "jb_batch_pcm_offset"):
        getattr(L, n).restype = sz
        getattr(L, n).argtypes = [vp, sz]
    L.jb_batch_read_pcm.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_pcm_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_batch_read_pcm_i16_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_batch_read_track.argtypes = [vp, sz, C.c_uint32, vp, sz]
    L.jb_batch_read_coefficients.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_first_coefficients.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_pcm_i16.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_excitation.argtypes = [vp, sz, vp, sz]
    L.jb_batch_device_pcm.restype = vp
    L.jb_batch_device_pcm.argtypes = [vp, C.POINTER(sz)]
    L.jb_batch_info.argtypes = [vp] + [C.POINTER(C.c_uint32)] * 4
    L.jb_batch_redo_stats.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.jb_batch_kernel_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.jb_batch_gang_fallbacks.argtypes = [vp]
    L.jb_batch_gang_fallbacks.restype = C.c_uint32
    L.jb_batch_free.argtypes = [vp]
    L.jb_batch_free.restype = None
    L.jb_paramgen_vocode_batch.argtypes = [C.POINTER(VoiceDesc), C.POINTER(StateUtt), sz,
                                           C.POINTER(BatchOpts), C.POINTER(dp), C.POINTER(sz)]
    L.jb_mlpg_batch.argtypes = [C.POINTER(VoiceDesc), C.POINTER(StateUtt), sz, C.POINTER(BatchOpts),
                                C.POINTER(dp), C.POINTER(sz)]
    L.jb_batch_create_from_tracks.argtypes = [C.POINTER(VoiceDesc), C.POINTER(TrackUtt), sz, C.POINTER(BatchOpts),
                                              C.POINTER(vp)]
    L.jb_vocode_tracks_batch.argtypes = [C.POINTER(VoiceDesc), C.POINTER(TrackUtt), sz, C.POINTER(BatchOpts),
                                         C.POINTER(dp), C.POINTER(sz)]
    L.jb_vocoder_synthesize_batch.argtypes = [C.POINTER(VoiceDesc), C.POINTER(TrackUtt), sz, C.POINTER(BatchOpts),
                                              C.POINTER(dp), C.POINTER(sz)]
    L.jb_generator_new_from_tracks.argtypes = [C.POINTER(VoiceDesc), C.POINTER(TrackUtt), C.POINTER(BatchOpts),
                                               C.POINTER(vp)]
    L.jb_set_cached_memory_limit.argtypes = [sz]
    L.jb_comm_unique_id.argtypes = [C.c_char_p, sz]
    L.jb_comm_init.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int32, C.POINTER(vp)]
    L.jb_comm_rank.argtypes = [vp]
    L.jb_comm_size.argtypes = [vp]
    L.jb_comm_free.argtypes = [vp]
    L.jb_comm_free.restype = None
    L.jb_gather_pcm.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_float)]
    L.jb_gathered_samples.argtypes = [vp, C.c_int]
    L.jb_gathered_samples.restype = sz
    L.jb_gathered_sample_bytes.argtypes = [vp]
    L.jb_gathered_sample_bytes.restype = sz
    L.jb_gathered_device.argtypes = [vp, C.c_int]
    L.jb_gathered_device.restype = vp
    L.jb_gathered_read.argtypes = [vp, C.c_int, vp, sz]
    L.jb_gathered_free.argtypes = [vp]
    L.jb_gathered_free.restype = None
    L.jb_lpt_partition.argtypes = [C.POINTER(C.c_uint64), sz, sz, C.POINTER(C.c_uint32)]
    L.jb_paramgen_vocode_batch_multi.argtypes = [C.POINTER(VoiceDesc), C.POINTER(StateUtt), sz, C.POINTER(BatchOpts),
                                                 C.POINTER(C.c_int32), sz, C.POINTER(dp), C.POINTER(sz)]
    L.jb_pcm_free.argtypes = [dp]
    L.jb_pcm_free.restype = None
    L.jb_batch_set_output_rate.argtypes = [vp, C.POINTER(C.c_uint32), sz]
    L.jb_batch_output_rate.argtypes = [vp, sz]
    L.jb_batch_output_rate.restype = C.c_uint32
    L.jb_batch_read_pcm_native.argtypes = [vp, sz, vp, sz]
    L.jb_resample_filter.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32), dp, sz]
    L.jb_resample_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, C.c_uint32, C.c_uint32, C.c_int32,
                                        C.POINTER(dp), C.POINTER(sz)]
    L.jb_resample_geometry.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(ResampleGeometry)]
    L.jb_engine_set_output_sampling_frequency.argtypes = [vp, sz]
    L.jb_engine_get_output_sampling_frequency.argtypes = [vp]
    L.jb_engine_get_output_sampling_frequency.restype = sz
    L.jb_batch_set_loudness_target.argtypes = [vp, dp, sz, C.c_double]
    L.jb_batch_loudness.argtypes = [vp, sz, dp, dp, dp]
    L.jb_loudness_filter.argtypes = [C.c_uint32, dp, dp, C.POINTER(C.c_uint32)]
    L.jb_loudness_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, C.c_uint32, C.c_int32, dp, dp]
    for n in ("loudness_target", "peak_ceiling"):
        getattr(L, "jb_engine_set_" + n).argtypes = [vp, C.c_double]
        getattr(L, "jb_engine_get_" + n).argtypes = [vp]
        getattr(L, "jb_engine_get_" + n).restype = C.c_double
    L.jb_batch_set_peak_mode.argtypes = [vp, C.POINTER(C.c_uint32), sz]
    u32p = C.POINTER(C.c_uint32)
    L.jb_batch_set_loudness_groups.argtypes = [vp, u32p, sz]
    L.jb_batch_loudness_group_of.argtypes = [vp, sz]
    L.jb_batch_loudness_group_of.restype = C.c_int32
    L.jb_batch_loudness_group.argtypes = [vp, sz, C.POINTER(LoudnessGroupReport)]
    L.jb_batch_set_loudness_report.argtypes = [vp, C.c_uint32]
    L.jb_batch_loudness_r128.argtypes = [vp, sz, C.POINTER(LoudnessR128)]
    L.jb_loudness_groups_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, u32p, C.c_uint32, C.c_int32,
                                               C.c_uint32, C.c_double, C.c_double, u32p,
                                               C.POINTER(LoudnessGroupReport), sz, C.POINTER(sz),
                                               C.POINTER(LoudnessR128), dp]
    L.jb_loudness_gate_host.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, C.c_uint32, dp, dp, C.c_double, C.c_double,
                                        C.POINTER(LoudnessGroupReport), C.POINTER(LoudnessR128)]
    L.jb_batch_loudness_report.argtypes = [vp, sz, C.POINTER(LoudnessReport)]
    L.jb_true_peak_filter.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), dp, sz]
    L.jb_true_peak_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, C.c_uint32, C.c_int32, dp]
    L.jb_engine_set_peak_mode.argtypes = [vp, C.c_uint32]
    L.jb_engine_set_loudness_scope.argtypes = [vp, C.c_uint32]
    L.jb_engine_get_loudness_scope.argtypes = [vp]
    L.jb_engine_get_loudness_scope.restype = C.c_uint32
    L.jb_engine_get_peak_mode.argtypes = [vp]
    L.jb_engine_get_peak_mode.restype = C.c_uint32
    L.jb_engine_set_tree_search.argtypes = [vp, C.c_uint32]
    L.jb_engine_get_tree_search.argtypes = [vp]
    L.jb_engine_get_tree_search.restype = C.c_uint32
    L.jb_engine_device_searched_labels.argtypes = [vp]
    L.jb_engine_device_searched_labels.restype = C.c_uint64
    i32p = C.POINTER(C.c_int32)
    L.jb_tree_search_batch.argtypes = [vp, C.POINTER(C.c_char_p), sz, C.c_int32, i32p, i32p, C.POINTER(C.c_uint8)]
    L.jb_tree_search_flat_host.argtypes = [vp, C.POINTER(C.c_char_p), sz, i32p, i32p, C.POINTER(C.c_uint8)]
    u8p, fop = C.POINTER(C.c_uint8), C.POINTER(FlacOpts)
    L.jb_batch_set_flac.argtypes = [vp, fop]
    L.jb_batch_flac_size.argtypes = [vp, sz, C.POINTER(sz)]
    L.jb_batch_read_flac.argtypes = [vp, sz, u8p, sz]
    L.jb_batch_read_flac_all.argtypes = [vp, C.POINTER(u8p)]
    L.jb_flac_encode_pcm_batch.argtypes = [C.POINTER(C.POINTER(C.c_int16)), C.POINTER(sz), sz, C.c_uint32, fop,
                                           C.c_int32, C.POINTER(u8p), C.POINTER(sz)]
    L.jb_flac_free.argtypes = [u8p]
    L.jb_flac_free.restype = None
    L.jb_synthesize_flac.argtypes = [vp, C.POINTER(C.c_char_p), sz, fop, C.POINTER(u8p), C.POINTER(sz)]
    L.jb_synthesize_batch_flac.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, fop,
                                           C.POINTER(u8p), C.POINTER(sz)]
    L.jb_synthesize_batch_each_flac.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32,
                                                fop, C.POINTER(u8p), C.POINTER(sz)]
    fmp, i16pp = C.POINTER(FlacMeta), C.POINTER(C.POINTER(C.c_int16))
    L.jb_batch_set_flac_meta.argtypes = [vp, fmp]
    L.jb_flac_encode_pcm_batch_meta.argtypes = [i16pp, C.POINTER(sz), sz, C.c_uint32, fop, fmp, C.c_int32,
                                                C.POINTER(u8p), C.POINTER(sz)]
    L.jb_flac_md5_pcm_batch.argtypes = [i16pp, C.POINTER(sz), sz, C.c_int32, vp]
    L.jb_md5_host.argtypes = [vp, sz, vp]
    L.jb_flac_seek_geometry.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
    L.jb_synthesize_flac_meta.argtypes = [vp, C.POINTER(C.c_char_p), sz, fop, fmp, C.POINTER(u8p), C.POINTER(sz)]
    L.jb_synthesize_batch_flac_meta.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, fop, fmp,
                                                C.POINTER(u8p), C.POINTER(sz)]
    L.jb_synthesize_batch_each_flac_meta.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(sz), sz,
                                                     C.c_int32, fop, fmp, C.POINTER(u8p), C.POINTER(sz)]
    mop = C.POINTER(FormatOpts)
    L.jb_format_bytes_per_sample.argtypes = [C.c_uint32]
    L.jb_format_bytes_per_sample.restype = sz
    L.jb_batch_set_format.argtypes = [vp, mop]
    L.jb_batch_formatted_size.argtypes = [vp, sz, C.POINTER(sz)]
    L.jb_batch_read_formatted.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_formatted_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_format_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, mop, C.c_int32, C.POINTER(u8p), C.POINTER(sz)]
    L.jb_format_pcm_host.argtypes = [vp, sz, mop, vp, sz]
    L.jb_format_free.argtypes = [u8p]
    L.jb_format_free.restype = None
    L.jb_synthesize_formatted.argtypes = [vp, C.POINTER(C.c_char_p), sz, mop, C.POINTER(u8p), C.POINTER(sz)]
    L.jb_synthesize_batch_formatted.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, mop,
                                                C.POINTER(u8p), C.POINTER(sz)]
    L.jb_synthesize_batch_each_formatted.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(sz), sz,
                                                     C.c_int32, mop, C.POINTER(u8p), C.POINTER(sz)]
    L.jb_write_wav_formatted.argtypes = [C.c_char_p, vp, sz, C.c_uint32, C.c_uint32]
    aop, u32p = C.POINTER(AdpcmOpts), C.POINTER(C.c_uint32)
    L.jb_batch_set_adpcm.argtypes = [vp, aop]
    L.jb_batch_adpcm_size.argtypes = [vp, sz, C.POINTER(sz)]
    L.jb_batch_adpcm_block_align.argtypes = [vp, sz, u32p]
    L.jb_batch_read_adpcm.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_adpcm_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_adpcm_geometry.argtypes = [C.c_uint32, C.c_uint32, sz, u32p, u32p, C.POINTER(sz), C.POINTER(sz)]
    L.jb_adpcm_encode_host.argtypes = [vp, sz, C.c_uint32, aop, vp, sz]
    L.jb_adpcm_encode_i16_host.argtypes = [vp, sz, C.c_uint32, aop, vp, sz]
    L.jb_adpcm_decode_host.argtypes = [vp, sz, C.c_uint32, sz, vp, sz]
    L.jb_adpcm_encode_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, u32p, aop, C.c_int32, C.POINTER(u8p),
                                            C.POINTER(sz)]
    L.jb_adpcm_free.argtypes = [u8p]
    L.jb_adpcm_free.restype = None
    fop = C.POINTER(FbankOpts)
    L.jb_batch_set_fbank.argtypes = [vp, fop]
    L.jb_batch_fbank_shape.argtypes = [vp, sz, C.POINTER(sz), u32p, u32p]
    L.jb_batch_fbank_size.argtypes = [vp, sz, C.POINTER(sz)]
    L.jb_batch_read_fbank.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_fbank_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_fbank_geometry.argtypes = [C.c_uint32, fop, sz, u32p, u32p, u32p, C.POINTER(sz), C.POINTER(sz)]
    L.jb_fbank_window.argtypes = [C.c_uint32, fop, vp, sz]
    L.jb_fbank_filterbank.argtypes = [C.c_uint32, fop, vp, sz]
    L.jb_fbank_host.argtypes = [vp, sz, C.c_uint32, fop, vp, sz]
    L.jb_fbank_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, u32p, fop, C.c_int32, C.POINTER(u8p),
                                     C.POINTER(sz)]
    L.jb_fbank_free.argtypes = [u8p]
    L.jb_fbank_free.restype = None
    msop = C.POINTER(MelspecOpts)
    L.jb_melspec_whisper.argtypes = [C.c_uint32, msop]
    L.jb_melspec_geometry.argtypes = [C.c_uint32, msop, sz, u32p, u32p, u32p, C.POINTER(sz), C.POINTER(sz)]
    L.jb_melspec_window.argtypes = [C.c_uint32, msop, vp, sz]
    L.jb_melspec_filterbank.argtypes = [C.c_uint32, msop, vp, sz]
    L.jb_melspec_host.argtypes = [vp, sz, C.c_uint32, msop, vp, sz]
    L.jb_melspec_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, u32p, msop, C.c_int32, C.POINTER(u8p),
                                       C.POINTER(sz)]
    L.jb_batch_set_melspec.argtypes = [vp, msop]
    L.jb_batch_melspec_shape.argtypes = [vp, sz, C.POINTER(sz), u32p, u32p]
    L.jb_batch_melspec_size.argtypes = [vp, sz, C.POINTER(sz)]
    L.jb_batch_read_melspec.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_melspec_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_melspec_free.argtypes = [u8p]
    L.jb_melspec_free.restype = None
    cop = C.POINTER(MfccOpts)
    L.jb_mfcc_geometry.argtypes = [C.c_uint32, fop, cop, sz, C.POINTER(sz), u32p, C.POINTER(sz)]
    L.jb_mfcc_dct.argtypes = [C.c_uint32, cop, vp, sz, vp, sz]
    L.jb_mfcc_delta_kernel.argtypes = [C.c_uint32, C.c_uint32, vp, sz]
    L.jb_mfcc_host.argtypes = [vp, sz, C.c_uint32, cop, vp, sz]
    L.jb_mfcc_pcm_host.argtypes = [vp, sz, C.c_uint32, fop, cop, vp, sz]
    L.jb_mfcc_frames_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, C.c_uint32, cop, C.c_int32, C.POINTER(u8p),
                                       C.POINTER(sz)]
    L.jb_mfcc_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, u32p, fop, cop, C.c_int32, C.POINTER(u8p),
                                    C.POINTER(sz)]
    L.jb_mfcc_free.argtypes = [u8p]
    L.jb_mfcc_free.restype = None
    frp = C.POINTER(FrameOpts)
    L.jb_frame_kaldi.argtypes = [C.c_uint32, fop, frp]
    L.jb_frame_check.argtypes = [fop, cop, frp]
    L.jb_fbank_framed_geometry.argtypes = [C.c_uint32, fop, frp, sz, u32p, u32p, u32p, C.POINTER(sz), C.POINTER(sz)]
    L.jb_frame_window.argtypes = [C.c_uint32, fop, frp, vp, sz]
    L.jb_fbank_framed_host.argtypes = [vp, sz, C.c_uint32, fop, frp, vp, sz]
    L.jb_mfcc_framed_pcm_host.argtypes = [vp, sz, C.c_uint32, fop, cop, frp, vp, sz]
    L.jb_fbank_framed_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, u32p, fop, frp, C.c_int32,
                                            C.POINTER(u8p), C.POINTER(sz)]
    L.jb_mfcc_framed_pcm_batch.argtypes = [C.POINTER(dp), C.POINTER(sz), sz, u32p, fop, cop, frp, C.c_int32,
                                           C.POINTER(u8p), C.POINTER(sz)]
    L.jb_batch_set_frame_opts.argtypes = [vp, frp]
    L.jb_engine_set_frame_opts.argtypes = [vp, frp]
    L.jb_batch_set_mfcc.argtypes = [vp, fop, cop]
    L.jb_batch_mfcc_shape.argtypes = [vp, sz, C.POINTER(sz), u32p, u32p]
    L.jb_batch_mfcc_size.argtypes = [vp, sz, C.POINTER(sz)]
    L.jb_batch_read_mfcc.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_mfcc_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_synthesize_mfcc.argtypes = [vp, C.POINTER(C.c_char_p), sz, fop, cop, C.POINTER(u8p), C.POINTER(sz),
                                     C.POINTER(sz)]
    L.jb_synthesize_batch_mfcc.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, fop, cop,
                                           C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_batch_each_mfcc.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32,
                                                fop, cop, C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_programme_mfcc.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, fop, cop,
                                               C.POINTER(JoinOpts), C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz),
                                               C.POINTER(C.c_uint64)]
    L.jb_synthesize_fbank.argtypes = [vp, C.POINTER(C.c_char_p), sz, fop, C.POINTER(u8p), C.POINTER(sz),
                                      C.POINTER(sz)]
    L.jb_synthesize_batch_fbank.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, fop,
                                            C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_batch_each_fbank.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32,
                                                 fop, C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_programme_fbank.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, fop,
                                                C.POINTER(JoinOpts), C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz),
                                                C.POINTER(C.c_uint64)]
    L.jb_synthesize_melspec.argtypes = [vp, C.POINTER(C.c_char_p), sz, msop, C.POINTER(u8p), C.POINTER(sz),
                                        C.POINTER(sz)]
    L.jb_synthesize_batch_melspec.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, msop,
                                              C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_batch_each_melspec.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32,
                                                   msop, C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_programme_melspec.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, msop,
                                                  C.POINTER(JoinOpts), C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz),
                                                  C.POINTER(C.c_uint64)]
    L.jb_write_wav_adpcm.argtypes = [C.c_char_p, vp, sz, sz, C.c_uint32, C.c_uint32]
    L.jb_synthesize_adpcm.argtypes = [vp, C.POINTER(C.c_char_p), sz, aop, C.POINTER(u8p), C.POINTER(sz),
                                      C.POINTER(sz)]
    L.jb_synthesize_batch_adpcm.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, aop,
                                            C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_batch_each_adpcm.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32,
                                                 aop, C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    jup, jop, u64p = C.POINTER(JoinUtt), C.POINTER(JoinOpts), C.POINTER(C.c_uint64)
    L.jb_batch_set_join.argtypes = [vp, jup, sz]
    L.jb_batch_num_outputs.argtypes = [vp]
    L.jb_batch_num_outputs.restype = sz
    L.jb_batch_programme_of.argtypes = [vp, sz]
    L.jb_batch_programme_of.restype = C.c_int32
    L.jb_batch_programme_layout.argtypes = [vp, sz, C.POINTER(sz), u64p, u32p]
    L.jb_batch_member_start.argtypes = [vp, sz, u64p]
    L.jb_batch_read_programme_pcm.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_programme_pcm_i16.argtypes = [vp, sz, vp, sz]
    L.jb_join_ms_to_samples.argtypes = [C.c_double, C.c_uint32]
    L.jb_join_ms_to_samples.restype = C.c_uint64
    L.jb_join_geometry.argtypes = [jup, C.POINTER(sz), u32p, sz, u32p, u64p, C.POINTER(sz), u64p]
    L.jb_join_host.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, jup, C.POINTER(vp), C.POINTER(sz)]
    L.jb_join_i16_host.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, jup, C.POINTER(vp), C.POINTER(sz)]
    L.jb_join_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, jup, C.c_int32, C.POINTER(vp), C.POINTER(sz),
                                    C.POINTER(sz)]
    L.jb_join_pcm_batch_i16.argtypes = L.jb_join_pcm_batch.argtypes
    L.jb_join_free.argtypes = [vp]
    L.jb_join_free.restype = None
    mxup, mxop, mxrp = C.POINTER(MixUtt), C.POINTER(MixOpts), C.POINTER(MixReport)
    L.jb_batch_set_mix.argtypes = [vp, mxup, sz, mxop]
    L.jb_batch_mix_report.argtypes = [vp, sz, mxrp]
    L.jb_mix_gain.argtypes = [C.c_double]
    L.jb_mix_gain.restype = C.c_double
    L.jb_mix_geometry.argtypes = [mxup, C.POINTER(sz), u32p, sz, mxop, u32p, u64p, C.POINTER(sz), u64p, u32p, u64p]
    L.jb_mix_host.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, mxup, mxop, C.POINTER(C.c_double), C.POINTER(vp),
                              C.POINTER(sz), mxrp]
    L.jb_mix_i16_host.argtypes = L.jb_mix_host.argtypes
    L.jb_mix_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, mxup, mxop, C.c_int32, C.POINTER(vp), C.POINTER(sz),
                                   C.POINTER(sz), mxrp]
    L.jb_mix_pcm_batch_i16.argtypes = L.jb_mix_pcm_batch.argtypes
    L.jb_mix_free.argtypes = [vp]
    L.jb_mix_free.restype = None
    strp, dbp, i64p = C.POINTER(StemReport), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    L.jb_batch_set_mix_stems.argtypes = [vp, u32p, sz, C.c_uint32]
    L.jb_batch_num_programmes.argtypes = [vp]
    L.jb_batch_num_programmes.restype = sz
    L.jb_batch_stem_unit.argtypes = [vp, sz]
    L.jb_batch_stem_unit.restype = C.c_int64
    L.jb_batch_stem_layout.argtypes = [vp, sz, u32p, u32p, u32p, u64p, u64p]
    L.jb_batch_stem_report.argtypes = [vp, sz, strp]
    L.jb_mix_stems_geometry.argtypes = [mxup, u32p, C.POINTER(sz), u32p, sz, mxop, C.POINTER(sz), C.POINTER(sz), i64p,
                                        u64p, u32p, u32p, u32p, u64p, u64p, u32p]
    L.jb_mix_stems_host.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, mxup, u32p, C.c_uint32, mxop, dbp, C.POINTER(vp),
                                    C.POINTER(sz), mxrp, strp]
    L.jb_mix_stems_i16_host.argtypes = L.jb_mix_stems_host.argtypes
    L.jb_mix_levels_host.argtypes = [vp, vp, sz, C.c_uint64, C.c_uint64, dbp, dbp, dbp]
    L.jb_mix_levels_i16_host.argtypes = L.jb_mix_levels_host.argtypes
    L.jb_mix_levels_db.argtypes = [C.c_double, C.c_double, C.c_double, dbp, dbp, dbp]
    L.jb_mix_levels_db.restype = None
    L.jb_mix_stems_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, mxup, u32p, C.c_uint32, mxop, C.c_int32,
                                         C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), mxrp, strp]
    L.jb_mix_stems_pcm_batch_i16.argtypes = L.jb_mix_stems_pcm_batch.argtypes
    L.jb_engine_set_programme_mix.argtypes = [vp, C.POINTER(MixPlace), sz, mxop]
    L.jb_engine_get_programme_mix.argtypes = [vp, C.POINTER(MixPlace), sz, C.POINTER(sz), mxop]
    acop, acrp, acup = C.POINTER(ActivityOpts), C.POINTER(ActivityReport), C.POINTER(ActivityUnitReport)
    L.jb_activity_geometry.argtypes = [acop, C.c_uint32, sz, u32p, u32p, u64p]
    L.jb_activity_host.argtypes = [vp, sz, C.c_uint32, acop, vp, sz, acrp]
    L.jb_activity_members_host.argtypes = [C.POINTER(vp), C.POINTER(sz), u64p, C.POINTER(C.c_double), sz, C.c_uint64,
                                           C.c_uint32, acop, vp, sz, acrp, acup]
    L.jb_activity_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, mxup, mxop, u32p, acop, C.c_int32,
                                        C.POINTER(vp), u64p, u32p, C.POINTER(sz), acrp, acup]
    L.jb_activity_pcm_batch_i16.argtypes = L.jb_activity_pcm_batch.argtypes
    L.jb_activity_free.argtypes = [vp]
    L.jb_activity_free.restype = None
    L.jb_batch_set_activity.argtypes = [vp, acop]
    L.jb_batch_activity_shape.argtypes = [vp, sz, u64p, u32p, u32p]
    L.jb_batch_activity_size.argtypes = [vp, sz, C.POINTER(sz)]
    L.jb_batch_read_activity.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_activity_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_batch_activity_report.argtypes = [vp, sz, sz, acrp]
    L.jb_batch_activity_unit_report.argtypes = [vp, sz, acup]
    ptop = C.POINTER(PitchOpts)
    L.jb_pitch_kaldi.argtypes = [ptop]
    L.jb_pitch_geometry.argtypes = [ptop, C.c_uint32, sz, C.POINTER(PitchGeometry)]
    L.jb_pitch_lags.argtypes = [ptop, vp, sz, C.POINTER(sz)]
    L.jb_pitch_host.argtypes = [vp, sz, C.c_uint32, ptop, vp, sz, vp, vp, vp]
    L.jb_pitch_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, u32p, ptop, C.c_int32, C.POINTER(vp), u64p, u32p,
                                     C.POINTER(vp)]
    L.jb_pitch_free.argtypes = [vp]
    L.jb_pitch_free.restype = None
    L.jb_batch_set_pitch.argtypes = [vp, ptop]
    L.jb_batch_pitch_shape.argtypes = [vp, sz, C.POINTER(sz), u32p, u32p]
    L.jb_batch_pitch_size.argtypes = [vp, sz, C.POINTER(sz)]
    L.jb_batch_read_pitch.argtypes = [vp, sz, vp, sz]
    L.jb_batch_read_pitch_all.argtypes = [vp, C.POINTER(vp)]
    L.jb_synthesize_pitch.argtypes = [vp, C.POINTER(C.c_char_p), sz, ptop, C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_batch_pitch.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, ptop,
                                            C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_batch_each_pitch.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32,
                                                 ptop, C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz)]
    L.jb_synthesize_programme_pitch.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_int32, ptop,
                                                C.POINTER(JoinOpts), C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz),
                                                C.POINTER(C.c_uint64)]
    flp, bqp = C.POINTER(Filter), C.POINTER(Biquad)
    L.jb_batch_set_filter.argtypes = [vp, flp, sz]
    L.jb_batch_filter_coefficients.argtypes = [vp, sz, bqp, u32p]
    L.jb_filter_design.argtypes = [flp, C.c_uint32, bqp]
    L.jb_filter_pcm_host.argtypes = [dp, sz, flp, C.c_uint32, dp, sz]
    L.jb_filter_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, flp, u32p, C.c_int32, C.POINTER(vp),
                                      C.POINTER(sz)]
    L.jb_filter_pcm_batch_i16.argtypes = L.jb_filter_pcm_batch.argtypes
    L.jb_filter_free.argtypes = [vp]
    L.jb_filter_free.restype = None
    L.jb_engine_set_filter.argtypes = [vp, flp]
    L.jb_engine_get_filter.argtypes = [vp, flp]
    frp = C.POINTER(Fir)
    L.jb_batch_set_fir.argtypes = [vp, frp, sz]
    L.jb_batch_fir_geometry.argtypes = [vp, sz, u32p, u32p, u32p]
    L.jb_engine_set_fir.argtypes = [vp, frp]
    L.jb_fir_host.argtypes = [dp, sz, frp, dp, sz]
    L.jb_fir_geometry.argtypes = [C.c_uint32, u32p, u32p, u32p]
    L.jb_fir_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, frp, u32p, C.c_int32, C.POINTER(vp),
                                   C.POINTER(sz)]
    L.jb_fir_pcm_batch_i16.argtypes = L.jb_fir_pcm_batch.argtypes
    L.jb_fir_free.argtypes = [vp]
    L.jb_fir_free.restype = None
    rmp, d3 = C.POINTER(Room), C.POINTER(C.c_double)
    L.jb_room_host.argtypes = [rmp, dp, sz]
    L.jb_room_rir_batch.argtypes = [rmp, sz, C.c_int32, C.POINTER(vp), C.POINTER(sz)]
    L.jb_room_free.argtypes = [vp]
    L.jb_room_free.restype = None
    L.jb_room_geometry.argtypes = [rmp, C.POINTER(RoomInfo)]
    L.jb_room_lowpass.argtypes = [dp, sz, u32p, u32p]
    L.jb_room_design.argtypes = [d3, C.c_double, C.c_double, d3]
    L.jb_room_vary.argtypes = [C.c_uint64, C.c_uint64, d3, C.c_double, d3, d3]
    L.jb_batch_set_room.argtypes = [vp, rmp, sz]
    L.jb_batch_room_report.argtypes = [vp, sz, C.POINTER(RoomReport)]
    L.jb_engine_set_room.argtypes = [vp, rmp, C.c_uint32, C.c_uint64, C.c_double]
    nzp, nrp = C.POINTER(Noise), C.POINTER(NoiseReport)
    L.jb_batch_set_noise.argtypes = [vp, nzp, sz]
    L.jb_batch_noise_report.argtypes = [vp, sz, nrp]
    L.jb_engine_set_noise.argtypes = [vp, nzp]
    L.jb_engine_get_noise.argtypes = [vp, nzp]
    L.jb_noise_host.argtypes = [dp, sz, nzp, dp, dp, sz, nrp]
    L.jb_noise_host_i16.argtypes = [dp, sz, nzp, dp, C.POINTER(C.c_int16), sz, nrp]
    L.jb_noise_white.argtypes = [C.c_uint64, C.c_uint64, sz, dp]
    L.jb_noise_vary.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), u32p]
    L.jb_noise_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, nzp, u32p, C.c_int32, C.POINTER(vp),
                                     C.POINTER(sz), nrp]
    L.jb_noise_pcm_batch_i16.argtypes = L.jb_noise_pcm_batch.argtypes
    L.jb_noise_free.argtypes = [vp]
    L.jb_noise_free.restype = None
    lop, lrp = C.POINTER(LimiterOpts), C.POINTER(LimiterReport)
    L.jb_batch_set_limiter.argtypes = [vp, lop, sz]
    L.jb_batch_limiter_report.argtypes = [vp, sz, lrp]
    L.jb_limiter_window.argtypes = [C.c_uint32, lop, u32p, u32p, dp, sz]
    L.jb_limiter_host.argtypes = [dp, C.c_uint64, C.c_uint32, C.c_double, C.c_double, C.c_uint32, lop, dp, lrp]
    L.jb_limiter_host_i16.argtypes = [dp, C.c_uint64, C.c_uint32, C.c_double, C.c_double, C.c_uint32, lop,
                                      C.POINTER(C.c_int16), lrp]
    L.jb_limiter_pcm_batch.argtypes = [C.POINTER(vp), C.POINTER(sz), sz, u32p, dp, dp, u32p, lop, C.c_int32,
                                       C.POINTER(vp), lrp]
    L.jb_limiter_pcm_batch_i16.argtypes = L.jb_limiter_pcm_batch.argtypes
    L.jb_limiter_free.argtypes = [vp]
    L.jb_limiter_free.restype = None
    L.jb_engine_set_limiter.argtypes = [vp, lop]
    L.jb_engine_get_limiter.argtypes = [vp, lop]
    lines, szp = C.POINTER(C.c_char_p), C.POINTER(sz)
    L.jb_synthesize_programme.argtypes = [vp, lines, szp, sz, C.c_int32, jop, C.POINTER(vp), szp, u64p]
    L.jb_synthesize_programme_i16.argtypes = [vp, lines, szp, sz, C.c_int32, jop, C.POINTER(vp), szp, u64p]
    L.jb_synthesize_programme_stems.argtypes = [vp, lines, szp, sz, C.c_int32, jop, u32p, C.c_uint32, C.POINTER(vp), szp,
                                                szp, C.POINTER(StemReport), u64p]
    L.jb_synthesize_programme_stems_flac_meta.argtypes = [vp, lines, szp, sz, C.c_int32, C.POINTER(FlacOpts),
                                                          C.POINTER(FlacMeta), jop, u32p, C.c_uint32, C.POINTER(u8p),
                                                          szp, szp, C.POINTER(StemReport), u64p]
    L.jb_synthesize_programme_activity.argtypes = [vp, lines, szp, sz, C.c_int32, jop, C.POINTER(ActivityOpts),
                                                   C.POINTER(vp), szp, C.POINTER(vp), u64p, u32p, u64p]
    L.jb_synthesize_programme_flac_meta.argtypes = [vp, lines, szp, sz, C.c_int32, C.POINTER(FlacOpts),
                                                    C.POINTER(FlacMeta), jop, C.POINTER(u8p), szp, u64p]
    L.jb_synthesize_programme_formatted.argtypes = [vp, lines, szp, sz, C.c_int32, mop, jop, C.POINTER(u8p), szp,
                                                    u64p]
    L.jb_synthesize_programme_adpcm.argtypes = [vp, lines, szp, sz, C.c_int32, aop, jop, C.POINTER(u8p), szp, szp,
                                                u64p]
    L.jb_write_wav_i16.argtypes = [C.c_char_p, vp, sz, C.c_uint32]
    L.jb_write_wav_f64.argtypes = [C.c_char_p, vp, sz, C.c_uint32]
    _lib = L
    return L


def write_wav(path, pcm, sampling_frequency: int) -> None:
    """16-bit mono WAV as the reference's examples write it (examples/is-bonsai/main.rs:37-49).
    int16 samples are written as they are; float64 samples are clamped and truncated first."""
    import numpy as np

    a = np.ascontiguousarray(pcm)
    if a.dtype == np.int16:
        check(lib().jb_write_wav_i16(str(path).encode(), a.ctypes.data, a.size, sampling_frequency))
    else:
        a = np.ascontiguousarray(a, dtype=np.float64)
        check(lib().jb_write_wav_f64(str(path).encode(), a.ctypes.data, a.size, sampling_frequency))


def resample_filter(in_hz: int, out_hz: int):
    """The library's polyphase table for in_hz -> out_hz (include/jbonsai_amd.h jb_resample_filter; host only):
    (L, M, taps) with taps a float64 array [L][ntaps]."""
    import numpy as np

    L = lib()
    l_, m_, nt = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(L.jb_resample_filter(in_hz, out_hz, C.byref(l_), C.byref(m_), C.byref(nt), None, 0))
    taps = np.zeros((l_.value, nt.value), dtype=np.float64)
    check(L.jb_resample_filter(in_hz, out_hz, C.byref(l_), C.byref(m_), C.byref(nt),
                               taps.ctypes.data_as(C.POINTER(C.c_double)), taps.size))
    return l_.value, m_.value, taps


def resample_geometry(in_hz: int, out_hz: int):
    """jb_resample_geometry: the ResampleGeometry of in_hz -> out_hz (pure; no GPU needed)."""
    g = ResampleGeometry()
    check(lib().jb_resample_geometry(int(in_hz), int(out_hz), C.byref(g)))
    return g


def loudness_filter(hz: int):
    """The library's K-weighting at hz (include/jbonsai_amd.h jb_loudness_filter; host only): (b, a, hop) with b and a
    float64 arrays [2][3] (shelf, then high-pass)."""
    import numpy as np

    b, a, hop = np.zeros(6), np.zeros(6), C.c_uint32()
    dp = C.POINTER(C.c_double)
    check(lib().jb_loudness_filter(hz, b.ctypes.data_as(dp), a.ctypes.data_as(dp), C.byref(hop)))
    return b.reshape(2, 3), a.reshape(2, 3), hop.value


def _pcm_args(pcms, dtype, void: bool = False):
    """The inputs of a jb_*_pcm_batch call: (arrs, n, ins, nin) -- `pcms` as contiguous arrays of dtype (kept alive by
    the caller over the call), their count, their pointers (typed, or void * where the entry's argtypes say so) and
    their lengths."""
    import numpy as np

    arrs = [np.ascontiguousarray(a, dtype=dtype) for a in pcms]
    n = len(arrs)
    pt = C.c_void_p if void else C.POINTER(np.ctypeslib.as_ctypes_type(dtype))
    ins = (pt * max(n, 1))(*[a.ctypes.data_as(pt) for a in arrs])
    nin = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    return arrs, n, ins, nin


def _take(free, bufs, ns, n, dtype=None):
    """n library-owned buffers of ns[u] elements copied out -- bytes, or arrays of dtype -- and each released with
    `free`."""
    import numpy as np

    out = []
    for u in range(n):
        if dtype is None:
            out.append(C.string_at(bufs[u], ns[u]) if ns[u] else b"")
        elif ns[u]:
            ptr = C.cast(bufs[u], C.POINTER(np.ctypeslib.as_ctypes_type(dtype)))
            out.append(np.ctypeslib.as_array(ptr, shape=(int(ns[u]),)).copy())
        else:
            out.append(np.zeros(0, dtype=dtype))
        if bufs[u]:
            free(bufs[u])
    return out


def _feature_pcm(entry: str, free: str, pcms, hz, opts, device: int, rows):
    """A feature entry on caller-held PCM: `entry`(ins, nin, n, hzs, *opts, device, bufs, ns) over the float64 arrays
    of `pcms` (or one array) at hz (one rate, or one per array), every output through rows(bytes) and released with
    `free`.  A single array in gives a single array out."""
    import numpy as np

    single = isinstance(pcms, np.ndarray)
    arrs, n, ins, nin = _pcm_args([pcms] if single else pcms, np.float64)
    rates = [int(hz)] * n if np.isscalar(hz) else [int(h) for h in hz]
    if len(rates) != n:
        raise ValueError("give one rate, or one per array")
    L = lib()
    hzs = (C.c_uint32 * max(n, 1))(*rates)
    bufs, ns = (C.POINTER(C.c_uint8) * max(n, 1))(), (C.c_size_t * max(n, 1))()
    check(getattr(L, entry)(ins, nin, n, hzs, *[C.byref(o) for o in opts], device, bufs, ns))
    res = [rows(d) for d in _take(getattr(L, free), bufs, ns, n)]
    return res[0] if single else res


def _feature_host(entry: str, pcm, hz: int, opts, size):
    """A host entry into a sized byte buffer: `entry`(pcm, n, hz, *opts, out, size(n)) over float64 samples; the
    bytes."""
    import numpy as np

    a = np.ascontiguousarray(pcm, dtype=np.float64)
    nby = size(a.size)
    out = np.empty(max(1, nby), dtype=np.uint8)
    check(getattr(lib(), entry)(a.ctypes.data, a.size, hz, *[C.byref(o) for o in opts], out.ctypes.data, nby))
    return out[:nby].tobytes()


def loudness(pcms, hz: int, device: int = -1):
    """jb_loudness_pcm_batch: (lufs, peak_dbfs) of each float64 array of `pcms` (or of one array) at hz, on the GPU."""
    import numpy as np

    single = isinstance(pcms, np.ndarray)
    arrs, n, ins, nin = _pcm_args([pcms] if single else pcms, np.float64)
    dp = C.POINTER(C.c_double)
    lufs, peak = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    check(lib().jb_loudness_pcm_batch(ins, nin, n, hz, device, lufs.ctypes.data_as(dp), peak.ctypes.data_as(dp)))
    res = [(float(lufs[u]), float(peak[u])) for u in range(n)]
    return res[0] if single else res


def _group_ids(group, n):
    """A ctypes array of n group ids: None entries (or group None) are JB_LOUDNESS_NO_GROUP."""
    ids = [LOUDNESS_NO_GROUP] * n if group is None else [LOUDNESS_NO_GROUP if g is None else int(g) for g in group]
    if len(ids) != n:
        raise ValueError("one group per utterance")
    return (C.c_uint32 * max(n, 1))(*ids)


def loudness_groups(pcms, hz: int, group=None, device: int = -1, mode: int = 0, target=float("nan"),
                    ceiling=float("inf")):
    """jb_loudness_groups_pcm_batch: the float64 arrays of `pcms` at hz, measured on the GPU in the groups of `group`
    (ids below len(pcms); None = an utterance of its own).  Returns a dict: group_of (the dense group of each
    utterance), groups (a dict per group: lufs, sample_peak_dbfs, true_peak_dbtp, gain_db, peak_mode, oversampling,
    members, flags, r128), r128 (a dict per utterance) and lufs (each utterance's own L)."""
    import numpy as np

    arrs, n, ins, nin = _pcm_args(pcms, np.float64)
    dp = C.POINTER(C.c_double)
    ids = _group_ids(group, n)
    of = (C.c_uint32 * max(n, 1))()
    reps = (LoudnessGroupReport * max(n, 1))()
    r128 = (LoudnessR128 * max(n, 1))()
    lufs = np.zeros(max(n, 1))
    ng = C.c_size_t()
    check(lib().jb_loudness_groups_pcm_batch(ins, nin, n, ids, hz, device, mode, float(target), float(ceiling), of,
                                             reps, n, C.byref(ng), r128, lufs.ctypes.data_as(dp)))
    return {"group_of": [int(of[u]) for u in range(n)], "groups": [_struct_dict(reps[g]) for g in range(ng.value)],
            "r128": [_struct_dict(r128[u]) for u in range(n)], "lufs": [float(lufs[u]) for u in range(n)]}


def loudness_gate_host(z, hop: int, peak, true_peak=None, target=float("nan"), ceiling=float("inf")):
    """jb_loudness_gate_host (host only): the group rules on hop energies the caller holds.  z: one float64 array of
    hop energies per member; peak / true_peak: their largest magnitudes in 16-bit units.  Returns (group, members):
    the set's report as a dict (r128 included) and each member's own R128 fields."""
    import numpy as np

    zs = [np.ascontiguousarray(a, dtype=np.float64) for a in z]
    n = len(zs)
    dp = C.POINTER(C.c_double)
    zp = (dp * max(n, 1))(*[a.ctypes.data_as(dp) for a in zs])
    nh = (C.c_size_t * max(n, 1))(*[a.size for a in zs])
    pk = np.ascontiguousarray(peak, dtype=np.float64)
    tp = None if true_peak is None else np.ascontiguousarray(true_peak, dtype=np.float64)
    rep = LoudnessGroupReport()
    mr = (LoudnessR128 * max(n, 1))()
    check(lib().jb_loudness_gate_host(zp, nh, n, hop, pk.ctypes.data_as(dp),
                                      None if tp is None else tp.ctypes.data_as(dp), float(target), float(ceiling),
                                      C.byref(rep), mr))
    return _struct_dict(rep), [_struct_dict(mr[m]) for m in range(n)]


def true_peak_filter(hz: int):
    """The library's true-peak interpolator at hz (include/jbonsai_amd.h jb_true_peak_filter; host only): (F, taps)
    with taps a float64 array [F - 1][12], the phases 1..F-1."""
    import numpy as np

    L = lib()
    f, nt = C.c_uint32(), C.c_uint32()
    check(L.jb_true_peak_filter(hz, C.byref(f), C.byref(nt), None, 0))
    taps = np.zeros((f.value - 1, nt.value), dtype=np.float64)
    check(L.jb_true_peak_filter(hz, C.byref(f), C.byref(nt), taps.ctypes.data_as(C.POINTER(C.c_double)), taps.size))
    return f.value, taps


def true_peak(pcms, hz: int, device: int = -1):
    """jb_true_peak_pcm_batch: the true peak (dBTP) of each float64 array of `pcms` (or of one array) at hz, on the
    GPU."""
    import numpy as np

    single = isinstance(pcms, np.ndarray)
    arrs, n, ins, nin = _pcm_args([pcms] if single else pcms, np.float64)
    dp = C.POINTER(C.c_double)
    tp = np.zeros(max(n, 1))
    check(lib().jb_true_peak_pcm_batch(ins, nin, n, hz, device, tp.ctypes.data_as(dp)))
    res = [float(tp[u]) for u in range(n)]
    return res[0] if single else res


def take_flac(L, bufs, ns, n):
    """bytes of n library-owned FLAC streams, each released with jb_flac_free."""
    return _take(L.jb_flac_free, bufs, ns, n)


def flac_encode(pcms, hz: int, block_size: int = 0, max_lpc_order=None, device: int = -1, md5: bool = False,
                seek_interval_ms: int = 0):
    """jb_flac_encode_pcm_batch[_meta]: one FLAC stream (bytes) per int16 array of `pcms` at hz, encoded on the GPU;
    md5: the samples' MD5 in STREAMINFO; seek_interval_ms > 0: a SEEKTABLE with a point about that often."""
    import numpy as np

    arrs, n, ins, nin = _pcm_args(pcms, np.int16)
    L = lib()
    u8p = C.POINTER(C.c_uint8)
    bufs, ns = (u8p * max(n, 1))(), (C.c_size_t * max(n, 1))()
    opts, meta = flac_opts(block_size, max_lpc_order), flac_meta(md5, seek_interval_ms)
    if meta is None:
        check(L.jb_flac_encode_pcm_batch(ins, nin, n, hz, C.byref(opts), device, bufs, ns))
    else:
        check(L.jb_flac_encode_pcm_batch_meta(ins, nin, n, hz, C.byref(opts), C.byref(meta), device, bufs, ns))
    return take_flac(L, bufs, ns, n)


def flac_md5(pcms, device: int = -1):
    """jb_flac_md5_pcm_batch: the MD5 digest (16 bytes) of each int16 array of `pcms` as little-endian bytes, on the
    GPU."""
    import numpy as np

    arrs, n, ins, nin = _pcm_args(pcms, np.int16)
    out = C.create_string_buffer(16 * max(n, 1))
    check(lib().jb_flac_md5_pcm_batch(ins, nin, n, device, C.cast(out, C.c_void_p)))
    return [out.raw[16 * u:16 * u + 16] for u in range(n)]


def md5_host(data) -> bytes:
    """jb_md5_host: MD5 (RFC 1321) of bytes in plain C++ on the host (no GPU)."""
    data = bytes(data)
    buf = C.create_string_buffer(data, max(1, len(data)))
    out = C.create_string_buffer(16)
    check(lib().jb_md5_host(C.cast(buf, C.c_void_p), len(data), C.cast(out, C.c_void_p)))
    return out.raw


def flac_seek_geometry(n_samples: int, block_size: int, hz: int, seek_interval_ms: int):
    """jb_flac_seek_geometry: (frames between two seek points, points, bytes in front of the first frame) of a
    stream (host only)."""
    step, pts, hdr = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().jb_flac_seek_geometry(n_samples, block_size, hz, seek_interval_ms, C.byref(step), C.byref(pts),
                                      C.byref(hdr)))
    return step.value, pts.value, hdr.value


def take_formatted(L, bufs, ns, n):
    """bytes of n library-owned formatted outputs, each released with jb_format_free."""
    return _take(L.jb_format_free, bufs, ns, n)


def format_pcm(pcms, fmt, dither=False, seed: int = 0, device: int = -1):
    """jb_format_pcm_batch: the bytes of each float64 array of `pcms` (or of one array) in the sample format, on the
    GPU."""
    import numpy as np

    single = isinstance(pcms, np.ndarray)
    arrs, n, ins, nin = _pcm_args([pcms] if single else pcms, np.float64)
    L = lib()
    u8p = C.POINTER(C.c_uint8)
    bufs, ns = (u8p * max(n, 1))(), (C.c_size_t * max(n, 1))()
    opts = format_opts(fmt, dither, seed)
    check(L.jb_format_pcm_batch(ins, nin, n, C.byref(opts), device, bufs, ns))
    res = take_formatted(L, bufs, ns, n)
    return res[0] if single else res


def format_pcm_host(pcm, fmt, dither=False, seed: int = 0) -> bytes:
    """jb_format_pcm_host: the same rules in plain C++ on the host (no GPU)."""
    import numpy as np

    a = np.ascontiguousarray(pcm, dtype=np.float64)
    opts = format_opts(fmt, dither, seed)
    L = lib()
    out = np.empty(max(1, a.size * L.jb_format_bytes_per_sample(opts.format)), dtype=np.uint8)
    check(L.jb_format_pcm_host(a.ctypes.data, a.size, C.byref(opts), out.ctypes.data, out.size))
    return out[:a.size * L.jb_format_bytes_per_sample(opts.format)].tobytes()


def write_wav_formatted(path, data: bytes, sampling_frequency: int, fmt) -> None:
    """jb_write_wav_formatted: a mono WAV file of formatted bytes (format tag 1, 3, 7 or 6 by the format)."""
    f = FORMATS[fmt] if isinstance(fmt, str) else int(fmt)
    L = lib()
    nb = L.jb_format_bytes_per_sample(f)
    if nb and len(data) % nb:
        raise ValueError("the bytes are no whole number of samples")
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    check(L.jb_write_wav_formatted(str(path).encode(), C.cast(buf, C.c_void_p), len(data) // nb if nb else 0,
                                   sampling_frequency, f))


class AdpcmStream(collections.namedtuple("AdpcmStream", "data n_samples hz block_align")):
    """One utterance as IMA ADPCM: its blocks, the samples they encode, its rate and its block size."""

    def write_wav(self, path) -> None:
        write_wav_adpcm(path, self.data, self.n_samples, self.hz, self.block_align)

    def decode(self):
        return adpcm_decode_host(self.data, self.block_align, self.n_samples)


def adpcm_streams(L, bufs, ns, nsamp, rates, block_align, n):
    """AdpcmStream of n library-owned outputs at their rates (released here)."""
    datas = take_adpcm(L, bufs, ns, n)
    return [AdpcmStream(datas[u], nsamp[u], rates[u], adpcm_geometry(rates[u], 0, block_align)[0]) for u in range(n)]


def take_adpcm(L, bufs, ns, n):
    """bytes of n library-owned ADPCM outputs, each released with jb_adpcm_free."""
    return _take(L.jb_adpcm_free, bufs, ns, n)


def adpcm_geometry(hz: int, n: int, block_align: int = 0):
    """jb_adpcm_geometry: (A, samples per block, blocks, bytes) of n samples at hz."""
    A, spb, nb, nby = C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_size_t()
    check(lib().jb_adpcm_geometry(hz, block_align, n, C.byref(A), C.byref(spb), C.byref(nb), C.byref(nby)))
    return A.value, spb.value, nb.value, nby.value


def adpcm_encode_host(pcm, hz: int, block_align: int = 0) -> bytes:
    """jb_adpcm_encode_host / jb_adpcm_encode_i16_host (by the array's dtype): IMA ADPCM blocks of float64 samples in
    16-bit scale, or of int16 samples, in plain C++ on the host (no GPU)."""
    import numpy as np

    a = np.ascontiguousarray(pcm)
    i16 = a.dtype == np.int16
    if not i16:
        a = np.ascontiguousarray(a, dtype=np.float64)
    L = lib()
    opts = adpcm_opts(block_align)
    nby = adpcm_geometry(hz, a.size, block_align)[3]
    out = np.empty(max(1, nby), dtype=np.uint8)
    fn = L.jb_adpcm_encode_i16_host if i16 else L.jb_adpcm_encode_host
    check(fn(a.ctypes.data, a.size, hz, C.byref(opts), out.ctypes.data, nby))
    return out[:nby].tobytes()


def adpcm_decode_host(data: bytes, block_align: int, n_samples: int):
    """jb_adpcm_decode_host: the first n_samples int16 samples of IMA ADPCM blocks of block_align bytes."""
    import numpy as np

    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(max(1, n_samples), dtype=np.int16)
    check(lib().jb_adpcm_decode_host(buf.ctypes.data if buf.size else None, buf.size, block_align, n_samples,
                                     out.ctypes.data, n_samples))
    return out[:n_samples]


def adpcm_encode(pcms, hz, block_align: int = 0, device: int = -1):
    """jb_adpcm_encode_pcm_batch: the IMA ADPCM blocks of each float64 array of `pcms` (or of one array) on the GPU;
    hz: one rate, or one per array."""
    import numpy as np

    single = isinstance(pcms, np.ndarray)
    arrs, n, ins, nin = _pcm_args([pcms] if single else pcms, np.float64)
    rates = [int(hz)] * n if np.isscalar(hz) else [int(h) for h in hz]
    if len(rates) != n:
        raise ValueError("give one rate, or one per array")
    L = lib()
    u8p = C.POINTER(C.c_uint8)
    hzs = (C.c_uint32 * max(n, 1))(*rates)
    bufs, ns = (u8p * max(n, 1))(), (C.c_size_t * max(n, 1))()
    opts = adpcm_opts(block_align)
    check(L.jb_adpcm_encode_pcm_batch(ins, nin, n, hzs, C.byref(opts), device, bufs, ns))
    res = take_adpcm(L, bufs, ns, n)
    return res[0] if single else res


def fbank_geometry(hz: int, opts: FbankOpts, n: int = 0):
    """jb_fbank_geometry: (wl, hop, n_fft, T, bytes) of n samples at hz."""
    wl, hop, nfft, T, nby = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_size_t()
    check(lib().jb_fbank_geometry(hz, C.byref(opts), n, C.byref(wl), C.byref(hop), C.byref(nfft), C.byref(T),
                                  C.byref(nby)))
    return wl.value, hop.value, nfft.value, T.value, nby.value


def fbank_window(hz: int, opts: FbankOpts):
    """jb_fbank_window: the wl window values the options give at hz."""
    import numpy as np

    w = np.empty(fbank_geometry(hz, opts)[0], dtype=np.float64)
    check(lib().jb_fbank_window(hz, C.byref(opts), w.ctypes.data, w.size))
    return w


def fbank_filterbank(hz: int, opts: FbankOpts):
    """jb_fbank_filterbank: the mel weights [n_mels, n_fft / 2 + 1] the options give at hz."""
    import numpy as np

    W = np.empty((opts.n_mels, fbank_geometry(hz, opts)[2] // 2 + 1), dtype=np.float64)
    check(lib().jb_fbank_filterbank(hz, C.byref(opts), W.ctypes.data, W.size))
    return W


def fbank_frames(data: bytes, opts: FbankOpts):
    """The bytes of a unit's features as an ndarray [T, n_mels]."""
    import numpy as np

    return np.frombuffer(data, dtype=opts.dtype).reshape(-1, opts.n_mels).copy()


def take_fbank(L, bufs, ns, n, opts: FbankOpts):
    """ndarrays [T, n_mels] of n library-owned outputs, each released with jb_fbank_free."""
    return [fbank_frames(d, opts) for d in _take(L.jb_fbank_free, bufs, ns, n)]


def fbank_host(pcm, hz: int, opts: FbankOpts):
    """jb_fbank_host: the features [T, n_mels] of float64 samples in 16-bit scale, in plain C++ on the host (no GPU)."""
    return fbank_frames(_feature_host("jb_fbank_host", pcm, hz, (opts,), lambda n: fbank_geometry(hz, opts, n)[4]),
                        opts)



def fbank_pcm(pcms, hz, opts: FbankOpts, device: int = -1):
    """jb_fbank_pcm_batch: the features [T, n_mels] of each float64 array of `pcms` (or of one array) on the GPU; hz:
    one rate, or one per array."""
    return _feature_pcm("jb_fbank_pcm_batch", "jb_fbank_free", pcms, hz, (opts,), device,
                        lambda d: fbank_frames(d, opts))



def fbank_framed_geometry(hz: int, opts: FbankOpts, fr: FrameOpts, n: int = 0):
    """jb_fbank_framed_geometry: (wl, hop, n_fft, T, bytes) of n samples at hz under the frame request."""
    wl, hop, nfft, T, nby = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_size_t()
    check(lib().jb_fbank_framed_geometry(hz, C.byref(opts), C.byref(fr), n, C.byref(wl), C.byref(hop), C.byref(nfft),
                                         C.byref(T), C.byref(nby)))
    return wl.value, hop.value, nfft.value, T.value, nby.value


def frame_window(hz: int, opts: FbankOpts, fr: FrameOpts):
    """jb_frame_window: the wl window values of a conditioned frame at hz."""
    import numpy as np

    w = np.empty(fbank_geometry(hz, opts)[0], dtype=np.float64)
    check(lib().jb_frame_window(hz, C.byref(opts), C.byref(fr), w.ctypes.data, w.size))
    return w


def fbank_framed_host(pcm, hz: int, opts: FbankOpts, fr: FrameOpts):
    """jb_fbank_framed_host: fbank_host under the frame request (no GPU)."""
    return fbank_frames(_feature_host("jb_fbank_framed_host", pcm, hz, (opts, fr),
                                      lambda n: fbank_framed_geometry(hz, opts, fr, n)[4]), opts)



def fbank_framed_pcm(pcms, hz, opts: FbankOpts, fr: FrameOpts, device: int = -1):
    """jb_fbank_framed_pcm_batch: fbank_pcm under the frame request, on the GPU."""
    return _feature_pcm("jb_fbank_framed_pcm_batch", "jb_fbank_free", pcms, hz, (opts, fr), device,
                        lambda d: fbank_frames(d, opts))



def melspec_geometry(hz: int, opts: MelspecOpts, n: int = 0):
    """jb_melspec_geometry: (n_fft, win_length, hop_length, T, bytes) of n samples at hz."""
    nfft, wl, hop, T, nby = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_size_t()
    check(lib().jb_melspec_geometry(hz, C.byref(opts), n, C.byref(nfft), C.byref(wl), C.byref(hop), C.byref(T),
                                    C.byref(nby)))
    return nfft.value, wl.value, hop.value, T.value, nby.value


def melspec_window(hz: int, opts: MelspecOpts):
    """jb_melspec_window: the n_fft window values a frame is multiplied by (the Hann window centred, zeros around it)."""
    import numpy as np

    w = np.empty(melspec_geometry(hz, opts)[0], dtype=np.float64)
    check(lib().jb_melspec_window(hz, C.byref(opts), w.ctypes.data, w.size))
    return w


def melspec_filterbank(hz: int, opts: MelspecOpts):
    """jb_melspec_filterbank: the mel weights [n_mels, n_fft / 2 + 1] the options give at hz."""
    import numpy as np

    W = np.empty((opts.n_mels, melspec_geometry(hz, opts)[0] // 2 + 1), dtype=np.float64)
    check(lib().jb_melspec_filterbank(hz, C.byref(opts), W.ctypes.data, W.size))
    return W


def melspec_frames(data: bytes, opts: MelspecOpts):
    """The bytes of a unit's mel spectrogram as an ndarray [T, n_mels]."""
    import numpy as np

    return np.frombuffer(data, dtype=opts.dtype).reshape(-1, opts.n_mels).copy()


def take_melspec(L, bufs, ns, n, opts: MelspecOpts):
    """ndarrays [T, n_mels] of n library-owned outputs, each released with jb_melspec_free."""
    return [melspec_frames(d, opts) for d in _take(L.jb_melspec_free, bufs, ns, n)]


def melspec_host(pcm, hz: int, opts: MelspecOpts):
    """jb_melspec_host: the mel spectrogram [T, n_mels] of float64 samples in 16-bit scale, in plain C++ on the host
    (no GPU)."""
    return melspec_frames(_feature_host("jb_melspec_host", pcm, hz, (opts,),
                                        lambda n: melspec_geometry(hz, opts, n)[4]), opts)



def melspec_pcm(pcms, hz, opts: MelspecOpts, device: int = -1):
    """jb_melspec_pcm_batch: the mel spectrogram [T, n_mels] of each float64 array of `pcms` (or of one array) on the
    GPU; hz: one rate, or one per array."""
    return _feature_pcm("jb_melspec_pcm_batch", "jb_melspec_free", pcms, hz, (opts,), device,
                        lambda d: melspec_frames(d, opts))



def mfcc_geometry(hz: int, fopts: FbankOpts, opts: MfccOpts, n: int = 0):
    """jb_mfcc_geometry: (T, width, bytes) of n samples at hz."""
    T, w, nby = C.c_size_t(), C.c_uint32(), C.c_size_t()
    check(lib().jb_mfcc_geometry(hz, C.byref(fopts), C.byref(opts), n, C.byref(T), C.byref(w), C.byref(nby)))
    return T.value, w.value, nby.value


def mfcc_dct(n_mels: int, opts: MfccOpts):
    """jb_mfcc_dct: (D [n_ceps, n_mels], lifter [n_ceps]) of the options behind n_mels filters."""
    import numpy as np

    D, l = np.empty((opts.n_ceps, n_mels), dtype=np.float64), np.empty(opts.n_ceps, dtype=np.float64)
    check(lib().jb_mfcc_dct(n_mels, C.byref(opts), D.ctypes.data, D.size, l.ctypes.data, l.size))
    return D, l


def mfcc_delta_kernel(order: int, window: int):
    """jb_mfcc_delta_kernel: s_order[-order * window .. order * window]."""
    import numpy as np

    s = np.empty(2 * max(order, 0) * max(window, 0) + 1, dtype=np.float64)
    check(lib().jb_mfcc_delta_kernel(order, window, s.ctypes.data, s.size))
    return s


def mfcc_rows(data: bytes, opts: MfccOpts, n_mels: int):
    """The bytes of a unit's rows as an ndarray [T, width]."""
    import numpy as np

    return np.frombuffer(data, dtype=opts.dtype).reshape(-1, opts.width(n_mels)).copy()


def take_mfcc(L, bufs, ns, n, opts: MfccOpts, n_mels: int):
    """ndarrays [T, width] of n library-owned outputs, each released with jb_mfcc_free."""
    return [mfcc_rows(d, opts, n_mels) for d in _take(L.jb_mfcc_free, bufs, ns, n)]


def mfcc_request(opts, fbank_opts, kw):
    """(FbankOpts, MfccOpts) of a call that takes `opts` (MfccOpts, or None with the keywords of J.mfcc in kw) and
    `fbank` (FbankOpts, a dict of J.fbank's keywords, or None: the defaults)."""
    fo = fbank_opts if isinstance(fbank_opts, FbankOpts) else fbank(**(fbank_opts or {}))
    return fo, (opts if opts is not None else mfcc(**kw))


def mfcc_host(logmel, opts: MfccOpts):
    """jb_mfcc_host: the rows [T, width] of float64 log-mel frames [T, n_mels], in plain C++ on the host (no GPU)."""
    import numpy as np

    a = np.ascontiguousarray(logmel, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("log-mel frames are [T, n_mels]")
    T, n_mels = a.shape
    nby = T * opts.width(n_mels) * opts.dtype.itemsize
    out = np.empty(max(1, nby), dtype=np.uint8)
    check(lib().jb_mfcc_host(a.ctypes.data, T, n_mels, C.byref(opts), out.ctypes.data, nby))
    return mfcc_rows(out[:nby].tobytes(), opts, n_mels)


def mfcc_pcm_host(pcm, hz: int, fopts: FbankOpts, opts: MfccOpts):
    """jb_mfcc_pcm_host: the rows [T, width] of float64 samples in 16-bit scale, on the host (no GPU)."""
    return mfcc_rows(_feature_host("jb_mfcc_pcm_host", pcm, hz, (fopts, opts),
                                   lambda n: mfcc_geometry(hz, fopts, opts, n)[2]), opts, fopts.n_mels)



def mfcc_frames(logmels, opts: MfccOpts, device: int = -1):
    """jb_mfcc_frames_batch: the rows [T, width] of each float64 array [T, n_mels] of `logmels` (or of one array) on
    the GPU."""
    import numpy as np

    single = isinstance(logmels, np.ndarray)
    units = [np.ascontiguousarray(a, dtype=np.float64) for a in ([logmels] if single else logmels)]
    if any(a.ndim != 2 for a in units) or len({a.shape[1] for a in units}) > 1:
        raise ValueError("log-mel frames are [T, n_mels], with one n_mels for all")
    n_mels = units[0].shape[1] if units else 1
    arrs, n, ins, _ = _pcm_args(units, np.float64)
    L = lib()
    u8p = C.POINTER(C.c_uint8)
    Ts = (C.c_size_t * max(n, 1))(*[a.shape[0] for a in units])
    bufs, ns = (u8p * max(n, 1))(), (C.c_size_t * max(n, 1))()
    check(L.jb_mfcc_frames_batch(ins, Ts, n, n_mels, C.byref(opts), device, bufs, ns))
    res = [mfcc_rows(d, opts, n_mels) for d in _take(L.jb_mfcc_free, bufs, ns, n)]
    return res[0] if single else res


def mfcc_pcm(pcms, hz, fopts: FbankOpts, opts: MfccOpts, device: int = -1):
    """jb_mfcc_pcm_batch: the rows [T, width] of each float64 array of `pcms` (or of one array) on the GPU; hz: one
    rate, or one per array."""
    return _feature_pcm("jb_mfcc_pcm_batch", "jb_mfcc_free", pcms, hz, (fopts, opts), device,
                        lambda d: mfcc_rows(d, opts, fopts.n_mels))



def mfcc_framed_pcm_host(pcm, hz: int, fopts: FbankOpts, opts: MfccOpts, fr: FrameOpts):
    """jb_mfcc_framed_pcm_host: mfcc_pcm_host under the frame request (no GPU)."""
    def size(n):
        return fbank_framed_geometry(hz, fopts, fr, n)[3] * opts.width(fopts.n_mels) * opts.dtype.itemsize

    return mfcc_rows(_feature_host("jb_mfcc_framed_pcm_host", pcm, hz, (fopts, opts, fr), size), opts, fopts.n_mels)



def mfcc_framed_pcm(pcms, hz, fopts: FbankOpts, opts: MfccOpts, fr: FrameOpts, device: int = -1):
    """jb_mfcc_framed_pcm_batch: mfcc_pcm under the frame request, on the GPU."""
    return _feature_pcm("jb_mfcc_framed_pcm_batch", "jb_mfcc_free", pcms, hz, (fopts, opts, fr), device,
                        lambda d: mfcc_rows(d, opts, fopts.n_mels))



def write_wav_adpcm(path, data: bytes, n_samples: int, sampling_frequency: int, block_align: int) -> None:
    """jb_write_wav_adpcm: a mono WAV file (format tag 0x11) of IMA ADPCM blocks."""
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    check(lib().jb_write_wav_adpcm(str(path).encode(), C.cast(buf, C.c_void_p), len(data), n_samples,
                                   sampling_frequency, block_align))


def join_ms_to_samples(ms: float, hz: int) -> int:
    """jb_join_ms_to_samples: floor(ms * hz / 1000.0 + 0.5)."""
    return int(lib().jb_join_ms_to_samples(float(ms), int(hz)))


def join_geometry(req, lengths, hz=None):
    """jb_join_geometry: (programme_of [n], member_start [n], programme_samples [P]) of a request (join_request's
    forms) over members of `lengths` samples; hz: one rate per member to compare, or None."""
    n = len(lengths)
    arr = join_request(req)
    nin = (C.c_size_t * max(n, 1))(*[int(x) for x in lengths])
    hzs = None if hz is None else (C.c_uint32 * max(n, 1))(*[int(h) for h in hz])
    po, ms = (C.c_uint32 * max(n, 1))(), (C.c_uint64 * max(n, 1))()
    P, ps = C.c_size_t(), (C.c_uint64 * max(n, 1))()
    check(lib().jb_join_geometry(arr, nin, hzs, n, po, ms, C.byref(P), ps))
    return list(po[:n]), list(ms[:n]), list(ps[:P.value])


def _join_inputs(pcms):
    import numpy as np

    i16 = len(pcms) > 0 and all(np.asarray(a).dtype == np.int16 for a in pcms)
    return (i16,) + _pcm_args(pcms, np.int16 if i16 else np.float64, void=True)


def join_host(pcms, req):
    """jb_join_host / jb_join_i16_host (by the arrays' dtype): the programmes of the members `pcms` under the request
    `req`, in plain C++ on the host (no GPU).  Every output buffer holds exactly its programme's samples."""
    import numpy as np

    i16, arrs, n, ins, nin = _join_inputs(pcms)
    arr = join_request(req)
    _, _, ps = join_geometry(arr[:n], [a.size for a in arrs])
    outs = [np.empty(int(k), dtype=np.int16 if i16 else np.float64) for k in ps]
    P = len(outs)
    optr = (C.c_void_p * max(P, 1))(*[o.ctypes.data if o.size else None for o in outs])
    caps = (C.c_size_t * max(P, 1))(*[o.size for o in outs])
    L = lib()
    check((L.jb_join_i16_host if i16 else L.jb_join_host)(ins, nin, n, arr, optr, caps))
    return outs


def join_pcm(pcms, req, device: int = -1):
    """jb_join_pcm_batch / _i16 (by the arrays' dtype): the same programmes, joined on the GPU."""
    import numpy as np

    i16, arrs, n, ins, nin = _join_inputs(pcms)
    arr = join_request(req)
    outs, ns, P = (C.c_void_p * max(n, 1))(), (C.c_size_t * max(n, 1))(), C.c_size_t()
    L = lib()
    check((L.jb_join_pcm_batch_i16 if i16 else L.jb_join_pcm_batch)(ins, nin, n, arr, device, outs, ns, C.byref(P)))
    return _take(L.jb_join_free, outs, ns, P.value, np.int16 if i16 else np.float64)


def mix_gain(gain_db: float) -> float:
    """jb_mix_gain: 10^(gain_db / 20) formed in long double and rounded once; exactly 1 at 0 dB, 0 at -inf."""
    return float(lib().jb_mix_gain(float(gain_db)))


def mix_geometry(req, lengths, hz=None, opts=None):
    """jb_mix_geometry: (programme_of [n], member_start [n], programme_samples [P], depth [P], overlap [P]) of a
    request (mix_request's forms) over members of `lengths` samples; hz: one rate per member to compare, or None."""
    n = len(lengths)
    arr = mix_request(req)
    nin = (C.c_size_t * max(n, 1))(*[int(x) for x in lengths])
    hzs = None if hz is None else (C.c_uint32 * max(n, 1))(*[int(h) for h in hz])
    po, ms = (C.c_uint32 * max(n, 1))(), (C.c_uint64 * max(n, 1))()
    P, ps = C.c_size_t(), (C.c_uint64 * max(n, 1))()
    dp, ov = (C.c_uint32 * max(n, 1))(), (C.c_uint64 * max(n, 1))()
    check(lib().jb_mix_geometry(arr, nin, hzs, n, None if opts is None else C.byref(opts), po, ms, C.byref(P), ps,
                                dp, ov))
    return list(po[:n]), list(ms[:n]), list(ps[:P.value]), list(dp[:P.value]), list(ov[:P.value])


def mix_host(pcms, req, opts=None, scale=None):
    """jb_mix_host / jb_mix_i16_host (by the arrays' dtype): (programmes, reports) of the members `pcms` under the
    request `req` and the MixOpts `opts`, in plain C++ on the host (no GPU); scale: one given s per programme."""
    import numpy as np

    i16, arrs, n, ins, nin = _join_inputs(pcms)
    arr = mix_request(req)
    ps = mix_geometry(arr[:n], [a.size for a in arrs])[2]
    outs = [np.empty(int(k), dtype=np.int16 if i16 else np.float64) for k in ps]
    P = len(outs)
    optr = (C.c_void_p * max(P, 1))(*[o.ctypes.data if o.size else None for o in outs])
    caps = (C.c_size_t * max(P, 1))(*[o.size for o in outs])
    reps = (MixReport * max(P, 1))()
    sc = None if scale is None else (C.c_double * max(P, 1))(*[float(v) for v in scale])
    L = lib()
    check((L.jb_mix_i16_host if i16 else L.jb_mix_host)(ins, nin, n, arr, None if opts is None else C.byref(opts), sc,
                                                        optr, caps, reps))
    return outs, list(reps[:P])


def mix_pcm(pcms, req, opts=None, device: int = -1):
    """jb_mix_pcm_batch / _i16 (by the arrays' dtype): the same (programmes, reports), mixed on the GPU."""
    import numpy as np

    i16, arrs, n, ins, nin = _join_inputs(pcms)
    arr = mix_request(req)
    outs, ns, P = (C.c_void_p * max(n, 1))(), (C.c_size_t * max(n, 1))(), C.c_size_t()
    reps = (MixReport * max(n, 1))()
    L = lib()
    check((L.jb_mix_pcm_batch_i16 if i16 else L.jb_mix_pcm_batch)(ins, nin, n, arr,
                                                                  None if opts is None else C.byref(opts), device, outs,
                                                                  ns, C.byref(P), reps))
    return _take(L.jb_mix_free, outs, ns, P.value, np.int16 if i16 else np.float64), list(reps[:P.value])


def mix_stems_geometry(req, stem_of, lengths, hz=None, opts=None):
    """jb_mix_stems_geometry: a dict of P, the units' number U = P + S, stem_unit [n] (-1: none) and per unit
    samples, programme, stem_id (MIX_NO_STEM for a programme), members, first, end and depth."""
    n = len(lengths)
    arr, ids = mix_request(req), stem_ids(stem_of)
    nin = (C.c_size_t * max(n, 1))(*[int(x) for x in lengths])
    hzs = None if hz is None else (C.c_uint32 * max(n, 1))(*[int(h) for h in hz])
    m = max(2 * n, 1)
    P, U, su = C.c_size_t(), C.c_size_t(), (C.c_int64 * max(n, 1))()
    ns, fi, en = (C.c_uint64 * m)(), (C.c_uint64 * m)(), (C.c_uint64 * m)()
    pr, si, me, de = (C.c_uint32 * m)(), (C.c_uint32 * m)(), (C.c_uint32 * m)(), (C.c_uint32 * m)()
    check(lib().jb_mix_stems_geometry(arr, ids, nin, hzs, n, None if opts is None else C.byref(opts), C.byref(P),
                                      C.byref(U), su, ns, pr, si, me, fi, en, de))
    u = U.value
    return {"P": P.value, "U": u, "stem_unit": list(su[:n]), "samples": list(ns[:u]), "programme": list(pr[:u]),
            "stem_id": list(si[:u]), "members": list(me[:u]), "first": list(fi[:u]), "end": list(en[:u]),
            "depth": list(de[:u])}


def mix_stems_host(pcms, req, stem_of, opts=None, scale=None, levels: bool = False):
    """jb_mix_stems_host / _i16_host (by the arrays' dtype): (units, reports, stem_reports) -- the P programmes and the
    S stems behind them, the MixReports [P] and the StemReports [S] -- by the rule in plain C++ on the host."""
    import numpy as np

    i16, arrs, n, ins, nin = _join_inputs(pcms)
    arr, ids = mix_request(req), stem_ids(stem_of)
    g = mix_stems_geometry(arr[:n], stem_of, [a.size for a in arrs])
    outs = [np.empty(int(k), dtype=np.int16 if i16 else np.float64) for k in g["samples"]]
    U, P = len(outs), g["P"]
    optr = (C.c_void_p * max(U, 1))(*[o.ctypes.data if o.size else None for o in outs])
    caps = (C.c_size_t * max(U, 1))(*[o.size for o in outs])
    reps, sreps = (MixReport * max(P, 1))(), (StemReport * max(U - P, 1))()
    sc = None if scale is None else (C.c_double * max(P, 1))(*[float(v) for v in scale])
    L = lib()
    check((L.jb_mix_stems_i16_host if i16 else L.jb_mix_stems_host)(
        ins, nin, n, arr, ids, MIX_STEM_LEVELS * bool(levels), None if opts is None else C.byref(opts), sc, optr, caps,
        reps, sreps))
    return outs, list(reps[:P]), list(sreps[:U - P])


def mix_stems_pcm(pcms, req, stem_of, opts=None, levels: bool = False, device: int = -1):
    """jb_mix_stems_pcm_batch / _i16 (by the arrays' dtype): the same (units, reports, stem_reports), on the GPU."""
    import numpy as np

    i16, arrs, n, ins, nin = _join_inputs(pcms)
    arr, ids = mix_request(req), stem_ids(stem_of)
    m = max(2 * n, 1)
    outs, ns, P, U = (C.c_void_p * m)(), (C.c_size_t * m)(), C.c_size_t(), C.c_size_t()
    reps, sreps = (MixReport * max(n, 1))(), (StemReport * max(n, 1))()
    L = lib()
    check((L.jb_mix_stems_pcm_batch_i16 if i16 else L.jb_mix_stems_pcm_batch)(
        ins, nin, n, arr, ids, MIX_STEM_LEVELS * bool(levels), None if opts is None else C.byref(opts), device, outs, ns,
        C.byref(P), C.byref(U), reps, sreps))
    return (_take(L.jb_mix_free, outs, ns, U.value, np.int16 if i16 else np.float64), list(reps[:P.value]),
            list(sreps[:U.value - P.value]))


def mix_levels_host(stem, mix, first: int = 0, end=None):
    """jb_mix_levels_host / _i16_host (by the arrays' dtype): (E_s, D, E_p) of a stem and its mixture by the stage's
    summation order; [first, end): the stem's extent (default: the whole length)."""
    import numpy as np

    i16 = np.asarray(stem).dtype == np.int16
    a = np.ascontiguousarray(stem, dtype=np.int16 if i16 else np.float64)
    m = np.ascontiguousarray(mix, dtype=a.dtype)
    if a.size != m.size:
        raise ValueError("the stem and the mixture have one length")
    e, d, p = C.c_double(), C.c_double(), C.c_double()
    L = lib()
    check((L.jb_mix_levels_i16_host if i16 else L.jb_mix_levels_host)(
        a.ctypes.data if a.size else None, m.ctypes.data if m.size else None, a.size, int(first),
        a.size if end is None else int(end), C.byref(e), C.byref(d), C.byref(p)))
    return e.value, d.value, p.value


def mix_levels_db(e_s: float, d: float, e_p: float):
    """jb_mix_levels_db: (level_db, sir_db, si_sdr_db) of the three sums, formed in long double."""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    lib().jb_mix_levels_db(float(e_s), float(d), float(e_p), C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def activity_geometry(opts, hz: int, n: int):
    """jb_activity_geometry: (wl, hop, T) of a unit of n samples at hz under the ActivityOpts `opts`."""
    wl, hop, T = C.c_uint32(), C.c_uint32(), C.c_uint64()
    check(lib().jb_activity_geometry(C.byref(opts), int(hz), int(n), C.byref(wl), C.byref(hop), C.byref(T)))
    return wl.value, hop.value, T.value


def activity_host(pcm, hz: int, opts):
    """jb_activity_host: (labels [T] uint8, ActivityReport) of one column over the float64 samples `pcm`, in plain C++
    on the host (no GPU)."""
    import numpy as np

    a = np.ascontiguousarray(pcm, dtype=np.float64)
    T = activity_geometry(opts, hz, a.size)[2]
    out = np.zeros(max(T, 1), dtype=np.uint8)
    rep = ActivityReport()
    check(lib().jb_activity_host(a.ctypes.data, a.size, int(hz), C.byref(opts), out.ctypes.data, T, C.byref(rep)))
    return out[:T].copy(), rep


def activity_members_host(pcms, starts, n_unit: int, hz: int, opts, gain_db=None):
    """jb_activity_members_host: (labels [T][m] uint8, [ActivityReport] * m, ActivityUnitReport) of a unit of n_unit
    samples from its members `pcms` (float64) at `starts`; gain_db: one per member, -inf mutes."""
    import numpy as np

    arrs, m, ins, nin = _pcm_args(pcms, np.float64, void=True)
    st = (C.c_uint64 * max(m, 1))(*[int(v) for v in starts])
    gd = None if gain_db is None else (C.c_double * max(m, 1))(*[float(g) for g in gain_db])
    T = activity_geometry(opts, hz, int(n_unit))[2]
    out = np.zeros(max(T * m, 1), dtype=np.uint8)
    reps, unit = (ActivityReport * max(m, 1))(), ActivityUnitReport()
    check(lib().jb_activity_members_host(ins, nin, st, gd, m, int(n_unit), int(hz), C.byref(opts), out.ctypes.data, T * m,
                                         reps, C.byref(unit)))
    return out[:T * m].reshape(T, m).copy(), list(reps[:m]), unit


def activity_pcm(pcms, hz, opts, req=None, mix=None, device: int = -1):
    """jb_activity_pcm_batch / _i16 (by the arrays' dtype): the labels of caller-held PCM, measured on the GPU.  req: a
    mix request (mix_request's forms) that makes programmes of the utterances, or None: every utterance a unit of its
    own; mix: the MixOpts of the mixture that columns="unit" is measured on; hz: one rate, or one per array.
    ([labels [T][C] uint8 per unit], [[ActivityReport] * C per unit], [ActivityUnitReport per unit])."""
    import numpy as np

    i16, arrs, n, ins, nin = _join_inputs(pcms)
    rates = [int(hz)] * n if np.isscalar(hz) else [int(h) for h in hz]
    if len(rates) != n:
        raise ValueError("give one rate, or one per array")
    hzs = (C.c_uint32 * max(n, 1))(*rates)
    arr = None if req is None else mix_request(req)
    outs, Ts, Cs, P = (C.c_void_p * max(n, 1))(), (C.c_uint64 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), C.c_size_t()
    reps, units = (ActivityReport * max(n, 1))(), (ActivityUnitReport * max(n, 1))()
    L = lib()
    check((L.jb_activity_pcm_batch_i16 if i16 else L.jb_activity_pcm_batch)(
        ins, nin, n, arr, None if mix is None else C.byref(mix), hzs, C.byref(opts), device, outs, Ts, Cs, C.byref(P),
        reps, units))
    sizes = [int(Ts[p]) * int(Cs[p]) for p in range(P.value)]
    flat = _take(L.jb_activity_free, outs, sizes, P.value, np.uint8)
    labels, cols, k = [], [], 0
    for p in range(P.value):
        labels.append(flat[p].reshape(int(Ts[p]), int(Cs[p])))
        cols.append(list(reps[k:k + int(Cs[p])]))
        k += int(Cs[p])
    return labels, cols, list(units[:P.value])


def pitch_frames(data: bytes, opts):
    """The rows [T][width] of a pitch sink's bytes under the PitchOpts `opts`."""
    import numpy as np

    width = 2 if opts.flags & PITCH_RAW else 4 if opts.flags & PITCH_RAW_LOG else 3
    return np.frombuffer(data, dtype=np.float64 if opts.flags & PITCH_F64 else np.float32).reshape(-1, width).copy()


def take_pitch(L, bufs, ns, n, opts):
    """ndarrays [T, width] of n library-owned outputs, each released with jb_pitch_free."""
    return [pitch_frames(d, opts) for d in _take(L.jb_pitch_free, bufs, ns, n)]


def pitch_geometry(opts, hz: int, n: int):
    """jb_pitch_geometry: the PitchGeometry of a unit of n samples at hz under the PitchOpts `opts`."""
    g = PitchGeometry()
    check(lib().jb_pitch_geometry(C.byref(opts), int(hz), int(n), C.byref(g)))
    return g


def pitch_lags(opts):
    """jb_pitch_lags: the lags of the grid in seconds, a float64 array [S]."""
    import numpy as np

    S = C.c_size_t()
    check(lib().jb_pitch_lags(C.byref(opts), None, 0, C.byref(S)))
    out = np.zeros(S.value, dtype=np.float64)
    check(lib().jb_pitch_lags(C.byref(opts), out.ctypes.data, out.size, None))
    return out


def pitch_host(pcm, hz: int, opts, grid: bool = False):
    """jb_pitch_host: (rows [T][width], lag_index [T] uint32) of the float64 samples `pcm`, in plain C++ on the host (no
    GPU); with grid=True also (Q, p), each [T][S]: the two NCCFs over the lag grid."""
    import numpy as np

    a = np.ascontiguousarray(pcm, dtype=np.float64)
    g = pitch_geometry(opts, hz, a.size)
    T = int(g.T)
    out = np.zeros((T, g.width), dtype=np.float64 if g.elem == 8 else np.float32)
    idx = np.zeros(T, dtype=np.uint32)
    Q = np.zeros((T, g.S) if grid else (0, g.S), dtype=np.float64)
    P = np.zeros_like(Q)
    check(lib().jb_pitch_host(a.ctypes.data if a.size else None, a.size, int(hz), C.byref(opts),
                              out.ctypes.data if T else None, out.nbytes, idx.ctypes.data if T else None,
                              Q.ctypes.data if grid and T else None, P.ctypes.data if grid and T else None))
    return (out, idx, Q, P) if grid else (out, idx)


def pitch_pcm(pcms, hz, opts, device: int = -1):
    """jb_pitch_pcm_batch: the pitch rows of caller-held float64 PCM, tracked on the GPU; hz: one rate, or one per array.
    ([rows [T][width] per unit], [lag_index [T] uint32 per unit])."""
    import numpy as np

    arrs, n, ins, nin = _pcm_args(pcms, np.float64, void=True)
    rates = [int(hz)] * n if np.isscalar(hz) else [int(h) for h in hz]
    if len(rates) != n:
        raise ValueError("give one rate, or one per array")
    hzs = (C.c_uint32 * max(n, 1))(*rates)
    outs, lags = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
    Ts, Ws = (C.c_uint64 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
    L = lib()
    check(L.jb_pitch_pcm_batch(ins, nin, n, hzs, C.byref(opts), device, outs, Ts, Ws, lags))
    dtype = np.float64 if opts.flags & PITCH_F64 else np.float32
    flat = _take(L.jb_pitch_free, outs, [int(Ts[u]) * int(Ws[u]) for u in range(n)], n, dtype)
    idx = _take(L.jb_pitch_free, lags, [int(Ts[u]) for u in range(n)], n, np.uint32)
    return [flat[u].reshape(int(Ts[u]), int(Ws[u])) for u in range(n)], idx


def _biquads(arr, n):
    import numpy as np
    return np.array([[arr[i].b0, arr[i].b1, arr[i].b2, arr[i].a1, arr[i].a2] for i in range(n)],
                    dtype=np.float64).reshape(n, 5)


def filter_design(f, hz: int):
    """jb_filter_design: the coefficients [n_sections, 5] (b0 b1 b2 a1 a2, a0 = 1) of Filter `f` at `hz`."""
    out = (Biquad * FILTER_MAX_SECTIONS)()
    check(lib().jb_filter_design(C.byref(f), int(hz), out))
    return _biquads(out, f.n_sections)


def filter_sos(f, hz: int):
    """The same as rows of b0 b1 b2 1 a1 a2, as scipy.signal takes them."""
    import numpy as np
    c = filter_design(f, hz)
    return np.concatenate([c[:, :3], np.ones((c.shape[0], 1)), c[:, 3:]], axis=1)


def filter_pcm_host(pcm, f, hz: int):
    """jb_filter_pcm_host: the serial recursion on the host (no GPU), f64 in and out."""
    import numpy as np
    x = np.ascontiguousarray(pcm, dtype=np.float64)
    y = np.empty_like(x)
    dp = C.POINTER(C.c_double)
    check(lib().jb_filter_pcm_host(x.ctypes.data_as(dp), x.size, C.byref(f if f is not None else Filter()), int(hz),
                                   y.ctypes.data_as(dp), y.size))
    return y


def filter_pcm(pcms, filters, hz, device: int = -1, i16: bool = False):
    """jb_filter_pcm_batch / _i16: the f64 utterances `pcms` filtered on the GPU, utterance u under filters[u] (a
    Filter, or None) at hz[u]; one Filter or one rate stands for all.  f64 out, or int16 by the 16-bit sink's rule."""
    import numpy as np
    L = lib()
    arrs, n, ins, nin = _pcm_args(pcms, np.float64, void=True)
    farr, nf = filter_array(filters, n)
    if nf != n:
        raise ValueError("filter_pcm: one filter, or one per utterance")
    rates = [int(hz)] * n if np.isscalar(hz) else [int(h) for h in hz]
    if len(rates) != n:
        raise ValueError("filter_pcm: one rate, or one per utterance")
    hzs = (C.c_uint32 * max(1, n))(*rates)
    outs = (C.c_void_p * max(1, n))()
    ns = (C.c_size_t * max(1, n))()
    check((L.jb_filter_pcm_batch_i16 if i16 else L.jb_filter_pcm_batch)(ins, nin, n, farr, hzs, device, outs, ns))
    return _take(L.jb_filter_free, outs, ns, n, np.int16 if i16 else np.float64)


def fir_geometry(n_taps: int):
    """jb_fir_geometry: (mode, block, partitions) of a response of n_taps taps -- FIR_DIRECT with the tile, or
    FIR_PARTITIONED with Bk = n_fft / 2 and P = ceil(n_taps / Bk)."""
    m, b, p = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().jb_fir_geometry(int(n_taps), C.byref(m), C.byref(b), C.byref(p)))
    return m.value, b.value, p.value


def fir_host(pcm, f):
    """jb_fir_host: the host rule (no GPU), f64 in and out; f: a Fir, or None."""
    import numpy as np
    x = np.ascontiguousarray(pcm, dtype=np.float64)
    y = np.empty_like(x)
    dp = C.POINTER(C.c_double)
    check(lib().jb_fir_host(x.ctypes.data_as(dp), x.size, C.byref(f if f is not None else Fir()),
                            y.ctypes.data_as(dp), y.size))
    return y


def fir_pcm(pcms, firs, hz, device: int = -1, i16: bool = False):
    """jb_fir_pcm_batch / _i16: the f64 utterances `pcms` convolved on the GPU, utterance u with firs[u] (a Fir, or
    None) at hz[u]; one Fir or one rate stands for all.  f64 out, or int16 by the 16-bit sink's rule."""
    import numpy as np
    L = lib()
    arrs, n, ins, nin = _pcm_args(pcms, np.float64, void=True)
    farr, nf = fir_array(firs, n)
    if nf != n:
        raise ValueError("fir_pcm: one response, or one per utterance")
    rates = [int(hz)] * n if np.isscalar(hz) else [int(h) for h in hz]
    if len(rates) != n:
        raise ValueError("fir_pcm: one rate, or one per utterance")
    hzs = (C.c_uint32 * max(1, n))(*rates)
    outs = (C.c_void_p * max(1, n))()
    ns = (C.c_size_t * max(1, n))()
    check((L.jb_fir_pcm_batch_i16 if i16 else L.jb_fir_pcm_batch)(ins, nin, n, farr, hzs, device, outs, ns))
    return _take(L.jb_fir_free, outs, ns, n, np.int16 if i16 else np.float64)


def room_host(r):
    """jb_room_host: the taps of Room r by the rule on the host (no GPU)."""
    import numpy as np
    h = np.empty(int(r.n_taps), dtype=np.float64)
    check(lib().jb_room_host(C.byref(r), h.ctypes.data_as(C.POINTER(C.c_double)), h.size))
    return h


def room_rir(rooms, device: int = -1):
    """jb_room_rir_batch: the taps of every Room of `rooms`, generated on the GPU; equal rooms are generated once."""
    import numpy as np
    L = lib()
    rs = list(rooms)
    arr, n = room_array(rs)
    n = len(rs)
    outs = (C.c_void_p * max(1, n))()
    ns = (C.c_size_t * max(1, n))()
    check(L.jb_room_rir_batch(arr, n, device, outs, ns))
    return _take(L.jb_room_free, outs, ns, n, np.float64)


def room_geometry(r):
    """jb_room_geometry: the RoomInfo of Room r (pure)."""
    info = RoomInfo()
    check(lib().jb_room_geometry(C.byref(r), C.byref(info)))
    return info


def room_lowpass():
    """jb_room_lowpass: (F, Wh, Q) -- the low-pass interpolator's table of Q Wh + 3 entries and its constants."""
    import numpy as np
    wh, q = C.c_uint32(), C.c_uint32()
    check(lib().jb_room_lowpass(None, 0, C.byref(wh), C.byref(q)))
    F = np.empty(wh.value * q.value + 3, dtype=np.float64)
    check(lib().jb_room_lowpass(F.ctypes.data_as(C.POINTER(C.c_double)), F.size, None, None))
    return F, wh.value, q.value


def room_design(size, rt60: float, c: float = 343.0):
    """jb_room_design: the six reflection coefficients of a room of edges `size` with the reverberation time rt60
    (Eyring's formula)."""
    s = (C.c_double * 3)(*[float(v) for v in size])
    b = (C.c_double * 6)()
    check(lib().jb_room_design(s, float(rt60), float(c), b))
    return list(b)


def room_vary(seed: int, k: int, size, margin: float = 0.5):
    """jb_room_vary: (source, mic) of the utterance of index k, at least `margin` from every wall."""
    s = (C.c_double * 3)(*[float(v) for v in size])
    src, mic = (C.c_double * 3)(), (C.c_double * 3)()
    check(lib().jb_room_vary(int(seed) & (2**64 - 1), int(k), s, float(margin), src, mic))
    return list(src), list(mic)


def noise_host(pcm, req, gain=None, i16: bool = False):
    """jb_noise_host / _i16: the host rule (no GPU) on f64 `pcm` under `req` (a Noise, or None); gain None: the
    rule's gain, else taken as given.  Returns (y, NoiseReport)."""
    import numpy as np
    x = np.ascontiguousarray(pcm, dtype=np.float64)
    y = np.empty(x.size, dtype=np.int16 if i16 else np.float64)
    dp = C.POINTER(C.c_double)
    g = None if gain is None else C.byref(C.c_double(float(gain)))
    rep = NoiseReport()
    fn = lib().jb_noise_host_i16 if i16 else lib().jb_noise_host
    check(fn(x.ctypes.data_as(dp), x.size, C.byref(req if req is not None else Noise()), g,
             y.ctypes.data_as(C.POINTER(C.c_int16) if i16 else dp), y.size, C.byref(rep)))
    return y, rep


def noise_white(seed: int, first: int, count: int):
    """jb_noise_white: samples first .. first + count of the white sequence of `seed` (exact integers in +-131070)."""
    import numpy as np
    out = np.empty(int(count), dtype=np.float64)
    check(lib().jb_noise_white(int(seed) & (2**64 - 1), int(first), out.size,
                               out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def noise_vary(seed: int, k: int, bed_len: int = 0):
    """jb_noise_vary: (seed_k, offset_k) of the utterance of index k under NOISE_VARY."""
    s, o = C.c_uint64(), C.c_uint32()
    check(lib().jb_noise_vary(int(seed) & (2**64 - 1), int(k), int(bed_len), C.byref(s), C.byref(o)))
    return s.value, o.value


def noise_pcm(pcms, reqs, hz, device: int = -1, i16: bool = False):
    """jb_noise_pcm_batch / _i16: the f64 utterances `pcms` under reqs[u] (a Noise, or None) at hz[u] on the GPU; one
    Noise or one rate stands for all.  Returns (outs, reports): f64, or int16 by the 16-bit sink's rule."""
    import numpy as np
    L = lib()
    arrs, n, ins, nin = _pcm_args(pcms, np.float64, void=True)
    rarr, nr = noise_array(reqs, n)
    if nr != n:
        raise ValueError("noise_pcm: one request, or one per utterance")
    rates = [int(hz)] * n if np.isscalar(hz) else [int(h) for h in hz]
    if len(rates) != n:
        raise ValueError("noise_pcm: one rate, or one per utterance")
    hzs = (C.c_uint32 * max(1, n))(*rates)
    outs = (C.c_void_p * max(1, n))()
    ns = (C.c_size_t * max(1, n))()
    reps = (NoiseReport * max(1, n))()
    check((L.jb_noise_pcm_batch_i16 if i16 else L.jb_noise_pcm_batch)(ins, nin, n, rarr, hzs, device, outs, ns, reps))
    return _take(L.jb_noise_free, outs, ns, n, np.int16 if i16 else np.float64), list(reps)[:n]


def limiter_window(hz: int, opts=None):
    """jb_limiter_window: (L, H, w[0..L]) of a LimiterOpts (None: the defaults) at `hz`."""
    import numpy as np
    L_, H_ = C.c_uint32(), C.c_uint32()
    o = None if opts is None else C.byref(opts)
    check(lib().jb_limiter_window(int(hz), o, C.byref(L_), C.byref(H_), None, 0))
    w = np.empty(L_.value + 1, dtype=np.float64)
    check(lib().jb_limiter_window(int(hz), o, None, None, w.ctypes.data_as(C.POINTER(C.c_double)), w.size))
    return L_.value, H_.value, w


def limiter_host(pcm, hz: int, gain: float, ceiling_db: float, peak_mode: int = 0, opts=None, i16: bool = False):
    """jb_limiter_host / _i16: the limiter's rule on the host (no GPU): (y, report dict) of the f64 samples `pcm`
    under the linear `gain` and the ceiling in dBFS (dBTP with peak_mode = PEAK_TRUE)."""
    import numpy as np
    x = np.ascontiguousarray(pcm, dtype=np.float64)
    y = np.empty(x.size, dtype=np.int16 if i16 else np.float64)
    rep = LimiterReport()
    o = None if opts is None else C.byref(opts)
    fn = lib().jb_limiter_host_i16 if i16 else lib().jb_limiter_host
    check(fn(x.ctypes.data_as(C.POINTER(C.c_double)), x.size, int(hz), float(gain), float(ceiling_db), int(peak_mode),
             o, y.ctypes.data_as(C.POINTER(C.c_int16 if i16 else C.c_double)), C.byref(rep)))
    return y, rep.as_dict()


def limiter_pcm(pcms, hz, gain, ceiling_db, peak_mode=0, opts=None, device: int = -1, i16: bool = False):
    """jb_limiter_pcm_batch / _i16: the f64 utterances `pcms` limited on the GPU; hz, gain, ceiling_db, peak_mode and
    opts are one value for all or one per utterance.  Returns ([y], [report dict])."""
    import numpy as np
    L = lib()
    arrs, n, ins, nin = _pcm_args(pcms, np.float64, void=True)

    def per(v, what):
        vs = [v] * n if np.isscalar(v) else list(v)
        if len(vs) != n:
            raise ValueError("limiter_pcm: one %s, or one per utterance" % what)
        return vs
    oarr, no = limiter_array(limiter() if opts is None else opts, n)
    if no != n and n:
        raise ValueError("limiter_pcm: one request, or one per utterance")
    hzs = (C.c_uint32 * max(1, n))(*[int(h) for h in per(hz, "rate")])
    gs = (C.c_double * max(1, n))(*[float(g) for g in per(gain, "gain")])
    cs = (C.c_double * max(1, n))(*[float(c) for c in per(ceiling_db, "ceiling")])
    ms = (C.c_uint32 * max(1, n))(*[int(m) for m in per(peak_mode, "peak mode")])
    outs = (C.c_void_p * max(1, n))()
    reps = (LimiterReport * max(1, n))()
    check((L.jb_limiter_pcm_batch_i16 if i16 else L.jb_limiter_pcm_batch)(ins, nin, n, hzs, gs, cs, ms, oarr, device,
                                                                          outs, reps))
    res = _take(L.jb_limiter_free, outs, [a.size for a in arrs], n, np.int16 if i16 else np.float64)
    return res, [reps[u].as_dict() for u in range(n)]


def resample(pcms, in_hz: int, out_hz: int, device: int = -1):
    """jb_resample_pcm_batch: each float64 array of `pcms` (or one array) converted from in_hz to out_hz on the GPU."""
    import numpy as np

    single = isinstance(pcms, np.ndarray)
    arrs, n, ins, nin = _pcm_args([pcms] if single else pcms, np.float64)
    L = lib()
    outs = (C.POINTER(C.c_double) * max(n, 1))()
    nout = (C.c_size_t * max(n, 1))()
    check(L.jb_resample_pcm_batch(ins, nin, n, in_hz, out_hz, device, outs, nout))
    res = _take(L.jb_pcm_free, outs, nout, n, np.float64)
    return res[0] if single else res


def check(rc):
    if rc != JB_OK:
        raise JbError(rc, (lib().jb_last_error() or b"").decode(errors="replace"))

"""Host-side mirror of jbonsai's public API over the C ABI.

  Engine.load / load_from_bytes / synthesize / generator   src/engine.rs:257-366
  Condition setters/getters                                src/engine.rs:127-243
  SpeechGenerator.{fperiod, synthesized_frames, generate_step, generate_all}
                                                           src/speech.rs:53-96
Names, argument meaning and error behaviour follow the reference so that the
tests read like the reference's own (src/lib.rs:38-160).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Sequence

import numpy as np

from . import _ffi as F
from .batch import StreamInfo, StreamStates, Utterance, VoiceInfo


def _bind(L):
    if getattr(L, "_engine_bound", False):
        return
    vp, sz, dp = C.c_void_p, C.c_size_t, C.POINTER(C.c_double)
    cpp = C.POINTER(C.c_char_p)
    L.jb_engine_load.argtypes = [cpp, sz, C.POINTER(vp)]
    L.jb_engine_load_from_bytes.argtypes = [C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.POINTER(vp)]
    L.jb_engine_free.argtypes = [vp]
    L.jb_engine_free.restype = None
    for n in ("sampling_frequency", "fperiod"):
        getattr(L, "jb_engine_set_" + n).argtypes = [vp, sz]
        getattr(L, "jb_engine_get_" + n).argtypes = [vp]
        getattr(L, "jb_engine_get_" + n).restype = sz
    for n in ("volume", "speed", "alpha", "beta", "additional_half_tone"):
        getattr(L, "jb_engine_set_" + n).argtypes = [vp, C.c_double]
        getattr(L, "jb_engine_get_" + n).argtypes = [vp]
        getattr(L, "jb_engine_get_" + n).restype = C.c_double
    for n in ("msd_threshold", "gv_weight"):
        getattr(L, "jb_engine_set_" + n).argtypes = [vp, sz, C.c_double]
        getattr(L, "jb_engine_get_" + n).argtypes = [vp, sz]
        getattr(L, "jb_engine_get_" + n).restype = C.c_double
    L.jb_engine_set_phoneme_alignment_flag.argtypes = [vp, C.c_int]
    L.jb_engine_get_phoneme_alignment_flag.argtypes = [vp]
    L.jb_engine_set_batch_invariant.argtypes = [vp, C.c_int]
    L.jb_engine_get_batch_invariant.argtypes = [vp]
    L.jb_engine_set_output_sampling_frequency.argtypes = [vp, sz]
    L.jb_engine_get_output_sampling_frequency.argtypes = [vp]
    L.jb_engine_get_output_sampling_frequency.restype = sz
    for n in ("loudness_target", "peak_ceiling"):
        getattr(L, "jb_engine_set_" + n).argtypes = [vp, C.c_double]
        getattr(L, "jb_engine_get_" + n).argtypes = [vp]
        getattr(L, "jb_engine_get_" + n).restype = C.c_double
    L.jb_engine_set_peak_mode.argtypes = [vp, C.c_uint32]
    L.jb_engine_get_peak_mode.argtypes = [vp]
    L.jb_engine_get_peak_mode.restype = C.c_uint32
    L.jb_engine_set_fast_invariant.argtypes = [vp, C.c_int]
    L.jb_engine_get_fast_invariant.argtypes = [vp]
    for n in ("num_voices", "num_streams", "num_states"):
        getattr(L, "jb_engine_" + n).argtypes = [vp]
        getattr(L, "jb_engine_" + n).restype = sz
    L.jb_engine_set_interpolation_weight.argtypes = [vp, C.c_int, sz, dp, sz]
    L.jb_engine_get_interpolation_weight.argtypes = [vp, C.c_int, sz, dp, sz, C.POINTER(sz)]
    L.jb_engine_new.argtypes = [vp, vp, C.POINTER(vp)]
    L.jb_engine_model_shape.argtypes = [vp, sz, C.c_int, C.POINTER(sz), C.POINTER(sz)]
    L.jb_engine_pdf_table.argtypes = [vp, sz, C.c_int, sz, C.POINTER(C.POINTER(C.c_float)), C.POINTER(sz)]
    L.jb_engine_tree_index.argtypes = [vp, sz, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]
    L.jb_synthesize.argtypes = [vp, cpp, sz, C.POINTER(dp), C.POINTER(sz)]
    L.jb_pcm_free.argtypes = [dp]
    L.jb_pcm_free.restype = None
    L.jb_synthesize_batch.argtypes = [vp, cpp, C.POINTER(sz), sz, C.c_int32, C.POINTER(dp), C.POINTER(sz)]
    L.jb_synthesize_batch_i16.argtypes = [vp, cpp, C.POINTER(sz), sz, C.c_int32,
                                          C.POINTER(C.POINTER(C.c_int16)), C.POINTER(sz)]
    L.jb_synthesize_batch_multi.argtypes = [vp, cpp, C.POINTER(sz), sz, C.POINTER(C.c_int32), sz, C.POINTER(dp),
                                            C.POINTER(sz)]
    L.jb_synthesize_batch_i16_multi.argtypes = [vp, cpp, C.POINTER(sz), sz, C.POINTER(C.c_int32), sz,
                                                C.POINTER(C.POINTER(C.c_int16)), C.POINTER(sz)]
    L.jb_synthesize_batch_each.argtypes = [C.POINTER(vp), cpp, C.POINTER(sz), sz, C.c_int32, C.POINTER(dp),
                                           C.POINTER(sz)]
    L.jb_synthesize_batch_each_i16.argtypes = [C.POINTER(vp), cpp, C.POINTER(sz), sz, C.c_int32,
                                               C.POINTER(C.POINTER(C.c_int16)), C.POINTER(sz)]
    L.jb_pcm_i16_free.argtypes = [C.POINTER(C.c_int16)]
    L.jb_pcm_i16_free.restype = None
    L.jb_engine_states.argtypes = [vp, cpp, sz, C.POINTER(vp)]
    L.jb_states_utt.argtypes = [vp]
    L.jb_states_utt.restype = C.POINTER(F.StateUtt)
    L.jb_engine_voice_desc.argtypes = [vp]
    L.jb_engine_voice_desc.restype = C.POINTER(F.VoiceDesc)
    L.jb_states_duration_params.argtypes = [vp]
    L.jb_states_duration_params.restype = C.POINTER(C.c_double)
    L.jb_states_free.argtypes = [vp]
    L.jb_states_free.restype = None
    L.jb_generator_new.argtypes = [vp, cpp, sz, C.POINTER(vp)]
    for n in ("fperiod", "synthesized_frames", "total_frames"):
        getattr(L, "jb_generator_" + n).argtypes = [vp]
        getattr(L, "jb_generator_" + n).restype = sz
    L.jb_generator_step.argtypes = [vp, dp, sz]
    L.jb_generator_step.restype = C.c_long
    L.jb_generator_step_n.argtypes = [vp, dp, sz, sz]
    L.jb_generator_step_n.restype = C.c_long
    L.jb_generator_free.argtypes = [vp]
    L.jb_generator_free.restype = None
    L._engine_bound = True


def _lines(labels: Sequence[str]):
    arr = (C.c_char_p * max(1, len(labels)))()
    for i, s in enumerate(labels):
        arr[i] = s.encode() if isinstance(s, str) else bytes(s)
    return arr


def _utt_lines(utterances):
    """(lines, offs, B) of B utterances: their labels in one array, utterance u's being lines[offs[u]:offs[u + 1]]."""
    B = len(utterances)
    offs = (C.c_size_t * (B + 1))(*np.cumsum([0] + [len(u) for u in utterances]).tolist())
    return _lines([l for u in utterances for l in u]), offs, B


def _byte_outs(B, counts=False):
    """The output arrays of a byte-sink entry of B outputs: (bufs, ns), with counts (bufs, ns, counts)."""
    sz = C.c_size_t * max(1, B)
    return ((C.POINTER(C.c_uint8) * max(1, B))(), sz()) + ((sz(),) if counts else ())


def _fbank_opts(opts, kw):
    return opts if opts is not None else F.fbank(**kw)


def _melspec_opts(opts, kw):
    return opts if opts is not None else F.melspec(**kw)


def _pitch_opts(opts, kw):
    return opts if opts is not None else F.pitch(**kw)


def _drain(kw):
    """The keywords left in kw, taken out of it."""
    rest = dict(kw)
    kw.clear()
    return rest


# synthesize_programme's byte sinks: the option structs a sink builds from the call's keywords (taking out of them what
# it knows; None: a NULL pointer), its C entry, whether the entry has a per-output count, and the output of
# (engine, library, buffer, bytes, count, option structs)
_PROGRAMME_SINKS = {
    "flac": (lambda kw: (F.flac_opts(kw.pop("block_size", 0), kw.pop("max_lpc_order", None)),
                         F.flac_meta(kw.pop("md5", False), kw.pop("seek_interval_ms", 0))),
             "jb_synthesize_programme_flac_meta", False, lambda e, L, buf, n, cnt, o: F.take_flac(L, [buf], [n], 1)[0]),
    "formatted": (lambda kw: (F.format_opts(kw.pop("fmt"), kw.pop("dither", False), kw.pop("seed", 0)),),
                  "jb_synthesize_programme_formatted", False,
                  lambda e, L, buf, n, cnt, o: F.take_formatted(L, [buf], [n], 1)[0]),
    "adpcm": (lambda kw: (F.adpcm_opts(kw.pop("block_align", 0)),), "jb_synthesize_programme_adpcm", True,
              lambda e, L, buf, n, cnt, o: F.adpcm_streams(L, [buf], [n], [cnt], [e._out_hz()], o[0].block_align, 1)[0]),
    "fbank": (lambda kw: (_fbank_opts(kw.pop("opts", None), _drain(kw)),), "jb_synthesize_programme_fbank", True,
              lambda e, L, buf, n, cnt, o: F.take_fbank(L, [buf], [n], 1, o[0])[0]),
    "mfcc": (lambda kw: F.mfcc_request(kw.pop("opts", None), kw.pop("fbank", None), _drain(kw)),
             "jb_synthesize_programme_mfcc", True,
             lambda e, L, buf, n, cnt, o: F.take_mfcc(L, [buf], [n], 1, o[1], o[0].n_mels)[0]),
    "melspec": (lambda kw: (_melspec_opts(kw.pop("opts", None), _drain(kw)),), "jb_synthesize_programme_melspec", True,
                lambda e, L, buf, n, cnt, o: F.take_melspec(L, [buf], [n], 1, o[0])[0]),
    "pitch": (lambda kw: (_pitch_opts(kw.pop("opts", None), _drain(kw)),), "jb_synthesize_programme_pitch", True,
              lambda e, L, buf, n, cnt, o: F.take_pitch(L, [buf], [n], 1, o[0])[0]),
}


class _Condition:
    """View of the engine's Condition (src/engine.rs:31-243)."""

    def __init__(self, eng):
        self._e = eng

    def _h(self):
        return self._e._h

    def _L(self):
        return self._e._L

    def set_sampling_frequency(self, i): F.check(self._L().jb_engine_set_sampling_frequency(self._h(), int(i)))
    def get_sampling_frequency(self): return self._L().jb_engine_get_sampling_frequency(self._h())
    def set_fperiod(self, i): F.check(self._L().jb_engine_set_fperiod(self._h(), int(i)))
    def get_fperiod(self): return self._L().jb_engine_get_fperiod(self._h())
    def set_volume(self, db): F.check(self._L().jb_engine_set_volume(self._h(), float(db)))
    def get_volume(self): return self._L().jb_engine_get_volume(self._h())
    def set_msd_threshold(self, s, f): F.check(self._L().jb_engine_set_msd_threshold(self._h(), s, float(f)))
    def get_msd_threshold(self, s): return self._L().jb_engine_get_msd_threshold(self._h(), s)
    def set_gv_weight(self, s, f): F.check(self._L().jb_engine_set_gv_weight(self._h(), s, float(f)))
    def get_gv_weight(self, s): return self._L().jb_engine_get_gv_weight(self._h(), s)
    def set_speed(self, f): F.check(self._L().jb_engine_set_speed(self._h(), float(f)))
    def get_speed(self): return self._L().jb_engine_get_speed(self._h())
    def set_phoneme_alignment_flag(self, b): F.check(self._L().jb_engine_set_phoneme_alignment_flag(self._h(), int(bool(b))))
    def get_phoneme_alignment_flag(self): return bool(self._L().jb_engine_get_phoneme_alignment_flag(self._h()))
    def set_batch_invariant(self, b): F.check(self._L().jb_engine_set_batch_invariant(self._h(), int(bool(b))))
    def get_batch_invariant(self): return bool(self._L().jb_engine_get_batch_invariant(self._h()))
    def set_fast_invariant(self, b): F.check(self._L().jb_engine_set_fast_invariant(self._h(), int(bool(b))))
    def get_fast_invariant(self): return bool(self._L().jb_engine_get_fast_invariant(self._h()))
    def set_output_sampling_frequency(self, hz):
        F.check(self._L().jb_engine_set_output_sampling_frequency(self._h(), int(hz)))
    def get_output_sampling_frequency(self): return self._L().jb_engine_get_output_sampling_frequency(self._h())
    def set_loudness_target(self, lufs):
        """Target loudness (LUFS) of every entry's output; NaN (the default) = off."""
        F.check(self._L().jb_engine_set_loudness_target(self._h(), float(lufs)))
    def get_loudness_target(self): return self._L().jb_engine_get_loudness_target(self._h())
    def set_peak_ceiling(self, dbfs):
        """Sample-peak ceiling (dBFS) that goes with the target: default 0, inf = none."""
        F.check(self._L().jb_engine_set_peak_ceiling(self._h(), float(dbfs)))
    def get_peak_ceiling(self): return self._L().jb_engine_get_peak_ceiling(self._h())
    def set_peak_mode(self, mode):
        """What the ceiling bounds: 0 = the sample peak (the default), 1 = the true peak (dBTP)."""
        F.check(self._L().jb_engine_set_peak_mode(self._h(), int(mode)))
    def get_peak_mode(self): return self._L().jb_engine_get_peak_mode(self._h())
    def set_filter(self, f):
        """The output filter (an _ffi.Filter: J.highpass(70), J.telephone_band(), ...) of every entry's output, behind
        the output rate and in front of the loudness target; None (the default) = off."""
        F.check(self._L().jb_engine_set_filter(self._h(), None if f is None else C.byref(f)))
    def set_fir(self, f):
        """The impulse response (an _ffi.Fir: J.fir(taps, hz, delay)) of every entry's output, in front of the
        filter's sections; None for none.  The taps are copied."""
        F.check(self._L().jb_engine_set_fir(self._h(), None if f is None else C.byref(f)))
    def set_frame(self, fr=None, **kw):
        """The frame request (an _ffi.FrameOpts: J.frame(...), or its keywords) of every *_fbank and *_mfcc entry's
        features; None without keywords for none."""
        if fr is None and kw:
            fr = F.frame(**kw)
        F.check(self._L().jb_engine_set_frame_opts(self._h(), None if fr is None else C.byref(fr)))
    def set_room(self, room, vary=False, seed=0, margin=0.5):
        """The room (an _ffi.Room: J.room(size, source, mic, rt60=..., hz=..., n_taps=...)) of every entry's output,
        in the impulse response's place (the later of set_room and set_fir replaces the earlier); None for none.
        vary: the utterance of index k in a call gets the positions J.room_vary(seed, k, size, margin)."""
        F.check(self._L().jb_engine_set_room(self._h(), None if room is None else C.byref(room),
                                             F.ROOM_VARY if vary else 0, int(seed) & (2**64 - 1), float(margin)))
    def set_noise(self, r):
        """The noise request (an _ffi.Noise: J.noise(bed, hz, snr_db, ...)) of every entry's output, behind the
        impulse response and in front of the filter's sections; None for none.  The bed is copied."""
        F.check(self._L().jb_engine_set_noise(self._h(), None if r is None else C.byref(r)))
    def get_filter(self):
        f = F.Filter()
        F.check(self._L().jb_engine_get_filter(self._h(), C.byref(f)))
        return f
    def set_limiter(self, opts):
        """The look-ahead peak limiter (an _ffi.LimiterOpts: J.limiter(max_reduction_db=6)) of every entry's output,
        in effect with a loudness target and a ceiling; None (the default) = off."""
        F.check(self._L().jb_engine_set_limiter(self._h(), None if opts is None else C.byref(opts)))
    def get_limiter(self):
        """The request as it was given, or None."""
        o = F.LimiterOpts()
        rc = self._L().jb_engine_get_limiter(self._h(), C.byref(o))
        F.check(min(rc, 0))
        return o if rc == 1 else None
    def set_loudness_scope(self, scope):
        """What one gain of the target covers: 0 = each utterance (the default), 1 = the whole request
        (_ffi.LOUDNESS_PER_UTTERANCE / LOUDNESS_PER_REQUEST): the utterances of one synthesize_batch call keep
        their relative levels."""
        F.check(self._L().jb_engine_set_loudness_scope(self._h(), int(scope)))
    def get_loudness_scope(self): return self._L().jb_engine_get_loudness_scope(self._h())
    def set_tree_search(self, mode):
        """Where the per-label tree search runs: 0 = host threads (the default), 1 = the device from the measured
        request size on, 2 = the device always (_ffi.SEARCH_*)."""
        F.check(self._L().jb_engine_set_tree_search(self._h(), int(mode)))
    def get_tree_search(self): return self._L().jb_engine_get_tree_search(self._h())
    def set_alpha(self, f): F.check(self._L().jb_engine_set_alpha(self._h(), float(f)))
    def get_alpha(self): return self._L().jb_engine_get_alpha(self._h())
    def set_beta(self, f): F.check(self._L().jb_engine_set_beta(self._h(), float(f)))
    def get_beta(self): return self._L().jb_engine_get_beta(self._h())
    def set_additional_half_tone(self, f): F.check(self._L().jb_engine_set_additional_half_tone(self._h(), float(f)))
    def get_additional_half_tone(self): return self._L().jb_engine_get_additional_half_tone(self._h())

    # InterporationWeight (src/model/interporation_weight.rs:48-126)
    def _setw(self, which, stream, w):
        a = np.ascontiguousarray(w, dtype=np.float64)
        F.check(self._L().jb_engine_set_interpolation_weight(
            self._h(), which, stream, a.ctypes.data_as(C.POINTER(C.c_double)), len(a)))

    def _getw(self, which, stream):
        n = C.c_size_t()
        F.check(self._L().jb_engine_get_interpolation_weight(self._h(), which, stream, None, 0, C.byref(n)))
        a = np.zeros(n.value)
        F.check(self._L().jb_engine_get_interpolation_weight(
            self._h(), which, stream, a.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
        return a

    def get_interpolation_duration(self): return self._getw(0, 0)
    def get_interpolation_parameter(self, stream): return self._getw(1, stream)
    def get_interpolation_gv(self, stream): return self._getw(2, stream)
    def set_interpolation_duration(self, w): self._setw(0, 0, w)
    def set_interpolation_parameter(self, stream, w): self._setw(1, stream, w)
    def set_interpolation_gv(self, stream, w): self._setw(2, stream, w)


class Engine:
    """jbonsai::Engine over libjbonsai_amd.so."""

    def __init__(self, handle, L):
        self._h, self._L = handle, L
        self.condition = _Condition(self)

    @classmethod
    def load(cls, voices: Sequence[str]) -> "Engine":
        L = F.lib()
        _bind(L)
        h = C.c_void_p()
        paths = [str(p) for p in voices]
        F.check(L.jb_engine_load(_lines(paths), len(paths), C.byref(h)))
        return cls(h, L)

    @classmethod
    def load_from_bytes(cls, voices: Sequence[bytes]) -> "Engine":
        L = F.lib()
        _bind(L)
        h = C.c_void_p()
        bufs = (C.c_char_p * max(1, len(voices)))(*[C.c_char_p(b) for b in voices])
        lens = (C.c_size_t * max(1, len(voices)))(*[len(b) for b in voices])
        F.check(L.jb_engine_load_from_bytes(bufs, lens, len(voices), C.byref(h)))
        return cls(h, L)

    @classmethod
    def new(cls, voices_of: "Engine", condition_of: "Engine") -> "Engine":
        """Engine::new(voices, condition) (src/engine.rs:289-291): the voices of one engine (shared) with a
        copy of the Condition of another; Engine.new(e, e) is Engine::clone."""
        h = C.c_void_p()
        F.check(voices_of._L.jb_engine_new(voices_of._h, condition_of._h, C.byref(h)))
        return cls(h, voices_of._L)

    def clone(self) -> "Engine":
        return Engine.new(self, self)

    def set_loudness_scope(self, scope):
        """jb_engine_set_loudness_scope (the Condition's setter, on the engine): _ffi.LOUDNESS_PER_UTTERANCE or
        _ffi.LOUDNESS_PER_REQUEST."""
        self.condition.set_loudness_scope(scope)

    def get_loudness_scope(self):
        return self.condition.get_loudness_scope()

    def set_filter(self, f):
        """jb_engine_set_filter (the Condition's setter, on the engine): an _ffi.Filter, or None for none."""
        self.condition.set_filter(f)

    def set_fir(self, f):
        """jb_engine_set_fir (the Condition's setter, on the engine): an _ffi.Fir, or None for none."""
        self.condition.set_fir(f)

    def set_frame(self, fr=None, **kw):
        """jb_engine_set_frame_opts (the Condition's setter, on the engine): an _ffi.FrameOpts or the keywords of
        J.frame, or None for none."""
        self.condition.set_frame(fr, **kw)

    def set_room(self, room, vary=False, seed=0, margin=0.5):
        """jb_engine_set_room (the Condition's setter, on the engine): an _ffi.Room, or None for none; vary: positions
        of each utterance's own by J.room_vary(seed, k, size, margin)."""
        self.condition.set_room(room, vary=vary, seed=seed, margin=margin)

    def set_noise(self, r):
        """jb_engine_set_noise (the Condition's setter, on the engine): an _ffi.Noise, or None for none."""
        self.condition.set_noise(r)

    def set_programme_mix(self, place, fit: bool = False, ceiling_db: float = 0.0):
        """jb_engine_set_programme_mix: place = [(start_ms, gain_db), ...], one per utterance of the
        synthesize_programme calls to come, which then MIX their utterances (utterance u starts lead_ms + start_ms[u]
        into the programme, under gain_db[u]) instead of joining them; fit: a programme over ceiling_db (dBFS) is
        scaled down to it.  None withdraws the setting."""
        if place is None:
            F.check(self._L.jb_engine_set_programme_mix(self._h, None, 0, None))
            return
        arr = (F.MixPlace * max(1, len(place)))()
        for u, (start_ms, gain_db) in enumerate(place):
            arr[u].start_ms, arr[u].gain_db = float(start_ms), float(gain_db)
        o = F.mix_opts(fit, ceiling_db)
        F.check(self._L.jb_engine_set_programme_mix(self._h, arr, len(place), C.byref(o)))

    def get_programme_mix(self):
        """(place, fit, ceiling_db) as set_programme_mix took them; place None without a setting."""
        n, o = C.c_size_t(), F.MixOpts()
        F.check(self._L.jb_engine_get_programme_mix(self._h, None, 0, C.byref(n), C.byref(o)))
        if not n.value:
            return None, False, 0.0
        arr = (F.MixPlace * n.value)()
        F.check(self._L.jb_engine_get_programme_mix(self._h, arr, n.value, None, None))
        return [(a.start_ms, a.gain_db) for a in arr], bool(o.flags & F.MIX_FIT), o.ceiling_db

    def get_filter(self):
        return self.condition.get_filter()

    def set_limiter(self, opts):
        """jb_engine_set_limiter (the Condition's setter, on the engine): an _ffi.LimiterOpts, or None for none."""
        self.condition.set_limiter(opts)

    def get_limiter(self):
        return self.condition.get_limiter()

    def close(self):
        if getattr(self, "_h", None):
            self._L.jb_engine_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- introspection --
    @property
    def num_voices(self): return self._L.jb_engine_num_voices(self._h)
    @property
    def num_streams(self): return self._L.jb_engine_num_streams(self._h)
    @property
    def num_states(self): return self._L.jb_engine_num_states(self._h)

    def model_shape(self, kind, voice=0):
        nt, pl = C.c_size_t(), C.c_size_t()
        F.check(self._L.jb_engine_model_shape(self._h, voice, kind, C.byref(nt), C.byref(pl)))
        return nt.value, pl.value

    def pdf_table(self, kind, tree, voice=0) -> np.ndarray:
        _, pl = self.model_shape(kind, voice)
        p, n = C.POINTER(C.c_float)(), C.c_size_t()
        F.check(self._L.jb_engine_pdf_table(self._h, voice, kind, tree, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(n.value, pl)).copy()

    def tree_index(self, kind, state_index, label, voice=0):
        ts, pi = C.c_int(), C.c_int()
        F.check(self._L.jb_engine_tree_index(self._h, voice, kind, state_index, label.encode(),
                                             C.byref(ts), C.byref(pi)))
        return (None if ts.value < 0 else ts.value, pi.value)

    @property
    def device_searched_labels(self) -> int:
        """Labels whose trees were searched on a device for this engine so far (0 in host mode)."""
        return int(self._L.jb_engine_device_searched_labels(self._h))

    def tree_search(self, labels: Sequence[str], device: int = -1, host: bool = False):
        """jb_tree_search_batch (host=True: jb_tree_search_flat_host, no GPU): (tree_state, pdf_index, gv_on) with
        the first two int32 [n_labels][num_voices][1 + num_streams][num_states] -- what tree_index returns for kind k
        and state index 2 + s, tree_state -1 for None -- and gv_on uint8 [n_labels]."""
        n = len(labels)
        shape = (n, self.num_voices, 1 + min(self.num_streams, F.MAX_STREAM), self.num_states)
        ts, pi = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        gv = np.zeros(n, np.uint8)
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        args = (ts.ctypes.data_as(i32p), pi.ctypes.data_as(i32p), gv.ctypes.data_as(u8p))
        if host:
            F.check(self._L.jb_tree_search_flat_host(self._h, _lines(labels), n, *args))
        else:
            F.check(self._L.jb_tree_search_batch(self._h, _lines(labels), n, device, *args))
        return ts, pi, gv

    def voice_info(self) -> VoiceInfo:
        d = self._L.jb_engine_voice_desc(self._h).contents
        streams = []
        for i in range(d.nstream):
            s = d.stream[i]
            off, wins = 0, []
            for w in range(s.num_windows):
                n = s.win_width[w]
                wins.append([s.win_coef[off + k] for k in range(n)])
                off += n
            streams.append(StreamInfo(s.vector_length, bool(s.is_msd), bool(s.use_gv), wins))
        return VoiceInfo(d.sampling_frequency, d.fperiod, d.alpha, streams, volume=d.volume,
                         beta=d.beta, stage=d.stage, use_log_gain=bool(d.use_log_gain))

    def states(self, labels: Sequence[str]) -> Utterance:
        """Front half only: labels -> state-level utterance (durations + per-state pdfs)."""
        h = C.c_void_p()
        F.check(self._L.jb_engine_states(self._h, _lines(labels), len(labels), C.byref(h)))
        try:
            u = self._L.jb_states_utt(h).contents
            vi = self.voice_info()
            S = u.num_states
            dur = np.ctypeslib.as_array(u.durations, shape=(S,)).copy() if S else np.zeros(0, np.uint32)
            sts = []
            for i, si in enumerate(vi.streams):
                s = u.stream[i]
                WL = si.vector_length * len(si.windows)
                arr = lambda p, shape, t=np.float64: (np.ctypeslib.as_array(p, shape=shape).copy()
                                                      if p and int(np.prod(shape)) else
                                                      (np.zeros(shape, t) if p or shape[0] == 0 else None))
                mean, var = arr(s.mean, (S, WL)), arr(s.var, (S, WL))
                if mean is None:
                    mean, var = np.zeros((S, WL)), np.zeros((S, WL))
                msd = arr(s.msd, (S,)) if s.msd else None
                gm = arr(s.gv_mean, (si.vector_length,)) if s.gv_mean else None
                gv = arr(s.gv_var, (si.vector_length,)) if s.gv_var else None
                gs = (np.ctypeslib.as_array(s.gv_switch, shape=(S,)).copy() if s.gv_switch and S else None)
                sts.append(StreamStates(mean, var, msd, gm, gv, gs, s.gv_weight, s.msd_threshold))
            return Utterance(dur, sts)
        finally:
            self._L.jb_states_free(h)

    def duration_params(self, labels: Sequence[str]) -> np.ndarray:
        """Models::duration() (src/model/mod.rs:80-92): [S][2] blended (mean, variance) of the duration pdfs."""
        h = C.c_void_p()
        F.check(self._L.jb_engine_states(self._h, _lines(labels), len(labels), C.byref(h)))
        try:
            S = self._L.jb_states_utt(h).contents.num_states
            p = self._L.jb_states_duration_params(h)
            return np.ctypeslib.as_array(p, shape=(S, 2)).copy() if S and p else np.zeros((0, 2))
        finally:
            self._L.jb_states_free(h)

    # -- synthesis --
    def synthesize(self, labels: Sequence[str]) -> np.ndarray:
        pcm, n = C.POINTER(C.c_double)(), C.c_size_t()
        F.check(self._L.jb_synthesize(self._h, _lines(labels), len(labels), C.byref(pcm), C.byref(n)))
        try:
            return np.ctypeslib.as_array(pcm, shape=(n.value,)).copy() if n.value else np.zeros(0)
        finally:
            if pcm:
                self._L.jb_pcm_free(pcm)

    def synthesize_batch(self, utterances: Sequence[Sequence[str]], device: int = -1,
                         i16: bool = False, devices: Sequence[int] = None) -> List[np.ndarray]:
        """jb_synthesize_batch / jb_synthesize_batch_i16 (or, with `devices`, their _multi forms: the
        utterances are LPT-split over the listed GPUs, one host thread per device).  The arrays view
        the library-owned buffers (no copy); each is released with jb_pcm_free / jb_pcm_i16_free when
        its array dies."""
        lines, offs, B = _utt_lines(utterances)
        ety = C.c_int16 if i16 else C.c_double
        pcm = (C.POINTER(ety) * max(1, B))()
        ns = (C.c_size_t * max(1, B))()
        free = self._L.jb_pcm_i16_free if i16 else self._L.jb_pcm_free
        if devices is not None:
            fn = self._L.jb_synthesize_batch_i16_multi if i16 else self._L.jb_synthesize_batch_multi
            dv = (C.c_int32 * max(1, len(devices)))(*[int(d) for d in devices])
            F.check(fn(self._h, lines, offs, B, dv, len(devices), pcm, ns))
        else:
            fn = self._L.jb_synthesize_batch_i16 if i16 else self._L.jb_synthesize_batch
            F.check(fn(self._h, lines, offs, B, device, pcm, ns))
        return _pcm_arrays(pcm, ns, B, i16, free)

    def synthesize_flac(self, labels: Sequence[str], block_size: int = 0, max_lpc_order=None, md5: bool = False,
                        seek_interval_ms: int = 0) -> bytes:
        """jb_synthesize_flac[_meta]: the FLAC stream of what synthesize_batch([labels], i16=True) returns; md5 /
        seek_interval_ms as Batch.set_flac's."""
        buf, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        opts, meta = F.flac_opts(block_size, max_lpc_order), F.flac_meta(md5, seek_interval_ms)
        if meta is None:
            F.check(self._L.jb_synthesize_flac(self._h, _lines(labels), len(labels), C.byref(opts), C.byref(buf),
                                               C.byref(n)))
        else:
            F.check(self._L.jb_synthesize_flac_meta(self._h, _lines(labels), len(labels), C.byref(opts),
                                                    C.byref(meta), C.byref(buf), C.byref(n)))
        return F.take_flac(self._L, [buf], [n.value], 1)[0]

    def synthesize_batch_flac(self, utterances: Sequence[Sequence[str]], device: int = -1, block_size: int = 0,
                              max_lpc_order=None, md5: bool = False, seek_interval_ms: int = 0) -> List[bytes]:
        """jb_synthesize_batch_flac[_meta]: one FLAC stream per utterance of synthesize_batch(..., i16=True)."""
        lines, offs, B = _utt_lines(utterances)
        bufs, ns = _byte_outs(B)
        opts, meta = F.flac_opts(block_size, max_lpc_order), F.flac_meta(md5, seek_interval_ms)
        if meta is None:
            F.check(self._L.jb_synthesize_batch_flac(self._h, lines, offs, B, device, C.byref(opts), bufs, ns))
        else:
            F.check(self._L.jb_synthesize_batch_flac_meta(self._h, lines, offs, B, device, C.byref(opts),
                                                          C.byref(meta), bufs, ns))
        return F.take_flac(self._L, bufs, ns, B)

    def synthesize_formatted(self, labels: Sequence[str], fmt, dither=False, seed: int = 0) -> bytes:
        """jb_synthesize_formatted: what synthesize(labels) returns as bytes of a sample format ("f32", "s16", "s24",
        "ulaw", "alaw"; dither=True: TPDF with `seed`), formatted on the GPU."""
        buf, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        opts = F.format_opts(fmt, dither, seed)
        F.check(self._L.jb_synthesize_formatted(self._h, _lines(labels), len(labels), C.byref(opts), C.byref(buf),
                                                C.byref(n)))
        return F.take_formatted(self._L, [buf], [n.value], 1)[0]

    def synthesize_batch_formatted(self, utterances: Sequence[Sequence[str]], fmt, dither=False, seed: int = 0,
                                   device: int = -1) -> List[bytes]:
        """jb_synthesize_batch_formatted: the bytes of each utterance of synthesize_batch(...) in the format."""
        lines, offs, B = _utt_lines(utterances)
        bufs, ns = _byte_outs(B)
        opts = F.format_opts(fmt, dither, seed)
        F.check(self._L.jb_synthesize_batch_formatted(self._h, lines, offs, B, device, C.byref(opts), bufs, ns))
        return F.take_formatted(self._L, bufs, ns, B)

    def _out_hz(self) -> int:
        return self.condition.get_output_sampling_frequency() or self.condition.get_sampling_frequency()

    def synthesize_adpcm(self, labels: Sequence[str], block_align: int = 0) -> "F.AdpcmStream":
        """jb_synthesize_adpcm: what synthesize(labels) returns, quantised to 16 bits and encoded as IMA ADPCM blocks
        (WAV tag 0x11) on the GPU.  block_align 0: by the output rate."""
        buf, n, ns = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_size_t()
        opts = F.adpcm_opts(block_align)
        F.check(self._L.jb_synthesize_adpcm(self._h, _lines(labels), len(labels), C.byref(opts), C.byref(buf),
                                            C.byref(n), C.byref(ns)))
        return F.adpcm_streams(self._L, [buf], [n.value], [ns.value], [self._out_hz()], block_align, 1)[0]

    def synthesize_adpcm_batch(self, utterances: Sequence[Sequence[str]], block_align: int = 0,
                               device: int = -1) -> List["F.AdpcmStream"]:
        """jb_synthesize_batch_adpcm: each utterance of synthesize_batch(...) as IMA ADPCM blocks."""
        lines, offs, B = _utt_lines(utterances)
        bufs, ns, nsamp = _byte_outs(B, counts=True)
        opts = F.adpcm_opts(block_align)
        F.check(self._L.jb_synthesize_batch_adpcm(self._h, lines, offs, B, device, C.byref(opts), bufs, ns, nsamp))
        return F.adpcm_streams(self._L, bufs, ns, nsamp, [self._out_hz()] * B, block_align, B)

    def synthesize_fbank(self, labels: Sequence[str], opts=None, **kw) -> np.ndarray:
        """jb_synthesize_fbank: the log-mel filterbank frames [T, n_mels] of what synthesize(labels) returns, computed
        on the GPU.  opts: F.FbankOpts, or the keywords of J.fbank."""
        opts = _fbank_opts(opts, kw)
        buf, n, nf = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_size_t()
        F.check(self._L.jb_synthesize_fbank(self._h, _lines(labels), len(labels), C.byref(opts), C.byref(buf),
                                            C.byref(n), C.byref(nf)))
        return F.take_fbank(self._L, [buf], [n.value], 1, opts)[0]

    def synthesize_fbank_batch(self, utterances: Sequence[Sequence[str]], opts=None, device: int = -1,
                               **kw) -> List[np.ndarray]:
        """jb_synthesize_batch_fbank: each utterance of synthesize_batch(...) as filterbank frames."""
        opts = _fbank_opts(opts, kw)
        lines, offs, B = _utt_lines(utterances)
        bufs, ns, nf = _byte_outs(B, counts=True)
        F.check(self._L.jb_synthesize_batch_fbank(self._h, lines, offs, B, device, C.byref(opts), bufs, ns, nf))
        return F.take_fbank(self._L, bufs, ns, B, opts)

    def synthesize_mfcc(self, labels: Sequence[str], opts=None, fbank=None, **kw) -> np.ndarray:
        """jb_synthesize_mfcc: the cepstral features [T, width] of what synthesize(labels) returns, computed on the GPU.
        opts: F.MfccOpts, or the keywords of J.mfcc; fbank: F.FbankOpts or a dict of J.fbank's keywords."""
        fo, mo = F.mfcc_request(opts, fbank, kw)
        buf, n, nf = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_size_t()
        F.check(self._L.jb_synthesize_mfcc(self._h, _lines(labels), len(labels), C.byref(fo), C.byref(mo),
                                           C.byref(buf), C.byref(n), C.byref(nf)))
        return F.take_mfcc(self._L, [buf], [n.value], 1, mo, fo.n_mels)[0]

    def synthesize_mfcc_batch(self, utterances: Sequence[Sequence[str]], opts=None, fbank=None, device: int = -1,
                              **kw) -> List[np.ndarray]:
        """jb_synthesize_batch_mfcc: each utterance of synthesize_batch(...) as cepstral features."""
        fo, mo = F.mfcc_request(opts, fbank, kw)
        lines, offs, B = _utt_lines(utterances)
        bufs, ns, nf = _byte_outs(B, counts=True)
        F.check(self._L.jb_synthesize_batch_mfcc(self._h, lines, offs, B, device, C.byref(fo), C.byref(mo), bufs, ns,
                                                 nf))
        return F.take_mfcc(self._L, bufs, ns, B, mo, fo.n_mels)

    def synthesize_melspec(self, labels: Sequence[str], opts=None, **kw) -> np.ndarray:
        """jb_synthesize_melspec: the mel spectrogram [T, n_mels] of what synthesize(labels) returns, computed on the
        GPU.  opts: F.MelspecOpts (J.melspec(...), J.whisper_mel(...)), or the keywords of J.melspec."""
        opts = _melspec_opts(opts, kw)
        buf, n, nf = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_size_t()
        F.check(self._L.jb_synthesize_melspec(self._h, _lines(labels), len(labels), C.byref(opts), C.byref(buf),
                                              C.byref(n), C.byref(nf)))
        return F.take_melspec(self._L, [buf], [n.value], 1, opts)[0]

    def synthesize_melspec_batch(self, utterances: Sequence[Sequence[str]], opts=None, device: int = -1,
                                 **kw) -> List[np.ndarray]:
        """jb_synthesize_batch_melspec: each utterance of synthesize_batch(...) as a mel spectrogram."""
        opts = _melspec_opts(opts, kw)
        lines, offs, B = _utt_lines(utterances)
        bufs, ns, nf = _byte_outs(B, counts=True)
        F.check(self._L.jb_synthesize_batch_melspec(self._h, lines, offs, B, device, C.byref(opts), bufs, ns, nf))
        return F.take_melspec(self._L, bufs, ns, B, opts)

    def synthesize_pitch(self, labels: Sequence[str], opts=None, **kw) -> np.ndarray:
        """jb_synthesize_pitch: the pitch features [T, width] of what synthesize(labels) returns, tracked on the GPU.
        opts: F.PitchOpts (J.kaldi_pitch(), J.pitch(...)), or the keywords of J.pitch."""
        opts = _pitch_opts(opts, kw)
        buf, n, nf = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_size_t()
        F.check(self._L.jb_synthesize_pitch(self._h, _lines(labels), len(labels), C.byref(opts), C.byref(buf),
                                            C.byref(n), C.byref(nf)))
        return F.take_pitch(self._L, [buf], [n.value], 1, opts)[0]

    def synthesize_pitch_batch(self, utterances: Sequence[Sequence[str]], opts=None, device: int = -1,
                               **kw) -> List[np.ndarray]:
        """jb_synthesize_batch_pitch: each utterance of synthesize_batch(...) as pitch features."""
        opts = _pitch_opts(opts, kw)
        lines, offs, B = _utt_lines(utterances)
        bufs, ns, nf = _byte_outs(B, counts=True)
        F.check(self._L.jb_synthesize_batch_pitch(self._h, lines, offs, B, device, C.byref(opts), bufs, ns, nf))
        return F.take_pitch(self._L, bufs, ns, B, opts)

    def synthesize_programme(self, utterances: Sequence[Sequence[str]], sink: str = "f64", lead_ms: float = 0.0,
                             gap_ms: float = 0.0, trail_ms: float = 0.0, fade_ms: float = 0.0, device: int = -1,
                             mix=None, fit: bool = False, ceiling_db: float = 0.0, stems=None, levels: bool = False,
                             **sink_opts):
        """jb_synthesize_programme*: the utterances as ONE programme -- lead_ms of zeros, the first utterance, gap_ms,
        the next, ..., trail_ms, a fade of fade_ms at both edges of each -- joined on the GPU in front of the sink.
        sink: "f64" or "i16" (PCM arrays), "flac" (bytes; block_size, max_lpc_order, md5, seek_interval_ms),
        "formatted" (bytes; fmt, dither, seed), "adpcm" (an AdpcmStream; block_align), "fbank" (an ndarray
        [T, n_mels]; opts=F.FbankOpts or the keywords of J.fbank), "mfcc" (an ndarray [T, width]; opts=F.MfccOpts or
        the keywords of J.mfcc, fbank=F.FbankOpts or a dict of J.fbank's keywords) or "melspec" (an ndarray
        [T, n_mels]; opts=F.MelspecOpts or the keywords of J.melspec).  Returns (output, starts):
        starts[u] is utterance u's first sample within the programme.
        mix=[(start_ms, gain_db), ...] (a convenience: set_programme_mix for this call alone, the engine's setting put
        back behind it) sums the utterances instead, each at its start and under its gain; fit and ceiling_db as there.
        stems=[id or None, ...] (behind a mix, sink "f64" or "flac"; another sink: ValueError; at batch level every
        sink takes stems): jb_synthesize_programme_stems*, one stem id per utterance.  The output is then a list, the
        mixture first and the S stems behind it, and the return (outputs, starts, reports) with one F.StemReport per
        stem; levels: the reports' three sums and dB values."""
        if stems is not None and sink not in ("f64", "flac"):
            raise ValueError('stems= goes with sink "f64" or "flac" (any other sink with stems: Batch.set_mix_stems)')
        if mix is not None:
            was = self.get_programme_mix()
            self.set_programme_mix(mix, fit, ceiling_db)
            try:
                return self.synthesize_programme(utterances, sink, lead_ms, gap_ms, trail_ms, fade_ms, device,
                                                 stems=stems, levels=levels, **sink_opts)
            finally:
                self.set_programme_mix(*was)
        lines, offs, B = _utt_lines(utterances)
        join = F.join_opts(lead_ms, gap_ms, trail_ms, fade_ms)
        starts = (C.c_uint64 * max(1, B))()
        out, n = C.c_void_p(), C.c_size_t()
        L = self._L
        if stems is not None:
            if len(stems) != B:
                raise ValueError("one stem id (or None) per utterance")
            ids, flags = F.stem_ids(stems), F.MIX_STEM_LEVELS * bool(levels)
            ns, U, reps = (C.c_size_t * (B + 1))(), C.c_size_t(), (F.StemReport * max(1, B))()
            if sink == "f64":
                if sink_opts:
                    raise TypeError(f"unknown options {sorted(sink_opts)}")
                outs = (C.c_void_p * (B + 1))()
                F.check(L.jb_synthesize_programme_stems(self._h, lines, offs, B, device, C.byref(join), ids, flags, outs,
                                                        ns, C.byref(U), reps, starts))
                res = F._take(L.jb_join_free, outs, ns, U.value, np.float64)
            else:
                opts = _PROGRAMME_SINKS["flac"][0](sink_opts)
                if sink_opts:
                    raise TypeError(f"unknown options {sorted(sink_opts)}")
                bufs = (C.POINTER(C.c_uint8) * (B + 1))()
                refs = [o if o is None else C.byref(o) for o in opts]
                F.check(L.jb_synthesize_programme_stems_flac_meta(self._h, lines, offs, B, device, *refs, C.byref(join),
                                                                  ids, flags, bufs, ns, C.byref(U), reps, starts))
                res = F.take_flac(L, bufs, ns, U.value)
            return res, list(starts[:B]), list(reps[:max(U.value, 1) - 1])
        if sink in ("f64", "i16"):
            if sink_opts:
                raise TypeError(f"unknown options {sorted(sink_opts)}")
            fn = L.jb_synthesize_programme_i16 if sink == "i16" else L.jb_synthesize_programme
            F.check(fn(self._h, lines, offs, B, device, C.byref(join), C.byref(out), C.byref(n), starts))
            ety, dt = (C.c_int16, np.int16) if sink == "i16" else (C.c_double, np.float64)
            res = np.frombuffer((ety * n.value).from_address(out.value), dtype=dt).copy() if n.value else np.zeros(0, dt)
            L.jb_join_free(out)  # (malloc'ed by the library, as every output is)
            return res, list(starts[:B])
        if sink not in _PROGRAMME_SINKS:
            raise ValueError('sink is "f64", "i16", "flac", "formatted", "adpcm", "fbank", "mfcc", "melspec" or "pitch"')
        build, entry, counted, take = _PROGRAMME_SINKS[sink]
        opts = build(sink_opts)
        if sink_opts:
            raise TypeError(f"unknown options {sorted(sink_opts)}")
        buf, count = C.POINTER(C.c_uint8)(), C.c_size_t()
        F.check(getattr(L, entry)(self._h, lines, offs, B, device, *[o if o is None else C.byref(o) for o in opts],
                                  C.byref(join), C.byref(buf), C.byref(n), *([C.byref(count)] if counted else []),
                                  starts))
        return take(self, L, buf, n.value, count.value, opts), list(starts[:B])

    def synthesize_programme_activity(self, utterances: Sequence[Sequence[str]], opts=None, lead_ms: float = 0.0,
                                      gap_ms: float = 0.0, trail_ms: float = 0.0, fade_ms: float = 0.0,
                                      device: int = -1, mix=None, fit: bool = False, ceiling_db: float = 0.0, **kw):
        """jb_synthesize_programme_activity: synthesize_programme(..., sink="f64") with the programme's speech-activity
        labels from the same run.  opts: F.ActivityOpts, or the keywords of J.activity.  Returns (pcm, labels, starts):
        labels is uint8 [T, C], with columns="members" one column per utterance, placed at starts[u].  mix, fit and
        ceiling_db as in synthesize_programme."""
        if mix is not None:
            was = self.get_programme_mix()
            self.set_programme_mix(mix, fit, ceiling_db)
            try:
                return self.synthesize_programme_activity(utterances, opts, lead_ms, gap_ms, trail_ms, fade_ms, device,
                                                          **kw)
            finally:
                self.set_programme_mix(*was)
        if opts is None:
            opts = F.activity(**kw)
        elif kw:
            raise TypeError(f"unknown options {sorted(kw)}")
        lines, offs, B = _utt_lines(utterances)
        join = F.join_opts(lead_ms, gap_ms, trail_ms, fade_ms)
        starts = (C.c_uint64 * max(1, B))()
        out, n, lab, T, Cc = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        L = self._L
        F.check(L.jb_synthesize_programme_activity(self._h, lines, offs, B, device, C.byref(join), C.byref(opts),
                                                   C.byref(out), C.byref(n), C.byref(lab), C.byref(T), C.byref(Cc),
                                                   starts))
        pcm = np.frombuffer((C.c_double * n.value).from_address(out.value), dtype=np.float64).copy() if n.value \
            else np.zeros(0, np.float64)
        L.jb_join_free(out)
        cells = T.value * Cc.value
        labels = np.frombuffer((C.c_uint8 * cells).from_address(lab.value), dtype=np.uint8).copy() if cells \
            else np.zeros(0, np.uint8)
        L.jb_activity_free(lab)
        return pcm, labels.reshape(T.value, Cc.value), list(starts[:B])

    def generator(self, labels: Sequence[str]) -> "SpeechGenerator":
        h = C.c_void_p()
        F.check(self._L.jb_generator_new(self._h, _lines(labels), len(labels), C.byref(h)))
        return SpeechGenerator(h, self._L, self.condition.get_output_sampling_frequency(),
                               self.condition.get_sampling_frequency())


def _pcm_arrays(pcm, ns, B, i16, free):
    """numpy views of library-owned PCM buffers, each released with `free` when its array dies."""
    ety = C.c_int16 if i16 else C.c_double
    out = []
    for i in range(B):
        if not ns[i]:
            out.append(np.zeros(0, dtype=np.int16 if i16 else np.float64))
            continue
        buf = (ety * ns[i]).from_address(C.addressof(pcm[i].contents))
        arr = np.frombuffer(buf, dtype=np.int16 if i16 else np.float64)
        weakref.finalize(buf, free, C.cast(C.addressof(pcm[i].contents), C.POINTER(ety)))
        out.append(arr)
    return out


def _each_call(engines, utterances):
    """(L, engine handles, lines, offs, B) of a synthesize_batch_each* call: one engine per utterance."""
    if len(engines) != len(utterances):
        raise ValueError("one engine per utterance")
    L = engines[0]._L if engines and engines[0] is not None else F.lib()
    _bind(L)
    hs = (C.c_void_p * max(1, len(engines)))(*[e._h if e is not None else None for e in engines])
    return (L, hs) + _utt_lines(utterances)


def synthesize_batch_each(engines: Sequence["Engine"], utterances: Sequence[Sequence[str]], i16: bool = False,
                          device: int = -1) -> List[np.ndarray]:
    """jb_synthesize_batch_each[_i16]: utterance u under engines[u]'s Condition, all in one batch.  The engines
    share one voice set (Engine.new / clone of one another) and agree on sampling frequency, fperiod, stage,
    log gain and the batch-invariant flag."""
    L, hs, lines, offs, B = _each_call(engines, utterances)
    ety = C.c_int16 if i16 else C.c_double
    pcm = (C.POINTER(ety) * max(1, B))()
    ns = (C.c_size_t * max(1, B))()
    fn = L.jb_synthesize_batch_each_i16 if i16 else L.jb_synthesize_batch_each
    F.check(fn(hs, lines, offs, B, device, pcm, ns))
    return _pcm_arrays(pcm, ns, B, i16, L.jb_pcm_i16_free if i16 else L.jb_pcm_free)


def synthesize_batch_each_formatted(engines: Sequence["Engine"], utterances: Sequence[Sequence[str]], fmt,
                                    dither=False, seed: int = 0, device: int = -1) -> List[bytes]:
    """jb_synthesize_batch_each_formatted: the bytes of synthesize_batch_each(...) in the sample format."""
    L, hs, lines, offs, B = _each_call(engines, utterances)
    bufs, ns = _byte_outs(B)
    opts = F.format_opts(fmt, dither, seed)
    F.check(L.jb_synthesize_batch_each_formatted(hs, lines, offs, B, device, C.byref(opts), bufs, ns))
    return F.take_formatted(L, bufs, ns, B)


def synthesize_batch_each_adpcm(engines: Sequence["Engine"], utterances: Sequence[Sequence[str]],
                                block_align: int = 0, device: int = -1) -> List["F.AdpcmStream"]:
    """jb_synthesize_batch_each_adpcm: synthesize_batch_each(...) as IMA ADPCM blocks, each utterance at its engine's
    output rate (and, with block_align 0, at that rate's block size)."""
    L, hs, lines, offs, B = _each_call(engines, utterances)
    bufs, ns, nsamp = _byte_outs(B, counts=True)
    opts = F.adpcm_opts(block_align)
    F.check(L.jb_synthesize_batch_each_adpcm(hs, lines, offs, B, device, C.byref(opts), bufs, ns, nsamp))
    return F.adpcm_streams(L, bufs, ns, nsamp, [e._out_hz() for e in engines], block_align, B)


def synthesize_batch_each_flac(engines: Sequence["Engine"], utterances: Sequence[Sequence[str]], device: int = -1,
                               block_size: int = 0, max_lpc_order=None, md5: bool = False,
                               seek_interval_ms: int = 0) -> List[bytes]:
    """jb_synthesize_batch_each_flac[_meta]: the FLAC streams of synthesize_batch_each(..., i16=True)."""
    L, hs, lines, offs, B = _each_call(engines, utterances)
    bufs, ns = _byte_outs(B)
    opts, meta = F.flac_opts(block_size, max_lpc_order), F.flac_meta(md5, seek_interval_ms)
    if meta is None:
        F.check(L.jb_synthesize_batch_each_flac(hs, lines, offs, B, device, C.byref(opts), bufs, ns))
    else:
        F.check(L.jb_synthesize_batch_each_flac_meta(hs, lines, offs, B, device, C.byref(opts), C.byref(meta), bufs,
                                                     ns))
    return F.take_flac(L, bufs, ns, B)


class SpeechGenerator:
    """jbonsai::speech::SpeechGenerator (src/speech.rs:9-96)."""

    def __init__(self, handle, L, output_rate: int = 0, voice_rate: int = 0):
        self._h, self._L = handle, L
        self.output_rate = output_rate if output_rate and output_rate != voice_rate else 0  # 0: native
        self.voice_rate = voice_rate

    def fperiod(self): return self._L.jb_generator_fperiod(self._h)
    def synthesized_frames(self): return self._L.jb_generator_synthesized_frames(self._h)
    def total_frames(self): return self._L.jb_generator_total_frames(self._h)

    def generate_step(self, speech: np.ndarray) -> int:
        """Writes fperiod samples to speech[0:fperiod]; returns fperiod, or 0 when exhausted.  With an output rate
        (L/M of the voice's) step k writes samples [ceil(k F L / M), ceil((k + 1) F L / M)) of the converted
        utterance and returns their count: a variable length."""
        assert speech.dtype == np.float64 and speech.flags["C_CONTIGUOUS"]
        r = self._L.jb_generator_step(self._h, speech.ctypes.data_as(C.POINTER(C.c_double)), speech.size)
        if r < 0:
            F.check(int(r))
        return int(r)

    def generate_steps(self, speech: np.ndarray, max_frames: int) -> int:
        """Up to max_frames generate_step calls in one (jb_generator_step_n): returns the samples written."""
        assert speech.dtype == np.float64 and speech.flags["C_CONTIGUOUS"]
        r = self._L.jb_generator_step_n(self._h, speech.ctypes.data_as(C.POINTER(C.c_double)), speech.size,
                                        int(max_frames))
        if r < 0:
            F.check(int(r))
        return int(r)

    def generate_all(self) -> np.ndarray:
        """generate_all (src/speech.rs:87-96): the frames not yet synthesized."""
        fp = self.fperiod()
        left = self.total_frames() - self.synthesized_frames()
        if self.output_rate:
            # variable-length steps: a buffer for the most one step of this rate pair writes, the steps concatenated
            step_max = -(-fp * self.output_rate // self.voice_rate)
            buf, parts = np.zeros(max(step_max, 1)), []
            while True:
                n = self.generate_step(buf)
                if n == 0:
                    break
                parts.append(buf[:n].copy())
            return np.concatenate(parts) if parts else np.zeros(0)
        buf = np.zeros(left * fp)
        if left:
            got = self.generate_steps(buf, left)
            assert got == left * fp
        return buf

    def close(self):
        if getattr(self, "_h", None):
            self._L.jb_generator_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synthesize_batch_each_fbank(engines: Sequence["Engine"], utterances: Sequence[Sequence[str]], opts=None,
                                device: int = -1, **kw) -> List[np.ndarray]:
    """jb_synthesize_batch_each_fbank: synthesize_batch_each(...) as filterbank frames, each utterance at its engine's
    output rate and that rate's geometry."""
    L, hs, lines, offs, B = _each_call(engines, utterances)
    opts = _fbank_opts(opts, kw)
    bufs, ns, nf = _byte_outs(B, counts=True)
    F.check(L.jb_synthesize_batch_each_fbank(hs, lines, offs, B, device, C.byref(opts), bufs, ns, nf))
    return F.take_fbank(L, bufs, ns, B, opts)

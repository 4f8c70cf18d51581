"""State-level batch API: the image of ModelStream + durations for B utterances
(reference: src/model/model_stream.rs:6-15, src/engine.rs:321-365)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi as F


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


@dataclass
class StreamInfo:
    """Static stream description (vector length, MSD/GV flags, delta windows)."""
    vector_length: int
    is_msd: bool
    use_gv: bool
    windows: List[List[float]]


@dataclass
class VoiceInfo:
    sampling_frequency: int
    fperiod: int
    alpha: float
    streams: List[StreamInfo]
    volume: float = 1.0
    beta: float = 0.0
    stage: int = 0
    use_log_gain: bool = False

    def c_struct(self):
        v = F.VoiceDesc()
        v.sampling_frequency, v.fperiod = self.sampling_frequency, self.fperiod
        v.nstream, v.stage, v.use_log_gain = len(self.streams), self.stage, int(self.use_log_gain)
        v.alpha, v.beta, v.volume = self.alpha, self.beta, self.volume
        keep = []
        for i, s in enumerate(self.streams):
            d = v.stream[i]
            d.vector_length, d.num_windows = s.vector_length, len(s.windows)
            d.is_msd, d.use_gv = int(s.is_msd), int(s.use_gv)
            coef = np.array([c for w in s.windows for c in w], dtype=np.float64)
            for k, w in enumerate(s.windows):
                d.win_width[k] = len(w)
            d.win_coef = _dp(coef)
            keep.append(coef)
        return v, keep


@dataclass
class StreamStates:
    mean: np.ndarray            # [S, W*L]
    var: np.ndarray             # [S, W*L]
    msd: Optional[np.ndarray] = None      # [S]
    gv_mean: Optional[np.ndarray] = None  # [L]
    gv_var: Optional[np.ndarray] = None
    gv_switch: Optional[np.ndarray] = None  # [S] uint8
    gv_weight: float = 1.0
    msd_threshold: float = 0.5

    def __post_init__(self):
        f = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
        self.mean, self.var = f(self.mean, np.float64), f(self.var, np.float64)
        self.msd, self.gv_mean, self.gv_var = f(self.msd, np.float64), f(self.gv_mean, np.float64), f(self.gv_var, np.float64)
        self.gv_switch = f(self.gv_switch, np.uint8)


@dataclass
class Utterance:
    durations: np.ndarray       # [S] uint32
    streams: List[StreamStates] = field(default_factory=list)

    def __post_init__(self):
        self.durations = np.ascontiguousarray(self.durations, dtype=np.uint32)

    def c_struct(self):
        u = F.StateUtt()
        u.num_states = len(self.durations)
        u.durations = self.durations.ctypes.data_as(C.POINTER(C.c_uint32))
        for i, s in enumerate(self.streams):
            d = u.stream[i]
            d.mean, d.var, d.msd = _dp(s.mean), _dp(s.var), _dp(s.msd)
            d.gv_mean, d.gv_var = _dp(s.gv_mean), _dp(s.gv_var)
            d.gv_switch = s.gv_switch.ctypes.data_as(C.POINTER(C.c_uint8)) if s.gv_switch is not None else None
            d.gv_weight, d.msd_threshold = s.gv_weight, s.msd_threshold
        return u


class PdfSet:
    """Device-resident pdf tables of a voice set (jb_pdf_set_create): tables[v][s] = float32 array
    [n_rows, row_len] of stream s of voice v, all trees of the stream concatenated."""

    def __init__(self, tables: Sequence[Sequence[np.ndarray]], device: int = -1):
        L = F.lib()
        self._L = L
        nv, ns = len(tables), len(tables[0])
        self._keep = [[np.ascontiguousarray(t, dtype=np.float32) for t in row] for row in tables]
        arr = (F.PdfTable * (nv * ns))()
        for v in range(nv):
            for s in range(ns):
                t = self._keep[v][s]
                arr[v * ns + s].rows = t.ctypes.data_as(C.POINTER(C.c_float))
                arr[v * ns + s].n_rows, arr[v * ns + s].row_len = t.shape
        h = C.c_void_p()
        F.check(L.jb_pdf_set_create(arr, nv, ns, device, C.byref(h)))
        self._h, self.n_voices, self.nstream, self.device = h, nv, ns, device

    def close(self):
        if getattr(self, "_h", None):
            self._L.jb_pdf_set_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class IndexStreamStates:
    """One stream of an utterance as pdf row indices (jb_index_stream): rows[v] = uint32 [S] rows of
    voice v's table; weights [n_voices]."""
    rows: List[np.ndarray]
    weights: np.ndarray
    gv_mean: Optional[np.ndarray] = None
    gv_var: Optional[np.ndarray] = None
    gv_switch: Optional[np.ndarray] = None
    gv_weight: float = 1.0
    msd_threshold: float = 0.5

    def __post_init__(self):
        f = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
        self.rows = [np.ascontiguousarray(r, dtype=np.uint32) for r in self.rows]
        self.weights = np.ascontiguousarray(self.weights, dtype=np.float64)
        self.gv_mean, self.gv_var = f(self.gv_mean, np.float64), f(self.gv_var, np.float64)
        self.gv_switch = f(self.gv_switch, np.uint8)

    def __setattr__(self, name, value):
        # (an IndexUtterance that has marshalled this stream keys its cached struct on the identity of every array it
        # points into: any replacement, of a field or of an element of `rows`, makes it marshal again)
        object.__setattr__(self, name, value)


@dataclass
class IndexUtterance:
    durations: np.ndarray
    streams: List[IndexStreamStates] = field(default_factory=list)
    lf0_offset: float = 0.0

    def __post_init__(self):
        self.durations = np.ascontiguousarray(self.durations, dtype=np.uint32)

    def c_struct(self):
        # marshalled once per object (the struct only points into arrays this object owns; an utterance is not
        # edited after its first use): a job that creates its batches again every pass -- bench.py's config-3
        # job -- spent 12 of the 27 ms of a 512-utterance creation building these
        # -- until one is.  The cached struct is valid for exactly the arrays it points into: the key is the identity
        # of every array (and the value of every scalar) placed in it, and the arrays are kept referenced beside it,
        # so that replacing an element in place (u.streams[i] = other, st.rows[v] = new) can neither leave the struct
        # pointing into freed memory nor go unseen (a sum of version counters missed both)
        arrays = [self.durations]
        for s in self.streams:
            arrays += list(s.rows) + [s.weights, s.gv_mean, s.gv_var, s.gv_switch]
        key = (tuple(id(a) for a in arrays), self.lf0_offset,
               tuple((s.gv_weight, s.msd_threshold) for s in self.streams))
        c = self.__dict__.get("_c")
        if c is not None and self.__dict__.get("_c_key") == key:
            return c
        u = F.IndexUtt()
        u.num_states = len(self.durations)
        u.durations = self.durations.ctypes.data_as(C.POINTER(C.c_uint32))
        u.lf0_offset = self.lf0_offset
        for i, s in enumerate(self.streams):
            d = u.stream[i]
            for v, r in enumerate(s.rows):
                d.row[v] = r.ctypes.data_as(C.POINTER(C.c_uint32))
            d.weight = _dp(s.weights)
            d.gv_mean, d.gv_var = _dp(s.gv_mean), _dp(s.gv_var)
            d.gv_switch = s.gv_switch.ctypes.data_as(C.POINTER(C.c_uint8)) if s.gv_switch is not None else None
            d.gv_weight, d.msd_threshold = s.gv_weight, s.msd_threshold
        self.__dict__["_c"] = u
        self.__dict__["_c_key"] = key
        self.__dict__["_c_arrays"] = arrays  # what the struct points into stays alive as long as the struct
        return u

    def __setattr__(self, name, value):
        object.__setattr__(self, name, value)
        self.__dict__.pop("_c", None)


@dataclass
class TrackUtterance:
    """The three parameter tracks of one utterance as SpeechGenerator::new takes them (src/speech.rs:25-50):
    spectrum [T][nmcp], lf0 [T][1] (NODATA = unvoiced frame), lpf [T][nlpf]."""
    spectrum: np.ndarray
    lf0: np.ndarray
    lpf: np.ndarray

    def __post_init__(self):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        self.spectrum, self.lpf = f(self.spectrum), f(self.lpf)
        self.lf0 = f(self.lf0)
        if self.lf0.ndim == 1:
            self.lf0 = self.lf0.reshape(-1, 1)

    def c_struct(self):
        u = F.TrackUtt()
        u.n_spectrum, u.n_lf0, u.n_lpf = len(self.spectrum), len(self.lf0), len(self.lpf)
        w = lambda a: int(a.shape[1]) if a.ndim == 2 else 0
        u.spectrum_width, u.lf0_width, u.lpf_width = w(self.spectrum), w(self.lf0), w(self.lpf)
        u.spectrum, u.lf0, u.lpf = _dp(self.spectrum), _dp(self.lf0), _dp(self.lpf)
        return u


# Batch(voc=VOC_NULL): jb_batch_create[_indexed]_voc with voc = NULL -- every utterance under the voice's own alpha,
# beta and volume, through the per-utterance entry
VOC_NULL = object()


class Batch:
    """A batch of utterances resident in HBM (jb_batch_*).  `utts` are state-level utterances
    (Utterance), or -- with `pdf_set` -- pdf row indices (IndexUtterance: the per-state Gaussians are
    gathered and blended on the device, jb_batch_create_indexed), or parameter tracks (TrackUtterance:
    jb_batch_create_from_tracks, the run starts at the vocoder's frame prologue).  mlpg_only=True: the run
    ends with the parameter tracks (JB_BATCH_MLPG_ONLY; read them with track()).  fast_invariant=True: each
    utterance's output bits depend on the utterance alone, not on the rest of the batch (JB_BATCH_INVARIANT)."""

    def __init__(self, voice: VoiceInfo, utts: Sequence[Utterance], device: int = -1,
                 keep_tracks: bool = False, generic_mlpg: bool = False, serial: bool = False,
                 chunk_frames: int = 0, warmup_frames: int = 0, verify_tol: float = 0.0,
                 kernel: str = "auto", serial_gv: bool = False, pcm_i16: bool = False,
                 pdf_set: Optional[PdfSet] = None, mlpg_only: bool = False,
                 test_gang_timeout: bool = False, no_exc_table: bool = False, voc=None,
                 fast_invariant: bool = False):
        L = F.lib()
        self._L = L
        self.voice = voice
        self._utts = list(utts)  # keep host arrays alive during create
        vd, keep = voice.c_struct()
        from_tracks = bool(self._utts) and isinstance(self._utts[0], TrackUtterance)
        ty = F.TrackUtt if from_tracks else F.IndexUtt if pdf_set is not None else F.StateUtt
        arr = (ty * max(1, len(utts)))()
        for i, u in enumerate(self._utts):
            arr[i] = u.c_struct()
        opts = F.BatchOpts()
        opts.device = device
        opts.flags = ((F.BATCH_KEEP_TRACKS if keep_tracks else 0) | (F.BATCH_GENERIC_MLPG if generic_mlpg else 0)
                      | (F.BATCH_SERIAL if serial else 0) | (F.BATCH_SERIAL_GV if serial_gv else 0)
                      | (F.BATCH_PCM_I16 if pcm_i16 else 0) | (F.BATCH_MLPG_ONLY if mlpg_only else 0)
                      | (F.BATCH_TEST_GANG_TIMEOUT if test_gang_timeout else 0)
                      | (F.BATCH_NO_EXC_TABLE if no_exc_table else 0)
                      | (F.BATCH_INVARIANT if fast_invariant else 0)
                      | {"auto": 0, "wave": F.BATCH_WAVE_KERNEL, "triple": F.BATCH_LANE_KERNEL}[kernel])
        opts.chunk_frames, opts.warmup_frames, opts.verify_tol = chunk_frames, warmup_frames, verify_tol
        self.flags, self.device = opts.flags | (F.BATCH_KEEP_TRACKS if mlpg_only else 0), device
        h = C.c_void_p()
        if voc is not None:
            # per-utterance vocoder conditions (jb_batch_create[_indexed]_voc): UttVoc or (alpha, beta, volume) each
            if from_tracks:
                raise ValueError("voc= takes state-level or indexed utterances")
            if voc is VOC_NULL:
                va = None
            elif len(voc) != len(self._utts):
                raise ValueError("voc= needs one entry per utterance")
            else:
                va = (F.UttVoc * max(1, len(voc)))()
                for i, v in enumerate(voc):
                    va[i] = v if isinstance(v, F.UttVoc) else F.UttVoc(*[float(x) for x in v])
            if pdf_set is not None:
                F.check(L.jb_batch_create_indexed_voc(C.byref(vd), pdf_set._h, arr, len(utts), va, C.byref(opts),
                                                      C.byref(h)))
            else:
                F.check(L.jb_batch_create_voc(C.byref(vd), arr, len(utts), va, C.byref(opts), C.byref(h)))
        elif from_tracks:
            F.check(L.jb_batch_create_from_tracks(C.byref(vd), arr, len(utts), C.byref(opts), C.byref(h)))
        elif pdf_set is not None:
            F.check(L.jb_batch_create_indexed(C.byref(vd), pdf_set._h, arr, len(utts), C.byref(opts), C.byref(h)))
        else:
            F.check(L.jb_batch_create(C.byref(vd), arr, len(utts), C.byref(opts), C.byref(h)))
        self._h = h
        self._keep = keep
        self._fbank = None  # the filterbank request the batch holds (set_fbank)
        self._mfcc = None   # the cepstral request the batch holds (set_mfcc): (FbankOpts, MfccOpts)
        self._melspec = None  # the mel spectrogram request the batch holds (set_melspec)
        self._pitch = None  # the pitch request the batch holds (set_pitch)

    def __len__(self):
        return self._L.jb_batch_size(self._h)

    def run(self):
        F.check(self._L.jb_batch_run(self._h))

    def sync(self):
        F.check(self._L.jb_batch_sync(self._h))

    def run_timed(self):
        t, v = C.c_float(), C.c_float()
        F.check(self._L.jb_batch_run_timed(self._h, C.byref(t), C.byref(v)))
        return t.value, v.value

    def last_timing(self):
        """(total_ms, vocoder_kernel_ms) of the last completed run (after sync())."""
        t, v = C.c_float(), C.c_float()
        F.check(self._L.jb_batch_last_timing(self._h, C.byref(t), C.byref(v)))
        return t.value, v.value

    def info(self):
        """(chunk_frames, warmup_frames, n_items, n_redo) of the last run."""
        v = [C.c_uint32() for _ in range(4)]
        F.check(self._L.jb_batch_info(self._h, *[C.byref(x) for x in v]))
        return dict(chunk_frames=v[0].value, warmup_frames=v[1].value, n_items=v[2].value, n_redo=v[3].value)

    def kernel_info(self):
        """(kernel name, waves per SIMD) of the vocoder kernel the work list was built for ("k_vocoder" stands for
        its two-wave form k_vocoder_pair as well, which launches of at most two chunks per CU take)."""
        lt, w = C.c_uint32(), C.c_uint32()
        F.check(self._L.jb_batch_kernel_info(self._h, C.byref(lt), C.byref(w)))
        return ("k_vocoder_lt" if lt.value else "k_vocoder"), w.value

    def num_samples(self, i):
        return self._L.jb_batch_num_samples(self._h, i)

    def num_frames(self, i):
        return self._L.jb_batch_num_frames(self._h, i)

    @property
    def total_samples(self):
        return self._L.jb_batch_total_samples(self._h)

    def pcm(self, i) -> np.ndarray:
        n = self.num_samples(i)
        out = np.empty(n, dtype=np.float64)
        F.check(self._L.jb_batch_read_pcm(self._h, i, out.ctypes.data, n))
        return out

    def pcm_i16(self, i) -> np.ndarray:
        """16-bit PCM of a batch created with pcm_i16=True (fused clamp + truncate sink)."""
        n = self.num_samples(i)
        out = np.empty(n, dtype=np.int16)
        F.check(self._L.jb_batch_read_pcm_i16(self._h, i, out.ctypes.data, n))
        return out

    def pcm_all(self, out: Optional[List[np.ndarray]] = None) -> List[np.ndarray]:
        """Every utterance's PCM through the staged whole-slab read (jb_batch_read_pcm_all /
        _i16_all); `out` re-uses caller buffers (already touched pages: the read then runs at link rate)."""
        i16 = bool(self.flags & F.BATCH_PCM_I16)
        dt = np.int16 if i16 else np.float64
        n = len(self)
        if out is None:
            out = [np.empty(self.num_samples(i), dtype=dt) for i in range(n)]
        ptrs = (C.c_void_p * max(1, n))(*[o.ctypes.data if o.size else None for o in out])
        fn = self._L.jb_batch_read_pcm_i16_all if i16 else self._L.jb_batch_read_pcm_all
        F.check(fn(self._h, ptrs))
        return out

    def set_output_rate(self, out_hz):
        """jb_batch_set_output_rate: one rate (int) for the whole batch or one per utterance; 0 or the voice's rate =
        native.  Before the first run only.  The PCM reads (pcm, pcm_i16, pcm_all, num_samples, device_pcm...) then
        hand out the converted audio."""
        rates = [int(out_hz)] if np.isscalar(out_hz) else [int(r) for r in out_hz]
        arr = (C.c_uint32 * max(1, len(rates)))(*rates)
        F.check(self._L.jb_batch_set_output_rate(self._h, arr, len(rates)))

    def set_filter(self, filters):
        """jb_batch_set_filter: one F.Filter for the whole batch or one per utterance (None in a list: no sections);
        None withdraws the request.  Before the first run only.  The stage runs behind the output rate and in front of
        the loudness target; pcm_native stays the unfiltered vocoder PCM."""
        if filters is None:
            F.check(self._L.jb_batch_set_filter(self._h, None, 0))
            return
        arr, n = F.filter_array(filters)
        F.check(self._L.jb_batch_set_filter(self._h, arr, n))

    def set_fir(self, firs):
        """jb_batch_set_fir: one F.Fir (J.fir(taps, hz, delay)) for the whole batch or one per utterance (None in a
        list: no response); None withdraws the request.  Before the first run.  The convolution runs behind the
        output rate and in front of the filter's sections; pcm_native stays the vocoder's PCM."""
        if firs is None:
            F.check(self._L.jb_batch_set_fir(self._h, None, 0))
            return
        arr, n = F.fir_array(firs)
        F.check(self._L.jb_batch_set_fir(self._h, arr, n))

    def set_room(self, rooms):
        """jb_batch_set_room: one F.Room (J.room(size, source, mic, rt60=..., hz=..., n_taps=...)) for the whole batch
        or one per utterance (None in a list: no room); None withdraws the request.  Before the first run.  The rooms'
        responses are generated on the batch's device in this call and installed in set_fir's place, advanced by the
        direct path's index; the later of set_room and set_fir replaces the earlier."""
        if rooms is None:
            F.check(self._L.jb_batch_set_room(self._h, None, 0))
            return
        arr, n = F.room_array(rooms)
        F.check(self._L.jb_batch_set_room(self._h, arr, n))

    def room_report(self, i):
        """jb_batch_room_report: the F.RoomReport of utterance i's room (direct index, delay, energy, DRR in dB)."""
        r = F.RoomReport()
        F.check(self._L.jb_batch_room_report(self._h, i, C.byref(r)))
        return r

    def set_noise(self, reqs):
        """jb_batch_set_noise: one F.Noise (J.noise(bed, hz, snr_db, ...)) for the whole batch or one per utterance
        (None in a list: no request); None withdraws the request.  Before the first run.  The noise is added behind
        the convolution and in front of the filter's sections; pcm_native stays the vocoder's PCM."""
        if reqs is None:
            F.check(self._L.jb_batch_set_noise(self._h, None, 0))
            return
        arr, n = F.noise_array(reqs)
        F.check(self._L.jb_batch_set_noise(self._h, arr, n))

    def noise_report(self, i):
        """jb_batch_noise_report: the F.NoiseReport of utterance i, after a run."""
        r = F.NoiseReport()
        F.check(self._L.jb_batch_noise_report(self._h, i, C.byref(r)))
        return r

    def fir_geometry(self, i):
        """jb_batch_fir_geometry: (mode, block, partitions) of utterance i's response."""
        m, b, p = C.c_uint32(), C.c_uint32(), C.c_uint32()
        F.check(self._L.jb_batch_fir_geometry(self._h, i, C.byref(m), C.byref(b), C.byref(p)))
        return m.value, b.value, p.value

    def filter_coefficients(self, i) -> np.ndarray:
        """jb_batch_filter_coefficients: [n_sections, 5] (b0 b1 b2 a1 a2) of what the device runs for utterance i at
        its output rate; [0, 5] without a filter."""
        out = (F.Biquad * F.FILTER_MAX_SECTIONS)()
        n = C.c_uint32()
        F.check(self._L.jb_batch_filter_coefficients(self._h, i, out, C.byref(n)))
        return F._biquads(out, n.value)

    def set_limiter(self, opts):
        """jb_batch_set_limiter: one F.LimiterOpts (J.limiter(...)) for the whole batch or one per utterance (None in a
        list: that utterance is not limited); None withdraws the request.  Before the first run only.  With a loudness
        target and a ceiling, the static gain may then put the highest peak max_reduction_db over the ceiling and the
        limiter holds the ceiling on the device."""
        if opts is None:
            F.check(self._L.jb_batch_set_limiter(self._h, None, 0))
            return
        arr, n = F.limiter_array(opts)
        F.check(self._L.jb_batch_set_limiter(self._h, arr, n))

    def limiter_report(self, i) -> dict:
        """jb_batch_limiter_report: max_reduction_db, limited_samples, lookahead and hold (samples) of utterance i."""
        rep = F.LimiterReport()
        F.check(self._L.jb_batch_limiter_report(self._h, i, C.byref(rep)))
        return rep.as_dict()

    def set_loudness_target(self, target_lufs, ceiling_dbfs=float("inf")):
        """jb_batch_set_loudness_target: one target (float) for the whole batch or one per utterance (NaN: measured,
        gain 0 dB unless above the ceiling).  Before the first run only.  The PCM reads then hand out x * gain."""
        ts = [float(target_lufs)] if np.isscalar(target_lufs) else [float(t) for t in target_lufs]
        arr = (C.c_double * max(1, len(ts)))(*ts)
        F.check(self._L.jb_batch_set_loudness_target(self._h, arr, len(ts), float(ceiling_dbfs)))

    def loudness(self, i):
        """(lufs, peak_dbfs, gain_db) the last run measured and applied for utterance i (jb_batch_loudness)."""
        v = [C.c_double(), C.c_double(), C.c_double()]
        F.check(self._L.jb_batch_loudness(self._h, i, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def set_peak_mode(self, mode):
        """jb_batch_set_peak_mode: what the ceiling bounds, F.PEAK_SAMPLE (0, the default) or F.PEAK_TRUE (1, dBTP);
        one mode (int) for the whole batch or one per utterance.  Before the first run only."""
        ms = [int(mode)] if np.isscalar(mode) else [int(m) for m in mode]
        arr = (C.c_uint32 * max(1, len(ms)))(*ms)
        F.check(self._L.jb_batch_set_peak_mode(self._h, arr, len(ms)))

    def set_loudness_groups(self, group):
        """jb_batch_set_loudness_groups: one group id (below the batch size) per utterance, None for an utterance of
        its own; group None withdraws the request.  The members of a group share one measurement and one gain."""
        if group is None:
            F.check(self._L.jb_batch_set_loudness_groups(self._h, None, 0))
            return
        ids = F._group_ids(group, len(group))
        F.check(self._L.jb_batch_set_loudness_groups(self._h, ids, len(group)))

    def loudness_group_of(self, i):
        """The dense group of utterance i (numbered by first member), -1 without a group request."""
        return int(self._L.jb_batch_loudness_group_of(self._h, i))

    def loudness_group(self, i):
        """jb_batch_loudness_group for the group of utterance i: a dict of lufs, sample_peak_dbfs, true_peak_dbtp,
        gain_db, peak_mode, oversampling, members, flags and r128 (filled with a report request)."""
        r = F.LoudnessGroupReport()
        F.check(self._L.jb_batch_loudness_group(self._h, i, C.byref(r)))
        return F._struct_dict(r)

    def set_loudness_report(self, flags=F.LOUDNESS_R128):
        """jb_batch_set_loudness_report: F.LOUDNESS_R128 asks for the R128 fields, 0 withdraws the request."""
        F.check(self._L.jb_batch_set_loudness_report(self._h, int(flags)))

    def loudness_r128(self, i):
        """jb_batch_loudness_r128 for utterance i: a dict of max_momentary_lufs, max_short_term_lufs, lra_lu,
        lra_low_lufs, lra_high_lufs and n_windows."""
        r = F.LoudnessR128()
        F.check(self._L.jb_batch_loudness_r128(self._h, i, C.byref(r)))
        return F._struct_dict(r)

    def loudness_report(self, i):
        """jb_batch_loudness_report for utterance i: a dict of lufs, sample_peak_dbfs, true_peak_dbtp (NaN in sample
        mode), gain_db, peak_mode and oversampling."""
        r = F.LoudnessReport()
        F.check(self._L.jb_batch_loudness_report(self._h, i, C.byref(r)))
        return {k: getattr(r, k) for k, _ in F.LoudnessReport._fields_}

    def set_flac(self, block_size: int = 0, max_lpc_order=None, md5: bool = False, seek_interval_ms: int = 0):
        """jb_batch_set_flac: the run also encodes each utterance's 16-bit output as a FLAC stream (pcm_i16=True,
        not mlpg_only; before the first run only).  Defaults: block size 4096, LPC order up to 8.  md5 /
        seek_interval_ms: set_flac_meta behind it."""
        opts = F.flac_opts(block_size, max_lpc_order)
        F.check(self._L.jb_batch_set_flac(self._h, C.byref(opts)))
        if md5 or seek_interval_ms:
            self.set_flac_meta(md5, seek_interval_ms)

    def set_flac_meta(self, md5: bool = False, seek_interval_ms: int = 0):
        """jb_batch_set_flac_meta: the streams carry the MD5 of their samples and / or a SEEKTABLE with a point about
        every seek_interval_ms (after set_flac, before the first run)."""
        meta = F.flac_meta(md5, seek_interval_ms) or F.FlacMeta()
        F.check(self._L.jb_batch_set_flac_meta(self._h, C.byref(meta)))

    # The byte sinks -- "flac", "formatted", "adpcm", "fbank", "mfcc", "melspec" -- are read through one path: the C entries are
    # jb_batch_<name>_size, jb_batch_read_<name> and jb_batch_read_<name>_all
    def _sink_size(self, name, i) -> int:
        n = C.c_size_t()
        F.check(getattr(self._L, f"jb_batch_{name}_size")(self._h, i, C.byref(n)))
        return n.value

    def _sink_read(self, name, i) -> bytes:
        n = self._sink_size(name, i)
        buf = np.empty(max(1, n), dtype=np.uint8)
        F.check(getattr(self._L, f"jb_batch_read_{name}")(self._h, i, buf.ctypes.data_as(C.POINTER(C.c_uint8)), n))
        return buf[:n].tobytes()

    def _sink_read_all(self, name) -> List[bytes]:
        B = self.num_outputs()
        ns = [self._sink_size(name, i) for i in range(B)]
        bufs = [np.empty(max(1, n), dtype=np.uint8) for n in ns]
        arr = (C.c_void_p * max(1, B))(*[b.ctypes.data for b in bufs])
        fn = getattr(self._L, f"jb_batch_read_{name}_all")
        F.check(fn(self._h, C.cast(arr, fn.argtypes[1])))  # (bound as uint8_t ** for FLAC, void ** for the others)
        return [b[:n].tobytes() for b, n in zip(bufs, ns)]

    def flac(self, i) -> bytes:
        """Utterance i's FLAC stream (jb_batch_flac_size + jb_batch_read_flac)."""
        return self._sink_read("flac", i)

    def flac_all(self) -> List[bytes]:
        """Every utterance's (with a join: every programme's) FLAC stream through one device-to-host copy
        (jb_batch_read_flac_all)."""
        return self._sink_read_all("flac")

    def set_format(self, fmt, dither=False, seed: int = 0):
        """jb_batch_set_format: the run also writes each utterance's final f64 PCM as bytes of a sample format --
        "f32", "s16", "s24", "ulaw" or "alaw"; dither=True: TPDF (s16 and s24) with `seed` -- on the GPU.  An f64
        batch (not pcm_i16, not mlpg_only), before the first run only."""
        opts = F.format_opts(fmt, dither, seed)
        F.check(self._L.jb_batch_set_format(self._h, C.byref(opts)))

    def formatted(self, i) -> bytes:
        """Utterance i's bytes in the batch's sample format (jb_batch_formatted_size + jb_batch_read_formatted)."""
        return self._sink_read("formatted", i)

    def formatted_all(self) -> List[bytes]:
        """Every utterance's (with a join: every programme's) formatted bytes through one device-to-host copy
        (jb_batch_read_formatted_all)."""
        return self._sink_read_all("formatted")

    def set_adpcm(self, block_align: int = 0):
        """jb_batch_set_adpcm: the run also encodes each utterance's final PCM as IMA ADPCM blocks (WAV tag 0x11) on
        the GPU.  block_align 0: by each utterance's output rate (256 / 512 / 1024), else a multiple of 4 in 32..8192.
        An f64 or a pcm_i16 batch (not mlpg_only), before the first run only."""
        opts = F.adpcm_opts(block_align)
        F.check(self._L.jb_batch_set_adpcm(self._h, C.byref(opts)))

    def adpcm_block_align(self, i) -> int:
        """Utterance i's block size A (jb_batch_adpcm_block_align)."""
        a = C.c_uint32()
        F.check(self._L.jb_batch_adpcm_block_align(self._h, i, C.byref(a)))
        return a.value

    def adpcm_size(self, i) -> int:
        return self._sink_size("adpcm", i)

    def read_adpcm(self, i) -> bytes:
        """Utterance i's IMA ADPCM blocks (jb_batch_adpcm_size + jb_batch_read_adpcm)."""
        return self._sink_read("adpcm", i)

    def read_adpcm_all(self) -> List[bytes]:
        """Every utterance's (with a join: every programme's) blocks through one device-to-host copy
        (jb_batch_read_adpcm_all)."""
        return self._sink_read_all("adpcm")

    def set_fbank(self, opts=None, **kw):
        """jb_batch_set_fbank: the run also turns each utterance's (with a join: each programme's) final f64 PCM into
        log-mel filterbank frames on the GPU.  opts: F.FbankOpts (J.fbank(...)), or the keywords of J.fbank; None
        without keywords withdraws the request.  An f64 batch (neither pcm_i16 nor mlpg_only), before the first run
        only."""
        if opts is None and kw:
            opts = F.fbank(**kw)
        F.check(self._L.jb_batch_set_fbank(self._h, C.byref(opts) if opts is not None else None))
        self._fbank = opts  # (a refused call leaves the batch's request, and this copy of it, as they were)

    def fbank_shape(self, i):
        """(T, n_mels, hz) of unit i's features (jb_batch_fbank_shape)."""
        T, m, hz = C.c_size_t(), C.c_uint32(), C.c_uint32()
        F.check(self._L.jb_batch_fbank_shape(self._h, i, C.byref(T), C.byref(m), C.byref(hz)))
        return T.value, m.value, hz.value

    def fbank_size(self, i) -> int:
        return self._sink_size("fbank", i)

    def read_fbank(self, i):
        """Unit i's features, an ndarray [T, n_mels] (jb_batch_fbank_size + jb_batch_read_fbank)."""
        return F.fbank_frames(self._sink_read("fbank", i), self._fbank)

    def read_fbank_all(self):
        """Every utterance's (with a join: every programme's) features through one device-to-host copy
        (jb_batch_read_fbank_all)."""
        return [F.fbank_frames(d, self._fbank) for d in self._sink_read_all("fbank")]

    def set_mfcc(self, opts=None, fbank=None, **kw):
        """jb_batch_set_mfcc: the run also turns each utterance's (with a join: each programme's) final f64 PCM into
        cepstral features on the GPU -- cepstra, deltas, CMVN -- behind a filterbank pass of their own.  opts:
        F.MfccOpts (J.mfcc(...)), or the keywords of J.mfcc; fbank: F.FbankOpts or a dict of J.fbank's keywords (None:
        the defaults) for the geometry.  None without keywords withdraws the request.  An f64 batch, before the first
        run only; independent of set_fbank."""
        if opts is None and not kw and fbank is None:
            F.check(self._L.jb_batch_set_mfcc(self._h, None, None))
            self._mfcc = None
            return
        fo, mo = F.mfcc_request(opts, fbank, kw)
        F.check(self._L.jb_batch_set_mfcc(self._h, C.byref(fo), C.byref(mo)))
        self._mfcc = (fo, mo)

    def set_frame(self, fr=None, **kw):
        """jb_batch_set_frame_opts: Kaldi-style frame conditioning (DC removal, pre-emphasis, the Povey and the other
        symmetric windows, reflected edges, the frame's log energy as c0) for set_fbank's and set_mfcc's features.
        fr: F.FrameOpts (J.frame(...)), or the keywords of J.frame; None without keywords withdraws the request.
        Before the first run, in either order with set_fbank / set_mfcc."""
        if fr is None and kw:
            fr = F.frame(**kw)
        F.check(self._L.jb_batch_set_frame_opts(self._h, C.byref(fr) if fr is not None else None))

    def mfcc_shape(self, i):
        """(T, width, hz) of unit i's rows (jb_batch_mfcc_shape)."""
        T, w, hz = C.c_size_t(), C.c_uint32(), C.c_uint32()
        F.check(self._L.jb_batch_mfcc_shape(self._h, i, C.byref(T), C.byref(w), C.byref(hz)))
        return T.value, w.value, hz.value

    def mfcc_size(self, i) -> int:
        return self._sink_size("mfcc", i)

    def read_mfcc(self, i):
        """Unit i's rows, an ndarray [T, width] (jb_batch_mfcc_size + jb_batch_read_mfcc)."""
        return F.mfcc_rows(self._sink_read("mfcc", i), self._mfcc[1], self._mfcc[0].n_mels)

    def read_mfcc_all(self):
        """Every utterance's (with a join: every programme's) rows through one device-to-host copy
        (jb_batch_read_mfcc_all)."""
        return [F.mfcc_rows(d, self._mfcc[1], self._mfcc[0].n_mels) for d in self._sink_read_all("mfcc")]

    def set_melspec(self, opts=None, **kw):
        """jb_batch_set_melspec: the run also turns each utterance's (with a join: each programme's) final f64 PCM into
        a mel spectrogram in the librosa / Whisper convention on the GPU.  opts: F.MelspecOpts (J.melspec(...),
        J.whisper_mel(...)), or the keywords of J.melspec; None without keywords withdraws the request.  An f64 batch
        (neither pcm_i16 nor mlpg_only), before the first run only; independent of set_fbank and set_mfcc."""
        if opts is None and kw:
            opts = F.melspec(**kw)
        F.check(self._L.jb_batch_set_melspec(self._h, C.byref(opts) if opts is not None else None))
        self._melspec = opts  # (a refused call leaves the batch's request, and this copy of it, as they were)

    def set_pitch(self, opts=None, **kw):
        """jb_batch_set_pitch: the run also tracks the pitch features of each utterance's (behind a join or mix: each
        programme's and stem's) final f64 PCM on the GPU.  opts: F.PitchOpts (J.kaldi_pitch(), J.pitch(...)), or the
        keywords of J.pitch; None without keywords withdraws the request.  An f64 batch only; before the first run."""
        if opts is None and kw:
            opts = F.pitch(**kw)
        F.check(self._L.jb_batch_set_pitch(self._h, C.byref(opts) if opts is not None else None))
        self._pitch = opts  # (a refused call leaves the batch's request, and this copy of it, as they were)

    def pitch_shape(self, i):
        """(T, width, hz) of unit i's pitch features (jb_batch_pitch_shape)."""
        T, w, hz = C.c_size_t(), C.c_uint32(), C.c_uint32()
        F.check(self._L.jb_batch_pitch_shape(self._h, i, C.byref(T), C.byref(w), C.byref(hz)))
        return T.value, w.value, hz.value

    def pitch_size(self, i) -> int:
        return self._sink_size("pitch", i)

    def read_pitch(self, i):
        """Unit i's pitch features, an ndarray [T, width] (jb_batch_pitch_size + jb_batch_read_pitch)."""
        return F.pitch_frames(self._sink_read("pitch", i), self._pitch)

    def read_pitch_all(self):
        """Every unit's pitch features through one device-to-host copy (jb_batch_read_pitch_all)."""
        return [F.pitch_frames(d, self._pitch) for d in self._sink_read_all("pitch")]

    def melspec_shape(self, i):
        """(T, n_mels, hz) of unit i's mel spectrogram (jb_batch_melspec_shape)."""
        T, m, hz = C.c_size_t(), C.c_uint32(), C.c_uint32()
        F.check(self._L.jb_batch_melspec_shape(self._h, i, C.byref(T), C.byref(m), C.byref(hz)))
        return T.value, m.value, hz.value

    def melspec_size(self, i) -> int:
        return self._sink_size("melspec", i)

    def read_melspec(self, i):
        """Unit i's mel spectrogram, an ndarray [T, n_mels] (jb_batch_melspec_size + jb_batch_read_melspec)."""
        return F.melspec_frames(self._sink_read("melspec", i), self._melspec)

    def read_melspec_all(self):
        """Every utterance's (with a join: every programme's) mel spectrogram through one device-to-host copy
        (jb_batch_read_melspec_all)."""
        return [F.melspec_frames(d, self._melspec) for d in self._sink_read_all("melspec")]

    def set_activity(self, opts=None, **kw):
        """jb_batch_set_activity: the run also measures per-frame speech-activity labels on the GPU, a uint8 [T, C]
        matrix per unit (an utterance; with a join or mix request a programme), one column per member
        (columns="members") or one for the unit (columns="unit"): a side output beside whatever sinks the batch has.
        opts: F.ActivityOpts (J.activity(...)), or the keywords of J.activity; None without keywords withdraws the
        request.  Before the first run only."""
        if opts is None and kw:
            opts = F.activity(**kw)
        F.check(self._L.jb_batch_set_activity(self._h, C.byref(opts) if opts is not None else None))

    def activity_shape(self, i):
        """(T, C, hz) of unit i's label matrix (jb_batch_activity_shape)."""
        T, c, hz = C.c_uint64(), C.c_uint32(), C.c_uint32()
        F.check(self._L.jb_batch_activity_shape(self._h, i, C.byref(T), C.byref(c), C.byref(hz)))
        return T.value, c.value, hz.value

    def read_activity(self, i) -> np.ndarray:
        """Unit i's labels, uint8 [T, C] (jb_batch_activity_size + jb_batch_read_activity)."""
        T, c, _ = self.activity_shape(i)
        n = C.c_size_t()
        F.check(self._L.jb_batch_activity_size(self._h, i, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        F.check(self._L.jb_batch_read_activity(self._h, i, out.ctypes.data, n.value))
        return out[:n.value].reshape(T, c)

    def read_activity_all(self):
        """Every unit's labels through one device-to-host copy (jb_batch_read_activity_all)."""
        # (the stems of a mix are no units of this stage: it keeps the programmes)
        shapes = [self.activity_shape(i)[:2] for i in range(self.num_programmes())]
        outs = [np.zeros(max(T * c, 1), dtype=np.uint8) for T, c in shapes]
        ptrs = (C.c_void_p * max(1, len(outs)))(*[o.ctypes.data for o in outs])
        F.check(self._L.jb_batch_read_activity_all(self._h, ptrs))
        return [o[:T * c].reshape(T, c) for o, (T, c) in zip(outs, shapes)]

    def activity_report(self, i, col=0):
        """jb_batch_activity_report: the F.ActivityReport of column col of unit i, after a run."""
        r = F.ActivityReport()
        F.check(self._L.jb_batch_activity_report(self._h, i, col, C.byref(r)))
        return r

    def activity_unit_report(self, i):
        """jb_batch_activity_unit_report: the F.ActivityUnitReport of unit i, after a run."""
        r = F.ActivityUnitReport()
        F.check(self._L.jb_batch_activity_unit_report(self._h, i, C.byref(r)))
        return r

    def set_join(self, req):
        """jb_batch_set_join: one request per utterance -- F.JoinUtt entries, or (programme, pad_before, pad_after,
        fade_in, fade_out) tuples with programme None for an utterance of its own, in samples at the output rate; None
        withdraws the request.  The run then gathers the final PCM into programmes on the GPU, and flac(i),
        formatted(i) and read_adpcm(i) (and their _all forms) index programmes.  Before the first run only."""
        if req is None:
            F.check(self._L.jb_batch_set_join(self._h, None, 0))
            return
        F.check(self._L.jb_batch_set_join(self._h, F.join_request(req), len(req)))

    def set_mix(self, req, fit: bool = False, ceiling_db: float = 0.0):
        """jb_batch_set_mix: one request per utterance -- F.MixUtt entries, or (programme, start, gain_db, pad_after,
        fade_in, fade_out) tuples with programme None for an utterance of its own, in samples at the output rate; None
        withdraws the request.  The run then sums the final PCM into programmes on the GPU, in the join's place: a
        batch holds a join or a mix request.  fit: a programme over ceiling_db (dBFS) is scaled down to it."""
        if req is None:
            F.check(self._L.jb_batch_set_mix(self._h, None, 0, None))
            return
        o = F.mix_opts(fit, ceiling_db)
        F.check(self._L.jb_batch_set_mix(self._h, F.mix_request(req), len(req), C.byref(o)))

    def mix_report(self, p):
        """jb_batch_mix_report: the F.MixReport of programme p, after a run."""
        r = F.MixReport()
        F.check(self._L.jb_batch_mix_report(self._h, p, C.byref(r)))
        return r

    def set_mix_stems(self, stem_of, levels: bool = False):
        """jb_batch_set_mix_stems, behind set_mix and before the first run: stem_of[u] is utterance u's stem id within
        its programme, or None for no stem; members of one programme with the same id form one stem, a unit behind the
        programmes (num_outputs is then P + S).  levels: the three sums and the dB values of stem_report.  None
        withdraws the request."""
        if stem_of is None:
            F.check(self._L.jb_batch_set_mix_stems(self._h, None, 0, 0))
            return
        F.check(self._L.jb_batch_set_mix_stems(self._h, F.stem_ids(stem_of), len(stem_of),
                                               F.MIX_STEM_LEVELS * bool(levels)))

    def num_programmes(self) -> int:
        """P: the programmes among the outputs (jb_batch_num_programmes); the stems follow them."""
        return self._L.jb_batch_num_programmes(self._h)

    def stem_unit(self, u) -> int:
        """The unit of utterance u's stem, or -1 (jb_batch_stem_unit)."""
        return int(self._L.jb_batch_stem_unit(self._h, u))

    def stem_layout(self, unit):
        """(programme, stem_id, members, first_sample, end_sample) of a stem's unit (jb_batch_stem_layout)."""
        p, i, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
        a, e = C.c_uint64(), C.c_uint64()
        F.check(self._L.jb_batch_stem_layout(self._h, unit, C.byref(p), C.byref(i), C.byref(m), C.byref(a), C.byref(e)))
        return p.value, i.value, m.value, a.value, e.value

    def stem_report(self, unit):
        """jb_batch_stem_report: the F.StemReport of a stem's unit, after a run."""
        r = F.StemReport()
        F.check(self._L.jb_batch_stem_report(self._h, unit, C.byref(r)))
        return r

    def num_outputs(self) -> int:
        """What the encoders' entries index: the utterances; with a join or mix request the P programmes, and with
        a stems request behind a mix the P programmes and the S stems behind them (P + S)."""
        return self._L.jb_batch_num_outputs(self._h)

    def programme_of(self, i) -> int:
        """The programme of utterance i (numbered by first member), -1 without a join request."""
        return int(self._L.jb_batch_programme_of(self._h, i))

    def programme_layout(self, p):
        """(members, samples, rate) of programme p (jb_batch_programme_layout)."""
        m, n, hz = C.c_size_t(), C.c_uint64(), C.c_uint32()
        F.check(self._L.jb_batch_programme_layout(self._h, p, C.byref(m), C.byref(n), C.byref(hz)))
        return m.value, n.value, hz.value

    def member_start(self, i) -> int:
        """The first sample of utterance i within its programme (jb_batch_member_start): the cue list."""
        k = C.c_uint64()
        F.check(self._L.jb_batch_member_start(self._h, i, C.byref(k)))
        return k.value

    def programme_pcm(self, p) -> np.ndarray:
        """The PCM of programme p: float64, or int16 on a pcm_i16 batch (jb_batch_read_programme_pcm / _i16)."""
        i16 = bool(self.flags & F.BATCH_PCM_I16)
        n = self.programme_layout(p)[1]
        out = np.empty(n, dtype=np.int16 if i16 else np.float64)
        fn = self._L.jb_batch_read_programme_pcm_i16 if i16 else self._L.jb_batch_read_programme_pcm
        F.check(fn(self._h, p, out.ctypes.data, n))
        return out

    def output_rate(self, i) -> int:
        """Rate of utterance i's PCM as the read entries hand it out (the voice's rate when native)."""
        return self._L.jb_batch_output_rate(self._h, i)

    def pcm_native(self, i) -> np.ndarray:
        """The vocoder's f64 PCM of utterance i at the voice's rate (jb_batch_read_pcm_native)."""
        n = self.num_frames(i) * self.voice.fperiod
        out = np.empty(n, dtype=np.float64)
        F.check(self._L.jb_batch_read_pcm_native(self._h, i, out.ctypes.data, n))
        return out

    def track(self, i, stream) -> np.ndarray:
        T, Lv = self.num_frames(i), self.voice.streams[stream].vector_length
        out = np.empty((T, Lv), dtype=np.float64)
        F.check(self._L.jb_batch_read_track(self._h, i, stream, out.ctypes.data, out.size))
        return out

    def coefficients(self, i) -> np.ndarray:
        """MLSA filter coefficients per frame, mc2b(postfilter_mcp(spectrum)) (vocoder/mod.rs:116-118)."""
        T, Lv = self.num_frames(i), self.voice.streams[0].vector_length
        out = np.empty((T, Lv), dtype=np.float64)
        F.check(self._L.jb_batch_read_coefficients(self._h, i, out.ctypes.data, out.size))
        return out

    def first_coefficients(self, i) -> np.ndarray:
        """The coefficients frame 0 starts from (un-filtered spectrum when a post-filter / stage is on)."""
        Lv = self.voice.streams[0].vector_length
        out = np.zeros(Lv, dtype=np.float64)
        F.check(self._L.jb_batch_read_first_coefficients(self._h, i, out.ctypes.data, out.size))
        return out

    def excitation(self, i) -> np.ndarray:
        n = self.num_frames(i) * self.voice.fperiod  # at the voice's rate, output rate or not
        out = np.empty(n, dtype=np.float64)
        F.check(self._L.jb_batch_read_excitation(self._h, i, out.ctypes.data, n))
        return out

    def redo_stats(self):
        """(settled at the checkpoint, recomputed to the end) of the chunks that failed the hand-off check."""
        a, b = C.c_uint32(), C.c_uint32()
        F.check(self._L.jb_batch_redo_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def gang_fallbacks(self) -> int:
        """Times the resident GV kernel timed out in formation and the multi-launch sweeps took over."""
        return self._L.jb_batch_gang_fallbacks(self._h)

    def device_pcm(self):
        n = C.c_size_t()
        p = self._L.jb_batch_device_pcm(self._h, C.byref(n))
        return p, n.value

    def pcm_offset(self, i):
        return self._L.jb_batch_pcm_offset(self._h, i)

    def close(self):
        if getattr(self, "_h", None):
            self._L.jb_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def mlpg_batch(voice: VoiceInfo, utts: Sequence[Utterance], device: int = -1, serial_gv: bool = False):
    """jb_mlpg_batch = MlpgAdjust::create for every stream of every utterance (mlpg_adjust/mod.rs:31-51):
    returns [[track of stream 0, 1, 2] per utterance], each [T][L] (NODATA in unvoiced LF0 frames)."""
    L = F.lib()
    vd, keep = voice.c_struct()
    arr = (F.StateUtt * max(1, len(utts)))()
    for i, u in enumerate(utts):
        arr[i] = u.c_struct()
    ns = len(voice.streams)
    nfr = (C.c_size_t * max(1, len(utts)))()
    opts = F.BatchOpts()
    opts.device, opts.flags = device, (F.BATCH_SERIAL_GV if serial_gv else 0)
    F.check(L.jb_mlpg_batch(C.byref(vd), arr, len(utts), C.byref(opts), None, nfr))
    out = [[np.empty((nfr[i], voice.streams[s].vector_length)) for s in range(ns)] for i in range(len(utts))]
    ptrs = (C.POINTER(C.c_double) * max(1, len(utts) * ns))(*[_dp(t) for u in out for t in u])
    F.check(L.jb_mlpg_batch(C.byref(vd), arr, len(utts), C.byref(opts), ptrs, nfr))
    del keep
    return out


def vocode_tracks_batch(voice: VoiceInfo, utts: Sequence["TrackUtterance"], device: int = -1):
    """jb_vocode_tracks_batch = SpeechGenerator::new + generate_all on given parameter tracks
    (speech.rs:25-50,87-96): a list of f64 PCM arrays."""
    L = F.lib()
    vd, keep = voice.c_struct()
    arr = (F.TrackUtt * max(1, len(utts)))()
    for i, u in enumerate(utts):
        arr[i] = u.c_struct()
    ns = (C.c_size_t * max(1, len(utts)))()
    opts = F.BatchOpts()
    opts.device = device
    F.check(L.jb_vocode_tracks_batch(C.byref(vd), arr, len(utts), C.byref(opts), None, ns))
    out = [np.empty(ns[i], dtype=np.float64) for i in range(len(utts))]
    ptrs = (C.POINTER(C.c_double) * max(1, len(utts)))(*[_dp(o) for o in out])
    F.check(L.jb_vocode_tracks_batch(C.byref(vd), arr, len(utts), C.byref(opts), ptrs, ns))
    del keep
    return out


def vocoder_synthesize_batch(voice: VoiceInfo, utts: Sequence["TrackUtterance"], device: int = -1):
    """jb_vocoder_synthesize_batch = Vocoder::new + Vocoder::synthesize per frame (vocoder/mod.rs:45-178): like
    vocode_tracks_batch without SpeechGenerator::new's LPF checks, so that nlpf == 0 (voice.streams[2]
    .vector_length == 0, lpf tracks of width 0) reaches Excitation::get's ring-buffer-less branch."""
    L = F.lib()
    vd, keep = voice.c_struct()
    arr = (F.TrackUtt * max(1, len(utts)))()
    for i, u in enumerate(utts):
        arr[i] = u.c_struct()
    ns = (C.c_size_t * max(1, len(utts)))()
    opts = F.BatchOpts()
    opts.device = device
    F.check(L.jb_vocoder_synthesize_batch(C.byref(vd), arr, len(utts), C.byref(opts), None, ns))
    out = [np.empty(ns[i], dtype=np.float64) for i in range(len(utts))]
    ptrs = (C.POINTER(C.c_double) * max(1, len(utts)))(*[_dp(o) for o in out])
    F.check(L.jb_vocoder_synthesize_batch(C.byref(vd), arr, len(utts), C.byref(opts), ptrs, ns))
    del keep
    return out


def generator_from_tracks(voice: VoiceInfo, utt: "TrackUtterance", device: int = -1):
    """jb_generator_new_from_tracks = SpeechGenerator::new on caller-held tracks (speech.rs:25-50); step it with
    generate_step / generate_steps / generate_all."""
    from .engine import SpeechGenerator

    L = F.lib()
    vd, keep = voice.c_struct()
    arr = (F.TrackUtt * 1)()
    arr[0] = utt.c_struct()
    opts = F.BatchOpts()
    opts.device = device
    h = C.c_void_p()
    F.check(L.jb_generator_new_from_tracks(C.byref(vd), arr, C.byref(opts), C.byref(h)))
    g = SpeechGenerator(h, L)
    g._keep = (keep, utt)
    return g


def paramgen_vocode_batch(voice: VoiceInfo, utts: Sequence[Utterance], device: int = -1,
                          devices: Optional[Sequence[int]] = None):
    """One-shot jb_paramgen_vocode_batch: returns a list of f64 PCM arrays.  With `devices` the batch
    goes through jb_paramgen_vocode_batch_multi: LPT split by frames over the listed GPUs, one host
    thread per device (a device may be listed more than once)."""
    if devices is None:
        with Batch(voice, utts, device=device) as b:
            b.run()
            b.sync()
            return [b.pcm(i) for i in range(len(utts))]
    L = F.lib()
    vd, keep = voice.c_struct()
    arr = (F.StateUtt * max(1, len(utts)))()
    for i, u in enumerate(utts):
        arr[i] = u.c_struct()
    fp = voice.fperiod
    out = [np.empty(int(u.durations.sum()) * fp, dtype=np.float64) for u in utts]
    ptrs = (C.POINTER(C.c_double) * max(1, len(utts)))(*[_dp(o) for o in out])
    ns = (C.c_size_t * max(1, len(utts)))()
    dv = (C.c_int32 * max(1, len(devices)))(*[int(d) for d in devices])
    F.check(L.jb_paramgen_vocode_batch_multi(C.byref(vd), arr, len(utts), None, dv, len(devices), ptrs, ns))
    assert all(ns[i] == len(out[i]) for i in range(len(utts)))
    del keep
    return out

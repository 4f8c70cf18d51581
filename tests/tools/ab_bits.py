"""Bitwise A/B aid: SHA-256 of the MCP/LF0 tracks and the PCM of fixed batches, to compare two builds of the
library (swap jbonsai_amd/libjbonsai_amd.so between runs): a mid-size batch of label utterances (wave
kernel), and 8 x the 25,546-frame synthetic utterance + 3 distinct ones (lane-triple kernel, resident GV,
LDS-staged band solve, split excitation: the kernels of BASELINE config 2), f64 and the 16-bit sink.  Then the
stages behind the vocoder: all eight rows of the output routing table (f64 / 16-bit sink x output
rate x loudness target; FLAC on the 16-bit rows) on three ragged utterances, with the default geometry and with the
redo-heavy one of the redo tests (each row with the run's redo counters), and the entries on caller-held PCM on seeded input: three on long inputs, then
every one of their bodies on utterances of 0, 1, 1,025 and 5,000 samples -- the spectral stages (filterbank, cepstra,
mel spectrogram) at every transform size class and both element types, the framed filterbank and cepstral entries
(the all-zero frame request, every option alone, the Kaldi preset) at one small and one large class, the convolution
in direct mode and at both partitioned transform sizes, the noise stage -- and the host halves of the spectral stages,
the framed ones included, which need no device.

    python tests/tools/ab_bits.py               every hash (what tools/ab_bits.sh compares between two libraries)
    python tests/tools/ab_bits.py --seams       the hashes of the entries on caller-held PCM alone
    python tests/tools/ab_bits.py --host        the hashes of the spectral stages' host halves alone (no device)
    python tests/tools/ab_bits.py --redo-time N  no hash: run() + sync() of the redo-heavy rows, wall ms, N times each"""
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.conftest import VOICE  # noqa: E402
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2  # noqa: E402
from tests.helpers import oracle_states, to_utt, voice_info  # noqa: E402

redo_time = int(sys.argv[sys.argv.index("--redo-time") + 1]) if "--redo-time" in sys.argv else 0


def digest(arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


FB_FFT = (64, 128, 512, 2048, 4096)
ML_FFT = (64, 96, 400, 1024, 1200, 4000)
SPEC_HZ = 16000


def fbank_opts(N, f64):
    """A window of N samples at SPEC_HZ every N / 4, transformed at n_fft = N."""
    return J.fbank(win_ms=1e3 * N / SPEC_HZ, hop_ms=250.0 * N / SPEC_HZ, n_fft=N, n_mels=10 if N < 256 else 40, f64=f64)


def melspec_cases(f64):
    for N in ML_FFT:
        for scale, norm in (("htk", "none"), ("slaney", "slaney")):
            for rng in (0.0, 8.0):
                yield (N, scale, rng), J.melspec(n_fft=N, hop=N // 4, n_mels=10 if N < 256 else 40, mel_scale=scale,
                                                 norm=norm, range=rng, f64=f64)


FR_FFT = (64, 2048)  # the framed entries: one small and one large transform class
SEAM_LENGTHS = (0, 1, 1025, 5000)


def frame_cases(cepstra):
    """The frame requests of the framed entries: the all-zero one, every option alone and the Kaldi preset's
    (JB_FRAME_ENERGY stands behind a cepstral request only)."""
    yield "zero", J.frame()
    yield "remove_dc", J.frame(remove_dc=True)
    yield "preemph", J.frame(preemph=0.97)
    yield "povey", J.frame(window="povey")
    yield "reflect", J.frame(reflect=True)
    if cepstra:
        yield "energy", J.frame(energy=True)
    yield "kaldi", J.kaldi_frame()[1]


def seam_mfcc(f64):
    return J.mfcc(n_ceps=8, delta_order=1, cmvn="mean_var", f64=f64)


def host_framed_bits():
    """jb_fbank_framed_host and jb_mfcc_framed_pcm_host at the seams' lengths, both element types."""
    rng = np.random.default_rng(1025)
    pcm = [9000.0 * rng.standard_normal(n) for n in SEAM_LENGTHS]
    for N in FR_FFT:
        for f64 in (False, True):
            for name, fr in frame_cases(True):
                row = ["host framed", N, "f64" if f64 else "f32", name]
                if name != "energy":
                    row += [digest([J.fbank_framed_host(x, SPEC_HZ, fbank_opts(N, f64), fr) for x in pcm])]
                row += ["mfcc", digest([J.mfcc_framed_pcm_host(x, SPEC_HZ, fbank_opts(N, False), seam_mfcc(f64), fr)
                                        for x in pcm])]
                print(*row)
    kf, kfr = J.kaldi_frame()
    print("host framed kaldi preset", digest([J.fbank_framed_host(x, SPEC_HZ, kf, kfr) for x in pcm]), "mfcc",
          digest([J.mfcc_framed_pcm_host(x, SPEC_HZ, kf, J.mfcc(), kfr) for x in pcm]))


def framed_seams(pcm):
    """fbank_framed_pcm and mfcc_framed_pcm under every frame request, both element types."""
    for N in FR_FFT:
        for f64 in (False, True):
            for name, fr in frame_cases(True):
                row = ["seam framed", N, "f64" if f64 else "f32", name]
                if name != "energy":
                    row += [digest(J.fbank_framed_pcm(pcm, SPEC_HZ, fbank_opts(N, f64), fr))]
                print(*row, "mfcc", digest(J.mfcc_framed_pcm(pcm, SPEC_HZ, fbank_opts(N, False), seam_mfcc(f64), fr)))
    kf, kfr = J.kaldi_frame()
    print("seam framed kaldi preset", digest(J.fbank_framed_pcm(pcm, SPEC_HZ, kf, kfr)), "mfcc",
          digest(J.mfcc_framed_pcm(pcm, SPEC_HZ, kf, J.mfcc(), kfr)))


def host_bits():
    """The host halves of the spectral stages on seeded input: windows, dense filterbanks and frames."""
    host_framed_bits()
    x = 9000.0 * np.random.default_rng(64).standard_normal(3 * 4096 + 17)
    for N in FB_FFT:
        o = fbank_opts(N, True)
        print("host fbank", N, digest([J.fbank_window(SPEC_HZ, o)]), digest([J.fbank_filterbank(SPEC_HZ, o)]),
              digest([J.fbank_host(x, SPEC_HZ, o)]), digest([J.fbank_host(x, SPEC_HZ, fbank_opts(N, False))]))
    for key, o in melspec_cases(True):
        print("host melspec", *key, digest([J.melspec_window(SPEC_HZ, o)]), digest([J.melspec_filterbank(SPEC_HZ, o)]),
              digest([J.melspec_host(x, SPEC_HZ, o)]))
    print("host mfcc", digest([J.mfcc_pcm_host(x, SPEC_HZ, J.fbank(), J.mfcc())]))


def spectral_seams(pcm):
    """fbank_pcm, mfcc_pcm and melspec_pcm at every transform size, f32 and f64 elements; fir_pcm in direct mode and at
    both partitioned transform sizes, f64 and the 16-bit sink; noise_pcm."""
    rng = np.random.default_rng(950)
    pcm = pcm + [9000.0 * rng.standard_normal(48000)]  # (several workgroups at every transform size)
    for f64 in (False, True):
        for N in FB_FFT:
            o = fbank_opts(N, f64)
            print("seam fbank", N, "f64" if f64 else "f32", digest(J.fbank_pcm(pcm, SPEC_HZ, o)), "mfcc",
                  digest(J.mfcc_pcm(pcm, SPEC_HZ, fbank_opts(N, False), seam_mfcc(f64))))
        for key, o in melspec_cases(f64):
            print("seam melspec", *key, "f64" if f64 else "f32", digest(J.melspec_pcm(pcm, SPEC_HZ, o)))
    framed_seams(pcm)
    for K in (256, 257, 2049, 5000):
        f = J.fir(rng.standard_normal(K) / np.sqrt(K), SPEC_HZ, delay=K // 3)
        print("seam fir", K, digest(J.fir_pcm(pcm, f, SPEC_HZ)), "i16", digest(J.fir_pcm(pcm, f, SPEC_HZ, i16=True)))
    y, rep = J.noise_pcm(pcm, J.noise(snr_db=15.0, seed=3), SPEC_HZ)
    print("seam noise", digest(y), digest([bytes(r) for r in rep]))


def pcm_seams():
    """Every body behind the jb_*_pcm_batch entries (f64 and 16-bit instances) on seeded utterances."""
    rng = np.random.default_rng(1025)
    pcm = [9000.0 * rng.standard_normal(n) for n in SEAM_LENGTHS]
    pcm16 = [np.clip(x, -32768, 32767).astype(np.int16) for x in pcm]
    print("seam resample", digest(J.resample(pcm, 48000, 16000)), digest(J.resample(pcm, 48000, 48000)))
    print("seam loudness", digest([np.array(J.loudness(pcm, 48000))]), "true_peak",
          digest([np.array(J.true_peak(pcm, 48000))]), "groups",
          digest([repr(J.loudness_groups(pcm, 48000, [1, 1, None, 1], mode=1, target=-23.0, ceiling=-1.0)).encode()]))
    print("seam flac", digest(J.flac_encode(pcm16, 48000)), "meta",
          digest(J.flac_encode(pcm16, 22050, block_size=1152, md5=True, seek_interval_ms=10)), "md5",
          digest(J.flac_md5(pcm16)))
    print("seam format",
          *[digest(J.format_pcm(pcm, f, dither=f == "s24", seed=7)) for f in ("alaw", "f32", "s16", "s24", "ulaw")])
    print("seam adpcm", digest(J.adpcm_encode(pcm, [8000, 16000, 22050, 48000])))
    req = [(0, 3, 0, 0, 0), (0, 0, 5, 0, 0), (None, 0, 0, 64, 64), (0, 7, 7, 100, 100)]
    print("seam join", digest(J.join_pcm(pcm, req)), "i16", digest(J.join_pcm(pcm16, req)))
    filt = [J.highpass(120.0), None, J.telephone_band(), J.highpass(80.0) + J.peaking(2500.0, 3.0)]
    print("seam filter", digest(J.filter_pcm(pcm, filt, [48000, 48000, 8000, 16000])), "i16",
          digest(J.filter_pcm(pcm, filt, [48000, 48000, 8000, 16000], i16=True)))
    for i16 in (False, True):
        y, rep = J.limiter_pcm(pcm, [48000, 16000, 48000, 22050], 2.0, -1.0, [0, 0, 1, 1], i16=i16)
        print("seam limiter", "i16" if i16 else "f64", digest(y), digest([repr(rep).encode()]))
    spectral_seams(pcm)


def output_rows(vi, utts, geometry, label):
    """Every row of the routing table: what the read entries return (per utterance and _all), pcm_native where there
    is one, jb_batch_loudness' values, the FLAC streams (non-default block size and LPC order)."""
    B = len(utts)
    for i16 in (False, True):
        for rates in (None, [22050, 16000, 0], [96000] * B):
            for target in (None, [-20.0, -26.0, float("nan")]):
                name = f"{label} {'i16' if i16 else 'f64'} rate={rates} target={target}"
                with J.Batch(vi, utts, pcm_i16=i16, **geometry) as b:
                    if rates:
                        b.set_output_rate(rates)
                    if target:
                        b.set_loudness_target(target, -1.0)
                    if i16:
                        b.set_flac(block_size=1152, max_lpc_order=12)
                    if redo_time:
                        ms = []
                        for _ in range(redo_time):
                            t0 = time.perf_counter()
                            b.run()
                            b.sync()
                            ms.append(1e3 * (time.perf_counter() - t0))
                        print(name, "n_redo", b.info()["n_redo"], "redo_stats", b.redo_stats(), "run+sync ms",
                              " ".join(f"{x:.3f}" for x in ms))
                        continue
                    b.run()
                    b.sync()
                    read = b.pcm_i16 if i16 else b.pcm
                    out = [name, "n_redo", b.info()["n_redo"], "redo_stats", b.redo_stats(),
                           "n", [b.num_samples(i) for i in range(B)],
                           "hz", [b.output_rate(i) for i in range(B)], "off", [b.pcm_offset(i) for i in range(B + 1)],
                           "pcm", digest([read(i) for i in range(B)]), "all", digest(b.pcm_all())]
                    if not i16 or rates or target:
                        out += ["native", digest([b.pcm_native(i) for i in range(B)])]
                    if target:
                        out += ["loudness", digest([np.array(b.loudness(i)) for i in range(B)])]
                    if i16:
                        out += ["flac", digest([b.flac(i) for i in range(B)]), "flac_all", digest(b.flac_all())]
                    print(*out)


def output_stages():
    eng = J.Engine.load([VOICE])
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 40 + T) for T in (600, 1100, 37)]
    if not redo_time:
        output_rows(vi, utts, {}, "default")
    output_rows(vi, utts, dict(chunk_frames=96, warmup_frames=2, verify_tol=1e-12), "redo")
    if redo_time:
        return
    rng = np.random.default_rng(20240)
    pcm = [8000.0 * rng.standard_normal(n) * np.sin(np.arange(n) * 0.01) for n in (48000, 0, 131071, 777)]
    for hz in (16000, 22050, 96000):
        print("resample_pcm_batch", hz, digest(J.resample(pcm, 48000, hz)))
    print("loudness_pcm_batch", digest([np.array(J.loudness(pcm, 48000))]))
    pcm16 = [np.clip(x, -32768, 32767).astype(np.int16) for x in pcm]
    print("flac_encode_pcm_batch", digest(J.flac_encode(pcm16, 48000)),
          digest(J.flac_encode(pcm16, 22050, block_size=1152, max_lpc_order=12)))
    pcm_seams()
    host_bits()


from jbonsai_amd import synth  # noqa: E402

if redo_time:
    output_stages()
    sys.exit(0)
if "--seams" in sys.argv:
    pcm_seams()
    sys.exit(0)
if "--host" in sys.argv:
    host_bits()
    sys.exit(0)

v = O.Voice(VOICE)
utts = []
for lab, reps in ((SAMPLE_SENTENCE_2, 30), (SAMPLE_SENTENCE_1, 7), (SAMPLE_SENTENCE_2, 1)):
    d, s = oracle_states(v, list(lab) * reps)
    utts.append(to_utt(d, s))
with J.Batch(voice_info(v), utts * 3, keep_tracks=True) as b:
    b.run()
    b.sync()
    for name, arrs in (("mcp", [b.track(i, 0) for i in range(3)]), ("lf0", [b.track(i, 1) for i in range(3)]),
                       ("pcm", [b.pcm(i) for i in range(9)])):
        h = hashlib.sha256()
        for a in arrs:
            h.update(np.ascontiguousarray(a).tobytes())
        print(name, h.hexdigest()[:16])

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
big = [synth.u128(tab, 0)] * 8 + [synth.synth_utterance(tab, 9000 + 700 * i, 50 + i) for i in range(3)]
with J.Batch(vi, big, keep_tracks=True) as b:
    b.run()
    b.sync()
    print("config-2 kernels:", b.info())
    for name, arrs in (("mcp", [b.track(i, 0) for i in (0, 8, 10)]), ("lf0", [b.track(i, 1) for i in (0, 8, 10)]),
                       ("lpf", [b.track(i, 2) for i in (0, 9)]), ("exc", [b.excitation(i) for i in (0, 9)]),
                       ("pcm", [b.pcm(i) for i in (0, 7, 8, 9, 10)])):
        h = hashlib.sha256()
        for a in arrs:
            h.update(np.ascontiguousarray(a).tobytes())
        print("big", name, h.hexdigest()[:16])
with J.Batch(vi, big, pcm_i16=True) as b:
    b.run()
    b.sync()
    h = hashlib.sha256()
    for i in (0, 8, 10):
        h.update(b.pcm_i16(i).tobytes())
    print("big pcm_i16", h.hexdigest()[:16])
output_stages()

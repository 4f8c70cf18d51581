"""The reference's `examples/is-bonsai` on the GPU path: full-context labels -> PCM -> 16-bit WAV.

    python examples/is_bonsai.py [voice.htsvoice] [out.wav] [--loudness LUFS [--ceiling DBFS] [--true-peak] [--limiter DB]]
                                 [--programme] [--format f32|s16|s24|ulaw|alaw [--dither]] [--adpcm [--rate HZ]]
                                 [--flac] [--highpass HZ] [--fbank OUT.npy [--rate HZ]] [--mfcc OUT.npy [--rate HZ]] [--kaldi]
                                 [--melspec OUT.npy [--whisper | --rate HZ]] [--pitch OUT.npy [--rate HZ]]
                                 [--fir taps.npy [--fir-delay D]] [--noise bed.npy|white --snr DB [--snr-active]]
                                 [--room LX,LY,LZ --rt60 S [--room-taps K]] [--activity OUT.npy [--rate HZ]]

Mirrors examples/is-bonsai/main.rs of jbonsai: Engine::load, Engine::synthesize, then the 16-bit mono
WAV the example writes with hound (clamp to i16, truncate).  Needs an MI355X: the library has no CPU path.
With --loudness the audio is normalized on the GPU to that integrated loudness (BS.1770-4), its sample peak kept at or
under --ceiling (dBFS, default 0); with --true-peak the ceiling bounds the true peak (dBTP, BS.1770-4 Annex 2) instead.
With --programme (and --loudness) the reference's two sample sentences are synthesized side by side as sentence
utterances under ONE programme gain (per-request loudness scope: one gated measurement over both, one peak, one gain), so
the level between them is kept as synthesized; they are written back to back, and the programme's loudness, loudness
range and largest momentary and short-term loudness are printed.
With --format the samples are converted to that format on the GPU (ulaw and alaw at 8 kHz, the telephony rate; --dither:
TPDF dither for s16 and s24) and the WAV file carries them as they are.
With --adpcm the audio is encoded as IMA ADPCM (WAV format tag 0x11, half a byte per sample) on the GPU, at --rate if
given, with the block size that goes with the rate.
With --flac the 16-bit audio is encoded as a FLAC stream on the GPU, with the MD5 of its samples in STREAMINFO and a
SEEKTABLE with a point about every second, and written as it is.
With --highpass the audio passes a second-order high-pass at that corner on the GPU (Engine.set_filter), behind the
output rate and in front of the loudness measurement and every encoder above.
With --fir the audio is convolved on the GPU with the impulse response in that .npy file (a 1-D array of taps sampled at
the output rate: the voice's, or --rate), advanced by --fir-delay samples (Engine.set_fir): in front of --highpass, the
loudness measurement and every encoder above.
With --room the audio is reverberated on the GPU by a simulated shoebox room of those edges in metres with the
reverberation time --rt60 (Engine.set_room: the image-source method, Eyring's coefficients; source and microphone from
jb_room_vary with seed 0; --room-taps taps at the output rate, by default 1.2 rt60), in --fir's place.
With --noise background noise is added on the GPU at --snr dB (Engine.set_noise): the samples of that .npy file (a 1-D
array at the output rate, 16-bit units, looped) or, with "white", noise generated on the device; --snr-active measures
the speech over its active tiles (within 20 dB of the mean power), not over the leading and trailing silence.  Behind
--fir, in front of --highpass, the loudness measurement and every encoder above.
With --fbank the sentence's log-mel filterbank frames (25 ms windows every 10 ms, 80 filters, float32 [T, 80]) are
computed on the GPU from the final PCM, at --rate if given, and saved as a .npy file; no WAV file is written.
With --mfcc the same frames go on, still on the GPU, to 13 liftered cepstra with delta and delta-delta rows, mean and
variance normalised over the sentence (float32 [T, 39]), saved the same way.
With --kaldi beside --fbank or --mfcc the frames are conditioned as Kaldi's compute-fbank-feats does it, still on the GPU
(Engine.set_frame, J.kaldi_frame): per-frame DC removal, pre-emphasis 0.97, the Povey window, 20 Hz to half the rate,
23 filters; the cepstra then carry the frame's log energy as c0.
With --melspec the sentence's mel spectrogram in the librosa / Whisper convention -- a centred, reflected 25 ms Hann
window every 10 ms, 80 Slaney filters, natural logarithm, float32 [T, 80] -- is computed on the GPU from the final PCM,
at --rate if given; with --whisper it is Whisper's own front end (400 / 160 samples at 16 kHz, log10 clamped 8 under the
sentence's maximum, (y + 4) / 4: what log_mel_spectrogram gives before its padding to 30 s).  Saved the same way.
With --limiter (and --loudness) the gain may put the highest peak that many dB over the ceiling and a look-ahead limiter
on the GPU holds the ceiling (Engine.set_limiter): the target is reached where the peak alone stood in the way.
With --activity the sentence's per-frame speech-activity labels on --fbank's frame grid (25 ms windows every 10 ms; 1 =
the frame's energy lies within 40 dB of the loudest frame's, pauses of up to 200 ms closed) are measured on the GPU in
the run that makes the PCM (Engine.synthesize_programme_activity), at --rate if given, and saved as a .npy file of uint8
[T, 1]: the mask that says which of --fbank's frames hold speech.  The WAV file is written as usual.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jbonsai_amd as J  # noqa: E402
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2  # the reference's example label lines  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("voice", nargs="?", default=os.path.join(
    os.path.dirname(__file__), "..", "tests", "golden", "voice", "nitech_jp_atr503_m001.htsvoice"))
ap.add_argument("out", nargs="?", default="is-bonsai.wav")
ap.add_argument("--loudness", type=float, default=None, metavar="LUFS", help="target integrated loudness")
ap.add_argument("--ceiling", type=float, default=0.0, metavar="DBFS", help="sample-peak ceiling (with --loudness)")
ap.add_argument("--true-peak", action="store_true", help="the ceiling bounds the true peak (dBTP), not the sample peak")
ap.add_argument("--programme", action="store_true",
                help="two sentences as one programme under one gain (with --loudness)")
ap.add_argument("--format", choices=["f32", "s16", "s24", "ulaw", "alaw"], default=None,
                help="sample format of the WAV file, converted on the GPU")
ap.add_argument("--dither", action="store_true", help="TPDF dither (with --format s16 or s24)")
ap.add_argument("--adpcm", action="store_true", help="IMA ADPCM (4-bit) WAV file, encoded on the GPU")
ap.add_argument("--rate", type=int, default=None, metavar="HZ", help="output rate (with --adpcm, --fbank, --mfcc or --melspec)")
ap.add_argument("--fbank", default=None, metavar="OUT.npy", help="log-mel filterbank frames, computed on the GPU")
ap.add_argument("--mfcc", default=None, metavar="OUT.npy", help="MFCC + deltas + CMVN rows, computed on the GPU")
ap.add_argument("--kaldi", action="store_true", help="with --fbank or --mfcc: Kaldi's frame conditioning and defaults")
ap.add_argument("--melspec", default=None, metavar="OUT.npy", help="mel spectrogram (librosa / Whisper convention), computed on the GPU")
ap.add_argument("--whisper", action="store_true", help="with --melspec: Whisper's front end at 16 kHz")
ap.add_argument("--pitch", default=None, metavar="OUT.npy", help="Kaldi-style pitch features [T, 3] (POV, normalised log-pitch, delta), tracked on the GPU; --rate applies")
ap.add_argument("--flac", action="store_true", help="FLAC file with MD5 and a SEEKTABLE, encoded on the GPU")
ap.add_argument("--highpass", type=float, default=None, metavar="HZ", help="high-pass corner, filtered on the GPU")
ap.add_argument("--fir", default=None, metavar="taps.npy", help="impulse response at the output rate, convolved on the GPU")
ap.add_argument("--fir-delay", type=int, default=0, metavar="D", help="samples the convolved output is advanced by")
ap.add_argument("--room", default=None, metavar="LX,LY,LZ", help="edges of a simulated room in metres, reverberated on the GPU")
ap.add_argument("--rt60", type=float, default=0.4, metavar="S", help="reverberation time of --room")
ap.add_argument("--room-taps", type=int, default=0, metavar="K", help="taps of --room's response (0: 1.2 rt60)")
ap.add_argument("--noise", default=None, metavar="bed.npy|white", help="background noise, added on the GPU at --snr")
ap.add_argument("--snr", type=float, default=15.0, metavar="DB", help="speech power over added-noise power")
ap.add_argument("--snr-active", action="store_true", help="the speech power of the active tiles, not of the whole signal")
ap.add_argument("--activity", default=None, metavar="OUT.npy", help="per-frame speech-activity labels, measured on the GPU")
ap.add_argument("--limiter", type=float, default=None, metavar="DB",
                help="look-ahead limiter on the GPU: dB the gain may put the highest peak over the ceiling (with --loudness)")
args = ap.parse_args()
voice, out = args.voice, args.out

engine = J.Engine.load([voice])
if args.fir is not None:
    import numpy as np

    if args.rate:
        engine.condition.set_output_sampling_frequency(args.rate)
    engine.set_fir(J.fir(np.load(args.fir), args.rate or engine.condition.get_sampling_frequency(), args.fir_delay))
if args.room is not None:
    if args.rate:
        engine.condition.set_output_sampling_frequency(args.rate)
    hz = args.rate or engine.condition.get_sampling_frequency()
    size = [float(v) for v in args.room.split(",")]
    src, mic = J.room_vary(0, 0, size, 0.5)
    engine.set_room(J.room(size, src, mic, rt60=args.rt60, hz=hz, n_taps=args.room_taps or int(1.2 * args.rt60 * hz)))
if args.noise is not None:
    import numpy as np

    if args.rate:
        engine.condition.set_output_sampling_frequency(args.rate)
    engine.set_noise(J.noise(None if args.noise == "white" else np.load(args.noise),
                             args.rate or engine.condition.get_sampling_frequency(), args.snr,
                             reference="active" if args.snr_active else "whole"))
if args.highpass is not None:
    engine.set_filter(J.highpass(args.highpass))
if args.loudness is not None:
    engine.condition.set_loudness_target(args.loudness)
    engine.condition.set_peak_ceiling(args.ceiling)
    if args.limiter is not None:
        engine.set_limiter(J.limiter(max_reduction_db=args.limiter))
    engine.condition.set_peak_mode(J.PEAK_TRUE if args.true_peak else J.PEAK_SAMPLE)
if args.programme:
    if args.loudness is None:
        ap.error("--programme goes with --loudness")
    import numpy as np

    engine.set_loudness_scope(J.LOUDNESS_PER_REQUEST)
    hz = engine.condition.get_sampling_frequency()
    parts = [np.asarray(x) for x in engine.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2])]
    rep = J.loudness_groups(parts, hz, [0, 0], mode=J.PEAK_TRUE if args.true_peak else J.PEAK_SAMPLE)
    g, r = rep["groups"][0], rep["groups"][0]["r128"]
    print(f"programme of {len(parts)} sentences: {g['lufs']:.2f} LUFS, sample peak {g['sample_peak_dbfs']:.2f} dBFS, "
          f"LRA {r['lra_lu']:.2f} LU, max momentary {r['max_momentary_lufs']:.2f}, "
          f"max short-term {r['max_short_term_lufs']:.2f} LUFS")
    print("each sentence alone: " + ", ".join(f"{v:.2f} LUFS" for v in rep["lufs"]))
    J.write_wav(out, np.concatenate(parts), hz)
    print(f"wrote {out}")
    sys.exit(0)
if args.activity:
    import numpy as np

    if args.rate:
        engine.condition.set_output_sampling_frequency(args.rate)
    hz = engine.condition.get_output_sampling_frequency() or engine.condition.get_sampling_frequency()
    pcm, labels, _ = engine.synthesize_programme_activity([SAMPLE_SENTENCE_2], J.activity(25, 10, gate_db=40, min_gap=20))
    np.save(args.activity, labels)
    on = np.flatnonzero(labels[:, 0])
    print(f"wrote {args.activity}: {labels.shape[0]} frames, {on.size} active, the first {on[0] if on.size else '-'} and "
          f"the last {on[-1] if on.size else '-'}")
    J.write_wav(out, pcm, hz)
    print(f"wrote {out}: {pcm.size} samples at {hz} Hz")
    sys.exit(0)
if args.fbank:
    import numpy as np

    if args.rate:
        engine.condition.set_output_sampling_frequency(args.rate)
    if args.kaldi:
        fopts, fr = J.kaldi_frame()
        engine.set_frame(fr)
        feats = engine.synthesize_fbank(SAMPLE_SENTENCE_2, fopts)
    else:
        feats = engine.synthesize_fbank(SAMPLE_SENTENCE_2)
    np.save(args.fbank, feats)
    hz = engine.condition.get_output_sampling_frequency() or engine.condition.get_sampling_frequency()
    print(f"wrote {args.fbank}: {feats.shape[0]} frames of {feats.shape[1]} log-mel values at {hz} Hz")
    sys.exit(0)
if args.mfcc:
    import numpy as np

    if args.rate:
        engine.condition.set_output_sampling_frequency(args.rate)
    if args.kaldi:
        fopts, fr = J.kaldi_frame()
        fr.flags |= J.FRAME_ENERGY
        engine.set_frame(fr)
        feats = engine.synthesize_mfcc(SAMPLE_SENTENCE_2, fbank=fopts, delta_order=2, cmvn="mean_var")
    else:
        feats = engine.synthesize_mfcc(SAMPLE_SENTENCE_2, delta_order=2, cmvn="mean_var")
    np.save(args.mfcc, feats)
    hz = engine.condition.get_output_sampling_frequency() or engine.condition.get_sampling_frequency()
    print(f"wrote {args.mfcc}: {feats.shape[0]} frames of {feats.shape[1]} cepstral values at {hz} Hz")
    sys.exit(0)
if args.pitch:
    import numpy as np

    if args.rate:
        engine.condition.set_output_sampling_frequency(args.rate)
    hz = engine.condition.get_output_sampling_frequency() or engine.condition.get_sampling_frequency()
    feats = engine.synthesize_pitch(SAMPLE_SENTENCE_2, J.kaldi_pitch())
    np.save(args.pitch, feats)
    print(f"wrote {args.pitch}: {feats.shape[0]} frames of {feats.shape[1]} pitch columns at {hz} Hz")
    sys.exit(0)
if args.melspec:
    import numpy as np

    if args.whisper or args.rate:
        engine.condition.set_output_sampling_frequency(16000 if args.whisper else args.rate)
    hz = engine.condition.get_output_sampling_frequency() or engine.condition.get_sampling_frequency()
    opts = J.whisper_mel(80) if args.whisper else J.melspec(win_ms=25, hop_ms=10, rate=hz)
    feats = engine.synthesize_melspec(SAMPLE_SENTENCE_2, opts)
    np.save(args.melspec, feats)
    print(f"wrote {args.melspec}: {feats.shape[0]} frames of {feats.shape[1]} mel values at {hz} Hz")
    sys.exit(0)
if args.adpcm:
    if args.rate:
        engine.condition.set_output_sampling_frequency(args.rate)
    stream = engine.synthesize_adpcm(SAMPLE_SENTENCE_2)
    stream.write_wav(out)
    print(f"wrote {out}: {stream.n_samples} samples at {stream.hz} Hz in {len(stream.data)} bytes of IMA ADPCM "
          f"(blocks of {stream.block_align}, {len(stream.data) / max(stream.n_samples, 1):.3f} bytes per sample)")
    sys.exit(0)
if args.flac:
    data = engine.synthesize_flac(SAMPLE_SENTENCE_2, md5=True, seek_interval_ms=1000)
    with open(out, "wb") as f:
        f.write(data)
    print(f"wrote {out}: {len(data)} bytes of FLAC, MD5 {data[26:42].hex()}")
    sys.exit(0)
if args.format is not None:
    if args.format in ("ulaw", "alaw"):
        engine.condition.set_output_sampling_frequency(8000)
    hz = engine.condition.get_output_sampling_frequency() or engine.condition.get_sampling_frequency()
    data = engine.synthesize_formatted(SAMPLE_SENTENCE_2, args.format, dither=args.dither, seed=1)
    J.write_wav_formatted(out, data, hz, args.format)
    print(f"wrote {out}: {len(data)} bytes of {args.format} at {hz} Hz")
    sys.exit(0)
speech = engine.synthesize(SAMPLE_SENTENCE_2)
print(f"The synthesized voice has {len(speech)} samples in total.")
if args.loudness is not None:
    lufs, peak = J.loudness(speech, engine.condition.get_sampling_frequency())
    tp = J.true_peak(speech, engine.condition.get_sampling_frequency())
    print(f"normalized: {lufs:.2f} LUFS, sample peak {peak:.2f} dBFS, true peak {tp:.2f} dBTP")
J.write_wav(out, speech, engine.condition.get_sampling_frequency())
print(f"wrote {out}")

# the batched entry with the 16-bit sink fused into the vocoder: four speeds of the same sentence
outs = []
for speed in (0.8, 1.0, 1.2, 1.4):
    engine.condition.set_speed(speed)
    outs.append(engine.synthesize_batch([SAMPLE_SENTENCE_2], i16=True)[0])
print("samples at speeds 0.8 / 1.0 / 1.2 / 1.4:", [len(o) for o in outs])

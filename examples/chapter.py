"""A chapter as one file: several label files in, ONE FLAC stream or WAV file out -- sentence, pause, sentence.

    python examples/chapter.py voice.htsvoice first.lab second.lab ... -o chapter.flac
                               [--lead-ms MS] [--gap-ms MS] [--trail-ms MS] [--fade-ms MS]
                               [--loudness LUFS [--ceiling DBFS] [--limiter DB]] [--rate HZ] [--highpass HZ]
                               [--fbank OUT.npy] [--mfcc OUT.npy] [--kaldi] [--melspec OUT.npy [--whisper]] [--pitch OUT.npy] [--fir taps.npy [--fir-delay D]]
                               [--noise bed.npy|white --snr DB] [--room LX,LY,LZ --rt60 S [--room-taps K]]

Each label file holds the full-context labels of one sentence, one per line.  The sentences are synthesized in one
batch and joined on the GPU (Engine.synthesize_programme) in front of the encoder, so a .flac output is one stream whose
frame numbers, STREAMINFO, MD5 and SEEKTABLE (a point about every second) cover the whole chapter; any other name is
written as a 16-bit WAV file.  With --loudness the chapter gets ONE gain (per-request loudness scope), so the sentences
keep their relative levels.  With --highpass a rumble and DC high-pass at that corner runs on the GPU in front of the
loudness measurement and the encoder (Engine.set_filter).  With --fir every sentence is convolved on the GPU with the impulse
response in that .npy file (taps at the output rate; --fir-delay removes its leading latency), in front of --highpass
(Engine.set_fir).  With --room every sentence is reverberated on the GPU by a simulated shoebox room of those edges in
metres with the reverberation time --rt60, in --fir's place, every sentence from positions of its own (Engine.set_room
with vary=True, seed 0: jb_room_vary).  With --noise every sentence gets background noise at --snr dB on the GPU, behind --fir and in front
of --highpass: the looped samples of that .npy file (at the output rate) or "white", every sentence from a place of
its own in the bed (Engine.set_noise with vary=True); the pads between the sentences stay silent.  With --limiter (and --loudness) the chapter's gain may put its
highest peak that many dB over the ceiling and a look-ahead limiter holds the ceiling on the GPU (Engine.set_limiter), so
one loud peak no longer holds the whole chapter under its target.  With --fbank the chapter's log-mel filterbank frames
(25 ms windows every 10 ms, 80 filters, float32 [T, 80]) are computed on the GPU from the joined programme, frames across
the pauses and the seams included, and saved as a .npy file INSTEAD of the audio: a request has one sink, so no audio
file is written (run again without --fbank for it; the cue list is the same).  --mfcc does the same with 13 liftered
cepstra, delta and delta-delta rows, normalised in mean and variance over the whole chapter (float32 [T, 39]); --melspec with the chapter's mel spectrogram in
the librosa / Whisper convention (a centred, reflected 25 ms Hann window every 10 ms, 80 Slaney filters, natural
logarithm), or with --whisper Whisper's own front end at 16 kHz, its clamp 8 under the whole chapter's maximum.  The cue list -- each sentence's first sample and time within the chapter -- is printed.
Needs an MI355X: the library has no CPU path.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jbonsai_amd as J  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("voice")
ap.add_argument("labels", nargs="+", help="one label file per sentence")
ap.add_argument("-o", "--out", default="chapter.flac")
ap.add_argument("--lead-ms", type=float, default=0.0, help="silence in front of the first sentence")
ap.add_argument("--gap-ms", type=float, default=500.0, help="silence between two sentences")
ap.add_argument("--trail-ms", type=float, default=0.0, help="silence behind the last sentence")
ap.add_argument("--fade-ms", type=float, default=5.0, help="fade at both edges of every sentence")
ap.add_argument("--loudness", type=float, default=None, metavar="LUFS", help="target loudness of the chapter")
ap.add_argument("--ceiling", type=float, default=-1.0, metavar="DBFS", help="sample-peak ceiling (with --loudness)")
ap.add_argument("--limiter", type=float, default=None, metavar="DB",
                help="look-ahead limiter: the gain may put the highest peak this far over the ceiling (with --loudness)")
ap.add_argument("--rate", type=int, default=None, metavar="HZ", help="output rate")
ap.add_argument("--highpass", type=float, default=None, metavar="HZ", help="high-pass corner (50 to 80 Hz removes rumble and DC)")
ap.add_argument("--noise", default=None, metavar="bed.npy|white",
                help="background noise added to every sentence on the GPU at --snr (Engine.set_noise)")
ap.add_argument("--snr", type=float, default=15.0, metavar="DB", help="speech power over added-noise power")
ap.add_argument("--room", default=None, metavar="LX,LY,LZ",
                help="edges of a simulated room in metres: every sentence reverberated on the GPU (Engine.set_room)")
ap.add_argument("--rt60", type=float, default=0.5, metavar="S", help="reverberation time of --room")
ap.add_argument("--room-taps", type=int, default=0, metavar="K", help="taps of --room's response (0: 1.2 rt60)")
ap.add_argument("--fir", default=None, metavar="taps.npy",
                help="impulse response at the output rate (a 1-D .npy), convolved with every sentence on the GPU (Engine.set_fir)")
ap.add_argument("--fir-delay", type=int, default=0, metavar="D", help="samples the convolved output is advanced by")
ap.add_argument("--fbank", default=None, metavar="OUT.npy", help="the chapter's log-mel filterbank frames from the GPU, instead of the audio")
ap.add_argument("--mfcc", default=None, metavar="OUT.npy", help="the chapter's MFCC + deltas + CMVN rows from the GPU, instead of the audio")
ap.add_argument("--kaldi", action="store_true", help="with --fbank or --mfcc: Kaldi's frame conditioning and defaults (J.kaldi_frame)")
ap.add_argument("--melspec", default=None, metavar="OUT.npy", help="the chapter's mel spectrogram (librosa / Whisper convention) from the GPU, instead of the audio")
ap.add_argument("--whisper", action="store_true", help="with --melspec: Whisper's front end; sets the output rate to 16 kHz")
ap.add_argument("--pitch", default=None, metavar="OUT.npy", help="the chapter's Kaldi-style pitch features [T, 3] from the GPU, the log-pitch normalised over the whole chapter, instead of the audio")
args = ap.parse_args()
if args.melspec and args.whisper:
    args.rate = 16000

sentences = []
for path in args.labels:
    with open(path) as f:
        sentences.append([ln for ln in f.read().split("\n") if ln and not ln.startswith("#")])

engine = J.Engine.load([args.voice])
if args.rate:
    engine.condition.set_output_sampling_frequency(args.rate)
if args.fir is not None:
    import numpy as np

    engine.set_fir(J.fir(np.load(args.fir), args.rate or engine.condition.get_sampling_frequency(), args.fir_delay))
if args.room is not None:
    hz = args.rate or engine.condition.get_sampling_frequency()
    size = [float(v) for v in args.room.split(",")]
    src, mic = J.room_vary(0, 0, size, 0.5)
    engine.set_room(J.room(size, src, mic, rt60=args.rt60, hz=hz, n_taps=args.room_taps or int(1.2 * args.rt60 * hz)),
                    vary=True, seed=0)
if args.noise is not None:
    import numpy as np

    engine.set_noise(J.noise(None if args.noise == "white" else np.load(args.noise),
                             args.rate or engine.condition.get_sampling_frequency(), args.snr, vary=True))
if args.highpass is not None:
    engine.set_filter(J.highpass(args.highpass))
if args.loudness is not None:
    engine.condition.set_loudness_target(args.loudness)
    engine.condition.set_peak_ceiling(args.ceiling)
    if args.limiter is not None:
        engine.set_limiter(J.limiter(max_reduction_db=args.limiter))
    engine.set_loudness_scope(J.LOUDNESS_PER_REQUEST)
hz = engine.condition.get_output_sampling_frequency() or engine.condition.get_sampling_frequency()
join = dict(lead_ms=args.lead_ms, gap_ms=args.gap_ms, trail_ms=args.trail_ms, fade_ms=args.fade_ms)
if args.fbank:
    import numpy as np

    kaldi = {}
    if args.kaldi:  # DC removal, pre-emphasis 0.97, the Povey window, 23 filters from 20 Hz
        kaldi["opts"], fr = J.kaldi_frame()
        engine.set_frame(fr)
    feats, starts = engine.synthesize_programme(sentences, sink="fbank", **kaldi, **join)
    np.save(args.fbank, feats)
    print(f"wrote {args.fbank}: {feats.shape[0]} frames of {feats.shape[1]} log-mel values at {hz} Hz")
elif args.mfcc:
    import numpy as np

    kaldi = {}
    if args.kaldi:  # ... and the frame's log energy as c0
        kaldi["fbank"], fr = J.kaldi_frame()
        fr.flags |= J.FRAME_ENERGY
        engine.set_frame(fr)
    feats, starts = engine.synthesize_programme(sentences, sink="mfcc", delta_order=2, cmvn="mean_var", **kaldi, **join)
    np.save(args.mfcc, feats)
    print(f"wrote {args.mfcc}: {feats.shape[0]} frames of {feats.shape[1]} cepstral values at {hz} Hz")
elif args.pitch:
    import numpy as np

    feats, starts = engine.synthesize_programme(sentences, sink="pitch", opts=J.kaldi_pitch(), **join)
    np.save(args.pitch, feats)
    print(f"wrote {args.pitch}: {feats.shape[0]} frames of {feats.shape[1]} pitch columns at {hz} Hz")
elif args.melspec:
    import numpy as np

    opts = J.whisper_mel(80) if args.whisper else J.melspec(win_ms=25, hop_ms=10, rate=hz)
    feats, starts = engine.synthesize_programme(sentences, sink="melspec", opts=opts, **join)
    np.save(args.melspec, feats)
    print(f"wrote {args.melspec}: {feats.shape[0]} frames of {feats.shape[1]} mel values at {hz} Hz")
elif args.out.endswith(".flac"):
    data, starts = engine.synthesize_programme(sentences, sink="flac", md5=True, seek_interval_ms=1000, **join)
    with open(args.out, "wb") as f:
        f.write(data)
    print(f"wrote {args.out}: {len(data)} bytes of FLAC at {hz} Hz, MD5 {data[26:42].hex()}")
else:
    pcm, starts = engine.synthesize_programme(sentences, sink="i16", **join)
    J.write_wav(args.out, pcm, hz)
    print(f"wrote {args.out}: {pcm.size} samples at {hz} Hz")
for k, (s, path) in enumerate(zip(starts, args.labels)):
    print(f"cue {k} {s} {s / hz:.3f} {path}")

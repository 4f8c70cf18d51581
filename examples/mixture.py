"""Overlapping talkers as one file: several label files in, ONE FLAC stream or WAV file out -- every sentence at a
start of its own and under a gain of its own, summed on the GPU.

    python examples/mixture.py voice.htsvoice first.lab second.lab ... -o mixture.flac
                               --start-ms MS,MS,... [--gain-db DB,DB,...] [--fit [--ceiling DBFS]]
                               [--lead-ms MS] [--trail-ms MS] [--fade-ms MS] [--rate HZ]
                               [--room LX,LY,LZ --rt60 S [--vary]]
                               [--stems DIR [--talker ID ...] [--levels levels.csv]]
                               [--activity labels.npy] [--rttm out.rttm] [--gate-db DB]

Each label file holds the full-context labels of one sentence, one per line.  The sentences are synthesized in one
batch and mixed on the GPU (Engine.set_programme_mix, then Engine.synthesize_programme) in front of the encoder, so a
.flac output is one stream whose frame numbers, STREAMINFO, MD5 and SEEKTABLE cover the mixture; any other name is
written as a 16-bit WAV file.  --start-ms and --gain-db take one value per sentence (a gain of 0 dB by default).  With
--fit a mixture whose peak passes --ceiling is scaled down to it on the GPU; without it the 16-bit sink clamps.  With
--room every sentence is reverberated by a simulated shoebox room of those edges in metres, with --vary every talker
from a position of their own (Engine.set_room with vary=True).  With --stems the mixture and its stems in programme
coordinates -- each source exactly as it entered the sum, at its start, under its fades, its gain and the fit's scale,
zero elsewhere and as long as the mixture -- come from one more run (Engine.synthesize_programme(..., stems=)) and are
written to DIR as mix and s<id>, FLAC or 16-bit WAV as the output is; --talker gives one id per sentence (sentences of
one id form one stem; by default every sentence is a stem of its own), and --levels writes one CSV row per stem: its
peak, the mixture's scale, the three sums E_s, D and E_p measured on the GPU and level_db, sir_db and si_sdr_db (the
input SI-SDR of the corpus metadata).  The cue list -- each sentence's first sample and time within the mixture -- and
the stage's report (the host rule over the members: the same numbers) are printed.
With --activity the per-frame speech-activity labels of the talkers, a uint8 matrix [frames][talkers] at 25 / 10 ms
measured on the GPU in a run of the same mixture (Engine.synthesize_programme_activity: a gate --gate-db under each
talker's loudest frame, pauses of up to 200 ms closed, 20 ms of hang at both ends), are saved as a .npy file; with --rttm
the runs of each column are written as RTTM lines, `SPEAKER <name> 1 <start> <dur> <NA> <NA> spk<j> <NA> <NA>`.
Needs an MI355X: the library has no CPU path.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jbonsai_amd as J  # noqa: E402


def floats(s):
    return [float(v) for v in s.split(",")]


ap = argparse.ArgumentParser()
ap.add_argument("voice")
ap.add_argument("labels", nargs="+", help="one label file per sentence")
ap.add_argument("-o", "--out", default="mixture.flac")
ap.add_argument("--start-ms", type=floats, required=True, metavar="MS,MS,...", help="each sentence's start")
ap.add_argument("--gain-db", type=floats, default=None, metavar="DB,DB,...", help="each sentence's gain (0 dB)")
ap.add_argument("--fit", action="store_true", help="scale a mixture over the ceiling down to it")
ap.add_argument("--ceiling", type=float, default=-1.0, metavar="DBFS", help="the ceiling of --fit")
ap.add_argument("--lead-ms", type=float, default=0.0, help="silence in front of every start")
ap.add_argument("--trail-ms", type=float, default=0.0, help="silence every sentence claims behind its end")
ap.add_argument("--fade-ms", type=float, default=5.0, help="fade at both edges of every sentence")
ap.add_argument("--rate", type=int, default=None, metavar="HZ", help="output rate")
ap.add_argument("--room", default=None, metavar="LX,LY,LZ", help="edges of a simulated room in metres (Engine.set_room)")
ap.add_argument("--rt60", type=float, default=0.5, metavar="S", help="reverberation time of --room")
ap.add_argument("--vary", action="store_true", help="with --room: every talker at a position of their own")
ap.add_argument("--stems", default=None, metavar="DIR", help="write the mixture and its stems there (mix, s<id>)")
ap.add_argument("--talker", type=int, nargs="*", default=None, metavar="ID", help="with --stems: each sentence's stem id")
ap.add_argument("--levels", default=None, metavar="CSV", help="with --stems: each stem's level against the mixture")
ap.add_argument("--activity", default=None, metavar="NPY", help="save the talkers' per-frame activity labels there")
ap.add_argument("--rttm", default=None, metavar="RTTM", help="write the talkers' active runs there as RTTM lines")
ap.add_argument("--gate-db", type=float, default=40.0, help="the activity gate under each talker's loudest frame")
args = ap.parse_args()
gains = args.gain_db or [0.0] * len(args.labels)
if len(args.start_ms) != len(args.labels) or len(gains) != len(args.labels):
    ap.error("--start-ms and --gain-db take one value per label file")
talkers = args.talker if args.talker else list(range(len(args.labels)))
if len(talkers) != len(args.labels) or ((args.talker or args.levels) and not args.stems):
    ap.error("--talker takes one id per label file; --talker and --levels go with --stems")

sentences = []
for path in args.labels:
    with open(path) as f:
        sentences.append([ln for ln in f.read().split("\n") if ln and not ln.startswith("#")])

engine = J.Engine.load([args.voice])
if args.rate:
    engine.condition.set_output_sampling_frequency(args.rate)
hz = engine.condition.get_output_sampling_frequency() or engine.condition.get_sampling_frequency()
if args.room is not None:
    size = floats(args.room)
    src, mic = J.room_vary(0, 0, size, 0.5)
    engine.set_room(J.room(size, src, mic, rt60=args.rt60, hz=hz, n_taps=int(1.2 * args.rt60 * hz)), vary=args.vary,
                    seed=0)
place = list(zip(args.start_ms, gains))
opts = dict(lead_ms=args.lead_ms, trail_ms=args.trail_ms, fade_ms=args.fade_ms, mix=place, fit=args.fit,
            ceiling_db=args.ceiling)
if args.out.endswith(".flac"):
    data, starts = engine.synthesize_programme(sentences, sink="flac", md5=True, seek_interval_ms=1000, **opts)
    with open(args.out, "wb") as f:
        f.write(data)
    print(f"wrote {args.out}: {len(data)} bytes of FLAC at {hz} Hz, MD5 {data[26:42].hex()}")
else:
    pcm, starts = engine.synthesize_programme(sentences, sink="i16", **opts)
    J.write_wav(args.out, pcm, hz)
    print(f"wrote {args.out}: {pcm.size} samples at {hz} Hz")
for k, (s, path) in enumerate(zip(starts, args.labels)):
    print(f"cue {k} {s} {s / hz:.3f} {path}")
# the members, and the stage's report from them by the host rule
stems = engine.synthesize_batch(sentences, i16=True)
fade, trail = J.join_ms_to_samples(args.fade_ms, hz), J.join_ms_to_samples(args.trail_ms, hz)
req = [(0, s, g, trail, fade, fade) for s, g in zip(starts, gains)]
_, (rep,) = J.mix_host(stems, req, J.mix_opts(args.fit, args.ceiling))
print(f"report peak {rep.peak:.1f} scale {rep.scale:.6f} depth {rep.depth} overlap {rep.overlap} samples "
      f"({rep.overlap / hz:.3f} s)")
if args.stems:
    import numpy as np

    os.makedirs(args.stems, exist_ok=True)
    flac = args.out.endswith(".flac")
    kw = dict(md5=True, seek_interval_ms=1000) if flac else {}
    ids = list(dict.fromkeys(talkers))  # the stems' order: by the first sentence of each id
    # (the library's stem ids lie below the number of sentences: the caller's ids are numbered in that order)
    units, _, reports = engine.synthesize_programme(sentences, sink="flac" if flac else "f64",
                                                    stems=[ids.index(t) for t in talkers], levels=True, **kw, **opts)
    for name, x in zip(["mix"] + [f"s{i}" for i in ids], units):
        path = os.path.join(args.stems, name + (".flac" if flac else ".wav"))
        if flac:
            with open(path, "wb") as f:
                f.write(x)
        else:  # the 16-bit sink's rule: clamp, then truncate toward zero
            J.write_wav(path, np.trunc(np.clip(x, -32768.0, 32767.0)).astype(np.int16), hz)
        print(f"stem {name} {path}")
    if args.levels:
        with open(args.levels, "w") as f:
            f.write("stem,peak,scale,e_s,d,e_p,level_db,sir_db,si_sdr_db\n")
            for i, r in zip(ids, reports):
                f.write(f"s{i},{r.peak!r},{r.scale!r},{r.e_s!r},{r.d!r},{r.e_p!r},{r.level_db!r},{r.sir_db!r},"
                        f"{r.si_sdr_db!r}\n")
if args.activity or args.rttm:
    import numpy as np

    hop_ms = 10.0
    _, labels, _ = engine.synthesize_programme_activity(
        sentences, J.activity(25, hop_ms, gate_db=args.gate_db, grid="center", min_gap=20, hang_before=2, hang_after=2),
        lead_ms=args.lead_ms, trail_ms=args.trail_ms, fade_ms=args.fade_ms, mix=place, fit=args.fit,
        ceiling_db=args.ceiling)
    k = labels.sum(axis=1)
    print(f"activity {labels.shape[0]} frames by {labels.shape[1]} talkers: {int((k == 0).sum())} silent, "
          f"{int((k == 1).sum())} under one talker, {int((k >= 2).sum())} overlapped")
    if args.activity:
        np.save(args.activity, labels)
    if args.rttm:
        name = os.path.splitext(os.path.basename(args.out))[0]
        with open(args.rttm, "w") as f:
            for j in range(labels.shape[1]):
                edges = np.flatnonzero(np.diff(np.concatenate(([0], labels[:, j], [0]))))
                for a, b in zip(edges[::2], edges[1::2]):  # frames [a, b) are active
                    f.write(f"SPEAKER {name} 1 {a * hop_ms / 1000:.3f} {(b - a) * hop_ms / 1000:.3f} <NA> <NA> spk{j} "
                            "<NA> <NA>\n")

"""The cepstral stage in the output plan (jbonsai_amd/csrc/jb_output.h, plan_output) on the host, without a GPU: the
slab the stage reads, its two slabs (the f64 log-mel scratch and the feature bytes), each unit's frames, row width and
16-byte aligned places (behind a join: each programme's) -- and that a plain filterbank request's plan is the same with
and without the cepstral request, and the whole plan without it what it was.  A probe of its own
(tests/plan/mfcc_probe.cpp), built the way tests/test_adpcm_plan.py builds its probe."""
import itertools
import json
import subprocess

import pytest

from tests import fbank_ref as R
from tests.test_adpcm_plan import build
from tests.test_fbank_plan import run_fb
from tests.test_output_plan import BATCHES, VOICE_HZ

CENTER, LINEAR, F64 = 1, 2, 8
MFCC_F64 = 1


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("mfcc_plan")
    return build(d, "mfcc_probe"), build(d, "fbank_probe")


def run_mf(exe, n, mfcc=True, fb_flags=0, n_mels=80, n_fft=0, n_ceps=13, order=0, window=2, cmvn=0, flags=0,
           fbank=False, fbank_mels=64, want=None, join=None, i16=False, loudness=False, flac=False, fmt_bytes=0,
           adpcm=False, align=0):
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, int(adpcm), align,
            int(fbank), 25000, 10000, 0, fbank_mels, 0,
            int(mfcc), 25000, 10000, n_fft, n_mels, fb_flags, n_ceps, order, window, cmvn, flags,
            len(n), *n, *off, len(want or []), *(want or []), len(join or []), *[v for j in (join or []) for v in j]]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    p["fbank"] = [dict(zip(("off", "bytes", "T", "wl", "hop", "n_fft"), w)) for w in p["fbank"]]
    p["mfcc"] = [dict(zip(("off", "bytes", "T", "width", "n_fft", "loff"), w)) for w in p["mfcc"]]
    return p


def test_slabs_offsets_and_sizes(probes):
    """13 cepstra of f32 with one delta row (104 bytes a frame, no multiple of 16) and 23 filters (an odd count of
    doubles a frame) over lengths around a window: every unit starts on a 16-byte boundary of both slabs, no two
    overlap, the byte counts are the geometry's and the slabs hold them all."""
    wl, hop, _ = R.geometry(VOICE_HZ)
    n = [0, wl - 1, wl, wl + hop - 1, wl + hop, 5 * hop + wl + 1]
    for fb_flags, flags, order, n_ceps, elem in ((0, 0, 1, 13, 4), (CENTER, MFCC_F64, 2, 13, 8), (0, 0, 0, 0, 4)):
        p = run_mf(probes[0], n, n_mels=23, fb_flags=fb_flags, flags=flags, order=order, n_ceps=n_ceps)
        T = [R.n_frames(k, wl, hop, bool(fb_flags & CENTER)) for k in n]
        width = (n_ceps or 23) * (order + 1)
        assert [w["T"] for w in p["mfcc"]] == T and [w["width"] for w in p["mfcc"]] == [width] * len(n)
        assert [w["bytes"] for w in p["mfcc"]] == [t * width * elem for t in T]
        end = lend = 0
        for w in p["mfcc"]:
            assert w["off"] % 16 == 0 and w["off"] >= end
            assert w["loff"] % 2 == 0 and w["loff"] >= lend  # doubles: 16 bytes
            end, lend = w["off"] + w["bytes"], w["loff"] + w["T"] * 23
        assert p["alloc"]["Mfcc"][1] == 1 and p["alloc"]["Mfcc"][0] >= end and p["alloc"]["Mfcc"][0] % 16 == 0
        assert p["alloc"]["MfccL"][1] == 8 and p["alloc"]["MfccL"][0] >= lend
        assert p["mfcc_src"] == p["final"][0] == "V64"
    p = run_mf(probes[0], n, n_mels=23, order=1)
    assert [w["off"] for w in p["mfcc"]] == [0, 0, 0, 112, 224, 432]  # packed as tightly as the alignment allows
    assert [w["loff"] for w in p["mfcc"]] == [0, 0, 0, 24, 48, 94]


def test_geometry_follows_each_utterance_rate_and_refused_options_are_no_request(probes):
    n = [30000] * 4
    want = [8000, 0, 22050, 16000]
    p = run_mf(probes[0], n, want=want, order=2)
    for w, u in zip(p["mfcc"], p["utt"]):
        wl, hop, n_fft = R.geometry(u["hz"])
        assert w["n_fft"] == n_fft and w["T"] == R.n_frames(u["n"], wl, hop, False) and w["bytes"] == w["T"] * 39 * 4
    nothing = dict(mfcc_src="none", mfcc=[])
    for kw in (dict(n_fft=1024, want=want),  # 1200 samples at 48 kHz do not fit
               dict(fb_flags=LINEAR), dict(fb_flags=F64),  # the stage makes f64 logarithms itself
               dict(n_ceps=81), dict(order=3), dict(window=0), dict(window=6), dict(cmvn=3), dict(flags=2),
               dict(i16=True)):  # no f64 for the stage
        r = run_mf(probes[0], n, **kw)
        assert {k: r[k] for k in nothing} == nothing and "Mfcc" not in r["alloc"] and "MfccL" not in r["alloc"], kw


def test_behind_a_join_the_units_are_the_programmes(probes):
    wl, hop, _ = R.geometry(VOICE_HZ)
    n = [5000, 7001, 3000, 0]
    join = [(2, 100, 50), (-1, 0, 0), (2, 0, 333), (-1, 7, 0)]
    p = run_mf(probes[0], n, join=join, fb_flags=CENTER, order=2, cmvn=2)
    assert p["join"] == ["Join64", "f64"] and p["mfcc_src"] == "Join64"
    lens = [100 + 5000 + 50 + 3000 + 333, 7001, 7]
    assert [u[1] for u in p["units"]] == lens and len(p["mfcc"]) == 3
    assert [w["T"] for w in p["mfcc"]] == [R.n_frames(k, wl, hop, True) for k in lens]
    q = run_mf(probes[0], n, join=join, want=[16000, 0, 16000, 8000])  # a programme at another rate than its neighbour's
    assert [w["n_fft"] for w in q["mfcc"]] == [512, 2048, 256]
    assert [w["T"] for w in q["mfcc"]] == [R.n_frames(u[1], *R.geometry(u[0])[:2], False) for u in q["units"]]


@pytest.mark.parametrize("i16,rate,loudness,flac,fmt_bytes,adpcm",
                         list(itertools.product([False, True], [False, True], [False, True], [False, True], [0, 3],
                                                [False, True])))
def test_request_changes_no_other_field_and_a_plain_fbank_plan_is_unchanged(probes, i16, rate, loudness, flac, fmt_bytes,
                                                                          adpcm):
    for n in BATCHES.values():
        want = [22050] * len(n) if rate else None
        kw = dict(want=want, i16=i16, loudness=loudness, flac=flac, fmt_bytes=fmt_bytes, adpcm=adpcm)
        for fbank in (False, True):
            # the plan of the probe without the stage (a tree before it prints the same), field for field
            before = run_fb(probes[1], n, fbank=fbank, n_mels=64, **kw)
            off = run_mf(probes[0], n, mfcc=False, fbank=fbank, **kw)
            assert off.pop("mfcc_src") == "none" and off.pop("mfcc") == []
            assert off == before
            on = run_mf(probes[0], n, fbank=fbank, order=2, cmvn=2, **kw)
            src, units = on.pop("mfcc_src"), on.pop("mfcc")
            if i16:
                assert src == "none" and units == [] and "Mfcc" not in on["alloc"] and "MfccL" not in on["alloc"]
            else:
                assert src == on["final"][0] and len(units) == len(n)
                assert on["alloc"].pop("Mfcc")[1] == 1 and on["alloc"].pop("MfccL")[1] == 8
            assert on == before  # the fbank request's slab, places and bytes among them


def test_empty_batch(probes):
    p = run_mf(probes[0], [])
    assert p["mfcc"] == [] and p["mfcc_src"] == "V64" and p["alloc"] == {"MfccL": [2, 8], "Mfcc": [16, 1]}

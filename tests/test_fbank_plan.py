"""The filterbank stage in the output plan (jbonsai_amd/csrc/jb_output.h, plan_output) on the host, without a GPU: the
slab the stage reads, each unit's geometry by its own rate (behind a join: each programme's) and its 16-byte aligned
place in the feature slab -- and, without a request, the plan as it was.  A probe of its own
(tests/plan/fbank_probe.cpp), built the way tests/test_adpcm_plan.py builds its probe."""
import itertools
import json
import subprocess

import pytest

from tests import fbank_ref as R
from tests.test_adpcm_plan import build, run_ad
from tests.test_output_plan import BATCHES, VOICE_HZ

CENTER, F64 = 1, 8


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("fbank_plan")
    return build(d, "fbank_probe"), build(d, "adpcm_probe")


def run_fb(exe, n, fbank=True, win_us=25000, hop_us=10000, n_fft=0, n_mels=80, flags=0, want=None, join=None,
           i16=False, loudness=False, flac=False, fmt_bytes=0, adpcm=False, align=0):
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, int(adpcm), align,
            int(fbank), win_us, hop_us, n_fft, n_mels, flags, len(n), *n, *off, len(want or []), *(want or []),
            len(join or []), *[v for j in (join or []) for v in j]]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    p["fbank"] = [dict(zip(("off", "bytes", "T", "wl", "hop", "n_fft"), w)) for w in p["fbank"]]
    return p


def test_offsets_aligned_and_disjoint(probes):
    """23 filters of f32 (92 bytes a frame, no multiple of 16) over lengths around a window: every unit starts on a
    16-byte boundary, no two overlap, the byte counts are the geometry's and the slab holds them all."""
    wl, hop, _ = R.geometry(VOICE_HZ)
    n = [0, wl - 1, wl, wl + hop - 1, wl + hop, 5 * hop + wl + 1]
    for flags, elem in ((0, 4), (F64, 8), (CENTER, 4)):
        p = run_fb(probes[0], n, n_mels=23, flags=flags)
        T = [R.n_frames(k, wl, hop, bool(flags & CENTER)) for k in n]
        assert [w["T"] for w in p["fbank"]] == T and [w["bytes"] for w in p["fbank"]] == [t * 23 * elem for t in T]
        end = 0
        for w in p["fbank"]:
            assert w["off"] % 16 == 0 and w["off"] >= end
            end = w["off"] + w["bytes"]
        assert p["alloc"]["Feat"][1] == 1 and p["alloc"]["Feat"][0] >= end and p["alloc"]["Feat"][0] % 16 == 0
    p = run_fb(probes[0], n, n_mels=23)
    assert [w["off"] for w in p["fbank"]] == [0, 0, 0, 96, 192, 384]  # packed as tightly as the alignment allows


def test_geometry_follows_each_utterance_rate(probes):
    n = [30000] * 4
    want = [8000, 0, 22050, 16000]
    p = run_fb(probes[0], n, want=want)
    assert [w["hz"] for w in p["utt"]] == [8000, VOICE_HZ, 22050, 16000]
    for w, u in zip(p["fbank"], p["utt"]):
        wl, hop, n_fft = R.geometry(u["hz"])
        assert (w["wl"], w["hop"], w["n_fft"]) == (wl, hop, n_fft)
        assert w["T"] == R.n_frames(u["n"], wl, hop, False) and w["bytes"] == w["T"] * 80 * 4
    q = run_fb(probes[0], n, want=want, n_fft=4096)  # an explicit n_fft holds for every rate
    assert [w["n_fft"] for w in q["fbank"]] == [4096] * 4
    # options that one of the rates refuses are no request: the chain has refused them before
    r = run_fb(probes[0], n, want=want, n_fft=1024)  # 1200 samples at 48 kHz do not fit
    assert r["fbank_src"] == "none" and r["fbank"] == [] and "Feat" not in r["alloc"]


def test_behind_a_join_the_units_are_the_programmes(probes):
    wl, hop, _ = R.geometry(VOICE_HZ)
    n = [5000, 7001, 3000, 0]
    join = [(2, 100, 50), (-1, 0, 0), (2, 0, 333), (-1, 7, 0)]
    p = run_fb(probes[0], n, join=join, flags=CENTER)
    assert p["join"] == ["Join64", "f64"] and p["fbank_src"] == "Join64"
    lens = [100 + 5000 + 50 + 3000 + 333, 7001, 7]
    assert [u[1] for u in p["units"]] == lens and len(p["fbank"]) == 3
    assert [w["T"] for w in p["fbank"]] == [R.n_frames(k, wl, hop, True) for k in lens]
    # a programme at another rate than its neighbour's
    q = run_fb(probes[0], n, join=join, want=[16000, 0, 16000, 8000])
    assert [(w["wl"], w["n_fft"]) for w in q["fbank"]] == [(400, 512), (1200, 2048), (200, 256)]
    assert [w["T"] for w in q["fbank"]] == [R.n_frames(u[1], *R.geometry(u[0])[:2], False) for u in q["units"]]


@pytest.mark.parametrize("rate,loudness", list(itertools.product([False, True], repeat=2)))
def test_stage_reads_what_final_names(probes, rate, loudness):
    n = BATCHES["ragged"]
    want = [16000] * len(n) if rate else None
    p = run_fb(probes[0], n, want=want, loudness=loudness)
    assert p["fbank_src"] == p["final"][0] and p["final"][1] == "f64" and len(p["fbank"]) == len(n)
    # a 16-bit batch has no f64 for the stage (the chain refuses the request): nothing is planned
    q = run_fb(probes[0], n, want=want, loudness=loudness, i16=True)
    assert q["fbank_src"] == "none" and q["fbank"] == [] and "Feat" not in q["alloc"]


@pytest.mark.parametrize("i16,rate,loudness,flac,fmt_bytes,adpcm",
                         list(itertools.product([False, True], [False, True], [False, True], [False, True], [0, 3],
                                                [False, True])))
def test_request_changes_no_other_field_and_no_request_lists_nothing(probes, i16, rate, loudness, flac, fmt_bytes, adpcm):
    for n in BATCHES.values():
        want = [22050] * len(n) if rate else None
        kw = dict(want=want, i16=i16, loudness=loudness, flac=flac, fmt_bytes=fmt_bytes, adpcm=adpcm)
        before = run_ad(probes[1], n, **kw)  # the plan of a tree without the stage, field for field
        off = run_fb(probes[0], n, fbank=False, **kw)
        assert off.pop("fbank_src") == "none" and off.pop("fbank") == [] and "Feat" not in off["alloc"]
        assert off.pop("join") == ["none", "-"] and off.pop("units") == []
        assert off == before
        on = run_fb(probes[0], n, **kw)
        src, units = on.pop("fbank_src"), on.pop("fbank")
        if i16:
            assert src == "none" and units == [] and "Feat" not in on["alloc"]
        else:
            assert src == on["final"][0] and len(units) == len(n) and on["alloc"].pop("Feat")[1] == 1
        assert on.pop("join") == ["none", "-"] and on.pop("units") == []
        assert on == before


def test_empty_batch(probes):
    p = run_fb(probes[0], [])
    assert p["fbank"] == [] and p["fbank_src"] == "V64" and p["alloc"] == {"Feat": [16, 1]}

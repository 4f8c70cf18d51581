"""The mel spectrogram stage in the output plan (jbonsai_amd/csrc/jb_output.h, plan_output) on the host, without a GPU:
the slab the stage reads, each unit's frames (behind a join: each programme's), its 16-byte aligned place in the Mel
slab and, with a range, in the f64 scratch -- and, without a request, the plan as it was.  A probe of its own
(tests/plan/melspec_probe.cpp), built the way tests/test_adpcm_plan.py builds its probe."""
import itertools
import json
import subprocess

import pytest

from tests import melspec_ref as R
from tests.test_adpcm_plan import build
from tests.test_fbank_plan import run_fb
from tests.test_output_plan import BATCHES, VOICE_HZ

DROP_LAST, F64 = 2, 4


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("melspec_plan")
    return build(d, "melspec_probe"), build(d, "fbank_probe")


def run_ml(exe, n, melspec=True, n_fft=400, win=0, hop=160, n_mels=80, pad=R.REFLECT, flags=0, rng=0.0, want=None,
           join=None, i16=False, loudness=False, flac=False, fmt_bytes=0, adpcm=False, align=0):
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, int(adpcm), align,
            int(melspec), n_fft, win, hop, n_mels, pad, flags, rng, len(n), *n, *off, len(want or []), *(want or []),
            len(join or []), *[v for j in (join or []) for v in j]]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    p["melspec"] = [dict(zip(("off", "bytes", "T", "n_fft", "hop", "yoff"), w)) for w in p["melspec"]]
    return p


def test_offsets_aligned_and_disjoint(probes):
    """23 filters of f32 (92 bytes a frame, no multiple of 16) over lengths around half a transform and a hop: every
    unit starts on a 16-byte boundary, no two overlap, the byte counts are the geometry's and the slabs hold them all;
    the scratch of the range clamp is there with a range only, its units on 16-byte boundaries too."""
    N, H = 400, 160
    n = [0, N // 2, N // 2 + 1, H - 1, N, 5 * H + N + 1]
    for pad, flags, elem in ((R.REFLECT, 0, 4), (R.REFLECT, F64, 8), (R.ZERO, DROP_LAST, 4), (R.NONE, 0, 4)):
        for rng in (0.0, 8.0):
            p = run_ml(probes[0], n, n_mels=23, pad=pad, flags=flags, rng=rng)
            T = [R.n_frames(k, N, H, pad, bool(flags & DROP_LAST)) for k in n]
            assert [w["T"] for w in p["melspec"]] == T and [w["bytes"] for w in p["melspec"]] == [t * 23 * elem for t in T]
            assert all((w["n_fft"], w["hop"]) == (N, H) for w in p["melspec"])
            end = yend = 0
            for w, t in zip(p["melspec"], T):
                assert w["off"] % 16 == 0 and w["off"] >= end
                end = w["off"] + w["bytes"]
                if rng:
                    assert w["yoff"] % 2 == 0 and w["yoff"] >= yend
                    yend = w["yoff"] + t * 23
                else:
                    assert w["yoff"] == 0
            assert p["alloc"]["Mel"][1] == 1 and p["alloc"]["Mel"][0] >= end and p["alloc"]["Mel"][0] % 16 == 0
            assert ("MelY" in p["alloc"]) == bool(rng)
            if rng:
                assert p["alloc"]["MelY"][1] == 8 and p["alloc"]["MelY"][0] >= max(yend, 2)
    p = run_ml(probes[0], n, n_mels=23)
    assert [w["T"] for w in p["melspec"]] == [0, 0, 2, 0, 3, 8]
    assert [w["off"] for w in p["melspec"]] == [0, 0, 0, 192, 192, 480]  # packed as tightly as the alignment allows


def test_geometry_by_each_units_rate(probes):
    """Window and hop are in samples: the same N and H at every rate, so T follows each unit's own length; the band's
    upper edge is checked at each rate, and options that one of the rates refuses are no request."""
    n = [30000] * 4
    want = [8000, 0, 22050, 16000]
    p = run_ml(probes[0], n, want=want)
    assert [w["hz"] for w in p["utt"]] == [8000, VOICE_HZ, 22050, 16000]
    for w, u in zip(p["melspec"], p["utt"]):
        assert (w["n_fft"], w["hop"]) == (400, 160)
        assert w["T"] == R.n_frames(u["n"], 400, 160) and w["bytes"] == w["T"] * 80 * 4
    assert len({w["T"] for w in p["melspec"]}) == 4
    # (no field of the probe's input sets f_max; an n_fft no rate accepts stands for a refusal at some rate)
    r = run_ml(probes[0], n, want=want, n_fft=402)
    assert r["melspec_src"] == "none" and r["melspec"] == [] and "Mel" not in r["alloc"] and "MelY" not in r["alloc"]


def test_behind_a_join_the_units_are_the_programmes(probes):
    n = [5000, 7001, 3000, 0]
    join = [(2, 100, 50), (-1, 0, 0), (2, 0, 333), (-1, 7, 0)]
    p = run_ml(probes[0], n, join=join, rng=8.0)
    assert p["join"] == ["Join64", "f64"] and p["melspec_src"] == "Join64"
    lens = [100 + 5000 + 50 + 3000 + 333, 7001, 7]
    assert [u[1] for u in p["units"]] == lens and len(p["melspec"]) == 3
    assert [w["T"] for w in p["melspec"]] == [R.n_frames(k, 400, 160) for k in lens] == [54, 44, 0]
    q = run_ml(probes[0], n, join=join, want=[16000, 0, 16000, 8000], pad=R.NONE)
    assert [w["T"] for w in q["melspec"]] == [R.n_frames(u[1], 400, 160, R.NONE) for u in q["units"]]


@pytest.mark.parametrize("rate,loudness", list(itertools.product([False, True], repeat=2)))
def test_stage_reads_what_final_names(probes, rate, loudness):
    n = BATCHES["ragged"]
    want = [16000] * len(n) if rate else None
    p = run_ml(probes[0], n, want=want, loudness=loudness)
    assert p["melspec_src"] == p["final"][0] and p["final"][1] == "f64" and len(p["melspec"]) == len(n)
    # a 16-bit batch has no f64 for the stage (the chain refuses the request): nothing is planned
    q = run_ml(probes[0], n, want=want, loudness=loudness, i16=True)
    assert q["melspec_src"] == "none" and q["melspec"] == [] and "Mel" not in q["alloc"]


@pytest.mark.parametrize("i16,rate,loudness,flac,fmt_bytes,adpcm",
                         list(itertools.product([False, True], [False, True], [False, True], [False, True], [0, 3],
                                                [False, True])))
def test_request_changes_no_other_field_and_no_request_lists_nothing(probes, i16, rate, loudness, flac, fmt_bytes, adpcm):
    for n in BATCHES.values():
        want = [22050] * len(n) if rate else None
        kw = dict(want=want, i16=i16, loudness=loudness, flac=flac, fmt_bytes=fmt_bytes, adpcm=adpcm)
        before = run_fb(probes[1], n, fbank=False, **kw)  # the plan without either stage, field for field
        off = run_ml(probes[0], n, melspec=False, **kw)
        assert off.pop("melspec_src") == "none" and off.pop("melspec") == [] and "Mel" not in off["alloc"]
        assert off == before
        on = run_ml(probes[0], n, rng=8.0, **kw)
        src, units = on.pop("melspec_src"), on.pop("melspec")
        if i16:
            assert src == "none" and units == [] and "Mel" not in on["alloc"] and "MelY" not in on["alloc"]
        else:
            assert src == on["final"][0] and len(units) == len(n)
            assert on["alloc"].pop("Mel")[1] == 1 and on["alloc"].pop("MelY")[1] == 8
        assert on == before


def test_empty_batch(probes):
    p = run_ml(probes[0], [])
    assert p["melspec"] == [] and p["melspec_src"] == "V64" and p["alloc"] == {"Mel": [16, 1]}

"""The filter stage in the output plan (jbonsai_amd/csrc/jb_output.h: plan_output) on the host, without a GPU: the
routing over {f64, 16-bit} x {rate, none} x {loudness, none}, "fits" against New16, a request without sections as no
request, and the order against a join, a format and ADPCM.  A probe of its own (tests/plan/filter_probe.cpp), built the
way tests/test_adpcm_plan.py builds its probes."""
import itertools
import json
import subprocess

import pytest

from tests.test_adpcm_plan import build
from tests.test_join_plan import run_plan as run_join_plan
from tests.test_join_plan import words
from tests.test_output_plan import BATCHES, ROWS, VOICE_HZ, build_probe, run_probe

N4 = BATCHES["ragged"]


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_plan")
    return build(d, "filter_probe"), build_probe(d), build(d, "join_probe")


def run_plan(exe, n, filt=None, req=None, want=None, i16=False, loudness=False, flac=False, fmt_bytes=0, adpcm=False):
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, int(adpcm), 0, len(n), *n, *off,
            len(want or []), *(want or []), len(req or []), *words(req or []), len(filt or []), *(filt or [])]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    return p


@pytest.mark.parametrize("i16,rate,loudness", sorted(ROWS))
def test_routing_table(probes, i16, rate, loudness):
    """Behind the converter (or the vocoder), in front of the measurement: the stage reads that stage's f64; with a
    target it writes Filt64 and the measurement and the apply pass read it; without one it writes what is handed out."""
    for hz, out16 in ((16000, "S16"), (96000, "New16")) if rate else ((None, "S16"),):
        want = [hz] * len(N4) if hz else None
        p = run_plan(probes[0], N4, filt=[1, 0, 1, 1], want=want, i16=i16, loudness=loudness, flac=i16)
        plain = run_plan(probes[0], N4, want=want, i16=i16, loudness=loudness, flac=i16)
        # the stage in front writes f64, whatever the batch hands out
        assert p["vocoder"] == ["Voc64" if i16 else "V64", "f64"]
        assert p["converter"] == (["Conv64", "f64"] if rate else ["none", "-"])
        assert p["filter_src"] == ("Conv64" if rate else p["vocoder"][0])
        assert p["native64"] == p["vocoder"][0]  # the native read stays the unfiltered vocoder PCM
        assert p["active"] is True and p["convert"] == rate
        if loudness:
            assert p["filter"] == ["Filt64", "f64"] and p["measure"] == "Filt64"
            assert p["apply"] == plain["apply"] == ([out16, "i16"] if i16 else ["Apply64", "f64"])
            assert p["final"] == p["apply"]
        else:
            assert p["filter"] == ([out16, "i16"] if i16 else ["Filt64", "f64"])
            assert p["final"] == p["filter"] and p["apply"] == ["none", "-"] and p["measure"] == "none"
        assert p["flac"] == (p["final"][0] if i16 else "none")
        # the slabs: every slab a stage writes but the two of the batch as created
        written = {x[0] for x in (p["vocoder"], p["converter"], p["filter"], p["apply"])} - {"none", "V64", "S16"}
        assert set(p["alloc"]) == written
        for s in written:
            size = p["native_total"] if s == "Voc64" else p["total"]
            assert p["alloc"][s] == [max(size, 1), 2 if s == "New16" else 8]
        # the geometry is the plan's without the request
        assert p["utt"] == plain["utt"] and p["total"] == plain["total"]


def test_fits_against_new16(probes):
    n = [66480, 100800, 1680]
    down = run_plan(probes[0], n, filt=[1, 1, 1], want=[16000, 16000, 96000], i16=True)
    assert down["total"] <= down["native_total"] and down["filter"] == down["final"] == ["S16", "i16"]
    up = run_plan(probes[0], n, filt=[1, 1, 1], want=[96000, 16000, 96000], i16=True)
    assert up["total"] > up["native_total"] and up["filter"] == up["final"] == ["New16", "i16"]
    assert up["alloc"]["New16"] == [up["total"], 2]
    native = run_plan(probes[0], n, filt=[0, 0, 1], i16=True)
    assert native["filter"] == ["S16", "i16"] and native["vocoder"] == ["Voc64", "f64"]


@pytest.mark.parametrize("i16,rate,loudness,flac", list(itertools.product([False, True], repeat=4)))
def test_a_request_without_sections_is_no_request(probes, i16, rate, loudness, flac):
    """Field for field what tests/plan/output_probe.cpp prints for the same input, and what the plan without the
    request is in every other field."""
    want = [22050] * len(N4) if rate else None
    kw = dict(want=want, i16=i16, loudness=loudness, flac=flac)
    before = run_probe(probes[1], N4, **kw)
    for filt in (None, [0, 0, 0, 0]):
        p = run_plan(probes[0], N4, filt=filt, **kw)
        assert p["filter"] == ["none", "-"] and p["filter_src"] == "none" and "Filt64" not in p["alloc"]
        assert {k: p[k] for k in before} == before
    zero = run_plan(probes[0], N4, filt=[0, 0, 0, 0], fmt_bytes=0 if i16 else 3, adpcm=True, **kw)
    joined = run_join_plan(probes[2], N4, None, fmt_bytes=0 if i16 else 3, adpcm=True, **kw)
    assert {k: zero[k] for k in joined} == joined


@pytest.mark.parametrize("i16,rate,loudness", sorted(ROWS))
def test_the_encoders_and_the_join_follow_final(probes, i16, rate, loudness):
    want = [8000] * len(N4) if rate else None
    req = [(0, 10, 20, 0, 0), (0,), (None, 0, 5, 3, 3), (0,)]
    kw = dict(want=want, i16=i16, loudness=loudness, flac=i16, fmt_bytes=0 if i16 else 1, adpcm=True)
    p = run_plan(probes[0], N4, filt=[1, 1, 0, 1], **kw)
    assert p["adpcm_src"] == p["final"] and p["fmt_src"] == ("none" if i16 else p["final"][0])
    j = run_plan(probes[0], N4, filt=[1, 1, 0, 1], req=req, **kw)
    assert j["join_src"] == j["final"] == p["final"]
    assert j["join"] == (["Join16", "i16"] if i16 else ["Join64", "f64"])
    assert j["adpcm_src"] == j["join"] and j["fmt_src"] == ("none" if i16 else "Join64")
    assert j["flac"] == ("Join16" if i16 else "none")
    # the join's own geometry does not depend on the filter
    plain = run_plan(probes[0], N4, req=req, **kw)
    for key in ("units", "prog_of", "prog_start", "prog_first", "prog_members", "fmt", "adpcm"):
        assert j[key] == plain[key]


def test_empty_batch(probes):
    p = run_plan(probes[0], [], filt=[])
    assert p["filter"] == ["none", "-"] and p["alloc"] == {}
    p = run_plan(probes[0], [0, 0], filt=[1, 1], loudness=True)
    assert p["filter"] == ["Filt64", "f64"] and p["alloc"] == {"Filt64": [1, 8], "Apply64": [1, 8]}

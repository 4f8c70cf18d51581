"""The noise stage's place in the output plan, without a GPU: it is part of the filter stage -- the plan's filter flag
of an utterance is "a section, a response or a noise request", and the plan is field for field the filter plan of these
flags -- and what the host makes of a request (jb_noise.h: noise_fault, noise_ratio, noise_gain).  A probe of its own
(tests/plan/noise_probe.cpp, which runs tests/plan/filter_probe.cpp's printer), built the way tests/test_adpcm_plan.py
builds its probes."""
import itertools
import json
import subprocess

import pytest

from tests import noise_ref as R
from tests.test_adpcm_plan import build
from tests.test_filter_plan import run_plan as run_filter_plan
from tests.test_join_plan import words
from tests.test_output_plan import BATCHES, VOICE_HZ

N4 = BATCHES["ragged"]


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("noise_plan")
    return build(d, "noise_probe"), build(d, "filter_probe")


def run_plan(exe, n, filt=None, resp=None, noise=None, req=None, want=None, i16=False, loudness=False, flac=False,
             fmt_bytes=0, adpcm=False):
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, int(adpcm), 0, len(n), *n, *off,
            len(want or []), *(want or []), len(req or []), *words(req or []), len(filt or []), *(filt or []),
            len(resp or []), *(resp or []), len(noise or []), *(noise or [])]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    first, rest = r.stdout.split("\n", 1)
    p = json.loads(rest)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    return json.loads(first)["flags"], p


@pytest.mark.parametrize("i16,rate,loudness", list(itertools.product([False, True], repeat=3)))
def test_the_flag_is_a_section_a_response_or_a_noise_request(probes, i16, rate, loudness):
    """Utterance 0: noise only; 1: sections and noise; 2: a response only; 3: none of the three.  The plan is the
    filter plan of the flags [1, 1, 1, 0], field for field, and the geometry is the plan's without any request."""
    want = [16000] * len(N4) if rate else None
    kw = dict(want=want, i16=i16, loudness=loudness, flac=i16)
    flags, p = run_plan(probes[0], N4, filt=[0, 1, 0, 0], resp=[0, 0, 1, 0], noise=[1, 1, 0, 0], **kw)
    assert flags == [1, 1, 1, 0]
    assert p == run_filter_plan(probes[1], N4, filt=[1, 1, 1, 0], **kw)
    assert p["filter"][0] != "none" and p["filter_src"] == ("Conv64" if rate else p["vocoder"][0])
    assert p["native64"] == p["vocoder"][0]  # the native read stays the vocoder's PCM
    plain = run_filter_plan(probes[1], N4, **kw)
    assert p["utt"] == plain["utt"] and p["total"] == plain["total"]


def test_each_request_alone_and_none(probes):
    # a noise request alone: no filter entries and no responses at all
    flags, p = run_plan(probes[0], N4, noise=[1, 0, 0, 1], loudness=True)
    assert flags == [1, 0, 0, 1]
    assert p == run_filter_plan(probes[1], N4, filt=[1, 0, 0, 1], loudness=True)
    assert p["filter"] == ["Filt64", "f64"] and p["measure"] == "Filt64"
    # all three on one utterance, and each pair
    for filt, resp, noise in (([1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]), (None, [1, 0, 0, 0], [1, 0, 0, 0]),
                              ([1, 0, 0, 0], None, [1, 0, 0, 0])):
        flags, p = run_plan(probes[0], N4, filt=filt, resp=resp, noise=noise)
        assert flags == [1, 0, 0, 0] and p == run_filter_plan(probes[1], N4, filt=[1, 0, 0, 0])
    # the other two alone: the flags are their own
    flags, p = run_plan(probes[0], N4, filt=[0, 1, 0, 0], resp=[0, 0, 1, 0])
    assert flags == [0, 1, 1, 0] and p == run_filter_plan(probes[1], N4, filt=[0, 1, 1, 0])
    # none, and requests that name no utterance: the plan without the stage
    none = run_filter_plan(probes[1], N4)
    for filt, resp, noise in ((None, None, None), (None, None, [0] * 4), ([0] * 4, [0] * 4, [0] * 4)):
        flags, p = run_plan(probes[0], N4, filt=filt, resp=resp, noise=noise)
        assert not any(flags) and p == none
        assert p["filter"] == ["none", "-"] and p["filter_src"] == "none" and "Filt64" not in p["alloc"]


def test_sixteen_bit_without_loudness_writes_what_is_handed_out(probes):
    flags, p = run_plan(probes[0], N4, noise=[1, 1, 1, 1], i16=True)
    assert flags == [1, 1, 1, 1] and p["filter"] == p["final"] == ["S16", "i16"] and p["vocoder"] == ["Voc64", "f64"]


def ask(exe, snr, gate=0.0, ref=0):
    r = subprocess.run([str(exe)], input=f"request {snr} {gate} {ref}\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_an_infinite_snr_is_a_request_that_copies(probes):
    """snr_db = +INFINITY is accepted, counts as a request (the utterance is flagged and the stage copies it) and gives
    the gain 0; a finite one gives the rule's gain with r rounded once from long double."""
    got = ask(probes[0], "inf")
    assert got == {"fault": None, "none": 0, "r": "inf", "gain": 0.0}
    for snr in (-40.0, -3.0, 0.0, 15.0, 100.0):
        got = ask(probes[0], snr)
        r = R.ratio(snr)
        assert got["fault"] is None and got["none"] == 0 and got["r"] == r
        assert got["gain"] == (((4.0 * 4.0) / (8.0 * 2.0)) / r) ** 0.5
    assert "snr_db" in ask(probes[0], 100.25)["fault"] and "snr_db" in ask(probes[0], "nan")["fault"]
    assert "gate_db" in ask(probes[0], 10.0, 0.0, 1)["fault"] and ask(probes[0], 10.0, 20.0, 1)["fault"] is None

"""The pitch stage in the output plan (jbonsai_amd/csrc/jb_output.h, plan_output) on the host, without a GPU: the slab
the stage reads (pitch_src: what fbank_src would name), each unit's frames, its 16-byte aligned places in the stage's
byte block and in its 4 kHz block and the blocks' sizes, the [P] units behind a join and a mix and the [P + S] units
with stems -- and, without a request, the plan field for field as it is without one.  A probe of its own
(tests/plan/pitch_probe.cpp), built the way tests/test_adpcm_plan.py builds its probe."""
import itertools
import json
import subprocess

import pytest

from tests.test_adpcm_plan import build
from tests.test_output_plan import VOICE_HZ

KALDI, F64, RAW, RAW_LOG = 1, 1, 2, 4
KEYS = ("off", "bytes", "T", "width", "elem", "n4", "yoff")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pitch_plan"), "pitch_probe")


def run(exe, n, pitch=True, win_us=25000, hop_us=10000, grid=KALDI, flags=0, want=None, join=None, mix=None, i16=False,
        loudness=False):
    off = [0] + list(itertools.accumulate(n))[:-1]
    mode = 1 if join else 2 if mix else 0
    nums = [VOICE_HZ, int(i16), int(loudness), int(pitch), win_us, hop_us, grid, flags, len(n), *n, *off,
            len(want or []), *(want or []), mode, *[v for j in (join or mix or []) for v in j]]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    p["pitch"] = [dict(zip(KEYS, w)) for w in p["pitch"]]
    return p


def frames(n, hz, grid, win_us=25000, hop_us=10000):
    wl, hop = (hz * win_us + 500000) // 1000000, (hz * hop_us + 500000) // 1000000
    return (n + hop // 2) // hop if grid == KALDI else (1 + (n - wl) // hop if n >= wl else 0)


def check_places(p, units, grid, width, elem):
    """units: (hz, n) of every unit the stage takes"""
    assert len(p["pitch"]) == len(units)
    end, yend = 0, 0
    for w, (hz, n) in zip(p["pitch"], units):
        assert (w["T"], w["width"], w["elem"]) == (frames(n, hz, grid), width, elem)
        assert w["bytes"] == w["T"] * width * elem and w["n4"] == -(-n * 4000 // hz)
        assert w["off"] % 16 == 0 and w["off"] == end and (w["yoff"] * 8) % 16 == 0 and w["yoff"] == yend
        end = w["off"] + (w["bytes"] + 15) // 16 * 16
        yend = w["yoff"] + (w["n4"] + 1) // 2 * 2
    assert p["pitch_bytes"] == max(end, 16) and p["pitch_words"] == max(yend, 2)


@pytest.mark.parametrize("grid", [0, KALDI])
@pytest.mark.parametrize("flags,width,elem", [(0, 3, 4), (F64, 3, 8), (RAW, 2, 4), (RAW_LOG | F64, 4, 8)])
def test_places_are_aligned_and_packed(probe, grid, flags, width, elem):
    wl, hop = 1200, 480
    n = [0, 1, wl - 1, wl, wl + hop, 7 * hop + hop // 2 - 1, 7 * hop + hop // 2, 50001]
    p = run(probe, n, grid=grid, flags=flags)
    assert p["pitch_src"] == p["final_slab"] != 0
    check_places(p, [(VOICE_HZ, k) for k in n], grid, width, elem)
    q = run(probe, n, grid=grid, flags=flags, want=[16000] * len(n), loudness=True)  # behind the converter
    assert q["pitch_src"] == q["final_slab"] and q["convert"] == 1
    check_places(q, [(16000, u[3]) for u in q["utt"]], grid, width, elem)


def test_without_the_request_the_plan_is_the_parents(probe):
    n = [66480, 0, 420 * 240, 7 * 240]
    for kw in (dict(), dict(want=[16000, 0, 44100, 8000], loudness=True), dict(join=[(0, 10, 20), (-1, 0, 0), (0, 0, 5), (1, 0, 0)]),
               dict(mix=[(0, 0, 0, 0), (0, 500, 9, 1), (-1, 0, 0, -1), (0, 77, 0, 0)]), dict(i16=True)):
        with_, without = run(probe, n, **kw), run(probe, n, pitch=False, **kw)
        assert without["pitch_src"] == 0 and without["pitch"] == [] and without["pitch_bytes"] == without["pitch_words"] == 0
        for key in with_:  # every other field: the routing, every slab's size, the utterances, the units, the other sinks
            if not key.startswith("pitch"):
                assert with_[key] == without[key], (kw, key)
    assert run(probe, n, i16=True)["pitch_src"] == 0  # a 16-bit batch has no f64 for the stage
    assert run(probe, n, want=[16000, 0, 3000, 0])["pitch_src"] == 0  # a rate under the analysis rate: no request


def test_units_behind_a_join_a_mix_and_stems(probe):
    n = [4800, 9600, 2400, 7200]
    p = run(probe, n, join=[(0, 10, 20), (-1, 0, 0), (0, 0, 5), (-1, 3, 3)], flags=F64)
    assert p["n_progs"] == 3 == len(p["units"]) and p["pitch_src"] == p["join_slab"] != p["final_slab"]
    check_places(p, [(u[0], u[1]) for u in p["units"]], KALDI, 3, 8)  # [P]: a programme's T is its whole length's
    assert p["units"][0][1] == 10 + 4800 + 20 + 2400 + 5
    m = run(probe, n, mix=[(0, 0, 0, -1), (0, 500, 9, -1), (-1, 0, 0, -1), (0, 77, 0, -1)])
    assert m["mixed"] == 1 and m["n_progs"] == 2 == len(m["units"]) and m["pitch_src"] == m["join_slab"]
    check_places(m, [(u[0], u[1]) for u in m["units"]], KALDI, 3, 4)
    s = run(probe, n, mix=[(0, 0, 0, 0), (0, 500, 9, 1), (-1, 0, 0, -1), (0, 77, 0, 0)])
    assert s["n_progs"] == 2 and len(s["units"]) == 4  # [P + S]: two stems behind the two programmes
    check_places(s, [(u[0], u[1]) for u in s["units"]], KALDI, 3, 4)
    assert [u[1] for u in s["units"][2:]] == [s["units"][0][1]] * 2  # stems in programme coordinates

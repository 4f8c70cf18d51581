"""The convolution stage on the host, without a GPU: the geometry of a tap count (jb_fir.h: fir_geometry, and the same
through jb_fir_geometry), and the stage's place in the output plan -- it is part of the filter stage: the plan's filter
flag of an utterance is "a section or a response", and the plan is field for field the filter plan of these flags.
A probe of its own (tests/plan/fir_probe.cpp, which runs tests/plan/filter_probe.cpp's printer), built the way
tests/test_adpcm_plan.py builds its probes."""
import itertools
import json
import subprocess

import pytest

import jbonsai_amd as J
from tests.test_adpcm_plan import build
from tests.test_filter_plan import run_plan as run_filter_plan
from tests.test_join_plan import words
from tests.test_output_plan import BATCHES, VOICE_HZ

N4 = BATCHES["ragged"]

# K -> (mode, block, partitions, n_fft): direct up to 256 taps; blocks of 1024 up to 4096 taps, of 2048 above
GEOMETRY = {
    1: (0, 2048, 1, 0), 256: (0, 2048, 1, 0), 257: (1, 1024, 1, 2048),
    1024: (1, 1024, 1, 2048), 1025: (1, 1024, 2, 2048), 2 * 1024 + 3: (1, 1024, 3, 2048),
    4096: (1, 1024, 4, 2048), 4097: (1, 2048, 3, 4096),
    2048: (1, 1024, 2, 2048), 2049: (1, 1024, 3, 2048), 2 * 2048 + 3: (1, 2048, 3, 4096), 5000: (1, 2048, 3, 4096),
    24000: (1, 2048, 12, 4096), 131072: (1, 2048, 64, 4096),
}


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("fir_plan")
    return build(d, "fir_probe"), build(d, "filter_probe")


def test_geometry_of_a_tap_count(probes):
    ks = sorted(GEOMETRY)
    r = subprocess.run([str(probes[0])], input="geometry " + " ".join(map(str, ks)) + "\n", capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [tuple(json.loads(line)) for line in r.stdout.splitlines()]
    assert got == [GEOMETRY[k] for k in ks]
    for k in ks:
        mode, block, parts, n_fft = GEOMETRY[k]
        assert J.fir_geometry(k) == (mode, block, parts)  # the C entry says the same
        if mode == J.FIR_PARTITIONED:
            assert block == n_fft // 2 and parts == -(-k // block) and (parts - 1) * block < k <= parts * block
        else:
            assert k <= J.FIR_DIRECT_MAX and parts == 1
    assert J.FIR_DIRECT_MAX == 256 and J.FIR_MAX_TAPS == 131072
    for bad in (0, 131073):
        with pytest.raises(J.JbError, match="n_taps"):
            J.fir_geometry(bad)


def run_plan(exe, n, filt=None, resp=None, req=None, want=None, i16=False, loudness=False, flac=False, fmt_bytes=0,
             adpcm=False):
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, int(adpcm), 0, len(n), *n, *off,
            len(want or []), *(want or []), len(req or []), *words(req or []), len(filt or []), *(filt or []),
            len(resp or []), *(resp or [])]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    first, rest = r.stdout.split("\n", 1)
    p = json.loads(rest)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    return json.loads(first)["flags"], p


@pytest.mark.parametrize("i16,rate,loudness", list(itertools.product([False, True], repeat=3)))
def test_the_flag_is_a_section_or_a_response(probes, i16, rate, loudness):
    """Utterance 0: a response only; 1: sections only; 2: both; 3: neither.  The plan is the filter plan of the flags
    [1, 1, 1, 0], field for field, and the geometry is the plan's without any request."""
    want = [16000] * len(N4) if rate else None
    kw = dict(want=want, i16=i16, loudness=loudness, flac=i16)
    flags, p = run_plan(probes[0], N4, filt=[0, 1, 1, 0], resp=[1, 0, 1, 0], **kw)
    assert flags == [1, 1, 1, 0]
    assert p == run_filter_plan(probes[1], N4, filt=[1, 1, 1, 0], **kw)
    assert p["filter"][0] != "none" and p["filter_src"] == ("Conv64" if rate else p["vocoder"][0])
    assert p["native64"] == p["vocoder"][0]  # the native read stays the vocoder's PCM
    plain = run_filter_plan(probes[1], N4, **kw)
    assert p["utt"] == plain["utt"] and p["total"] == plain["total"]


def test_each_request_alone_and_none(probes):
    # a convolution request alone: no filter entries at all
    flags, p = run_plan(probes[0], N4, resp=[1, 0, 0, 1], loudness=True)
    assert flags == [1, 0, 0, 1]
    assert p == run_filter_plan(probes[1], N4, filt=[1, 0, 0, 1], loudness=True)
    assert p["filter"] == ["Filt64", "f64"] and p["measure"] == "Filt64"
    # sections alone: the flags are the filter's own
    flags, p = run_plan(probes[0], N4, filt=[0, 1, 0, 0])
    assert flags == [0, 1, 0, 0] and p == run_filter_plan(probes[1], N4, filt=[0, 1, 0, 0])
    # neither, and requests that name no utterance: the plan without the stage
    none = run_filter_plan(probes[1], N4)
    for filt, resp in ((None, None), ([0] * 4, None), (None, [0] * 4), ([0] * 4, [0] * 4)):
        flags, p = run_plan(probes[0], N4, filt=filt, resp=resp)
        assert not any(flags) and p == none
        assert p["filter"] == ["none", "-"] and p["filter_src"] == "none" and "Filt64" not in p["alloc"]


def test_sixteen_bit_without_loudness_writes_what_is_handed_out(probes):
    flags, p = run_plan(probes[0], N4, resp=[1, 1, 1, 1], i16=True)
    assert flags == [1, 1, 1, 1] and p["filter"] == p["final"] == ["S16", "i16"] and p["vocoder"] == ["Voc64", "f64"]

"""The routing of the stages behind the vocoder (jbonsai_amd/csrc/jb_output.h, plan_output) on the host, without a
GPU: which slab the vocoder, the converter and the loudness apply pass write and in which type, what the measurement
and FLAC read, what the PCM read entries hand out, the slabs to allocate, and each utterance's output rate, L/M, length
and offset.  A small C++ probe (tests/plan/output_probe.cpp) is compiled with g++ against jb_output.cpp, reads a batch
and its requests on stdin and prints the plan as JSON.  ROWS is the table of DESIGN.md section 3; the lengths are the
ones tests/test_gpu_resample.py pins on the device."""
import itertools
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"
VOICE_HZ, FPERIOD = 48000, 240
SENTENCE = 277 * FPERIOD  # 66,480 samples
BATCHES = {"one": [SENTENCE], "ragged": [SENTENCE, 0, 420 * FPERIOD, 7 * FPERIOD]}


def build_probe(out_dir):
    exe = Path(out_dir) / "output_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "output_probe.cpp"), str(CSRC / "jb_output.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("output_plan"))


def run_probe(exe, n, want=None, i16=False, loudness=False, flac=False, voice_hz=VOICE_HZ):
    """The plan of a batch of len(n) utterances of n[u] native samples, packed; want None = no rate requested."""
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [voice_hz, int(i16), int(loudness), int(flac), len(n), *n, *off, len(want or []), *(want or [])]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    return p


def ceil_div(a, b):
    return -(-a // b)


# (16-bit sink, output rate, loudness) -> vocoder writes, converter writes, apply writes, measurement reads, handed out,
# native f64.  OUT16: the 16-bit slab of the batch as created (S16) if the output fits, else a new one (New16)
OUT16 = "OUT16"
ROWS = {
    (False, False, False): (("V64", "f64"), None, None, None, "V64", "V64"),
    (True, False, False): (("S16", "i16"), None, None, None, "S16", None),
    (False, True, False): (("V64", "f64"), ("Conv64", "f64"), None, None, "Conv64", "V64"),
    (True, True, False): (("Voc64", "f64"), (OUT16, "i16"), None, None, OUT16, "Voc64"),
    (False, False, True): (("V64", "f64"), None, ("Apply64", "f64"), "V64", "Apply64", "V64"),
    (True, False, True): (("Voc64", "f64"), None, ("S16", "i16"), "Voc64", "S16", "Voc64"),
    (False, True, True): (("V64", "f64"), ("Conv64", "f64"), ("Apply64", "f64"), "Conv64", "Apply64", "V64"),
    (True, True, True): (("Voc64", "f64"), ("Conv64", "f64"), (OUT16, "i16"), "Conv64", OUT16, "Voc64"),
}


def check_row(p, i16, rate, loudness, flac, out16):
    voc, conv, app, measure, final, native = ROWS[i16, rate, loudness]

    def w(x):
        return ["none", "-"] if x is None else [out16 if x[0] == OUT16 else x[0], x[1]]
    final = out16 if final == OUT16 else final
    assert p["vocoder"] == w(voc) and p["converter"] == w(conv) and p["apply"] == w(app), p
    assert p["measure"] == (measure or "none") and p["native64"] == (native or "none"), p
    assert p["final"] == [final, "i16" if i16 else "f64"], p
    assert p["convert"] == rate and p["active"] == (rate or loudness), p
    # FLAC reads the 16-bit slab handed out (and nothing of an f64 batch, which jb_batch_set_flac refuses at once)
    assert p["flac"] == (final if flac and i16 else "none"), p
    # the slabs to allocate: every slab a stage writes but the two the batch was created with, the vocoder's at the
    # native size, the others at the output's; never an empty block
    written = {x[0] for x in (p["vocoder"], p["converter"], p["apply"])} - {"none", "V64", "S16"}
    assert set(p["alloc"]) == written, p
    for s, (count, elem) in p["alloc"].items():
        assert count == max(p["native_total"] if s == "Voc64" else p["total"], 1) and elem == (2 if s == "New16" else 8)


def check_geometry(p, n, hz):
    """Each utterance's rate, reduced L/M, ceil(n L / M) samples, and the plain prefix sum of those as its offset."""
    from math import gcd
    off = 0
    for u, w in enumerate(p["utt"]):
        g = gcd(VOICE_HZ, hz[u])
        assert (w["hz"], w["L"], w["M"]) == (hz[u], hz[u] // g, VOICE_HZ // g), (u, w)
        assert w["n"] == ceil_div(n[u] * w["L"], w["M"]) and w["off"] == off, (u, w)
        off += w["n"]
    assert p["total"] == off and p["native_total"] == sum(n)


@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize("flac", [False, True])
@pytest.mark.parametrize("i16,rate,loudness", sorted(ROWS))
def test_routing_table(probe, batch, i16, rate, loudness, flac):
    """All eight rows, for one utterance and for a ragged batch with an empty utterance; rates that go down (the
    16-bit output fits the slab the batch was created with) and up to 96 kHz (it does not)."""
    n = BATCHES[batch]
    for hz, out16 in ((16000, "S16"), (96000, "New16")) if rate else ((None, "S16"),):
        p = run_probe(probe, n, want=[hz] * len(n) if hz else None, i16=i16, loudness=loudness, flac=flac)
        check_row(p, i16, rate, loudness, flac, out16)
        check_geometry(p, n, [hz or VOICE_HZ] * len(n))


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("want", [[0, 0, 0, 0], [VOICE_HZ] * 4, [0, VOICE_HZ, 0, VOICE_HZ]])
def test_all_native_request_is_no_request(probe, want, i16):
    """A rate request whose entries are all native converts nothing and allocates nothing: the batch as created."""
    n = BATCHES["ragged"]
    for loudness in (False, True):
        p = run_probe(probe, n, want=want, i16=i16, loudness=loudness)
        assert p == run_probe(probe, n, i16=i16, loudness=loudness)
        check_row(p, i16, False, loudness, False, "S16")
        assert p["alloc"] == {} or loudness


@pytest.mark.parametrize("i16", [False, True])
def test_mixed_rates_identity_routing(probe, i16):
    """[0, 16000, native]: the batch converts, and its native utterances go through the converter too (L/M = 1/1: the
    identity table), packed with the others in the converter's slab."""
    n = [SENTENCE, 420 * FPERIOD, 7 * FPERIOD]
    p = run_probe(probe, n, want=[0, 16000, VOICE_HZ], i16=i16)
    check_row(p, i16, True, False, False, "S16")
    check_geometry(p, n, [VOICE_HZ, 16000, VOICE_HZ])
    assert [(w["L"], w["M"], w["n"]) for w in p["utt"]] == [(1, 1, n[0]), (1, 3, n[1] // 3), (1, 1, n[2])]
    # some utterances up, some down: the sum decides whether the created 16-bit slab is reused
    up = run_probe(probe, n, want=[96000, 16000, 96000], i16=True)
    assert up["total"] > up["native_total"] and up["final"] == ["New16", "i16"]
    down = run_probe(probe, n, want=[16000, 16000, 96000], i16=True)
    assert down["total"] <= down["native_total"] and down["final"] == ["S16", "i16"]


@pytest.mark.parametrize("hz,L,M,n_out", [(22050, 147, 320, 30540), (24000, 1, 2, 33240), (16000, 1, 3, 22160)])
def test_lengths_pinned_on_the_device(probe, hz, L, M, n_out):
    """The 277-frame sentence (66,480 samples at 48 kHz), as tests/test_gpu_resample.py reads them off a batch."""
    p = run_probe(probe, [SENTENCE], want=[hz])
    assert p["utt"] == [dict(hz=hz, L=L, M=M, n=n_out, off=0)] and p["total"] == n_out


def test_offsets_without_conversion_are_the_native_ones(probe):
    n = BATCHES["ragged"]
    p = run_probe(probe, n, loudness=True, i16=True, flac=True)
    assert [w["off"] for w in p["utt"]] == [0, n[0], n[0], n[0] + n[2]] and [w["n"] for w in p["utt"]] == n
    assert p["total"] == p["native_total"] == sum(n)


def test_empty_batches(probe):
    """No utterance, or none with a sample: the plan stands, and a slab to allocate is never empty."""
    p = run_probe(probe, [], want=None, i16=True, loudness=True, flac=True)
    assert p["utt"] == [] and p["total"] == 0 and p["alloc"] == {"Voc64": [1, 8]} and p["flac"] == "S16"
    p = run_probe(probe, [0, 0], want=[16000, 96000], loudness=True)
    assert p["convert"] and p["total"] == 0 and p["alloc"] == {"Conv64": [1, 8], "Apply64": [1, 8]}

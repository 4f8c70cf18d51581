"""The IMA ADPCM stage in the output plan (jbonsai_amd/csrc/jb_output.h, plan_output) on the host, without a GPU: the
slab the stage reads (f64 or 16-bit), each utterance's block size and its 16-byte aligned place in the byte slab -- and,
without a request, the plan as it was.  A probe of its own (tests/plan/adpcm_probe.cpp), built the way
tests/test_format_plan.py builds its probe."""
import itertools
import json
import subprocess
from pathlib import Path

import pytest

from tests import adpcm_ref as R
from tests.test_format_plan import run_fmt
from tests.test_output_plan import BATCHES, CSRC, ROOT, VOICE_HZ


def build(d, name):
    exe = Path(d) / name
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / (name + ".cpp")), str(CSRC / "jb_output.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("adpcm_plan")
    return build(d, "adpcm_probe"), build(d, "format_probe")


def run_ad(exe, n, adpcm=True, align=0, want=None, i16=False, loudness=False, flac=False, fmt_bytes=0):
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, int(adpcm), align, len(n), *n, *off,
            len(want or []), *(want or [])]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    return p


def test_offsets_aligned_and_disjoint(probes):
    """A = 36 (no multiple of 16) over lengths around a block: every utterance starts on a 16-byte boundary, no two
    overlap, the byte counts are the geometry's and the slab holds them all."""
    n = [0, 1, 65, 66, 130, 5]
    p = run_ad(probes[0], n, align=36)
    assert [w[1] for w in p["adpcm"]] == [R.geometry(VOICE_HZ, k, 36)[3] for k in n] == [0, 36, 36, 72, 72, 36]
    assert all(w[2] == 36 for w in p["adpcm"])
    end = 0
    for off, nbytes, _ in p["adpcm"]:
        assert off % 16 == 0 and off >= end
        end = off + nbytes
    assert p["alloc"]["Adpcm"][1] == 1 and p["alloc"]["Adpcm"][0] >= end and p["alloc"]["Adpcm"][0] % 16 == 0
    assert [w[0] for w in p["adpcm"]] == [0, 0, 48, 96, 176, 256]  # packed as tightly as the alignment allows


def test_block_size_follows_each_utterance_rate(probes):
    """Mixed rates in one batch under block_align 0: 256 / 512 / 1024 by each utterance's own output rate."""
    n = [3000, 3000, 3000, 3000]
    want = [8000, 0, 22050, 44100]
    p = run_ad(probes[0], n, want=want)
    assert [w["hz"] for w in p["utt"]] == [8000, VOICE_HZ, 22050, 44100]
    assert [w[2] for w in p["adpcm"]] == [256, R.block_align(VOICE_HZ), 512, 1024]
    assert [w[1] for w in p["adpcm"]] == [R.geometry(w["hz"], w["n"])[3] for w in p["utt"]]
    # an explicit size holds for every rate
    q = run_ad(probes[0], n, align=128, want=want)
    assert [w[2] for w in q["adpcm"]] == [128] * 4


@pytest.mark.parametrize("i16,rate,loudness", list(itertools.product([False, True], repeat=3)))
def test_stage_reads_what_final_names(probes, i16, rate, loudness):
    """f64 against 16-bit: the source is the slab the read entries hand out, in its type."""
    n = BATCHES["ragged"]
    want = [16000] * len(n) if rate else None
    p = run_ad(probes[0], n, want=want, i16=i16, loudness=loudness)
    assert p["adpcm_src"] == p["final"] and p["final"][1] == ("i16" if i16 else "f64")
    assert len(p["adpcm"]) == len(n)


@pytest.mark.parametrize("i16,rate,loudness,flac,fmt_bytes",
                         [c for c in itertools.product([False, True], [False, True], [False, True], [False, True],
                                                       [0, 3])])
def test_request_changes_no_other_field_and_no_request_lists_nothing(probes, i16, rate, loudness, flac, fmt_bytes):
    for n in BATCHES.values():
        want = [22050] * len(n) if rate else None
        kw = dict(want=want, i16=i16, loudness=loudness, flac=flac)
        before = run_fmt(probes[1], n, fmt_bytes, **kw)  # the plan of a tree without the stage, field for field
        off = run_ad(probes[0], n, adpcm=False, fmt_bytes=fmt_bytes, **kw)
        assert off.pop("adpcm_src") == ["none", "-"] and off.pop("adpcm") == [] and "Adpcm" not in off["alloc"]
        assert off == before
        on = run_ad(probes[0], n, fmt_bytes=fmt_bytes, **kw)
        assert on.pop("adpcm_src")[0] != "none" and len(on.pop("adpcm")) == len(n)
        assert on["alloc"].pop("Adpcm")[1] == 1
        assert on == before


def test_empty_batch(probes):
    p = run_ad(probes[0], [])
    assert p["adpcm"] == [] and p["adpcm_src"] == ["V64", "f64"] and p["alloc"] == {"Adpcm": [16, 1]}

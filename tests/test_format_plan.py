"""The format stage in the output plan (jbonsai_amd/csrc/jb_output.h, plan_output) on the host, without a GPU: the f64
slab the stage reads, each utterance's 16-byte aligned place in the byte slab, the slab's size -- and, without a
request, the plan as it was.  A probe of its own (tests/plan/format_probe.cpp), built the way tests/test_output_plan.py
builds its probe."""
import itertools
import json
import subprocess
from pathlib import Path

import pytest

from tests.test_output_plan import BATCHES, CSRC, ROOT, VOICE_HZ, build_probe, run_probe


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("format_plan")
    exe = Path(d) / "format_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "format_probe.cpp"), str(CSRC / "jb_output.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, build_probe(d)


def run_fmt(exe, n, fmt_bytes, want=None, i16=False, loudness=False, flac=False):
    off = [0] + list(itertools.accumulate(n))[:-1]
    nums = [VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, len(n), *n, *off, len(want or []), *(want or [])]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    return p


def test_offsets_aligned_and_disjoint(probes):
    """Lengths {0, 1, 5, 16, 17} at 3 bytes per sample: every utterance starts on a 16-byte boundary, no two overlap,
    the byte counts are n * 3 and the slab holds them all."""
    n = [0, 1, 5, 16, 17]
    p = run_fmt(probes[0], n, 3)
    assert [w[1] for w in p["fmt"]] == [3 * k for k in n]
    end = 0
    for off, nbytes in p["fmt"]:
        assert off % 16 == 0 and off >= end
        end = off + nbytes
    assert p["alloc"]["Fmt"][1] == 1 and p["alloc"]["Fmt"][0] >= end and p["alloc"]["Fmt"][0] % 16 == 0
    # packed as tightly as the alignment allows
    assert [w[0] for w in p["fmt"]] == [0, 0, 16, 32, 80]


@pytest.mark.parametrize("rate,loudness,src", [(False, False, "V64"), (True, False, "Conv64"),
                                               (False, True, "Apply64"), (True, True, "Apply64")])
@pytest.mark.parametrize("fmt_bytes", [1, 2, 3, 4])
def test_stage_reads_the_final_f64(probes, rate, loudness, src, fmt_bytes):
    n = BATCHES["ragged"]
    p = run_fmt(probes[0], n, fmt_bytes, want=[16000] * len(n) if rate else None, loudness=loudness)
    assert p["fmt_src"] == src == p["final"][0] and p["final"][1] == "f64"
    assert [w[1] for w in p["fmt"]] == [w["n"] * fmt_bytes for w in p["utt"]]
    assert all(w[0] % 16 == 0 for w in p["fmt"])
    # the other stages are routed as without the format
    q = run_fmt(probes[0], n, 0, want=[16000] * len(n) if rate else None, loudness=loudness)
    for k in ("vocoder", "converter", "apply", "final", "measure", "native64", "utt", "total", "convert"):
        assert p[k] == q[k], k
    assert {k: v for k, v in p["alloc"].items() if k != "Fmt"} == q["alloc"]


def test_a_16_bit_batch_has_no_format_stage(probes):
    """The stage reads f64: a JB_BATCH_PCM_I16 plan has none (jb_batch_set_format refuses such a batch at once)."""
    p = run_fmt(probes[0], BATCHES["ragged"], 2, i16=True, flac=True)
    assert p["fmt_src"] == "none" and p["fmt"] == [] and "Fmt" not in p["alloc"] and p["flac"] == "S16"


@pytest.mark.parametrize("i16,rate,loudness,flac", list(itertools.product([False, True], repeat=4)))
def test_no_request_is_the_plan_of_today(probes, i16, rate, loudness, flac):
    """Field for field what tests/plan/output_probe.cpp prints, and no format stage."""
    for n in BATCHES.values():
        want = [22050] * len(n) if rate else None
        p = run_fmt(probes[0], n, 0, want=want, i16=i16, loudness=loudness, flac=flac)
        assert p.pop("fmt_src") == "none" and p.pop("fmt") == []
        assert p == run_probe(probes[1], n, want=want, i16=i16, loudness=loudness, flac=flac)


def test_empty_batch(probes):
    p = run_fmt(probes[0], [], 4)
    assert p["fmt"] == [] and p["fmt_src"] == "V64" and p["alloc"] == {"Fmt": [16, 1]}

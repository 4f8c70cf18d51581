"""The host half of every jb_*_pcm_batch entry (jbonsai_amd/csrc/jb_pcm_call.h) without a GPU: the check of the input
lists, the packing of the inputs one after the other, and the hand-out of each output's share of one host slab -- with
an allocator that fails on the k-th allocation, to see the rollback.  A small C++ probe (tests/plan/pcm_call_probe.cpp)
is compiled with g++ against the header alone."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"
OK, INVALID = 0, -1
# three outputs of a slab of 2-byte elements (the slab's bytes count 0, 1, 2, ...): the middle one is empty
ELEM = 2
SHARES = [(1, 2), (3, 0), (4, 3)]
WANT = [[2, 3, 4, 5], [], [8, 9, 10, 11, 12, 13]]


def build_probe(out_dir, *extra):
    exe = Path(out_dir) / "pcm_call_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", *extra, "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "pcm_call_probe.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("pcm_call_plan"))


def run(exe, *words):
    r = subprocess.run([str(exe)], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def check(exe, n, lists, null_in, n_in):
    return run(exe, "check", n, int(lists), null_in, *n_in)


def hand(exe, fail):
    return run(exe, "hand", len(SHARES), fail, ELEM, *[x for s in SHARES for x in s])


def test_input_check(probe):
    assert check(probe, 0, False, -1, [])["rc"] == OK  # no utterance: the lists may be NULL
    assert check(probe, 1, False, -1, [1])["rc"] == INVALID
    for lists in (False, True):
        assert check(probe, 0x80000000, lists, -1, [1] * 8)["rc"] == INVALID
    # a NULL in[1]: refused with a sample behind it, accepted without
    assert check(probe, 3, True, 1, [4, 1, 4]) == {"rc": INVALID, "cleared": 3}
    assert check(probe, 3, True, 1, [4, 0, 4]) == {"rc": OK, "cleared": 3}
    assert check(probe, 3, True, -1, [4, 1, 0]) == {"rc": OK, "cleared": 3}


def test_packing(probe):
    assert run(probe, "pack", 4, 0, 1, 1025, 0)["off"] == [0, 0, 1, 1026, 1026]
    assert run(probe, "pack", 0)["off"] == [0]


def test_hand_out(probe):
    r = hand(probe, 0)
    assert r["rc"] == OK and r["err"] == ""
    assert r["out"] == WANT  # (the empty output is a buffer, not null)
    assert r["n_out"] == [n for _, n in SHARES]
    assert r["allocs"] == 3 and r["frees"] == 0


@pytest.mark.parametrize("k", [1, 2, 3])
def test_hand_out_rolls_back_when_allocation_k_fails(probe, k):
    r = hand(probe, k)
    assert r["rc"] == INVALID and r["err"] == "out of host memory"
    assert r["out"] == [None] * 3 and r["n_out"] == [0] * 3
    assert r["allocs"] == k - 1 and r["frees"] == r["allocs"]

"""What a redo round of the output chain runs again (jbonsai_amd/csrc/jb_output.h: redo_scope, pick_renumbered) on the
host, without a GPU: the three masks the stages follow -- `measured` (the utterances the round rewrote), `post` (the
members of every touched loudness group) and `units` (the programmes of `post` behind a join) -- and the renumbering of
the items a mask picks.  A small C++ probe (tests/plan/redo_probe.cpp) is compiled with g++ against jb_output.cpp.
The request is the one of tests/test_gpu_join.py's redo test: four utterances, the loudness group {1, 2}, the
programmes {0, 2} and {1, 3}."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"
NONE = 4294967295
GROUPS = [NONE, 0, 0, NONE]  # dense: utterance 0 -> group 0, {1, 2} -> group 1, utterance 3 -> group 2
PROG_OF = [0, 1, 0, 1]


def build_probe(out_dir, *extra):
    exe = Path(out_dir) / "redo_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", *extra, "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "redo_probe.cpp"), str(CSRC / "jb_output.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("redo_plan"))


def run(exe, *nums):
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def scope(exe, only, groups=(), prog_of=(), P=0):
    return run(exe, "scope", len(only), len(groups), *groups, len(prog_of), *prog_of, P, *only)


def pick(exe, mask, count):
    return run(exe, "pick", len(count), *mask, *count)


def test_scope_of_the_join_redo_request(probe):
    """Utterance 2 rewritten: its group reaches utterance 1, and the two of them both programmes."""
    s = scope(probe, [0, 0, 1, 0], GROUPS, PROG_OF, 2)
    assert s["group_of"] == [0, 1, 1, 2]
    assert s["measured"] == [0, 0, 1, 0] and s["post"] == [0, 1, 1, 0]
    assert s["touched_groups"] == [0, 1, 0]  # the group {1, 2} alone
    assert s["units"] == [1, 1]


def test_scope_without_groups_and_without_a_join(probe):
    only = [0, 0, 1, 0]
    s = scope(probe, only, prog_of=PROG_OF, P=2)
    assert s["measured"] == s["post"] == only and s["units"] == [1, 0]
    s = scope(probe, only, groups=GROUPS)
    assert s["measured"] == only and s["units"] == s["post"] and len(s["units"]) == 4
    s = scope(probe, only)
    assert s["measured"] == s["post"] == s["units"] == only and s["touched_groups"] == []


@pytest.mark.parametrize("groups,prog_of,P", [((), (), 0), (GROUPS, (), 0), ((), PROG_OF, 2), (GROUPS, PROG_OF, 2)])
def test_scope_of_nothing_and_of_everything(probe, groups, prog_of, P):
    G, U = (3 if groups else 0), (P if prog_of else 4)
    s = scope(probe, [0, 0, 0, 0], groups, prog_of, P)
    assert s["measured"] == s["post"] == [0] * 4 and s["units"] == [0] * U and s["touched_groups"] == [0] * G
    s = scope(probe, [1, 1, 1, 1], groups, prog_of, P)
    assert s["measured"] == s["post"] == [1] * 4 and s["units"] == [1] * U and s["touched_groups"] == [1] * G


def test_pick_renumbered(probe):
    count = [3, 0, 5, 1]
    # the item of count 0 is kept: it takes the base of the item behind it
    assert pick(probe, [1, 1, 0, 1], count) == {"index": [0, 1, 3], "base": [0, 3, 3], "total": 4}
    assert pick(probe, [0, 0, 0, 0], count) == {"index": [], "base": [], "total": 0}
    assert pick(probe, [], []) == {"index": [], "base": [], "total": 0}
    assert pick(probe, [1, 1, 1, 1], count) == {"index": [0, 1, 2, 3], "base": [0, 3, 3, 8], "total": 9}

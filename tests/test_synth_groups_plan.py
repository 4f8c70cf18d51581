"""The group split of an engine request (plan_synth_groups, jbonsai_amd/csrc/jb_plan.h) on the host, without a GPU: the
boundaries of the groups that jb_synthesize_batch pipelines a request in.  The `groups` word of the C++ probe
(tests/plan/create_probe.cpp), compiled with g++ against jb_plan.cpp, reads a list of cases on stdin and prints each
case's boundaries as JSON; the test holds them to the rule restated below."""
import itertools
import json
import random
import subprocess
from pathlib import Path

import pytest

from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"
MIN_UTTS, MIN_LABELS = 8, 16000  # two groups from here on (measured choices: DESIGN.md)
COUNTS = (0, 1, 7, 2000, 4000)   # label lines of an utterance in the sweep


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("synth_groups") / "create_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "create_probe.cpp"), str(CSRC / "jb_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def groups_input(cases):
    """cases: (labels per utterance, forced, one_batch) -> the probe's request"""
    words = ["groups", len(cases)]
    for labels, forced, one_batch in cases:
        words += [len(labels), forced, int(one_batch), *labels]
    return " ".join(str(w) for w in words) + "\n"


def groups(exe, cases):
    r = subprocess.run([str(exe)], input=groups_input(cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert len(got) == len(cases)
    return got


def wanted_groups(labels, forced, one_batch):
    """How many groups the request asks for, before there can be no more groups than utterances."""
    if one_batch:
        return 1
    if forced:
        return forced
    return 2 if len(labels) >= MIN_UTTS and sum(labels) >= MIN_LABELS else 1


def groups_rule(labels, forced, one_batch):
    """The rule as jb_plan.h words it: boundary g is the first utterance whose line_off reaches g / ngroups of the
    request's lines (all utterances where none does)."""
    n, total = len(labels), sum(labels)
    ngroups = min(max(1, wanted_groups(labels, forced, one_batch)), max(1, n))
    off = [0] + list(itertools.accumulate(labels))
    glo = [0]
    for g in range(1, ngroups):
        glo.append(next((u for u in range(n) if off[u] >= total * g // ngroups), n))
    return glo + [n]


# the suite's nine-utterance list (test_synthesize_batch_in_groups_equals_one_batch): empty utterances included
S1, S2 = len(SAMPLE_SENTENCE_1), len(SAMPLE_SENTENCE_2)
NINE = [S1, 6 * S2, 0, S2, 6 * S2, S1, 0, 6 * S2, S2]


def test_groups_pinned(probe):
    assert (S1, S2) == (8, 20) and sum(NINE) == 416  # line_off: 0 8 128 128 148 268 276 276 396 416
    cases = [(NINE, 1, False), (NINE, 2, False), (NINE, 3, False), (NINE, 9, False), (NINE, 0, False),
             (NINE, 3, True),
             ([], 0, False), ([], 5, False), ([5], 4, False),
             ([2000] * 8, 0, False), ([2000] * 7 + [1999], 0, False), ([4000] * 7, 0, False),
             ([2000] * 8, 0, True), ([2000] * 8, 1, False),
             ([0, 0, 4000, 0], 2, False), ([0, 0, 0], 3, False)]
    want = [[0, 9],
            [0, 5, 9],                         # 208 lines are reached at utterance 5 (268)
            [0, 4, 8, 9],                      # 138 at utterance 4 (148), 277 at utterance 8 (396)
            [0, 2, 2, 4, 5, 5, 8, 8, 8, 9],    # 46 92 138 184 231 277 323 369: empty groups where a long one spans
            [0, 9],
            [0, 9],
            [0, 0], [0, 0], [0, 1],
            [0, 4, 8], [0, 8], [0, 7],
            [0, 8], [0, 8],
            [0, 3, 4], [0, 0, 0, 3]]
    got = groups(probe, cases)
    for c, g, w in zip(cases, got, want):
        assert g == w == groups_rule(*c), c


def sweep_cases():
    """n_utts 0..12 with label counts drawn from COUNTS: every sequence up to four utterances, and from five on the
    constant sequences, the sequences at the label threshold and 40 drawn ones (a fixed seed); each under forced 0..13
    and both values of one_batch."""
    rng = random.Random(20261019)
    seqs = [list(s) for n in range(0, 5) for s in itertools.product(COUNTS, repeat=n)]
    for n in range(5, 13):
        seqs += [[c] * n for c in COUNTS]
        seqs += [[2000] * (n - 1) + [c] for c in COUNTS] + [[c] + [2000] * (n - 1) for c in COUNTS]
        seqs += [[rng.choice(COUNTS) for _ in range(n)] for _ in range(40)]
    return [(s, forced, one_batch) for s in seqs for forced in range(0, 14) for one_batch in (False, True)]


def test_groups_sweep(probe):
    cases = sweep_cases()
    got = groups(probe, cases)
    two_unforced = set()
    for (labels, forced, one_batch), glo in zip(cases, got):
        n, total, case = len(labels), sum(labels), (labels, forced, one_batch)
        ngroups = len(glo) - 1
        assert ngroups == min(max(1, wanted_groups(labels, forced, one_batch)), max(1, n)), case
        assert glo[0] == 0 and glo[-1] == n and all(a <= b for a, b in zip(glo, glo[1:])), case
        off = [0] + list(itertools.accumulate(labels))
        for g in range(1, ngroups):
            want = total * g // ngroups
            assert all(off[u] < want for u in range(glo[g])) and (glo[g] == n or off[glo[g]] >= want), case
        assert glo == groups_rule(labels, forced, one_batch), case
        if one_batch:
            assert ngroups == 1, case
        elif not forced:
            assert ngroups == (2 if n >= MIN_UTTS and total >= MIN_LABELS else 1), case
            if ngroups == 2:
                two_unforced.add((n, total))
    # the threshold itself is in the sweep, from both sides
    assert (8, 16000) in two_unforced and min(t for _, t in two_unforced) == 16000
    assert min(n for n, _ in two_unforced) == 8
    assert any(len(s) == 7 and sum(s) >= 16000 for s, f, o in cases if not f and not o)
    assert any(len(s) >= 8 and 14000 < sum(s) < 16000 for s, f, o in cases if not f and not o)

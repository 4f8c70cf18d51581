"""The loudness group bookkeeping (jbonsai_amd/csrc/jb_output.h: plan_loudness_groups, loudness_groups_closure) on the
host, without a GPU: dense numbering by first member, member lists in utterance order, every refusal of a mixed group
and the redo closure.  A probe of its own (tests/plan/loudness_groups_probe.cpp), built the way
tests/test_adpcm_plan.py builds its probe."""
import json
import subprocess

import pytest

from tests.test_adpcm_plan import build

NO = 0xFFFFFFFF


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("loudness_groups_plan"), "loudness_groups_probe")


def run(exe, group, target=None, ceiling=None, mode=None, hz=None, touched=None):
    B = len(group)
    has_target = target is not None
    nums = [B, *group, int(has_target), *(target or [0.0] * B), *(ceiling or [0.0] * B), *(mode or [0] * B),
            *(hz or [48000] * B), *(touched or [0] * B)]
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_dense_renumbering_by_first_member(probe):
    """Caller's ids 5, 2, 5, none, 0, 2, none: the groups are numbered as their first members appear, an utterance of
    its own among them."""
    p = run(probe, [5, 2, 5, NO, 0, 2, NO])
    assert p["ok"]
    assert p["group_of"] == [0, 1, 0, 2, 3, 1, 4]
    assert p["first"] == [0, 2, 4, 5, 6, 7]


def test_member_lists_ascend(probe):
    p = run(probe, [3, 1, 3, 1, 3, 0, 1])
    assert p["group_of"] == [0, 1, 0, 1, 0, 2, 1]
    members = [p["members"][p["first"][g]:p["first"][g + 1]] for g in range(3)]
    assert members == [[0, 2, 4], [1, 3, 6], [5]]


def test_all_ungrouped_is_one_group_each(probe):
    p = run(probe, [NO] * 4)
    assert p["group_of"] == [0, 1, 2, 3] and p["members"] == [0, 1, 2, 3] and p["first"] == [0, 1, 2, 3, 4]


def test_empty_batch(probe):
    p = run(probe, [])
    assert p["ok"] and p["group_of"] == [] and p["first"] == [0] and p["members"] == []


def test_id_out_of_range_is_refused(probe):
    p = run(probe, [0, 3, 1])
    assert p == {"ok": False, "bad_group": 3, "bad_field": "group id"}


@pytest.mark.parametrize("field,kw", [
    ("target", dict(target=[-16.0, -23.0, -16.0, -16.1], ceiling=[0.0] * 4)),
    ("target", dict(target=[-16.0, -23.0, -16.0, "nan"], ceiling=[0.0] * 4)),
    ("ceiling", dict(target=[-16.0] * 4, ceiling=[-1.0, -1.0, -1.0, "inf"])),
    ("peak mode", dict(mode=[0, 1, 0, 1])),
    ("output rate", dict(hz=[48000, 16000, 48000, 16000])),
])
def test_mixed_group_is_refused(probe, field, kw):
    """Group 3 = utterances 0, 2, 3; group 1 = utterance 1.  A difference inside group 3 is refused with the
    caller's id and the field; the same values across groups are fine."""
    p = run(probe, [3, 1, 3, 3], **kw)
    assert p == {"ok": False, "bad_group": 3, "bad_field": field}
    # the odd one in a group of its own: accepted
    q = run(probe, [3, 1, 3, NO], **kw) if field in ("target", "ceiling") else run(probe, [3, 1, 3, 1], **kw)
    assert q["ok"]


def test_two_nan_targets_agree(probe):
    p = run(probe, [0, 0, 1], target=["nan", "nan", -20.0], ceiling=[-1.0, -1.0, -1.0])
    assert p["ok"] and p["group_of"] == [0, 0, 1]


def test_without_a_target_only_mode_and_rate_are_compared(probe):
    assert run(probe, [0, 0])["ok"]
    assert run(probe, [0, 0], mode=[0, 1]) == {"ok": False, "bad_group": 0, "bad_field": "peak mode"}


def test_closure(probe):
    """Groups {0, 3, 5}, {1, 4}, utterances 2 and 6 on their own.  A touched member pulls in its whole group; an
    untouched group stays out; an ungrouped utterance stands for itself, as without groups."""
    group = [2, 0, NO, 2, 0, 2, NO]
    p = run(probe, group, touched=[0, 0, 0, 1, 0, 0, 0])
    assert p["group_of"] == [0, 1, 2, 0, 1, 0, 3]
    assert p["closure_groups"] == [1, 0, 0, 0] and p["closure_members"] == [1, 0, 0, 1, 0, 1, 0]
    p = run(probe, group, touched=[0, 0, 1, 0, 0, 0, 0])
    assert p["closure_groups"] == [0, 0, 1, 0] and p["closure_members"] == [0, 0, 1, 0, 0, 0, 0]
    p = run(probe, group, touched=[0, 1, 0, 0, 0, 0, 1])
    assert p["closure_groups"] == [0, 1, 0, 1] and p["closure_members"] == [0, 1, 0, 0, 1, 0, 1]
    p = run(probe, group, touched=[0] * 7)
    assert p["closure_groups"] == [0] * 4 and p["closure_members"] == [0] * 7
    p = run(probe, group, touched=[1] * 7)
    assert p["closure_groups"] == [1] * 4 and p["closure_members"] == [1] * 7

"""The stems request in the output plan (jbonsai_amd/csrc/jb_output.h: mix_layout with stem_of, plan_output, redo_scope)
on the host, without a GPU: the numbering, the extents, each stem's segments against a brute-force membership per
sample, the old layout field for field where no stems are asked for, the refusals, the activity layout that keeps the P
programmes as its units, and the redo closure in which a touched member touches its programme's stems.  A small C++
probe (tests/plan/stems_probe.cpp) is compiled with g++ against jb_output.cpp."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"
NINF = float("-inf")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("stems_plan")
    exes = []
    for name in ("stems_probe", "mix_probe"):
        exe = d / name
        cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC),
               str(ROOT / "tests" / "plan" / (name + ".cpp")), str(CSRC / "jb_output.cpp"), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        exes.append(exe)
    return exes


def words(req):
    out = []
    for r in req:
        r = tuple(r) + (0,) * (6 - len(r))
        out += [-1 if r[0] is None else r[0], r[1], "ninf" if r[2] == NINF else r[2], r[3], r[4], r[5]]
    return out


def ids(stem_of, B):
    if stem_of is None:
        return [0] + [-1] * B
    return [1] + [-1 if s is None else s for s in stem_of]


def run(exe, *nums):
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def layout(exe, req, stem_of, n, elem=8):
    return run(exe, "layout", elem, len(req), *words(req), *ids(stem_of, len(req)), *n)


def plan(exe, req, stem_of, n, i16=0, fmt_bytes=0, act=0, only=None):
    only = only if only is not None else [0] * len(n)
    return run(exe, "plan", i16, fmt_bytes, act, len(n), *n, *words(req), *ids(stem_of, len(n)), *only)


def brute(L, req, stem_of, n, elem=8):
    """What the layout must say, sample by sample: numbering, extents, and for every sample of every stem the unmuted
    members of at least one sample that cover it, in ascending utterance index"""
    B = len(req)
    req = [tuple(r) + (0,) * (6 - len(r)) for r in req]
    P = L["P"]
    per = 16 // elem
    stems = []  # (programme, id, members)
    for p in range(P):
        seen = {}
        for u in range(B):
            if L["prog_of"][u] != p or stem_of[u] is None:
                continue
            if stem_of[u] not in seen:
                seen[stem_of[u]] = len(stems)
                stems.append((p, stem_of[u], []))
            stems[seen[stem_of[u]]][2].append(u)
    assert len(L["units"]) == P + len(stems) and len(L["stems"]) == len(stems)
    assert len(L["seg_first"]) == P + len(stems) + 1 and len(L["depth"]) == len(L["overlap"]) == P + len(stems)
    off = (L["units"][P - 1][2] + L["units"][P - 1][1] + per - 1) // per * per if P else 0
    for s, (p, sid, mem) in enumerate(stems):
        unit = P + s
        live = [u for u in mem if req[u][2] != NINF and n[u]]
        first = min([req[u][1] for u in live], default=0)
        end = max([req[u][1] + n[u] for u in live], default=0)
        assert L["stems"][s] == [p, sid, len(mem), first, end], s
        N = L["units"][p][1]
        assert L["units"][unit] == [L["units"][p][0], N, off], s  # the programme's length, the next 16-byte boundary
        assert off % per == 0
        off = (off + N + per - 1) // per * per
        for u in mem:
            assert L["stem_unit"][u] == unit
        segs = L["segs"][L["seg_first"][unit]:L["seg_first"][unit + 1]]
        k, depth, overlap = 0, 0, 0
        for k0, k1, l0, nl in segs:  # from 0 to the length without a hole, never empty
            assert k0 == k and k1 > k0
            listed = L["lists"][l0:l0 + nl]
            for j in sorted({k0, k1 - 1, (k0 + k1) // 2}):
                assert listed == [u for u in live if req[u][1] <= j < req[u][1] + n[u]], (s, j)
            depth = max(depth, nl)
            overlap += (k1 - k0) * (nl >= 2)
            k = k1
        assert k == N and (N or not segs)
        # a cut stands exactly where the cover changes
        for (a0, a1, al0, anl), (b0, b1, bl0, bnl) in zip(segs, segs[1:]):
            assert L["lists"][al0:al0 + anl] != L["lists"][bl0:bl0 + bnl]
        assert L["depth"][unit] == depth and L["overlap"][unit] == overlap
    for u in range(B):
        if stem_of[u] is None:
            assert L["stem_unit"][u] == -1
    assert L["total"] == off
    return stems


REQ = [(0, 10, 0.0), (0, 0, -6.0), (0, 5, 0.0, 4), (0, 0, NINF, 100), (None, 2, 3.0), (0, 12, 2.0), (0, 3, 0.0)]
LEN = [10, 8, 10, 30, 3, 0, 9]

CASES = {
    "every member a stem of its own": list(range(7)),
    "one stem of all members": [5] * 7,
    "talkers": [1, 0, 1, 0, None, 0, 1],
    "a member of no stem": [1, None, 1, 0, None, None, 0],
    "a stem of muted and empty members only": [0, 0, 0, 3, None, 3, 0],
    "an utterance of its own with an id": [None, None, None, None, 6, None, None],
    "no member carries an id": [None] * 7,
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("elem", [8, 2])
def test_numbering_extents_and_segments(probe, name, elem):
    stem_of = CASES[name]
    L = layout(probe[0], REQ, stem_of, LEN, elem)
    assert L["ok"] and L["P"] == 2
    stems = brute(L, REQ, stem_of, LEN, elem)
    if name == "talkers":
        # by programme, within one by the first member: id 1 (utterance 0) in front of id 0 (utterance 1)
        assert [(p, i) for p, i, _ in stems] == [(0, 1), (0, 0)] and L["stem_unit"] == [2, 3, 2, 3, -1, 3, 2]
        assert L["stems"][1][2] == 3  # the muted member and the empty one are counted
    if name == "a stem of muted and empty members only":
        assert L["stems"][1] == [0, 3, 2, 0, 0]  # it exists, without an extent: silence of the programme's length
        assert L["segs"][L["seg_first"][3]:L["seg_first"][4]] == [[0, 130, L["segs"][L["seg_first"][3]][2], 0]]
    if name == "an utterance of its own with an id":
        assert L["stems"] == [[1, 6, 1, 2, 5]] and L["units"][2][1] == 5
    if name == "no member carries an id":
        assert L["stems"] == [] and L["stem_unit"] == [-1] * 7


def test_without_a_request_the_layout_is_the_old_one_field_for_field(probe):
    new = layout(probe[0], REQ, None, LEN)
    assert new["stems"] == [] and new["stem_unit"] == []
    old = run(probe[1], "layout", 8, len(REQ), *words(REQ), *LEN, 0)
    for key in ("ok", "prog_of", "start", "units", "total", "seg_first", "segs", "lists", "depth", "overlap"):
        assert new[key] == old[key], key
    # ... and with one the programmes' part stands as it stood: the stems lie behind
    L = layout(probe[0], REQ, CASES["talkers"], LEN)
    ns = old["seg_first"][-1]
    assert L["units"][:2] == old["units"] and L["segs"][:ns] == old["segs"] and L["seg_first"][:3] == old["seg_first"]
    assert L["lists"][:len(old["lists"])] == old["lists"] and L["depth"][:2] == old["depth"]


def test_a_programme_of_one_member_and_empty_batches(probe):
    L = layout(probe[0], [(None, 3, 0.0, 2)], [0], [7])
    assert L["units"] == [[0, 12, 0], [0, 12, 12]] and L["stems"] == [[0, 0, 1, 3, 10]]
    assert [s[:2] + s[3:] for s in L["segs"]] == [[0, 3, 0], [3, 10, 1], [10, 12, 0]] * 2
    L = layout(probe[0], [(None, 3, 0.0, 2)], [0], [7], elem=2)
    assert L["units"] == [[0, 12, 0], [0, 12, 16]] and L["total"] == 32
    L = layout(probe[0], [], [], [])
    assert L["ok"] and L["units"] == [] and L["stems"] == []
    L = layout(probe[0], [(0, 0, 0.0)] * 2, [0, 1], [0, 0])  # a programme of no samples: stems of none, no segment
    assert L["units"] == [[0, 0, 0]] * 3 and L["segs"] == [] and L["stems"] == [[0, 0, 1, 0, 0], [0, 1, 1, 0, 0]]


def test_refusals(probe):
    L = layout(probe[0], REQ, [0, 0, 7, 0, None, 0, 0], LEN)  # an id of the batch size
    assert not L["ok"] and L["field"] == "stem id" and L["bad"] == 2
    assert layout(probe[0], REQ, [0, 0, 6, 0, None, 0, 0], LEN)["ok"]
    # the slab: a programme that fits alone, and no longer with a stem behind it
    big = 2 ** 61
    req = [(0, 0, 0.0, big), (0, 0, 0.0), (0, 0, 0.0)]
    assert layout(probe[0], req, None, [4, 4, 4])["ok"]
    assert layout(probe[0], req, [0, 1, None], [4, 4, 4])["ok"]  # three units of 2^61 samples and a little
    L = layout(probe[0], req, [0, 1, 2], [4, 4, 4])
    assert not L["ok"] and L["field"] == "slab length" and L["bad"] == 3  # the fourth unit passes 2^63 samples
    # the lists' limit counts the stems' lists too: 4000 members over each other are 8,002,000 entries, with one stem
    # of all of them as many again, above 2^24
    n = 4000
    req = [(0, u, 0.0) for u in range(n)]
    assert layout(probe[0], req, None, [n] * n)["ok"]
    L = layout(probe[0], req, [0] * n, [n] * n)
    assert not L["ok"] and L["field"] == "work lists" and L["bad"] == 1


@pytest.mark.parametrize("i16", [0, 1])
def test_the_plan_lists_the_stems_as_units_behind_the_programmes(probe, i16):
    n = [1680, 240, 9600, 720, 100]
    req = [(0, 100, 0.0, 3, 5, 5), (1, 0, -6.0), (0, 0, 2.0, 0, 9, 9), (1, 50, 0.0, 7), (None, 0, 0.0)]
    stem_of = [0, 0, 1, None, None]
    kw = dict(i16=i16, fmt_bytes=0 if i16 else 3)
    none, st = plan(probe[0], req, None, n, **kw), plan(probe[0], req, stem_of, n, **kw)
    assert none["n_progs"] == st["n_progs"] == 3 and none["stems"] == [] and none["unit_parent"] == []
    assert len(none["units"]) == 3 and st["units"][:3] == none["units"]
    assert st["stems"] == [[0, 0, 1, 100, 1780], [0, 1, 1, 0, 9600], [1, 0, 1, 0, 240]]
    assert st["unit_parent"] == [0, 0, 1] and st["stem_unit"] == [3, 5, 4, -1, -1]
    per = 8 if i16 else 2
    off = none["join_alloc"]
    for s, p in enumerate(st["unit_parent"]):
        assert st["units"][3 + s] == [48000, st["units"][p][1], off]
        off = (off + st["units"][p][1] + per - 1) // per * per
    assert st["join_alloc"] == off
    assert st["mix_depth"] == [2, 2, 1, 1, 1, 1] and st["prog_first"] == none["prog_first"]
    # the encoders' places follow the units
    assert i16 or [f[1] for f in st["fmt"]] == [u[1] * 3 for u in st["units"]]
    assert i16 or st["fmt"][:3] == none["fmt"]


def test_the_activity_layout_keeps_the_programmes_as_its_units(probe):
    n = [1680, 2400, 9600, 720, 1000]
    req = [(0, 100, 0.0), (1, 0, -6.0), (0, 0, 2.0), (1, 50, 0.0, 7), (None, 0, 0.0)]
    none, st = plan(probe[0], req, None, n, act=1), plan(probe[0], req, [0, 0, 1, 1, 0], n, act=1)
    assert none["act_fault"] == st["act_fault"] == ""
    assert len(st["units"]) == 8 and st["act_units"] == none["act_units"] == 3 and st["act_cols"] == none["act_cols"] == 5


def test_a_touched_member_touches_its_programmes_stems(probe):
    n = [1680, 240, 9600, 720, 100]
    req = [(0, 100, 0.0), (1, 0, -6.0), (0, 0, 2.0), (1, 50, 0.0, 7), (None, 0, 0.0)]
    stem_of = [0, 0, 1, None, 4]  # units: programmes 0 1 2, stems (0, 0) (0, 1) (1, 0) (2, 4)
    r = plan(probe[0], req, stem_of, n, only=[0, 0, 0, 1, 0])  # a member of no stem: its programme and that one's stem
    assert r["redo_post"] == [0, 0, 0, 1, 0] and r["redo_units"] == [0, 1, 0, 0, 0, 1, 0]
    r = plan(probe[0], req, stem_of, n, only=[1, 0, 0, 0, 0])  # one talker: both stems of the programme, whole
    assert r["redo_units"] == [1, 0, 0, 1, 1, 0, 0]
    r = plan(probe[0], req, stem_of, n, only=[0, 0, 0, 0, 1])
    assert r["redo_units"] == [0, 0, 1, 0, 0, 0, 1]
    r = plan(probe[0], req, None, n, only=[0, 0, 0, 0, 1])
    assert r["redo_units"] == [0, 0, 1]
    assert plan(probe[0], req, stem_of, n)["redo_units"] == [0] * 7

"""The mix request in the output plan (jbonsai_amd/csrc/jb_output.h: mix_layout, plan_output) on the host, without a
GPU: the geometry (length as the largest reach, members out of start order, empty and muted members, a programme of
pads alone), the segments and their member lists (the work the kernel is given), the depth and overlap counts, the
refusals, and the routing -- a mix request goes exactly where a join request goes, and never beside one.  A small C++
probe (tests/plan/mix_probe.cpp) is compiled with g++ against jb_output.cpp."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mix_plan") / "mix_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "mix_probe.cpp"), str(CSRC / "jb_output.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def words(req):
    out = []
    for r in req:
        r = tuple(r) + (0,) * (6 - len(r))
        out += [-1 if r[0] is None else r[0], r[1], "ninf" if r[2] == float("-inf") else r[2], r[3], r[4], r[5]]
    return out


def run(exe, *nums):
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def layout(exe, req, n, elem=8, hz=()):
    return run(exe, "layout", elem, len(req), *words(req), *n, len(hz), *hz)


def plan(exe, kind, req, n, i16=0, loudness=0, flac=0, fmt_bytes=0, adpcm=0, want=()):
    off = [sum(n[:u]) for u in range(len(n))]
    return run(exe, "plan", kind, 48000, i16, loudness, flac, fmt_bytes, adpcm, len(n), *n, *off, len(want), *want,
               *words(req))


NINF = float("-inf")
# (programme, start, gain_db, pad_after, fade_in, fade_out)
REQ = [(0, 10, 0.0), (0, 0, -6.0), (0, 5, 0.0, 4), (0, 0, NINF, 100), (None, 2, 3.0)]
LEN = [10, 8, 10, 30, 3]


def test_geometry_segments_and_counts(probe):
    L = layout(probe, REQ, LEN)
    assert L["ok"] and L["prog_of"] == [0, 0, 0, 0, 1] and L["start"] == [10, 0, 5, 0, 2]
    # length: the largest start + n + pad_after (here the muted member's); programme 1 on the next 16-byte boundary
    assert L["units"] == [[0, 130, 0], [0, 5, 130]] and L["total"] == 136
    assert L["gain"][0] == 1.0 and L["gain"][3] == 0.0 and abs(L["gain"][1] - 10 ** (-6 / 20)) < 1e-15
    # cut at every start and end of an unmuted member: the cover is constant between two cuts, listed in ascending
    # utterance index whatever the starts; the muted member is in no list
    assert L["seg_first"] == [0, 6, 8]
    segs = [(k0, k1, L["lists"][l0:l0 + nl]) for k0, k1, l0, nl in L["segs"]]
    assert segs == [(0, 5, [1]), (5, 8, [1, 2]), (8, 10, [2]), (10, 15, [0, 2]), (15, 20, [0]), (20, 130, []),
                    (0, 2, []), (2, 5, [4])]
    assert L["depth"] == [2, 1] and L["overlap"] == [8, 0]
    # 16-bit samples: eight to the boundary
    assert layout(probe, REQ, LEN, elem=2)["units"] == [[0, 130, 0], [0, 5, 136]]


def test_empty_members_and_pads_alone(probe):
    L = layout(probe, [(0, 2, 0.0, 3)] * 3, [0, 0, 0])
    assert L["units"] == [[0, 5, 0]] and L["segs"] == [[0, 5, 0, 0]] and L["depth"] == [0] and L["overlap"] == [0]
    L = layout(probe, [(0, 0, 0.0), (0, 3, 0.0), (0, 4, 0.0)], [8, 0, 2])  # an empty member inside another: no cut
    assert [s[:2] for s in L["segs"]] == [[0, 4], [4, 6], [6, 8]] and L["depth"] == [2]
    L = layout(probe, [(None, 7, NINF, 1)], [4])  # a muted programme: silence of its length
    assert L["units"] == [[0, 12, 0]] and L["segs"] == [[0, 12, 0, 0]]
    assert layout(probe, [], [])["units"] == []
    # identical starts and ends: one segment
    L = layout(probe, [(2, 5, 0.0)] * 3, [9, 9, 9])
    assert [s[:2] + s[3:] for s in L["segs"]] == [[0, 5, 0], [5, 14, 3]] and L["overlap"] == [9]


def test_refusals(probe):
    L = layout(probe, [(5, 0, 0.0)] + REQ[1:], LEN)
    assert not L["ok"] and L["field"] == "programme id" and L["bad"] == 5
    L = layout(probe, REQ, LEN, hz=[48000, 48000, 44100, 48000, 8000])
    assert not L["ok"] and L["field"] == "output rate" and L["bad"] == 0
    assert layout(probe, REQ, LEN, hz=[48000] * 4 + [8000])["units"] == [[48000, 130, 0], [8000, 5, 130]]
    L = layout(probe, [(0, 2 ** 63 - 4, 0.0)], [10])
    assert not L["ok"] and L["field"] == "length" and L["bad"] == 0
    n = 6000  # 6000 members, each over all the starts behind it: 6000 * 6001 / 2 list entries, above 2^24
    L = layout(probe, [(0, u, 0.0) for u in range(n)], [n] * n)
    assert not L["ok"] and L["field"] == "work lists"


@pytest.mark.parametrize("i16", [0, 1])
def test_a_mix_request_is_routed_where_the_join_goes(probe, i16):
    n = [1680, 240, 9600, 720]
    req = [(0, 100, 0.0, 3, 5, 5), (1, 0, -6.0), (0, 0, 2.0, 0, 9, 9), (1, 50, 0.0, 7)]
    kw = dict(i16=i16, flac=i16, fmt_bytes=0 if i16 else 3, adpcm=1)
    none, mix, join = plan(probe, "mix", [], []), plan(probe, "mix", req, n, **kw), plan(probe, "join", req, n, **kw)
    assert none["join"] == "none" and not none["mixed"] and none["units"] == []
    slab = "Join16" if i16 else "Join64"
    assert mix["mixed"] and not join["mixed"]
    for key in ("final", "join_src", "join", "join_i16", "flac", "fmt_src", "adpcm_src", "prog_of", "prog_first",
                "prog_members"):
        assert mix[key] == join[key], key
    assert mix["join"] == slab and mix["join_src"] == mix["final"] and mix["adpcm_src"] == slab
    assert mix["flac"] == (slab if i16 else "none") and mix["fmt_src"] == ("none" if i16 else slab)
    # the programmes' geometry is the mix's own: starts as given, lengths the largest reach
    assert mix["prog_start"] == [100, 0, 0, 50] and [u[1] for u in mix["units"]] == [9600, 50 + 720 + 7]
    assert mix["mix_depth"] == [2, 2] and mix["mix_overlap"] == [1680, 190]
    per = 8 if i16 else 2
    assert mix["units"][1][2] == 9600 and mix["join_alloc"] == (9600 + 777 + per - 1) // per * per
    # the encoders' places follow the programmes
    assert [a[1] for a in mix["adpcm"]] and len(mix["adpcm"]) == 2 and (i16 or len(mix["fmt"]) == 2)
    assert i16 or [f[1] for f in mix["fmt"]] == [9600 * 3, 777 * 3]
    # never both: a join request beside it wins the plan (the chain refuses the second setter before it comes to that)
    both = plan(probe, "both", req, n, **kw)
    assert not both["mixed"] and both["units"] == join["units"]
    # behind the converter the lengths are the converted ones
    conv = plan(probe, "mix", req, n, want=[44100] * 4, **kw)
    assert conv["mixed"] and conv["units"][0][0] == 44100 and conv["units"][0][1] == (9600 * 147 + 159) // 160

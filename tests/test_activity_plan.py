"""The speech-activity request in the output plan (jbonsai_amd/csrc/jb_output.h: plan_output with OutPlanIn::activity,
jb_activity.h: act_layout) on the host, without a GPU: the units with their T, C and offsets on 16-byte boundaries, the
compact energy layout, the word scratch, what the stage reads, nothing planned without the request, the refusals, and
the mask of redo_scope the stage follows; and the packed smoothing steps the kernel runs, word by word on the host,
against the naive statement (tests/activity_ref.py).  A small C++ probe (tests/plan/activity_probe.cpp) is compiled
with g++ against jb_output.cpp."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import activity_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"
NINF = float("-inf")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("activity_plan") / "activity_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "activity_probe.cpp"), str(CSRC / "jb_output.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, *nums):
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def words(req):
    out = []
    for r in req:
        r = tuple(r) + (0,) * (6 - len(r))
        out += [-1 if r[0] is None else r[0], r[1], "ninf" if r[2] == NINF else r[2], r[3], r[4], r[5]]
    return out


def plan(exe, kind, n, req=None, i16=0, want=(), act=1, win=400, hop=160, gate_db=40.0, grid=0, columns=0, flags=1,
         min_gap=0, only=None, hz=48000):
    req = req if req is not None else [(None, 0, 0.0)] * len(n)
    only = only if only is not None else [0] * len(n)
    return run(exe, "plan", kind, hz, i16, len(n), *n, len(want), *want, act, win, hop, gate_db, grid, columns, flags,
               min_gap, *only, *words(req))


# (programme, start, gain_db, pad_after): programme 0 = {0, 1, 3}, utterance 1 muted, utterance 3 of no samples
REQ = [(0, 37, 0.0), (0, 4001, NINF), (None, 5, 0.0, 11), (0, 555, -6.0, 7)]
LEN = [9000, 7000, 5000, 0]


def frames_touching(grid, T, wl, hop, start, n):
    s0 = R.frames(grid, max(T, 1) * hop + wl, wl, hop)[1]
    t = [k for k in range(T) if n and s0 + k * hop < start + n and s0 + k * hop + wl > start]
    assert t == list(range(t[0], t[-1] + 1)) if t else True
    return (t[0], len(t)) if t else (0, 0)


@pytest.mark.parametrize("grid", list(R.GRIDS.values()))
def test_units_columns_and_the_compact_energy_layout(probe, grid):
    wl, hop = 400, 160
    p = plan(probe, "mix", LEN, REQ, grid=grid, min_gap=2)
    assert p["act_src"] == p["final"] == "V64" and p["join"] == "Join64" and not p["act_i16"] and p["fault"] == ""
    n0 = max(37 + 9000, 4001 + 7000, 555 + 7)
    n1 = 5 + 5000 + 11
    T0, T1 = R.frames(grid, n0, wl, hop)[0], R.frames(grid, n1, wl, hop)[0]
    # the units: offsets on 16-byte boundaries, T by the grid, C the members in ascending utterance index
    assert p["units"] == [[0, T0, 3, wl, hop, 0], [(T0 * 3 + 15) // 16 * 16, T1, 1, wl, hop, 3]]
    assert p["bytes"] == p["units"][1][0] + (T1 + 15) // 16 * 16
    cols = p["cols"]
    assert [c[:2] for c in cols] == [[0, 0], [0, 1], [0, 3], [1, 2]]
    # each column's source: the member at its start; a muted member and one of no samples: a column of zeros
    assert [c[2:4] for c in cols] == [[37, 9000], [4001, 0], [555, 0], [5, 5000]]
    # the compact energies: per column only the frames that touch its source, laid one after the other
    e0 = 0
    for c, T in zip(cols, (T0, T0, T0, T1)):
        assert c[4:6] == list(frames_touching(grid, T, wl, hop, c[2], c[3])) and c[6] == e0
        e0 += c[5]
    assert p["energies"] == e0
    # the scratch grows with the members' samples, not with T * C
    assert e0 <= sum((n + wl) // hop + 2 for n in LEN) and e0 < T0 * 3 + T1
    # the word scratch: three runs of ceil(T / 64) words per column, with a smoothing length only
    assert [c[7] for c in cols] == [0, 3 * -(-T0 // 64), 6 * -(-T0 // 64), 9 * -(-T0 // 64)]
    assert p["words"] == 9 * -(-T0 // 64) + 3 * -(-T1 // 64)
    q = plan(probe, "mix", LEN, REQ, grid=grid)
    assert q["words"] == 0 and all(c[7] == 0 for c in q["cols"]) and q["units"] == p["units"]


def test_what_the_stage_reads(probe):
    # members: what the join reads (the final PCM); the unit: what the encoders read (the join slab, or the final PCM)
    for i16, final, join in ((0, "V64", "Join64"), (1, "S16", "Join16")):
        for kind, req in (("mix", REQ), ("join", REQ)):
            p = plan(probe, kind, LEN, req, i16=i16)
            assert (p["act_src"], p["act_i16"], p["join"]) == (final, bool(i16), join)
            assert [u[2] for u in p["units"]] == [3, 1]
            p = plan(probe, kind, LEN, req, i16=i16, columns=1)
            assert (p["act_src"], p["act_i16"]) == (join, bool(i16)) and [u[2] for u in p["units"]] == [1, 1]
            assert [c[2:4] for c in p["cols"]] == [[0, p_n] for p_n in unit_lengths(kind)]
        for columns in (0, 1):
            p = plan(probe, "none", LEN, i16=i16, columns=columns)
            assert (p["act_src"], p["join"]) == (final, "none")
            assert [u[2] for u in p["units"]] == [1] * 4 and [c[:4] for c in p["cols"]] == \
                [[u, u, 0, n] for u, n in enumerate(LEN)]
    # behind the converter the units take their own rates: in microseconds the window and the hop follow them
    p = plan(probe, "none", [4800, 4800], want=[0, 16000], flags=0, win=25000, hop=10000)
    assert p["act_src"] == "Conv64" and [u[3:5] for u in p["units"]] == [[1200, 480], [400, 160]]
    assert [u[1] for u in p["units"]] == [1 + (4800 - 1200) // 480, 1 + (1600 - 400) // 160]


def unit_lengths(kind):
    if kind == "mix":
        return [max(37 + 9000, 4001 + 7000, 555 + 7), 5 + 5000 + 11]
    # the join: each member behind the one in front, the word `start` read as pad_before
    return [37 + 9000 + 4001 + 7000 + 555 + 7, 5 + 5000 + 11]


def test_nothing_is_planned_without_the_request(probe):
    for kind, req in (("mix", REQ), ("join", REQ), ("none", None)):
        for i16 in (0, 1):
            off = plan(probe, kind, LEN, req, i16=i16, act=0)
            on = plan(probe, kind, LEN, req, i16=i16, min_gap=1)
            assert off["act_src"] == "none" and off["units"] == off["cols"] == []
            assert off["bytes"] == off["energies"] == off["words"] == 0
            # ... and with it nothing else moves: every slab of the plan, the routing (the stage's three blocks are its own)
            for k in ("final", "join", "alloc"):
                assert on[k] == off[k]
            assert on["bytes"] > 0 and on["energies"] > 0 and on["words"] > 0


def test_refusals(probe):
    for kw, word in ((dict(grid=4), "grid"), (dict(columns=2), "columns"), (dict(flags=2), "flags"),
                     (dict(gate_db=0.5), "gate_db"), (dict(min_gap=65536), "min_gap"), (dict(win=1), "win_us"),
                     (dict(win=4097), "win_us"), (dict(hop=0), "hop_us")):
        p = plan(probe, "none", LEN, **kw)
        assert word in p["fault"] and p["act_src"] == "none" and not p["unsupported"] and p["bytes"] == 0, kw
    # at some unit's rate only: 80 ms are 3840 samples at 48 kHz and 7680 at 96 kHz
    p = plan(probe, "none", [4800, 4800], want=[0, 96000], flags=0, win=80000, hop=10000)
    assert "win_us" in p["fault"] and p["fault_unit"] == 1 and p["act_src"] == "none"
    assert plan(probe, "none", [4800, 4800], flags=0, win=80000, hop=10000)["fault"] == ""
    # the caps: T * C of a unit, and the batch's label bytes
    big = [(0, 0, 0.0)] * 3
    p = plan(probe, "mix", [2 ** 29] * 3, big, win=2, hop=1)
    assert "T * C" in p["fault"] and p["unsupported"] and p["fault_unit"] == 0
    assert plan(probe, "mix", [2 ** 29] * 3, big, win=2, hop=1, columns=1)["fault"] == ""
    p = plan(probe, "none", [2 ** 29] * 3, win=2, hop=1)
    assert "together" in p["fault"] and p["unsupported"] and p["fault_unit"] == 2
    # 256 members by the flagship configuration's frames pass
    many = [(0, 0, 0.0)] * 256
    p = plan(probe, "mix", [3_270_000 * 160] + [160] * 255, many)
    assert p["fault"] == "" and p["units"][0][1:3] == [1 + (3_270_000 * 160 - 400) // 160, 256]


def test_the_stage_follows_the_units_mask(probe):
    # a unit with a rewritten member is measured again, whole: programme 0 for utterance 3, programme 1 for utterance 2
    assert plan(probe, "mix", LEN, REQ, only=[0, 0, 0, 1])["redo_units"] == [1, 0]
    assert plan(probe, "mix", LEN, REQ, only=[0, 0, 1, 0])["redo_units"] == [0, 1]
    assert plan(probe, "join", LEN, REQ, only=[0, 1, 1, 0])["redo_units"] == [1, 1]
    assert plan(probe, "none", LEN, only=[0, 1, 0, 1])["redo_units"] == [0, 1, 0, 1]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 200, 4097])
def test_packed_smoothing_steps_are_the_naive_ones(probe, T):
    rng = np.random.default_rng(T)
    patterns = [(rng.random(T) < p).astype(np.uint8) for p in (0.5, 0.05, 0.95)]
    patterns += [np.zeros(T, dtype=np.uint8), np.ones(T, dtype=np.uint8)]
    edge = np.zeros(T, dtype=np.uint8)
    edge[[0, T - 1, min(T - 1, 63), min(T - 1, 64)]] = 1
    patterns.append(edge)
    for bits in patterns:
        for kw in (dict(min_gap=1), dict(min_gap=70), dict(min_gap=65535), dict(min_speech=2), dict(min_speech=66),
                   dict(hang_before=1), dict(hang_after=1), dict(hang_before=65, hang_after=130),
                   dict(min_gap=3, min_speech=5, hang_before=2, hang_after=1)):
            full = {**dict(min_gap=0, min_speech=0, hang_before=0, hang_after=0), **kw}
            got = run(probe, "words", T, full["min_gap"], full["min_speech"], full["hang_before"], full["hang_after"],
                      *bits.tolist())
            assert got == R.smooth(bits, **kw).tolist(), (T, kw)

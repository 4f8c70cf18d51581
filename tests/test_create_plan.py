"""The shape rules of Batch::create (jbonsai_amd/csrc/jb_plan.h) on the host, without a GPU: the blocks a frame's
samples are cut into (plan_frame_blocks), the voiced runs of an LF0 track (plan_voiced_runs), the vocoder conditions of
a batch (plan_voc_conditions) and each stream's MLPG mode (plan_stream_mode).  A small C++ probe
(tests/plan/create_probe.cpp) is compiled with g++ against jb_plan.cpp, reads one request on stdin and prints what the
rule decides as JSON."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"
NODATA = -1e10          # src/constants.rs:13
GENERIC_MLPG = 2        # JB_BATCH_GENERIC_MLPG
MT_MAX_DIM = 60         # mlpg_mt_max_dim()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("create_plan") / "create_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "create_probe.cpp"), str(CSRC / "jb_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(exe, *words):
    r = subprocess.run([str(exe)], input=" ".join(repr(w) if isinstance(w, float) else str(w) for w in words) + "\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


# ---- frame blocks ----

def blocks(exe, fperiod, nlpf):
    return tuple(ask(exe, "blocks", fperiod, fperiod, nlpf, nlpf)[0])


def blocks_rule(fperiod, nlpf):
    """The rule as jb_plan.h words it: the largest divisor of the frame period that is <= 64 where there is a useful
    one -- it holds the filter's nlpf - 1 earlier samples and is at least 16, or it is already the largest block there
    can be --, otherwise the frame in the fewest blocks of at most 64, equal but for a shorter last one."""
    cap = min(64, fperiod)
    bs = max(d for d in range(1, cap + 1) if fperiod % d == 0)
    if bs != cap and (bs < nlpf - 1 or bs < 16):
        nblk = -(-fperiod // 64)
        bs = -(-fperiod // nblk)
    return bs, -(-fperiod // bs)


@pytest.mark.parametrize("fperiod,nlpf,bs,nblk", [
    (240, 31, 60, 4), (80, 31, 40, 2), (120, 15, 60, 2), (200, 31, 50, 4), (480, 31, 60, 8), (64, 31, 64, 1),
    (75, 31, 38, 2),  # short last block: 38 + 37
    (241, 31, 61, 4), (128, 0, 64, 2), (15, 31, 15, 1), (1, 31, 1, 1)])
def test_frame_blocks_pinned(probe, fperiod, nlpf, bs, nblk):
    assert blocks(probe, fperiod, nlpf) == (bs, nblk)


def test_frame_blocks_cover_the_frame(probe):
    """Every frame period 1..5000 under every tap count 0..129: blocks of 1..64 samples that cover the frame with
    none to spare, equal to the rule restated above; and wherever the split excitation kernels can take the shape
    (excite_is_split: a frame period that is a multiple of 4 and <= 256 under 15 or 31 taps), what they assume: at most
    four equal blocks."""
    F, N = range(1, 5001), range(0, 130)
    got = ask(probe, "blocks", F[0], F[-1], N[0], N[-1])
    assert len(got) == len(F) * len(N)
    it = iter(got)
    for fperiod in F:
        for nlpf in N:
            bs, nblk = next(it)
            assert 1 <= bs <= 64 and nblk * bs >= fperiod and (nblk - 1) * bs < fperiod, (fperiod, nlpf, bs, nblk)
            assert (bs, nblk) == blocks_rule(fperiod, nlpf), (fperiod, nlpf)
            if fperiod % 4 == 0 and fperiod <= 256 and nlpf in (15, 31):
                assert nblk <= 4 and fperiod % bs == 0, (fperiod, nlpf, bs, nblk)


# ---- voiced runs ----

def runs(exe, lf0):
    r = ask(exe, "runs", len(lf0), *[float(x) for x in lf0])
    d, m = r["durations"], r["msd"]
    assert len(d) == len(m) and sum(d) == len(lf0) and all(x > 0 for x in d)
    assert all(x in (0.0, 1.0) for x in m) and all(a != b for a, b in zip(m, m[1:]))
    return d, m


def test_voiced_runs(probe):
    assert runs(probe, []) == ([], [])
    assert runs(probe, [5.1, 5.2, 5.3]) == ([3], [1.0])
    assert runs(probe, [NODATA] * 4) == ([4], [0.0])
    u = NODATA
    assert runs(probe, [u, u, 5.0, 5.1, 5.2, u, 4.9, u, u, u]) == ([2, 3, 1, 1, 3], [0.0, 1.0, 0.0, 1.0, 0.0])
    # (only NODATA itself is unvoiced: a zero, a negative value, a value next to it are voiced frames)
    assert runs(probe, [0.0, -1.0, -0.99e10, u]) == ([3, 1], [1.0, 0.0])


# ---- vocoder conditions ----

def cond(exe, voice, utts, nmcp=35, stage=0):
    flat = [float(x) for t in (utts or []) for x in t]
    p = ask(exe, "cond", *[float(x) for x in voice], nmcp, stage, -1 if utts is None else len(utts), *flat)
    if not p["mixed"]:  # one condition: it stands in `batch`, and there is one class and no table
        assert p["utt"] == [] and p["cls"] == [] and p["n_classes"] == 1
    else:
        assert len(p["utt"]) == len(p["cls"]) == len(utts) and p["n_classes"] == max(p["cls"]) + 1
    return p


def test_one_condition(probe):
    voice = (0.55, 0.0, 1.0)
    p = cond(probe, voice, None)
    assert not p["mixed"] and p["pf_alphas"] == []
    assert p["batch"] == dict(alpha=0.55, volume=1.0, beta=0.0, beta_stage=0.0, pf=0)
    # every entry the same: the entries' condition, not the voice's, and still one
    p = cond(probe, voice, [(0.42, 0.3, 2.0)] * 5)
    assert not p["mixed"] and p["pf_alphas"] == [0.42]
    assert p["batch"] == dict(alpha=0.42, volume=2.0, beta=0.3, beta_stage=0.0, pf=0)
    # no utterance at all, with or without an (empty) list of entries
    assert cond(probe, (0.55, 0.4, 1.0), [])["batch"] == cond(probe, (0.55, 0.4, 1.0), None)["batch"]


def test_classes_and_operators_by_first_appearance(probe):
    #        alpha beta volume
    utts = [(0.55, 0.0, 1.0),   # class 0, no post-filter
            (0.42, 0.2, 1.0),   # class 1, operator 0.42
            (0.55, 0.3, 1.0),   # class 0 (beta is not part of a class), operator 0.55
            (0.42, 0.0, 0.5),   # class 2 (the volume differs)
            (0.55, 0.1, 1.0),   # class 0, operator 0.55 again
            (0.60, 0.5, 0.5),   # class 3, operator 0.60
            (0.42, 0.4, 0.5)]   # class 2, operator 0.42 again
    p = cond(probe, (0.9, 0.9, 0.9), utts)
    assert p["mixed"] and p["cls"] == [0, 1, 0, 2, 0, 3, 2] and p["n_classes"] == 4
    assert p["pf_alphas"] == [0.42, 0.55, 0.60]
    assert [u["pf"] for u in p["utt"]] == [0, 0, 1, 0, 1, 2, 0]
    for u, (a, b, v) in zip(p["utt"], utts):
        assert (u["alpha"], u["volume"], u["beta"], u["beta_stage"]) == (a, v, b, 0.0)
    # the batch-wide condition is utterance 0's, with the maxima of beta
    assert (p["batch"]["alpha"], p["batch"]["volume"]) == (0.55, 1.0)
    assert p["batch"]["beta"] == 0.5 and p["batch"]["beta_stage"] == 0.0
    # its alpha comes first among the operators when its beta is positive
    p = cond(probe, (0.9, 0.9, 0.9), [(0.60, 0.1, 1.0), (0.42, 0.2, 1.0), (0.60, 0.3, 1.0), (0.42, 0.0, 1.0)])
    assert p["pf_alphas"] == [0.60, 0.42] and [u["pf"] for u in p["utt"]] == [0, 1, 0, 0]
    assert p["cls"] == [0, 1, 0, 1] and p["batch"]["beta"] == 0.3


@pytest.mark.parametrize("nmcp,stage", [(2, 0), (1, 0), (35, 1), (35, 4), (2, 3)])
def test_beta_rule(probe, nmcp, stage):
    """postfilter_mcp acts only with more than two coefficients at stage 0; with stage > 0 beta goes to beta_stage."""
    p = cond(probe, (0.55, 0.4, 1.0), None, nmcp=nmcp, stage=stage)
    assert p["batch"]["beta"] == 0.0 and p["batch"]["beta_stage"] == (0.4 if stage else 0.0) and p["pf_alphas"] == []
    p = cond(probe, (0.55, 0.4, 1.0), [(0.55, 0.1, 1.0), (0.55, 0.7, 1.0), (0.42, 0.2, 1.0)], nmcp=nmcp, stage=stage)
    # (utterances that differ in beta alone differ only where some filter reads it)
    assert p["mixed"] and p["cls"] == [0, 0, 1] and p["pf_alphas"] == []
    assert [u["beta"] for u in p["utt"]] == [0.0] * 3 and [u["pf"] for u in p["utt"]] == [0] * 3
    assert [u["beta_stage"] for u in p["utt"]] == ([0.1, 0.7, 0.2] if stage else [0.0] * 3)
    assert p["batch"]["beta"] == 0.0 and p["batch"]["beta_stage"] == (0.7 if stage else 0.0)


def test_beta_alone_does_not_mix_where_no_filter_reads_it(probe):
    p = cond(probe, (0.55, 0.0, 1.0), [(0.55, 0.1, 1.0), (0.55, 0.7, 1.0)], nmcp=2, stage=0)
    assert not p["mixed"]
    p = cond(probe, (0.55, 0.0, 1.0), [(0.55, 0.1, 1.0), (0.55, 0.7, 1.0)], nmcp=35, stage=0)
    assert p["mixed"] and p["n_classes"] == 1 and p["batch"]["beta"] == 0.7 and p["pf_alphas"] == [0.55]


# ---- stream mode ----

def stream(exe, L, widths, is_msd=0, use_gv=0, si=0, flags=0, stage=0, from_tracks=False, mt_max_dim=MT_MAX_DIM):
    return ask(exe, "stream", L, len(widths), is_msd, use_gv, *widths, si, flags, stage, int(from_tracks), mt_max_dim)


MCP = dict(L=35, widths=[1, 3, 3], use_gv=1, si=0)
LF0 = dict(L=1, widths=[1, 3, 3], is_msd=1, use_gv=1, si=1)
LPF = dict(L=31, widths=[1], si=2)


def test_nitech_streams(probe):
    """the MCP stream in the [dim][frame] workspace with its transpose deferred to mc2b, the LF0 stream
    (MSD, one dim) with the generic kernels, the LPF stream the one-window case."""
    assert stream(probe, **MCP) == dict(W=3, BW=3, is_msd=0, use_gv=1, mt=1, defer_out=1, is_static=False)
    assert stream(probe, **LF0) == dict(W=3, BW=3, is_msd=1, use_gv=1, mt=0, defer_out=0, is_static=False)
    assert stream(probe, **LPF) == dict(W=1, BW=1, is_msd=0, use_gv=0, mt=0, defer_out=0, is_static=True)


def test_generic_mlpg_turns_the_fast_paths_off(probe):
    for s in (MCP, LF0, LPF):
        m = stream(probe, flags=GENERIC_MLPG, **s)
        assert (m["mt"], m["defer_out"], m["is_static"]) == (0, 0, False)
        assert {k: m[k] for k in ("W", "BW", "is_msd", "use_gv")} == \
               {k: stream(probe, **s)[k] for k in ("W", "BW", "is_msd", "use_gv")}


def test_tracks_as_the_source(probe):
    for s in (MCP, LF0, LPF):
        m = stream(probe, from_tracks=True, **s)
        assert m == dict(W=1, BW=1, is_msd=int(s["si"] == 1), use_gv=0, mt=0, defer_out=0, is_static=True)
    # the window description is not read (it may be absent): none at all gives the same
    assert stream(probe, 35, [], si=0, from_tracks=True) == stream(probe, from_tracks=True, **MCP)
    # MSD goes by the stream's index, not by its description
    assert stream(probe, 35, [1], is_msd=1, si=0, from_tracks=True)["is_msd"] == 0
    assert stream(probe, 1, [1], is_msd=0, si=1, from_tracks=True)["is_msd"] == 1


def test_defer_out_is_the_mcp_streams_at_stage_0(probe):
    assert stream(probe, **dict(MCP, stage=2)) == dict(stream(probe, **MCP), defer_out=0)
    assert stream(probe, **dict(MCP, si=2))["defer_out"] == 0
    assert stream(probe, **dict(MCP, is_msd=1)) == dict(stream(probe, **MCP), is_msd=1, defer_out=0)


def test_band_width_and_workspace(probe):
    assert stream(probe, 35, [1, 5, 3], use_gv=1) == dict(W=3, BW=5, is_msd=0, use_gv=1, mt=0, defer_out=0,
                                                         is_static=False)
    assert stream(probe, 35, [1, 3, 9])["BW"] == 9
    # [dim][frame]: band width 3, up to three windows, 3..mt_max_dim dims
    assert [stream(probe, L, [1, 3, 3])["mt"] for L in (1, 2, 3, 60, 61)] == [0, 0, 1, 1, 0]
    assert stream(probe, 35, [1, 3, 3], mt_max_dim=34)["mt"] == 0
    assert stream(probe, 35, [1, 3, 3, 3])["mt"] == 0 and stream(probe, 35, [1, 3])["mt"] == 1
    # the one-window case: a single window of width 1 and no GV
    assert stream(probe, 31, [1], use_gv=1)["is_static"] is False
    assert stream(probe, 31, [1, 1])["is_static"] is False
    assert stream(probe, 31, [3])["is_static"] is False

"""The MLPG / GV kernels (jb_mlpg.hip, jb_gv_gang.hip) through the C ABI against the dense extended-precision reference
(tests/mlpg_ref.py) and the oracle, on the case table of tests/mlpg_cases.py: stream shapes and voicing patterns that
no other GPU test feeds to launch_mlpg_bw -- MSD streams of 2, 4 and 35 dims on the [dim][frame] path, L = 2, L = 1
without MSD, MSD under band widths 5 / 7 / 9, voiced runs of 1..17 frames, more runs than a wave has lanes, zero-duration
states at run edges, msd equal to the threshold.

A voice needs three streams and the vocoder cannot take an MSD spectrum, so every case is an MLPG-only batch
(J.Batch(mlpg_only=True)); the stream under test sits in the slot whose shape rules take it (Case.slot) beside two
one-window streams.  Each case runs with the default flags, with generic_mlpg where the band width has fused kernels,
and with serial_gv and an injected gang timeout where the GV is time-parallel (serial_gv changes nothing elsewhere).

Gates (u = 2^-53), per utterance and dim:
  * the NODATA mask is the dense reference's and the oracle's;
  * where GV does not act: backward error <= 32 u and ||c - x||inf <= 64 cond_inf(A) u ||x||inf against the dense
    solve (tests/test_mlpg_dense.py has the reasoning);
  * where GV acts: e_gpu <= 4 e_oracle + 64 u, both relative to the dense long-double ascent in the inf-norm; the
    factor covers the fixed-shape sums of the time-parallel kernels;
  * the project's own contract: bit-equal to the oracle on every path but the time-parallel GV sums (serial_gv
    included), rtol 1e-12 / atol 1e-13 there; a duplicate utterance is bit-equal to its twin;
  * the path: what launch_mlpg_bw launches for the stream's mode (plan_stream_mode, asked through the create probe of
    tests/test_create_plan.py) is the path the case names, and gang_fallbacks() tells the resident GV kernel from its
    fallback.

JB_MLPG_DENSE_REPORT=<file> appends the measured worst values per window set."""
import copy
import os
import time

import numpy as np
import pytest

import jbonsai_amd as J
from oracle import oracle as O
from tests import mlpg_cases as C
from tests import mlpg_ref as R
from tests.test_create_plan import GENERIC_MLPG, probe, stream as plan_stream  # noqa: F401 (probe is a fixture)
from tests.test_mlpg_dense import BACKWARD_GATE, FORWARD_FACTOR

pytestmark = pytest.mark.gpu

_worst = {}
_t0 = time.time()


def _note(wset, **kw):
    w = _worst.setdefault(wset, dict(systems=0, backward_u=0.0, forward_cond_u=0.0, gv_ratio=0.0, gv_e_gpu=0.0,
                                     oracle_rel=0.0))
    for k, v in kw.items():
        w[k] = w[k] + v if k == "systems" else max(w[k], v)


@pytest.fixture(scope="module", autouse=True)
def report():
    assert J.lib().jb_device_count() > 0
    yield
    path = os.environ.get("JB_MLPG_DENSE_REPORT")
    if path and _worst:
        with open(path, "a") as fh:
            fh.write("GPU against the dense reference (tests/test_gpu_mlpg_dense.py), %.1f s for the file\n" % (time.time() - _t0))
            fh.write("%-22s %8s %12s %16s %22s %12s %14s\n" % ("window set", "systems", "backward/u", "forward/(cond u)",
                                                             "GV e_gpu/(e_oracle+16u)", "GV e_gpu", "vs oracle, rel"))
            for wset, w in _worst.items():
                fh.write("%-22s %8d %12.2f %16.2f %22.3f %12.2e %14.2e\n" % (
                    wset, w["systems"], w["backward_u"], w["forward_cond_u"], w["gv_ratio"], w["gv_e_gpu"], w["oracle_rel"]))


# ---- the voice and the batch ----

def _filler(slot):
    """A one-window stream for a slot the case does not use: (StreamInfo, states of an utterance of S states)."""
    L, msd = (2, False) if slot == 0 else (1, slot == 1)
    info = J.StreamInfo(L, msd, False, [[1.0]])
    return info, lambda S: J.StreamStates(np.zeros((S, L)), np.ones((S, L)), np.ones(S) if msd else None)


def voice_and_utts(case, dup=(3, 4)):
    """The case as a three-stream voice and its utterances; utterance dup[0] once more as the same object and dup[1]
    as a deep copy (the twins of the duplicate gate), at the end of the batch."""
    infos, fill = [None] * 3, [None] * 3
    for slot in range(3):
        infos[slot], fill[slot] = _filler(slot)
    infos[case.slot] = J.StreamInfo(case.L, case.is_msd, case.use_gv, case.windows)
    vi = J.VoiceInfo(48000, 240, 0.55, infos)
    utts = []
    for u in case.utts:
        s, S = u.stream, len(u.durations)
        sts = [fill[slot](S) for slot in range(3)]
        sts[case.slot] = J.StreamStates(s.mean, s.var, s.msd, s.gv_mean, s.gv_var, s.gv_switch, s.gv_weight,
                                        s.msd_threshold)
        utts.append(J.Utterance(u.durations, sts))
    twins = [k for k in dup if k < len(utts)]
    if twins:
        utts.append(utts[twins[0]])
    if len(twins) > 1:
        utts.append(copy.deepcopy(utts[twins[1]]))
    return vi, utts, twins


def run(case, **flags):
    vi, utts, twins = voice_and_utts(case)
    with J.Batch(vi, utts, mlpg_only=True, keep_tracks=True, **flags) as b:
        b.run()
        b.sync()
        tracks = [b.track(i, case.slot) for i in range(len(utts))]
        fallbacks = b.gang_fallbacks()
    n = len(case.utts)
    for k, t in zip(twins, tracks[n:]):
        assert np.array_equal(t, tracks[k]), (case.name, case.utts[k].name, "duplicate differs from its twin", flags)
    return tracks[:n], fallbacks


# ---- the path ----

def launch_path(mode, L, serial_gv=False, generic=False, win0_taps=1):
    """What launch_mlpg_bw launches for a stream of mode `mode` (plan_stream_mode's answer), restated."""
    bw, msd, gv = mode["BW"], bool(mode["is_msd"]), bool(mode["use_gv"])
    if mode["is_static"]:
        return "k_mlpg_static"
    t = "false" if msd else "true"  # the NONMSD template flag
    if bw == 3 and mode["mt"]:
        tp = gv and not serial_gv
        out = "k_mc2b_mt" if mode["defer_out"] else "k_mlpg_scatter_mt"
        return "k_mlpg_build_mt2 %s %s" % ("launch_fb time_parallel_gv" if tp else "k_mlpg_solve3<%s,true,true>" % t, out)
    if bw == 3 and not generic:
        if gv and L <= 2:
            fb = "k_mlpg_fb_runs" if (msd and L == 1 and win0_taps == 1) else "k_mlpg_solve3<%s,false>" % t
            return "k_mlpg_build<3> %s k_mlpg_gv_vt<%s>" % (fb, t)
        return "k_mlpg_build<3> k_mlpg_solve3<%s,true>" % t
    return "k_mlpg_build<%d> k_mlpg_solve<%d>" % (bw, bw)


# The path each stream shape NAMES under band width 3 with the default flags: (L, MSD, GV) -> launches
NAMED = {
    (1, True, True): "k_mlpg_build<3> k_mlpg_fb_runs k_mlpg_gv_vt<false>",
    (1, True, False): "k_mlpg_build<3> k_mlpg_solve3<false,true>",
    (1, False, True): "k_mlpg_build<3> k_mlpg_solve3<true,false> k_mlpg_gv_vt<true>",
    (1, False, False): "k_mlpg_build<3> k_mlpg_solve3<true,true>",
    (2, True, True): "k_mlpg_build<3> k_mlpg_solve3<false,false> k_mlpg_gv_vt<false>",
    (2, True, False): "k_mlpg_build<3> k_mlpg_solve3<false,true>",
    (2, False, True): "k_mlpg_build<3> k_mlpg_solve3<true,false> k_mlpg_gv_vt<true>",
    (2, False, False): "k_mlpg_build<3> k_mlpg_solve3<true,true>",
    (4, True, True): "k_mlpg_build_mt2 launch_fb time_parallel_gv k_mlpg_scatter_mt",
    (4, True, False): "k_mlpg_build_mt2 k_mlpg_solve3<false,true,true> k_mlpg_scatter_mt",
    (4, False, True): "k_mlpg_build_mt2 launch_fb time_parallel_gv k_mc2b_mt",
    (4, False, False): "k_mlpg_build_mt2 k_mlpg_solve3<true,true,true> k_mc2b_mt",
    (35, True, True): "k_mlpg_build_mt2 launch_fb time_parallel_gv k_mlpg_scatter_mt",
    (35, True, False): "k_mlpg_build_mt2 k_mlpg_solve3<false,true,true> k_mlpg_scatter_mt",
}


def named_path(case):
    bw = C.band_width(case.windows)
    if bw == 3:
        return NAMED[(case.L, case.is_msd, case.use_gv)]
    return "k_mlpg_build<%d> k_mlpg_solve<%d>" % (bw, bw)


def modes_of(case):
    """[(label, Batch flags, serial_gv, generic)] the case runs with."""
    out = [("default", {}, False, False)]
    if C.band_width(case.windows) == 3:
        out.append(("generic_mlpg", dict(generic_mlpg=True), False, True))
        if case.L > 2 and len(case.windows) <= 3 and case.use_gv:
            out.append(("serial_gv", dict(serial_gv=True), True, False))
            out.append(("gang_timeout", dict(test_gang_timeout=True), False, False))
    return out


def plan_mode(exe, case, generic=False):
    return plan_stream(exe, case.L, [len(w) for w in case.windows], is_msd=int(case.is_msd), use_gv=int(case.use_gv),
                       si=case.slot, flags=GENERIC_MLPG if generic else 0)


# ---- the gates ----

def contract_miss(got, want, exact):
    """The project's own contract against the oracle: None where it holds, else what misses it."""
    if not np.array_equal(got == O.NODATA, want == O.NODATA):
        return "NODATA mask differs from the oracle's"
    if exact:
        return None if np.array_equal(got, want) else "not bit-equal: max |diff| %.3e" % float(np.abs(got - want).max())
    over = np.abs(got - want) / (1e-13 + 1e-12 * np.abs(want))
    return None if (over <= 1.0).all() else "%d elements over rtol 1e-12 / atol 1e-13, worst %.2f x at %s (|diff| %.3e)" % (
        int((over > 1.0).sum()), float(over.max()), np.unravel_index(int(over.argmax()), over.shape),
        float(np.abs(got - want).max()))


def contract(got, want, exact, what):
    miss = contract_miss(got, want, exact)
    assert miss is None, (what, miss)


def check_case(case, tracks, exact, what):
    """Every gate on every utterance; the figures of what misses are printed and returned, nothing stops early."""
    misses = []

    def gate(ok, *words):
        if not ok:
            print("MISS", *words)
            misses.append(words)

    for i, u in enumerate(case.utts):
        d = C.dense(case.wset, case.shape, case.use_gv, i)
        got, ref = tracks[i], C.oracle_track(case, i)
        w = what + (u.name,)
        mask = R.voiced_mask(u.stream, u.durations)
        assert got.shape == ref.shape == (len(mask), case.L), w
        gate(np.array_equal(got != R.NODATA, np.repeat(mask[:, None], case.L, axis=1)), w, "NODATA mask differs from dense")
        miss = contract_miss(got, ref, exact)
        gate(miss is None, w, miss)
        if len(d["vidx"]):
            v = ref[d["vidx"]]
            _note(case.wset, oracle_rel=float(np.abs(got[d["vidx"]] - v).max() / np.abs(v).max()))
        for k, dim in enumerate(d["dims"]):
            A, b = d["systems"][k]
            if len(b) == 0:
                continue
            c = got[d["vidx"], dim]
            _note(case.wset, systems=1)
            if not (case.use_gv and R.gv_switch_frames(u.stream, u.durations, d["vidx"]).any()):
                be = R.backward_error(A, b, c)
                fe = R.rel_inf(c, d["x"][k]) / (d["cond"][k] * R.U)
                _note(case.wset, backward_u=be / R.U, forward_cond_u=fe)
                gate(be <= BACKWARD_GATE, w, dim, "backward error / u", be / R.U)
                gate(fe <= FORWARD_FACTOR, w, dim, "forward error / (cond u)", fe)
            else:
                e_gpu = R.rel_inf(c, d["par"][k])
                e_oracle = R.rel_inf(ref[d["vidx"], dim], d["par"][k])
                _note(case.wset, gv_ratio=e_gpu / (e_oracle + 16 * R.U), gv_e_gpu=e_gpu)
                gate(e_gpu <= 4 * e_oracle + 64 * R.U, w, dim, "GV e_gpu, e_oracle", e_gpu, e_oracle)
    return misses


@pytest.mark.parametrize("wset,shape,use_gv", C.TABLE, ids=["%s-%s-%s" % (w, s, "gv" if g else "nogv") for w, s, g in C.TABLE])
def test_gpu_against_dense_and_oracle(probe, wset, shape, use_gv):
    case = C.build_case(wset, shape, use_gv)
    misses = []
    for label, flags, serial_gv, generic in modes_of(case):
        path = launch_path(plan_mode(probe, case, generic), case.L, serial_gv, generic)
        if label == "default":
            assert path == named_path(case), (case.name, path)
        elif label == "generic_mlpg":
            assert path == "k_mlpg_build<3> k_mlpg_solve<3>", (case.name, path)
        elif label == "serial_gv":
            assert "k_mlpg_solve3" in path and "time_parallel_gv" not in path, (case.name, path)
        tracks, fallbacks = run(case, **flags)
        time_parallel = "time_parallel_gv" in path
        # the resident kernel (jb_gv_gang.hip) where it is planned, k_mlpg_gv_tp after the injected timeout
        assert fallbacks == (1 if label == "gang_timeout" else 0), (case.name, label, fallbacks)
        misses += check_case(case, tracks, not time_parallel, (case.name, label))
    assert not misses, misses


def test_every_branch_the_suite_never_ran_is_named():
    """The launch branches no other GPU test reaches, each named by a case of the table (which asserts above that the
    stream's mode leads there)."""
    named = {named_path(C.build_case(*k)) for k in C.TABLE}
    for path in ("k_mlpg_build_mt2 launch_fb time_parallel_gv k_mlpg_scatter_mt",           # MSD, L >= 3, GV
                 "k_mlpg_build_mt2 k_mlpg_solve3<false,true,true> k_mlpg_scatter_mt",       # ... without GV / serial
                 "k_mlpg_build<3> k_mlpg_solve3<false,false> k_mlpg_gv_vt<false>",           # L = 2, MSD
                 "k_mlpg_build<3> k_mlpg_solve3<true,false> k_mlpg_gv_vt<true>",             # L = 1 or 2 without MSD, GV
                 "k_mlpg_build<3> k_mlpg_fb_runs k_mlpg_gv_vt<false>",                       # one lane per voiced run
                 "k_mlpg_build<5> k_mlpg_solve<5>", "k_mlpg_build<7> k_mlpg_solve<7>", "k_mlpg_build<9> k_mlpg_solve<9>"):
        assert path in named, path
    for bw in (5, 7, 9):  # ... the generic solve with an MSD stream of L >= 2
        assert any(C.band_width(C.WINDOW_SETS[w]) == bw and C.SHAPES[s] in ((2, True), (4, True), (35, True))
                   for w, s, _ in C.TABLE), bw


def test_mlpg_batch_entry_and_the_multi_launch_sweeps(probe):
    """The same case through jb_mlpg_batch (the one-shot entry), and the time-parallel GV of an MSD stream in its
    third form, k_mlpg_gv_gsweep (the invariant mode's fallback: the resident kernel's sums, so the same bits)."""
    case = C.build_case("nitech_1_3_3", "L4_msd", True)
    vi, utts, _ = voice_and_utts(case, dup=())
    want, _ = run(case)
    for serial_gv in (False, True):
        got = J.mlpg_batch(vi, utts, serial_gv=serial_gv)
        for i, u in enumerate(case.utts):
            contract(got[i][case.slot], C.oracle_track(case, i), serial_gv, (case.name, "mlpg_batch", serial_gv, u.name))
            if not serial_gv:
                assert np.array_equal(got[i][case.slot], want[i]), u.name
    resident, f0 = run(case, fast_invariant=True)
    swept, f1 = run(case, fast_invariant=True, test_gang_timeout=True)
    assert (f0, f1) == (0, 1)
    assert not check_case(case, swept, False, (case.name, "gsweep"))
    for a, b in zip(resident, swept):
        assert np.array_equal(a, b)


def test_long_msd_utterance(probe):
    """2,055 voiced frames of 2,582, L = 4, MSD, GV with a third of the states switched off: one 2,048-frame tile of
    the time-parallel GV plus its halo, five wave windows of the resident kernel, on the compacted system.  Against the
    oracle (a dense long-double solve of this size takes too long), under the project's own contract."""
    case = C.long_msd_case()
    want = C.oracle_track(case, 0)
    assert int((want[:, 0] != O.NODATA).sum()) == 2055 and np.isfinite(want).all()
    assert launch_path(plan_mode(probe, case), case.L) == NAMED[(4, True, True)]
    misses = []
    for label, flags, exact in (("default", {}, False), ("gang_timeout", dict(test_gang_timeout=True), False),
                                ("serial_gv", dict(serial_gv=True), True), ("generic_mlpg", dict(generic_mlpg=True), True)):
        vi, utts, _ = voice_and_utts(case, dup=())
        with J.Batch(vi, utts + [utts[0]], mlpg_only=True, **flags) as b:
            b.run()
            b.sync()
            got, twin, fallbacks = b.track(0, 0), b.track(1, 0), b.gang_fallbacks()
        assert fallbacks == (1 if label == "gang_timeout" else 0), label
        assert np.array_equal(got, twin), label
        miss = contract_miss(got, want, exact)
        if miss:
            print("MISS long", label, miss)
            misses.append((label, miss))
    assert not misses, misses


# ---- a first window of more than one tap: the reference's own result (tests/test_mlpg_dense.py), oracle only ----

def quirk_case(wset, shape):
    """The case with the utterances whose oracle track is finite.  Where no dynamic window reaches the last voiced frames
    (one or two voiced frames, isolated one-frame runs) the terms that the reference drops leave its matrix singular
    and the reference itself divides by zero; there is no parity to hold there."""
    full = C.build_case(wset, shape, True, quirk=True)
    keep = [u for i, u in enumerate(full.utts) if np.isfinite(C.oracle_track(full, i)).all()]
    return C.Case(full.wset, full.shape, True, full.windows, full.L, full.is_msd, keep, tag="-quirk-finite")


@pytest.mark.parametrize("wset,shape", [("static_3_taps", "L1_msd"), ("static_3_taps", "L4"), ("static_2_taps", "L1_msd"),
                                        ("static_2_taps", "L4")])
def test_static_window_of_more_than_one_tap(probe, wset, shape):
    """[[0.1, 0.8, 0.1], ...] and [[0.2, 0.8], ...] as the first window.  It is never zeroed at an MSD boundary, so it
    couples the voiced runs of the compacted sequence: the one-lane-per-run kernel (k_mlpg_fb_runs) does not apply and
    launch_mlpg_bw sends such a stream through the whole-utterance sweep of k_mlpg_solve3.  Bit-equal to the oracle on the LF0-shaped and the serial
    paths, rtol 1e-12 on the time-parallel sums."""
    case = quirk_case(wset, shape)
    assert len(case.utts) >= 12 and any(int(u.durations.sum()) >= 12 for u in case.utts)
    if case.is_msd:  # several runs, more than a wave has lanes among them
        assert any(u.name == "runs_1_to_17" for u in case.utts) and any(u.name == "130_one_frame_states" for u in case.utts)
    for i in range(len(case.utts)):
        assert np.isfinite(C.oracle_track(case, i)).all(), case.utts[i].name
    misses = []
    for label, flags, serial_gv, generic in modes_of(case):
        path = launch_path(plan_mode(probe, case, generic), case.L, serial_gv, generic, win0_taps=len(case.windows[0]))
        if label == "default" and shape == "L1_msd":
            assert path == "k_mlpg_build<3> k_mlpg_solve3<false,false> k_mlpg_gv_vt<false>"
        vi, utts, twins = voice_and_utts(case)
        with J.Batch(vi, utts, mlpg_only=True, **flags) as b:
            b.run()
            b.sync()
            tracks = [b.track(i, case.slot) for i in range(len(utts))]
        for k, t in zip(twins, tracks[len(case.utts):]):
            assert np.array_equal(t, tracks[k]), (case.name, label)
        for i, u in enumerate(case.utts):
            miss = contract_miss(tracks[i], C.oracle_track(case, i), "time_parallel_gv" not in path)
            if miss:
                print("MISS", case.name, label, u.name, miss)
                misses.append((label, u.name, miss))
    assert not misses, misses

"""The loudness measurement on the GPU (jb_loudness.hip: k_ln_tiles<false/true>, k_ln_scan, k_ln_gate, k_ln_gate_group,
k_ln_windows, k_ln_range, k_ln_true_peak) under a measured gate, at every tiling class of tests/loudness_ld_cases.py.

Error measure: for a loudness value V (L, the momentary and the short-term maximum, the two order statistics of LRA)
e(V) = |V - V_ld| in LU, V_ld from the long-double definition (tests/loudness_ld_ref.py).  e64 is that measure for the
ordinary serial f64 evaluation (tests/loudness_ref.py), the largest over the rate's cases of one signal kind and over
the values.  The device is held to

    e_gpu <= GATE * e64 + FLOOR_ULPS * spacing(|V_ld|),    GATE = 8 (tests/fbank_ref.py, the project's one factor).

The floor is what a value handed out as one f64 cannot resolve, whatever the hop energies behind it: on white noise e64
is as small as 1e-15 LU, a third of the spacing of L itself (3.6e-15 in [-32, -16)).  Behind the last sum stand
  a division  sum / count    half an ulp of the mean square, 10 / ln 10 * 2^-53 = 4.8e-16 LU:    <= 0.14 ulp(V)
  a log10     2 ulp of log10(ms) on the device (the accuracy class of the device library's f64 log10; libm's, which
              e64 contains, is below 1): V' = 10 log10(ms) lies three or four binades above log10(ms), so one ulp of
              the logarithm is 10/8 = 1.25 ulp(V') at most:                                       <= 2.5 ulp(V)
  a product   10 * log10:                                                                        <= 0.5 ulp(V)
  an add      -0.691 + V' (|V| <= |V'| here, V' < 0):                                             <= 0.5 ulp(V)
in all 3.64, rounded up: FLOOR_ULPS = 4.  It is not sized from any device result.

The sample peak in dB is within 2 ulp of 20 log10(max |x| / 32768) in long double (the maximum itself is exact), and
-inf is matched exactly for 4 H - 1 samples, silence and an input under -70 LUFS.

What the gate found (profiles/loudness_ld.txt): with the powers of the state transition squared in f64 on the host and
states carried as the recursion holds them, a DC offset cost 8e-10 LU at 48 kHz (9 times the gate), 3.4e-7 at 384 kHz
and 2.9e-6 at 614,390 Hz (750 times), white noise up to 36 times the gate above 300 kHz -- all invisible to a 1e-8
comparison at the rates the older tests run.  With the powers made in extended precision and states carried as
(t0 + t1, t1) (jb_loudness.hip: mat_pow, ln_to_scan) the worst value uses 0.70 of the gate.

The true peak at the classes tests/test_gpu_true_peak.py leaves out goes through that file's reference and gate.

JB_LOUDNESS_LD_REPORT=<file> appends, per rate and signal kind, e64, the device's worst e, their ratio, the worst share
of the gate used and the smallest gate margin of the cases."""
import math
import os
import time

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import loudness_ld_cases as T
from tests import loudness_ld_ref as R
from tests.conftest import VOICE
from tests.fbank_ref import GATE, have_long_double
from tests.loudness_ref import integrated
from tests.true_peak_ref import factor, true_peak

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not have_long_double(), reason="numpy.longdouble has no 64-bit mantissa here")]

FLOOR_ULPS = 4
PEAK_ULPS = 2
TP_TOL = 1e-10  # tests/test_gpu_true_peak.py
R128_KEYS = {"max_momentary": "max_momentary_lufs", "max_short_term": "max_short_term_lufs",
             "lra_low": "lra_low_lufs", "lra_high": "lra_high_lufs"}

_rows = {}
_t0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def report():
    assert J.lib().jb_device_count() > 0
    yield
    path = os.environ.get("JB_LOUDNESS_LD_REPORT")
    if path and _rows:
        with open(path, "a") as fh:
            fh.write("GPU against the long-double definition (tests/test_gpu_loudness_ld.py), %.1f s for the file\n"
                     % (time.time() - _t0))
            fh.write("%8s %-8s %6s %11s %11s %10s %12s %10s\n" % ("hz", "kind", "values", "e64", "e_gpu", "e_gpu/e64",
                                                                 "e_gpu/gate", "margin LU"))
            for (hz, kind), w in _rows.items():
                fh.write("%8d %-8s %6d %11.3e %11.3e %10.3f %12.3f %10.3g\n" % (
                    hz, kind, w["values"], w["e64"], w["e_gpu"], w["e_gpu"] / w["e64"] if w["e64"] else math.inf,
                    w["share"], w["margin"]))


def _note(hz, kind, e64, e, share, margin):
    w = _rows.setdefault((hz, kind), dict(values=0, e64=e64, e_gpu=0.0, share=0.0, margin=math.inf))
    w["values"] += 1
    w["e_gpu"], w["share"], w["margin"] = max(w["e_gpu"], e), max(w["share"], share), min(w["margin"], margin)


def hold(hz, kind, n, name, got, ref, e64, failures):
    """One device value against the gate; a miss is collected, so that a failing rate shows every value that misses."""
    want = getattr(ref, name)
    if not np.isfinite(want):
        ok = (math.isnan(got) and np.isnan(want)) or got == want
        if not ok:
            failures.append("%s %d %s: %r, the definition gives %r" % (kind, n, name, got, float(want)))
        return
    e = T.err(got, want)
    gate = GATE * e64 + FLOOR_ULPS * float(np.spacing(abs(float(want))))
    print("%7d %-8s %7d %-15s e_gpu %.3e  e64 %.3e  gate %.3e" % (hz, kind, n, name, e, e64, gate))
    _note(hz, kind, e64, e, e / gate, ref.margin)
    if not e <= gate:
        failures.append("%s %d %s: e_gpu %.3e over the gate %.3e (e64 %.3e, %.1f x)" % (kind, n, name, e, gate, e64,
                                                                                       e / gate))


def hold_peak(kind, n, P, x, failures):
    want = R.peak_db_ld(x)
    if not np.isfinite(want):
        if P != want:
            failures.append("%s %d peak: %r for silence" % (kind, n, P))
        return
    e, tol = T.err(P, want), PEAK_ULPS * float(np.spacing(abs(float(want))))
    print("        %-8s %7d peak            e %.3e  %d ulp %.3e" % (kind, n, e, PEAK_ULPS, tol))
    if not e <= tol:
        failures.append("%s %d peak: %.3e off, %d ulp are %.3e" % (kind, n, e, PEAK_ULPS, tol))


# ---- the measurement by tiling class ----------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", list(T.RATES))
def test_seam_by_tiling_class(hz):
    T.check_table()
    cases = T.cases(hz)
    sigs = [T.pcm(hz, k, n) for k, n in cases]
    got = J.loudness(sigs, hz)
    grp = J.loudness_groups(sigs, hz)            # every utterance its own group: steps 6 to 8 over the same hop energies
    e64 = {k: T.e64(hz, k, cases) for k in {k for k, _ in cases}}
    H = T.RATES[hz][0]
    failures = []
    for i, ((kind, n), x, (L, P)) in enumerate(zip(cases, sigs, got)):
        ref = T.reference(hz, kind, n)
        hold(hz, kind, n, "lufs", L, ref, e64[kind], failures)
        hold_peak(kind, n, P, x, failures)
        g = grp["groups"][grp["group_of"][i]]
        # a group of one member is the ungrouped result bit for bit (the header's step 6)
        assert grp["lufs"][i] == L and g["lufs"] == L and g["sample_peak_dbfs"] == P and g["members"] == 1
        for r128 in (grp["r128"][i], g["r128"]):
            hold(hz, kind, n, "max_momentary", r128["max_momentary_lufs"], ref, e64[kind], failures)
            assert r128["max_short_term_lufs"] == -math.inf and r128["n_windows"] == 0 and r128["lra_lu"] == 0.0
        if n < 4 * H or kind in ("quiet", "silence"):
            assert L == -math.inf, (kind, n, L)
        if kind == "silence":
            assert P == -math.inf
    assert not failures, "\n".join(failures)


def test_hop_and_block_count_edges():
    """The lane chunks of k_ln_scan (64 lanes: 63, 64, 65, 127, 128 and 129 hops) and more blocks than k_ln_gate has
    lanes (300 hops: 297 blocks, 271 short-term windows), on a carried state under level steps, every utterance its own
    group: utt_lufs and the group's L, and both copies of the R128 fields."""
    hz = T.EDGE_HZ
    cases = T.edge_cases()
    sigs = [T.pcm(hz, k, n) for k, n in cases]
    grp = J.loudness_groups(sigs, hz)
    e64 = T.e64(hz, "edge", cases)
    failures = []
    for i, ((kind, n), x) in enumerate(zip(cases, sigs)):
        ref = T.reference(hz, kind, n)
        g = grp["groups"][grp["group_of"][i]]
        assert g["lufs"] == grp["lufs"][i] and g["members"] == 1
        hold(hz, kind, n, "lufs", grp["lufs"][i], ref, e64, failures)
        hold_peak(kind, n, g["sample_peak_dbfs"], x, failures)
        for r128 in (grp["r128"][i], g["r128"]):
            assert r128["n_windows"] == ref.n_windows > 0
            for name, key in R128_KEYS.items():
                hold(hz, kind, n, name, r128[key], ref, e64, failures)
            # LRA is the difference of its two order statistics: both gates, and the rounding of the quotient's log10
            lo, hi = float(ref.lra_low), float(ref.lra_high)
            tol = 2 * GATE * e64 + FLOOR_ULPS * float(np.spacing(abs(lo)) + np.spacing(abs(hi)))
            if not T.err(r128["lra_lu"], ref.lra) <= tol:
                failures.append("%s %d lra: %.3e off, the gate is %.3e" % (kind, n, T.err(r128["lra_lu"], ref.lra), tol))
    assert not failures, "\n".join(failures)


# ---- true peak at the classes it has not seen -------------------------------------------------------------------------
def quarter_sine(n, amp=20000.0):
    return amp * np.sin(0.5 * np.pi * np.arange(n) + 0.25 * np.pi)


def pair(n, k, v=10000.0):
    x = np.zeros(n)
    x[k] = x[k + 1] = v
    return x


def sample_peak(x):
    m = float(np.max(np.abs(x)))
    return 20.0 * math.log10(m / 32768.0) if m > 0 else -math.inf


@pytest.mark.parametrize("hz, F, b", [(3000, 64, 300), (40960, 5, 4096), (81920, 3, 4096)])
def test_true_peak_at_the_cap_and_at_a_boundary_of_4096(hz, F, b):
    """3,000 Hz: F = 64, the cap of the oversampling factor (and a rate under the loudness limit: the true peak reads no
    hop energy and is measured all the same).  40,960 and 81,920 Hz: the first tile ends at exactly 4096 samples, a hop
    boundary at the one and an inner tile boundary at the other.  Pulse pairs at k = b - 7 .. b + 5 around it."""
    h, tph, S, G, last = T.tile_of(hz)
    assert factor(hz) == F and min(G, h) == b and (hz == 3000 or G == 4096) and tph == (2 if hz == 81920 else 1)
    rng = np.random.default_rng(hz)
    N = b + h + 13
    sigs = [rng.standard_normal(N) * 2000.0, quarter_sine(N)] + [pair(N, k) for k in range(b - 7, b + 6)]
    got = J.true_peak(sigs, hz)
    want_pair = true_peak(sigs[2], hz)
    for i, (x, tp) in enumerate(zip(sigs, got)):
        want = true_peak(x, hz)
        assert abs(tp - want) <= TP_TOL, (i, tp, want)
        assert tp >= sample_peak(x)
        if i >= 2:  # the pair's value does not depend on where the pair stands
            assert abs(want - want_pair) <= 1e-12
    if F % 2 == 0:  # the half-sample phase exists: the pair's midpoint is reached
        assert got[2] == pytest.approx(20.0 * math.log10(1.24054 * 10000.0 / 32768.0), abs=1e-4)


# ---- the low-rate refusal in a batch ----------------------------------------------------------------------------------
# (from the voice's 48 kHz the converter reaches 3,360 Hz = 48000 * 7 / 100 and 3,375 Hz = 48000 * 9 / 128, not 3,363 or
# 3,364 themselves; the limit itself is held at the seams, tests/test_loudness_abi.py)
@pytest.fixture(scope="module")
def voice():
    eng = J.Engine.load([VOICE])
    return eng.voice_info(), [synth.synth_utterance(synth.VoiceTables(eng), 700, 4100)]


def _run(voice, out_hz, target, report=False, mode=None):
    vi, utts = voice
    with J.Batch(vi, utts) as b:
        b.set_output_rate(out_hz)
        b.set_loudness_target(target, math.inf)
        if mode is not None:
            b.set_peak_mode(mode)
        if report:
            b.set_loudness_report()
        b.run()
        b.sync()
        return b.pcm(0), b.loudness(0), (b.loudness_r128(0) if report else None)


@pytest.mark.parametrize("how", ["target", "measure only", "r128 report", "true-peak mode"])
def test_batch_refuses_a_loudness_value_at_3360_hz(voice, how):
    kw = {"target": dict(target=-23.0), "measure only": dict(target=math.nan),
          "r128 report": dict(target=math.nan, report=True),
          "true-peak mode": dict(target=-23.0, mode=J.PEAK_TRUE)}[how]
    with pytest.raises(J.JbError) as ei:
        _run(voice, 3360, **kw)
    assert ei.value.code == -2
    assert "3360 Hz" in str(ei.value) and "shelf" in str(ei.value) and "Nyquist" in str(ei.value)


def test_batch_accepts_3375_hz(voice):
    pcm, (lufs, peak, gain), r128 = _run(voice, 3375, math.nan, report=True)
    assert gain == 0.0 and pcm.size > 30 * 338
    ref = R.measure(pcm, 3375)
    ref.check_margin("3375 Hz")
    wL, wP = integrated(pcm, 3375)
    # (accepted and measured: the gate of tests/test_gpu_loudness.py; the class is held to the measured gate at 3,400 Hz)
    assert math.isfinite(wL) and abs(lufs - wL) <= 1e-8 and abs(peak - wP) <= 1e-12
    assert T.err(lufs, ref.lufs) <= 1e-8
    assert r128["n_windows"] == ref.n_windows > 0

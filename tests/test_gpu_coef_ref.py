"""The coefficient kernels through the C ABI against the extended-precision reference (tests/coef_ref.py) on the tables
of tests/coef_cases.py: k_postfilter with k_pf_table (jb_postfilter.hip, the mel-cepstral post-filter, beta > 0) and
k_stage_coef (jb_mglsa.hip, Stage::NonZero: postfilter_lsp, check_lsp_stability, lsp2lpc, ignorm, gc2gc, gnorm, mc2b).
tests/test_coef_ref.py holds the CPU oracle to the same reference; its worst error per class and gate group is the
e_oracle here.

The gate is R.within: e_gpu <= 4 e_oracle + floor.  Post-filter, per row, absolute: floor 64 u max(1, |b'[0]|) for
b'[0] and 16 u max|b'| for b'[1:].  Stage, worst over the class's rows on both sides, relative in the inf-norm: 64 u.
Beside it, bit for bit: first_coefficients() is the plain mc2b of frame 0, a one-frame utterance is frame 0 of the long
one, the all-zero row stays zero, beta = 0 utterances of a mixed batch are the plain mc2b, two runs agree.  The PCM of
these batches is checked for length and finiteness only (fperiod = 16; tests/test_gpu_mlsa_transfer.py has the filter).

Every gate of a case is evaluated and printed before the test fails.  JB_COEF_REF_REPORT=<file> appends the worst
e_gpu, e_oracle and e_gpu / (e_oracle + floor / 4) per class (profiles/coef_ref.txt)."""
import os
import time

import numpy as np
import pytest

import jbonsai_amd as J
from tests import coef_cases as C
from tests import coef_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.wide_enough(), reason="numpy.longdouble is no wider than f64 here")]

_worst = {}


def _note(key, e_gpu, e_oracle, floor):
    w = _worst.setdefault(key, dict(e_gpu=0.0, e_oracle=e_oracle, ratio=0.0))
    w["e_gpu"], w["e_oracle"] = max(w["e_gpu"], e_gpu), max(w["e_oracle"], e_oracle)
    w["ratio"] = max(w["ratio"], C.ratio(e_gpu, e_oracle, floor))


@pytest.fixture(scope="module", autouse=True)
def report():
    assert J.lib().jb_device_count() > 0
    _t0 = time.time()
    yield
    path = os.environ.get("JB_COEF_REF_REPORT")
    if path and _worst:
        with open(path, "a") as fh:
            fh.write("GPU against the extended-precision reference (tests/test_gpu_coef_ref.py), %.1f s for the file\n"
                     % (time.time() - _t0))
            fh.write("%-44s %10s %10s %s\n" % ("class", "e_gpu", "e_oracle", "e_gpu / (e_oracle + floor / 4); the gate is 4"))
            for key, w in _worst.items():
                fh.write("%-44s %10.2e %10.2e %.3f\n" % (key, w["e_gpu"], w["e_oracle"], w["ratio"]))
            fh.write("\n")


class Gates:
    """Collects what misses; nothing stops early."""

    def __init__(self):
        self.misses = []

    def __call__(self, ok, *words):
        if not ok:
            print("MISS", *words)
            self.misses.append(words)


# ---- voices and utterances -------------------------------------------------------------------------------------------
def voice_of(n, alpha, beta=0.0, stage=0, log_gain=False):
    streams = [J.StreamInfo(n, False, False, [[1.0]]), J.StreamInfo(1, True, False, [[1.0]]),
               J.StreamInfo(1, False, False, [[1.0]])]
    return J.VoiceInfo(C.FS, C.FPERIOD, alpha, streams, beta=beta, stage=stage, use_log_gain=log_gain)


def track_utt(rows):
    """Parameter tracks: the rows as the spectrum, every frame unvoiced, lpf = [1.0]."""
    T = len(rows)
    return J.TrackUtterance(np.asarray(rows), np.full((T, 1), R.M.NODATA), np.ones((T, 1)))


def state_utt(rows):
    """State level: one frame per state, one-tap windows, mean = the row (so the generated track is the rows)."""
    S = len(rows)
    return J.Utterance(np.ones(S, dtype=np.uint32),
                       [J.StreamStates(np.asarray(rows), np.ones((S, rows.shape[1]))),
                        J.StreamStates(np.zeros((S, 1)), np.ones((S, 1)), np.zeros(S)),
                        J.StreamStates(np.ones((S, 1)), np.ones((S, 1)))])


def run_twice(voice, utts, g, what, first=True, tracks=False, **kw):
    """[(coefficients, first_coefficients or None, track or None)] per utterance; two runs must agree bit for bit, and
    the PCM has T * fperiod finite samples."""
    with J.Batch(voice, utts, keep_tracks=tracks, **kw) as b:
        outs = []
        for _ in range(2):
            b.run()
            b.sync()
            n = [b.num_frames(i) for i in range(len(utts))]
            outs.append(([b.coefficients(i) for i in range(len(utts))], [b.pcm(i) for i in range(len(utts))],
                         [b.first_coefficients(i) if first and n[i] else None for i in range(len(utts))]))
        trk = [b.track(i, 0) if tracks else None for i in range(len(utts))]
    for i in range(len(utts)):
        g(np.array_equal(outs[0][0][i], outs[1][0][i]) and np.array_equal(outs[0][1][i], outs[1][1][i]), what, i,
          "two runs differ")
        g(len(outs[0][1][i]) == n[i] * C.FPERIOD and np.isfinite(outs[0][1][i]).all(), what, i, "PCM length or value")
    return list(zip(outs[0][0], outs[0][2], trk))


# ---- the post-filter ---------------------------------------------------------------------------------------------------
def gate_pf_rows(g, got, ref, worst, kinds, idx, key, what):
    """Rows `idx` of a class (got [len(idx)][nmcp]) under R.within, b'[0] and b'[1:]."""
    for k, r in enumerate(idx):
        e0, e1, f0, f1 = R.pf_errors(got[k], ref[r])
        e_or = worst[C.pf_group(r, kinds)]
        _note("%s %s b'[0]" % (key, C.pf_group(r, kinds)), e0, e_or[0], f0)
        _note("%s %s b'[1:]" % (key, C.pf_group(r, kinds)), e1, e_or[1], f1)
        g(R.within(e0, e_or[0], f0), what, "row", r, kinds[r], "b'[0]: e_gpu, e_oracle, floor", e0, e_or[0], f0)
        g(R.within(e1, e_or[1], f1), what, "row", r, kinds[r], "b'[1:]: e_gpu, e_oracle, floor", e1, e_or[1], f1)


@pytest.mark.parametrize("name,beta", C.PF_TABLE, ids=["%s-b%g" % t for t in C.PF_TABLE])
def test_postfilter_through_tracks(name, beta):
    """Measured on an MI355X (profiles/coef_ref.txt): the worst e_gpu / (e_oracle + floor / 4), against the gate's 4, is
    0.24 for b'[0] on ordinary rows (e_gpu <= 3.4e-15), 0.19 for b'[1:], and 1.61 on the c0 = +-20 rows (n7_a42)."""
    nmcp, alpha, _ = C.PF_CLASSES[name]
    rows, ref = C.pf_rows(name), C.pf_reference(name, beta)
    worst = C.pf_e_oracle(name)
    utts = [track_utt(rows[:T]) for T in C.FRAMES]
    plain0 = C.mc2b_f64(rows[0], alpha)
    g = Gates()
    for label, kw in (("default", {}), ("chunk_frames=8", dict(chunk_frames=8))):
        what = (name, beta, label)
        out = run_twice(voice_of(nmcp, alpha, beta), utts, g, what, **kw)
        full = out[0][0]
        assert full.shape == (C.ROWS, nmcp) and np.isfinite(full).all(), what
        gate_pf_rows(g, full, ref["b"], worst, C.PF_KINDS, range(C.ROWS), "post-filter %s beta %g" % (name, beta), what)
        g(not full[C.ZERO_ROW].any(), what, "the all-zero row is not zero", full[C.ZERO_ROW])
        for i, T in enumerate(C.FRAMES):
            coef, first, _ = out[i]
            g(coef.shape == (T, nmcp) and np.array_equal(coef, full[:T]), what, "T =", T, "is not the long one's head")
            if T:
                g(np.array_equal(first, plain0), what, "T =", T, "first_coefficients is not mc2b of frame 0", first - plain0)
    assert not g.misses, g.misses


def test_postfilter_mixed_conditions():
    """Per-utterance alpha and beta in one batch of state-level utterances (k_postfilter's uvoc path: the search over
    frame_off, the `continue` of beta = 0 utterances, one operator per alpha), 8,213 frames, empty utterances first, in
    the middle and last.  Measured worst ratio: 0.21 on ordinary rows, 1.44 at c0 = +20 (alpha 0.55, beta 0.3)."""
    plan, rows = C.mixed_plan(), C.mixed_rows()
    utts = [state_utt(rows[idx]) for _, _, idx in plan]
    voc = [C.MIXED_CONDS[c] + (1.0,) for _, c, _ in plan]
    plain = [np.stack([C.mc2b_f64(row, a) for row in rows]) for a, _ in C.MIXED_CONDS]
    g = Gates()
    out = run_twice(voice_of(C.MIXED_NMCP, 0.55), utts, g, "mixed", tracks=True, voc=voc)
    seen = set()
    for i, (T, c, idx) in enumerate(plan):
        coef, first, track = out[i]
        alpha, beta = C.MIXED_CONDS[c]
        what = ("mixed", i, "T", T, "alpha", alpha, "beta", beta)
        assert coef.shape == (T, C.MIXED_NMCP), what
        if T == 0:
            continue
        seen.add((T, c))
        g(np.array_equal(track, rows[idx]), what, "the generated track is not the means")
        g(np.array_equal(first, plain[c][idx[0]]), what, "first_coefficients is not mc2b of frame 0")
        if beta == 0.0:
            g(np.array_equal(coef, plain[c][idx]), what, "beta = 0 is not the plain mc2b")
        else:
            ref, worst = C.mixed_reference(c)
            gate_pf_rows(g, coef, ref, worst, C.MIXED_KINDS, idx, "post-filter mixed alpha %g beta %g" % (alpha, beta), what)
    assert len(seen) == len(C.MIXED_T) * len(C.MIXED_CONDS)
    assert not g.misses, g.misses[:20]


# ---- Stage::NonZero ----------------------------------------------------------------------------------------------------
def gate_stage(g, out, idxs, ref, e_or, e_or_first, key, what):
    """The utterances `out` (row indices idxs[i]) of a class: the worst error over all rows against the oracle's worst."""
    e = e_first = 0.0
    for (coef, first, _), idx in zip(out, idxs):
        if len(idx) == 0:
            continue
        assert np.isfinite(coef).all() and np.isfinite(first).all(), what
        e = max([e] + [R.rel_inf(coef[k], ref["filtered"][r]) for k, r in enumerate(idx)])
        e_first = max(e_first, R.rel_inf(first, ref["first"][idx[0]]))
    _note(key + " filtered", e, e_or, R.STAGE_FLOOR)
    _note(key + " first frame", e_first, e_or_first, R.STAGE_FLOOR)
    g(R.within(e, e_or, R.STAGE_FLOOR), what, "filtered: e_gpu, e_oracle", e, e_or)
    g(R.within(e_first, e_or_first, R.STAGE_FLOOR), what, "first frame: e_gpu, e_oracle", e_first, e_or_first)


@pytest.mark.parametrize("name", list(C.STAGE_CLASSES))
def test_stage_coefficients_through_tracks(name):
    """Measured on an MI355X (profiles/coef_ref.txt): the worst e_gpu / (e_oracle + floor / 4), against the gate's 4, is
    1.13 (n35_s2, filtered: e_gpu 5.2e-9, e_oracle 4.6e-9); 0.2 at n = 3 and 4, where the floor is most of the bound."""
    n, stage, log_gain, alpha, beta = C.STAGE_CLASSES[name]
    rows, ref = C.stage_case(name)
    _, _, e_or, e_or_first = C.stage_oracle(name)
    idxs = C.stage_utterance_rows(rows)
    g = Gates()
    what = (name,)
    out = run_twice(voice_of(n, alpha, beta, stage, log_gain), [track_utt(rows[idx]) for idx in idxs], g, what)
    gate_stage(g, out, idxs, ref, e_or, e_or_first, "stage %s" % name, what)
    full = out[0][0]
    for i, T in enumerate(C.FRAMES):
        g(out[i][0].shape == (T, n) and np.array_equal(out[i][0], full[:T]), what, "T =", T, "is not the long one's head")
    for i, idx in enumerate(idxs[len(C.FRAMES):], len(C.FRAMES)):
        g(np.array_equal(out[i][0], full[idx]), what, "row", idx[0], "alone differs from the row in the long utterance")
    assert not g.misses, g.misses


@pytest.mark.parametrize("name", C.STAGE_MIXED)
def test_stage_coefficients_mixed_conditions(name):
    """Per-utterance alpha and beta (state-level utterances, Batch(voc=...)): two alphas, beta 0 and 0.3."""
    n, stage, log_gain, alpha, _ = C.STAGE_CLASSES[name]
    rows, _ = C.stage_case(name)
    conds = C.stage_mixed_conds(name)
    g = Gates()
    out = run_twice(voice_of(n, alpha, 0.0, stage, log_gain), [state_utt(rows)] * len(conds), g, (name, "mixed"),
                    tracks=True, voc=[c + (1.0,) for c in conds])
    for c, (a, be) in enumerate(conds):
        what = (name, "alpha", a, "beta", be)
        ref, e_or, e_or_first = C.stage_mixed_reference(name, c)
        g(np.array_equal(out[c][2], rows), what, "the generated track is not the means")
        gate_stage(g, [out[c]], [np.arange(C.ROWS)], ref, e_or, e_or_first, "stage %s alpha %g beta %g" % (name, a, be), what)
    assert not g.misses, g.misses

"""The extended-precision reference of the coefficient kernels (tests/coef_ref.py) against its closed forms and, where
mpmath imports, against 50 digits; the CPU oracle (O.postfilter_mcp, O.stage_coefficients) against that reference on
the tables of tests/coef_cases.py; and the gate of tests/test_gpu_coef_ref.py shown to bite.  No GPU.

The oracle's worst error per class and gate group is the e_oracle of the GPU gates (R.within).  Measured
(JB_COEF_REF_REPORT=<file> appends the table; profiles/coef_ref.txt): post-filter, b'[0]: 2e-16 to 5e-15 on ordinary
rows, up to 1e-10 at c0 = +20 (tests/coef_cases.py says why); b'[1:]: <= 1.6e-16.  Stage: 4e-16 at n = 3 and 4, 3e-15
at 9, 2e-14 at 12 and 13, 2e-9 to 6e-9 at 34 and 35; long double is 1/1500 of that or closer to the 50-digit run.  Not
gated, recorded: on an even grid the f64 conversion is 5e-6 off at n = 48, 2e-3 at 61 and 2e-2 at 64 (the kernels
take nmcp <= 64)."""
import os
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import coef_cases as C
from tests import coef_ref as R

pytestmark = pytest.mark.skipif(not R.wide_enough(), reason="numpy.longdouble is no wider than f64 here")

_lines = []


@pytest.fixture(scope="module", autouse=True)
def report():
    _t0 = time.time()
    yield
    path = os.environ.get("JB_COEF_REF_REPORT")
    if path and _lines:
        with open(path, "a") as fh:
            fh.write("CPU oracle against the extended-precision reference (tests/test_coef_ref.py), %.1f s for the file\n"
                     % (time.time() - _t0))
            fh.write("\n".join(_lines) + "\n\n")


# ---- the reference against its closed forms -------------------------------------------------------------------------
# the closed form's own error is about eps (n + log2 N) of the largest |G| (|exp(G)|) on the circle (closed_form_ir's
# `noise`: the Horner steps and the transform, in long double); the gate is 16 times that
@pytest.mark.parametrize("nmcp,alpha", [(35, 0.55), (64, 0.77), (9, -0.3), (5, 0.0), (3, 0.55), (4, 0.42)])
def test_freqt_and_c2ir_against_taylor_coefficients(nmcp, alpha):
    rng = np.random.default_rng(3 + nmcp)
    mc = rng.normal(size=nmcp) * 0.3
    mc[0] = 1.3
    for a in (-alpha, alpha):  # b2en passes -alpha
        g = R.freqt_operator(nmcp, a) @ mc.astype(R.LD)
        ir = R.c2ir(g)
        g_cf, ir_cf, noise = R.closed_form_ir(mc, a)
        eg, ei = float(np.abs(g_cf - g).max()), float(np.abs(ir_cf - ir).max())
        print(nmcp, a, "freqt against the closed form", eg, "of", noise[0], "c2ir", ei, "of", noise[1])
        assert eg <= 16 * noise[0] and ei <= 16 * noise[1], (nmcp, a, eg, ei, noise)
        # ... which is a check worth having: far below the coefficients themselves
        assert 16 * noise[0] <= 1e-12 * np.abs(g).max() and 16 * noise[1] <= 1e-9 * np.abs(ir).max()


def test_freqt_operator_is_the_recurrence_on_a_row():
    """The cached operator against cepstrum.rs:153-173 run on one vector, and linearity used rightly."""
    nmcp, a = 7, -0.42
    c = C.pf_rows("n7_a42")[3].astype(R.LD)
    g, aa = np.zeros(R.IRLENG, dtype=R.LD), 1 - R.LD(a) * R.LD(a)
    for x in c:
        f = g.copy()
        g[0] = x + R.LD(a) * f[0]
        g[1] = aa * f[0] + R.LD(a) * f[1]
        for j in range(2, R.IRLENG):
            g[j] = f[j - 1] + R.LD(a) * (f[j] - g[j - 1])
    assert float(np.abs(R.freqt_operator(nmcp, a) @ c - g).max()) <= 2.0 ** -60 * float(np.abs(g).max())


def test_postfilter_energy_against_parseval():
    """Where the response has died out before 576 samples, b2en is the whole energy: the mean of |exp(C)|^2 over the
    circle (tests/mlsa_ref.py reversed_energy, no recursion at all)."""
    for name in ("n3_a55", "n4_a0"):
        nmcp, alpha, _ = C.PF_CLASSES[name]
        for row in C.pf_rows(name)[:4]:
            b = R.M.mc2b(row, alpha)
            ir = R.impulse_response(b, alpha)
            assert R.tail_over_peak(ir) <= 1e-20
            e, want = np.sum(ir * ir), R.M.reversed_energy(b, alpha, 4096)
            assert abs(e / want - 1) <= 2.0 ** -55, (name, float(e / want - 1))


@pytest.mark.parametrize("name", list(C.STAGE_CLASSES))
def test_lsp2lpc_against_its_factors(name):
    """The recursion of lsp.rs:27-91 against the product of its second-order sections, even and odd m, in long double.
    Both sides round, and the partial products reach 1e7 times the result at n = 35 before they cancel; what that
    costs is read off the same recursion in f64 (O.lsp2lpc) and scaled by the formats' ratio eps / 2u, times 64 for the
    two sides' independent rounding and the multiplied-out product's own growth, plus 64 eps.  (At 50 digits, below,
    the two agree to 1e-38.)"""
    rows, _ = C.stage_case(name)
    eps = float(np.finfo(R.LD).eps)
    for row in rows:
        l = [R.LD(x) for x in row]
        rec = R.as_ld(R.lsp2lpc(l, R.LDK))
        e = R.rel_inf(R.as_ld(R.lsp2lpc_closed(l, R.LDK)), rec)
        e_f64 = R.rel_inf(O.lsp2lpc(row), rec)
        assert e <= 64 * eps + 64 * e_f64 * eps / (2 * R.U), (name, e, e_f64)


def test_lsp2lpc_against_its_factors_at_50_digits():
    pytest.importorskip("mpmath")
    K = R.mp_kit()
    for name in ("n4_s4_log", "n12_s2_log", "n13_s2_log", "n34_s2_log", "n35_s2"):
        for row in C.stage_case(name)[0][::5]:
            l = [K.c(float(x)) for x in row]
            a, b = R.lsp2lpc(l, K), R.lsp2lpc_closed(l, K)
            assert max(abs(x - y) for x, y in zip(a, b)) <= 1e-38 * max(abs(y) for y in b), name


# ---- long double against 50 digits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.STAGE_CLASSES))
def test_long_double_within_a_64th_of_the_oracles_distance(name):
    """The builder's last condition: the long-double reference is at most 1/64 as far from the 50-digit run as the
    oracle is, so gating on it measures f64 arithmetic; and both take the same branches of check_lsp_stability."""
    pytest.importorskip("mpmath")
    K = R.mp_kit()
    n, stage, log_gain, alpha, beta = C.STAGE_CLASSES[name]
    rows, ref = C.stage_case(name)
    orc = C.stage_oracle(name)
    e_ld = e_or = 0.0
    for r, row in enumerate(rows):
        for filtered, ld, o in ((True, ref["filtered"][r], orc[0][r]), (False, ref["first"][r], orc[1][r])):
            want, tr = R.stage_coefficients(row, alpha, beta, log_gain, stage, K, filtered=filtered)
            e_ld, e_or = max(e_ld, R.rel_inf_kit(ld, want, K)), max(e_or, R.rel_inf_kit(o, want, K))
            if filtered:
                assert R.decisive(tr, C.TIE_MARGIN) == R.decisive(ref["trace"][r], C.TIE_MARGIN), (name, r)
    _lines.append("stage %-12s long double against 50 digits %.2e, oracle %.2e: 1/%.0f" % (name, e_ld, e_or, e_or / e_ld))
    assert e_ld <= e_or / 64.0, (name, e_ld, e_or)


def test_the_boundary_is_recorded():
    """n = 48, 61, 64 on a jittered even grid: what the f64 conversion keeps.  Recorded, not gated."""
    pytest.importorskip("mpmath")
    K = R.mp_kit()
    for n in (35, 48, 61, 64):
        rng = np.random.default_rng(n)
        row = C._lsp_row(rng, n, "grid")
        got = O.stage_coefficients(row, 0.55, 0.0, False, 2)
        want, _ = R.stage_coefficients(row, 0.55, 0.0, False, 2, K)
        ld, _ = R.stage_coefficients(row, 0.55, 0.0, False, 2)
        e, eld = R.rel_inf_kit(got, want, K), R.rel_inf_kit(ld, want, K)
        _lines.append("boundary n = %d (2 stages, alpha 0.55, even grid): oracle against 50 digits %.1e, long double %.1e"
                      % (n, e, eld))
        assert np.isfinite(e)


# ---- the oracle against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,beta", C.PF_TABLE, ids=["%s-b%g" % t for t in C.PF_TABLE])
def test_oracle_postfilter_against_reference(name, beta):
    """O.postfilter_mcp (with the vocoder's mc2b behind it) on the class.  b'[1:] is one multiplication and the b2mc /
    mc2b round trip, whose recursion damps its own rounding by |alpha| a step: 16 u max|b'|.  The shift is half the log
    of a ratio of two sums of 576 squares, each term the end of a convolution recursion of up to 575 products: 576 u
    where nothing cancels, which is so on the ordinary rows; at c0 = +-20 it is not (tests/coef_cases.py) and the figure
    is recorded only.  The all-zero row stays exactly zero."""
    nmcp, alpha, _ = C.PF_CLASSES[name]
    ref = C.pf_reference(name, beta)
    got, worst = C.pf_oracle(name, beta)
    assert not got[C.ZERO_ROW].any()
    for r in range(C.ROWS):
        e0, e1, f0, f1 = R.pf_errors(got[r], ref["b"][r])
        assert e1 <= f1, (name, beta, r, e1, f1)
        if C.pf_group(r) == "ordinary":
            assert e0 <= 576 * R.U + f0, (name, beta, r, e0)
        # (O.b2en itself: the two energies)
    _lines.append("post-filter %-8s beta %-6g oracle b'[0] %.2e (c0 = +-20: %.2e)  b'[1:] %.2e  tail/peak %.1e" % (
        name, beta, worst["ordinary"][0], worst["c0_20"][0], max(w[1] for w in worst.values()), ref["tail"].max()))


def test_oracle_b2en_against_reference():
    """O.b2en alone against the reference's energy, relative: 576 u as above."""
    for name in ("n7_a42", "n35_a55", "n64_a77"):
        nmcp, alpha, _ = C.PF_CLASSES[name]
        for r, row in enumerate(C.pf_rows(name)):
            if C.pf_group(r) != "ordinary":
                continue
            b = C.mc2b_f64(row, alpha)
            ir = R.impulse_response(b, alpha)
            want = np.sum(ir * ir)
            assert abs(R.LD(O.b2en(b, alpha)) / want - 1) <= 576 * R.U, (name, r)


@pytest.mark.parametrize("name", list(C.STAGE_CLASSES))
def test_oracle_stage_against_reference(name):
    """O.stage_coefficients on the class, both conversions.  The conversion loses digits in its own recursions (the
    sections' partial products cancel; a change of u in every input moves the result by 1e4 u at n = 35, the f64
    conversion is 1e7 u off), so the scale of a correct f64 restatement's error is taken from the format: the
    reference's own text run in f64 (R.F64K).  The oracle passes the gate the kernels get, against that."""
    n, stage, log_gain, alpha, beta = C.STAGE_CLASSES[name]
    rows, ref = C.stage_case(name)
    f, f0, e, e0 = C.stage_oracle(name)
    k = k0 = 0.0
    for r, row in enumerate(rows):
        assert row[0] < row[1], (name, r, "the gain slot is not below the first frequency")
        out, tr = R.stage_coefficients(row, alpha, beta, log_gain, stage, R.F64K)
        assert R.decisive(tr, C.TIE_MARGIN) == R.decisive(ref["trace"][r], C.TIE_MARGIN), (name, r)
        out0, _ = R.stage_coefficients(row, alpha, beta, log_gain, stage, R.F64K, filtered=False)
        k, k0 = max(k, R.rel_inf(out, ref["filtered"][r])), max(k0, R.rel_inf(out0, ref["first"][r]))
    _lines.append("stage %-12s oracle filtered %.2e  first %.2e  (the reference's text in f64: %.2e, %.2e)" % (name, e, e0, k, k0))
    assert R.within(e, k, R.STAGE_FLOOR) and R.within(e0, k0, R.STAGE_FLOOR), (name, e, k, e0, k0)


# ---- the tables -----------------------------------------------------------------------------------------------------
def test_tables_cover_what_they_say():
    small = {b for name, b in C.PF_TABLE if C.PF_CLASSES[name][0] <= 7}
    large = {b for name, b in C.PF_TABLE if C.PF_CLASSES[name][0] >= 35}
    assert small == large == {1e-6, 0.1, 0.3, 1.0}
    assert {(v[0], v[1]) for v in C.PF_CLASSES.values()} == {(3, .55), (4, 0), (7, .42), (25, .42), (35, .55), (35, 0),
                                                              (63, .55), (64, .55), (64, .77), (9, -0.3)}
    assert len(C.PF_KINDS) == len(C.STAGE_KINDS) == C.ROWS
    plan = C.mixed_plan()
    assert sum(p[0] for p in plan) >= C.MIXED_MIN_FRAMES
    assert plan[0][0] == 0 and plan[-1][0] == 0 and any(p[0] == 0 for p in plan[len(plan) // 3:2 * len(plan) // 3])
    assert {p[0] for p in plan} == {0, 1, 2, 7, 33}
    for c in range(len(C.MIXED_CONDS)):
        C.mixed_reference(c)  # (asserts the energies' range)
    assert {v[0] % 2 for v in C.STAGE_CLASSES.values()} == {0, 1}
    for name in C.STAGE_MIXED:
        for c in range(4):
            C.stage_mixed_reference(name, c)  # (asserts the margins under the other alpha and beta)


# ---- the gate bites -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,beta", [("n3_a55", 0.3), ("n7_a42", 1.0), ("n35_a55", 0.3), ("n64_a55", 1e-6)])
def test_gate_fails_a_gain_moved_by_1e_13(name, beta):
    ref = C.pf_reference(name, beta)
    got, e_or = C.pf_oracle(name, beta)[0], C.pf_e_oracle(name)["ordinary"]
    for r in range(C.ROWS):
        if C.pf_group(r) != "ordinary":
            continue
        e0, e1, f0, f1 = R.pf_errors(got[r], ref["b"][r])
        assert R.within(e0, e_or[0], f0) and R.within(e1, e_or[1], f1)  # the oracle passes its own gate
        moved = np.array(ref["b"][r])
        moved[0] += R.LD(1e-13)
        e0, e1, f0, f1 = R.pf_errors(moved, ref["b"][r])
        assert not R.within(e0, e_or[0], f0), (name, r, e0, e_or[0], f0)
        assert R.within(e1, e_or[1], f1)


@pytest.mark.parametrize("name", ["n12_s2_log", "n35_s2", "n34_s2_log"])
def test_gate_fails_a_swapped_branch_and_exchanged_p_q(name):
    n, stage, log_gain, alpha, beta = C.STAGE_CLASSES[name]
    rows, ref = C.stage_case(name)
    e_or = C.stage_oracle(name)[2]
    r = len(C.STAGE_KINDS) - 1  # a bunch of six: check_lsp_stability is still moving it in its fourth pass
    cmp = ref["trace"][r]["cmp"]
    k = max(i for i, (p, kind, _, fired, margin) in enumerate(cmp) if p == 3 and fired and margin >= 1e-6)
    same, _ = R.stage_coefficients(rows[r], alpha, beta, log_gain, stage)
    assert R.within(R.rel_inf(R.as_ld(same), ref["filtered"][r]), e_or, R.STAGE_FLOOR)
    flipped, _ = R.stage_coefficients(rows[r], alpha, beta, log_gain, stage, flip=k)
    e = R.rel_inf(R.as_ld(flipped), ref["filtered"][r])
    assert not R.within(e, e_or, R.STAGE_FLOOR), (name, "a swapped stability branch passes", e, e_or)
    for r in (0, 5):
        swapped, _ = R.stage_coefficients(rows[r], alpha, beta, log_gain, stage, swap_pq=True)
        e = R.rel_inf(R.as_ld(swapped), ref["filtered"][r])
        assert not R.within(e, e_or, R.STAGE_FLOOR), (name, "p and q exchanged passes", e, e_or)

"""The CPU oracle's parameter generation against the dense extended-precision reference (tests/mlpg_ref.py) on the
whole case table (tests/mlpg_cases.py): this pins the oracle where no golden of the reference does -- windows of 5, 7
and 9 taps, mixed and even widths, zero taps, two and four windows, MSD streams of more than one dimension.  No GPU.

Gates (u = 2^-53):
  * NODATA mask identical;
  * without GV, backward error <= 32 u: the textbook bound of a band Cholesky / LDL' of half-bandwidth p <= 4 is of
    order (3p + 4) u, 32 u is twice that.  A wrong tap, sign, boundary flag or index gives >= 1e-3;
  * without GV, forward error ||c - x||inf <= 64 cond_inf(A) u ||x||inf;
  * with GV, the conditions on the inputs that make the GPU test's GV gate sound: cond_inf(A) <= 1e8, at least three
    switched-on voiced frames with distinct means wherever GV acts, min |obj_i - obj_(i-1)| / |obj_i| >= 1e-9 (the
    ascent's step-size branch cannot differ between two f64 evaluations), the oracle's deviation from the dense
    long-double ascent <= 1e-9 relative;
  * with time-parallel GV (the [dim][frame] path), the oracle's own elementwise error at most half of the project's
    contract for those sums, rtol 1e-12 / atol 1e-13: two f64 evaluations within e of the exact result differ by up
    to 2 e, so only such a case can hold a kernel to that contract (tests/mlpg_cases.py: how the inputs meet it).

JB_MLPG_DENSE_REPORT=<file> appends the measured worst values per window set (profiles/r13_mlpg_dense.txt holds them)."""
import os
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import mlpg_cases as C
from tests import mlpg_ref as R

BACKWARD_GATE = 32 * R.U
FORWARD_FACTOR = 64
COND_MAX = 1e8
OBJ_MARGIN_MIN = 1e-9
GV_ORACLE_DEV_MAX = 1e-9
TP_ORACLE_SHARE_MAX = 0.5  # of atol 1e-13 + rtol 1e-12 |x|, elementwise

_worst = {}  # window set -> dict of worst measured values
_t0 = time.time()


def _note(wset, **kw):
    w = _worst.setdefault(wset, dict(systems=0, backward_u=0.0, forward_cond_u=0.0, cond=0.0, gv_dev=0.0,
                                     obj_margin=float("inf"), tp_share=0.0))
    for k, v in kw.items():
        w[k] = w[k] + v if k == "systems" else min(w[k], v) if k == "obj_margin" else max(w[k], v)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    path = os.environ.get("JB_MLPG_DENSE_REPORT")
    if path and _worst:
        with open(path, "a") as fh:
            fh.write("oracle against the dense reference (tests/test_mlpg_dense.py), %.1f s for the file\n" % (time.time() - _t0))
            fh.write("%-22s %8s %12s %16s %10s %12s %12s %18s\n" % ("window set", "systems", "backward/u", "forward/(cond u)",
                                                                  "cond_inf", "GV deviation", "min dobj/obj", "err / tp contract"))
            for wset, w in _worst.items():
                fh.write("%-22s %8d %12.2f %16.2f %10.2e %12.2e %12.2e %18.3f\n" % (
                    wset, w["systems"], w["backward_u"], w["forward_cond_u"], w["cond"], w["gv_dev"], w["obj_margin"],
                    w["tp_share"]))


def test_long_double_is_wider_than_f64():
    """The reference has to carry more digits than the arithmetic it judges (x87 extended: eps 1.08e-19)."""
    assert np.finfo(R.LD).eps <= 2.0 ** -63


def test_boundary_distances_against_a_walk():
    rng = np.random.default_rng(1)
    for _ in range(50):
        m = rng.random(int(rng.integers(0, 40))) < 0.6
        left, right = R.boundary_distances(m)
        for t in range(len(m)):
            a = b = t
            while m[t] and a > 0 and m[a - 1]:
                a -= 1
            while m[t] and b + 1 < len(m) and m[b + 1]:
                b += 1
            assert (left[t], right[t]) == (t - a, b - t)
        ol, orr = O.boundary_distances(m.astype(np.uint8))
        assert np.array_equal(ol, left) and np.array_equal(orr, right)


def test_reference_pieces():
    """The row-wise form of W' diag(ivar) W equals the literal matrix product; solve() leaves a residual at the level
    of long double; window_matrix puts tap k of a window of declared width w at column tau + k - w // 2."""
    rng = np.random.default_rng(2)
    for coef in ([1.0], [-0.5, 0.0, 0.5], [-1.0, 1.0], [0.25, -0.5, -0.25, 0.5], [0, 0, -0.5, 0, 0.5, 0, 0]):
        for N in (1, 2, 3, 7, 12):
            Wm = R.window_matrix(coef, N)
            iv, mu = rng.uniform(1.0, 1e3, N).astype(R.LD), rng.standard_normal(N).astype(R.LD)
            A1, b1 = R.normal_equations(Wm, iv, mu, sparse=True)
            A2, b2 = R.normal_equations(Wm, iv, mu, sparse=False)
            assert float(np.abs(A1 - A2).max()) <= 4 * float(np.finfo(R.LD).eps) * float(np.abs(A2).max() + 1)
            assert float(np.abs(b1 - b2).max()) <= 4 * float(np.finfo(R.LD).eps) * float(np.abs(b2).max() + 1)
    Wm = R.window_matrix([0.25, -0.5, -0.25, 0.5], 5)  # even width 4: lw = 2, rw = 1
    assert [float(x) for x in Wm[2]] == [0.25, -0.5, -0.25, 0.5, 0.0]
    assert [float(x) for x in Wm[0]] == [-0.25, 0.5, 0.0, 0.0, 0.0]
    M = rng.standard_normal((30, 30)).astype(R.LD)
    A = M @ M.T + 30 * np.eye(30, dtype=R.LD)
    b = rng.standard_normal(30).astype(R.LD)
    assert R.backward_error(A, b, R.solve(A, b)) <= 64 * float(np.finfo(R.LD).eps)
    assert R.backward_error(A, b, A @ np.zeros(30, R.LD)) > 0.1 and R.backward_error(A, A @ b, b) <= 1e-17


def check_inputs(case):
    """The conditions on the inputs that do not need a solve."""
    for u in case.utts:
        s = u.stream
        assert s.var.min() >= 1e-3 and s.var.max() <= 1.0
        assert len(s.windows[0]) == 1
        if not s.use_gv:
            continue
        on = np.repeat(s.gv_switch.astype(bool), u.durations) & R.voiced_mask(s, u.durations)
        states = np.unique(np.repeat(np.arange(len(u.durations)), u.durations)[on])
        if len(states) == 0:
            continue  # gv_length = 0: no GV for this utterance
        for d in range(s.L):
            assert len(np.unique(s.mean[states, d])) >= 3, (case.name, u.name, d)


@pytest.mark.parametrize("wset,shape,use_gv", C.TABLE, ids=["%s-%s-%s" % (w, s, "gv" if g else "nogv") for w, s, g in C.TABLE])
def test_oracle_against_dense(wset, shape, use_gv):
    case = C.build_case(wset, shape, use_gv)
    check_inputs(case)
    some_gv = False
    for i, u in enumerate(case.utts):
        d = C.dense(wset, shape, use_gv, i)
        got = C.oracle_track(case, i)
        what = (case.name, u.name)
        mask = R.voiced_mask(u.stream, u.durations)
        assert got.shape == (len(mask), case.L)
        assert np.array_equal(got != R.NODATA, np.repeat(mask[:, None], case.L, axis=1)), what
        for k, dim in enumerate(d["dims"]):
            A, b = d["systems"][k]
            if len(b) == 0:
                continue
            c = got[d["vidx"], dim]
            assert d["cond"][k] <= COND_MAX, what
            _note(wset, systems=1, cond=d["cond"][k])
            acts = use_gv and bool(R.gv_switch_frames(u.stream, u.durations, d["vidx"]).any())
            if C.time_parallel_gv(case.windows, case.L, use_gv):
                x = np.asarray(d["par"][k], dtype=np.float64)
                share = float((np.abs(c - x) / (1e-13 + 1e-12 * np.abs(x))).max())
                _note(wset, tp_share=share)
                assert share <= TP_ORACLE_SHARE_MAX, (what, dim, share)
            if not acts:  # the solve itself (a GV-on case reaches it where every switch is off)
                be = R.backward_error(A, b, c)
                fe = R.rel_inf(c, d["x"][k]) / (d["cond"][k] * R.U)
                _note(wset, backward_u=be / R.U, forward_cond_u=fe)
                assert be <= BACKWARD_GATE, (what, dim, be / R.U)
                assert fe <= FORWARD_FACTOR, (what, dim, fe)
            else:
                some_gv = True
                dev = R.rel_inf(c, d["par"][k])
                _note(wset, gv_dev=dev, obj_margin=d["margin"][k])
                assert d["margin"][k] >= OBJ_MARGIN_MIN, (what, dim, d["margin"][k])
                assert dev <= GV_ORACLE_DEV_MAX, (what, dim, dev)
    assert some_gv == use_gv, case.name
    print(case.name, _worst[wset])


def test_table_covers_what_it_says():
    """Every window set and every stream shape with GV on, off and gv_weight 0.7; the three switch patterns; the
    lengths shorter than the widest window; more voiced runs than a wave has lanes."""
    assert {w for w, _, _ in C.TABLE} == set(C.WINDOW_SETS)
    for shape in C.SHAPES:
        assert {g for w, s, g in C.TABLE if s == shape and w == "nitech_1_3_3"} == {True, False}
        assert len({w for w, s, _ in C.TABLE if s == shape and C.band_width(C.WINDOW_SETS[w]) > 3}) >= 2, shape
    case = C.build_case("nitech_1_3_3", "L1_msd", True)
    assert {u.stream.gv_weight for u in case.utts} == {1.0, 0.7}
    frac = [u.stream.gv_switch.mean() for u in case.utts]
    assert 0.0 in frac and 1.0 in frac and any(0.5 < f < 0.9 for f in frac)
    runs = {u.name: int((np.diff(np.concatenate(([0], R.voiced_mask(u.stream, u.durations).astype(int)))) == 1).sum())
            for u in case.utts}
    assert runs["70_runs_of_one"] == 70 and runs["none_voiced"] == 0 and runs["runs_1_to_17"] == 13
    assert [int(u.durations.sum()) for u in C.build_case("1_9_9", "L4", True).utts[:9]] == [1, 2, 3, 4, 5, 8, 9, 10, 15]
    long = C.long_msd_case().utts[0]
    assert int(R.voiced_mask(long.stream, long.durations).sum()) == 2055 and 2500 <= int(long.durations.sum()) <= 2700


def test_static_window_of_three_taps_is_the_reference_s_own():
    """A FIRST (static) window wider than one tap is where the reference is not the normal equations.  In
    calc_wuw_and_wum the `break` of mlpg.rs:48-56 sits inside a reversed iteration over the taps: near the end of the
    sequence it leaves the loop at the first tap past the end and with it drops the terms that are in range.  For a
    dynamic window those carry a zeroed inverse variance (mod.rs:74) and nothing is lost; the first window is never
    zeroed.  With [[0.1, 0.8, 0.1]] at T = 1 the diagonal entry 0.8 * 0.8 / var is dropped: the oracle, which restates
    the loop as it stands, divides by zero, where the normal equations give mu / 0.8.  The product's parity target is
    the reference, quirk included (tests/test_gpu_mlpg_dense.py compares these window sets with the oracle).  A
    two-tap static window [0.2, 0.8] has no tap past the end at the last frame and agrees."""
    mean, var = np.array([[1.5]]), np.array([[0.25]])
    s3 = R.Stream(1, [[0.1, 0.8, 0.1]], mean, var)
    got = C.oracle_track(C.Case("quirk3", "T1", False, s3.windows, 1, False, [C.Utt("T1", np.array([1], np.uint32), s3)]), 0)
    assert np.isinf(got[0, 0])
    _, [(A, b)] = R.dense_system(s3, [1])
    assert abs(float(R.solve(A, b)[0]) - 1.5 / 0.8) <= 1e-15
    rng = np.random.default_rng(3)
    for T in (1, 2, 5):
        s2 = R.Stream(1, [[0.2, 0.8], [-0.5, 0.0, 0.5]], rng.standard_normal((T, 2)), rng.uniform(0.1, 1.0, (T, 2)))
        dur = np.ones(T, np.uint32)
        got = C.oracle_track(C.Case("quirk2", "T%d" % T, False, s2.windows, 1, False, [C.Utt("T", dur, s2)]), 0)
        _, [(A, b)] = R.dense_system(s2, dur)
        assert R.backward_error(A, b, got[:, 0]) <= BACKWARD_GATE

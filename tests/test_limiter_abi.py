"""The limiter without a GPU: the struct layouts, the smoothing window, every refusal, and the host seam
(jb_limiter_host) against the numpy statement of the rule in tests/limiter_ref.py on the edge shapes both test files
share: agreement within 1e-12 of the ceiling, the exact sample-peak bound, untouched samples bit for bit, the report,
the 16-bit form, and the true peak of limited white noise."""
import ctypes as C
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from tests import limiter_ref as R

INVALID, UNSUPPORTED, BUFFER = -1, -2, -8  # JB_ERR_*
CASES = R.cases()
IDS = [c[0] for c in CASES]


def opts_of(case):
    o = case[4]
    return J.limiter() if o is None else J.limiter(lookahead_ms=o[0], hold_ms=o[1])


def ref_of(case, true_peak):
    _, x, hz, g, o = case
    kw = {} if o is None else {"lookahead_ms": o[0], "hold_ms": o[1]}
    return R.limit(x, hz, g, R.CEILING, true_peak, **kw)


def test_layouts():
    assert C.sizeof(F.LimiterOpts) == 32 and F.LimiterOpts.max_reduction_db.offset == 16
    assert F.LimiterOpts.flags.offset == 24 and F.LimiterOpts.reserved.offset == 28
    assert C.sizeof(F.LimiterReport) == 24 and F.LimiterReport.limited_samples.offset == 8
    assert F.LimiterReport.lookahead.offset == 16 and F.LimiterReport.hold.offset == 20


@pytest.mark.parametrize("hz", [8000, 16000, 22050, 48000])
def test_window_sums_to_one_and_is_symmetric(hz):
    """w is rounded once from extended precision: each entry within half an ulp of its own size of the reference, the
    sum of all within 1 ulp of 1."""
    for la in (0.05, 2.0, 3.3, 10.0):
        L, H, w = J.limiter_window(hz, J.limiter(lookahead_ms=la, hold_ms=8.0))
        assert (L, H) == R.geometry(hz, la, 8.0)
        assert w.size == L + 1 and np.all(w > 0)
        assert np.array_equal(w, w[::-1])
        assert abs(math.fsum(w) - 1.0) <= np.spacing(1.0)
        want = R.window(L)
        assert np.max(np.abs(w.astype(np.longdouble) - want) / want) <= 2.0 ** -52
    L, H, w = J.limiter_window(hz)  # the defaults: 2 ms, 8 ms
    assert (L, H) == R.geometry(hz)


def refused(opts, code=INVALID, hz=16000):
    with pytest.raises(J.JbError) as e:
        J.limiter_window(hz, opts)
    assert e.value.code == code
    return str(e.value)


def test_refusals_name_the_field():
    nan, inf = float("nan"), float("inf")
    assert "lookahead_ms" in refused(J.limiter(lookahead_ms=0.0))
    assert "lookahead_ms" in refused(J.limiter(lookahead_ms=-1.0))
    assert "lookahead_ms" in refused(J.limiter(lookahead_ms=10.001))
    assert "lookahead_ms" in refused(J.limiter(lookahead_ms=nan))
    assert "hold_ms" in refused(J.limiter(hold_ms=-0.1))
    assert "hold_ms" in refused(J.limiter(hold_ms=50.5))
    assert "hold_ms" in refused(J.limiter(hold_ms=inf))
    assert "max_reduction_db" in refused(J.limiter(max_reduction_db=-0.5))
    assert "max_reduction_db" in refused(J.limiter(max_reduction_db=24.5))
    assert "max_reduction_db" in refused(J.limiter(max_reduction_db=nan))
    assert "flags" in refused(F.LimiterOpts(2.0, 8.0, 6.0, 4, 0))
    assert "reserved" in refused(F.LimiterOpts(2.0, 8.0, 6.0, 0, 1))
    assert "0 Hz" in refused(J.limiter(), hz=0)
    # the ends of the ranges are inside
    J.limiter_window(16000, J.limiter(lookahead_ms=10.0, hold_ms=50.0, max_reduction_db=24.0))
    J.limiter_window(16000, J.limiter(hold_ms=0.0, max_reduction_db=0.0))
    # zeros without JB_LIMITER_EXACT are the defaults
    assert J.limiter_window(16000, F.LimiterOpts())[:2] == (32, 128)


def test_span_2048_runs_and_2049_is_unsupported():
    assert J.limiter_window(48000, J.limiter(lookahead_ms=10.0, hold_ms=1088 / 48.0))[:2] == (480, 1088)
    msg = refused(J.limiter(lookahead_ms=10.0, hold_ms=1089 / 48.0), UNSUPPORTED, hz=48000)
    assert "2048" in msg
    with pytest.raises(J.JbError) as e:
        J.limiter_host(np.zeros(8), 48000, 1.0, -1.0, 0, J.limiter(lookahead_ms=10.0, hold_ms=1089 / 48.0))
    assert e.value.code == UNSUPPORTED


def test_host_seam_refusals():
    x = np.zeros(4)
    with pytest.raises(J.JbError) as e:
        J.limiter_host(x, 16000, 1.0, -1.0, 2)
    assert e.value.code == INVALID and "mode" in str(e.value)
    with pytest.raises(J.JbError) as e:
        J.limiter_host(x, 16000, 1.0, -1.0, 0, J.limiter(hold_ms=51.0))
    assert "hold_ms" in str(e.value)
    L = F.lib()
    w = (C.c_double * 4)()
    assert L.jb_limiter_window(16000, None, None, None, w, 4) == BUFFER
    assert L.jb_limiter_host(None, 4, 16000, 1.0, -1.0, 0, None, None, None) == INVALID
    y, rep = J.limiter_host(np.zeros(0), 16000, 1.0, -1.0)  # no samples: nothing to do
    assert y.size == 0 and rep["limited_samples"] == 0 and rep["max_reduction_db"] == 0.0


@pytest.mark.parametrize("true_peak", [False, True], ids=["sample", "true"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_seam_follows_the_rule(case, true_peak):
    """Against the long-double statement within 1e-12 of c (the seam's FMA chain against a long-double dot product);
    |y| <= c exactly; y = x g bit for bit wherever no over-ceiling detector value is in reach; the report's fields."""
    name, x, hz, g, _ = case
    want, a, d, c, L, H = ref_of(case, true_peak)
    y, rep = J.limiter_host(x, hz, g, R.CEILING, int(true_peak), opts_of(case))
    err = np.max(np.abs(y.astype(np.longdouble) - want))
    print(name, "true" if true_peak else "sample", "err / c = %.3e" % float(err / c))
    assert err <= 1e-12 * c
    assert np.max(np.abs(y)) <= c
    assert (d > c).any(), "every case has something to limit"
    if name == "long_run":  # a run of over-ceiling samples longer than the tile and its halo
        assert R.longest_run(d > c) >= R.TILE + 2 * L + H
    mask = R.reach(d, c, L, H)
    u = x * np.float64(g)
    assert np.array_equal(y[~mask], u[~mask])
    assert (rep["lookahead"], rep["hold"]) == (L, H)
    assert rep["limited_samples"] == int(mask.sum())
    assert abs(rep["max_reduction_db"] - float(-20.0 * np.log10(a.min()))) <= 1e-9
    y16, rep16 = J.limiter_host(x, hz, g, R.CEILING, int(true_peak), opts_of(case), i16=True)
    assert np.array_equal(y16, np.trunc(np.clip(y, -32768.0, 32767.0)).astype(np.int16)) and rep16 == rep


def test_under_the_ceiling_nothing_changes():
    """A gain that puts the highest peak at the ceiling (what max_reduction_db = 0 asks of the gain rule): a = 1."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal(3000) * 4000.0
    c = 32768.0 * 10.0 ** (R.CEILING / 20.0)
    g = c / np.abs(x).max() * (1.0 - 1e-12)
    for o in (J.limiter(), J.limiter(max_reduction_db=0.0), J.no_limiter()):
        y, rep = J.limiter_host(x, 16000, g, R.CEILING, 0, o)
        assert np.array_equal(y, x * g) and rep["limited_samples"] == 0 and rep["max_reduction_db"] == 0.0
    y, rep = J.limiter_host(x, 16000, 2.0 * g, float("inf"), 0)  # no ceiling: nothing to hold
    assert np.array_equal(y, x * (2.0 * g)) and rep["limited_samples"] == 0
    y, rep = J.limiter_host(x, 16000, 2.0 * g, R.CEILING, 0, J.no_limiter())  # JB_LIMITER_OFF: the plain product
    assert np.array_equal(y, x * (2.0 * g)) and rep["limited_samples"] == 0
    # ... whose values are not read: no geometry, so no rate is refused (the defaults do not fit 192 kHz)
    y, rep = J.limiter_host(x, 192000, 2.0 * g, R.CEILING, 0, J.no_limiter())
    assert np.array_equal(y, x * (2.0 * g)) and (rep["lookahead"], rep["hold"]) == (0, 0)
    with pytest.raises(J.JbError) as e:
        J.limiter_host(x, 192000, 2.0 * g, R.CEILING, 0, J.limiter())
    assert e.value.code == UNSUPPORTED
    # the seam takes the gain as given and does not read max_reduction_db: over the ceiling it limits, depth 0 or not
    y0, rep0 = J.limiter_host(x, 16000, 2.0 * g, R.CEILING, 0, J.limiter(max_reduction_db=0.0))
    y6, rep6 = J.limiter_host(x, 16000, 2.0 * g, R.CEILING, 0, J.limiter(max_reduction_db=6.0))
    assert np.array_equal(y0, y6) and rep0 == rep6 and rep0["limited_samples"] > 0 and np.max(np.abs(y0)) <= c


@pytest.mark.parametrize("hz", [16000, 48000])
def test_true_peak_of_limited_white_noise(hz):
    """White noise driven 7 dB over a -1 dBTP ceiling: with the true-peak detector the output's true peak stays within
    0.01 dB of the ceiling (the rule bounds the inter-sample peaks of u, not of y: reported, not guaranteed); with the
    sample detector the same input overshoots by more than 1 dB."""
    rng = np.random.default_rng(hz)
    x = rng.standard_normal(4 * hz // 10)
    c = 32768.0 * 10.0 ** (R.CEILING / 20.0)
    x *= c * 10.0 ** (7.0 / 20.0) / R.true_peak_of(x, hz)
    y, rep = J.limiter_host(x, hz, 1.0, R.CEILING, F.PEAK_TRUE)
    over = 20.0 * math.log10(R.true_peak_of(y, hz) / c)
    ys, _ = J.limiter_host(x, hz, 1.0, R.CEILING, F.PEAK_SAMPLE)
    over_s = 20.0 * math.log10(R.true_peak_of(ys, hz) / c)
    print("hz", hz, "true-peak detector: %+.5f dB, sample detector: %+.3f dB over the ceiling" % (over, over_s),
          "reduction %.2f dB" % rep["max_reduction_db"])
    assert np.max(np.abs(y)) <= c and np.max(np.abs(ys)) <= c
    assert over <= 0.01
    assert over_s > 1.0

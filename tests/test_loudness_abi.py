"""Loudness normalization, host side (no GPU): the symbols, jb_loudness_filter against the BS.1770-4 table and the
formula, and the engine's target and ceiling."""
import ctypes as C
import math

import numpy as np

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests.conftest import VOICE
from tests.loudness_ref import k_filter

NEW_SYMBOLS = ["jb_batch_set_loudness_target", "jb_batch_loudness", "jb_loudness_filter", "jb_loudness_pcm_batch",
               "jb_engine_set_loudness_target", "jb_engine_get_loudness_target", "jb_engine_set_peak_ceiling",
               "jb_engine_get_peak_ceiling"]


def test_symbols_exported_and_mirrored():
    L = J.lib()
    for s in NEW_SYMBOLS:
        assert s in _ffi.SYMBOLS, s
        assert hasattr(L, s), s


def test_filter_at_48k_is_the_bs1770_table():
    b, a, hop = J.loudness_filter(48000)
    assert hop == 4800
    np.testing.assert_allclose(b[0], [1.53512485958697, -2.69169618940638, 1.19839281085285], rtol=0, atol=1e-14)
    np.testing.assert_allclose(a[0], [1.0, -1.69065929318241, 0.73248077421585], rtol=0, atol=1e-14)
    np.testing.assert_array_equal(b[1], [1.0, -2.0, 1.0])
    np.testing.assert_allclose(a[1], [1.0, -1.99004745483398, 0.99007225036621], rtol=0, atol=1e-14)


def test_filter_at_other_rates_is_the_formula():
    for hz in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000):
        b, a, hop = J.loudness_filter(hz)
        rb, ra, rh = k_filter(hz)
        np.testing.assert_allclose(b, rb, rtol=1e-14, atol=1e-15, err_msg=str(hz))
        np.testing.assert_allclose(a, ra, rtol=1e-14, atol=1e-15, err_msg=str(hz))
        assert hop == rh == (hz + 5) // 10
    assert J.loudness_filter(11025)[2] == 1103


def test_filter_null_pointers_and_zero_rate():
    L = J.lib()
    hop = C.c_uint32()
    assert L.jb_loudness_filter(16000, None, None, C.byref(hop)) == 0 and hop.value == 1600
    assert L.jb_loudness_filter(16000, None, None, None) == 0
    assert L.jb_loudness_filter(0, None, None, C.byref(hop)) == -1


def test_engine_target_and_ceiling_setter_getter_and_copy():
    eng = J.Engine.load([VOICE])
    c = eng.condition
    assert math.isnan(c.get_loudness_target())
    assert c.get_peak_ceiling() == 0.0
    c.set_loudness_target(-16.0)
    c.set_peak_ceiling(-1.5)
    assert c.get_loudness_target() == -16.0 and c.get_peak_ceiling() == -1.5
    L = J.lib()
    h = C.c_void_p()
    assert L.jb_engine_new(eng._h, eng._h, C.byref(h)) == 0
    try:
        assert L.jb_engine_get_loudness_target(h) == -16.0
        assert L.jb_engine_get_peak_ceiling(h) == -1.5
    finally:
        L.jb_engine_free(h)
    assert eng.clone().condition.get_loudness_target() == -16.0
    c.set_peak_ceiling(math.inf)
    assert c.get_peak_ceiling() == math.inf
    c.set_loudness_target(math.nan)
    assert math.isnan(c.get_loudness_target())
    # other fields stay as they were
    assert c.get_output_sampling_frequency() == 0 and c.get_sampling_frequency() == 48000


# ---- the two refusals of the measurement: both return before any device is opened -------------------------------------
def _raises(fn):
    try:
        fn()
    except J.JbError as e:
        return e
    return None


def _seams(hz):
    x = [np.zeros(8)]
    return [lambda: J.loudness(x, hz), lambda: J.loudness_groups(x, hz)]


def test_a_hop_above_61439_samples_is_refused_and_named():
    for seam in _seams(614395):
        e = _raises(seam)
        assert e is not None and e.code == -2, e
        assert "614395 Hz" in str(e) and "hop of 61440" in str(e), str(e)
    for seam in _seams(614394):  # accepted: a hop of 61439; without a device what is left is the device's own error
        e = _raises(seam)
        assert e is None or e.code == -3, e


def test_a_rate_whose_nyquist_is_not_above_the_shelf_is_refused_and_named():
    """At 3363 Hz and below K = tan(pi 1681.97 / fs) is not positive and the shelf is unstable (a2 = 1.00125 at
    3363 Hz, 0.99993 at 3364 Hz by the formula)."""
    assert k_filter(3363)[1][0][2] > 1.0 > k_filter(3364)[1][0][2] > 0.9999
    for hz in (3363, 3000, 400, 1):
        for seam in _seams(hz):
            e = _raises(seam)
            assert e is not None and e.code == -2, (hz, e)
            assert "%d Hz" % hz in str(e) and "shelf" in str(e) and "Nyquist" in str(e), str(e)
    for seam in _seams(3364):
        e = _raises(seam)
        assert e is None or e.code == -3, e
    # the coefficients stay a pure function of the rate, and the true peak reads no hop energy: neither refuses
    assert J.loudness_filter(3000)[2] == 300
    e = _raises(lambda: J.true_peak([np.zeros(8)], 3000))
    assert e is None or e.code == -3, e
    e = _raises(lambda: J.loudness([np.zeros(8)], 0))
    assert e is not None and e.code == -1

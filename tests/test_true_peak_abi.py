"""True-peak ceiling, host side (no GPU): the symbols, jb_true_peak_filter against the formula, its argument rules,
and the engine's peak mode."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests.conftest import VOICE
from tests.true_peak_ref import factor, table

NEW_SYMBOLS = ["jb_batch_set_peak_mode", "jb_batch_loudness_report", "jb_true_peak_filter", "jb_true_peak_pcm_batch",
               "jb_engine_set_peak_mode", "jb_engine_get_peak_mode"]

FACTORS = {48000: 4, 44100: 5, 96000: 2, 192000: 1, 32000: 6, 24000: 8, 22050: 9, 16000: 12, 11025: 18, 8000: 24,
           1000: 64}


def test_symbols_exported_and_mirrored():
    L = J.lib()
    for s in NEW_SYMBOLS:
        assert s in _ffi.SYMBOLS, s
        assert hasattr(L, s), s
    assert J.PEAK_SAMPLE == 0 and J.PEAK_TRUE == 1
    assert C.sizeof(_ffi.LoudnessReport) == 40 and _ffi.LoudnessReport.peak_mode.offset == 32


def test_factor_per_rate():
    for hz, want in FACTORS.items():
        F, taps = J.true_peak_filter(hz)
        assert F == want == factor(hz), hz
        assert taps.shape == (F - 1, 12)
    assert J.true_peak_filter(384000)[0] == 1


def test_taps_are_the_formula():
    for hz in FACTORS:
        F, taps = J.true_peak_filter(hz)
        rF, rtaps = table(hz)
        assert F == rF
        np.testing.assert_allclose(taps, rtaps, rtol=0, atol=1e-14, err_msg=str(hz))
    # the middle phase at 48 kHz is symmetric, and two equal neighbours interpolate to 1.24054 of their value
    _, t48 = J.true_peak_filter(48000)
    np.testing.assert_allclose(t48[1], t48[1][::-1], rtol=0, atol=1e-14)
    assert t48[1][5] + t48[1][6] == pytest.approx(1.24054, abs=5e-6)
    # phase p read backwards is phase F - p
    np.testing.assert_allclose(t48[0], t48[2][::-1], rtol=0, atol=1e-14)


def test_null_pointers_zero_rate_and_short_buffer():
    L = J.lib()
    F, nt = C.c_uint32(), C.c_uint32()
    assert L.jb_true_peak_filter(16000, C.byref(F), None, None, 0) == 0 and F.value == 12
    assert L.jb_true_peak_filter(16000, None, C.byref(nt), None, 0) == 0 and nt.value == 12
    assert L.jb_true_peak_filter(16000, None, None, None, 0) == 0
    assert L.jb_true_peak_filter(0, C.byref(F), C.byref(nt), None, 0) == -1
    buf = np.full(11 * 12 + 1, 7.0)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.jb_true_peak_filter(16000, None, None, dp, 11 * 12 - 1) == -8   # JB_ERR_BUFFER
    assert (buf == 7.0).all()
    assert L.jb_true_peak_filter(16000, None, None, dp, 11 * 12) == 0
    assert buf[-1] == 7.0 and (buf[:-1] != 7.0).all()
    # F = 1: no phase is tabled, any buffer will do
    assert L.jb_true_peak_filter(192000, C.byref(F), None, dp, 0) == 0 and F.value == 1


def test_engine_peak_mode_setter_getter_and_copy():
    eng = J.Engine.load([VOICE])
    c = eng.condition
    assert c.get_peak_mode() == J.PEAK_SAMPLE
    c.set_peak_mode(J.PEAK_TRUE)
    assert c.get_peak_mode() == J.PEAK_TRUE
    L = J.lib()
    h = C.c_void_p()
    assert L.jb_engine_new(eng._h, eng._h, C.byref(h)) == 0
    try:
        assert L.jb_engine_get_peak_mode(h) == J.PEAK_TRUE
    finally:
        L.jb_engine_free(h)
    assert eng.clone().condition.get_peak_mode() == J.PEAK_TRUE
    with pytest.raises(J.JbError):
        c.set_peak_mode(2)
    assert L.jb_engine_set_peak_mode(eng._h, 0xFFFFFFFF) == -1
    assert c.get_peak_mode() == J.PEAK_TRUE
    c.set_peak_mode(J.PEAK_SAMPLE)
    assert c.get_peak_mode() == J.PEAK_SAMPLE
    # other fields stay as they were
    assert c.get_peak_ceiling() == 0.0 and c.get_sampling_frequency() == 48000

"""The filter stage without a GPU: the design against the Audio EQ Cookbook restated in numpy, |H| at f0, every refusal
with the utterance, the section and the field in jb_last_error, the struct layouts against ctypes, and the host seam
(jb_filter_pcm_host) against the long-double reference of tests/filter_ref.py under its gate."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from tests import filter_ref as R

ROOT = Path(__file__).resolve().parent.parent
RATES = [8000, 16000, 22050, 48000, 96000]
KINDS = {"highpass": F.FILTER_HIGHPASS, "lowpass": F.FILTER_LOWPASS, "peaking": F.FILTER_PEAKING,
         "lowshelf": F.FILTER_LOWSHELF, "highshelf": F.FILTER_HIGHSHELF, "notch": F.FILTER_NOTCH}


def cookbook(kind, f0, q, gain_db, fs):
    """The RBJ forms: w0 = 2 pi f0 / fs, alpha = sin(w0) / (2 q), A = 10^(gain_db / 40); b0 b1 b2 a1 a2 over a0."""
    w0 = np.float64(2.0) * np.pi * np.float64(f0) / np.float64(fs)
    cw, alpha = np.cos(w0), np.sin(w0) / (2.0 * np.float64(q))
    A = np.power(np.float64(10.0), np.float64(gain_db) / 40.0)
    if kind == "highpass":
        b, a = [(1 + cw) / 2, -(1 + cw), (1 + cw) / 2], [1 + alpha, -2 * cw, 1 - alpha]
    elif kind == "lowpass":
        b, a = [(1 - cw) / 2, 1 - cw, (1 - cw) / 2], [1 + alpha, -2 * cw, 1 - alpha]
    elif kind == "peaking":
        b, a = [1 + alpha * A, -2 * cw, 1 - alpha * A], [1 + alpha / A, -2 * cw, 1 - alpha / A]
    elif kind == "notch":
        b, a = [np.float64(1.0), -2 * cw, np.float64(1.0)], [1 + alpha, -2 * cw, 1 - alpha]
    else:
        t = 2 * np.sqrt(A) * alpha
        if kind == "lowshelf":
            b = [A * ((A + 1) - (A - 1) * cw + t), 2 * A * ((A - 1) - (A + 1) * cw), A * ((A + 1) - (A - 1) * cw - t)]
            a = [(A + 1) + (A - 1) * cw + t, -2 * ((A - 1) + (A + 1) * cw), (A + 1) + (A - 1) * cw - t]
        else:
            b = [A * ((A + 1) + (A - 1) * cw + t), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - t)]
            a = [(A + 1) - (A - 1) * cw + t, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - t]
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]], dtype=np.float64)


@pytest.mark.parametrize("hz", RATES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_design_is_the_cookbook(kind, hz):
    """The library and the restatement do the same f64 operations in the same order; what may differ is the last bit of
    cos(w0), sin(w0) and 10^(g / 40) between two math libraries (1 ulp each).  A coefficient is a sum of at most three
    terms no larger than the section's largest numerator or denominator, over a0: the two trigonometric inputs move it
    by at most 1 ulp of the largest coefficient each, a0's own last bit moves all five by 1 ulp more, and the rounding
    of the quotient may then fall the other way, 1 ulp: 4 ulp of the section's largest coefficient."""
    for f0, q, g in ((50.0, 0.5, -6.0), (300.0, 1 / math.sqrt(2), 4.0), (1000.0, 2.0, 6.0), (3400.0, 30.0, -3.0)):
        got = J.filter_design(F.filter_section(KINDS[kind], f0, q, g), hz)
        want = cookbook(kind, f0, q, g, hz)
        big = np.max(np.abs(want))
        assert got.shape == (1, 5)
        assert np.max(np.abs(got[0] - want)) <= 4 * np.spacing(big), (kind, hz, f0, got[0] - want)


@pytest.mark.parametrize("hz", RATES)
def test_magnitude_at_f0(hz):
    from scipy import signal

    def mag_db(f, f0):
        _, h = signal.sosfreqz(J.filter_sos(f, hz), worN=[f0], fs=hz)
        return 20 * math.log10(abs(h[0]))

    for f0 in (70.0, 1000.0, 3400.0):
        assert abs(mag_db(J.highpass(f0, 1 / math.sqrt(2)), f0) - -3.0103) < 1e-3
        assert abs(mag_db(J.lowpass(f0, 1 / math.sqrt(2)), f0) - -3.0103) < 1e-3
        for g in (6.0, -4.5):
            assert abs(mag_db(J.peaking(f0, g, 2.0), f0) - g) < 1e-6
        # (the zero sits on the unit circle up to the rounding of b1 = -2 cos(w0): 4.4e-16 over a denominator of
        # about 2 alpha sin(w0) >= 7e-7 here, -184 dB at the worst)
        assert mag_db(J.notch(f0, 30.0), f0) < -120
    # the shelves reach their gain away from the corner
    assert abs(mag_db(J.lowshelf(1000.0, -6.0), 1.0) - -6.0) < 1e-3
    assert abs(mag_db(J.highshelf(1000.0, 4.0), hz / 2 - 1.0) - 4.0) < 1e-3


def refused(call):
    with pytest.raises(J.JbError) as e:
        call()
    assert "JB_ERR_INVALID" in str(e.value)
    return str(e.value)


def test_every_refusal_names_utterance_section_and_field():
    ok = J.highpass(70.0)
    raw = J.raw_filter([[1.0, 0.0, 0.0, -1.2, 0.5]])

    def bad_section(**kw):
        f = ok + J.peaking(1000.0, 3.0, 2.0)
        for k, v in kw.items():
            setattr(f.section[1], k, v)
        return f

    def bad_raw(**kw):
        f = ok + raw
        for k, v in kw.items():
            setattr(f.section[1], k, v)
        return f

    cases = [
        (bad_section(kind=0), "kind"), (bad_section(kind=8), "kind"),
        (bad_section(f0_hz=0.0), "f0_hz"), (bad_section(f0_hz=-5.0), "f0_hz"),
        (bad_section(f0_hz=4000.0), "f0_hz"), (bad_section(f0_hz=5000.0), "f0_hz"),
        (bad_section(f0_hz=float("nan")), "f0_hz"), (bad_section(f0_hz=float("inf")), "f0_hz"),
        (bad_section(q=0.0), "q"), (bad_section(q=-1.0), "q"), (bad_section(q=float("nan")), "q"),
        (bad_section(q=float("inf")), "q"), (bad_section(gain_db=float("nan")), "gain_db"),
        (bad_section(gain_db=float("-inf")), "gain_db"),
        (bad_raw(b1=float("nan")), "b1"), (bad_raw(a2=float("inf")), "a2"),
        (bad_raw(a2=1.0), "a2"), (bad_raw(a2=-1.0), "a2"),           # |a2| < 1
        (bad_raw(a1=1.5, a2=0.5), "a1"), (bad_raw(a1=-1.5, a2=0.5), "a1"),  # |a1| < 1 + a2
    ]
    x = np.zeros(8)
    for f, field in cases:
        msg = refused(lambda: J.filter_design(f, 8000))
        assert "utterance 0, section 1: " + field in msg, msg
        # through the device seam: refused before any device is touched, naming the utterance
        msg = refused(lambda: J.filter_pcm([x, x, x], [ok, None, f], 8000))
        assert "utterance 2, section 1: " + field in msg, msg
        msg = refused(lambda: J.filter_pcm_host(x, f, 8000))
        assert "section 1: " + field in msg, msg
    # f0 is checked against that utterance's rate: the same filter passes at 16 kHz
    f = bad_section(f0_hz=4000.0)
    assert J.filter_design(f, 16000).shape == (2, 5)
    msg = refused(lambda: J.filter_pcm([x, x], [f, f], [16000, 8000]))
    assert "utterance 1, section 1: f0_hz" in msg
    # more than four sections
    five = ok + ok + ok + ok + ok
    assert five.n_sections == 5
    assert "n_sections" in refused(lambda: J.filter_design(five, 48000))
    assert "utterance 1: n_sections" in refused(lambda: J.filter_pcm([x, x], [ok, five], 48000))
    # a raw section is used as given at any rate, and a stable one passes
    assert np.array_equal(J.filter_design(raw, 8000), J.filter_design(raw, 96000))
    assert np.array_equal(J.filter_design(raw, 8000)[0], [1.0, 0.0, 0.0, -1.2, 0.5])


def test_struct_layouts_header_vs_ctypes(tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(jb_filter_section), sizeof(jb_filter), '
                   'sizeof(jb_biquad), offsetof(jb_filter_section, f0_hz), offsetof(jb_filter_section, gain_db), '
                   'offsetof(jb_filter_section, b0), offsetof(jb_filter, n_sections), offsetof(jb_biquad, a1));'
                   "return 0;}\n")
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == [C.sizeof(F.FilterSection), C.sizeof(F.Filter), C.sizeof(F.Biquad), F.FilterSection.f0_hz.offset,
                       F.FilterSection.gain_db.offset, F.FilterSection.b0.offset, F.Filter.n_sections.offset,
                       F.Biquad.a1.offset] == [72, 296, 40, 8, 24, 32, 288, 24]
    assert F.FILTER_MAX_SECTIONS == 4 and F.FILTER_RAW == 7


def test_constructors():
    t = J.telephone_band()
    assert t.n_sections == 2 and (t.section[0].kind, t.section[0].f0_hz) == (F.FILTER_HIGHPASS, 300.0)
    assert (t.section[1].kind, t.section[1].f0_hz) == (F.FILTER_LOWPASS, 3400.0)
    assert J.highpass(70.0).section[0].q == pytest.approx(0.7071, abs=1e-4)
    assert J.no_filter().n_sections == 0 and J.filter_design(J.no_filter(), 48000).shape == (0, 5)
    # a cascade designs to its members' sections, in order
    c = J.highpass(70.0) + J.peaking(3000.0, 6.0, 2.0)
    assert np.array_equal(J.filter_design(c, 48000), np.concatenate([J.filter_design(J.highpass(70.0), 48000),
                                                                      J.filter_design(J.peaking(3000.0, 6.0, 2.0), 48000)]))


def test_host_seam_is_the_reference():
    """Every case of the table; sosfilt itself stays inside the gate (it defines it) and so does the host seam."""
    gate = R.gate()
    sos, host = R.sosfilt_errors(), R.host_errors()
    assert set(host) == set(sos) == set(R.cases()) and len(host) == len(R.filters()) * len(R.LENGTHS)
    print(f"floor {R.floor():.3e}  gate {gate:.3e}  host seam's largest error {max(host.values()):.3e}")
    assert 0 < R.floor() < 1e-9  # (a floor of f64 rounding, not of a wrong reference)
    worst = max(host, key=host.get)
    assert host[worst] <= gate, (R.filters()[worst[0]][0], worst[1], host[worst], gate)


def test_no_sections_returns_the_input_bit_for_bit():
    x = R.signal_at(48000)[:10001]
    for f in (None, J.no_filter()):
        y = J.filter_pcm_host(x, f, 48000)
        assert y.tobytes() == x.tobytes()
    assert J.filter_pcm_host(np.zeros(0), J.highpass(70.0), 48000).size == 0

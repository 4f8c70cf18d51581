"""Frame conditioning on the host, without a GPU (jbonsai_amd/csrc/jb_fbank.h, jb_fbank.cpp, jb_mfcc.cpp): the
request's layout, every refusal naming its field, the identity of the zero request, the four window tables against long
double, the reflected index table, the exact properties of DC removal and pre-emphasis, and the host form of the rule
under the precision gate of tests/frame_ref.py (the linear f64 gate of tests/fbank_ref.py: at most GATE times the
error of a float64 numpy model of the same frames, both against a long double model).

JB_FRAME_ENERGY: with small integer samples and no DC removal e is an exact integer, so the reference ln(e) in long
double is off by its own rounding only; c0 is held to one f64 ulp for the host's logarithm plus half an ulp for the
rounding of the reference value."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import fbank_ref as R
from tests import frame_ref as FR

ROOT = Path(__file__).resolve().parent.parent
INVALID = -1
LD = np.longdouble

needs_ld = pytest.mark.skipif(not R.have_long_double(), reason="numpy.longdouble has no 64-bit mantissa here")


def test_opts_layout(tmp_path):
    fields = ("preemph", "window", "flags", "reserved")
    consts = ("JB_FRAME_WINDOW_OPTS", "JB_FRAME_POVEY", "JB_FRAME_HANN_SYM", "JB_FRAME_RECT", "JB_FRAME_BLACKMAN",
              "JB_FRAME_REMOVE_DC", "JB_FRAME_REFLECT", "JB_FRAME_ENERGY")
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){'
                   'printf("%zu\\n", sizeof(jb_frame_opts));' +
                   "".join(f'printf("%zu\\n", offsetof(jb_frame_opts, {f}));' for f in fields) +
                   "".join(f'printf("%u\\n", {c});' for c in consts) + "return 0;}\n")
    want = [32, 0, 8, 12, 16, 0, 1, 2, 3, 4, 1, 2, 4]
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == want
    assert C.sizeof(_ffi.FrameOpts) == 32
    assert [getattr(_ffi.FrameOpts, f).offset for f in fields] == want[1:5]
    assert (J.FRAME_WINDOW_OPTS, J.FRAME_POVEY, J.FRAME_HANN_SYM, J.FRAME_RECT, J.FRAME_BLACKMAN, J.FRAME_REMOVE_DC,
            J.FRAME_REFLECT, J.FRAME_ENERGY) == tuple(want[5:])


def _refused(field, fr, fopts=None, mopts=None, every=True):
    """jb_frame_check and, for an fbank request, the host entries refuse the request naming `field`."""
    L = J.lib()
    f = fopts if fopts is not None else J.fbank()
    assert L.jb_frame_check(C.byref(f), C.byref(mopts) if mopts is not None else None, C.byref(fr)) == INVALID
    assert field in L.jb_last_error().decode(), (field, L.jb_last_error())
    x = np.zeros(1000)
    out = np.zeros(1 << 16, dtype=np.uint8)
    if mopts is not None:
        rc = L.jb_mfcc_framed_pcm_host(x.ctypes.data, 1000, 16000, C.byref(f), C.byref(mopts), C.byref(fr),
                                       out.ctypes.data, out.size)
        assert rc == INVALID and field in L.jb_last_error().decode()
        return
    assert L.jb_fbank_framed_host(x.ctypes.data, 1000, 16000, C.byref(f), C.byref(fr), out.ctypes.data,
                                  out.size) == INVALID
    assert field in L.jb_last_error().decode()
    if every:
        assert L.jb_fbank_framed_geometry(16000, C.byref(f), C.byref(fr), 1000, None, None, None, None, None) == INVALID
        assert field in L.jb_last_error().decode()
        assert L.jb_frame_window(16000, C.byref(f), C.byref(fr), out.ctypes.data, 400) == INVALID
        assert field in L.jb_last_error().decode()


def test_every_refusal_names_its_field():
    fr = J.frame()
    fr.window = 5
    _refused("window", fr)
    fr = J.frame()
    fr.flags = 8
    _refused("flags", fr)
    for word in range(4):
        fr = J.frame()
        fr.reserved[word] = 1
        _refused("reserved", fr)
    for c in (-0.01, 1.01, float("nan"), float("inf")):
        _refused("preemph", J.frame(preemph=c))
    _refused("flags", J.frame(reflect=True), fopts=J.fbank(center=True))
    # the energy: refused with an fbank request and with n_ceps = 0, taken with cepstra (geometry and window are the
    # mfcc request's too, so they do not refuse it)
    _refused("flags", J.frame(energy=True), every=False)
    _refused("flags", J.frame(energy=True), mopts=J.mfcc(n_ceps=0))
    L = J.lib()
    f, m = J.fbank(), J.mfcc()
    assert L.jb_frame_check(C.byref(f), C.byref(m), C.byref(J.frame(energy=True))) == 0
    assert L.jb_frame_check(C.byref(f), None, None) == INVALID
    assert L.jb_frame_check(C.byref(f), None, C.byref(J.frame(preemph=1.0, window="blackman", remove_dc=True,
                                                              reflect=True))) == 0
    # the filterbank's and the cepstral options' own refusals come through
    assert L.jb_frame_check(C.byref(J.fbank(n_mels=0)), None, C.byref(J.frame())) == INVALID
    assert "n_mels" in L.jb_last_error().decode()
    assert L.jb_frame_check(C.byref(f), C.byref(J.mfcc(n_ceps=81)), C.byref(J.frame())) == INVALID
    assert "n_ceps" in L.jb_last_error().decode()


def test_kaldi_defaults():
    f, fr = J.kaldi_frame()
    assert (f.win_us, f.hop_us, f.n_fft, f.n_mels, f.f_min_hz, f.f_max_hz, f.log_floor, f.window, f.flags) == \
        (25000, 10000, 0, 23, 20.0, 0.0, 2.0 ** -23, J.FBANK_HANN, 0)
    assert (fr.preemph, fr.window, fr.flags, list(fr.reserved)) == (0.97, J.FRAME_POVEY, J.FRAME_REMOVE_DC, [0] * 4)
    assert J.kaldi_frame(80)[0].n_mels == 80
    with pytest.raises(J.JbError, match="n_mels"):
        J.kaldi_frame(0)
    assert J.lib().jb_frame_check(C.byref(f), None, C.byref(fr)) == 0


@pytest.mark.parametrize("hz", [8000, 16000, 48000])
def test_the_zero_request_is_the_identity(hz):
    wl, hop, _ = R.geometry(hz)
    x = R.gate_signal(hz, 14 * hop + wl + 3)
    zero = J.frame()
    for o in (J.fbank(), J.fbank(window="hamming", center=True, f64=True), J.fbank(n_mels=23, linear=True, unit=True)):
        assert J.fbank_framed_host(x, hz, o, zero).tobytes() == J.fbank_host(x, hz, o).tobytes()
        assert J.frame_window(hz, o, zero).tobytes() == J.fbank_window(hz, o).tobytes()
        assert J.fbank_framed_geometry(hz, o, zero, x.size) == J.fbank_geometry(hz, o, x.size)
    m = J.mfcc(delta_order=2, cmvn="mean_var")
    assert J.mfcc_framed_pcm_host(x, hz, J.fbank(), m, zero).tobytes() == J.mfcc_pcm_host(x, hz, J.fbank(), m).tobytes()


@needs_ld
@pytest.mark.parametrize("hz", [8000, 16000, 22050, 48000])
def test_windows_are_the_long_double_formulas(hz):
    wl = R.geometry(hz)[0]
    for kind in (FR.POVEY, FR.HANN_SYM, FR.RECT, FR.BLACKMAN):
        w = J.frame_window(hz, J.fbank(), J.frame(window=FR.NAMES[kind]))
        ref = FR.window_ld(kind, wl)
        # one rounding of the long double value: half an f64 ulp, and the long double formula's own last bits
        slack = np.spacing(np.abs(ref.astype(np.float64))).astype(LD) * (LD("0.5") + LD(2) ** -8)
        assert w.shape == (wl,) and np.all(np.abs(w.astype(LD) - ref) <= slack), kind
        assert np.max(np.abs(w - w[::-1])) <= 2.3e-16  # symmetric
    assert np.all(J.frame_window(hz, J.fbank(), J.frame(window="rect")) == 1.0)
    assert J.frame_window(hz, J.fbank(), J.frame(window="povey"))[0] == 0.0
    ham = J.fbank(window="hamming")
    assert np.array_equal(J.frame_window(hz, ham, J.frame(preemph=0.5)), J.fbank_window(hz, ham))


@pytest.mark.parametrize("n", [0, 1, 79, 80, 81, 400, 401, 1000])
def test_reflected_frames_and_indices(n):
    """T and every index of every frame at 16 kHz (wl 400, hop 160) against the model's index table: frame t of the
    unit equals, bit for bit, the one snip frame of the wl samples the table names."""
    hz, (wl, hop, _) = 16000, R.geometry(16000)
    idx = FR.index_table(n, wl, hop, reflect=True)
    T = (n + hop // 2) // hop
    assert idx.shape == (T, wl) and (T == 0 or (idx.min() >= 0 and idx.max() < n))
    f, fr = J.fbank(n_mels=8, linear=True, f64=True), J.frame(window="rect", reflect=True)
    assert J.fbank_framed_geometry(hz, f, fr, n)[3:] == (T, T * 8 * 8)
    assert J.fbank_framed_host(np.zeros(n), hz, f, fr).shape == (T, 8)
    if n == 81:  # half a hop more than half a hop: one frame, and it reflects more than once
        assert T == 1 and idx[0, 0] == FR.reflect_index(80 - 200, 81) and len(set(idx[0])) == 81
        assert np.sum(idx[0] == 0) >= 4
    plain = J.fbank(n_mels=8, linear=True, f64=True)
    x = np.random.default_rng(n).integers(-2000, 2000, n).astype(np.float64)
    got = J.fbank_framed_host(x, hz, f, fr)
    for t in range(T):
        frame = x[idx[t]]
        want = J.fbank_framed_host(frame, hz, plain, J.frame(window="rect"))
        assert want.shape == (1, 8) and np.array_equal(got[t], want[0]), (n, t)


def test_exact_silence_of_a_constant_signal():
    """An integer-valued constant: the mean is the value itself (a division), so DC removal leaves exact zeros; with
    preemph = 1.0, y_i = v_i - v_{i-1} = 0 and y_0 = v_0 - v_0 = 0 exactly.  Every energy is the floor."""
    hz = 16000
    x = np.full(3000, 1234.0)
    ln_floor = float(np.log(LD(2.0 ** -52)))
    for fr in (J.frame(window="rect", remove_dc=True), J.frame(preemph=1.0), J.frame(preemph=1.0, window="povey"),
               J.frame(window="rect", remove_dc=True, reflect=True), J.frame(preemph=1.0, reflect=True)):
        E = J.fbank_framed_host(x, hz, J.fbank(linear=True, f64=True), fr)
        assert E.shape[0] >= 16 and np.all(E == 0.0)
        assert np.all(J.fbank_framed_host(x, hz, J.fbank(f64=True), fr) == ln_floor)
    # other windows under DC removal: zeros times anything
    assert np.all(J.fbank_framed_host(x, 48000, J.fbank(linear=True, f64=True),
                                      J.frame(window="blackman", remove_dc=True)) == 0.0)


RATES = ((8000, 23), (16000, 80), (48000, 80))


def _gate(hz, n_mels, **kw):
    wl, hop, _ = R.geometry(hz)
    x = FR.gate_signal(hz, 18 * hop + wl + 3, hop, offset=3000.0)
    return FR.check_gate(lambda x, f, fr: J.fbank_framed_host(x, hz, f, fr), x, hz, n_mels, "host", min_live=8, **kw)


@needs_ld
@pytest.mark.parametrize("hz,n_mels", RATES)
@pytest.mark.parametrize("window", FR.WINDOWS)
@pytest.mark.parametrize("reflect", [False, True])
def test_host_form_under_the_gate(hz, n_mels, window, reflect):
    """DC removal and 0.97 pre-emphasis on a signal with a DC offset of 3000 on its live part, every window, snip and
    reflected framing."""
    _gate(hz, n_mels, window=window, reflect=reflect, preemph=0.97, remove_dc=True)


@needs_ld
@pytest.mark.parametrize("hz,n_mels", RATES)
@pytest.mark.parametrize("preemph,remove_dc", [(0.97, False), (1.0, False), (0.0, True), (0.97, True), (1.0, True)])
def test_host_form_under_the_gate_by_preemphasis(hz, n_mels, preemph, remove_dc):
    _gate(hz, n_mels, window=FR.POVEY, preemph=preemph, remove_dc=remove_dc)


@needs_ld
def test_host_form_under_the_gate_in_centre_mode_and_unit_scale():
    _gate(16000, 80, window=FR.HANN_SYM, center=True, preemph=0.97, remove_dc=True, fbank_window=R.HAMMING)
    _gate(16000, 80, window=FR.WINDOW_OPTS, preemph=0.97, remove_dc=True, fbank_window=R.HAMMING, unit=True)


@needs_ld
@pytest.mark.parametrize("hz", [16000, 48000])
def test_energy_replaces_c0(hz):
    wl, hop, _ = R.geometry(hz)
    x = np.random.default_rng(hz).integers(-3000, 3001, 9 * hop + wl).astype(np.float64)
    x[:wl + hop] = 0.0  # two silent frames: the floor
    f = J.fbank(n_mels=40, log_floor=1e-3)
    m = J.mfcc(n_ceps=13, f64=True)
    for fr_kw in (dict(), dict(preemph=0.97, window="povey"), dict(reflect=True)):
        with_e = J.mfcc_framed_pcm_host(x, hz, f, m, J.frame(energy=True, **fr_kw))
        without = J.mfcc_framed_pcm_host(x, hz, f, m, J.frame(**fr_kw))
        assert with_e.shape == without.shape and with_e.shape[1] == 13
        assert np.array_equal(with_e[:, 1:], without[:, 1:])
        _, _, e = FR.model_ld(x, hz, 40, reflect=fr_kw.get("reflect", False))
        assert np.all(e == np.round(e)) and e.max() < 2 ** 53
        silent = e == 0
        assert silent.sum() >= 1 and (~silent).sum() >= 6
        assert np.all(with_e[silent, 0] == float(np.log(LD(1e-3))))
        ref = np.log(e[~silent])
        ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(LD)
        assert np.all(np.abs(with_e[~silent, 0].astype(LD) - ref) <= LD("1.5") * ulp)
    # before CMVN and the deltas: the rows equal jb_mfcc_host's on statics -- the deltas of c0 are the deltas of ln e
    md = J.mfcc(n_ceps=13, f64=True, delta_order=2, cmvn="mean")
    full = J.mfcc_framed_pcm_host(x, hz, f, md, J.frame(energy=True))
    stat = J.mfcc_framed_pcm_host(x, hz, f, m, J.frame(energy=True))
    mu = full[:, :13] - stat  # (c - mu) - c: the same per column, to rounding
    assert np.all(np.abs(mu - mu[0]) <= 1e-12) and full.shape == (stat.shape[0], 39)
    # f32 rows are one rounding of the f64 ones
    m32 = J.mfcc(n_ceps=13)
    assert np.array_equal(J.mfcc_framed_pcm_host(x, hz, f, m32, J.frame(energy=True)), stat.astype(np.float32))

"""Cepstral features on the host, without a GPU (jbonsai_amd/csrc/jb_mfcc.cpp): the options' layout, every refusal
naming its field, the DCT, the lifter and the delta kernels against the long double formulas (tests/mfcc_ref.py), and
the host form of the rule under the precision gate for every CMVN mode and delta order.

The gate (tests/mfcc_ref.py): e(X) = max |X - X_ld| / bound <= 8 e(model_f64), each element divided by the magnitude
bound the long double model makes by running the same pipeline on absolute values."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import mfcc_ref as R

ROOT = Path(__file__).resolve().parent.parent
INVALID, BUFFER = -1, -8
LD = np.longdouble
needs_ld = pytest.mark.skipif(not R.have_long_double(), reason="numpy.longdouble has no 64-bit mantissa here")


def test_opts_layout(tmp_path):
    fields = ("n_ceps", "delta_order", "delta_window", "cmvn", "lifter", "var_floor", "flags", "reserved")
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){'
                   'printf("%zu\\n", sizeof(jb_mfcc_opts));' +
                   "".join(f'printf("%zu\\n", offsetof(jb_mfcc_opts, {f}));' for f in fields) +
                   'printf("%u %u %u %u\\n", JB_CMVN_NONE, JB_CMVN_MEAN, JB_CMVN_MEAN_VAR, JB_MFCC_F64);return 0;}\n')
    want = [48, 0, 4, 8, 12, 16, 24, 32, 36, 0, 1, 2, 1]
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == want
    assert C.sizeof(_ffi.MfccOpts) == 48
    assert [getattr(_ffi.MfccOpts, f).offset for f in fields] == want[1:9]
    assert (J.CMVN_NONE, J.CMVN_MEAN, J.CMVN_MEAN_VAR, J.MFCC_F64) == tuple(want[9:])


def _refused(field, n_mels=23, fb=None, **kw):
    """Every entry that takes the options refuses them, naming the field, and touches no device."""
    o = J.mfcc(**kw) if not isinstance(kw.get("opts"), _ffi.MfccOpts) else kw["opts"]
    f = fb or J.fbank(n_mels=n_mels)
    L = J.lib()
    buf = np.zeros(1 << 12)
    x = np.zeros(800)
    u8p, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    ins, ns = (dp * 1)(buf.ctypes.data_as(dp)), (C.c_size_t * 1)(2)
    xs, nx, hz = (dp * 1)(x.ctypes.data_as(dp)), (C.c_size_t * 1)(800), (C.c_uint32 * 1)(16000)
    outs, nb = (u8p * 1)(), (C.c_size_t * 1)()
    calls = [
        lambda: L.jb_mfcc_geometry(16000, C.byref(f), C.byref(o), 800, None, None, None),
        lambda: L.jb_mfcc_pcm_host(x.ctypes.data, 800, 16000, C.byref(f), C.byref(o), buf.ctypes.data, buf.nbytes),
        lambda: L.jb_mfcc_pcm_batch(xs, nx, 1, hz, C.byref(f), C.byref(o), -1, outs, nb),
    ]
    if fb is None:
        calls += [
            lambda: L.jb_mfcc_host(buf.ctypes.data, 2, n_mels, C.byref(o), buf.ctypes.data, buf.nbytes),
            lambda: L.jb_mfcc_dct(n_mels, C.byref(o), None, 0, None, 0),
            lambda: L.jb_mfcc_frames_batch(ins, ns, 1, n_mels, C.byref(o), -1, outs, nb),
        ]
    for call in calls:
        assert call() == INVALID, (field, kw)
        assert field in L.jb_last_error().decode(), (field, L.jb_last_error())


def test_every_refusal_names_its_field():
    _refused("n_ceps", n_ceps=24)
    _refused("n_ceps", n_mels=1, n_ceps=2)
    _refused("delta_order", delta_order=3)
    for order in (0, 1, 2):  # the window is checked at every order
        _refused("delta_window", delta_order=order, delta_window=0)
        _refused("delta_window", delta_order=order, delta_window=6)
    _refused("cmvn", cmvn=3)
    _refused("lifter", lifter=-1.0)
    _refused("lifter", lifter=float("inf"))
    _refused("lifter", lifter=float("nan"))
    _refused("var_floor", var_floor=-1e-9)
    _refused("var_floor", var_floor=float("inf"))
    _refused("var_floor", var_floor=float("nan"))
    o = J.mfcc()
    o.flags = 2
    _refused("flags", opts=o)
    for word in range(3):
        o = J.mfcc()
        o.reserved[word] = 1
        _refused("reserved", opts=o)
    # the filterbank options: the stage makes f64 logarithms itself
    _refused("flags", fb=J.fbank(n_mels=23, linear=True))
    _refused("flags", fb=J.fbank(n_mels=23, f64=True))
    _refused("n_mels", fb=J.fbank(n_mels=0), n_ceps=0)
    L = J.lib()
    f, o = J.fbank(n_mels=23), J.mfcc()
    assert L.jb_mfcc_geometry(16000, C.byref(f), None, 0, None, None, None) == INVALID
    assert L.jb_mfcc_geometry(16000, None, C.byref(o), 0, None, None, None) == INVALID
    assert L.jb_mfcc_geometry(16000, C.byref(f), C.byref(o), 0, None, None, None) == 0  # every out pointer may be null
    # a rate the geometry refuses names the filterbank's field
    assert L.jb_mfcc_geometry(100, C.byref(f), C.byref(o), 0, None, None, None) == INVALID
    assert "n_fft" in L.jb_last_error().decode()
    s = np.zeros(21)
    assert L.jb_mfcc_delta_kernel(3, 2, s.ctypes.data, 21) == INVALID and "delta_order" in L.jb_last_error().decode()
    assert L.jb_mfcc_delta_kernel(1, 0, s.ctypes.data, 21) == INVALID and "delta_window" in L.jb_last_error().decode()
    assert L.jb_mfcc_delta_kernel(1, 6, s.ctypes.data, 21) == INVALID and "delta_window" in L.jb_last_error().decode()
    # the limits themselves pass; short buffers
    assert J.mfcc_geometry(16000, J.fbank(n_mels=128), J.mfcc(n_ceps=128, delta_order=2, delta_window=5,
                                                               cmvn="mean_var", f64=True), 400) == (1, 384, 384 * 8)
    assert J.mfcc_geometry(16000, J.fbank(n_mels=80), J.mfcc(n_ceps=0, delta_order=1), 560) == (2, 160, 2 * 160 * 4)
    assert L.jb_mfcc_delta_kernel(2, 5, s.ctypes.data, 20) == BUFFER
    assert L.jb_mfcc_dct(23, C.byref(o), s.ctypes.data, 13 * 23 - 1, None, 0) == BUFFER
    assert L.jb_mfcc_dct(23, C.byref(o), None, 0, s.ctypes.data, 12) == BUFFER
    buf = np.zeros(23 * 2)
    assert L.jb_mfcc_host(buf.ctypes.data, 2, 23, C.byref(o), buf.ctypes.data, 2 * 13 * 4 - 1) == BUFFER


@needs_ld
@pytest.mark.parametrize("n_mels,n_ceps,Q", [(23, 13, 22.0), (80, 80, 22.0), (128, 40, 0.0), (1, 1, 22.0), (128, 128, 0.0),
                                             (40, 13, 0.75)])
def test_dct_and_lifter_are_the_long_double_formulas_rounded_once(n_mels, n_ceps, Q):
    D, l = J.mfcc_dct(n_mels, J.mfcc(n_ceps=n_ceps, lifter=Q))
    assert np.array_equal(D, R.dct_ld(n_mels, n_ceps).astype(np.float64))
    assert np.array_equal(l, R.lifter_ld(n_ceps, Q).astype(np.float64))
    assert l[0] == 1.0 and (Q > 0 or np.all(l == 1.0))
    if n_ceps == n_mels:
        # (the product in long double: the bound is on the table, not on a float64 sum of n_mels products, which
        # alone misses it -- 1.6e-15 at 80)
        assert np.max(np.abs(D.astype(LD) @ D.astype(LD).T - np.eye(n_mels))) <= 1e-15


@needs_ld
def test_delta_kernels_are_the_long_double_formulas_rounded_once():
    for N in range(1, 6):
        den = sum(j * j for j in range(-N, N + 1))
        assert np.array_equal(J.mfcc_delta_kernel(0, N), [1.0])
        for q in (1, 2):
            s = J.mfcc_delta_kernel(q, N)
            ref = R.delta_kernel_ld(q, N)
            assert s.shape == (2 * q * N + 1,) and np.array_equal(s, ref.astype(np.float64))
            # s_q sums to 0: exactly in the long double table; the rounded one to the rounding of its entries
            assert abs(ref.sum()) <= 2.0 ** -63 * np.abs(ref).sum()
            assert abs(s.astype(LD).sum()) <= 2.0 ** -53 * np.abs(s).sum()
            # s_1 is odd and s_2 even, entry for entry
            assert np.array_equal(s, -s[::-1] if q == 1 else s[::-1])
        assert np.array_equal(J.mfcc_delta_kernel(1, N), np.arange(-N, N + 1) / den)
    assert np.array_equal(J.mfcc_delta_kernel(2, 1), [0.25, 0.0, -0.5, 0.0, 0.25])


def test_delta_of_a_ramp_is_one_away_from_the_edges():
    """c[t] = t.  With N = 1 the table is dyadic (+-1/2) and every product and sum exact: the delta is exactly 1 and
    the delta-delta exactly 0 from frame 2 N to T - 1 - 2 N, and the clamped ends are what the rule gives.  For N in
    2..5 the table holds k / 10, k / 28, k / 60, k / 110, none of which f64 represents, and the rule fixes the order of
    the sum, so exactly 1 cannot be had (measured: up to 1 + 1.8e-15 at t < 40); there the delta is 1 within the
    rounding of its 2 N + 1 products and sums, (2 N + 1) 2^-52 sum_j |s_1[j]| |t + j|."""
    T = 40
    ramp = np.arange(T, dtype=np.float64)[:, None]
    for N in range(1, 6):
        y = J.mfcc_host(ramp, J.mfcc(n_ceps=0, delta_order=2, delta_window=N, f64=True))
        assert y.shape == (T, 3) and np.array_equal(y[:, 0], ramp[:, 0])
        mid = slice(2 * N, T - 2 * N)
        s1 = np.abs(J.mfcc_delta_kernel(1, N))
        t = np.arange(T)[mid]
        bound1 = (2 * N + 1) * 2.0 ** -52 * sum(s1[j + N] * np.abs(t + j) for j in range(-N, N + 1))
        s2 = np.abs(J.mfcc_delta_kernel(2, N))
        bound2 = (4 * N + 1) * 2.0 ** -52 * sum(s2[j + 2 * N] * np.abs(t + j) for j in range(-2 * N, 2 * N + 1))
        print(f"N {N}: max |delta - 1| {np.abs(y[mid, 1] - 1).max():.2e}  max |delta-delta| {np.abs(y[mid, 2]).max():.2e}")
        if N == 1:
            assert np.all(y[mid, 1] == 1.0) and np.all(y[mid, 2] == 0.0)
            # the ends, clamped: t = 0 reads c[0], c[0], c[1]
            assert y[0, 1] == 0.5 and y[T - 1, 1] == 0.5 and y[1, 1] == 1.0
            assert y[0, 2] == 0.25 * 0 - 0.5 * 0 + 0.25 * 2 and y[1, 2] == 0.25 * 0 - 0.5 * 1 + 0.25 * 3
        assert np.all(np.abs(y[mid, 1] - 1.0) <= bound1) and np.all(np.abs(y[mid, 2]) <= bound2)


@needs_ld
@pytest.mark.parametrize("n_mels,n_ceps", [(23, 13), (80, 80), (128, 40), (128, 0), (1, 1)])
def test_host_form_under_the_gate(n_mels, n_ceps):
    L = R.logmel(n_mels)
    for cmvn in ("none", "mean", "mean_var"):
        for order, N in ((0, 2), (1, 2), (2, 1), (2, 2), (2, 5)):
            for T in (300, 70):
                kw = dict(n_ceps=n_ceps, delta_order=order, delta_window=N, cmvn=cmvn)
                R.gate(J.mfcc_host, L[:T], "host", **kw)
                y = J.mfcc_host(L[:T], J.mfcc(f64=True, **kw))
                y32 = J.mfcc_host(L[:T], J.mfcc(**kw))
                assert y32.dtype == np.float32 and np.array_equal(y32, y.astype(np.float32))
    R.gate(J.mfcc_host, L[:129], "host", n_ceps=n_ceps, delta_order=2, cmvn="mean_var", lifter=0.0, var_floor=0.5)


def test_no_dct_no_deltas_no_cmvn_is_the_log_mel_itself():
    L = R.logmel(23)
    assert np.array_equal(J.mfcc_host(L, J.mfcc(n_ceps=0, f64=True)), L)
    assert np.array_equal(J.mfcc_host(L, J.mfcc(n_ceps=0)), L.astype(np.float32))
    # and column block 0 of any order without CMVN
    assert np.array_equal(J.mfcc_host(L, J.mfcc(n_ceps=0, delta_order=2, f64=True))[:, :23], L)


def test_units_of_no_frame_and_of_one():
    L = R.logmel(23)
    for cmvn in ("none", "mean", "mean_var"):
        for order in (0, 1, 2):
            o = J.mfcc(delta_order=order, cmvn=cmvn, f64=True)
            assert J.mfcc_host(np.zeros((0, 23)), o).shape == (0, 13 * (order + 1))
            y = J.mfcc_host(L[20:21], o)
            assert y.shape == (1, 13 * (order + 1))
            # one frame: every clamped neighbour is the frame itself and s_q sums to nothing but its rounding
            assert np.all(np.abs(y[:, 13:]) <= 1e-15 * np.abs(y[:, :13]).max() + 0.0)
            if cmvn == "none":
                assert np.array_equal(y[:, :13], J.mfcc_host(L[20:21], J.mfcc(f64=True)))
            else:
                assert np.all(y == 0.0)  # c - mu is exactly 0, and 0 / sqrt(floor) under MEAN_VAR
    # T = 0 writes nothing: a null buffer of no byte is enough
    o = J.mfcc()
    assert J.lib().jb_mfcc_host(None, 0, 23, C.byref(o), None, 0) == 0


def test_pcm_host_is_the_host_form_on_the_filterbanks_f64_logarithms():
    from tests import fbank_ref

    hz = 16000
    wl, hop, _ = fbank_ref.geometry(hz)
    x = fbank_ref.gate_signal(hz, 30 * hop + wl + 5)
    for center in (False, True):
        for unit in (False, True):
            L = J.fbank_host(x, hz, J.fbank(n_mels=40, center=center, unit=unit, f64=True))
            o = J.mfcc(delta_order=2, cmvn="mean_var")
            y = J.mfcc_pcm_host(x, hz, J.fbank(n_mels=40, center=center, unit=unit), o)
            assert J.mfcc_geometry(hz, J.fbank(n_mels=40, center=center), o, x.size) == (L.shape[0], 39, L.shape[0] * 39 * 4)
            assert y.dtype == np.float32 and np.array_equal(y, J.mfcc_host(L, o))
    assert J.mfcc_pcm_host(x[:wl - 1], hz, J.fbank(n_mels=40), J.mfcc()).shape == (0, 13)


def test_cmvn_sums_in_blocks_of_64_frames():
    """The mean's order is the rule's: block sums of 64 frames from 0.0, the block sums in order, times (double)(1 / T).
    Restated here in float64, operation for operation, and held bit for bit."""
    L = R.logmel(23)
    for T in (1, 2, 63, 64, 65, 129, 300):
        c = L[:T]
        tot = np.zeros(23)
        for t0 in range(0, T, 64):
            acc = np.zeros(23)
            for t in range(t0, min(T, t0 + 64)):
                acc = acc + c[t]
            tot = tot + acc
        mu = tot * np.float64(LD(1) / LD(T))
        assert np.array_equal(J.mfcc_host(c, J.mfcc(n_ceps=0, cmvn="mean", f64=True)), c - mu[None, :]), T

"""The convolution stage without a GPU: the host rule (jb_fir_host) against the long-double sum and against its own
restatement in Python, the identity bit for bit, the four delays, utterances shorter than the response, every refusal
with the utterance and the field in jb_last_error, the struct layout against ctypes, and the device seam's answer on a
machine without a device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from tests import fir_ref as R

ROOT = Path(__file__).resolve().parent.parent
INVALID, DEVICE, BUFFER = -1, -3, -8


def signal(n, seed=1):
    rng = np.random.default_rng(seed)
    return np.round(rng.standard_normal(n) * 6000.0, 3)


def response(k, seed=2):
    rng = np.random.default_rng(seed + k)
    return rng.standard_normal(k) * np.exp(-np.arange(k) / max(1.0, k / 4.0))


def test_error_codes_are_the_headers():
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    for name, val in (("JB_ERR_INVALID", INVALID), ("JB_ERR_DEVICE", DEVICE), ("JB_ERR_BUFFER", BUFFER)):
        assert f"#define {name} {val}" in hdr or f"{name} = {val}" in hdr, name


@pytest.mark.parametrize("k", [1, 2, 7, 64, 255, 256, 257, 700])
def test_host_rule_against_the_long_double_sum(k):
    """Every fused term rounds a partial sum that is at most ||h||_1 max|x| once, by at most 2^-53 of it: K roundings,
    so e <= K 2^-53."""
    for n in (1, 5, k - 1, k, k + 1, 901):
        if n < 1:
            continue
        x, h = signal(n), response(k)
        for d in R.delays(k):
            y = J.fir_host(x, J.fir(h, 48000, d))
            assert y.shape == x.shape
            e = R.rel_err(y, R.direct_ld(x, h, d), x, h)
            assert e <= k * 2.0 ** -53, (k, n, d, e)


@pytest.mark.parametrize("k,n", [(1, 1), (1, 9), (2, 1), (2, 7), (5, 3), (5, 4), (5, 33), (17, 16), (17, 40), (33, 1)])
def test_host_rule_is_its_restatement_bit_for_bit(k, n):
    x, h = signal(n, seed=k), response(k)
    x[::3] = -0.0  # (signed zeros take part in the first term's product)
    for d in R.delays(k):
        got = J.fir_host(x, J.fir(h, 16000, d))
        assert got.tobytes() == R.host_rule(x, h, d).tobytes(), (k, n, d)


def test_the_identity_is_bit_for_bit():
    x = signal(5001)
    x[10], x[11], x[12] = -0.0, 5e-324, -1.7976931348623157e308
    y = J.fir_host(x, J.fir([1.0], 48000))
    assert y.tobytes() == x.tobytes()
    assert J.fir_host(x, None).tobytes() == x.tobytes()                  # no response: the samples themselves
    assert J.fir_host(x, J.fir(None, 48000)).tobytes() == x.tobytes()
    assert J.fir_host(np.zeros(0), J.fir([1.0, 2.0], 48000)).size == 0
    # a delayed unit tap shifts: y[n] = x[n + d - 2] with h = [0, 0, 1]
    y = J.fir_host(x, J.fir([0.0, 0.0, 1.0], 48000, 2))
    assert np.array_equal(y, x)
    y = J.fir_host(x, J.fir([0.0, 0.0, 1.0], 48000, 0))
    assert np.array_equal(y[2:], x[:-2]) and np.all(y[:2] == 0.0)


def test_terms_outside_the_utterance_are_skipped_not_multiplied():
    """With the largest finite tap next to the edge a product with a zero from outside would still be 0, but a skipped
    term leaves the sign of a first product alone: h[k] x = -0.0 stays -0.0."""
    x = np.array([-0.0, 3.0])
    y = J.fir_host(x, J.fir([2.0, 5.0], 8000, 0))
    assert np.signbit(y[0]) and y[0] == 0.0  # the one term in range: 2.0 * -0.0
    assert y[1] == 2.0 * 3.0 + 5.0 * -0.0


def refused(call):
    with pytest.raises(J.JbError) as e:
        call()
    assert "JB_ERR_INVALID" in str(e.value)
    return str(e.value)


def test_every_refusal_names_the_utterance_and_the_field():
    x = np.zeros(8)
    ok = J.fir([0.5, 0.25], 8000, 1)

    def with_fields(**kw):
        f = J.fir([1.0, 0.5, 0.25], 8000, 1)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    nan, inf = J.fir([1.0, float("nan")], 8000), J.fir([float("-inf")], 8000)
    big = J.fir(np.zeros(F.FIR_MAX_TAPS + 1), 8000)
    cases = [(with_fields(n_taps=0), "n_taps is 0"), (big, "n_taps is above JB_FIR_MAX_TAPS"),
             (nan, "taps holds a value that is not finite"), (inf, "taps holds a value that is not finite"),
             (with_fields(delay=3), "delay must be below n_taps"), (with_fields(delay=7), "delay must be below n_taps"),
             (with_fields(hz=16000), "hz differs"), (with_fields(reserved=1), "reserved must be 0")]
    for f, what in cases:
        # through the device seam: refused before any device is touched
        msg = refused(lambda: J.fir_pcm([x, x, x], [ok, None, f], 8000))
        assert "jb_fir_pcm_batch: utterance 2: " + what in msg, msg
        msg = refused(lambda: J.fir_pcm([x, x], [f, ok], 8000, i16=True))
        assert "jb_fir_pcm_batch_i16: utterance 0: " + what in msg, msg
        if "hz" not in what:  # (the host rule has no rate of its own to hold f.hz against)
            msg = refused(lambda: J.fir_host(x, f))
            assert "jb_fir_host: utterance 0: " + what in msg, msg
    # the rate is each utterance's own
    msg = refused(lambda: J.fir_pcm([x, x], [ok, ok], [8000, 16000]))
    assert "utterance 1: hz differs" in msg and "8000 Hz against 16000 Hz" in msg
    # taps == NULL with a count
    ghost = J.fir(None, 8000)
    ghost.n_taps = 4
    assert "taps is NULL" in refused(lambda: J.fir_host(x, ghost))
    # the largest response passes the check (and the host rule runs it)
    assert J.fir_host(np.ones(3), J.fir(np.ones(F.FIR_MAX_TAPS), 8000, 0)).tolist() == [1.0, 2.0, 3.0]
    # a buffer that is too small
    L = J.lib()
    dp = C.POINTER(C.c_double)
    y = np.zeros(4)
    assert L.jb_fir_host(x.ctypes.data_as(dp), 8, C.byref(ok), y.ctypes.data_as(dp), 4) == BUFFER


def test_struct_layout_header_vs_ctypes(tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(jb_fir), offsetof(jb_fir, taps), offsetof(jb_fir, n_taps),'
                   ' offsetof(jb_fir, hz), offsetof(jb_fir, delay), offsetof(jb_fir, reserved));'
                   'printf("%u %u %u %u\\n", JB_FIR_MAX_TAPS, JB_FIR_DIRECT_MAX, JB_FIR_DIRECT, JB_FIR_PARTITIONED);'
                   "return 0;}\n")
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got[:6] == [C.sizeof(F.Fir), F.Fir.taps.offset, F.Fir.n_taps.offset, F.Fir.hz.offset,
                           F.Fir.delay.offset, F.Fir.reserved.offset] == [24, 0, 8, 12, 16, 20]
        assert got[6:] == [F.FIR_MAX_TAPS, F.FIR_DIRECT_MAX, F.FIR_DIRECT, F.FIR_PARTITIONED]


def test_the_request_keeps_its_taps_and_copies_of_them():
    taps = [1.0, -2.0, 3.0]
    f = J.fir(taps, 22050, 1)
    assert (f.n_taps, f.hz, f.delay, f.reserved) == (3, 22050, 1, 0) and [f.taps[i] for i in range(3)] == taps
    arr, n = F.fir_array([f, None, f])
    assert n == 3 and arr[1].n_taps == 0 and not arr[1].taps and arr[2].taps[2] == 3.0
    arr, n = F.fir_array(f, 4)
    assert n == 4 and all(arr[i].n_taps == 3 for i in range(4))


def test_entries_without_a_device():
    L = J.lib()
    assert L.jb_batch_set_fir(None, None, 0) == INVALID
    assert L.jb_batch_fir_geometry(None, 0, None, None, None) == INVALID
    assert L.jb_engine_set_fir(None, None) == INVALID
    L.jb_fir_free(None)
    if L.jb_device_count() > 0:
        return
    x = np.zeros(4)
    for i16 in (False, True):
        with pytest.raises(J.JbError) as e:
            J.fir_pcm([x], J.fir([1.0, 0.5], 8000), 8000, i16=i16)
        assert "JB_ERR_DEVICE" in str(e.value)

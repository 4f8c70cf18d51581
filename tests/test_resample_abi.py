"""Output-rate conversion at the boundary, without a GPU: the new symbols, the filter jb_resample_filter hands out
(L, M, ntaps, the taps against an independent numpy evaluation of the formula in include/jbonsai_amd.h, the quality of
the design), the unsupported-pair error, and the engine's output-rate setter."""
import ctypes as C
import re
import shutil
import subprocess
from math import gcd
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests.conftest import VOICE

ROOT = Path(__file__).resolve().parent.parent
HIPCC = "/opt/rocm/bin/hipcc"
UNSUPPORTED = -2
NEW_SYMBOLS = ["jb_batch_set_output_rate", "jb_batch_output_rate", "jb_batch_read_pcm_native", "jb_resample_filter",
               "jb_resample_pcm_batch", "jb_engine_set_output_sampling_frequency",
               "jb_engine_get_output_sampling_frequency", "jb_resample_geometry"]

# (in, out, L, M, ntaps)
PAIRS = [
    (48000, 8000, 1, 6, 428),
    (48000, 16000, 1, 3, 214),
    (48000, 22050, 147, 320, 156),
    (48000, 24000, 1, 2, 144),
    (48000, 44100, 147, 160, 78),
    (48000, 96000, 2, 1, 72),
    (22050, 48000, 320, 147, 72),
    (16000, 44100, 441, 160, 72),
    (44100, 8000, 80, 441, 392),
    # the pairs of tests/resample_ref.py that are not above: every path of k_resample, the largest L, M and ntaps
    (48000, 32000, 2, 3, 108),
    (16000, 48000, 3, 1, 72),
    (48000, 25000, 25, 48, 138),
    (48000, 1500, 1, 32, 2276),
    (48000, 11025, 147, 640, 310),
    (44100, 48000, 160, 147, 72),
    (8000, 44100, 441, 80, 72),
    (48000, 1000, 1, 48, 3414),
    (48000, 400, 1, 120, 8534),
    (2048, 1, 1, 2048, 145636),
    (1, 2048, 2048, 1, 72),
    (2048, 2047, 2047, 2048, 72),
]


def prototype(in_hz, out_hz):
    """h[p][j] straight from the definition, in numpy (its own sinc and I0)."""
    g = gcd(in_hz, out_hz)
    L, M = out_hz // g, in_hz // g
    r = min(1.0, L / M)
    fc = 0.45 * r
    H = 32.0 / (2.0 * fc)
    C_ = int(np.ceil(H))
    p = np.arange(L)[:, None]
    j = np.arange(2 * C_)[None, :]
    t = p / L + C_ - 1 - j
    inside = np.abs(t) < H
    w = np.i0(10.0 * np.sqrt(np.clip(1.0 - (t / H) ** 2, 0.0, None))) / np.i0(10.0)
    h = np.where(inside, 2.0 * fc * np.sinc(2.0 * fc * t) * w, 0.0)
    return L, M, C_, h


def test_symbols_exported_and_mirrored():
    L = J.lib()
    for s in NEW_SYMBOLS:
        assert s in _ffi.SYMBOLS, s
        assert hasattr(L, s), s


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b, *_ in PAIRS])
def test_filter_table(pair):
    in_hz, out_hz, L0, M0, nt0 = pair
    L, M, taps = J.resample_filter(in_hz, out_hz)
    assert (L, M, taps.shape) == (L0, M0, (L0, nt0))
    L1, M1, C_, ref = prototype(in_hz, out_hz)
    assert (L1, M1, 2 * C_) == (L0, M0, nt0)
    assert np.max(np.abs(taps - ref)) <= 1e-14
    # every phase has unit DC gain (the windowed sinc at its own cutoff)
    assert np.max(np.abs(taps.sum(axis=1) - 1.0)) <= 1e-5


def test_pairs_hold_every_case_of_the_path_tests():
    from tests import resample_ref as R

    assert {(c.in_hz, c.out_hz, c.L, c.M, c.ntaps) for c in R.CASES} <= set(PAIRS)


def test_filter_buffer_and_counts_only():
    l_, m_, nt = C.c_uint32(), C.c_uint32(), C.c_uint32()
    L = J.lib()
    assert L.jb_resample_filter(48000, 16000, C.byref(l_), C.byref(m_), C.byref(nt), None, 0) == 0
    assert (l_.value, m_.value, nt.value) == (1, 3, 214)
    small = np.zeros(213)
    assert L.jb_resample_filter(48000, 16000, None, None, None, small.ctypes.data_as(C.POINTER(C.c_double)),
                                small.size) == -8


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b, *_ in PAIRS])
def test_prototype_quality(pair):
    """The prototype's response on the input-rate axis: flat to +-0.001 dB up to 0.8 of the output Nyquist, at most
    -95 dB from the output Nyquist up (what the device's sine test then sees through the polyphase)."""
    in_hz, out_hz = pair[:2]
    L, M, taps = J.resample_filter(in_hz, out_hz)
    # the prototype at L x the input rate: phases interleaved back, gain L
    ntaps = taps.shape[1]
    proto = np.zeros(L * ntaps)
    for p in range(L):
        proto[p::L] = taps[p][::-1]  # h(p/L + C - 1 - j) sits at fine-grid point p + L (C - 1 - j), shifted by L C
    n = 1 << 20
    resp = np.abs(np.fft.rfft(proto, n))
    f = np.fft.rfftfreq(n, d=1.0 / (L * in_hz))  # Hz at the prototype's rate
    nyq_out = min(in_hz, out_hz) / 2.0
    pb = resp[f <= 0.8 * nyq_out] / L
    sb = resp[(f >= nyq_out) & (f <= L * in_hz / 2.0)] / L
    assert np.max(np.abs(20 * np.log10(pb))) <= 0.001
    assert 20 * np.log10(np.max(sb)) <= -95.0


def test_unsupported_pair_says_why():
    with pytest.raises(J.JbError) as ei:
        J.resample_filter(44100, 44099)
    assert ei.value.code == UNSUPPORTED
    assert "2048" in str(ei.value)
    with pytest.raises(J.JbError):
        J.resample_filter(48000, 0)


def test_engine_output_rate_setter_getter_and_copy():
    eng = J.Engine.load([VOICE])
    c = eng.condition
    assert c.get_output_sampling_frequency() == 0
    c.set_output_sampling_frequency(16000)
    assert c.get_output_sampling_frequency() == 16000
    L = J.lib()
    h = C.c_void_p()
    assert L.jb_engine_new(eng._h, eng._h, C.byref(h)) == 0
    try:
        assert L.jb_engine_get_output_sampling_frequency(h) == 16000
    finally:
        L.jb_engine_free(h)
    c.set_output_sampling_frequency(0)
    assert c.get_output_sampling_frequency() == 0
    # the pitch-conversion rate is another field
    assert c.get_sampling_frequency() == 48000


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_kernel_resources_and_scalar_taps(tmp_path):
    """k_resample (f64 and i16 outputs): no scratch, and the taps of the inner loop are SGPR operands of the FMAs (a
    wave-uniform scalar load), not a vector load per lane."""
    src = ROOT / "jbonsai_amd" / "csrc" / "jb_resample.hip"
    out = tmp_path / "rs.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
                        "--cuda-device-only", "-S", str(src), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
                       check=True, capture_output=True, text=True, cwd=src.parent)
    report = r.stderr
    names = re.findall(r"Function Name: (\S+)", report)
    kernels = [n for n in names if "k_resample" in n]
    assert len(kernels) == 2, names
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report)]
    spills = [int(x) for x in re.findall(r"(?:VGPRs|SGPRs) Spill: (\d+)", report)]
    assert scratch and all(s == 0 for s in scratch), report
    assert all(s == 0 for s in spills), report
    asm = out.read_text()
    fmas = re.findall(r"v_fmac?_f64\S*\s+([^\n]+)", asm)
    assert fmas
    assert sum(1 for f in fmas if re.search(r"\bs\[\d+:\d+\]", f)) >= len(fmas) // 2, fmas[:8]

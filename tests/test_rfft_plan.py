"""The packed real transform, the mel bank and the table images that the filterbank, mel spectrogram and convolution
stages share (jbonsai_amd/csrc/jb_rfft.h, jb_melbank.h, the class caches of jb_host.h) on the host, without a GPU: a
probe of its own (tests/plan/rfft_probe.cpp) built with the host pass of hipcc against the built library, which holds
the stages' tables."""
import json
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import fbank_ref, melspec_ref as R
from tests.test_output_plan import CSRC, ROOT

HIPCC = "/opt/rocm/bin/hipcc"
LIBDIR = ROOT / "jbonsai_amd"
LD = np.longdouble

pytestmark = pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = Path(tmp_path_factory.mktemp("rfft_plan")) / "rfft_probe"
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
           "-Wno-unused-result", "-I", str(CSRC), "-x", "hip", str(ROOT / "tests" / "plan" / "rfft_probe.cpp"),
           "-L", str(LIBDIR), "-ljbonsai_amd", "-Wl,-rpath," + str(LIBDIR), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, *args, stdin=""):
    r = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def doubles(bits):
    return np.array(struct.unpack(f"<{len(bits)}d", struct.pack(f"<{len(bits)}Q", *bits)), dtype=np.float64)


def frame(N, seed):
    return 9000.0 * np.random.default_rng(seed).standard_normal(N)


def powers(exe, x):
    return run(exe, "power", x.size, stdin=" ".join(float(v).hex() for v in x) + "\n")


@pytest.mark.parametrize("N", [64, 128, 4096])  # log2(M) odd, even, the largest
def test_generic_path_is_the_stage_indexed_one_bit_for_bit(probe, N):
    """An all-2 schedule through rfft_frame_power against the radix-2 loop indexed by stage that the filterbank's host
    frame used to run: the same twiddles (W_M^p of the whole circle is entry 2 p of the n_fft table, the same long double
    quotient) and the same places (digit reversal in radix 2 is bit reversal), so the same bits."""
    for seed in (1, 2, 3):
        p = powers(probe, frame(N, 100 * N + seed))
        assert len(p["generic"]) == N // 2 + 1 and p["generic"] == p["stage"]


@pytest.mark.skipif(not R.have_long_double(), reason="needs an extended-precision long double")
@pytest.mark.parametrize("N", [90, 120, 400, 3888])  # 2 3^2 5, 2^3 3 5, 2^4 5^2, 2^4 3^5
def test_mixed_radix_power_within_the_gate_of_a_long_double_dft(probe, N):
    """melspec_ref's measure with the identity for a bank: e(X) = max_k |S_X[k] - S_ld[k]| / sum_k S_ld[k], held to
    GATE times e of numpy's float64 transform of the same frame."""
    x = frame(N, N)
    p = powers(probe, x)
    assert p["stage"] == []
    c, s = R._dft_ld(N)
    re, im = x.astype(LD) @ c, x.astype(LD) @ s
    S_ld = (re * re + im * im)[None, :]
    total = S_ld.sum(axis=1)
    X = np.fft.rfft(x)
    e64 = R.rel_err((X.real * X.real + X.imag * X.imag)[None, :], S_ld, total, LD(1))
    e = R.rel_err(doubles(p["generic"])[None, :], S_ld, total, LD(1))
    print(f"n_fft {N}: e {e:.3e}, e(float64 rfft) {e64:.3e}, ratio {e / e64:.2f}")
    assert 0 < e64 < 1e-14 and e <= R.GATE * e64


def check_bank(p, n_mels):
    """The by-bin form against the dense matrix: W[m][k] is wr[k] on the rising part of filter m's support and wf[k] on
    its falling part, 0 outside it; wts is the support's slice; no other entry of wr or wf is set."""
    assert p["ok"] and len(p["W"]) == n_mels == len(p["first"]) == len(p["count"]) == len(p["rise"]) == len(p["woff"])
    K = p["K"]
    assert len(p["wr"]) == K == len(p["wf"])
    wr, wf = [0] * K, [0] * K
    at = 0
    for m, row in enumerate(p["W"]):
        first, count, rise = p["first"][m], p["count"][m], p["rise"][m]
        assert [k for k, _ in row] == list(range(first, first + count)) and rise <= count  # (0 outside the support)
        assert p["woff"][m] == at and p["wts"][at:at + count] == [w for _, w in row]
        at += count
        for k, w in row:
            side = wr if k < first + rise else wf
            assert side[k] == 0  # (a bin rises in one filter at most, and falls in one at most)
            side[k] = w
    assert at == len(p["wts"]) and wr == p["wr"] and wf == p["wf"]


@pytest.mark.parametrize("shape", fbank_ref.SHAPES)
def test_fbank_bank_by_bin_is_the_dense_matrix(probe, shape):
    check_bank(run(probe, "fbank", *shape), shape[1])


@pytest.mark.parametrize("shape", R.SHAPES)
def test_melspec_bank_by_bin_is_the_dense_matrix(probe, shape):
    check_bank(run(probe, "mel", *shape[:5], int(shape[5])), shape[4])


def test_words_is_the_size_of_the_image_bind_makes(probe):
    """Each class cache: words(), which sizes the device block, against the image bind filled for it; the classes'
    pointers lie inside the image; a rate or a response seen twice is one class."""
    p = run(probe, "words")
    for name, classes in (("fbank", 3), ("melspec", 2), ("fir", 3)):
        words, image, n, inside = p[name]
        assert words == image > 0 and n == classes and inside, name

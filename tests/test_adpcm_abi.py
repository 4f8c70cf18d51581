"""IMA ADPCM on the host, without a GPU (jbonsai_amd/csrc/jb_adpcm.cpp): the options' layout, the geometry, the host
encoder and decoder against the pure-Python model (tests/adpcm_ref.py) byte for byte, the coder against audioop where
Python still has it, the WAV writer, and the quality gate of the block-local start index against the carried one."""
import ctypes as C
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import adpcm_ref as R

ROOT = Path(__file__).resolve().parent.parent
INVALID = -1
ALIGNS = (32, 256, 1024)  # spb = 57, 505, 2041


def lengths(spb):
    return [0, 1, 2, 8, 9, spb - 1, spb, spb + 1, 2 * spb + 3]


def signals(n, seed):
    """name -> n float64 samples in 16-bit scale"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    odd = np.array([40000.7, -40000.7, 32767.999, -32768.999, 32768.0, -32769.0, 12.999, -12.999, 0.999, -0.999,
                    1e9, -1e9, 100.001, -100.001])
    return {
        "silence": np.zeros(n),
        "square": np.where((k // 4) % 2 == 0, 32767.0, -32768.0),
        "ramp": 0.01 * k,
        "odd": odd[rng.integers(0, odd.size, n)],
        "noise": rng.standard_normal(n) * 8000.0,
    }


def test_opts_layout(tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){'
                   'printf("%zu %zu %zu\\n", sizeof(jb_adpcm_opts), offsetof(jb_adpcm_opts, block_align), '
                   'offsetof(jb_adpcm_opts, reserved));return 0;}\n')
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == [16, 0, 4]
    assert C.sizeof(_ffi.AdpcmOpts) == 16 and _ffi.AdpcmOpts.reserved.offset == 4
    assert "adpcm" not in _ffi.FORMATS  # a stage of its own, no sixth sample format


@pytest.mark.parametrize("hz,A,spb", [(8000, 256, 505), (16000, 256, 505), (22050, 512, 1017), (44100, 1024, 2041),
                                      (48000, 1024, 2041), (22049, 256, 505), (44099, 512, 1017)])
def test_geometry_by_rate(hz, A, spb):
    for n in (0, 1, spb - 1, spb, spb + 1, 10 * spb, 10 * spb + 1, 123457):
        nb = -(-n // spb)
        assert J.adpcm_geometry(hz, n) == (A, spb, nb, nb * A) == R.geometry(hz, n)
    assert J.adpcm_geometry(hz, 0)[3] == 0


def test_geometry_explicit_and_bad_options():
    assert J.adpcm_geometry(48000, 58, 32) == (32, 57, 2, 64)
    assert J.adpcm_geometry(8000, 1, 8192) == (8192, 16377, 1, 8192)
    L = J.lib()
    for bad in (4, 8196, 30, 28, 33, 8194):
        assert L.jb_adpcm_geometry(8000, bad, 10, None, None, None, None) == INVALID
        with pytest.raises(J.JbError):
            J.adpcm_encode_host(np.zeros(10), 8000, bad)
    assert L.jb_adpcm_geometry(8000, 32, 10, None, None, None, None) == 0  # every out pointer may be null
    x = np.zeros(10)
    out = np.zeros(256, dtype=np.uint8)
    for word in range(3):
        o = _ffi.adpcm_opts(0)
        o.reserved[word] = 1
        assert L.jb_adpcm_encode_host(x.ctypes.data, 10, 8000, C.byref(o), out.ctypes.data, 256) == INVALID
    o = _ffi.adpcm_opts(0)
    assert L.jb_adpcm_encode_host(x.ctypes.data, 10, 8000, None, out.ctypes.data, 256) == INVALID
    assert L.jb_adpcm_encode_host(x.ctypes.data, 10, 8000, C.byref(o), out.ctypes.data, 255) == -8  # JB_ERR_BUFFER
    assert L.jb_adpcm_encode_host(x.ctypes.data, 10, 8000, C.byref(o), out.ctypes.data, 256) == 0


@pytest.mark.parametrize("A", ALIGNS)
def test_host_encoder_and_decoder_are_the_model(A):
    spb = 2 * (A - 4) + 1
    for i, n in enumerate(lengths(spb)):
        for name, x in signals(n, 100 * A + i).items():
            want = R.encode(x, 8000, A)
            got = J.adpcm_encode_host(x, 8000, A)
            assert len(got) == -(-n // spb) * A
            assert got == want, (A, n, name)
            s16 = np.array(R.quantise(x), dtype=np.int16)
            assert J.adpcm_encode_host(s16, 8000, A) == got, (A, n, name)
            dec = J.adpcm_decode_host(got, A, n)
            assert dec.tobytes() == R.decode(got, A, n).tobytes(), (A, n, name)
            # the first sample of every block is exact
            assert np.array_equal(dec[::spb], s16[::spb]), (A, n, name)


def test_signals_reach_the_rails():
    """The square wave drives idx to 88 and the predictor into its clamp, the ramp drives idx to 0."""
    n = 2 * 505 + 3
    tr = []
    R.encode(signals(n, 0)["square"], 8000, 256, trace=tr)
    assert max(i for _, i in tr) == 88 and {32767, -32768} <= {p for p, _ in tr}
    tr = []
    R.encode(signals(n, 0)["ramp"], 8000, 256, trace=tr)
    assert min(i for _, i in tr) == 0


def test_default_block_align_follows_the_rate():
    x = signals(3000, 5)["noise"]
    for hz, A in ((8000, 256), (22050, 512), (48000, 1024)):
        assert J.adpcm_encode_host(x, hz) == R.encode(x, hz) == J.adpcm_encode_host(x, hz, A)


def test_decoder_arguments():
    L = J.lib()
    data = np.frombuffer(J.adpcm_encode_host(np.zeros(58), 8000, 32), dtype=np.uint8)
    out = np.zeros(58, dtype=np.int16)
    assert L.jb_adpcm_decode_host(data.ctypes.data, 64, 32, 58, out.ctypes.data, 58) == 0
    assert L.jb_adpcm_decode_host(data.ctypes.data, 64, 32, 58, out.ctypes.data, 57) == -8
    assert L.jb_adpcm_decode_host(data.ctypes.data, 32, 32, 58, out.ctypes.data, 58) == INVALID  # a block short
    assert L.jb_adpcm_decode_host(data.ctypes.data, 64, 30, 58, out.ctypes.data, 58) == INVALID
    assert L.jb_adpcm_decode_host(data.ctypes.data, 64, 0, 58, out.ctypes.data, 58) == INVALID


def test_coder_is_audioop():
    audioop = pytest.importorskip("audioop")
    x = signals(57, 9)["noise"]
    s = R.quantise(x)
    for i0 in (0, 20, 47, 88):
        blk = R.encode(x, 8000, 32, force_i0=i0)
        assert blk[2] == i0
        ours = [c for by in blk[4:] for c in (by & 15, by >> 4)]
        frag = np.array(s[1:], dtype="<i2").tobytes()
        theirs, _ = audioop.lin2adpcm(frag, 2, (s[0], i0))
        assert ours == [c for by in theirs for c in (by >> 4, by & 15)]  # audioop packs the first code high


@pytest.mark.parametrize("hz,A,n", [(8000, 256, 1234), (48000, 1024, 5000), (16000, 32, 0), (22050, 512, 1017)])
def test_wav(tmp_path, hz, A, n):
    x = signals(n, 3)["noise"]
    data = J.adpcm_encode_host(x, hz, A)
    path = tmp_path / "a.wav"
    J.write_wav_adpcm(path, data, n, hz, A)
    raw = path.read_bytes()
    spb = 2 * (A - 4) + 1
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and struct.unpack_from("<I", raw, 4)[0] == len(raw) - 8
    fmt_len, tag, ch, rate, byte_rate, align, bits, cb, wspb = struct.unpack_from("<IHHIIHHHH", raw, 16)
    assert (fmt_len, tag, ch, rate, byte_rate, align, bits, cb, wspb) == (20, 0x11, 1, hz, hz * A // spb, A, 4, 2, spb)
    assert raw[40:44] == b"fact" and struct.unpack_from("<II", raw, 44) == (4, n)
    assert raw[52:56] == b"data" and struct.unpack_from("<I", raw, 56)[0] == len(data) == len(raw) - 60
    assert raw[60:] == data
    assert R.decode(raw[60:], A, n).tobytes() == J.adpcm_decode_host(data, A, n).tobytes()
    with pytest.raises(J.JbError):  # the bytes are not the geometry's
        J.write_wav_adpcm(path, data + bytes(A), n, hz, A)


@pytest.mark.parametrize("fs,A", [(8000, 256), (16000, 256), (48000, 1024)])
def test_block_local_start_costs_no_quality(fs, A):
    """decode(encode) with the block-local start index against the carried-index encoder on the speech-like signal:
    at least its SNR minus 0.5 dB.  The model gives 13.02 / 24.81 / 43.53 dB block-local against 13.01 / 24.91 /
    43.50 dB carried at 8 / 16 / 48 kHz."""
    x = R.speech_like(fs)
    local = J.adpcm_decode_host(J.adpcm_encode_host(x, fs), A, x.size)
    carried = J.adpcm_decode_host(R.encode(x, fs, carry=True), A, x.size)
    snr_local, snr_carried = R.snr_db(x, local), R.snr_db(x, carried)
    print(f"{fs} Hz / A = {A}: block-local {snr_local:.2f} dB, carried {snr_carried:.2f} dB")
    assert snr_local >= snr_carried - 0.5

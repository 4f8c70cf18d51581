"""Output sample formats, host side (no GPU): the symbols, the jb_format_opts layout, the refusals that need no batch,
the numpy references themselves (tests/g711_ref.py against audioop), jb_format_pcm_host against tests/format_ref.py
bit for bit in every format, the dither, the identities that tie the formats to the 16-bit sink's rule, and the WAV
headers.  (The refusals of jb_batch_set_format need a batch, so a device: tests/test_gpu_format.py has them.)"""
import ctypes as C
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import format_ref as R
from tests.g711_ref import alaw2lin, lin2alaw, lin2ulaw, ulaw2lin

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["jb_format_bytes_per_sample", "jb_batch_set_format", "jb_batch_formatted_size",
               "jb_batch_read_formatted", "jb_batch_read_formatted_all", "jb_format_pcm_batch", "jb_format_pcm_host",
               "jb_format_free", "jb_synthesize_formatted", "jb_synthesize_batch_formatted",
               "jb_synthesize_batch_each_formatted", "jb_write_wav_formatted"]
ALL16 = np.arange(-32768, 32768, dtype=np.int16)


def test_symbols_declared_exported_and_mirrored():
    L = J.lib()
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _ffi.SYMBOLS, s
        assert hasattr(L, s), s


def test_opts_layout_and_bytes_per_sample():
    assert C.sizeof(_ffi.FormatOpts) == 16
    assert _ffi.FormatOpts.dither.offset == 4 and _ffi.FormatOpts.seed.offset == 8
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    assert "sizeof(jb_format_opts) == 16" in hdr and "offsetof(jb_format_opts, seed) == 8" in hdr
    L = J.lib()
    for name, val in (("F32", 1), ("S16", 2), ("S24", 3), ("ULAW", 4), ("ALAW", 5)):
        assert re.search(rf"#define JB_FMT_{name} {val}u", hdr) and getattr(_ffi, "FMT_" + name) == val
    assert [L.jb_format_bytes_per_sample(f) for f in (0, 1, 2, 3, 4, 5, 6, 99)] == [0, 4, 2, 3, 1, 1, 0, 0]
    assert {k: L.jb_format_bytes_per_sample(v) for k, v in _ffi.FORMATS.items()} == R.BYTES


def host_rc(fmt, dither, x=None, out=None, cap=None, opts_null=False):
    L = J.lib()
    x = np.zeros(4) if x is None else x
    out = np.zeros(64, dtype=np.uint8) if out is None else out
    o = _ffi.FormatOpts(fmt, dither, 0)
    return L.jb_format_pcm_host(x.ctypes.data, x.size, None if opts_null else C.byref(o), out.ctypes.data,
                                out.size if cap is None else cap)


def test_refusals_without_a_device():
    L = J.lib()
    for fmt in (0, 6, 255):  # unknown format
        assert host_rc(fmt, 0) == -1
    for fmt in (_ffi.FMT_F32, _ffi.FMT_ULAW, _ffi.FMT_ALAW):  # dither with F32 or G.711
        assert host_rc(fmt, _ffi.DITHER_TPDF) == -1
    assert host_rc(_ffi.FMT_S16, 2) == -1  # unknown dither
    assert host_rc(_ffi.FMT_S16, 0, opts_null=True) == -1  # null pointers
    o = _ffi.FormatOpts(_ffi.FMT_S16, 0, 0)
    out = np.zeros(64, dtype=np.uint8)
    assert L.jb_format_pcm_host(None, 4, C.byref(o), out.ctypes.data, 64) == -1
    assert L.jb_format_pcm_host(np.zeros(4).ctypes.data, 4, C.byref(o), None, 64) == -1
    assert L.jb_format_pcm_host(None, 0, C.byref(o), None, 0) == 0  # nothing to do
    for fmt, nb in ((_ffi.FMT_F32, 4), (_ffi.FMT_S16, 2), (_ffi.FMT_S24, 3), (_ffi.FMT_ULAW, 1)):  # a short cap
        assert host_rc(fmt, 0, cap=4 * nb - 1) == -8 and host_rc(fmt, 0, cap=4 * nb) == 0
    # the device seam and the engine entries decide the same before any device is looked for (there may be none)
    x = np.zeros(4)
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    ins, nin = (dp * 1)(x.ctypes.data_as(dp)), (C.c_size_t * 1)(4)
    bufs, ns = (u8p * 1)(), (C.c_size_t * 1)()
    for fmt, d in ((0, 0), (9, 0), (_ffi.FMT_F32, 1), (_ffi.FMT_ALAW, 1), (_ffi.FMT_S24, 3)):
        o = _ffi.FormatOpts(fmt, d, 0)
        assert L.jb_format_pcm_batch(ins, nin, 1, C.byref(o), -1, bufs, ns) == -1
        assert L.jb_synthesize_batch_formatted(None, None, None, 0, -1, C.byref(o), bufs, ns) == -1
        assert L.jb_synthesize_batch_each_formatted(None, None, None, 0, -1, C.byref(o), bufs, ns) == -1
        assert L.jb_synthesize_formatted(None, None, 0, C.byref(o), bufs, ns) == -1
    assert L.jb_format_pcm_batch(ins, nin, 1, None, -1, bufs, ns) == -1
    assert L.jb_synthesize_batch_formatted(None, None, None, 0, -1, None, bufs, ns) == -1
    assert L.jb_batch_set_format(None, C.byref(o)) == -1
    assert L.jb_write_wav_formatted(b"/nonexistent-dir/x.wav", None, 0, 8000, 0) == -1
    assert L.jb_write_wav_formatted(None, None, 0, 8000, _ffi.FMT_S16) == -1


def test_g711_reference_is_audioop():
    audioop = pytest.importorskip("audioop")
    raw = ALL16.astype("<i2").tobytes()
    assert lin2ulaw(ALL16).tobytes() == audioop.lin2ulaw(raw, 2)
    assert lin2alaw(ALL16).tobytes() == audioop.lin2alaw(raw, 2)
    codes = np.arange(256, dtype=np.uint8)
    assert ulaw2lin(codes).astype("<i2").tobytes() == audioop.ulaw2lin(codes.tobytes(), 2)
    assert alaw2lin(codes).astype("<i2").tobytes() == audioop.alaw2lin(codes.tobytes(), 2)


def test_g711_codes_and_round_trip():
    """Mu-law never emits 0x7F; encode(decode(c)) == c for the other 255 mu-law codes and for all 256 A-law codes --
    through the library's host seam."""
    codes = np.arange(256, dtype=np.uint8)
    mu = np.frombuffer(J.format_pcm_host(ALL16.astype(np.float64), "ulaw"), dtype=np.uint8)
    assert 0x7F not in set(mu.tolist()) and len(set(mu.tolist())) == 255
    back = np.frombuffer(J.format_pcm_host(ulaw2lin(codes).astype(np.float64), "ulaw"), dtype=np.uint8)
    assert (back != codes).nonzero()[0].tolist() == [0x7F]
    back = np.frombuffer(J.format_pcm_host(alaw2lin(codes).astype(np.float64), "alaw"), dtype=np.uint8)
    assert back.tobytes() == codes.tobytes()


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_host_seam_is_the_reference(fmt):
    """Every integer of the 16-bit range with seven offsets, beyond the range, both zeros, a subnormal, float32 ties."""
    got = J.format_pcm_host(R.VALUES, fmt)
    want = R.encode(R.VALUES, fmt)
    assert len(got) == R.VALUES.size * R.BYTES[fmt]
    assert got == want, np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[:8]


def tpdf_input(n, scale):
    rng = np.random.default_rng(1234)
    x = rng.uniform(-40000.0, 40000.0, n)
    x[:4096] = rng.integers(-32768, 32768, 4096) + rng.choice([0.0, 0.5, -0.5, 0.25], 4096)
    return x / scale


@pytest.mark.parametrize("fmt,scale", [("s16", 1.0), ("s24", 256.0)])
def test_tpdf_is_the_reference(fmt, scale):
    n = 100_000
    x = tpdf_input(n, scale)
    outs = []
    for seed in (0, 0xDEADBEEFCAFEF00D):
        got = J.format_pcm_host(x, fmt, dither=True, seed=seed)
        assert got == R.encode(x, fmt, dither_on=True, seed=seed), seed
        outs.append(got)
    assert outs[0] != outs[1] and outs[0] != J.format_pcm_host(x, fmt)
    # the dither itself: in (-1, 1), triangular (variance 1/6 LSB^2), zero mean
    d = R.dither(7, n)
    assert -1.0 < d.min() and d.max() < 1.0 and abs(d.mean()) < 0.01 and abs(d.var() - 1 / 6) < 0.005


@pytest.mark.parametrize("fmt,scale", [("s16", 1.0), ("s24", 256.0)])
def test_tpdf_carries_a_sub_lsb_level(fmt, scale):
    """A constant 0.3 LSB: the dithered output's mean is 0.3 within 0.01 LSB (standard error ~0.002 at n = 100,000);
    without dither it is 0."""
    x = np.full(100_000, 0.3 / scale)

    def level(data):
        return (np.frombuffer(data, "<i2") if fmt == "s16" else R.decode_s24(data)).mean()
    for seed in (1, 99):
        assert abs(level(J.format_pcm_host(x, fmt, dither=True, seed=seed)) - 0.3) < 0.01
    assert level(J.format_pcm_host(x, fmt)) == 0.0


def test_identities():
    v = R.VALUES
    s16 = np.frombuffer(J.format_pcm_host(v, "s16"), "<i2")
    assert s16.tobytes() == np.clip(v, -32768, 32767).astype(np.int16).tobytes()
    s24 = R.decode_s24(J.format_pcm_host(v, "s24"))
    assert np.array_equal(np.trunc(s24 / 256.0).astype(np.int64), s16.astype(np.int64))
    f32 = np.frombuffer(J.format_pcm_host(v, "f32"), "<f4")
    assert f32.tobytes() == (v / 32768).astype(np.float32).tobytes()
    # the zeros keep their signs
    z = np.frombuffer(J.format_pcm_host(np.array([0.0, -0.0]), "f32"), "<u4")
    assert z.tolist() == [0, 0x80000000]


def chunks(data):
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    out, pos = [], 12
    while pos < len(data):
        tag, n = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        out.append((tag, data[pos + 8:pos + 8 + n]))
        pos += 8 + n + (n & 1)
    assert pos == len(data)
    return out


@pytest.mark.parametrize("fmt,n", [("s16", 1001), ("s24", 1001), ("s24", 1000), ("f32", 333)])
def test_wav_pcm_and_float_read_back(tmp_path, fmt, n):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    x = np.random.default_rng(5).uniform(-33000, 33000, n)
    data = J.format_pcm_host(x, fmt)
    path = tmp_path / f"{fmt}.wav"
    J.write_wav_formatted(path, data, 22050, fmt)
    hz, got = wavfile.read(str(path))
    assert hz == 22050 and got.shape == (n,)
    if fmt == "s16":
        assert got.dtype == np.int16 and got.tobytes() == data
    elif fmt == "f32":
        assert got.dtype == np.float32 and got.tobytes() == data
    else:  # 24 bits arrive left-justified in int32
        assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64) >> 8, R.decode_s24(data))
    raw = path.read_bytes()
    tags = [t for t, _ in chunks(raw)]
    assert tags == ([b"fmt ", b"fact", b"data"] if fmt == "f32" else [b"fmt ", b"data"])
    assert len(raw) % 2 == 0


@pytest.mark.parametrize("fmt,tag", [("ulaw", 7), ("alaw", 6)])
@pytest.mark.parametrize("n", [0, 8, 9])
def test_wav_g711_header(tmp_path, fmt, tag, n):
    x = np.linspace(-30000, 30000, n)
    data = J.format_pcm_host(x, fmt)
    path = tmp_path / "g711.wav"
    J.write_wav_formatted(path, data, 8000, fmt)
    raw = path.read_bytes()
    (t0, fm), (t1, fact), (t2, body) = chunks(raw)
    assert (t0, t1, t2) == (b"fmt ", b"fact", b"data")
    # tag, channels, rate, byte rate, block align, bits, cbSize
    assert struct.unpack("<HHIIHHH", fm) == (tag, 1, 8000, 8000, 1, 8, 0)
    assert struct.unpack("<I", fact) == (n,)
    assert body == data
    assert len(raw) == 12 + 26 + 12 + 8 + n + (n & 1) and (n % 2 == 0 or raw[-1] == 0)

"""FLAC output, host side (no GPU): the symbols, the jb_flac_opts layout and its checks, and the test decoder
(tests/flac_ref.py) itself -- its CRCs against the known answers, and streams built here by a bit writer that it
must accept, or reject after a single corruption."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests.flac_ref import FlacError, crc8, crc16, decode

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["jb_batch_set_flac", "jb_batch_flac_size", "jb_batch_read_flac", "jb_batch_read_flac_all",
               "jb_flac_encode_pcm_batch", "jb_flac_free", "jb_synthesize_flac", "jb_synthesize_batch_flac",
               "jb_synthesize_batch_each_flac"]


def test_symbols_declared_exported_and_mirrored():
    L = J.lib()
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _ffi.SYMBOLS, s
        assert hasattr(L, s), s


def test_opts_layout_matches_the_header():
    assert C.sizeof(_ffi.FlacOpts) == 16
    assert _ffi.FlacOpts.max_lpc_order.offset == 4 and _ffi.FlacOpts.reserved.offset == 8
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    assert "sizeof(jb_flac_opts) == 16" in hdr and "offsetof(jb_flac_opts, reserved) == 8" in hdr


@pytest.mark.parametrize("bs,order,res", [(15, 8, 0), (4609, 8, 0), (1, 0, 0), (4096, 13, 0), (0, 13, 0),
                                          (4096, 8, 1), (0, 0, 7)])
def test_bad_options_are_invalid_without_a_device(bs, order, res):
    L = J.lib()
    o = _ffi.FlacOpts()
    o.block_size, o.max_lpc_order = bs, order
    o.reserved[1] = res
    x = (C.c_int16 * 4)(1, 2, 3, 4)
    ins = (C.POINTER(C.c_int16) * 1)(C.cast(x, C.POINTER(C.c_int16)))
    nin = (C.c_size_t * 1)(4)
    bufs, ns = (C.POINTER(C.c_uint8) * 1)(), (C.c_size_t * 1)()
    # JB_ERR_INVALID, decided before any device is looked for (this machine may have none)
    assert L.jb_flac_encode_pcm_batch(ins, nin, 1, 48000, C.byref(o), -1, bufs, ns) == -1
    assert L.jb_synthesize_batch_flac(None, None, None, 0, -1, C.byref(o), bufs, ns) == -1


def test_crc_known_answers():
    assert crc8(b"123456789") == 0xF4
    assert crc16(b"123456789") == 0xFEE8


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, nbits, val):
        self.v = (self.v << nbits) | (val & ((1 << nbits) - 1))
        self.n += nbits

    def align(self):
        if self.n % 8:
            self.put(8 - self.n % 8, 0)

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


def frame(number, samples, kind, rate_code=10, order=0, rice=None):
    """One frame by the book: header (block size 8-bit extra, rate code, 16 bits), one subframe, padding, CRC-16."""
    n = len(samples)
    h = BitWriter()
    h.put(14, 0x3FFE), h.put(1, 0), h.put(1, 0), h.put(4, 6), h.put(4, rate_code)
    h.put(4, 0), h.put(3, 4), h.put(1, 0)
    h.put(8, number)  # < 128
    h.put(8, n - 1)
    hb = h.bytes()
    w = BitWriter()
    for b in hb + bytes([crc8(hb)]):
        w.put(8, b)
    if kind == "constant":
        w.put(8, 0), w.put(16, samples[0])
    elif kind == "verbatim":
        w.put(8, 1 << 1)
        for s in samples:
            w.put(16, s)
    else:  # FIXED order with Rice partitions: rice = [(param, None) or ("esc", bits)] per partition, order p
        w.put(8, (8 + order) << 1)
        for s in samples[:order]:
            w.put(16, s)
        p = {1: 0, 2: 1, 4: 2}[len(rice)]
        w.put(2, 0), w.put(4, p)
        c = {0: [], 1: [1], 2: [2, -1]}[order]
        res = [samples[i] - sum(c[j] * samples[i - 1 - j] for j in range(order)) for i in range(order, n)]
        plen, k0 = n >> p, 0
        for j, (k, nb) in enumerate(rice):
            m = plen - (order if j == 0 else 0)
            part, k0 = res[k0:k0 + m], k0 + m
            if k == "esc":
                w.put(4, 15), w.put(5, nb)
                for e in part:
                    w.put(nb, e)
            else:
                w.put(4, k)
                for e in part:
                    u = 2 * e if e >= 0 else -2 * e - 1
                    w.put((u >> k) + 1, 1)
                    w.put(k, u)
    w.align()
    body = w.bytes()
    return body + crc16(body).to_bytes(2, "big")


def stream(frames, bs, total, rate=48000):
    sizes = [len(f) for f in frames]
    v = (rate << 44) | (0 << 41) | (15 << 36) | total
    si = (bs.to_bytes(2, "big") * 2 + (min(sizes) if sizes else 0).to_bytes(3, "big")
          + (max(sizes) if sizes else 0).to_bytes(3, "big") + v.to_bytes(8, "big") + bytes(16))
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + si + b"".join(frames)


def sample_stream():
    a = [3, -7, 100, 32767, -32768, 0, 5, 5, 9, -1, 2, 4, 8, 16, 32, 64]
    b = [1234] * 16
    c = [i * i - 50 for i in range(16)]
    fr = [frame(0, a, "verbatim"), frame(1, b, "constant"),
          frame(2, c, "fixed", order=2, rice=[(1, None), ("esc", 6)]), frame(3, c[:12], "fixed", order=1,
                                                                              rice=[(3, None)])]
    return stream(fr, 16, 16 * 3 + 12), a + b + c + c[:12], fr


def test_decoder_accepts_streams_built_by_the_book():
    data, want, _ = sample_stream()
    got, info = decode(data)
    np.testing.assert_array_equal(got, np.array(want, dtype=np.int16))
    assert info["types"] == ["verbatim", "constant", "fixed2", "fixed1"]
    empty, info = decode(stream([], 4096, 0))
    assert empty.size == 0 and info["total"] == 0


def flip(data, byte, bit):
    b = bytearray(data)
    b[byte] ^= 1 << bit
    return bytes(b)


def test_decoder_rejects_single_corruptions():
    data, _, fr = sample_stream()
    f1 = 42 + len(fr[0])  # second frame's first byte
    with pytest.raises(FlacError, match="CRC-16"):
        decode(flip(data, 42 + len(fr[0]) - 1, 0))  # a bit of the first frame's CRC-16
    with pytest.raises(FlacError, match="CRC-8|reserved"):
        decode(flip(data, f1 + 1, 1))  # the reserved bit after the sync code
    with pytest.raises(FlacError):
        decode(flip(data, f1 + 3, 0))  # the reserved bit after the sample size
    skipped = stream([fr[0], frame(2, [1234] * 16, "constant")] + fr[2:], 16, 16 * 3 + 12)
    with pytest.raises(FlacError, match="frame number"):
        decode(skipped)
    with pytest.raises(FlacError, match="total samples"):
        decode(stream(fr, 16, 16 * 3 + 11))
    with pytest.raises(FlacError, match="MD5"):
        decode(flip(data, 41, 0))

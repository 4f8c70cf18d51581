"""FLAC metadata, host side (no GPU): the symbols, the jb_flac_meta layout and its checks, jb_md5_host against RFC
1321's test suite and hashlib, jb_flac_seek_geometry against a restatement of the rule, and the test's own stream
splitter (tests/flac_meta_ref.py) on streams built here."""
import ctypes as C
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests.flac_meta_ref import check, split
from tests.flac_ref import FlacError, decode
from tests.test_flac_abi import sample_stream

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["jb_batch_set_flac_meta", "jb_flac_encode_pcm_batch_meta", "jb_flac_md5_pcm_batch", "jb_md5_host",
               "jb_flac_seek_geometry", "jb_synthesize_flac_meta", "jb_synthesize_batch_flac_meta",
               "jb_synthesize_batch_each_flac_meta"]


def test_symbols_declared_exported_and_mirrored():
    L = J.lib()
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _ffi.SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+JB_FLAC_MD5\s+1u", hdr) and _ffi.FLAC_MD5 == 1


def test_meta_layout_matches_the_header():
    assert C.sizeof(_ffi.FlacMeta) == 16
    assert _ffi.FlacMeta.flags.offset == 0 and _ffi.FlacMeta.seek_interval_ms.offset == 4
    assert _ffi.FlacMeta.reserved.offset == 8
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    assert "sizeof(jb_flac_meta) == 16" in hdr and "offsetof(jb_flac_meta, reserved) == 8" in hdr
    # the options' layout is untouched
    assert C.sizeof(_ffi.FlacOpts) == 16 and _ffi.FlacOpts.reserved.offset == 8


RFC1321 = [(b"", "d41d8cd98f00b204e9800998ecf8427e"), (b"a", "0cc175b9c0f1b6a831c399e269772661"),
           (b"abc", "900150983cd24fb0d6963f7d28e17f72"), (b"message digest", "f96b697d7cb7938d525a2f31aaf161d0"),
           (b"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"),
           (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"),
           (b"1234567890" * 8, "57edf4a22be3c955ac49da2e2107b67a")]


def test_md5_known_answers():
    for msg, want in RFC1321:
        assert J.md5_host(msg).hex() == want, msg


def test_md5_against_hashlib():
    rng = np.random.default_rng(1321)
    for n in list(range(201)) + [1 << 20]:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert J.md5_host(data) == hashlib.md5(data).digest(), n
    L = J.lib()
    out = C.create_string_buffer(16)
    assert L.jb_md5_host(None, 0, C.cast(out, C.c_void_p)) == 0 and out.raw.hex() == RFC1321[0][1]
    assert L.jb_md5_host(None, 4, C.cast(out, C.c_void_p)) == -1
    assert L.jb_md5_host(C.cast(out, C.c_void_p), 4, None) == -1


def geometry(n, bs, hz, ms):
    """The rule of include/jbonsai_amd.h ("SEEKTABLE"), restated."""
    nframes = -(-n // bs)
    if ms == 0 or nframes == 0:
        return 0, 0, 42
    step = max(1, (ms * hz + 500 * bs) // (1000 * bs))
    step = max(step, -(-nframes // 65535))
    points = -(-nframes // step)
    return step, points, 42 + 4 + 18 * points


def test_seek_geometry_over_a_grid():
    for bs in (16, 1152, 4096):
        for n in (0, 1, bs - 1, bs, bs + 1, 130 * bs + 5):
            for hz in (8000, 22050, 48000):
                for ms in (0, 1, 100, 1000, 10000):
                    assert J.flac_seek_geometry(n, bs, hz, ms) == geometry(n, bs, hz, ms), (n, bs, hz, ms)
    # the cap: more frames than points allowed at the rounded step
    for hz in (8000, 48000):
        step, points, hdr = J.flac_seek_geometry(70000 * 16, 16, hz, 1)
        assert (step, points, hdr) == geometry(70000 * 16, 16, hz, 1)
        assert points <= 65535 and step >= 2
    assert J.flac_seek_geometry(70000 * 16, 16, 8000, 1)[0] == 2  # rounded step 1, raised by the cap
    assert J.flac_seek_geometry(5 * 4096, 0, 48000, 1000) == geometry(5 * 4096, 4096, 48000, 1000)  # 0: 4096
    L = J.lib()
    for bad_bs in (15, 4609):
        assert L.jb_flac_seek_geometry(100, bad_bs, 48000, 100, None, None, None) == -1
    assert L.jb_flac_seek_geometry(100, 4096, 0, 100, None, None, None) == -1
    assert L.jb_flac_seek_geometry(1 << 36, 4096, 48000, 100, None, None, None) == -1
    assert L.jb_flac_seek_geometry(100, 4096, 48000, 100, None, None, None) == 0


@pytest.mark.parametrize("flags,res0,res1", [(2, 0, 0), (3, 0, 0), (0x80000000, 0, 0), (1, 1, 0), (0, 0, 9)])
def test_bad_meta_is_invalid_without_a_device(flags, res0, res1):
    L = J.lib()
    m = _ffi.FlacMeta()
    m.flags, m.seek_interval_ms = flags, 100
    m.reserved[0], m.reserved[1] = res0, res1
    x = (C.c_int16 * 4)(1, 2, 3, 4)
    ins = (C.POINTER(C.c_int16) * 1)(C.cast(x, C.POINTER(C.c_int16)))
    nin = (C.c_size_t * 1)(4)
    bufs, ns = (C.POINTER(C.c_uint8) * 1)(), (C.c_size_t * 1)()
    # JB_ERR_INVALID, decided before any device is looked for (this machine may have none)
    assert L.jb_flac_encode_pcm_batch_meta(ins, nin, 1, 48000, None, C.byref(m), -1, bufs, ns) == -1
    assert L.jb_synthesize_batch_flac_meta(None, None, None, 0, -1, None, C.byref(m), bufs, ns) == -1
    assert L.jb_synthesize_batch_each_flac_meta(None, None, None, 0, -1, None, C.byref(m), bufs, ns) == -1
    assert L.jb_synthesize_flac_meta(None, None, 0, None, C.byref(m), bufs, ns) == -1
    assert L.jb_batch_set_flac_meta(None, C.byref(m)) == -1


def with_meta(data, frames, bs, total, step, digest):
    """The stream of tests/test_flac_abi.py::stream with a digest and a SEEKTABLE of every step-th frame, by the
    book."""
    pts, off = [], 0
    for f, fr in enumerate(frames):
        if f % step == 0:
            pts.append((f * bs).to_bytes(8, "big") + off.to_bytes(8, "big") + min(bs, total - f * bs).to_bytes(2, "big"))
        off += len(fr)
    table = b"".join(pts)
    return (data[:4] + b"\x00" + data[5:26] + digest + bytes([0x83]) + len(table).to_bytes(3, "big") + table
            + data[42:])


def test_splitter_on_streams_built_by_the_book():
    data, want, fr = sample_stream()
    digest = hashlib.md5(np.array(want, dtype="<i2").tobytes()).digest()
    for step in (1, 2, 4):
        full = with_meta(data, fr, 16, len(want), step, digest)
        meta, plain = split(full)
        assert plain == data and meta["md5"] == digest and not meta["streaminfo_last"] and meta["seektable_last"]
        assert len(meta["points"]) == -(-len(fr) // step) and meta["header_bytes"] == 46 + 18 * len(meta["points"])
        got, info, _ = check(full)
        np.testing.assert_array_equal(got, np.array(want, dtype=np.int16))
        with pytest.raises(FlacError):
            decode(full)  # the strict decoder takes the plain form only
        bad = bytearray(full)
        bad[46 + 15] ^= 1  # the first point's offset
        with pytest.raises(FlacError, match="offset"):
            check(bytes(bad))
    meta, plain = split(data)  # a plain stream is its own plain form
    assert plain == data and meta["points"] is None and meta["md5"] == bytes(16) and meta["streaminfo_last"]

"""The join stage without a GPU (jbonsai_amd/csrc/jb_join.cpp): the structs' layout against the ctypes mirror, the unit
conversion, the geometry, the host seam against the numpy statement of the rules (tests/join_ref.py) bit for bit for
float64 and int16, the argument errors, and every new entry's answer on a machine without a device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import join_ref as R

ROOT = Path(__file__).resolve().parent.parent
INVALID, DEVICE, BUFFER = -1, -3, -8


def pcm_of(n, seed, i16):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 9000.0
    if n > 6:
        x[:3] = [32767.0, -32768.0, 12345.678]
        x[-3:] = [-1.0, 1.0, -32768.0]
    return np.trunc(np.clip(x, -32768, 32767)).astype(np.int16) if i16 else x


def same(a, b):
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def test_error_codes_are_the_headers():
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    for name, val in (("JB_ERR_INVALID", INVALID), ("JB_ERR_DEVICE", DEVICE), ("JB_ERR_BUFFER", BUFFER)):
        assert int(re.search(rf"\b{name} = (-?\d+)", hdr).group(1)) == val


def test_struct_layouts(tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(jb_join_utt), offsetof(jb_join_utt, programme), '
                   'offsetof(jb_join_utt, fade_in), offsetof(jb_join_utt, fade_out), offsetof(jb_join_utt, reserved), '
                   'offsetof(jb_join_utt, pad_before), offsetof(jb_join_utt, pad_after));'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(jb_join_opts), offsetof(jb_join_opts, lead_ms), '
                   'offsetof(jb_join_opts, gap_ms), offsetof(jb_join_opts, trail_ms), offsetof(jb_join_opts, fade_ms), '
                   'offsetof(jb_join_opts, reserved));printf("%u\\n", JB_JOIN_NONE);return 0;}\n')
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == [32, 0, 4, 8, 12, 16, 24, 40, 0, 8, 16, 24, 32, 0xFFFFFFFF]
    U, O = _ffi.JoinUtt, _ffi.JoinOpts
    assert [C.sizeof(U), U.programme.offset, U.fade_in.offset, U.fade_out.offset, U.reserved.offset,
            U.pad_before.offset, U.pad_after.offset] == [32, 0, 4, 8, 12, 16, 24]
    assert [C.sizeof(O), O.lead_ms.offset, O.gap_ms.offset, O.trail_ms.offset, O.fade_ms.offset,
            O.reserved.offset] == [40, 0, 8, 16, 24, 32]
    assert _ffi.JOIN_NONE == 0xFFFFFFFF


def test_ms_to_samples():
    for hz in (8000, 16000, 22050, 44100, 48000, 11025):
        for ms in (0.0, 0.01, 0.5, 1.0, 5.0, 12.3456, 500.0, 1000.0, 2999.99, 0.0113378684807):
            assert J.join_ms_to_samples(ms, hz) == R.ms_to_samples(ms, hz) == int(np.floor(ms * hz / 1000.0 + 0.5))
    assert J.join_ms_to_samples(500.0, 48000) == 24000 and J.join_ms_to_samples(5.0, 44100) == 221
    assert J.join_ms_to_samples(-3.0, 48000) == 0 and J.join_ms_to_samples(float("nan"), 48000) == 0


REQUESTS = {
    "interleaved": [(0, 3, 1, 2, 5), (1, 0, 4, 0, 0), (0, 0, 0, 7, 0), (1, 9, 0, 0, 3), (0, 2, 2, 1, 1)],
    "ids by first member": [(4, 1, 0), (2, 0, 1), (4, 0, 0), (None, 5, 6, 3, 3), (2, 0, 0)],
    "all none": [(None, 1, 2, 3, 4)] * 5,
    "one of all": [(3, 0, 0, 0, 0), (3, 0, 10, 4, 4), (3, 0, 0, 100, 100), (3, 7, 0, 1, 0), (3, 0, 0, 0, 1)],
}


@pytest.mark.parametrize("name", sorted(REQUESTS))
def test_geometry_and_numbering(name):
    req = REQUESTS[name]
    lengths = [11, 0, 64, 1, 30]
    prog_of, start, ps = J.join_geometry(req, lengths)
    _, want_of, want_start = R.join([np.zeros(n) for n in lengths], req)
    want_of2, members = R.number([r[0] for r in req])
    assert prog_of == want_of == want_of2 and start == want_start
    assert ps == [sum(req[u][1] + lengths[u] + (req[u][2] if len(req[u]) > 2 else 0) for u in m) for m in members]
    # dense numbering in the order of the first members
    seen = []
    for p in prog_of:
        if p not in seen:
            seen.append(p)
    assert seen == list(range(len(ps)))


def test_interleaved_membership_is_0_2_4_and_1_3():
    prog_of, start, ps = J.join_geometry(REQUESTS["interleaved"], [10, 20, 30, 40, 50])
    assert prog_of == [0, 1, 0, 1, 0]
    assert start == [3, 0, 3 + 10 + 1, 20 + 4 + 9, 14 + 30 + 2] and ps == [3 + 10 + 1 + 30 + 2 + 50 + 2, 20 + 4 + 9 + 40]


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("name", sorted(REQUESTS))
def test_host_seam_is_the_model(name, i16):
    req = REQUESTS[name]
    for lengths in ([11, 0, 64, 1, 30], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [200, 3, 7, 150, 2]):
        pcms = [pcm_of(n, 10 * n + u, i16) for u, n in enumerate(lengths)]
        want, _, _ = R.join(pcms, req)
        got = J.join_host(pcms, req)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert same(g, w), (name, lengths)


@pytest.mark.parametrize("i16", [False, True])
def test_fades_every_length_against_every_fade(i16):
    """fade_in + fade_out > n is allowed: both weights on one sample, in that order."""
    for n in (1, 2, 3, 8, 17):
        x = pcm_of(n, n, i16)
        for fin in (0, 1, 2, n, n + 5):
            for fout in (0, 1, 2, n, n + 5):
                (got,) = J.join_host([x], [(None, 1, 2, fin, fout)])
                want = np.concatenate([np.zeros(1, x.dtype), R.member(x, fin, fout), np.zeros(2, x.dtype)])
                assert same(got, want), (n, fin, fout)


def test_samples_outside_the_fades_keep_their_bits():
    x = np.array([np.nan, -0.0, 5e-324, 1e300, -np.inf, 3.25, 7.5, 1.0], dtype=np.float64)
    x[0] = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]  # a NaN payload
    (got,) = J.join_host([x], [(None, 0, 0, 2, 2)])
    assert got[2:6].tobytes() == x[2:6].tobytes()
    (plain,) = J.join_host([x], [(None, 3, 0)])
    assert plain[3:].tobytes() == x.tobytes() and not plain[:3].any()
    # the weights themselves: the first and the last of a fade of 4
    one = np.full(8, 1.0)
    (w,) = J.join_host([one], [(None, 0, 0, 4, 4)])
    t = np.array([1, 3, 5, 7]) / 8.0
    assert np.array_equal(w[:4], (t * t) * (3.0 - 2.0 * t)) and np.array_equal(w[4:], w[:4][::-1])


def test_int16_products_truncate_toward_zero():
    x = np.array([-32768, 32767, -3, 3, -1, 1], dtype=np.int16)
    (got,) = J.join_host([x], [(None, 0, 0, 6, 0)])
    k = np.arange(6)
    t = (2 * k + 1) / 12.0
    want = np.trunc(x.astype(np.float64) * ((t * t) * (3.0 - 2.0 * t))).astype(np.int16)
    assert np.array_equal(got, want) and got[2] == -1 and got[3] == 1  # -3 s = -1.13 goes to -1, not to -2


def test_argument_errors():
    L = J.lib()
    x = np.zeros(4)
    ins = (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    nin = (C.c_size_t * 2)(4, 4)
    out = np.zeros(16)
    outs = (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data)
    caps = (C.c_size_t * 2)(16, 16)

    def call(req, caps=caps):
        return L.jb_join_host(ins, nin, 2, _ffi.join_request(req), outs, caps)

    assert call([(0,), (0,)]) == 0
    assert call([(2,), (0,)]) == INVALID and b"programme id 2" in L.jb_last_error()  # an id of n or above
    assert call([(1,), (None,)]) == 0
    bad = _ffi.join_request([(0,), (0,)])
    bad[1].reserved = 1
    assert L.jb_join_host(ins, nin, 2, bad, outs, caps) == INVALID and b"reserved" in L.jb_last_error()
    assert L.jb_join_geometry(bad, nin, None, 2, None, None, None, None) == INVALID
    assert call([(0, 5), (0, 0, 4)], (C.c_size_t * 2)(16, 16)) == BUFFER  # 5 + 4 + 4 + 4 = 17 samples
    assert call([(0, 5), (0, 0, 3)], (C.c_size_t * 2)(16, 16)) == 0
    assert L.jb_join_host(None, nin, 2, _ffi.join_request([(0,), (0,)]), outs, caps) == INVALID
    # a programme of mixed rates is refused by name
    hz = (C.c_uint32 * 2)(48000, 44100)
    assert L.jb_join_geometry(_ffi.join_request([(1,), (1,)]), nin, hz, 2, None, None, None, None) == INVALID
    msg = L.jb_last_error()
    assert b"programme 1" in msg and b"output rate" in msg
    assert L.jb_join_geometry(_ffi.join_request([(1,), (0,)]), nin, hz, 2, None, None, None, None) == 0
    # every out pointer of the geometry may be null; an empty request has no programme
    P = C.c_size_t(7)
    assert L.jb_join_geometry(None, None, None, 0, None, None, C.byref(P), None) == 0 and P.value == 0


def test_entries_without_a_device():
    """Null handles are refused; the entries that need the GPU say JB_ERR_DEVICE on a machine without one, and the
    argument errors come first."""
    L = J.lib()
    assert L.jb_batch_set_join(None, None, 0) == INVALID
    assert L.jb_batch_num_outputs(None) == 0 and L.jb_batch_programme_of(None, 0) == -1
    assert L.jb_batch_programme_layout(None, 0, None, None, None) == INVALID
    assert L.jb_batch_member_start(None, 0, None) == INVALID
    assert L.jb_batch_read_programme_pcm(None, 0, None, 0) == INVALID
    assert L.jb_batch_read_programme_pcm_i16(None, 0, None, 0) == INVALID
    L.jb_join_free(None)
    # the engine entries check their options before anything else
    out, n = C.c_void_p(), C.c_size_t()
    buf = C.POINTER(C.c_uint8)()
    off = (C.c_size_t * 2)(0, 0)
    j = _ffi.join_opts(1.0, 2.0, 3.0, 4.0)
    assert L.jb_synthesize_programme(None, None, off, 1, -1, None, C.byref(out), C.byref(n), None) == INVALID
    for field in ("lead_ms", "gap_ms", "trail_ms", "fade_ms"):
        bad = _ffi.join_opts(1.0, 2.0, 3.0, 4.0)
        setattr(bad, field, -1.0)
        assert L.jb_synthesize_programme_i16(None, None, off, 1, -1, C.byref(bad), C.byref(out), C.byref(n),
                                             None) == INVALID
        setattr(bad, field, float("nan"))
        assert L.jb_synthesize_programme_formatted(None, None, off, 1, -1, C.byref(_ffi.format_opts("s16")),
                                                   C.byref(bad), C.byref(buf), C.byref(n), None) == INVALID
    bad = _ffi.join_opts()
    bad.reserved[1] = 1
    assert L.jb_synthesize_programme_adpcm(None, None, off, 1, -1, C.byref(_ffi.adpcm_opts()), C.byref(bad),
                                           C.byref(buf), C.byref(n), None, None) == INVALID
    assert L.jb_synthesize_programme(None, None, off, 0, -1, C.byref(j), C.byref(out), C.byref(n), None) == INVALID
    assert b"at least one utterance" in L.jb_last_error()
    assert L.jb_synthesize_programme_flac_meta(None, None, off, 1, -1, None, None, C.byref(j), C.byref(buf),
                                               C.byref(n), None) == INVALID  # (a null engine)
    if L.jb_device_count() > 0:
        return
    x = np.zeros(4)
    ins, nin = (C.c_void_p * 1)(x.ctypes.data), (C.c_size_t * 1)(4)
    outs, ns, P = (C.c_void_p * 1)(), (C.c_size_t * 1)(), C.c_size_t()
    req = _ffi.join_request([(None, 1, 1)])
    assert L.jb_join_pcm_batch(ins, nin, 1, req, -1, outs, ns, C.byref(P)) == DEVICE
    assert L.jb_join_pcm_batch_i16(ins, nin, 1, req, -1, outs, ns, C.byref(P)) == DEVICE
    # ... and the argument errors before the device
    assert L.jb_join_pcm_batch(ins, nin, 1, _ffi.join_request([(5,)]), -1, outs, ns, C.byref(P)) == INVALID

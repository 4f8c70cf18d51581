"""The mix stage without a GPU (jbonsai_amd/csrc/jb_mix.cpp): the structs' layout against the ctypes mirror, the gain,
the geometry, the host seam against the numpy statement of the rule (tests/mix_ref.py) bit for bit for float64 and
int16, the host seam against jb_join_host on join-shaped requests, the fit, every refusal with its message, and every
new entry's answer on a machine without a device."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import mix_ref as M

ROOT = Path(__file__).resolve().parent.parent
INVALID, UNSUPPORTED, DEVICE, BUFFER = -1, -2, -3, -8
NINF = -math.inf
# tests/test_gpu_join.py's lengths and pads
LENGTHS = [0, 1, 7, 8, 63, 64, 65, 4095, 4096, 4097]
PADS = [0, 1, 3, 4097]


def pcm_of(n, seed, i16):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 9000.0 + 0.25
    if n > 6:
        x[:3] = [32767.0, -32768.0, 12345.678]
        x[-3:] = [-1.0, 1.0, -32768.0]
    return np.trunc(np.clip(x, -32768, 32767)).astype(np.int16) if i16 else x


def same(a, b):
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def gains_of(req):
    return [J.mix_gain(r[2]) for r in M.norm(req)]


def check_host(pcms, req, fit=False, ceiling_db=0.0):
    """jb_mix_host is mix_ref: the programmes, the peak, the scale, the depth and the overlap"""
    opts = _ffi.mix_opts(fit, ceiling_db)
    got, reps = J.mix_host(pcms, req, opts)
    gains = gains_of(req)
    c = 32768.0 * math.pow(10.0, ceiling_db / 20.0)
    want, _, peaks, scales, _ = M.mix(pcms, req, gains, fit, c)
    _, _, ns, depth, overlap = M.geometry([np.asarray(x).size for x in pcms], req, gains)
    assert len(got) == len(want) == len(reps)
    for p, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (p, g.size, w.size, np.flatnonzero(g[:min(g.size, w.size)] != w[:min(g.size, w.size)])[:8])
        assert (reps[p].peak, reps[p].scale, reps[p].depth, reps[p].overlap, reps[p].reserved) == \
            (peaks[p], scales[p], depth[p], overlap[p], 0), p
    return got, reps


def test_error_code_of_an_unsupported_request_is_the_headers():
    import re
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    assert int(re.search(r"\bJB_ERR_UNSUPPORTED = (-?\d+)", hdr).group(1)) == UNSUPPORTED


def test_struct_layouts(tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(jb_mix_utt), offsetof(jb_mix_utt, programme), '
                   'offsetof(jb_mix_utt, fade_in), offsetof(jb_mix_utt, fade_out), offsetof(jb_mix_utt, reserved), '
                   'offsetof(jb_mix_utt, start), offsetof(jb_mix_utt, pad_after), offsetof(jb_mix_utt, gain_db), '
                   'offsetof(jb_mix_utt, reserved2));'
                   'printf("%zu %zu %zu %zu\\n", sizeof(jb_mix_opts), offsetof(jb_mix_opts, flags), '
                   'offsetof(jb_mix_opts, reserved), offsetof(jb_mix_opts, ceiling_db));'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(jb_mix_report), offsetof(jb_mix_report, peak), '
                   'offsetof(jb_mix_report, scale), offsetof(jb_mix_report, depth), offsetof(jb_mix_report, reserved), '
                   'offsetof(jb_mix_report, overlap));'
                   'printf("%zu %zu %zu\\n", sizeof(jb_mix_place), offsetof(jb_mix_place, start_ms), '
                   'offsetof(jb_mix_place, gain_db));printf("%u %u\\n", JB_MIX_NONE, JB_MIX_FIT);return 0;}\n')
    want = [48, 0, 4, 8, 12, 16, 24, 32, 40, 16, 0, 4, 8, 32, 0, 8, 16, 20, 24, 16, 0, 8, 0xFFFFFFFF, 1]
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == want
    U, O, R, P = _ffi.MixUtt, _ffi.MixOpts, _ffi.MixReport, _ffi.MixPlace
    assert [C.sizeof(U), U.programme.offset, U.fade_in.offset, U.fade_out.offset, U.reserved.offset, U.start.offset,
            U.pad_after.offset, U.gain_db.offset, U.reserved2.offset] == want[:9]
    assert [C.sizeof(O), O.flags.offset, O.reserved.offset, O.ceiling_db.offset] == want[9:13]
    assert [C.sizeof(R), R.peak.offset, R.scale.offset, R.depth.offset, R.reserved.offset, R.overlap.offset] == want[13:19]
    assert [C.sizeof(P), P.start_ms.offset, P.gain_db.offset] == want[19:22]
    assert (_ffi.MIX_NONE, _ffi.MIX_FIT) == (0xFFFFFFFF, 1)


def test_gain():
    assert J.mix_gain(0.0) == 1.0 and J.mix_gain(-0.0) == 1.0
    g = J.mix_gain(NINF)
    assert g == 0.0 and not math.copysign(1.0, g) < 0
    for db in (-120.0, -60.0, -20.0, -6.5, -6.0, -3.0, -0.1, 1e-9, 0.1, 3.0, 6.0, 12.0, 20.0, 39.999, 40.0):
        want = 10.0 ** (db / 20.0)
        assert abs(J.mix_gain(db) - want) <= 2.0 * np.spacing(want), db
    assert J.mix_gain(-20.0) == 0.1 and J.mix_gain(20.0) == 10.0 and J.mix_gain(40.0) == 100.0


REQUESTS = {
    # (programme, start, gain_db, pad_after, fade_in, fade_out)
    "out of start order": [(0, 40, 0.0, 0, 2, 5), (1, 0, -6.5), (0, 0, 12.0, 3, 7, 0), (1, 9, 0.0, 0, 0, 3), (0, 17, -3.0)],
    "ids by first member": [(4, 1), (2, 0, 0.0, 1), (4, 0, -1.0), (None, 5, 6.0, 6, 3, 3), (2, 0)],
    "all none": [(None, 1, -2.0, 2, 3, 4)] * 5,
    "identical starts": [(3, 5, 0.0, 0, 4, 4), (3, 5, -6.5, 10, 4, 4), (3, 5), (3, 5, 12.0, 0, 100, 100), (3, 5, 0.0, 0, 0, 1)],
    "muted": [(0, 0, NINF, 90), (0, 3), (0, 4, NINF), (0, 1000, NINF, 7), (0, 6, -6.0)],
}
LENGTH_SETS = ([11, 0, 64, 1, 30], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [200, 3, 7, 150, 2])


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("name", sorted(REQUESTS))
def test_host_seam_is_the_model(name, i16):
    for lengths in LENGTH_SETS:
        check_host([pcm_of(n, 10 * n + u, i16) for u, n in enumerate(lengths)], REQUESTS[name])


@pytest.mark.parametrize("name", sorted(REQUESTS))
def test_geometry_and_numbering(name):
    req = REQUESTS[name]
    for lengths in LENGTH_SETS:
        prog_of, start, ps, depth, overlap = J.mix_geometry(req, lengths)
        want_of, members, ns, wdepth, woverlap = M.geometry(lengths, req, gains_of(req))
        assert prog_of == want_of and start == [r[1] for r in M.norm(req)]
        assert (ps, depth, overlap) == (ns, wdepth, woverlap)
        # length: the maximum reach over the members
        assert ps == [max(M.norm(req)[u][1] + lengths[u] + M.norm(req)[u][3] for u in m) for m in members]


def test_geometry_by_hand():
    # members out of start order; a muted member extends the length and counts for neither depth nor overlap
    prog_of, start, ps, depth, overlap = J.mix_geometry(
        [(0, 10, 0.0), (0, 0, 0.0), (0, 5, -3.0, 4), (0, 0, NINF, 100), (None, 2)], [10, 8, 10, 30, 3])
    assert prog_of == [0, 0, 0, 0, 1] and start == [10, 0, 5, 0, 2]
    assert ps == [130, 5] and depth == [2, 1] and overlap == [3 + 5, 0]  # [5, 8) under 1 and 2, [10, 15) under 0 and 2
    # empty members; a programme of pads alone
    _, _, ps, depth, overlap = J.mix_geometry([(0, 2, 0.0, 3)] * 3, [0, 0, 0])
    assert ps == [5] and depth == [0] and overlap == [0]
    assert J.mix_geometry([], []) == ([], [], [], [], [])


@pytest.mark.parametrize("i16", [False, True])
def test_join_shaped_requests_equal_the_join(i16):
    """tests/test_gpu_join.py's lengths, pads and fade sets turned into starts: at 0 dB the mix is the join, bit for bit"""
    lengths = LENGTHS + LENGTHS[::-1]
    pcms = [pcm_of(n, 31 * u + n, i16) for u, n in enumerate(lengths)]

    def fades(n):
        return [0, 1, 2, n, n + 5]
    req = [(0, PADS[u % 4], PADS[(u // 4) % 4], fades(n)[u % 5], fades(n)[(u + 2) % 5]) for u, n in enumerate(lengths)]
    requests = [req, [(None,) + r[1:] for r in req], [(u % 3,) + r[1:] for u, r in enumerate(req)]]
    requests += [[(0, 1, 0, fades(n)[fi], fades(n)[(fi + 3) % 5]) for n in lengths] for fi in range(5)]
    for r in requests:
        want = J.join_host(pcms, r)
        got, reps = J.mix_host(pcms, M.from_join(r, lengths))
        assert len(got) == len(want)
        for p, (g, w) in enumerate(zip(got, want)):
            assert same(g, w), p
        assert all(rep.depth <= 1 and rep.overlap == 0 and rep.scale == 1.0 for rep in reps)
        assert J.mix_geometry(M.from_join(r, lengths), lengths)[:3] == tuple(J.join_geometry(r, lengths))


def test_a_sample_under_one_member_at_0_db_keeps_its_bits():
    x = np.arange(64, dtype=np.float64)
    x[5] = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]  # a NaN payload
    x[6], x[7], x[8] = -0.0, 5e-324, -np.inf
    (got,), (rep,) = check_host([x], [(None, 3, 0.0, 0, 2, 2)])
    assert got[3 + 2:3 + 62].tobytes() == x[2:62].tobytes() and not got[:3].any()
    assert rep.peak == math.inf  # (the NaN is passed over; the infinity is not)
    # under no member the sample is +0.0
    (z,), _ = J.mix_host([np.full(4, -0.0)], [(None, 2, 0.0, 2)])
    assert z[:2].tobytes() == np.zeros(2).tobytes() and z[6:].tobytes() == np.zeros(2).tobytes()
    assert z[2:6].tobytes() == np.full(4, -0.0).tobytes()


def test_int16_members_are_not_truncated_one_by_one():
    # 0.75 + 0.75 under a fade weight: each would truncate to 0, the sum is 1
    x = np.full(4, 3, dtype=np.int16)
    (got,), _ = check_host([x, x], [(0, 0, -12.0), (0, 0, -12.0)])
    g = J.mix_gain(-12.0)
    assert int(3 * g) == 0 and got.tolist() == [int(3 * g + 3 * g)] * 4 == [1] * 4
    # without fit the 16-bit sink clamps
    big = np.full(3, 30000, dtype=np.int16)
    got, reps = check_host([big, big, -big, -big, -big], [(0, 0)] * 2 + [(1, 0)] * 3)
    assert got[0].tolist() == [32767] * 3 and got[1].tolist() == [-32768] * 3
    assert [r.peak for r in reps] == [60000.0, 90000.0]


@pytest.mark.parametrize("i16", [False, True])
def test_fit(i16):
    pcms = [pcm_of(300, 1, i16), pcm_of(200, 2, i16), pcm_of(50, 3, i16), pcm_of(40, 4, i16)]
    req = [(0, 0, 6.0, 0, 10, 10), (0, 150, 3.0), (1, 0, -30.0), (1, 10, -30.0)]
    for ceiling_db in (-1.0, -6.0, 0.0):
        c = 32768.0 * math.pow(10.0, ceiling_db / 20.0)
        got, reps = check_host(pcms, req, True, ceiling_db)
        plain, preps = J.mix_host(pcms, req)
        assert reps[0].peak > c and reps[0].scale == c / reps[0].peak < 1.0
        assert np.max(np.abs(got[0].astype(np.float64))) <= c
        # a programme under the ceiling: no bit changes; the peak is measured without the flag too
        assert reps[1].scale == 1.0 and same(got[1], plain[1])
        assert [r.peak for r in preps] == [r.peak for r in reps] and all(r.scale == 1.0 for r in preps)
        # a given scale is taken as it is, and reported
        given = [0.25, 0.5]
        forced, freps = J.mix_host(pcms, req, _ffi.mix_opts(True, ceiling_db), given)
        want, _, _, _, _ = M.mix(pcms, req, gains_of(req), True, c, given)
        assert all(same(g, w) for g, w in zip(forced, want)) and [r.scale for r in freps] == given
    if i16:  # the scale is applied in front of the sink: 2 x 30000 at -6.02 dB is 30000 +- 1, not the clamp's 32767 halved
        big = np.full(8, 30000, dtype=np.int16)
        (got,), (rep,) = J.mix_host([big, big], [(0, 0), (0, 0)], _ffi.mix_opts(True, -6.0))
        c = 32768.0 * math.pow(10.0, -6.0 / 20.0)
        assert rep.peak == 60000.0 and got.tolist() == [int(min(60000.0 * (c / 60000.0), c))] * 8


def test_refusals():
    L = J.lib()
    x = np.zeros(4)
    ins = (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    nin = (C.c_size_t * 2)(4, 4)
    out = np.zeros(16)
    outs = (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data)
    caps = (C.c_size_t * 2)(16, 16)

    def call(req, opts=None, caps=caps):
        arr = req if not isinstance(req, list) else _ffi.mix_request(req)
        return L.jb_mix_host(ins, nin, 2, arr, None if opts is None else C.byref(opts), None, outs, caps, None)

    def refused(rc, *words):
        msg = L.jb_last_error()
        return rc == INVALID and all(w in msg for w in words)

    assert call([(0,), (0,)]) == 0
    assert refused(call([(2,), (0,)]), b"jb_mix_host", b"programme id 2")  # an id of n or above
    assert call([(1,), (None,)]) == 0
    for field in ("reserved", "reserved2"):
        bad = _ffi.mix_request([(0,), (0,)])
        setattr(bad[1], field, 1)
        assert refused(call(bad), b"reserved must be 0 (utterance 1)")
        assert L.jb_mix_geometry(bad, nin, None, 2, None, None, None, None, None, None, None) == INVALID
    for db in (40.5, -120.5, math.inf, math.nan):
        assert refused(call([(0,), (0, 0, db)]), b"gain_db", b"utterance 1"), db
    assert call([(0, 0, 40.0), (0, 0, -120.0)]) == 0 and call([(0, 0, NINF), (0, 0, NINF)]) == 0
    o = _ffi.mix_opts(True, -1.0)
    assert call([(0,), (0,)], o) == 0
    o.flags = 2
    assert refused(call([(0,), (0,)], o), b"unknown flag")
    o = _ffi.mix_opts(True, -1.0)
    o.reserved = 1
    assert refused(call([(0,), (0,)], o), b"reserved must be 0")
    for cdb in (0.5, -121.0, math.nan, NINF):
        assert refused(call([(0,), (0,)], _ffi.mix_opts(True, cdb)), b"ceiling_db"), cdb
    assert call([(0,), (0,)], _ffi.mix_opts(False, 7.0)) == 0  # (read with the flag only)
    assert refused(call([(0, 2 ** 63), (0,)]), b"too long", b"utterance 0")
    assert call([(0, 5), (0, 9, 0.0, 4)], caps=(C.c_size_t * 2)(16, 16)) == BUFFER  # 9 + 4 + 4 = 17 samples
    assert call([(0, 5), (0, 9, 0.0, 3)], caps=(C.c_size_t * 2)(16, 16)) == 0
    assert L.jb_mix_host(None, nin, 2, _ffi.mix_request([(0,), (0,)]), None, None, outs, caps, None) == INVALID
    # a programme of mixed rates is refused by name
    hz = (C.c_uint32 * 2)(48000, 44100)
    assert L.jb_mix_geometry(_ffi.mix_request([(1,), (1,)]), nin, hz, 2, None, None, None, None, None, None,
                             None) == INVALID
    assert refused(INVALID, b"programme 1", b"output rate")
    assert L.jb_mix_geometry(_ffi.mix_request([(1,), (0,)]), nin, hz, 2, None, None, None, None, None, None, None) == 0
    P = C.c_size_t(7)
    assert L.jb_mix_geometry(None, None, None, 0, None, None, None, C.byref(P), None, None, None) == 0 and P.value == 0


def test_work_lists_past_their_limit_are_unsupported():
    """6000 members over one sample: the segments' lists would hold 6000 * 6001 / 2 > 2^24 entries"""
    n = 6000
    req = [(0, u) for u in range(n)]
    L = J.lib()
    with pytest.raises(J.JbError, match="2\\^24 entries"):
        J.mix_geometry(req, [n] * n)
    nin = (C.c_size_t * n)(*[n] * n)
    assert L.jb_mix_geometry(_ffi.mix_request(req), nin, None, n, None, None, None, None, None, None, None) == UNSUPPORTED
    assert J.mix_geometry(req, [100] * n)[3] == [100]  # (100 deep: 100 * 6100 entries at the most, fits)


def test_entries_without_a_device():
    L = J.lib()
    assert L.jb_batch_set_mix(None, None, 0, None) == INVALID
    assert L.jb_batch_mix_report(None, 0, None) == INVALID
    assert L.jb_engine_set_programme_mix(None, None, 0, None) == INVALID
    assert L.jb_engine_get_programme_mix(None, None, 0, None, None) == INVALID
    L.jb_mix_free(None)
    if L.jb_device_count() > 0:
        return
    x = np.zeros(4)
    ins, nin = (C.c_void_p * 1)(x.ctypes.data), (C.c_size_t * 1)(4)
    outs, ns, P = (C.c_void_p * 1)(), (C.c_size_t * 1)(), C.c_size_t()
    req = _ffi.mix_request([(None, 1, 0.0, 1)])
    assert L.jb_mix_pcm_batch(ins, nin, 1, req, None, -1, outs, ns, C.byref(P), None) == DEVICE
    assert L.jb_mix_pcm_batch_i16(ins, nin, 1, req, None, -1, outs, ns, C.byref(P), None) == DEVICE
    # ... and the argument errors before the device
    assert L.jb_mix_pcm_batch(ins, nin, 1, _ffi.mix_request([(5,)]), None, -1, outs, ns, C.byref(P), None) == INVALID
    bad = _ffi.mix_request([(None, 0, 41.0)])
    assert L.jb_mix_pcm_batch(ins, nin, 1, bad, None, -1, outs, ns, C.byref(P), None) == INVALID
    assert b"gain_db" in L.jb_last_error()

"""The stems of a mix without a GPU (jbonsai_amd/csrc/jb_mix.cpp): jb_mix_stems_host against the numpy statement of the
rule (tests/stems_ref.py) bit for bit for float64 and int16, with and without the fit; the additivity the header states
(== at a depth of at most two, the stated bound at depths 3 and 9, `depth` counts in 16 bits); jb_mix_levels_host
against the numpy statement of the summation order, bit for bit, around the tile and the partial sizes; the three dB
values against a long-double evaluation of the whole signals; the geometry; the refusals with their messages; and the
new entries' answers on a machine without a device."""
import ctypes as C
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import mix_ref as M
from tests import stems_ref as S

INVALID, DEVICE, BUFFER = -1, -3, -8
NINF = -math.inf


def pcm_of(n, seed, i16, amp=9000.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * amp + 0.25
    if n > 6 and amp >= 9000.0:
        x[:3] = [32767.0, -32768.0, 12345.678]
        x[-3:] = [-1.0, 1.0, -32768.0]
    return np.trunc(np.clip(x, -32768, 32767)).astype(np.int16) if i16 else x


def same(a, b):
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def gains_of(req):
    return [J.mix_gain(r[2]) for r in M.norm(req)]


# (programme, start, gain_db, pad_after, fade_in, fade_out); two talkers of three and two sentences, a third with one,
# an utterance of its own, a muted member and one of no samples
REQ = [(0, 0, 0.0, 0, 16, 16), (0, 1500, -3.0, 0, 0, 40), (0, 2100, 0.0, 9), (0, 4000, 6.0, 0, 64, 64), (0, 1023, 0.0),
       (0, 3000, 2.5, 100), (None, 5, 0.0, 3, 4, 4), (0, 10, NINF, 0), (0, 700, 0.0)]
LEN = [2048, 1025, 4097, 300, 1, 2000, 777, 6000, 0]
STEMS = {
    "talkers": [0, 1, 0, 1, 0, 2, None, 1, 2],
    "each its own": [0, 1, 2, 3, 4, 5, 6, 7, 8],
    "one of all": [3] * 9,
    "one member has none": [0, 1, 0, None, 0, 1, 6, None, None],
}


def check_host(pcms, req, stem_of, fit=False, ceiling_db=0.0, levels=False):
    opts = _ffi.mix_opts(fit, ceiling_db)
    got, reps, sreps = J.mix_stems_host(pcms, req, stem_of, opts, levels=levels)
    gains = gains_of(req)
    c = 32768.0 * math.pow(10.0, ceiling_db / 20.0)
    want, _, peaks, scales = S.stems(pcms, req, stem_of, gains, fit, c)
    P, st = S.number(req, stem_of)
    assert len(got) == len(want) == P + len(st) and len(reps) == P and len(sreps) == len(st)
    for p, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (p, g.size, w.size, np.flatnonzero(g[:min(g.size, w.size)] != w[:min(g.size, w.size)])[:8])
    for s, (p, _, _) in enumerate(st):
        assert (sreps[s].peak, sreps[s].scale) == (peaks[P + s], scales[p]), s
    # the programmes are jb_mix_host's
    plain, preps = J.mix_host(pcms, req, opts)
    for p in range(P):
        assert same(plain[p], got[p]) and (preps[p].peak, preps[p].scale) == (reps[p].peak, reps[p].scale)
    return got, reps, sreps


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("name", sorted(STEMS))
def test_host_seam_is_the_model(name, i16):
    pcms = [pcm_of(n, 40 + u, i16) for u, n in enumerate(LEN)]
    check_host(pcms, REQ, STEMS[name])
    got, reps, sreps = check_host(pcms, REQ, STEMS[name], fit=True, ceiling_db=-6.0)
    assert reps[0].scale < 1.0  # (the fit is at work in programme 0)


def test_geometry():
    g = J.mix_stems_geometry(REQ, STEMS["talkers"], LEN)
    assert g["P"] == 2 and g["U"] == 5 and g["stem_unit"] == [2, 3, 2, 3, 2, 4, -1, 3, 4]
    assert g["samples"] == [6206, 785, 6206, 6206, 6206] and g["programme"] == [0, 1, 0, 0, 0]
    assert g["stem_id"] == [_ffi.MIX_NO_STEM, _ffi.MIX_NO_STEM, 0, 1, 2] and g["members"] == [8, 1, 3, 3, 2]
    assert g["first"] == [0, 0, 0, 1500, 3000] and g["end"] == [6206, 785, 6197, 4300, 5000]
    assert g["depth"][2:] == [2, 1, 1]
    gains = gains_of(REQ)
    for s, (_, _, mem) in enumerate(S.number(REQ, STEMS["talkers"])[1]):
        assert S.extent(REQ, LEN, gains, mem) == (g["first"][2 + s], g["end"][2 + s])


def test_a_fitted_stem_is_not_clamped():
    """Two talkers in antiphase: the mixture is quiet, each stem loud.  Under the fit the mixture is scaled to the
    ceiling and each stem by the same scale, above the ceiling, unclamped in f64; the 16-bit sink clamps"""
    n = 3000
    a = pcm_of(n, 1, False)
    b = -0.9 * a
    b[100] = 20000.0  # (one sample where the two add up: the programme's peak)
    a[100] = 12000.0
    req = [(0, 0, 6.0), (0, 0, 6.0)]
    got, reps, sreps = check_host([a, b], req, [0, 1], fit=True, ceiling_db=-12.0)
    c = 32768.0 * 10 ** (-12 / 20)
    assert reps[0].scale < 1.0 and np.abs(got[0]).max() <= c
    assert np.abs(got[1]).max() > c and sreps[0].peak * reps[0].scale > c
    a[100] = b[100] = 6000.0
    ai, bi = [np.trunc(np.clip(x, -32768, 32767)).astype(np.int16) for x in (a, b)]
    got, reps, sreps = check_host([ai, bi], req, [0, 1], fit=True, ceiling_db=-6.0)
    assert reps[0].scale < 1.0 and sreps[0].peak * reps[0].scale > 32767.0
    assert got[1].max() == 32767 and got[1].min() == -32768  # the sink's clamp alone


def test_a_stem_of_one_member_at_0_db_keeps_its_bits():
    x = pcm_of(500, 3, False)
    x[7] = -0.0
    x[9] = np.float64(5e-324)
    y = pcm_of(500, 4, False)
    got, _, _ = J.mix_stems_host([x, y], [(0, 40, 0.0, 0, 8, 8), (0, 0, 0.0)], [1, 0])
    assert same(got[1][40 + 8:40 + 492], x[8:492])  # outside its fades
    assert not got[1][:40].any() and not np.signbit(got[1][:40]).any() and not got[1][540:].any()


def overlapped(depth, n, i16, amp, talkers=None):
    """`depth` members, all over samples [depth, n): starts 0, 1, 2, ...; one stem each, or `talkers` stems taking
    the members in turn"""
    pcms = [pcm_of(n + depth - u, 70 + u, i16, amp) for u in range(depth)]
    req = [(0, u, [0.0, -2.0, 3.5][u % 3]) for u in range(depth)]
    return pcms, req, [u % (talkers or depth) for u in range(depth)]


@pytest.mark.parametrize("depth", [1, 2, 3, 9])
def test_additivity_in_f64(depth):
    # (one stem per member, added in unit order, is the mixture's own association: == at every depth)
    pcms, req, stem_of = overlapped(depth, 2500, False, 9000.0)
    got, reps, _ = J.mix_stems_host(pcms, req, stem_of)
    assert reps[0].depth == depth and reps[0].scale == 1.0
    total = got[1].copy()
    for s in got[2:]:
        total = total + s  # in unit order
    assert np.array_equal(total, got[0])
    if depth <= 2:
        return
    # two talkers taking the members in turn: the stems associate the terms otherwise than the mixture does
    pcms, req, stem_of = overlapped(depth, 2500, False, 9000.0, talkers=2)
    got, reps, _ = J.mix_stems_host(pcms, req, stem_of)
    assert len(got) == 3 and reps[0].depth == depth
    total = got[1] + got[2]
    terms = [np.abs(M.term(x, 0, 0, g)) for x, g in zip(pcms, gains_of(req))]
    sum_t = np.zeros(got[0].size)
    for u, t in enumerate(terms):
        sum_t[u:u + t.size] += t
    bound = (depth - 1) * 2.0 ** -52 * sum_t
    err = np.abs(total - got[0])
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert err.max() > 0.0  # (the association does differ somewhere: the bound is not idle)


def test_additivity_at_depth_two_with_a_third_talker_elsewhere():
    """== at every sample under at most two members, whatever lies elsewhere in the programme"""
    pcms = [pcm_of(n, 80 + u, False) for u, n in enumerate([3000, 3000, 3000])]
    req = [(0, 0, -1.0, 0, 30, 30), (0, 2000, 2.0, 0, 30, 30), (0, 4000, 0.5, 0, 30, 30)]
    got, reps, _ = J.mix_stems_host(pcms, req, [2, 1, 0])
    assert reps[0].depth == 2 and reps[0].overlap == 2000
    assert np.array_equal(got[1] + got[2] + got[3], got[0])


@pytest.mark.parametrize("depth", [2, 3, 9])
def test_additivity_in_16_bits(depth):
    pcms, req, stem_of = overlapped(depth, 2500, True, 32767.0 / (4.5 * depth * 1.5))  # (3.5 dB is a factor of 1.5)
    gains = gains_of(req)
    _, sums, _, _ = S.stems(pcms, req, stem_of, gains)
    assert max(np.abs(s).max() for s in sums) < 32767.0  # no term and no sum leaves the range: nothing clamps
    got, _, _ = J.mix_stems_host(pcms, req, stem_of)
    total = np.sum([s.astype(np.int64) for s in got[1:]], axis=0)
    assert np.abs(total - got[0].astype(np.int64)).max() <= depth


LEVEL_LENGTHS = [1, 255, 256, 1023, 1024, 1025, 3 * 1024 + 1]


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("n", LEVEL_LENGTHS)
def test_levels_are_the_stated_order_bit_for_bit(n, i16):
    mix = pcm_of(n, 5, i16)
    want_p = S.level_sum(mix, mix)
    extents = {(0, n), (0, 1), (n - 1, n), (0, 0)}
    for i in range(0, 4):
        for d in (-1, 0, 1):
            a = 1024 * i + d
            if 0 <= a < n:
                extents |= {(a, n), (a, min(a + 1, n)), (0, a)}
    for first, end in sorted(extents):
        stem = np.zeros_like(mix)
        stem[first:end] = pcm_of(end - first, 6, i16)
        e_s, d, e_p = J.mix_levels_host(stem, mix, first, end)
        assert (e_s, d) == (S.level_sum(stem, stem, first, end), S.level_sum(stem, mix, first, end)), (first, end)
        assert e_p == want_p
        if end > first:
            # the tiles outside the extent add nothing but zeros: over the whole length the sums are the same numbers
            assert e_s == S.level_sum(stem, stem) or first // 1024 > 0
    assert J.mix_levels_host(np.zeros(0), np.zeros(0)) == (0.0, 0.0, 0.0)


def test_levels_in_the_host_seam_are_taken_from_the_units_as_stored():
    for i16 in (False, True):
        pcms = [pcm_of(n, 40 + u, i16) for u, n in enumerate(LEN)]
        for fit in (False, True):
            got, reps, sreps = check_host(pcms, REQ, STEMS["talkers"], fit=fit, ceiling_db=-6.0, levels=True)
            g = J.mix_stems_geometry(REQ, STEMS["talkers"], LEN)
            for s, r in enumerate(sreps):
                u = g["P"] + s
                want = J.mix_levels_host(got[u], got[g["programme"][u]], g["first"][u], g["end"][u])
                assert (r.e_s, r.d, r.e_p) == want
                assert (r.level_db, r.sir_db, r.si_sdr_db) == J.mix_levels_db(*want) == S.db(*want)
    _, _, sreps = J.mix_stems_host(pcms, REQ, STEMS["talkers"])  # without the flag: no sums, no dB values
    assert all(r.e_s == r.d == r.e_p == 0.0 and math.isnan(r.level_db) and math.isnan(r.si_sdr_db) for r in sreps)


def test_db_values_of_edge_sums():
    inf = math.inf
    assert J.mix_levels_db(0.0, 0.0, 4.0) == (-inf, -inf, -inf) == S.db(0.0, 0.0, 4.0)  # a silent stem
    assert J.mix_levels_db(4.0, 4.0, 4.0) == (0.0, inf, inf) == S.db(4.0, 4.0, 4.0)  # the stem is the mixture
    assert J.mix_levels_db(4.0, 0.0, 0.0)[0] == inf  # a stem against silence
    lv, sir, sdr = J.mix_levels_db(1.0, 1.0, 2.0)  # two orthogonal sources of one power
    assert abs(lv + 10 * math.log10(2)) < 1e-12 and abs(sir) < 1e-12 and abs(sdr) < 1e-12


@pytest.mark.parametrize("snr_db", [-28.0, -10.0, 0.0, 12.0, 28.0])
@pytest.mark.parametrize("i16", [False, True])
def test_db_values_against_a_long_double_model(snr_db, i16, capsys):
    """The gate: 8 times the error that a plain sequential float64 evaluation of the same three sums shows against the
    long-double model on the same case.  Cases between -30 and +30 dB: neither denominator cancels"""
    n = 40000
    a = pcm_of(n, 11, False, 3000.0)
    b = pcm_of(n + 500, 12, False, 3000.0)
    req = [(0, 250, snr_db / 2), (0, 0, -snr_db / 2)]
    if i16:
        a, b = [np.trunc(x).astype(np.int16) for x in (a, b)]
    got, _, sreps = J.mix_stems_host([a, b], req, [0, 1], levels=True)
    model = S.db_model(got[1], got[0])
    assert -30.0 < model[2] < 30.0
    seq = S.db_sums(*S.seq_sums(got[1], got[0]))
    lib = (sreps[0].level_db, sreps[0].sir_db, sreps[0].si_sdr_db)
    with capsys.disabled():
        for name, m, q, v in zip(("level_db", "sir_db", "si_sdr_db"), model, seq, lib):
            allow, err = 8.0 * abs(q - m), abs(v - m)
            print(f"\n  stems dB gate {snr_db:+.0f} dB {'i16' if i16 else 'f64'} {name}: model {m:.12f}, "
                  f"sequential f64 off by {abs(q - m):.3e}, the stage by {err:.3e} "
                  f"(ratio {err / abs(q - m) if q != m else float('nan'):.3f})", end="")
            assert err <= allow, (name, err, allow)


def test_refusals():
    L = J.lib()
    x = np.zeros(4)
    ins = (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    nin = (C.c_size_t * 2)(4, 4)
    out = np.zeros(16)
    outs = (C.c_void_p * 4)(*[out.ctypes.data] * 4)
    caps = (C.c_size_t * 4)(*[16] * 4)

    def call(req, stem_of, flags=0, opts=None, caps=caps):
        ids = None if stem_of is None else _ffi.stem_ids(stem_of)
        return L.jb_mix_stems_host(ins, nin, 2, _ffi.mix_request(req), ids, flags, opts, None, outs, caps, None, None)

    def refused(rc, *words):
        msg = L.jb_last_error()
        return rc == INVALID and all(w in msg for w in words)

    assert call([(0,), (0,)], [0, 1]) == 0 and call([(0,), (0,)], [None, None]) == 0
    assert refused(call([(0,), (0,)], [0, 2]), b"jb_mix_stems_host", b"utterance 1", b"stem id", b"(2)")
    assert refused(call([(0,), (0,)], [0, 1], flags=2), b"unknown flag")
    assert call([(0,), (0,)], None) == INVALID
    assert refused(call([(2,), (0,)], [0, 1]), b"programme id 2")  # the mix's own refusals stand
    # the third unit's buffer: too small
    assert call([(0, 5), (0, 9, 0.0, 4)], [0, 0]) == BUFFER  # 17 samples
    assert call([(0, 5), (0, 9, 0.0, 3)], [0, 0], caps=(C.c_size_t * 4)(16, 15, 16, 16)) == BUFFER
    # a reserved word or an unknown flag of the mix request is refused as ever: the stems ride beside them
    bad = _ffi.mix_request([(0,), (0,)])
    bad[1].reserved = 1
    ids = _ffi.stem_ids([0, 1])
    assert L.jb_mix_stems_host(ins, nin, 2, bad, ids, 0, None, None, outs, caps, None, None) == INVALID
    assert b"reserved must be 0 (utterance 1)" in L.jb_last_error()
    assert L.jb_mix_stems_geometry(bad, ids, nin, None, 2, None, None, None, None, None, None, None, None, None, None,
                                   None) == INVALID
    o = _ffi.mix_opts(True, -1.0)
    o.flags = 2
    assert L.jb_mix_stems_host(ins, nin, 2, _ffi.mix_request([(0,), (0,)]), ids, 0, C.byref(o), None, outs, caps, None,
                               None) == INVALID
    assert C.sizeof(_ffi.StemReport) == 64 and _ffi.StemReport.e_s.offset == 16 and _ffi.StemReport.level_db.offset == 40
    # the levels' own entry
    e = C.c_double()
    assert L.jb_mix_levels_host(x.ctypes.data, x.ctypes.data, 4, 3, 2, C.byref(e), None, None) == INVALID
    assert L.jb_mix_levels_host(x.ctypes.data, x.ctypes.data, 4, 0, 5, C.byref(e), None, None) == INVALID
    assert L.jb_mix_levels_host(None, x.ctypes.data, 4, 0, 4, C.byref(e), None, None) == INVALID
    assert L.jb_mix_levels_host(x.ctypes.data, x.ctypes.data, 4, 4, 4, C.byref(e), None, None) == 0 and e.value == 0.0


def test_entries_without_a_device():
    L = J.lib()
    assert L.jb_batch_set_mix_stems(None, None, 0, 0) == INVALID
    assert L.jb_batch_num_programmes(None) == 0 and L.jb_batch_stem_unit(None, 0) == -1
    assert L.jb_batch_stem_layout(None, 0, None, None, None, None, None) == INVALID
    assert L.jb_batch_stem_report(None, 0, None) == INVALID
    U = C.c_size_t(9)
    ids1 = _ffi.stem_ids([0])
    assert L.jb_synthesize_programme_stems(None, None, None, 0, -1, None, ids1, 0, None, None, C.byref(U), None,
                                           None) == INVALID and U.value == 0
    assert L.jb_synthesize_programme_stems_flac_meta(None, None, None, 0, -1, None, None, None, ids1, 0, None, None,
                                                     C.byref(U), None, None) == INVALID
    if L.jb_device_count() > 0:
        return
    x = np.zeros(4)
    ins, nin = (C.c_void_p * 1)(x.ctypes.data), (C.c_size_t * 1)(4)
    outs, ns, P, U = (C.c_void_p * 2)(), (C.c_size_t * 2)(), C.c_size_t(), C.c_size_t()
    req, ids = _ffi.mix_request([(None, 1, 0.0, 1)]), _ffi.stem_ids([0])
    for fn in (L.jb_mix_stems_pcm_batch, L.jb_mix_stems_pcm_batch_i16):
        assert fn(ins, nin, 1, req, ids, 1, None, -1, outs, ns, C.byref(P), C.byref(U), None, None) == DEVICE
        # ... and the argument errors before the device
        assert fn(ins, nin, 1, req, _ffi.stem_ids([1]), 0, None, -1, outs, ns, C.byref(P), C.byref(U), None,
                  None) == INVALID
        assert b"stem id" in L.jb_last_error()
        assert fn(ins, nin, 1, req, ids, 4, None, -1, outs, ns, C.byref(P), C.byref(U), None, None) == INVALID
        assert fn(ins, nin, 1, req, None, 0, None, -1, outs, ns, C.byref(P), C.byref(U), None, None) == INVALID

"""The speech-activity stage without a GPU (jbonsai_amd/csrc/jb_activity.cpp): jb_activity_host against the numpy
statement of the rule (tests/activity_ref.py) byte for byte with its reports, an analytic case, the smoothing steps'
edges, T against the feature stages' shapes, jb_activity_members_host against jb_activity_host on zero-extended
members, every refusal with its field, and the structs' sizes."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import activity_ref as R

ROOT = Path(__file__).resolve().parent.parent
INVALID, UNSUPPORTED, BUFFER = -1, -2, -8
HZ = 16000
SMOOTH = dict(min_speech=3, min_gap=2, hang_before=1, hang_after=2)


def opts_of(grid, wl, hop, **kw):
    return J.activity(wl, hop, grid=grid, samples=True, **kw)


def check_host(x, grid, wl, hop, gate_db=40.0, reference="peak", **lengths):
    """jb_activity_host is the reference: the labels, and the report counted from the labels"""
    o = opts_of(grid, wl, hop, gate_db=gate_db, reference=reference, **lengths)
    lab, rep = J.activity_host(x, HZ, o)
    want, wrep = R.column(x, 0, len(x), R.GRIDS[grid], wl, hop, gate_db, reference, **lengths)
    assert lab.dtype == np.uint8 and lab.tobytes() == want.tobytes(), \
        (grid, wl, hop, len(x), lab.size, want.size, np.flatnonzero(lab[:want.size] != want[:lab.size])[:8])
    R.same_report(rep, wrep)
    R.same_report(rep, R.report_of(lab))
    return lab


@pytest.mark.parametrize("wl", R.WINDOWS)
@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_host_rule_is_the_reference(grid, wl):
    seed = 0
    for hop in R.hops_of(wl):
        for n in R.lengths_of(wl, hop):
            seed += 1
            x = R.speechy(n, seed)
            check_host(x, grid, wl, hop)
            check_host(x, grid, wl, hop, gate_db=20.0, **SMOOTH)
            assert J.activity_geometry(opts_of(grid, wl, hop), HZ, n) == (wl, hop, R.frames(R.GRIDS[grid], n, wl, hop)[0])


def test_longer_signals_and_the_absolute_gate():
    for seed, (grid, wl, hop, n) in enumerate([("snip", 400, 160, 40000), ("kaldi", 400, 160, 33333),
                                               ("center", 1200, 480, 50001), ("stft", 1024, 256, 30000)]):
        x = R.speechy(n, 100 + seed)
        check_host(x, grid, wl, hop)
        check_host(x, grid, wl, hop, gate_db=30.0, **SMOOTH)
        lab = check_host(x, grid, wl, hop, gate_db=26.0, reference="abs")
        assert 0 < lab.sum() < lab.size
    # the absolute threshold is wl 32768^2 10^(-gate_db / 10): a full-scale square wave sits 0 dB under it at gate_db 0+
    o = opts_of("snip", 64, 64, gate_db=1.0, reference="abs")
    lab, rep = J.activity_host(np.full(640, 32768.0), HZ, o)
    assert lab.all() and rep.thr == R.abs_threshold(1.0, 64) and rep.peak == 64 * 32768.0 ** 2
    lab, _ = J.activity_host(np.full(640, 32768.0 * 10 ** (-1.01 / 20)), HZ, o)
    assert not lab.any()


def test_sine_bursts_on_the_hop_grid():
    """Analytic, without the rule's code: bursts of a sine whose edges lie on multiples of the hop.  A frame wholly
    inside a burst is 1, one wholly outside is 0 (a frame across an edge may be either)."""
    hz, wl, hop = 16000, 400, 160
    n = 100 * hop
    k = np.arange(n)
    x = np.zeros(n)
    bursts = [(10, 25), (40, 41), (60, 90)]  # in hops
    for a, b in bursts:
        x[a * hop:b * hop] = 8000.0 * np.sin(2 * np.pi * 440.0 * k[a * hop:b * hop] / hz)
    for grid in R.GRIDS:
        o = J.activity(25, 10, gate_db=40, grid=grid)
        lab, _ = J.activity_host(x, hz, o)
        wl_, hop_, T = J.activity_geometry(o, hz, n)
        assert (wl_, hop_) == (wl, hop) and T == lab.size
        s0 = R.frames(R.GRIDS[grid], n, wl, hop)[1]
        seen_in = seen_out = 0
        for t in range(T):
            s, e = s0 + t * hop, s0 + t * hop + wl
            inside = any(a * hop <= s and e <= b * hop for a, b in bursts)
            outside = all(e <= a * hop or s >= b * hop for a, b in bursts)
            if inside:
                assert lab[t] == 1, (grid, t)
                seen_in += 1
            if outside:
                assert lab[t] == 0, (grid, t)
                seen_out += 1
        assert seen_in > 20 and seen_out > 20


def smooth_host(bits, **lengths):
    wl = 8
    o = opts_of("snip", wl, wl, **lengths)
    lab, rep = J.activity_host(R.pattern_pcm(bits, wl), HZ, o)
    assert lab.size == len(bits)
    R.same_report(rep, R.report_of(lab))
    return lab.tolist()


def test_smoothing_steps():
    raw = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0]
    assert smooth_host(raw) == raw  # all lengths at 0: the raw bits
    # a gap of exactly min_gap closes, one of min_gap + 1 does not; head and tail gaps stay
    assert smooth_host(raw, min_gap=3) == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0]
    assert smooth_host(raw, min_gap=4) == [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    assert smooth_host(raw, min_gap=65535) == [0, 0] + [1] * 11 + [0, 0]
    # a run of min_speech - 1 goes, one of min_speech stays; a run cut by the edge counts as long as is visible
    runs = [1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1]
    assert smooth_host(runs, min_speech=2) == runs
    assert smooth_host(runs, min_speech=3) == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1]
    assert smooth_host(runs, min_speech=4) == [0] * 14
    # close comes first: the closed run is long enough to stay
    assert smooth_host(runs, min_gap=1, min_speech=9) == [1] * 9 + [0] * 5
    # the hang is clipped at 0 and at T; lengths above T are accepted
    one = [0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert smooth_host(one, hang_before=2, hang_after=3) == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0]
    assert smooth_host(one, hang_before=9) == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert smooth_host(one, hang_after=9) == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
    assert smooth_host(one, hang_before=65535, hang_after=65535) == [1] * 10
    # open runs in front of the hang: a cleared run hangs nothing
    assert smooth_host([1, 0, 0, 0, 1, 1, 0, 0], min_speech=2, hang_after=1) == [0, 0, 0, 0, 1, 1, 1, 0]
    for bits in (raw, runs, one):
        for kw in (dict(min_gap=2), dict(min_speech=3), dict(hang_before=1, hang_after=4), SMOOTH):
            assert smooth_host(bits, **kw) == R.smooth(bits, **kw).tolist()


def test_frames_match_the_feature_stages():
    """For n >= 1, T (and the window and the hop) of each grid is what the feature stages give for the matching
    options: plain fbank, JB_FBANK_CENTER, JB_FRAME_REFLECT, and melspec without drop-last."""
    for hz in (16000, 22050, 48000):
        for n in (1, 159, 160, 399, 400, 401, 1103, 4000, 12345):
            for win_ms, hop_ms in ((25, 10), (20, 20), (10, 12.5)):
                o = {g: J.activity(win_ms, hop_ms, grid=g) for g in R.GRIDS}
                f = _ffi.fbank_geometry(hz, _ffi.fbank(win_ms, hop_ms), n)
                assert J.activity_geometry(o["snip"], hz, n) == (f[0], f[1], f[3])
                f = _ffi.fbank_geometry(hz, _ffi.fbank(win_ms, hop_ms, center=True), n)
                assert J.activity_geometry(o["center"], hz, n) == (f[0], f[1], f[3])
                f = _ffi.fbank_framed_geometry(hz, _ffi.fbank(win_ms, hop_ms), _ffi.frame(reflect=True), n)
                assert J.activity_geometry(o["kaldi"], hz, n) == (f[0], f[1], f[3])
                wl, hop = f[0], f[1]
                m = _ffi.melspec_geometry(hz, _ffi.melspec(n_fft=4096, hop=hop, win=wl, pad="zero"), n)
                assert J.activity_geometry(o["stft"], hz, n) == (m[1], m[2], m[3])
                if n > 2048:  # (reflect padding needs more than n_fft / 2 samples)
                    m = _ffi.melspec_geometry(hz, _ffi.melspec(n_fft=4096, hop=hop, win=wl), n)
                    assert J.activity_geometry(o["stft"], hz, n)[2] == m[3]
                assert J.activity_geometry(J.activity(wl, hop, grid="stft", samples=True), 0, n) == (wl, hop, m[3]) \
                    or n <= 2048


def test_members_are_zero_extended_columns():
    wl, hop = 400, 160
    n_unit = 9000
    pcms = [R.speechy(3000, 1), R.speechy(0, 2), R.speechy(5000, 3), R.speechy(2500, 4)]
    starts = [37, 500, 3999, 6500]
    gains = [0.0, 0.0, -6.0, -math.inf]
    for grid in R.GRIDS:
        for kw in ({}, SMOOTH):
            o = opts_of(grid, wl, hop, gate_db=30.0, **kw)
            mat, reps, unit = J.activity_members_host(pcms, starts, n_unit, HZ, o, gains)
            assert mat.shape[1] == 4
            for j, (x, s) in enumerate(zip(pcms, starts)):
                z = np.zeros(n_unit)
                if gains[j] != -math.inf:
                    z[s:s + x.size] = x
                lab, rep = J.activity_host(z, HZ, o)
                assert mat[:, j].tobytes() == lab.tobytes(), (grid, j)
                R.same_report(reps[j], {k: getattr(rep, k) for k in ("active", "first", "last", "peak", "thr")})
            assert not mat[:, 1].any() and not mat[:, 3].any() and mat[:, 0].any() and mat[:, 2].any()
            R.same_report(unit, R.unit_report_of(mat))
    # a programme of one at start 0 is the utterance alone
    o = opts_of("kaldi", wl, hop)
    mat, _, _ = J.activity_members_host([pcms[0]], [0], pcms[0].size, HZ, o)
    assert mat[:, 0].tobytes() == J.activity_host(pcms[0], HZ, o)[0].tobytes()


def refused(rc_want, word, fn):
    with pytest.raises(J.JbError) as e:
        fn()
    assert word in str(e.value), str(e.value)
    assert getattr(e.value, "code", rc_want) == rc_want


def test_refusals_name_their_field():
    x = np.ones(1000)

    def host(o, hz=HZ):
        return lambda: J.activity_host(x, hz, o)

    for field, val, word in (("grid", 4, "grid"), ("reference", 2, "reference"), ("columns", 2, "columns"),
                             ("flags", 2, "flags"), ("gate_db", 0.5, "gate_db"), ("gate_db", 121.0, "gate_db"),
                             ("gate_db", math.nan, "gate_db"), ("min_speech", 65536, "min_speech"),
                             ("min_gap", 65536, "min_gap"), ("hang_before", 65536, "hang_before"),
                             ("hang_after", 65536, "hang_after")):
        o = J.activity()
        setattr(o, field, val)
        refused(INVALID, word, host(o))
        refused(INVALID, word, lambda: J.activity_geometry(o, HZ, 10))
    o = J.activity()
    o.reserved[2] = 1
    refused(INVALID, "reserved", host(o))
    refused(INVALID, "win_us", host(J.activity(1, 1, samples=True)))
    refused(INVALID, "win_us", host(J.activity(4097, 1, samples=True)))
    refused(INVALID, "win_us", host(J.activity(300, 10), 16000))  # 4800 samples at this rate
    J.activity_host(x, 8000, J.activity(300, 10))                # 2400 at this one
    refused(INVALID, "hop_us", host(J.activity(400, 0, samples=True)))
    refused(INVALID, "hop_us", host(J.activity(25, 0.01), 16000))
    refused(INVALID, "rate", host(J.activity(), 0))
    J.activity_host(x, 0, J.activity(400, 160, samples=True))  # in samples no rate is needed
    # the buffer, and the members' entry's own checks
    o = J.activity(400, 160, samples=True)
    out = np.zeros(8, dtype=np.uint8)
    assert J.lib().jb_activity_host(x.ctypes.data, x.size, HZ, C.byref(o), out.ctypes.data, 3, None) == BUFFER
    refused(INVALID, "passes the unit", lambda: J.activity_members_host([x], [1], 1000, HZ, o))
    refused(INVALID, "columns", lambda: J.activity_members_host([x], [0], 1000, HZ, J.activity(columns="unit")))


def test_struct_sizes(tmp_path):
    assert (C.sizeof(_ffi.ActivityOpts), C.sizeof(_ffi.ActivityReport), C.sizeof(_ffi.ActivityUnitReport)) == (64, 40, 32)
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stdio.h>\nint main(void){printf("%zu %zu %zu %llu\\n", '
                   "sizeof(jb_activity_opts), sizeof(jb_activity_report), sizeof(jb_activity_unit_report), "
                   "(unsigned long long)JB_ACTIVITY_MAX_CELLS);return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in got] == [64, 40, 32, _ffi.ACTIVITY_MAX_CELLS]
    assert _ffi.ActivityOpts.gate_db.offset == 8 and _ffi.ActivityOpts.min_speech.offset == 32
    # 256 members by the flagship configuration's 3.27 million frames pass the cap
    assert 256 * 3_270_000 <= _ffi.ACTIVITY_MAX_CELLS

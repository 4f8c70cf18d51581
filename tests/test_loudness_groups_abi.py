"""Loudness groups and the R128 report without a GPU: the new symbols and struct layouts against the ctypes mirror,
and the host statement of the rules (jb_loudness_gate_host: the rule text the kernels compile, jb_loudness_rules.h)
against the numpy reference (tests/loudness_groups_ref.py) on hop energies made in numpy."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import loudness_groups_ref as R

ROOT = Path(__file__).resolve().parent.parent
H = 4800
LU_TOL = 1e-8     # close_lu of tests/test_gpu_loudness.py: the project's gate for loudness against the reference
PEAK_TOL = 1e-12  # what tests/test_gpu_loudness.py and tests/test_gpu_true_peak.py hold peaks to


def close(got, want, tol):
    if isinstance(want, float) and math.isnan(want):
        assert math.isnan(got), (got, want)
    elif math.isinf(want):
        assert got == want, (got, want)
    else:
        assert abs(got - want) <= tol, (got, want)


def check_r128(got, want):
    assert got["n_windows"] == want["n_windows"], (got, want)
    for k in ("max_momentary_lufs", "max_short_term_lufs", "lra_lu", "lra_low_lufs", "lra_high_lufs"):
        close(got[k], want[k], LU_TOL)


def check_group(got, want):
    close(got["lufs"], want["lufs"], LU_TOL)
    close(got["sample_peak_dbfs"], want["sample_peak_dbfs"], PEAK_TOL)
    close(got["true_peak_dbtp"], want["true_peak_dbtp"], PEAK_TOL)
    close(got["gain_db"], want["gain_db"], LU_TOL)


def energies(rng, nh, level_db=0.0):
    """Hop energies of a programme with dynamics: a slow swing of +-8 dB and noise, around -20 LUFS + level_db."""
    t = np.arange(nh)
    db = -20.0 + level_db + 8.0 * np.sin(2 * np.pi * t / 97.0 + rng.uniform(0, 6)) + rng.normal(0, 2.0, nh)
    return H * 10.0 ** ((db + 0.691) / 10.0)


def test_new_symbols_listed_and_exported():
    lib = C.CDLL(str(J.LIB_PATH))
    for s in ("jb_batch_set_loudness_groups", "jb_batch_loudness_group_of", "jb_batch_loudness_group",
              "jb_batch_set_loudness_report", "jb_batch_loudness_r128", "jb_loudness_groups_pcm_batch",
              "jb_loudness_gate_host"):
        assert s in _ffi.SYMBOLS and hasattr(lib, s), s


def test_struct_layouts_header_vs_ctypes(tmp_path):
    """jb_loudness_r128 and jb_loudness_group_report: the header (whose layout table asserts the same numbers at
    compile time, as C11 and as C++17) against the ctypes mirror."""
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(jb_loudness_r128), '
                   'offsetof(jb_loudness_r128, n_windows), sizeof(jb_loudness_group_report), '
                   'offsetof(jb_loudness_group_report, members), offsetof(jb_loudness_group_report, r128), '
                   'offsetof(jb_loudness_group_report, gain_db), JB_LOUDNESS_NO_GROUP, JB_LOUDNESS_R128);'
                   "return 0;}\n")
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        G, r = _ffi.LoudnessGroupReport, _ffi.LoudnessR128
        assert got == [C.sizeof(r), r.n_windows.offset, C.sizeof(G), G.members.offset, G.r128.offset,
                       G.gain_db.offset, _ffi.LOUDNESS_NO_GROUP, _ffi.LOUDNESS_R128] == [48, 40, 96, 40, 48, 24,
                                                                                        0xFFFFFFFF, 1]


def test_gate_host_group_with_every_edge_member():
    """One group of: no block (nh = 3), blocks but no window (nh = 29), exactly one window (nh = 30), a long member,
    a member 12 dB below the rest (the relative gate cuts part of it), and the long member again (ties in the
    selection)."""
    rng = np.random.default_rng(11)
    long_ = energies(rng, 700)
    zs = [energies(rng, 3), energies(rng, 29), energies(rng, 30), long_, energies(rng, 400, -12.0), long_.copy()]
    peaks = [900.0, 4000.0, 2500.0, 12000.0, 3000.0, 12000.0]
    got, members = J.loudness_gate_host(zs, H, peaks, target=-16.0, ceiling=-1.0)
    want = R.group(zs, H, peaks, None, -16.0, -1.0)
    check_group(got, want)
    assert got["members"] == 6 and got["peak_mode"] == 0 and got["flags"] == _ffi.LOUDNESS_R128
    check_r128(got["r128"], R.r128(zs, H))
    for z, m in zip(zs, members):
        check_r128(m, R.r128([z], H))
    # the edges are what they should be
    assert members[0]["max_momentary_lufs"] == -math.inf and members[0]["n_windows"] == 0
    assert members[1]["max_momentary_lufs"] > -70 and members[1]["max_short_term_lufs"] == -math.inf
    assert members[1]["lra_lu"] == 0.0 and math.isnan(members[1]["lra_low_lufs"])
    assert members[2]["n_windows"] == 1 and members[2]["lra_lu"] == 0.0
    assert members[2]["lra_low_lufs"] == members[2]["lra_high_lufs"] == members[2]["max_short_term_lufs"]
    # the quiet member: some of its blocks are under the group's relative gate, none under its own
    own = R.group([zs[4]], H, [peaks[4]])
    l4 = R.loud(R.block_ms(zs[4], H))
    gamma = want["lufs"]  # (the gate sits at least 10 LU under something not above L_G)
    assert np.any(l4 < gamma - 10.0) and own["lufs"] < want["lufs"] - 8.0
    # the duplicate puts ties into the selection: the set's range is the range of its sorted union
    assert got["r128"]["n_windows"] > 2 * members[3]["n_windows"]


def test_gate_host_group_of_one_is_the_utterance():
    rng = np.random.default_rng(5)
    z = energies(rng, 260)
    got, members = J.loudness_gate_host([z], H, [5000.0], target=-23.0)
    check_group(got, R.group([z], H, [5000.0], None, -23.0))
    assert got["r128"] == members[0]
    # the loudness of these blocks as tests/loudness_ref.py gates them for one utterance
    ms = R.block_ms(z, H)
    l = R.loud(ms)
    keep = l > -70
    gamma = -0.691 + 10 * math.log10(float(np.mean(ms[keep]))) - 10
    keep &= l > gamma
    close(got["lufs"], -0.691 + 10 * math.log10(float(np.mean(ms[keep]))), LU_TOL)


def test_gate_host_true_peak_mode_and_ceiling():
    rng = np.random.default_rng(8)
    zs = [energies(rng, 50), energies(rng, 80, -6.0)]
    peaks, tps = [20000.0, 9000.0], [20500.0, 9900.0]
    got, _ = J.loudness_gate_host(zs, H, peaks, true_peak=tps, target=-10.0, ceiling=-1.0)
    want = R.group(zs, H, peaks, tps, -10.0, -1.0)
    check_group(got, want)
    assert got["peak_mode"] == 1 and got["oversampling"] == 0
    # the ceiling binds, on the loudest member's true peak
    close(got["gain_db"], -1.0 - R.db(20500.0), 1e-12)


def test_gate_host_large_selection():
    """16 members of 3,000 hops: 47,536 windows, more than any one pass of a 256-lane histogram sees at once; the top
    bytes of the values are shared by thousands of them, so the two ranks are settled by the low bytes: every radix
    pass decides something."""
    rng = np.random.default_rng(21)
    zs = [energies(rng, 3000, -0.5 * m) for m in range(16)]
    got, _ = J.loudness_gate_host(zs, H, [1000.0] * 16)
    want = R.r128(zs, H)
    check_r128(got["r128"], want)
    assert want["n_windows"] > 40000
    # exact, not approximate: the reported percentiles are elements of the set, bit for bit
    w = np.sort(np.concatenate([R.window_ms(z, H) for z in zs]))
    kept = w[len(w) - want["n_windows"]:]
    lo = kept[int(math.floor((len(kept) - 1) * 0.10 + 0.5))]
    hi = kept[int(math.floor((len(kept) - 1) * 0.95 + 0.5))]
    close(got["r128"]["lra_lu"], 10 * math.log10(hi / lo), 1e-12)


def test_gate_host_silence_and_empty():
    got, members = J.loudness_gate_host([np.zeros(40), np.zeros(2)], H, [0.0, 0.0], target=-16.0, ceiling=-1.0)
    assert got["lufs"] == -math.inf and got["sample_peak_dbfs"] == -math.inf and got["gain_db"] == 0.0
    assert got["r128"]["n_windows"] == 0 and got["r128"]["lra_lu"] == 0.0
    assert got["r128"]["max_short_term_lufs"] == -math.inf
    with pytest.raises(J.JbError):
        J.loudness_gate_host([np.ones(4)], 0, [1.0])

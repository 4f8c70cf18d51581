"""The converter on the host, without a GPU: the path jb_resample_geometry reports for every case of
tests/resample_ref.py (each path of k_resample is named by a case, and the case must still reach it), the lengths the
device tests derive from that geometry, and the accuracy of the rule itself -- ascending j with real FMAs, by
tests/plan/resample_probe.cpp -- against the header's formula in long double."""
import ctypes as C
import shutil

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import resample_ref as R

INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not shutil.which(R.HIPCC):
        pytest.skip("hipcc not installed")
    return R.build_probe(tmp_path_factory.mktemp("resample_probe"))


def test_entry_and_layout():
    L = J.lib()
    assert "jb_resample_geometry" in _ffi.SYMBOLS and hasattr(L, "jb_resample_geometry")
    G = _ffi.ResampleGeometry
    assert C.sizeof(G) == 48 and G.pad.offset == 12 and G.lds.offset == 24 and G.identity.offset == 40
    assert L.jb_resample_geometry(48000, 16000, None) == INVALID
    for bad in ((0, 16000), (48000, 0), (0, 0)):
        with pytest.raises(J.JbError) as ei:
            J.resample_geometry(*bad)
        assert ei.value.code == INVALID
    with pytest.raises(J.JbError) as ei:
        J.resample_geometry(44100, 44099)
    assert ei.value.code == UNSUPPORTED and "2048" in str(ei.value)


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_case_reaches_its_path(c):
    g = J.resample_geometry(c.in_hz, c.out_hz)
    R.check_class(g, c)
    assert g.rows >= 1 and g.lds_bytes <= 65536 and g.reserved == 0
    L, M, taps = J.resample_filter(c.in_hz, c.out_hz)
    assert (L, M, taps.shape[1]) == (g.L, g.M, g.ntaps)
    if g.lds:
        wlen = g.rows * g.M + g.ntaps
        assert wlen <= g.cap and g.cap <= 8192
        slots = wlen + (wlen >> g.pad) + 1 if g.pad else wlen
        assert g.lds_bytes == 8 * slots and slots <= 8192
        # one more row would not fit, or the wave mapping caps the rows
        assert (g.rows + 1) * g.M + g.ntaps > g.cap or g.rows in (64, 128, 256)


def test_every_path_and_pad_is_named():
    """The classes of the table: each wave mapping, the row cap, the global path, and every pad shift."""
    geo = [J.resample_geometry(c.in_hz, c.out_hz) for c in R.CASES]
    assert {c.path for c in R.CASES} == {R.LDS4, R.LDS2, R.LDS1, R.GLOBAL}
    assert {g.pad for g in geo if g.lds} == {0, 4, 5, 6, 7}
    assert any(g.row_waves == 1 and g.rows == 64 and g.fit > 64 for g in geo)
    assert any(g.row_waves == 1 and g.rows == g.fit < 64 for g in geo)
    assert any(g.row_waves == 1 and g.L < 4 for g in geo) and any(g.L > 147 for g in geo)
    assert max(g.L for g in geo) == max(g.M for g in geo) == 2048


def test_identity_geometry():
    for hz in (48000, 1, 2048):
        g = J.resample_geometry(hz, hz)
        assert (g.identity, g.L, g.M, g.ntaps, g.lds, g.pad, g.lds_bytes) == (1, 1, 1, 1, 0, 0, 0)
        assert (g.rows, g.row_waves) == (16384, 4)


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_lengths_cross_every_boundary(c):
    g = J.resample_geometry(c.in_hz, c.out_hz)
    ns = R.lengths(g.L, g.M, g.ntaps, g.rows)
    assert ns[:4] == [0, 1, 2, g.ntaps - 1]
    rows = {-(-R.out_len(n, g.L, g.M) // g.L) for n in ns[4:]}
    assert rows == {1, g.rows - 1, g.rows, g.rows + 1, 2 * g.rows + 1} - {0}
    # last rows that are whole, of one output and one output short, wherever a length gives them (L <= M: always;
    # M = 1: every n_out is a multiple of L)
    want = set(R.last_rows(g.L, g.M))
    assert want == R.rests(ns[4:], g.L, g.M)
    if g.L <= g.M:
        assert want == {0, 1 % g.L, g.L - 1}
    else:
        assert want == {0} if g.M == 1 else len(want) == 3
    assert max(ns) <= (2 * g.rows + 1) * g.M and sum(ns) <= 3_000_000


@pytest.mark.skipif(not R.have_long_double(), reason="numpy.longdouble has no 64-bit mantissa here")
@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_fma_chain_within_the_gate_of_a_float64_sum(probe, tmp_path, c):
    """e(probe) <= GATE e(polyphase_seq64) on a Gaussian signal of sigma 3000, min(rows, 64) + 1 rows long: the rule
    the device is then held to bit for bit is as good as a plain float64 sum of the same terms.  The comparator's own
    error is never 0 (5.8e-16 at 214 taps to 2.1e-14 at 145,636; the chain's is 0.91 to 1.29 times it:
    profiles/r28_resample_paths.txt), so the gate cannot pass vacuously."""
    g = J.resample_geometry(c.in_hz, c.out_hz)
    n = (min(g.rows, 64) + 1) * g.M
    x, = R.signals(c, [n])
    y, = R.run_probe(probe, c.in_hz, c.out_hz, [x], tmp_path)
    y_ld = R.polyphase_ld(x, c.in_hz, c.out_hz)
    assert y.shape == y_ld.shape == (R.out_len(n, g.L, g.M),)
    e, e64 = R.err(y, y_ld), R.err(R.polyphase_seq64(x, c.in_hz, c.out_hz), y_ld)
    print(f"{c.in_hz} -> {c.out_hz}: ntaps {g.ntaps}, e {e:.3e}, e_seq64 {e64:.3e}, ratio {e / e64:.2f}")
    assert 0 < e64 < 1e-13 and e <= R.GATE * e64


def test_probe_returns_the_taps_and_keeps_utterances_apart(probe, tmp_path):
    """The probe's own indexing, on inputs whose answer is known exactly: an impulse gives one tap per output (a zero
    term adds nothing to an FMA chain), and two utterances in one file do not see each other."""
    in_hz, out_hz = 48000, 25000
    L, M, taps = J.resample_filter(in_hz, out_hz)
    Ch = taps.shape[1] // 2
    N, n0 = 900, 431
    x = np.zeros(N)
    x[n0] = 1.0
    rng = np.random.default_rng(5)
    a, b = R.SIGMA * rng.standard_normal(333), R.SIGMA * rng.standard_normal(70)
    y, ya, yb, ye = R.run_probe(probe, in_hz, out_hz, [x, a, b, np.zeros(0)], tmp_path)
    k = np.arange(y.size, dtype=np.int64)
    q, p = (k * M) // L, (k * M) % L
    j = n0 - q + Ch - 1
    hit = (j >= 0) & (j < taps.shape[1])
    want = np.zeros(y.size)
    want[hit] = taps[p[hit], j[hit]]
    assert hit.sum() > 50 and np.array_equal(y, want) and y[hit].tobytes() == want[hit].tobytes() and ye.size == 0
    ya1, = R.run_probe(probe, in_hz, out_hz, [a], tmp_path)
    yb1, = R.run_probe(probe, in_hz, out_hz, [b], tmp_path)
    assert ya.tobytes() == ya1.tobytes() and yb.tobytes() == yb1.tobytes()

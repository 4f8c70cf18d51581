"""Room responses without a GPU (jb_room.cpp): symbols and layouts, the low-pass table, Eyring's design, every refusal,
the geometry, the varied positions, and the host rule against the independent model of tests/room_ref.py.

The accuracy gate.  e = max_k |h - model_ld| / max_k S_k with S_k = sum |A lp| over tap k's terms; e_np is the same
metric of the float64 numpy model (numpy's own order), at least 2^-52; the host rule gets 8 e_np -- the project's gate
for "same algorithm class, other order".  The error is dominated by t = k - tau inheriting tau's ulp, which both
float64 evaluations share: hence a gate relative to a float64 yardstick and not an absolute number.

The rule against the images themselves (model_exact: numpy.sinc and the Hann window, no tables): per tap
|h_k - exact_k| <= 1.01 E_Q sum |A| over the terms in reach, plus the gate above, E_Q the largest difference between
the table's linear interpolation and the window-sinc over a fine grid (pi^2 / (24 Q^2) = 2.51e-5 at Q = 128)."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from tests import room_ref as R

HZ, K = 8000, 513
SIZE = (3.2, 4.1, 2.5)
SRC, MIC = (1.1, 1.4, 1.2), (2.5, 3.3, 1.6)  # the microphone within 1 m of two walls


def to_room(rm, keep_latency=False):
    return J.room(rm["size"], rm["source"], rm["mic"], beta=rm["beta"], hz=rm["hz"], n_taps=rm["n_taps"], c=rm["c"],
                  unit_direct=rm["unit"], keep_latency=keep_latency)


def rooms():
    """The rooms of the accuracy gate (also what tests/test_gpu_room.py runs on the device)."""
    return {
        "plain": R.room(SIZE, SRC, MIC, 0.8, HZ, K),
        "near wall": R.room(SIZE, SRC, (3.05, 3.95, 1.6), 0.8, HZ, K),  # 15 cm from two walls
        "cube diagonal": R.room((3.0, 3.0, 3.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), 0.7, HZ, K),
        "shared coordinate": R.room(SIZE, (1.6, 1.4, 1.2), (1.6, 3.3, 1.2), 0.75, HZ, K),
        "absorbing walls": R.room(SIZE, SRC, MIC, (0.8, 0.0, 0.7, 0.9, 0.0, 0.6), HZ, K),
        "negative beta": R.room(SIZE, SRC, MIC, (-0.8, 0.7, 0.6, -0.5, 0.9, -0.3), HZ, K),
        "anechoic": R.room(SIZE, SRC, MIC, 0.0, HZ, K),
        "1 cm apart": R.room(SIZE, SRC, (1.1, 1.4, 1.21), 0.8, HZ, K),
        "4 pi d": R.room(SIZE, SRC, MIC, 0.8, HZ, K, unit=False),
    }


@pytest.fixture(scope="module")
def refs():
    """The long-double model and the gate of every room, once."""
    return {name: R.gate(rm) for name, rm in rooms().items()}


def test_symbols_and_layouts():
    L = J.lib()
    for s in ("jb_room_host", "jb_room_rir_batch", "jb_room_free", "jb_room_geometry", "jb_room_lowpass",
              "jb_room_design", "jb_room_vary", "jb_batch_set_room", "jb_batch_room_report", "jb_engine_set_room"):
        assert hasattr(L, s) and s in F.SYMBOLS, s
    assert C.sizeof(F.Room) == 144 and F.Room.source.offset == 24 and F.Room.mic.offset == 48
    assert F.Room.beta.offset == 72 and F.Room.c.offset == 120 and F.Room.hz.offset == 128
    assert F.Room.n_taps.offset == 132 and F.Room.flags.offset == 136 and F.Room.reserved.offset == 140
    assert C.sizeof(F.RoomInfo) == 40 and F.RoomInfo.entries.offset == 24 and F.RoomInfo.direct_index.offset == 36
    assert C.sizeof(F.RoomReport) == 24 and F.RoomReport.direct_index.offset == 16 and F.RoomReport.delay.offset == 20
    assert (J.ROOM_WH, J.ROOM_Q) == (R.WH, R.Q) == J.room_lowpass()[1:]


def test_lowpass_table_is_the_formula():
    Ft, wh, q = J.room_lowpass()
    want = R.lowpass_ld()
    assert Ft.size == wh * q + 3 == want.size
    ulp = np.spacing(np.abs(want.astype(np.float64)))
    assert np.all(np.abs(Ft.astype(np.longdouble) - want) <= ulp)
    assert Ft[0] == 1.0 and np.all(Ft[q::q] == 0.0) and np.all(Ft[-3:] == 0.0)
    # the forms are the window-sinc itself
    grid = np.arange(wh * q + 1) / q
    assert np.max(np.abs(Ft[:-2] - R.lowpass_direct(grid))) <= 1e-15
    with pytest.raises(J.JbError, match="too small"):
        F.check(J.lib().jb_room_lowpass((C.c_double * 8)(), 8, None, None))


def test_design_is_eyrings_formula():
    for size, rt60, c in ((SIZE, 0.5, 343.0), ((8.0, 6.0, 3.5), 0.3, 343.0), ((20.0, 15.0, 6.0), 1.2, 340.0)):
        lx, ly, lz = (np.longdouble(v) for v in size)
        V, S = lx * ly * lz, 2 * (lx * ly + ly * lz + lx * lz)
        alpha = 1 - np.exp(-(24 * np.log(np.longdouble(10)) / np.longdouble(c)) * V / (S * np.longdouble(rt60)))
        want = float(np.sqrt(1 - alpha))
        got = J.room_design(size, rt60, c)
        assert len(got) == 6 and all(abs(b - want) <= 2 * np.spacing(want) for b in got) and 0 < want < 1
    assert J.room_design(SIZE, 0.5, 0.0) == J.room_design(SIZE, 0.5, 343.0)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(J.JbError, match="rt60"):
            J.room_design(SIZE, bad)
    rm = J.room(SIZE, SRC, MIC, rt60=0.4, hz=HZ, n_taps=K)
    assert list(rm.beta) == J.room_design(SIZE, 0.4)
    with pytest.raises(ValueError):
        J.room(SIZE, SRC, MIC, hz=HZ, n_taps=K)
    with pytest.raises(ValueError):
        J.room(SIZE, SRC, MIC, beta=0.5, rt60=0.4, hz=HZ, n_taps=K)


def test_refusals_name_the_room_and_the_field():
    def bad(match, **kw):
        args = dict(size=SIZE, source=SRC, mic=MIC, beta=0.8, hz=HZ, n_taps=K)
        reserved = kw.pop("reserved", 0)
        flags = kw.pop("flags", None)
        args.update(kw)
        rm = J.room(**args)
        rm.reserved = reserved
        if flags is not None:
            rm.flags = flags
        for call in (J.room_host, J.room_geometry):
            with pytest.raises(J.JbError, match=match) as e:
                call(rm)
            assert e.value.code == -1 and "room 0" in str(e.value)

    bad(r"size\[0\] is outside", size=(0.4, 4.1, 2.5), source=(0.2, 1.4, 1.2), mic=(0.3, 3.3, 1.6))
    bad(r"size\[2\] is outside", size=(3.2, 4.1, 1001.0))
    bad(r"size\[1\] is outside", size=(3.2, float("nan"), 2.5))
    bad(r"source\[1\] is not strictly inside", source=(1.1, 0.0, 1.2))
    bad(r"source\[0\] is not strictly inside", source=(3.2, 1.4, 1.2))
    bad(r"mic\[2\] is not strictly inside", mic=(2.5, 3.3, 2.6))
    bad(r"mic\[0\] is not strictly inside", mic=(float("nan"), 3.3, 1.6))
    bad(r"beta\[3\] is not in", beta=(0.8, 0.8, 0.8, 1.0, 0.8, 0.8))
    bad(r"beta\[0\] is not in", beta=(-1.0, 0.8, 0.8, 0.8, 0.8, 0.8))
    bad(r"beta\[5\] is not in", beta=(0.8, 0.8, 0.8, 0.8, 0.8, float("nan")))
    bad("closer than 1 cm", mic=(1.1, 1.4, 1.2099))
    bad("hz is outside", hz=999)
    bad("hz is outside", hz=768001)
    bad("n_taps is outside", n_taps=0)
    bad("n_taps is outside", n_taps=J.FIR_MAX_TAPS + 1)
    bad("direct index 56 is not below n_taps 48", n_taps=48)  # d0 = 2.394 m: 55.8 samples
    bad("reserved must be 0", reserved=1)
    bad("unknown flag", flags=4)
    bad("c is neither", c=10.0)


def test_direct_index_refusal_is_at_the_index_itself():
    info = J.room_geometry(J.room(SIZE, SRC, MIC, beta=0.8, hz=HZ, n_taps=K))
    d0 = float(np.sqrt(sum((s - m) ** 2 for s, m in zip(SRC, MIC))))
    assert info.direct_index == int(np.floor(d0 * HZ / 343.0 + 0.5)) and abs(info.direct_distance - d0) < 1e-15
    J.room_host(J.room(SIZE, SRC, MIC, beta=0.8, hz=HZ, n_taps=info.direct_index + 1))
    with pytest.raises(J.JbError, match="direct index %d is not below n_taps" % info.direct_index):
        J.room_host(J.room(SIZE, SRC, MIC, beta=0.8, hz=HZ, n_taps=info.direct_index))


def test_unsupported_bounds():
    # a long response in a small room: more than 1,024 entries on an axis
    with pytest.raises(J.JbError, match=r"axis \d has more than JB_ROOM_MAX_AXIS") as e:
        J.room_geometry(J.room(SIZE, SRC, MIC, beta=0.9, hz=HZ, n_taps=J.FIR_MAX_TAPS))
    assert e.value.code == -2
    # tables that fit, work that does not
    with pytest.raises(J.JbError, match="above 2\\^32") as e:
        J.room_geometry(J.room(SIZE, SRC, MIC, beta=0.9, hz=HZ, n_taps=24000))
    assert e.value.code == -2


def test_geometry_is_the_models_tables():
    for name, rm in rooms().items():
        tb = R.tables(rm)
        info = J.room_geometry(to_room(rm))
        assert list(info.entries) == tb["entries"], name
        assert info.direct_index == tb["direct"] and info.direct_distance == tb["d0"], name
        assert info.pair_visits == tb["entries"][0] * tb["entries"][1] * K and info.workgroups == (K + 255) // 256
    assert R.tables(rooms()["anechoic"])["entries"] == [1, 1, 1]
    # x = Lx absorbs: only n = 0 survives; z = 0 absorbs: only n = p
    tb = R.tables(rooms()["absorbing walls"])
    assert tb["entries"][0] == 2 and tb["entries"][2] == 2 and tb["entries"][1] > 2


def test_vary_is_deterministic_inside_and_different():
    size, margin = (6.0, 4.0, 3.0), 0.5
    seen = set()
    for k in range(64):
        s, m = J.room_vary(7, k, size, margin)
        assert (s, m) == J.room_vary(7, k, size, margin)
        for p in (s, m):
            assert all(margin <= v <= L - margin for v, L in zip(p, size))
        assert np.linalg.norm(np.subtract(s, m)) >= 0.01
        seen.add((tuple(s), tuple(m)))
    assert len(seen) == 64 and J.room_vary(8, 0, size, margin) != J.room_vary(7, 0, size, margin)
    # the stated rule, by hand
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    z = mix(mix(7) ^ 5)
    want = [margin + ((mix((z + j + 1) & M) >> 11) * 2.0 ** -53) * (size[j % 3] - 2 * margin) for j in range(6)]
    s, m = J.room_vary(7, 5, size, margin)
    assert s + m == want
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(J.JbError, match="margin"):
            J.room_vary(7, 0, size, bad)


def test_host_rule_holds_the_accuracy_gate(refs):
    for name, rm in rooms().items():
        h_ld, S, _, bound = refs[name]
        h = J.room_host(to_room(rm))
        e = R.metric(h, h_ld, S)
        print("%-18s e = %.3e  gate = %.3e" % (name, e, bound))
        assert h.size == K and np.all(np.isfinite(h)) and e <= bound, (name, e, bound)


def test_rule_against_the_images_themselves(refs):
    Ft = R.lowpass_ld().astype(np.float64)
    t = np.linspace(0.0, R.WH, 32 * R.TOP + 1)[:-1]
    u = t * R.Q
    i0 = np.floor(u).astype(int)
    E_Q = float(np.max(np.abs(Ft[i0] + (u - i0) * (Ft[i0 + 1] - Ft[i0]) - R.lowpass_direct(t))))
    assert abs(E_Q - np.pi ** 2 / (24 * R.Q ** 2)) <= 1e-7
    for name in ("plain", "negative beta", "4 pi d"):
        rm = rooms()[name]
        h_ld, S, SA, bound = refs[name]
        h = J.room_host(to_room(rm))
        exact = R.model_exact(rm)
        slack = 1.01 * E_Q * SA.astype(np.float64) + bound * float(np.max(S))
        print("%-18s max |h - exact| = %.3e" % (name, np.max(np.abs(h - exact))))
        assert np.all(np.abs(h - exact) <= slack), name


def test_reciprocity(refs):
    for name in ("plain", "negative beta", "near wall"):
        rm = rooms()[name]
        h_ld, S, _, bound = refs[name]
        a = J.room_host(to_room(rm))
        b = J.room_host(to_room(dict(rm, source=rm["mic"], mic=rm["source"])))
        assert float(np.max(np.abs(a - b)) / np.max(S)) <= bound, name


def test_anechoic_room_is_one_term():
    from fractions import Fraction as Fr

    Ft = J.room_lowpass()[0]
    for unit in (True, False):
        rm = dict(rooms()["anechoic"], unit=unit)
        tb = R.tables(rm)
        assert tb["entries"] == [1, 1, 1]
        h = J.room_host(to_room(rm))
        tau0 = tb["d0"] * tb["kappa"]
        want = np.zeros(K)
        for k in range(K):
            t = k - tau0
            if abs(t) < R.WH:
                u = abs(t) * R.Q
                i0 = int(np.floor(u))
                # the two fused operations, exactly: fma(f, F[i0 + 1] - F[i0], F[i0]), then fma(A, lp, +0.0)
                lp = float(Fr(u - i0) * Fr(float(Ft[i0 + 1] - Ft[i0])) + Fr(float(Ft[i0])))
                A = 1.0 / (tb["d0"] / tb["d0"]) if unit else 1.0 / (tb["fourpi"] * tb["d0"])
                want[k] = float(Fr(A) * Fr(lp))
        assert h.tobytes() == want.tobytes()
        if unit:
            frac = tau0 - np.floor(tau0)
            near = min(frac, 1.0 - frac)
            assert abs(np.max(h) - R.lowpass_direct(near)) <= 1.01 * np.pi ** 2 / (24 * R.Q ** 2)
            assert int(np.argmax(h)) == tb["direct"]

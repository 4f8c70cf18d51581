"""Room responses on the GPU (jb_room.hip): the device seam under the accuracy gate of tests/test_room_abi.py at the
edges of the 256-tap workgroups, over rooms that exercise ties, dropped entries, negative coefficients and both
amplitude conventions; then the request in a batch -- bit for bit jb_batch_set_fir with the seam's taps and the direct
index as the delay -- its replacement and withdrawal, and the engine with positions varied per utterance."""
import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import room_ref as R
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.test_room_abi import rooms, to_room

pytestmark = pytest.mark.gpu

EDGES = (1, 255, 256, 257, 513)  # the edges of the 256-tap workgroups
FRAMES = (300, 520, 410)


def same(a, b):
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def quant(y):
    return np.trunc(np.clip(y, -32768.0, 32767.0)).astype(np.int16)


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def tab(eng):
    return synth.VoiceTables(eng)


@pytest.fixture(scope="module")
def batch_utts(eng, tab):
    return eng.voice_info(), [synth.synth_utterance(tab, t, 11 + t) for t in FRAMES]


@pytest.fixture(scope="module")
def plain_pcm(batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts) as b:
        b.run()
        return [b.pcm(i) for i in range(len(utts))]


# ---- 1. the seam ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam():
    """Every room of the gate at every edge its direct index allows (K = 1: the room whose direct index is 0), in ONE
    call."""
    cases = []
    for name, rm in rooms().items():
        direct = R.tables(rm)["direct"]
        for k in EDGES:
            if k > direct:
                cases.append((name, dict(rm, n_taps=k)))
    got = J.room_rir([to_room(rm) for _, rm in cases])
    return cases, got


def test_seam_holds_the_accuracy_gate(seam):
    cases, got = seam
    assert {rm["n_taps"] for _, rm in cases} == set(EDGES)
    refs = {}
    for (name, rm), h in zip(cases, got):
        key = (name, rm["n_taps"])
        refs[key] = R.gate(rm)
        h_ld, S, _, bound = refs[key]
        host = J.room_host(to_room(rm))
        e, e_host = R.metric(h, h_ld, S), R.metric(host, h_ld, S)
        print("%-18s K = %3d  e = %.3e  host %.3e  gate %.3e  bits %s" % (name, rm["n_taps"], e, e_host, bound,
                                                                            same(h, host)))
        assert h.size == rm["n_taps"] and e <= bound and e_host <= bound, key


def test_sixteen_rooms_with_different_k_and_equal_rooms_in_one_call():
    rng = np.random.default_rng(5)
    rs = []
    for i in range(16):
        size = rng.uniform(2.5, 6.0, 3)
        src, mic = J.room_vary(3, i, size, 0.3)
        rs.append(J.room(size, src, mic, beta=float(rng.uniform(0.3, 0.9)), hz=8000, n_taps=200 + 37 * i,
                         unit_direct=bool(i % 2)))
    got = J.room_rir(rs + [rs[3], rs[3]])
    assert [h.size for h in got[:16]] == [200 + 37 * i for i in range(16)]
    assert same(got[16], got[3]) and same(got[17], got[3])
    # a room's bits do not depend on the call it is in
    alone = J.room_rir([rs[9]])
    assert same(alone[0], got[9])
    for i in (0, 9, 15):
        rm = R.room(list(rs[i].size), list(rs[i].source), list(rs[i].mic), list(rs[i].beta), 8000, rs[i].n_taps,
                    unit=bool(i % 2))
        h_ld, S, _, bound = R.gate(rm)
        assert R.metric(got[i], h_ld, S) <= bound, i
    # a refused room touches nothing and is named
    with pytest.raises(J.JbError, match=r"room 1: mic\[0\] is not strictly inside"):
        J.room_rir([rs[0], J.room((3.0, 3.0, 3.0), (1.0, 1.0, 1.0), (3.0, 2.0, 2.0), beta=0.5, hz=8000, n_taps=300)])


# ---- 2. the stage in a batch ----------------------------------------------------------------------------------------
def batch_rooms(hz, n_taps=700):
    size = (3.2, 4.1, 2.5)
    return [J.room(size, (1.1, 1.4, 1.2), (2.0, 2.3, 1.6), rt60=0.3, hz=hz, n_taps=n_taps),
            J.room((5.0, 4.0, 3.0), (1.0, 1.0, 1.0), (2.2, 1.9, 1.5), beta=0.6, hz=hz, n_taps=n_taps + 100,
                   unit_direct=False),
            J.room(size, (2.0, 2.3, 1.6), (1.1, 1.4, 1.2), beta=(0.7, -0.5, 0.6, 0.0, 0.8, 0.4), hz=hz, n_taps=200)]


def as_firs(rs, hz, keep=False):
    taps = J.room_rir(rs)
    return [J.fir(h, hz, 0 if keep else J.room_geometry(r).direct_index) for h, r in zip(taps, rs)]


def test_batch_is_set_fir_with_the_seams_taps(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    rs = batch_rooms(hz)
    # one room per utterance
    with J.Batch(vi, utts) as b:
        b.set_fir(as_firs(rs, hz))
        b.run()
        want = [b.pcm(i) for i in range(3)]
    with J.Batch(vi, utts) as b:
        b.set_room(rs)
        for i, r in enumerate(rs):
            rep, info = b.room_report(i), J.room_geometry(r)
            assert rep.direct_index == info.direct_index == rep.delay and rep.energy > 0
            # (the 200 taps of the third room end 12 taps behind its direct path: nothing outside +-Wh of it)
            assert np.isfinite(rep.drr_db) if i < 2 else rep.drr_db == np.inf
        assert b.fir_geometry(0) == J.fir_geometry(700) and b.fir_geometry(2) == J.fir_geometry(200)
        b.run()
        for i in range(3):
            assert same(b.pcm(i), want[i]) and not same(b.pcm(i), plain_pcm[i]), i
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_room(rs)
    # the report against the taps themselves
    h = J.room_rir([rs[0]])[0]
    d = J.room_geometry(rs[0]).direct_index
    with J.Batch(vi, utts) as b:
        b.set_room(rs)
        rep = b.room_report(0)
    near = float(np.sum(h[max(0, d - 32):d + 33] ** 2))
    np.testing.assert_allclose(rep.energy, float(np.sum(h ** 2)), rtol=1e-12)
    np.testing.assert_allclose(rep.drr_db, 10 * np.log10(near / (float(np.sum(h ** 2)) - near)), rtol=1e-9)
    # one room for all utterances; the latency kept; an utterance without a room
    with J.Batch(vi, utts) as b:
        b.set_fir(as_firs([rs[0]], hz)[0])
        b.run()
        want = [b.pcm(i) for i in range(3)]
    with J.Batch(vi, utts) as b:
        b.set_room(rs[0])
        b.run()
        assert all(same(b.pcm(i), want[i]) for i in range(3))
    keep = J.room((3.2, 4.1, 2.5), (1.1, 1.4, 1.2), (2.0, 2.3, 1.6), rt60=0.3, hz=hz, n_taps=700, keep_latency=True)
    with J.Batch(vi, utts) as b:
        b.set_fir([as_firs([keep], hz, keep=True)[0], None, None])
        b.run()
        want0 = b.pcm(0)
    with J.Batch(vi, utts) as b:
        b.set_room([keep, None, None])
        assert b.room_report(0).delay == 0 and b.room_report(0).direct_index == J.room_geometry(keep).direct_index
        with pytest.raises(J.JbError, match="utterance 1 has no room"):
            b.room_report(1)
        b.run()
        assert same(b.pcm(0), want0) and same(b.pcm(1), plain_pcm[1]) and same(b.pcm(2), plain_pcm[2])
    # the setter's refusals, before any device is touched
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="one room, or one per utterance"):
            b.set_room(rs[:2])
        with pytest.raises(J.JbError, match="utterance 2: hz differs"):
            b.set_room(rs[:2] + [J.room((3.0, 3.0, 3.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), beta=0.5, hz=hz + 1,
                                        n_taps=300)])
        with pytest.raises(J.JbError, match=r"room 1: beta\[0\]"):
            b.set_room([rs[0], J.room((3.0, 3.0, 3.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), beta=1.0, hz=hz, n_taps=300),
                        rs[2]])


def test_i16_batch_converter_noise_and_filter(batch_utts):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    rs = batch_rooms(hz)
    firs = as_firs(rs, hz)
    for kw, setup in (
        (dict(pcm_i16=True), lambda b: None),
        (dict(), lambda b: (b.set_noise(J.noise(None, hz, 15.0, seed=4)), b.set_filter(J.highpass(80.0)))),
    ):
        res = []
        for how in ("fir", "room"):
            with J.Batch(vi, utts, **kw) as b:
                b.set_fir(firs) if how == "fir" else b.set_room(rs)
                setup(b)
                b.run()
                res.append([(b.pcm_i16(i) if kw else b.pcm(i)) for i in range(3)])
        assert all(same(x, y) for x, y in zip(*res)), kw
    # behind the converter at 16 kHz: the rooms are made at the output rate, and a later rate request checks them again
    rs16 = batch_rooms(16000, 400)
    firs16 = as_firs(rs16, 16000)
    res = []
    for how in ("fir", "room"):
        with J.Batch(vi, utts) as b:
            if how == "room":
                with pytest.raises(J.JbError, match="utterance 0: hz differs"):
                    b.set_room(rs16)
            b.set_output_rate(16000)
            b.set_fir(firs16) if how == "fir" else b.set_room(rs16)
            if how == "room":
                with pytest.raises(J.JbError, match="utterance 0: hz of its impulse response differs"):
                    b.set_output_rate(8000)
            b.run()
            res.append([b.pcm(i) for i in range(3)])
    assert all(same(x, y) for x, y in zip(*res))


def test_replacement_and_withdrawal(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    rs = batch_rooms(hz)
    f = J.fir(np.array([0.5, 0.25, -0.125]), hz, 1)
    with J.Batch(vi, utts) as b:
        b.set_fir(f)
        b.run()
        want = [b.pcm(i) for i in range(3)]
    with J.Batch(vi, utts) as b:
        b.set_room(rs)
        b.set_fir(f)  # the later call replaces the earlier
        with pytest.raises(J.JbError, match="has no room"):
            b.room_report(0)
        b.run()
        assert all(same(b.pcm(i), want[i]) for i in range(3))
    with J.Batch(vi, utts) as b:
        b.set_fir(f)
        b.set_room(rs)
        b.set_room(None)
        b.run()
        assert all(same(b.pcm(i), plain_pcm[i]) for i in range(3))


# ---- 3. the engine --------------------------------------------------------------------------------------------------
def test_engine_varies_the_positions_per_utterance(eng):
    hz = eng._out_hz()
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
    plain = [np.array(x) for x in eng.synthesize_batch(sents)]
    size, seed, margin = (4.0, 5.0, 2.8), 21, 0.4
    base = J.room(size, (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), rt60=0.25, hz=hz, n_taps=900)
    er = eng.clone()
    er.set_room(base, vary=True, seed=seed, margin=margin)
    got = [np.array(x) for x in er.synthesize_batch(sents)]
    for k in range(3):
        src, mic = J.room_vary(seed, k, size, margin)
        rk = J.room(size, src, mic, beta=list(base.beta), hz=hz, n_taps=900)
        want = J.fir_pcm([plain[k]], as_firs([rk], hz)[0], hz)[0]
        assert same(got[k], want), k
    assert not same(got[0], got[2])  # the same sentence in another position of the call: another room
    # without vary: the room as given; the generator; the slot shared with set_fir; the refusals
    er.set_room(base)
    want0 = J.fir_pcm([plain[0]], as_firs([base], hz)[0], hz)[0]
    assert same(er.synthesize(SAMPLE_SENTENCE_1), want0)
    assert same(er.clone().generator(SAMPLE_SENTENCE_1).generate_all(), want0)
    er.set_fir(J.fir([1.0], hz))
    assert same(er.synthesize(SAMPLE_SENTENCE_1), plain[0])
    er.set_room(base)
    assert same(er.synthesize(SAMPLE_SENTENCE_1), want0)
    with pytest.raises(J.JbError, match="hz differs"):
        er.set_room(J.room(size, (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), rt60=0.25, hz=hz + 1, n_taps=900))
    with pytest.raises(J.JbError, match="margin"):
        er.set_room(base, vary=True, margin=3.0)
    er.set_room(None)
    assert all(same(np.array(g), w) for g, w in zip(er.synthesize_batch(sents), plain))
    assert all(same(np.array(g), w) for g, w in zip(eng.synthesize_batch(sents), plain))  # the engine itself: unchanged

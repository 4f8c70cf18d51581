"""The tree search on the device (jb_treesearch.hip) against the host search of the same build.  Everything it
produces is integers, or bytes that are a function of them: every comparison here is for equality."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import tree_search_inputs as T
from tests.conftest import VOICE
from tests.golden.labels import ALIGNED_1, BENCH_LETTER, GENJI, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.golden.make_permuted_voice import permuted_voice_path

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HOST, DEVICE = _ffi.SEARCH_HOST, _ffi.SEARCH_DEVICE


@pytest.fixture(scope="module")
def base():
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def voice2(tmp_path_factory):
    return permuted_voice_path(tmp_path_factory.mktemp("voice2"))


@pytest.fixture(scope="module")
def two(voice2):
    return J.Engine.load([VOICE, voice2])


@pytest.fixture(scope="module")
def mutated():
    return T.mutated_voice_bytes(VOICE.read_bytes())


@pytest.fixture(scope="module")
def bad_leaf(base):
    _, p = base.tree_index(1, 2, SAMPLE_SENTENCE_1[2])
    return T.bad_leaf_voice_bytes(VOICE.read_bytes(), b'"mgc_s2_%d"' % p)


def with_mode(e, mode):
    c = e.clone()
    c.condition.set_tree_search(mode)
    return c


def assert_device_equals_flat(e, labels):
    got = e.tree_search(labels)
    want = e.tree_search(labels, host=True)
    for g, w, what in zip(got, want, ("tree_state", "pdf_index", "gv_on")):
        assert g.shape == w.shape and np.array_equal(g, w), what
    return got


# ---- the seam: jb_tree_search_batch == jb_tree_search_flat_host ----------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, len(GENJI)])
def test_seam_label_counts(base, n):
    """Waves per workgroup and the tail: label counts around a workgroup's and around 64, and the whole text."""
    ts, pi, gv = assert_device_equals_flat(base, GENJI[:n])
    assert ts.shape == (n, 1, 4, 5) and gv.shape == (n,)


def test_seam_bench_letter_and_two_voices(base, two):
    assert_device_equals_flat(base, BENCH_LETTER)
    assert_device_equals_flat(two, BENCH_LETTER)
    ts, pi, gv = assert_device_equals_flat(two, GENJI)
    assert ts.shape == (len(GENJI), 2, 4, 5)


def test_seam_mutated_voice_every_pattern_kind(mutated):
    """Inner `*`, `?` first and last, Exact, `**`, a lone `*` and Suffix patterns at tree roots; labels and bare strings
    that make each answer both ways (tests/tree_search_inputs.py, checked in tests/test_tree_search_abi.py)."""
    inputs = T.seam_inputs()
    assert_device_equals_flat(J.Engine.load_from_bytes([mutated]), inputs)
    assert_device_equals_flat(J.Engine.load_from_bytes([mutated, VOICE.read_bytes()]), inputs)


def test_seam_big_questions():
    """More than 64 patterns in a question (records in chunks), more than 256 bytes of pattern text (read from the pool
    byte by byte), literals longer than a wave, a glob longer than a lane's registers hold."""
    e = J.Engine.load_from_bytes([T.big_question_voice_bytes(VOICE.read_bytes())])
    assert_device_equals_flat(e, T.seam_inputs())


def test_seam_out_of_range_leaf_is_reported(bad_leaf):
    e = J.Engine.load_from_bytes([bad_leaf])
    ts, pi, gv = assert_device_equals_flat(e, SAMPLE_SENTENCE_1)
    assert pi[2, 0, 1, 0] > e.pdf_table(1, 0).shape[0]


def test_seam_longest_label_and_positions(base):
    lab = SAMPLE_SENTENCE_1[3]
    long = lab.replace("/A:", "/A:" + "9" * (1023 - len(lab)), 1)
    assert len(long) == 1023
    labels = [long] + GENJI[:70] + [long, lab] + GENJI[70:130] + [lab, long]
    ts, pi, gv = assert_device_equals_flat(base, labels)
    for same in ([0, 71, len(labels) - 1], [72, len(labels) - 2]):  # one label, several places of one call
        for k in same[1:]:
            assert np.array_equal(pi[k], pi[same[0]]) and np.array_equal(ts[k], ts[same[0]]) and gv[k] == gv[same[0]]
    # 1,024 bytes: refused by the seam, naming the label
    L = J.lib()
    lines = (C.c_char_p * 2)(lab.encode(), (long + "9").encode())
    assert L.jb_tree_search_batch(base._h, lines, 2, -1, None, None, None) == -2
    assert "labels[1]" in (L.jb_last_error() or b"").decode()


# ---- jb_engine_states: device mode == host mode, bit for bit ---------------------------------------------------

def states_bits(e, labels):
    u = e.states(labels)
    out = [u.durations.tobytes(), e.duration_params(labels).tobytes()]
    for s in u.streams:
        for a in (s.mean, s.var, s.msd, s.gv_mean, s.gv_var, s.gv_switch):
            out.append(None if a is None else (a.dtype.str, a.shape, a.tobytes()))
    return out


@pytest.mark.parametrize("n", [8, 43, 200])
@pytest.mark.parametrize("speed", [1.0, 1.3])
def test_states_device_equals_host(base, n, speed):
    labels = {8: SAMPLE_SENTENCE_1, 43: BENCH_LETTER, 200: GENJI[100:300]}[n]
    assert len(labels) == n
    h, d = with_mode(base, HOST), with_mode(base, DEVICE)
    for e in (h, d):
        e.condition.set_speed(speed)
    assert states_bits(d, labels) == states_bits(h, labels)
    assert d.device_searched_labels == 2 * n and h.device_searched_labels == 0  # states + duration_params


def test_states_device_equals_host_alignment(base):
    h, d = with_mode(base, HOST), with_mode(base, DEVICE)
    for e in (h, d):
        e.condition.set_phoneme_alignment_flag(True)
    assert states_bits(d, ALIGNED_1) == states_bits(h, ALIGNED_1)
    assert d.device_searched_labels == 2 * len(ALIGNED_1)


def test_states_device_equals_host_two_voices_weighted(two):
    h, d = with_mode(two, HOST), with_mode(two, DEVICE)
    for e in (h, d):
        e.condition.set_interpolation_duration([0.3, 0.7])
        for s in range(3):
            e.condition.set_interpolation_parameter(s, [0.3, 0.7])
        for s in range(2):
            e.condition.set_interpolation_gv(s, [0.3, 0.7])
    for labels in (SAMPLE_SENTENCE_2, GENJI[:200]):
        assert states_bits(d, labels) == states_bits(h, labels)


# ---- PCM: device mode == host mode, bit for bit ------------------------------------------------------------------

NINE = [SAMPLE_SENTENCE_1, GENJI[10:53], SAMPLE_SENTENCE_2, GENJI[200:204], BENCH_LETTER, GENJI[300:420], GENJI[500:501],
        GENJI[600:665], GENJI[700:764]]
NINE_LABELS = sum(len(u) for u in NINE)


def test_pcm_synthesize(base):
    h, d = with_mode(base, HOST), with_mode(base, DEVICE)
    for labels in (SAMPLE_SENTENCE_1, BENCH_LETTER):
        before = d.device_searched_labels
        assert np.array_equal(d.synthesize(labels), h.synthesize(labels))
        assert d.device_searched_labels == before + len(labels)
    assert h.device_searched_labels == 0
    assert d.synthesize([]).size == 0 and d.device_searched_labels == len(SAMPLE_SENTENCE_1) + len(BENCH_LETTER)


def test_pcm_batch_i16(base):
    h, d = with_mode(base, HOST), with_mode(base, DEVICE)
    got, want = d.synthesize_batch(NINE, i16=True), h.synthesize_batch(NINE, i16=True)
    assert len(got) == len(want) == 9
    for g, w in zip(got, want):
        assert g.dtype == np.int16 and np.array_equal(g, w)
    assert d.device_searched_labels == NINE_LABELS and h.device_searched_labels == 0


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests.conftest import VOICE
from tests.test_gpu_tree_search import NINE, NINE_LABELS
base = J.Engine.load([VOICE])
out = {}
for mode in (_ffi.SEARCH_HOST, _ffi.SEARCH_DEVICE):
    e = base.clone()
    e.condition.set_tree_search(mode)
    out[mode] = e.synthesize_batch(NINE, i16=True)
    assert e.device_searched_labels == (NINE_LABELS if mode else 0), e.device_searched_labels
assert all(np.array_equal(a, b) for a, b in zip(out[0], out[2]))
print("equal", sum(a.size for a in out[0]))
"""


def test_pcm_batch_i16_two_groups_in_a_child_process():
    env = dict(os.environ, JB_SYNTH_GROUPS="2", JB_E2E_TIMING="1")
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("equal ") and int(r.stdout.split()[1]) > 0
    assert r.stderr.count("jb_synthesize_batch: 2 group(s)") == 2, r.stderr


def test_pcm_each_with_three_conditions(base):
    def engines(mode):
        es = [with_mode(base, mode) for _ in range(3)]
        es[1].condition.set_speed(1.3)
        es[1].condition.set_alpha(0.5)
        es[2].condition.set_additional_half_tone(2.0)
        es[2].condition.set_volume(-3.0)
        return es

    utts = [SAMPLE_SENTENCE_1, BENCH_LETTER, SAMPLE_SENTENCE_2]
    hs, ds = engines(HOST), engines(DEVICE)
    got, want = J.engine.synthesize_batch_each(ds, utts), J.engine.synthesize_batch_each(hs, utts)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert [e.device_searched_labels for e in ds] == [len(u) for u in utts]  # utterance u counts for engines[u]
    assert [e.device_searched_labels for e in hs] == [0, 0, 0]


def test_pcm_generator(base):
    h, d = with_mode(base, HOST), with_mode(base, DEVICE)
    got, want = d.generator(SAMPLE_SENTENCE_1).generate_all(), h.generator(SAMPLE_SENTENCE_1).generate_all()
    assert got.size > 0 and np.array_equal(got, want)
    assert d.device_searched_labels == len(SAMPLE_SENTENCE_1) and h.device_searched_labels == 0


def test_pcm_multi_with_the_device_listed_twice(base):
    h, d = with_mode(base, HOST), with_mode(base, DEVICE)
    got, want = d.synthesize_batch(NINE, devices=[0, 0]), h.synthesize_batch(NINE, devices=[0, 0])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert d.device_searched_labels == NINE_LABELS and h.device_searched_labels == 0


def test_auto_mode_uses_the_device_from_the_measured_size_on(base):
    """JB_SEARCH_AUTO: host below 1,024 label lines per request (profiles/r11_tree_search.txt), device from there on;
    the same PCM either way."""
    h, a = with_mode(base, HOST), with_mode(base, _ffi.SEARCH_AUTO)
    assert np.array_equal(a.synthesize(SAMPLE_SENTENCE_1), h.synthesize(SAMPLE_SENTENCE_1))
    a.synthesize(GENJI[:1023])
    assert a.device_searched_labels == 0
    assert np.array_equal(a.synthesize(GENJI[:1024]), h.synthesize(GENJI[:1024]))
    assert a.device_searched_labels == 1024
    got, want = a.synthesize_batch([GENJI[:600], GENJI[600:1100]], i16=True), h.synthesize_batch(
        [GENJI[:600], GENJI[600:1100]], i16=True)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and a.device_searched_labels == 1024 + 1100


# ---- errors keep their host meaning ------------------------------------------------------------------------------------

def test_out_of_range_leaf_through_synthesize(bad_leaf):
    e = J.Engine.load_from_bytes([bad_leaf])
    for mode in (HOST, DEVICE):
        with pytest.raises(J.JbError) as err:
            with_mode(e, mode).synthesize(SAMPLE_SENTENCE_1)
        assert err.value.code == -4 and "index not found" in str(err.value)


@pytest.mark.parametrize("size", [1024, 3000])
def test_label_above_the_limit_is_searched_on_the_host(base, size):
    labels = list(SAMPLE_SENTENCE_1)
    labels[4] = labels[4].replace("/A:", "/A:" + "9" * (size - len(labels[4])), 1)
    assert len(labels[4]) == size
    h, d = with_mode(base, HOST), with_mode(base, DEVICE)
    assert np.array_equal(d.synthesize(labels), h.synthesize(labels))
    assert d.device_searched_labels == 0

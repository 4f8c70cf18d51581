"""The device tree search at the boundary, without a GPU: the mode and its checks, and the flattened tables with
their scalar walker (jb_tree_search_flat_host) against the host search (jb_engine_tree_index), for equality, on
every (label, voice, kind, state)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import tree_search_inputs as T
from tests.conftest import VOICE
from tests.golden.labels import BENCH_LETTER, GENJI, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.golden.make_permuted_voice import permuted_voice_path

ROOT = Path(__file__).resolve().parent.parent
INVALID = -1
NEW = ["jb_engine_set_tree_search", "jb_engine_get_tree_search", "jb_engine_device_searched_labels",
       "jb_tree_search_batch", "jb_tree_search_flat_host"]


@pytest.fixture(scope="module")
def base():
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def voice2(tmp_path_factory):
    return permuted_voice_path(tmp_path_factory.mktemp("voice2"))


def host_index(e, labels):
    """jb_engine_tree_index for every (label, voice, kind, state), laid out as the seams lay out their results."""
    nk, ns = 1 + e.num_streams, e.num_states
    ts = np.full((len(labels), e.num_voices, nk, ns), -1, np.int32)
    pi = np.zeros_like(ts)
    for i, lab in enumerate(labels):
        for v in range(e.num_voices):
            for k in range(nk):
                for s in range(ns if k else 1):
                    a, b = e.tree_index(k, 2 + s, lab, voice=v)
                    ts[i, v, k, s] = -1 if a is None else a
                    pi[i, v, k, s] = b
    return ts, pi


def host_gv_on(e, labels):
    """!gv_off.test(label) from the GV switches of jb_engine_states (host mode): one state's switch per label."""
    assert e.condition.get_tree_search() == _ffi.SEARCH_HOST
    return e.states(labels).streams[0].gv_switch.reshape(len(labels), e.num_states)[:, 0]


def assert_flat_equals_host(e, labels):
    ts, pi, gv = e.tree_search(labels, host=True)
    want_ts, want_pi = host_index(e, labels)
    assert np.array_equal(ts, want_ts)
    assert np.array_equal(pi, want_pi)
    return ts, pi, gv


def test_symbols_exported_and_mirrored():
    header = (ROOT / "include" / "jbonsai_amd.h").read_text()
    L = J.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _ffi.SYMBOLS and hasattr(L, name)
    for k, v in (("JB_SEARCH_HOST", 0), ("JB_SEARCH_AUTO", 1), ("JB_SEARCH_DEVICE", 2)):
        assert re.search(rf"#define {k} {v}\b", header)
        assert getattr(_ffi, k[3:]) == v


def test_mode_setter_getter_and_copy(base):
    e = base.clone()
    assert e.condition.get_tree_search() == _ffi.SEARCH_HOST and e.device_searched_labels == 0
    for mode in (_ffi.SEARCH_DEVICE, _ffi.SEARCH_AUTO, _ffi.SEARCH_HOST, _ffi.SEARCH_DEVICE):
        e.condition.set_tree_search(mode)
        assert e.condition.get_tree_search() == mode
    c = J.Engine.new(base, e)  # jb_engine_new copies the mode with the rest of the Condition
    assert c.condition.get_tree_search() == _ffi.SEARCH_DEVICE
    assert base.condition.get_tree_search() == _ffi.SEARCH_HOST
    L = J.lib()
    for bad in (3, 7, 0xffffffff):
        assert L.jb_engine_set_tree_search(e._h, bad) == INVALID
        assert e.condition.get_tree_search() == _ffi.SEARCH_DEVICE
    assert L.jb_engine_set_tree_search(None, 0) == INVALID
    assert L.jb_engine_get_tree_search(None) == 0 and L.jb_engine_device_searched_labels(None) == 0


def test_null_arguments(base):
    L = J.lib()
    i32p = C.POINTER(C.c_int32)
    lines = (C.c_char_p * 2)(SAMPLE_SENTENCE_1[0].encode(), None)
    out = np.zeros(2 * 4 * 5, np.int32)
    assert L.jb_tree_search_flat_host(None, lines, 1, None, None, None) == INVALID
    assert L.jb_tree_search_flat_host(base._h, None, 1, None, None, None) == INVALID
    assert L.jb_tree_search_flat_host(base._h, lines, 2, out.ctypes.data_as(i32p), None, None) == INVALID  # a NULL label
    assert L.jb_tree_search_batch(None, lines, 1, -1, None, None, None) == INVALID
    assert L.jb_tree_search_batch(base._h, None, 1, -1, None, None, None) == INVALID
    assert L.jb_tree_search_batch(base._h, lines, 2, -1, None, None, None) == INVALID
    # every output may be NULL, and no labels is no work (no device is touched for either)
    assert L.jb_tree_search_flat_host(base._h, lines, 1, None, None, None) == 0
    assert L.jb_tree_search_flat_host(base._h, None, 0, None, None, None) == 0
    assert L.jb_tree_search_batch(base._h, None, 0, -1, None, None, None) == 0


def test_long_label_is_refused_by_the_device_seam_before_any_device(base):
    L = J.lib()
    lab = SAMPLE_SENTENCE_1[1]
    long = lab.replace("/A:", "/A:" + "9" * (1024 - len(lab)), 1)
    assert len(long) == 1024
    lines = (C.c_char_p * 2)(lab.encode(), long.encode())
    assert L.jb_tree_search_batch(base._h, lines, 2, -1, None, None, None) == -2  # JB_ERR_UNSUPPORTED
    msg = (L.jb_last_error() or b"").decode()
    assert "labels[1]" in msg and "1024" in msg and "1023" in msg
    ts, pi, gv = base.tree_search([long], host=True)  # the walker takes any length
    want_ts, want_pi = host_index(base, [long])
    assert np.array_equal(ts, want_ts) and np.array_equal(pi, want_pi)


def test_each_with_disagreeing_modes_is_refused_before_any_device(base):
    from tests.test_conditions_abi import _each

    a, b = base.clone(), base.clone()
    b.condition.set_tree_search(_ffi.SEARCH_DEVICE)
    rc, msg = _each([a, b], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2])
    assert rc == INVALID and "engines[1]" in msg and "tree_search" in msg
    assert a.device_searched_labels == 0 and b.device_searched_labels == 0


@pytest.mark.parametrize("labels", [GENJI, BENCH_LETTER], ids=["genji", "bench_letter"])
def test_flat_walker_equals_host_search_nitech(base, labels):
    ts, pi, gv = assert_flat_equals_host(base, labels)
    assert np.array_equal(gv, host_gv_on(base, labels))
    assert ts.shape == (len(labels), 1, 4, 5)
    assert np.all(ts[:, :, 0, 1:] == -1) and np.all(pi[:, :, 0, 1:] == 0)  # the duration model has one state index
    assert np.all(ts[:, :, 0, 0] == 2) and np.all(ts[:, :, 1:, :] == np.arange(2, 7))
    if labels is GENJI:
        assert 0 < gv.sum() < len(gv)  # pauses switch the GV off


@pytest.mark.parametrize("labels", [GENJI, BENCH_LETTER], ids=["genji", "bench_letter"])
def test_flat_walker_equals_host_search_two_voices(voice2, labels):
    e = J.Engine.load([VOICE, voice2])
    ts, pi, gv = assert_flat_equals_host(e, labels)
    assert ts.shape[1] == 2
    assert np.array_equal(gv, host_gv_on(e, labels))


@pytest.fixture(scope="module")
def mutated():
    return T.mutated_voice_bytes(VOICE.read_bytes())


def test_mutated_patterns_answer_both_ways_on_the_inputs(mutated):
    """The inputs make every live pattern of the mutated voice decide its question both ways (tree_search_inputs)."""
    inputs = [s.encode() for s in T.seam_inputs()]
    for name, pat in T.MUTATIONS.items():
        hits = [glob_hit for glob_hit in (T.glob_match(pat, s) for s in inputs)]
        assert any(hits) and not all(hits), name
    valid = [s.encode() for s in GENJI[:160] + BENCH_LETTER + T.edited_labels()]
    for name in ("q_first", "q_last", "suffix", "inner_star"):  # on labels the engine's entries accept, too
        hits = [T.glob_match(T.MUTATIONS[name], s) for s in valid]
        assert any(hits) and not all(hits), name
    # the voice's own Suffix pattern of the issue
    hits = [T.glob_match(b"*-23", s) for s in valid]
    assert any(hits) and not all(hits)
    for pat in (b"**", b"*"):
        assert all(T.glob_match(pat, s) for s in inputs)
    assert mutated != VOICE.read_bytes() and len(mutated) == VOICE.stat().st_size


def test_flat_walker_equals_host_search_mutated_voice(base, mutated):
    inputs = T.seam_inputs()
    e = J.Engine.load_from_bytes([mutated])
    ts, pi, gv = assert_flat_equals_host(e, inputs)
    # the mutations change the answers: the same inputs reach other leaves than in the voice as shipped
    ts0, pi0, gv0 = base.tree_search(inputs, host=True)
    for k in (0, 1, 2):
        assert not np.array_equal(pi[:, 0, k], pi0[:, 0, k]), k
    assert np.array_equal(gv, gv0)
    # a root question decides the first branch: both branches of the mutated roots are taken
    assert len(set(pi[:, 0, 0, 0])) > 1
    # two voices with different trees (mutated + as shipped), each searched with its own tables
    e2 = J.Engine.load_from_bytes([mutated, VOICE.read_bytes()])
    ts2, pi2, _ = assert_flat_equals_host(e2, inputs)
    assert np.array_equal(pi2[:, 0], pi[:, 0]) and np.array_equal(pi2[:, 1], pi0[:, 0])


def test_flat_walker_equals_host_search_big_questions(base):
    """A question of 72 patterns and one of 310 bytes of text at tree roots (the kernel's chunked and byte-wise paths;
    here they check the container rewrite and the walker)."""
    raw = T.big_question_voice_bytes(VOICE.read_bytes())
    inputs = T.seam_inputs()
    for pat in T.BIG_LIVE:
        hits = [T.glob_match(pat, s.encode()) for s in inputs]
        assert any(hits) and not all(hits), pat
    e = J.Engine.load_from_bytes([raw])
    ts, pi, gv = assert_flat_equals_host(e, inputs)
    ts0, pi0, gv0 = base.tree_search(inputs, host=True)
    assert not np.array_equal(pi[:, 0, 0], pi0[:, 0, 0]) and not np.array_equal(pi[:, 0, 1], pi0[:, 0, 1])
    assert np.array_equal(pi[:, 0, 2:], pi0[:, 0, 2:])  # the LF0 and LPF sections moved, and read the same


def test_out_of_range_leaf_is_reported_as_the_host_reports_it(base):
    lab = SAMPLE_SENTENCE_1[2]
    _, p = base.tree_index(1, 2, lab)
    raw = T.bad_leaf_voice_bytes(VOICE.read_bytes(), b'"mgc_s2_%d"' % p)
    e = J.Engine.load_from_bytes([raw])
    ts, pi, _ = assert_flat_equals_host(e, SAMPLE_SENTENCE_1)
    npdf = e.pdf_table(1, 0).shape[0]
    assert pi[2, 0, 1, 0] == int("9" * len(str(p))) > npdf  # reported, not refused, by the seam
    with pytest.raises(J.JbError) as err:  # the engine's entries refuse it, in host mode as ever
        e.states(SAMPLE_SENTENCE_1)
    assert err.value.code == -4 and "index not found" in str(err.value)

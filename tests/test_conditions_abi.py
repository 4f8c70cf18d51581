"""Per-utterance synthesis conditions at the boundary, without a GPU: the layout of jb_utt_voc and the checks
jb_synthesize_batch_each makes on its engines before it touches a device (one voice set; sampling frequency,
fperiod, stage, log gain and the batch-invariant flag in common)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

ROOT = Path(__file__).resolve().parent.parent


def test_utt_voc_layout_header_vs_ctypes(tmp_path):
    src = tmp_path / "voc.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){'
                   'printf("%zu %zu %zu %zu\\n", sizeof(jb_utt_voc), offsetof(jb_utt_voc, alpha),'
                   ' offsetof(jb_utt_voc, beta), offsetof(jb_utt_voc, volume)); return 0;}\n')
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("voc_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == [C.sizeof(_ffi.UttVoc), _ffi.UttVoc.alpha.offset, _ffi.UttVoc.beta.offset,
                       _ffi.UttVoc.volume.offset] == [24, 0, 8, 16]


def _each(engines, utterances):
    """jb_synthesize_batch_each straight through ctypes: (status, jb_last_error)."""
    L = J.lib()
    J.engine._bind(L)
    B = len(utterances)
    flat = [l for u in utterances for l in u]
    off = [0]
    for u in utterances:
        off.append(off[-1] + len(u))
    lines = (C.c_char_p * max(1, len(flat)))(*[s.encode() for s in flat])
    offs = (C.c_size_t * (B + 1))(*off)
    hs = (C.c_void_p * max(1, len(engines)))(*[e._h if e is not None else None for e in engines])
    pcm = (C.POINTER(C.c_double) * max(1, B))()
    ns = (C.c_size_t * max(1, B))()
    rc = L.jb_synthesize_batch_each(hs, lines, offs, B, -1, pcm, ns)
    if rc == 0:
        for i in range(B):
            if ns[i]:
                L.jb_pcm_free(pcm[i])
    return rc, (L.jb_last_error() or b"").decode()


@pytest.fixture(scope="module")
def base():
    return J.Engine.load([VOICE])


UTTS = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
INVALID = -1
DEVICE = -3


def test_null_engine_is_invalid(base):
    rc, msg = _each([base, None], UTTS)
    assert rc == INVALID and "engines[1]" in msg


def test_separately_loaded_engines_are_invalid(base):
    other = J.Engine.load([VOICE])  # same file, another voice set
    rc, msg = _each([base, other], UTTS)
    assert rc == INVALID and "voice set" in msg


@pytest.mark.parametrize("field,setter,value", [("fperiod", "set_fperiod", 200),
                                                ("sampling_frequency", "set_sampling_frequency", 44100),
                                                ("batch_invariant", "set_batch_invariant", True)])
def test_mismatched_shared_fields_are_invalid(base, field, setter, value):
    e = base.clone()
    getattr(e.condition, setter)(value)
    rc, msg = _each([base, e], UTTS)
    assert rc == INVALID and msg.endswith(field), msg


def test_engines_of_one_voice_set_pass_validation(base):
    """Engine.new / clone share the voice set: with per-utterance speed, volume, alpha, beta, half tone the call
    passes validation -- and then needs a device (JB_ERR_DEVICE without one)."""
    e1 = base.clone()
    e1.condition.set_speed(1.3)
    e1.condition.set_volume(-6.0)
    e1.condition.set_alpha(0.5)
    e1.condition.set_beta(0.4)
    e1.condition.set_additional_half_tone(4.0)
    e2 = J.Engine.new(base, e1)
    assert _each([], [])[0] == 0  # nothing to do
    if J.lib().jb_device_count() > 0:
        pytest.skip("a device is present: the call would synthesize (tests/test_gpu_conditions.py)")
    rc, _ = _each([base, e1, e2], UTTS + [SAMPLE_SENTENCE_1])
    assert rc == DEVICE


def test_batch_create_voc_checks_entries_before_the_device():
    eng = J.Engine.load([VOICE])
    vi = eng.voice_info()
    u = J.Utterance(np.array([5, 5], dtype=np.uint32),
                    [J.StreamStates(np.zeros((2, 3 * s.vector_length)), np.ones((2, 3 * s.vector_length)),
                                    np.ones(2) if s.is_msd else None) for s in vi.streams])
    with pytest.raises(J.JbError) as ei:
        J.Batch(vi, [u, u], voc=[(0.4, 0.0, 1.0), (0.4, -0.1, 1.0)])
    assert ei.value.code == INVALID and "jb_utt_voc[1]" in str(ei.value)
    with pytest.raises(J.JbError) as ei:
        J.Batch(vi, [u, u], voc=[(float("nan"), 0.0, 1.0), (0.4, 0.0, 1.0)])
    assert ei.value.code == INVALID and "jb_utt_voc[0]" in str(ei.value)

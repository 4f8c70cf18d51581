"""The fast batch-invariant mode at the boundary, without a GPU: JB_BATCH_INVARIANT in the header and its ctypes
mirror, the engine flag (setter, getter, carried by jb_engine_new), the agreement jb_synthesize_batch_each asks of
its engines, and the option combinations that are refused before any device is touched."""
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
INVALID = -1


def test_flag_header_vs_ctypes(tmp_path):
    src = tmp_path / "flag.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stdio.h>\nint main(void){'
                   'printf("%u %u\\n", (unsigned)JB_BATCH_INVARIANT, (unsigned)JB_BATCH_NO_EXC_TABLE); return 0;}\n')
    exe = tmp_path / "flag"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [_ffi.BATCH_INVARIANT, _ffi.BATCH_NO_EXC_TABLE] == [1024, 512]
    # the next free bit: no other flag shares it
    others = [v for k, v in vars(_ffi).items() if k.startswith("BATCH_") and k != "BATCH_INVARIANT"]
    assert all(v & _ffi.BATCH_INVARIANT == 0 for v in others)


@pytest.fixture(scope="module")
def base():
    return J.Engine.load([VOICE])


def test_setter_getter(base):
    e = base.clone()
    c = e.condition
    assert c.get_fast_invariant() is False
    c.set_fast_invariant(True)
    assert c.get_fast_invariant() is True
    assert c.get_batch_invariant() is False  # the serial invariant mode is a separate flag
    c.set_fast_invariant(False)
    assert c.get_fast_invariant() is False
    assert base.condition.get_fast_invariant() is False


def test_engine_new_carries_the_flag(base):
    cond = base.clone()
    cond.condition.set_fast_invariant(True)
    assert J.Engine.new(base, cond).condition.get_fast_invariant() is True
    assert J.Engine.new(cond, base).condition.get_fast_invariant() is False
    assert cond.clone().condition.get_fast_invariant() is True


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
    hs = (C.c_void_p * max(1, len(engines)))(*[e._h for e in engines])
    pcm = (C.POINTER(C.c_double) * max(1, B))()
    ns = (C.c_size_t * max(1, B))()
    rc = L.jb_synthesize_batch_each(hs, lines, offs, B, -1, pcm, ns)
    if rc == 0:
        for i in range(B):
            if ns[i]:
                L.jb_pcm_free(pcm[i])
    return rc, (L.jb_last_error() or b"").decode()


@pytest.mark.parametrize("first", [False, True])
def test_each_rejects_engines_that_disagree(base, first):
    a, b = base.clone(), base.clone()
    (a if first else b).condition.set_fast_invariant(True)
    rc, msg = _each([a, b], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2])
    assert rc == INVALID and msg.endswith("fast_invariant"), msg


def _utt(vi, frames=(5, 5)):
    return J.Utterance(np.array(frames, dtype=np.uint32),
                       [J.StreamStates(np.zeros((len(frames), 3 * s.vector_length)),
                                       np.ones((len(frames), 3 * s.vector_length)),
                                       np.ones(len(frames)) if s.is_msd else None) for s in vi.streams])


CONFLICTS = [("chunk_frames", dict(chunk_frames=32)), ("warmup_frames", dict(warmup_frames=12)),
             ("JB_BATCH_WAVE_KERNEL", dict(kernel="wave")), ("JB_BATCH_LANE_KERNEL", dict(kernel="triple"))]


@pytest.mark.parametrize("name,kw", CONFLICTS, ids=[c[0] for c in CONFLICTS])
def test_batch_create_refuses_conflicting_options(base, name, kw):
    vi = base.voice_info()
    u = _utt(vi)
    with pytest.raises(J.JbError) as ei:
        J.Batch(vi, [u, u], fast_invariant=True, **kw)
    assert ei.value.code == INVALID and name in str(ei.value)
    # the same options without the flag pass that check (and then need a device, or make a batch)
    if J.lib().jb_device_count() == 0:
        with pytest.raises(J.JbError) as ei:
            J.Batch(vi, [u, u], **kw)
        assert ei.value.code != INVALID


def _opts(flags, chunk=0, warmup=0):
    o = _ffi.BatchOpts()
    o.device, o.flags, o.chunk_frames, o.warmup_frames = -1, flags, chunk, warmup
    return o


@pytest.mark.parametrize("name,kw", CONFLICTS, ids=[c[0] for c in CONFLICTS])
def test_other_entries_refuse_conflicting_options(base, name, kw):
    """jb_paramgen_vocode_batch[_multi], jb_vocode_tracks_batch, jb_vocoder_synthesize_batch and
    jb_generator_new_from_tracks: the same refusal, before the device list or a device is looked at."""
    L = J.lib()
    flags = _ffi.BATCH_INVARIANT | {None: 0, "wave": _ffi.BATCH_WAVE_KERNEL,
                                    "triple": _ffi.BATCH_LANE_KERNEL}[kw.get("kernel")]
    o = _opts(flags, kw.get("chunk_frames", 0), kw.get("warmup_frames", 0))
    vi = base.voice_info()
    vd, keep = vi.c_struct()
    u = _utt(vi)
    su = (_ffi.StateUtt * 1)(u.c_struct())
    pcm = (C.POINTER(C.c_double) * 1)()
    ns = (C.c_size_t * 1)()
    devs = (C.c_int32 * 2)(0, 0)
    assert L.jb_paramgen_vocode_batch(C.byref(vd), su, 1, C.byref(o), None, ns) == INVALID
    assert name in L.jb_last_error().decode()
    assert L.jb_paramgen_vocode_batch_multi(C.byref(vd), su, 1, C.byref(o), devs, 2, None, ns) == INVALID
    assert name in L.jb_last_error().decode()
    T = 4
    sp = np.zeros((T, vi.streams[0].vector_length))
    lf0 = np.full((T, 1), 5.0)
    lpf = np.zeros((T, vi.streams[2].vector_length))
    tu = J.TrackUtterance(sp, lf0, lpf)
    tr = (_ffi.TrackUtt * 1)(tu.c_struct())
    assert L.jb_vocode_tracks_batch(C.byref(vd), tr, 1, C.byref(o), pcm, ns) == INVALID
    assert L.jb_vocoder_synthesize_batch(C.byref(vd), tr, 1, C.byref(o), pcm, ns) == INVALID
    g = C.c_void_p()
    assert L.jb_generator_new_from_tracks(C.byref(vd), tr, C.byref(o), C.byref(g)) == INVALID
    assert not g.value
    assert name in L.jb_last_error().decode()

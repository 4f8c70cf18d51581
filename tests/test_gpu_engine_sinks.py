"""One engine request through every entry family and every sink (synthesize_batch_impl, jb_engine.cpp): the single-engine
entry under JB_SYNTH_GROUPS 1, 2 and 5, the _each entry, the programme entry and the batch-level read of the same
states, all bit for bit.  The engine is batch-invariant (the serial recursion), so neither the grouping nor the batch an
utterance runs in can change a bit of it.  Five utterances: the two sample sentences, an empty one, one sentence three
times over, and the first again."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from jbonsai_amd.engine import _lines
from tests import join_ref as R
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.test_gpu_join import OPTS, same

pytestmark = pytest.mark.gpu

UTTS = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, [], list(SAMPLE_SENTENCE_1) * 3, SAMPLE_SENTENCE_1]
FLAC = dict(md5=True, seek_interval_ms=100)
FMT = dict(fmt="s24", dither=True, seed=3)
FB, MF = J.fbank(n_mels=40), J.mfcc(delta_order=1)


def each_mfcc(engines, utts):
    """jb_synthesize_batch_each_mfcc (the package has no wrapper of it)"""
    L, B = engines[0]._L, len(utts)
    offs = (C.c_size_t * (B + 1))(*np.cumsum([0] + [len(u) for u in utts]).tolist())
    hs = (C.c_void_p * B)(*[e._h for e in engines])
    bufs, ns, nf = (C.POINTER(C.c_uint8) * B)(), (C.c_size_t * B)(), (C.c_size_t * B)()
    F.check(L.jb_synthesize_batch_each_mfcc(hs, _lines([l for u in utts for l in u]), offs, B, -1, C.byref(FB),
                                            C.byref(MF), bufs, ns, nf))
    return F.take_mfcc(L, bufs, ns, B, MF, FB.n_mels)


# per sink: the single-engine entry, the _each entry, the programme entry's sink and options, and for the byte sinks
# the batch-level request and read of every output
SINKS = {
    "f64": (lambda e, u: e.synthesize_batch(u), lambda es, u: J.synthesize_batch_each(es, u), dict(sink="f64")),
    "i16": (lambda e, u: e.synthesize_batch(u, i16=True), lambda es, u: J.synthesize_batch_each(es, u, i16=True),
            dict(sink="i16")),
    "flac": (lambda e, u: e.synthesize_batch_flac(u, **FLAC), lambda es, u: J.synthesize_batch_each_flac(es, u, **FLAC),
             dict(sink="flac", **FLAC), lambda b: b.set_flac(**FLAC), lambda b: b.flac_all()),
    "formatted": (lambda e, u: e.synthesize_batch_formatted(u, **FMT),
                  lambda es, u: J.synthesize_batch_each_formatted(es, u, **FMT), dict(sink="formatted", **FMT),
                  lambda b: b.set_format(FMT["fmt"], FMT["dither"], FMT["seed"]), lambda b: b.formatted_all()),
    "adpcm": (lambda e, u: e.synthesize_adpcm_batch(u), lambda es, u: J.synthesize_batch_each_adpcm(es, u),
              dict(sink="adpcm"), lambda b: b.set_adpcm(), lambda b: b.read_adpcm_all()),
    "fbank": (lambda e, u: e.synthesize_fbank_batch(u, FB), lambda es, u: J.synthesize_batch_each_fbank(es, u, FB),
              dict(sink="fbank", opts=FB), lambda b: b.set_fbank(FB), lambda b: b.read_fbank_all()),
    "mfcc": (lambda e, u: e.synthesize_mfcc_batch(u, MF, fbank=FB), each_mfcc, dict(sink="mfcc", opts=MF, fbank=FB),
             lambda b: b.set_mfcc(MF, fbank=FB), lambda b: b.read_mfcc_all()),
}
I16_BATCH = ("i16", "flac", "adpcm")  # the sinks whose batches are made with the 16-bit PCM
BYTE_SINKS = ("flac", "formatted", "adpcm", "fbank", "mfcc")


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    e = J.Engine.load([VOICE])
    e.condition.set_batch_invariant(True)
    return e


@pytest.fixture(scope="module")
def states(eng):
    return eng.voice_info(), [eng.states(u) for u in UTTS]


def bits(x):
    """An output as something == compares bit for bit: arrays by type and bytes; bytes and AdpcmStream as they are."""
    return (x.dtype.str, x.tobytes()) if isinstance(x, np.ndarray) else x


def data_of(x):
    return x.data if isinstance(x, F.AdpcmStream) else x


def n_bytes(x):
    """The bytes that an output holds, given its bits()"""
    x = data_of(x)
    return len(x[1] if type(x) is tuple else x)


def empty_bytes(eng, sink):
    """An output of no samples: nothing, a FLAC stream of its header alone, or the features' geometry for 0 samples"""
    if sink == "fbank":
        return J.fbank_geometry(eng._out_hz(), FB, 0)[4]
    if sink == "mfcc":
        return J.mfcc_geometry(eng._out_hz(), FB, MF, 0)[2]
    return 42 if sink == "flac" else 0


@pytest.mark.parametrize("sink", list(SINKS))
def test_groups_each_and_batch_level_agree(eng, states, sink, monkeypatch):
    batch, each = SINKS[sink][:2]
    monkeypatch.setenv("JB_SYNTH_GROUPS", "1")
    one = [bits(x) for x in batch(eng, UTTS)]
    assert len(one) == len(UTTS) and all(n_bytes(x) > 0 for x in one[:2] + one[3:])
    assert n_bytes(one[2]) == empty_bytes(eng, sink)
    for g in ("2", "5"):
        monkeypatch.setenv("JB_SYNTH_GROUPS", g)
        assert [bits(x) for x in batch(eng, UTTS)] == one, g
    monkeypatch.delenv("JB_SYNTH_GROUPS")
    assert [bits(x) for x in batch(eng, UTTS)] == one
    # five engines that are copies of the first
    engines = [eng] + [eng.clone() for _ in UTTS[1:]]
    assert [bits(x) for x in each(engines, UTTS)] == one
    if sink not in BYTE_SINKS:
        return
    # the batch-level read of every output, from a batch of the same states
    request, read_all = SINKS[sink][3:]
    vi, utts = states
    with J.Batch(vi, utts, serial=True, serial_gv=True, pcm_i16=sink in I16_BATCH) as b:
        request(b)
        b.run()
        assert [bits(x) for x in read_all(b)] == [data_of(x) for x in one]
        if sink == "adpcm":
            assert [b.num_samples(u) for u in range(len(b))] == [x.n_samples for x in one]


@pytest.fixture(scope="module")
def programme_i16(eng, states):
    """The joined programme of the 16-bit PCM as the batch-level API gives it (jb_batch_set_join, read programme)"""
    vi, utts = states
    with J.Batch(vi, utts, serial=True, serial_gv=True, pcm_i16=True) as b:
        hz = b.output_rate(0)
        req = R.chapter([b.num_samples(u) for u in range(len(b))], hz, **OPTS)
        b.set_join(req)
        b.run()
        assert b.num_outputs() == 1
        return b.programme_pcm(0), [b.member_start(u) for u in range(len(b))]


@pytest.mark.parametrize("sink", list(SINKS))
def test_programme_entry(eng, programme_i16, sink):
    out, starts = eng.synthesize_programme(UTTS, **SINKS[sink][2], **OPTS)
    want, want_starts = programme_i16
    n = out.n_samples if sink == "adpcm" else out.size if sink in ("f64", "i16") else None
    # member starts: increasing (the gap also stands behind the empty member) and inside the programme
    assert starts == want_starts and all(a < b for a, b in zip(starts, starts[1:]))
    assert 0 <= starts[0] and starts[-1] < want.size
    if n is not None:
        assert n == want.size  # (ADPCM: the entry's sample count is the i16 programme's length)
    else:
        assert len(out) > 0
    if sink == "i16":
        assert same(out, want)


# jb_synthesize_batch* with a malformed label in the third utterance: refused on the host, before any launch for its
# group.  Code and message as the library has always given them
BAD = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, ["not-a-label"], list(SAMPLE_SENTENCE_1) * 3, SAMPLE_SENTENCE_1]
BAD_CODE, BAD_MESSAGE = -5, "jlabel failed to parse fullcontext-label: not-a-label"


@pytest.mark.parametrize("groups", ["1", "5"])
@pytest.mark.parametrize("sink", list(SINKS))
def test_failure_leaves_no_output(eng, sink, groups, monkeypatch):
    """Every output pointer NULL and every size 0 behind a failed request -- with five groups the first group ({0, 1}:
    the split goes by label count) has been launched and handed to the finisher when the third utterance is refused."""
    monkeypatch.setenv("JB_SYNTH_GROUPS", groups)
    L, B = eng._L, len(BAD)
    flat = [l for u in BAD for l in u]
    offs = (C.c_size_t * (B + 1))(*np.cumsum([0] + [len(u) for u in BAD]).tolist())
    ety = {"f64": C.c_double, "i16": C.c_int16}.get(sink, C.c_uint8)
    out, ns, nsamp = (C.POINTER(ety) * B)(), (C.c_size_t * B)(*[7] * B), (C.c_size_t * B)()
    head = (eng._h, _lines(flat), offs, B, -1)
    if sink == "f64":
        rc = L.jb_synthesize_batch(*head, out, ns)
    elif sink == "i16":
        rc = L.jb_synthesize_batch_i16(*head, out, ns)
    elif sink == "flac":
        rc = L.jb_synthesize_batch_flac_meta(*head, C.byref(F.flac_opts(0, None)), C.byref(F.flac_meta(**FLAC)), out, ns)
    elif sink == "formatted":
        rc = L.jb_synthesize_batch_formatted(*head, C.byref(F.format_opts(FMT["fmt"], FMT["dither"], FMT["seed"])), out,
                                             ns)
    elif sink == "fbank":
        rc = L.jb_synthesize_batch_fbank(*head, C.byref(FB), out, ns, nsamp)
    elif sink == "mfcc":
        rc = L.jb_synthesize_batch_mfcc(*head, C.byref(FB), C.byref(MF), out, ns, nsamp)
    else:
        rc = L.jb_synthesize_batch_adpcm(*head, C.byref(F.adpcm_opts(0)), out, ns, nsamp)
    assert rc == BAD_CODE and L.jb_last_error().decode() == BAD_MESSAGE
    assert not any(bool(p) for p in out) and list(ns) == [0] * B
    with pytest.raises(J.JbError, match=BAD_MESSAGE) as ei:
        eng.synthesize_programme(BAD, **SINKS[sink][2], **OPTS)
    assert ei.value.code == BAD_CODE

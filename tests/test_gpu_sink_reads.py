"""The batch-level size and read entries of the five byte sinks, held to one behaviour: what they answer before the set
call, between it and the run, and after the run; short buffers, NULL destinations and indices past the end; an output
of no samples; and the same with the two utterances joined into one programme.  One batch of a sentence and an empty
utterance: a non-empty output, an empty one and an index past the end.  Codes and texts are the library's own of
before the sinks shared one read path."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1
from tests.test_gpu_engine_sinks import bits

pytestmark = pytest.mark.gpu

INVALID, BUFFER = -1, -8
FB, MF = J.fbank(n_mels=40), J.mfcc(delta_order=1)
# per sink: its messages' prefix and setter, whether its batch holds 16-bit PCM, the set call, the C entries' stem, the
# Python reads of one and of every output, and the bytes of n samples at hz (None: known once the run has encoded them)
SINKS = {
    "flac": ("FLAC", "jb_batch_set_flac", True, lambda b: b.set_flac(), ("flac_size", "read_flac"),
             lambda b, i: b.flac(i), lambda b: b.flac_all(), None),
    "formatted": ("format", "jb_batch_set_format", False, lambda b: b.set_format("s24"),
                  ("formatted_size", "read_formatted"), lambda b, i: b.formatted(i), lambda b: b.formatted_all(),
                  lambda hz, n: 3 * n),
    "adpcm": ("ADPCM", "jb_batch_set_adpcm", False, lambda b: b.set_adpcm(), ("adpcm_size", "read_adpcm"),
              lambda b, i: b.read_adpcm(i), lambda b: b.read_adpcm_all(), lambda hz, n: J.adpcm_geometry(hz, n)[3]),
    "fbank": ("fbank", "jb_batch_set_fbank", False, lambda b: b.set_fbank(FB), ("fbank_size", "read_fbank"),
              lambda b, i: b.read_fbank(i), lambda b: b.read_fbank_all(), lambda hz, n: J.fbank_geometry(hz, FB, n)[4]),
    "mfcc": ("mfcc", "jb_batch_set_mfcc", False, lambda b: b.set_mfcc(MF, fbank=FB), ("mfcc_size", "read_mfcc"),
             lambda b, i: b.read_mfcc(i), lambda b: b.read_mfcc_all(), lambda hz, n: J.mfcc_geometry(hz, FB, MF, n)[2]),
}


@pytest.fixture(scope="module")
def states():
    assert J.lib().jb_device_count() > 0
    eng = J.Engine.load([VOICE])
    return eng.voice_info(), [eng.states(SAMPLE_SENTENCE_1), eng.states([])]


def check_reads(b, sink, samples):
    """Every case above for the outputs of b, which hold samples[u] samples each"""
    tag, setter, _, request, (size_name, read_name), read, read_all, geometry = SINKS[sink]
    L, hz, n_out = J.lib(), b.output_rate(0), len(samples)
    size_fn, read_fn = getattr(L, "jb_batch_" + size_name), getattr(L, "jb_batch_" + read_name)
    not_set, not_run = f"{tag}: {setter} was not called", f"{tag}: the batch has not run"
    assert b.num_outputs() == n_out
    buf = np.zeros(1 << 20, dtype=np.uint8)
    dst = buf.ctypes.data_as(C.POINTER(C.c_uint8)) if sink == "flac" else buf.ctypes.data

    def size(u):
        n = C.c_size_t(7)
        rc = size_fn(b._h, u, C.byref(n))
        return (rc, n.value) if rc == 0 else (rc, L.jb_last_error().decode())

    def read_into(u, to, cap):
        rc = read_fn(b._h, u, to, cap)
        return rc if rc == 0 else (rc, L.jb_last_error().decode())

    for u in range(n_out):  # before the set call
        assert size(u) == (INVALID, not_set) and read_into(u, dst, buf.size) == (INVALID, not_set)
    request(b)
    for u in range(n_out):  # between it and the run: the planned sinks know their sizes, FLAC's come from the encoder
        assert size(u) == ((0, geometry(hz, samples[u])) if geometry else (INVALID, not_run))
        assert read_into(u, dst, buf.size) == (INVALID, not_run)
    b.run()
    every = read_all(b)
    assert len(every) == n_out
    for u in range(n_out):
        rc, n = size(u)
        assert rc == 0 and n <= buf.size
        if geometry:
            assert n == geometry(hz, samples[u])
        else:
            assert n == 42 if samples[u] == 0 else n > 42  # (a stream of no samples is its header alone)
        assert samples[u] == 0 or n > 0
        one = read(b, u)
        assert bits(one) == bits(every[u])
        assert read_into(u, dst, n) == 0  # (for an output of no bytes too)
        assert buf[:n].tobytes() == (one.tobytes() if isinstance(one, np.ndarray) else one)
        if n:
            short = read_into(u, dst, n - 1)
            # (the FLAC entry gave the code alone before it shared the others' path)
            assert short[0] == BUFFER
            assert sink == "flac" or short[1] == f"jb_batch_{read_name}: the buffer is too small"
            assert read_into(u, None, n)[0] == INVALID
    assert size(n_out)[0] == INVALID and read_into(n_out, dst, buf.size)[0] == INVALID


@pytest.mark.parametrize("sink", list(SINKS))
def test_utterances(states, sink):
    vi, utts = states
    with J.Batch(vi, utts, serial=True, serial_gv=True, pcm_i16=SINKS[sink][2]) as b:
        samples = [b.num_samples(u) for u in range(len(b))]
        assert samples[0] > 0 and samples[1] == 0
        check_reads(b, sink, samples)


@pytest.mark.parametrize("sink", list(SINKS))
def test_programme(states, sink):
    vi, utts = states
    with J.Batch(vi, utts, serial=True, serial_gv=True, pcm_i16=SINKS[sink][2]) as b:
        b.set_join([(0, 0, 0, 0, 0), (0, 0, 0, 0, 0)])
        members, n, _ = b.programme_layout(0)
        assert members == 2 and n == b.num_samples(0)
        check_reads(b, sink, [n])

"""Every stage of the output chain at once through redo rounds: the converter, a filter, a loudness target with a group
and the R128 report, the join, and the encoders (FLAC with MD5 and SEEKTABLE, or the dithered 24-bit format; IMA ADPCM).
Each stage's own redo test leaves most of the others off; here a stage that followed the wrong part of a redo round
(tests/test_output_redo_plan.py has the three masks) would leave a stale sample somewhere between the vocoder and the
encoded bytes.

Bounds.  Behind the join everything is bit for bit, as in tests/test_gpu_join.py.  In front of it the final
per-utterance PCM is compared with the seams applied to the final native PCM: the converter in a batch agrees with its
seam to a relative RMS of 1e-13 (tests/test_gpu_resample.py's redo test, at this rate); one high-pass section and one
gain pass that error on and add roundings of 1e-16, so 1e-12 holds with a factor of ten to spare, and a chunk left stale
by a two-frame warm-up is off by many orders more.  Through the 16-bit sink the same error can move a sample across a
truncation boundary: one step at the most.  Loudness values and gains to 1e-8 LU (tests/test_gpu_loudness_groups.py);
a sample peak to 1e-9 dB, not that file's 1e-12, which is for a reference fed the device's own samples: here the peak
sample carries the converter's error, taken as at most a hundred times the RMS one (1e-10 relative, 8.7e-10 dB)."""
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from jbonsai_amd import synth
from tests import loudness_groups_ref as R
from tests.conftest import VOICE
from tests.helpers import rel_rms
from tests.test_gpu_join import REDO_REQ, check_flac, check_programmes
from tests.test_gpu_loudness import close_lu
from tests.test_gpu_loudness_groups import LU_TOL, check_r128

pytestmark = pytest.mark.gpu

IN, HZ = 48000, 22050
TARGET = -21.0
GROUPS = [None, 0, 0, None]  # the group {1, 2} spans both programmes of REDO_REQ


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


def check_group(got, want):
    close_lu(got["lufs"], want["lufs"], LU_TOL)
    close_lu(got["gain_db"], want["gain_db"], LU_TOL)
    close_lu(got["sample_peak_dbfs"], want["sample_peak_dbfs"], 1e-9)
    assert got["peak_mode"] == 0 and got["flags"] == F.LOUDNESS_R128


@pytest.mark.parametrize("i16", [True, False])
def test_whole_chain_through_redo_rounds(eng, i16):
    """Every hand-off of the long utterances fails, so redo rounds rewrite them behind the first pass of the chain;
    utterances 1 and 3 have one chunk and are never rewritten, but 1 shares utterance 2's gain and both share a
    programme with a rewritten one."""
    vi = eng.voice_info()
    tab = synth.VoiceTables(eng)
    utts = [synth.synth_utterance(tab, T, 40 + T) for T in (400, 90, 600, 30)]
    filt = J.highpass(70.0)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12, pcm_i16=i16) as b:
        b.set_output_rate(HZ)
        b.set_filter(filt)
        b.set_loudness_target(TARGET, math.inf)
        b.set_loudness_groups(GROUPS)
        b.set_loudness_report()
        b.set_join(REDO_REQ)
        if i16:
            b.set_flac(md5=True, seek_interval_ms=50)
        else:
            b.set_format("s24", dither=True, seed=5)
        b.set_adpcm()
        b.run()
        b.sync()
        print("n_redo", b.info()["n_redo"], "redo_stats", b.redo_stats())
        assert b.info()["n_redo"] >= 1
        # in front of the join: the seams on the final native PCM, the group's one gain, the report
        front = J.filter_pcm(J.resample([b.pcm_native(i) for i in range(4)], IN, HZ), filt, HZ)
        want, want_r, want_m = R.group_of_pcm(front[1:3], HZ, None, TARGET, math.inf)
        rep = b.loudness_group(1)
        check_group(rep, want)
        assert repr(rep) == repr(b.loudness_group(2)) and rep["members"] == 2
        assert b.loudness(1)[2] == b.loudness(2)[2] == rep["gain_db"]
        check_r128(rep["r128"], want_r)
        for i in (1, 2):
            check_r128(b.loudness_r128(i), want_m[i - 1])
        for i in (0, 3):
            own, own_r, _ = R.group_of_pcm([front[i]], HZ, None, TARGET, math.inf)
            check_group(b.loudness_group(i), own)
            check_r128(b.loudness_r128(i), own_r)
        for i in range(4):
            assert b.output_rate(i) == HZ
            scaled = front[i] * 10.0 ** (b.loudness(i)[2] / 20.0)
            if i16:
                got, q = b.pcm_i16(i), np.trunc(np.clip(scaled, -32768.0, 32767.0))
                step = int(np.max(np.abs(got.astype(np.int64) - q.astype(np.int64))))
                print("utterance", i, "largest 16-bit difference", step)
                assert got.size == q.size and step <= 1, (i, step)
            else:
                got = b.pcm(i)
                print("utterance", i, "relative RMS against the seams", rel_rms(got, scaled))
                assert got.size == scaled.size and rel_rms(got, scaled) <= 1e-12, (i, rel_rms(got, scaled))
        # behind it: the programmes recomputed from that PCM, and every encoder's bytes of those programmes
        progs = check_programmes(b, i16, REDO_REQ)
        for p, x in enumerate(progs):
            assert b.read_adpcm(p) == J.adpcm_encode_host(x, HZ), p
            if not i16:
                assert b.formatted(p) == J.format_pcm_host(x, "s24", True, 5), p
        if i16:
            check_flac(b, progs, HZ, decode=False, md5=True, seek_interval_ms=50)

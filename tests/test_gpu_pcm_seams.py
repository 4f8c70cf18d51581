"""What the shared part of the stand-alone entries on caller-held PCM (jb_*_pcm_batch: jbonsai_amd/csrc/jb_pcm_call.h
and DeviceScratch in jb_host.h) can get wrong on its own, through each of the ten bodies behind them: a call without an
utterance, an empty utterance beside others, a single sample, one sample past a 1,024-sample tile, the device picked
by -1 and by index, and the caller's current device after the call.  What the stages compute is held to their host
references by the tests of each stage; here an output is compared with the stage's host seam or reference helper."""
import math

import numpy as np
import pytest

import jbonsai_amd as J
from tests import flac_ref, loudness_groups_ref, loudness_ref, true_peak_ref
from tests.flac_meta_ref import check as flac_check

pytestmark = pytest.mark.gpu

HZ = 48000
LENGTHS = [0, 1, 1025]  # an empty utterance, a single sample, one sample past a 1,024-sample tile
HP = J.highpass(120.0)
GAIN, CEILING = 2.0, -1.0
ONE_PROGRAMME = [(0,)] * 3


@pytest.fixture(scope="module")
def pcm():
    assert J.lib().jb_device_count() > 0
    rng = np.random.default_rng(1025)
    return [9000.0 * rng.standard_normal(n) for n in LENGTHS]


@pytest.fixture(scope="module")
def pcm16(pcm):
    return [np.clip(x, -32768, 32767).astype(np.int16) for x in pcm]


def limited(x, device, i16):
    y, reports = J.limiter_pcm(x, HZ, GAIN, CEILING, device=device, i16=i16)
    return y + [repr(reports).encode()]


# name -> (takes int16, the call): every body (and every template instance) through its wrapper; the call returns a
# list of arrays, bytes or numbers
BODIES = {
    "resample": (False, lambda x, d: J.resample(x, HZ, 16000, device=d)),
    "loudness": (False, lambda x, d: [np.array(J.loudness(x, HZ, device=d))]),
    "true_peak": (False, lambda x, d: [np.array(J.true_peak(x, HZ, device=d))]),
    "loudness_groups": (False, lambda x, d: [repr(J.loudness_groups(x, HZ, [0] * len(x), device=d, mode=J.PEAK_TRUE,
                                                                    target=-23.0, ceiling=-1.0)).encode()]),
    "flac": (True, lambda x, d: J.flac_encode(x, HZ, device=d)),
    "flac_meta": (True, lambda x, d: J.flac_encode(x, HZ, block_size=1152, device=d, md5=True, seek_interval_ms=10)),
    "flac_md5": (True, lambda x, d: J.flac_md5(x, device=d)),
    "format": (False, lambda x, d: J.format_pcm(x, "s24", dither=True, seed=7, device=d)),
    "adpcm": (False, lambda x, d: J.adpcm_encode(x, HZ, device=d)),
    "join": (False, lambda x, d: J.join_pcm(x, ONE_PROGRAMME[:len(x)], device=d)),
    "join_i16": (True, lambda x, d: J.join_pcm(x, ONE_PROGRAMME[:len(x)], device=d)),
    "filter": (False, lambda x, d: J.filter_pcm(x, HP, HZ, device=d)),
    "filter_i16": (False, lambda x, d: J.filter_pcm(x, HP, HZ, device=d, i16=True)),
    "limiter": (False, lambda x, d: limited(x, d, False)),
    "limiter_i16": (False, lambda x, d: limited(x, d, True)),
}


def as_bytes(outs):
    return [o if isinstance(o, bytes) else np.asarray(o).tobytes() for o in outs]


@pytest.mark.parametrize("name", BODIES)
def test_no_utterance(name):
    outs = BODIES[name][1]([], -1)
    if name == "loudness_groups":
        assert J.loudness_groups([], HZ) == {"group_of": [], "groups": [], "r128": [], "lufs": []}
    elif name.startswith("limiter"):
        assert J.limiter_pcm([], HZ, GAIN, CEILING) == ([], [])
    elif name in ("loudness", "true_peak"):
        assert J.loudness([], HZ) == [] and J.true_peak([], HZ) == []
    else:
        assert outs == []


def test_empty_utterance_gives_an_empty_output(pcm, pcm16):
    for name in ("resample", "format", "filter", "filter_i16", "limiter", "limiter_i16"):
        outs = BODIES[name][1](pcm, -1)
        assert len(outs[0]) == 0 and len(outs[1]) > 0 and len(outs[2]) > 0, name
    # the join: in a programme of all three the empty member adds nothing; in one of its own it is an empty programme
    for x in (pcm, pcm16):
        (prog,) = J.join_pcm(x, ONE_PROGRAMME)
        assert prog.dtype == x[0].dtype and prog.tobytes() == np.concatenate(x).tobytes()
        own = J.join_pcm(x, [(None,)] * 3)
        assert [o.size for o in own] == LENGTHS and own[0].dtype == x[0].dtype


def test_outputs_against_the_host_seams(pcm, pcm16):
    """Every utterance of the call, the empty one above all, against what the stage's host seam or reference helper
    returns for it alone: the packing and the hand-out give each output its own share."""
    # the measurements: the numpy references (an empty utterance: -inf everywhere)
    for x, (lufs, peak), tp in zip(pcm, J.loudness(pcm, HZ), J.true_peak(pcm, HZ)):
        wl, wp = loudness_ref.integrated(x, HZ)
        wt = true_peak_ref.true_peak(x, HZ)
        for got, want in ((lufs, wl), (peak, wp), (tp, wt)):
            assert got == want if math.isinf(want) else abs(got - want) <= 1e-8, (x.size, got, want)
    groups = J.loudness_groups(pcm, HZ)  # every utterance a group of its own
    assert groups["group_of"] == [0, 1, 2]
    for x, g, r in zip(pcm, groups["groups"], groups["r128"]):
        wg, wr, _ = loudness_groups_ref.group_of_pcm([x], HZ)
        assert g["members"] == 1 and r["n_windows"] == wr["n_windows"]
        for got, want in ((g["lufs"], wg["lufs"]), (g["sample_peak_dbfs"], wg["sample_peak_dbfs"]),
                          (r["max_momentary_lufs"], wr["max_momentary_lufs"])):
            assert got == want if math.isinf(want) else abs(got - want) <= 1e-8, (x.size, got, want)
    # FLAC: the reference decoder returns the samples; the MD5 entry and STREAMINFO against the host MD5
    for x, plain, meta, digest in zip(pcm16, J.flac_encode(pcm16, HZ), BODIES["flac_meta"][1](pcm16, -1),
                                      J.flac_md5(pcm16)):
        y, info = flac_ref.decode(plain)
        assert info["total"] == x.size and np.array_equal(np.asarray(y, dtype=np.int16), x)
        y, _, meta_info = flac_check(meta)
        assert np.array_equal(np.asarray(y, dtype=np.int16), x)
        assert digest == J.md5_host(x.tobytes()) == meta_info["md5"]
    # the encoders and the stages with a host seam: byte for byte
    for x, fmt, ad, fil, fil16 in zip(pcm, J.format_pcm(pcm, "s24", dither=True, seed=7), J.adpcm_encode(pcm, HZ),
                                      J.filter_pcm(pcm, HP, HZ), J.filter_pcm(pcm, HP, HZ, i16=True)):
        assert fmt == J.format_pcm_host(x, "s24", dither=True, seed=7)
        assert ad == J.adpcm_encode_host(x, HZ)
        # (the device's tile scan against the serial recursion: |x| < 5e4 through a high-pass without a peak, 1,025
        # steps of f64 rounding each way stay under 1e-8; a share out of place is off by thousands)
        assert fil.size == x.size and np.allclose(fil, J.filter_pcm_host(x, HP, HZ), rtol=0, atol=1e-6)
        assert fil16.tobytes() == np.trunc(np.clip(fil, -32768, 32767)).astype(np.int16).tobytes()
    for x in (pcm, pcm16):
        for got, want in zip(J.join_pcm(x, ONE_PROGRAMME), J.join_host(x, ONE_PROGRAMME)):
            assert got.tobytes() == want.tobytes()
    for i16 in (False, True):
        ys, reports = J.limiter_pcm(pcm, HZ, GAIN, CEILING, i16=i16)
        for x, y, rep in zip(pcm, ys, reports):
            wy, wrep = J.limiter_host(x, HZ, GAIN, CEILING, i16=i16)
            assert y.dtype == wy.dtype and y.tobytes() == wy.tobytes() and rep == wrep


@pytest.mark.parametrize("name", BODIES)
def test_device_by_index_and_by_default_give_equal_bytes(name, pcm, pcm16):
    i16, call = BODIES[name]
    x = pcm16 if i16 else pcm
    assert as_bytes(call(x, -1)) == as_bytes(call(x, 0))


def test_the_callers_device_stays_current(pcm, pcm16):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    torch.cuda.set_device(0)
    for name, (i16, call) in BODIES.items():
        assert as_bytes(call(pcm16 if i16 else pcm, 1)) == as_bytes(call(pcm16 if i16 else pcm, 0)), name
        assert torch.cuda.current_device() == 0, name

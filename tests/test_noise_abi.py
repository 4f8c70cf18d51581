"""The noise stage without a GPU: the host rule (jb_noise_host) against its restatement in Python bit for bit, the
achieved SNR against the bound the rule implies, the active reference, the white generator's statistics, JB_NOISE_VARY,
the cases that do not mix, every refusal with the utterance and the field in jb_last_error, the struct layouts against
ctypes, and the device seam's answer on a machine without a device."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from tests import noise_ref as R

ROOT = Path(__file__).resolve().parent.parent
INVALID, DEVICE, BUFFER = -1, -3, -8
HZ = 16000


def request(bed, **kw):
    return J.noise(bed, HZ, **kw)


def sequence_of(n, bed, kw):
    return R.sequence(n, bed, kw.get("offset", 0), kw.get("seed", 0))


def test_error_codes_are_the_headers():
    hdr = (ROOT / "include" / "jbonsai_amd.h").read_text()
    for name, val in (("JB_ERR_INVALID", INVALID), ("JB_ERR_DEVICE", DEVICE), ("JB_ERR_BUFFER", BUFFER)):
        assert f"#define {name} {val}" in hdr or f"{name} = {val}" in hdr, name


@pytest.fixture(scope="module")
def restated():
    """The restatement of every shape, once: (A, C, Bs, g, y)."""
    out = []
    for x, bed, kw in R.cases():
        w = sequence_of(x.size, bed, kw)
        out.append(R.host_rule(x, w, kw["snr_db"], kw["reference"] == "active", kw["gate_db"]))
    return out


def test_host_rule_is_its_restatement_bit_for_bit(restated):
    cases = R.cases()
    assert len(cases) == len(R.LENGTHS) * (sum(len({0, lb - 1, lb // 2}) for lb in R.BEDS) + 2)
    mixed = 0
    for (x, bed, kw), (a, c, bs, g, y) in zip(cases, restated):
        got, rep = J.noise_host(x, request(bed, **kw))
        what = (x.size, None if bed is None else bed.size, kw)
        n = x.size
        assert rep.active_samples == c, what
        assert rep.speech_power == (a / c if c else 0.0) and rep.noise_power == bs / n, what
        assert rep.gain == g, what
        assert got.tobytes() == y.tobytes(), what
        assert rep.snr_db == kw["snr_db"] and rep.offset == kw.get("offset", 0) and rep.seed == kw.get("seed", 0)
        got16, _ = J.noise_host(x, request(bed, **kw), i16=True)
        assert got16.tobytes() == R.sink_i16(y).tobytes(), what
        mixed += g != 0.0
    assert mixed > len(cases) * 3 // 4  # (the shapes do mix: the comparison is not one of copies)


def test_achieved_snr_is_the_request():
    """Each of the sums A and Bs carries at most N / 1024 + 12 roundings of 2^-53 relative (up to four fused terms, eight
    tree levels, the tile sums), the gain four more (two products, two quotients; the square root halves what it is
    given): 10 log10 moves by 4.35 dB per unit relative error of a power, so the achieved SNR lies within
    8.7 (2 (N / 1024 + 12) + 4) 2^-53 dB of the request."""
    for x, bed, kw in R.cases():
        _, rep = J.noise_host(x, request(bed, **kw))
        if rep.gain == 0.0:
            continue
        n = x.size
        w = sequence_of(n, bed, kw)
        tiles = None
        if kw["reference"] == "active":
            tx = R.tile_sums(x)
            sq = R.total(tx) * R.ratio(-kw["gate_db"])
            tiles = [i for i, t in enumerate(tx) if t * float(n) >= sq * float(min(R.TILE, n - i * R.TILE))]
        got = R.achieved_snr_db(x, w, rep.gain, tiles)
        bound = 8.7 * (2 * (n / 1024 + 12) + 4) * 2.0 ** -53
        assert abs(got - kw["snr_db"]) <= bound, (n, kw, got - kw["snr_db"], bound)


def test_the_active_reference():
    rng = np.random.default_rng(5)
    t = R.TILE
    x = np.concatenate([np.zeros(8 * t), np.round(rng.standard_normal(8 * t) * 6000.0, 3), np.zeros(8 * t)])
    bed = R.bed_of(1000)
    _, whole = J.noise_host(x, request(bed, snr_db=12.0))
    _, act = J.noise_host(x, request(bed, snr_db=12.0, reference="active", gate_db=20.0))
    assert whole.active_samples == 24 * t and act.active_samples == 8 * t  # exactly the loud tiles
    assert abs(act.gain / whole.gain / math.sqrt(3.0) - 1.0) <= 1e-12
    assert abs(act.speech_power / whole.speech_power / 3.0 - 1.0) <= 1e-12
    # the loudest tile is active under every gate: its mean power is at least the utterance's
    for gate in (1.0, 2.5, 60.0):
        for seed in range(4):
            r = np.random.default_rng(seed)
            z = np.round(r.standard_normal(5 * t + 333) * r.uniform(1.0, 8000.0, 5 * t + 333), 3)
            _, rep = J.noise_host(z, request(bed, snr_db=0.0, reference="active", gate_db=gate))
            tx = R.tile_sums(z)
            means = [v / min(t, z.size - i * t) for i, v in enumerate(tx)]
            loud = int(np.argmax(means))
            assert rep.active_samples >= min(t, z.size - loud * t) and rep.gain > 0.0
    # a partial last tile is judged on its own count: 100 samples as loud as the tile in front are active at 1 dB
    # (judged as a tile of 1,024 they would lie 10 dB under the mean)
    z = np.round(np.random.default_rng(9).standard_normal(t + 100) * 3000.0, 3)
    z[t:] = np.sign(z[t:]) * 3000.0 + (z[t:] == 0) * 3000.0
    z[:t] = np.sign(z[:t]) * 3000.0 + (z[:t] == 0) * 3000.0
    _, rep = J.noise_host(z, request(bed, snr_db=0.0, reference="active", gate_db=1.0))
    assert rep.active_samples == t + 100
    z[t:] *= 0.5  # 6 dB down: out at a gate of 1 dB, in at 10 dB
    _, rep = J.noise_host(z, request(bed, snr_db=0.0, reference="active", gate_db=1.0))
    assert rep.active_samples == t
    _, rep = J.noise_host(z, request(bed, snr_db=0.0, reference="active", gate_db=10.0))
    assert rep.active_samples == t + 100


SEEDS = (1, 0xC0FFEE)


def test_the_white_generator():
    n = 65536
    var = (2.0 ** 32 - 1.0) / 3.0
    seqs = []
    for seed in SEEDS:
        w = J.noise_white(seed, 0, n)
        assert w.tobytes() == R.white(seed, 0, 4096).tobytes() + w[4096:].tobytes()  # the restatement, a stretch of it
        assert np.all(w == np.round(w)) and np.max(np.abs(w)) <= 131070
        assert abs(np.mean(w)) <= 5 * 37837 / 256          # five standard errors: sqrt(var / n) = 37837 / 256
        assert abs(np.var(w) / var - 1.0) <= 0.026         # five standard errors at the kurtosis of 2.7
        c = np.dot(w[:-1] - w.mean(), w[1:] - w.mean()) / ((n - 1) * np.var(w))
        assert abs(c) <= 0.02
        assert J.noise_white(seed, 1000, 77).tobytes() == w[1000:1077].tobytes()  # a slice of the longer call
        seqs.append(w)
    assert not np.array_equal(seqs[0], seqs[1])
    assert J.noise_white(3, 2 ** 40, 5).tobytes() == R.white(3, 2 ** 40, 5).tobytes()
    assert J.noise_white(7, 0, 0).size == 0


def test_vary_is_its_restatement():
    for seed in (0, 1, 2 ** 64 - 1, 0xDEADBEEF):
        for k in (0, 1, 255, 2 ** 33):
            for lb in (0, 1, 2, 7, 2 ** 24):
                s, o = J.noise_vary(seed, k, lb)
                assert (s, o) == R.vary(seed, k, lb)
                assert o < max(lb, 1)
    assert J.noise_vary(5, 0, 7) != J.noise_vary(5, 1, 7)  # the utterances do differ


def test_a_gain_of_zero_returns_the_input():
    x = R.signal(3000)
    x[10], x[11] = 5e-324, -1.7976931348623157e308
    bed = R.bed_of(7)
    for req in (request(bed, snr_db=float("inf")), request(np.zeros(5), snr_db=10.0),
                request(None, snr_db=float("inf"), seed=3)):
        y, rep = J.noise_host(x, req)
        assert rep.gain == 0.0 and y.tobytes() == x.tobytes()
    silent = np.zeros(2000)
    silent[::2] = -0.0
    for ref in ("whole", "active"):
        y, rep = J.noise_host(silent, request(bed, snr_db=10.0, reference=ref))
        assert rep.gain == 0.0 and rep.speech_power == 0.0 and y.tobytes() == silent.tobytes()
    # no request, an empty utterance
    assert J.noise_host(x, None)[0].tobytes() == x.tobytes()
    y, rep = J.noise_host(np.zeros(0), request(bed, snr_db=10.0))
    assert y.size == 0 and rep.gain == 0.0 and rep.active_samples == 0


def test_a_gain_given_is_taken_as_given():
    x, bed = R.signal(1500), R.bed_of(1000)
    w = R.sequence(x.size, bed, 17)
    for g in (0.5, 3.25e-3, 0.0):
        y, rep = J.noise_host(x, request(bed, snr_db=10.0, offset=17), gain=g)
        assert rep.gain == g
        assert y.tobytes() == R.host_rule(x, w, 10.0, gain=g)[4].tobytes()


def refused(call):
    with pytest.raises(J.JbError) as e:
        call()
    assert "JB_ERR_INVALID" in str(e.value)
    return str(e.value)


def test_every_refusal_names_the_utterance_and_the_field():
    x = np.zeros(8)
    ok = request([1.0, -2.0, 3.0], snr_db=10.0)

    def with_fields(white=False, **kw):
        r = request(None if white else [1.0, 0.5, 0.25], snr_db=10.0)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    nan = request([1.0, float("nan")], snr_db=10.0)
    inf = request([float("-inf")], snr_db=10.0)
    cases = [(with_fields(kind=2), "kind is neither"), (with_fields(reference=2), "reference is neither"),
             (with_fields(flags=2), "flags holds an unknown flag"), (nan, "bed holds a value that is not finite"),
             (inf, "bed holds a value that is not finite"), (with_fields(offset=3), "offset must be below bed_len"),
             (with_fields(bed_len=0), "bed_len is 0 with a bed given"), (with_fields(hz=8000), "hz differs"),
             (with_fields(snr_db=-40.5), "snr_db is not in"), (with_fields(snr_db=100.5), "snr_db is not in"),
             (with_fields(snr_db=float("nan")), "snr_db is not in"), (with_fields(snr_db=float("-inf")), "snr_db is not in"),
             (with_fields(gate_db=5.0), "gate_db must be 0"), (with_fields(reference=1, gate_db=0.5), "gate_db is not in"),
             (with_fields(reference=1, gate_db=61.0), "gate_db is not in"),
             (with_fields(reference=1, gate_db=float("nan")), "gate_db is not in"),
             (with_fields(white=True, snr_db=float("nan")), "snr_db is not in"),
             (with_fields(reserved=1), "reserved must be 0")]
    for r, what in cases:
        # through the device seam: refused before any device is touched
        msg = refused(lambda: J.noise_pcm([x, x, x], [ok, None, r], HZ))
        assert "jb_noise_pcm_batch: utterance 2: " + what in msg, msg
        msg = refused(lambda: J.noise_pcm([x, x], [r, ok], HZ, i16=True))
        assert "jb_noise_pcm_batch_i16: utterance 0: " + what in msg, msg
        if "hz" not in what:  # (the host rule has no rate of its own to hold the bed's against)
            msg = refused(lambda: J.noise_host(x, r))
            assert "jb_noise_host: utterance 0: " + what in msg, msg
    msg = refused(lambda: J.noise_pcm([x, x], [ok, ok], [HZ, 8000]))
    assert "utterance 1: hz differs" in msg and "16000 Hz against 8000 Hz" in msg
    # one request per utterance cannot vary
    msg = refused(lambda: J.noise_pcm([x], [request(None, snr_db=3.0, vary=True)], HZ))
    assert "utterance 0: flags" in msg and "JB_NOISE_VARY" in msg
    # bed == NULL with a length, a bed that is too long, a bed beside the generator
    ghost = request(None, snr_db=3.0)
    ghost.kind, ghost.bed_len = F.NOISE_BED, 4
    assert "bed is NULL" in refused(lambda: J.noise_host(x, ghost))
    long_bed = request(np.zeros(F.NOISE_MAX_BED + 1), snr_db=3.0)
    assert "bed_len is above JB_NOISE_MAX_BED" in refused(lambda: J.noise_host(x, long_bed))
    both = request([1.0, 2.0], snr_db=3.0)
    both.kind = F.NOISE_WHITE
    assert "bed is given with JB_NOISE_WHITE" in refused(lambda: J.noise_host(x, both))
    # the limits pass
    for snr in (-40.0, 100.0):
        J.noise_host(np.ones(3), request([1.0], snr_db=snr))
    for gate in (1.0, 60.0):
        J.noise_host(np.ones(3), request([1.0], snr_db=0.0, reference="active", gate_db=gate))
    # a buffer that is too small
    L = J.lib()
    dp = C.POINTER(C.c_double)
    y = np.zeros(4)
    assert L.jb_noise_host(x.ctypes.data_as(dp), 8, C.byref(ok), None, y.ctypes.data_as(dp), 4, None) == BUFFER


def test_struct_layout_header_vs_ctypes(tmp_path):
    src = tmp_path / "lay.c"
    fields = ("bed", "seed", "snr_db", "gate_db", "kind", "bed_len", "hz", "offset", "reference", "flags", "reserved")
    rfields = ("speech_power", "noise_power", "gain", "snr_db", "active_samples", "seed", "offset", "reserved")
    body = 'printf("%zu\\n", sizeof(jb_noise));'
    body += "".join(f'printf("%zu\\n", offsetof(jb_noise, {f}));' for f in fields)
    body += 'printf("%zu\\n", sizeof(jb_noise_report));'
    body += "".join(f'printf("%zu\\n", offsetof(jb_noise_report, {f}));' for f in rfields)
    body += ('printf("%u %u %u %u %u %u\\n", JB_NOISE_BED, JB_NOISE_WHITE, JB_NOISE_REF_WHOLE, JB_NOISE_REF_ACTIVE,'
             " JB_NOISE_VARY, JB_NOISE_MAX_BED);")
    src.write_text('#include "jbonsai_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' + body +
                   "return 0;}\n")
    want = ([C.sizeof(F.Noise)] + [getattr(F.Noise, f).offset for f in fields] + [C.sizeof(F.NoiseReport)] +
            [getattr(F.NoiseReport, f).offset for f in rfields] +
            [F.NOISE_BED, F.NOISE_WHITE, F.NOISE_REF_WHOLE, F.NOISE_REF_ACTIVE, F.NOISE_VARY, F.NOISE_MAX_BED])
    assert want[0] == 64 and want[12] == 56
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == want


def test_the_request_keeps_its_bed_and_copies_of_it():
    r = J.noise([1.0, -2.0, 3.0], 22050, snr_db=7.0, offset=2, reference="active", gate_db=30.0, vary=True)
    assert (r.kind, r.bed_len, r.hz, r.offset, r.reference, r.flags, r.reserved) == (0, 3, 22050, 2, 1, 1, 0)
    assert (r.snr_db, r.gate_db) == (7.0, 30.0) and [r.bed[i] for i in range(3)] == [1.0, -2.0, 3.0]
    w = J.noise(None, 0, snr_db=5.0, seed=2 ** 64 - 1)
    assert (w.kind, w.bed_len, w.seed, w.gate_db) == (1, 0, 2 ** 64 - 1, 0.0) and not w.bed
    arr, n = F.noise_array([r, None, w])
    assert n == 3 and arr[1].kind == 0 and arr[1].bed_len == 0 and not arr[1].bed and arr[0].bed[2] == 3.0
    arr, n = F.noise_array(r, 4)
    assert n == 4 and all(arr[i].bed_len == 3 for i in range(4))
    with pytest.raises(ValueError):
        J.noise(None, 0, reference="loud")


def test_entries_without_a_device():
    L = J.lib()
    assert L.jb_batch_set_noise(None, None, 0) == INVALID
    assert L.jb_batch_noise_report(None, 0, None) == INVALID
    assert L.jb_engine_set_noise(None, None) == INVALID
    assert L.jb_engine_get_noise(None, None) == INVALID
    L.jb_noise_free(None)
    if L.jb_device_count() > 0:
        return
    x = np.zeros(4)
    for i16 in (False, True):
        with pytest.raises(J.JbError) as e:
            J.noise_pcm([x], request([1.0, 0.5], snr_db=10.0), HZ, i16=i16)
        assert "JB_ERR_DEVICE" in str(e.value)

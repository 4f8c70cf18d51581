"""Per-utterance synthesis conditions in one batch on the GPU.

State level (jb_batch_create[_indexed]_voc): each utterance's alpha, beta and volume reach the mc2b, post-filter,
vocoder and MGLSA kernels; every utterance must equal the oracle's Vocoder::synthesize under its own condition, on
every vocoder path (wave kernel, wave pairs, the lane kernel's class-homogeneous waves, the serial mode, the redo
rounds).  Engine level (jb_synthesize_batch_each): utterance u equals Engine::synthesize of engines[u].  And where
every utterance has the same condition the new entries give the bits of the old ones."""
import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from jbonsai_amd.batch import VOC_NULL
from oracle import oracle as O
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, label_pool_utterances
from tests.golden.make_permuted_voice import permuted_voice_path
from tests.helpers import VERIFY_TOL, assert_pcm_close, rel_rms

pytestmark = pytest.mark.gpu
DMAX = 1.7976931348623157e308
KDB = 0.11512925464970228  # ln(10)/20


@pytest.fixture(scope="module")
def ctx():
    assert J.lib().jb_device_count() > 0
    eng = J.Engine.load([VOICE])
    return eng, synth.VoiceTables(eng), eng.voice_info()


def oracle_tracks(vi, u):
    sts = []
    for i, s in enumerate(u.streams):
        si = vi.streams[i]
        msd = s.msd if s.msd is not None else np.full(len(u.durations), DMAX)
        sts.append(O.StreamStates(si.vector_length, len(si.windows), si.is_msd, si.use_gv,
                                  [len(w) for w in si.windows], [c for w in si.windows for c in w],
                                  s.mean, s.var, msd, s.gv_mean, s.gv_var, s.gv_switch,
                                  s.gv_weight, s.msd_threshold))
    return [O.mlpg(s, u.durations) for s in sts]


def oracle_voc(vi, tr, voc, **kw):
    alpha, beta, volume = voc
    return O.vocoder(vi.sampling_frequency, vi.fperiod, alpha, volume, tr[1][:, 0], tr[0], tr[2], beta=beta, **kw)


def run(vi, utts, pcm_i16=False, **kw):
    with J.Batch(vi, utts, pcm_i16=pcm_i16, **kw) as b:
        b.run()
        b.sync()
        out = [b.pcm_i16(i) if pcm_i16 else b.pcm(i) for i in range(len(utts))]
        return out, b.info(), b.redo_stats(), b.kernel_info()


ALPHAS, VOLUMES, BETAS = (0.35, 0.42, 0.55), (0.5, 1.0, 2.7), (0.0, 0.4)


def mixed_voc(n):
    # every (alpha, volume, beta) combination turns up, in an order that interleaves the classes
    return [(ALPHAS[i % 3], BETAS[(i // 3) % 2], VOLUMES[(i // 2) % 3]) for i in range(n)]


def mixed_batch(tab, vi, nmcp, n=12, seed=0):
    utts = [synth.synth_utterance(tab, 240 + 37 * i, 500 + seed + i) for i in range(n)]
    if nmcp != vi.streams[0].vector_length:
        pairs = [synth.with_order(vi, u, nmcp) for u in utts]
        vi, utts = pairs[0][0], [p[1] for p in pairs]
    return vi, utts


# ---- 1. no behaviour change ------------------------------------------------------------------------------------

@pytest.mark.parametrize("pcm_i16", [False, True])
def test_uniform_voc_is_bitwise_the_plain_batch(ctx, pcm_i16):
    eng, tab, vi = ctx
    utts = [synth.synth_utterance(tab, 300 + 50 * i, 40 + i) for i in range(6)]
    same = [(vi.alpha, vi.beta, vi.volume)] * len(utts)
    for kw in (dict(), dict(kernel="triple", chunk_frames=32), dict(serial=True)):
        ref = run(vi, utts, pcm_i16, **kw)[0]
        for voc in (VOC_NULL, same):
            got = run(vi, utts, pcm_i16, voc=voc, **kw)[0]
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), kw
    # the indexed path
    iutts = [synth.synth_utterance(tab, 300 + 50 * i, 40 + i, indexed=True) for i in range(4)]
    ps = tab.pdf_set()
    try:
        ref = run(vi, iutts, pcm_i16, pdf_set=ps)[0]
        for voc in (VOC_NULL, same[:4]):
            got = run(vi, iutts, pcm_i16, pdf_set=ps, voc=voc)[0]
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    finally:
        ps.close()


@pytest.mark.parametrize("i16", [False, True])
def test_each_with_copies_of_one_engine_is_bitwise_synthesize_batch(ctx, i16):
    eng = ctx[0]
    labels = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2] + label_pool_utterances(6, seed=5)
    ref = eng.synthesize_batch(labels, i16=i16)
    got = J.synthesize_batch_each([eng] * len(labels), labels, i16=i16)
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))


# ---- 2. mixed conditions at state level against the oracle -----------------------------------------------------

@pytest.mark.parametrize("nmcp", [35, 30, 50])
def test_mixed_conditions_vs_oracle(ctx, nmcp):
    eng, tab, vi = ctx
    vi2, utts = mixed_batch(tab, vi, nmcp)
    voc = mixed_voc(len(utts))
    refs = []
    for u, c in zip(utts, voc):
        tr = oracle_tracks(vi2, u)
        refs.append(oracle_voc(vi2, tr, c))
    for kw in (dict(), dict(kernel="triple"), dict(kernel="triple", chunk_frames=24), dict(kernel="wave"),
               dict(serial=True)):
        got, info, _, kinfo = run(vi2, utts, voc=voc, **kw)
        if kw.get("kernel") == "triple":
            assert kinfo[0] == "k_vocoder_lt"
        for i, (g, r) in enumerate(zip(got, refs)):
            assert_pcm_close(g, r, 240, what=(nmcp, kw, i, voc[i]))


def test_mixed_conditions_indexed_path(ctx):
    eng, tab, vi = ctx
    iutts = [synth.synth_utterance(tab, 260 + 40 * i, 80 + i, indexed=True) for i in range(6)]
    voc = mixed_voc(6)
    ps = tab.pdf_set()
    try:
        got = run(vi, iutts, voc=voc, pdf_set=ps, keep_tracks=True)[0]
        with J.Batch(vi, iutts, pdf_set=ps, keep_tracks=True) as b:
            b.run()
            b.sync()
            tracks = [[b.track(i, s) for s in range(3)] for i in range(len(iutts))]
    finally:
        ps.close()
    for i in range(len(iutts)):
        ref = oracle_voc(vi, tracks[i], voc[i])
        assert_pcm_close(got[i], ref, 240, what=(i, voc[i]))


# ---- 3. an utterance of a mixed batch is the utterance alone ---------------------------------------------------

def test_mixed_batch_serial_equals_each_utterance_alone(ctx):
    eng, tab, vi = ctx
    _, utts = mixed_batch(tab, vi, 35, n=8, seed=30)
    voc = mixed_voc(len(utts))
    for i16 in (False, True):
        together = run(vi, utts, i16, voc=voc, serial=True)[0]
        for i, u in enumerate(utts):
            alone = run(vi, [u], i16, voc=[voc[i]], serial=True)[0][0]
            assert np.array_equal(together[i], alone), (i, i16)


# ---- 4. the redo rounds take the chunk's own condition ---------------------------------------------------------

@pytest.mark.parametrize("kernel", ["wave", "triple"])
def test_mixed_alpha_redo_path_vs_oracle(ctx, kernel):
    eng, tab, vi = ctx
    utts = [synth.synth_utterance(tab, 700 + 60 * i, 900 + i) for i in range(6)]
    voc = [(ALPHAS[i % 3], BETAS[i % 2], VOLUMES[(i + 1) % 3]) for i in range(6)]
    got, info, (n_part, n_full), _ = run(vi, utts, voc=voc, chunk_frames=64, warmup_frames=1, verify_tol=VERIFY_TOL,
                                         kernel=kernel)
    assert info["n_redo"] > 0 and n_part + n_full > 0, info
    for i, u in enumerate(utts):
        ref = oracle_voc(vi, oracle_tracks(vi, u), voc[i])
        assert_pcm_close(got[i], ref, 240, what=(kernel, i))


# ---- 5. as many classes as utterances in the lane kernel --------------------------------------------------------

@pytest.mark.parametrize("nmcp", [35, 50])
def test_lane_kernel_one_class_per_utterance(ctx, nmcp):
    eng, tab, vi = ctx
    vi2, utts = mixed_batch(tab, vi, nmcp, n=64, seed=200)
    voc = [(0.30 + 0.004 * i, 0.4 if i % 5 == 0 else 0.0, 0.6 + 0.03 * i) for i in range(64)]
    got, info, _, kinfo = run(vi2, utts, voc=voc, kernel="triple")
    assert kinfo[0] == "k_vocoder_lt"
    for i, u in enumerate(utts):
        ref = oracle_voc(vi2, oracle_tracks(vi2, u), voc[i])
        assert_pcm_close(got[i], ref, 240, what=(nmcp, i))


# ---- 6. Stage::NonZero (MGLSA) -----------------------------------------------------------------------------------

def lsp_utterance(tab, vi, frames, seed):
    """Spectrum stream of line spectral pairs (tests/test_gpu_stage.py's construction, narrow jitter: a filter the
    post-filter keeps stable): per state a gain and ordered frequencies on an even grid."""
    u = synth.synth_utterance(tab, frames, seed)
    rng = np.random.default_rng(seed)
    S, L = len(u.durations), vi.streams[0].vector_length
    mean, var = np.zeros((S, 3 * L)), np.zeros((S, 3 * L))
    h = np.pi / L
    base = h * (np.arange(1, L) + rng.uniform(-0.02, 0.02, L - 1))
    for s in range(S):
        mean[s, 0] = rng.uniform(0.02, 0.08)
        mean[s, 1:L] = np.sort(base + h * rng.uniform(-0.01, 0.01, L - 1))
    var[:, :L], var[:, L:] = 1e-4, 1e-3
    sts = list(u.streams)
    sts[0] = J.StreamStates(mean, var, None, None, None, None)
    return J.Utterance(u.durations, sts)


def test_stage_mixed_alpha_beta(ctx):
    """Levels of tests/test_gpu_stage.py: the MGLSA kernel on the GPU's own coefficients against the oracle's filter
    on them (1e-9: the kernel's arithmetic, with each utterance's alpha), the coefficients against the oracle's
    conversion under each utterance's alpha and beta (1e-6), end to end 1e-4."""
    eng, tab, vi = ctx
    stage = 2
    streams = [J.StreamInfo(s.vector_length, s.is_msd, s.use_gv and i != 0, s.windows) for i, s in enumerate(vi.streams)]
    v2 = J.VoiceInfo(vi.sampling_frequency, vi.fperiod, vi.alpha, streams, stage=stage, use_log_gain=False)
    utts = [lsp_utterance(tab, vi, 120 + 50 * k, 1300 + k) for k in range(6)]
    voc = [((0.42, 0.5)[k % 2], (0.0, 0.2, 0.0)[k % 3], (1.0, 0.7)[k % 2]) for k in range(6)]
    with J.Batch(v2, utts, voc=voc, keep_tracks=True) as b:
        b.run()
        b.sync()
        got = [b.pcm(i) for i in range(len(utts))]
        coef = [b.coefficients(i) for i in range(len(utts))]
        first = [b.first_coefficients(i) for i in range(len(utts))]
    for i, u in enumerate(utts):
        alpha, beta, volume = voc[i]
        tr = oracle_tracks(v2, u)
        with np.errstate(all="ignore"):
            ref = oracle_voc(v2, tr, voc[i], stage=stage)
        same = oracle_voc(v2, tr, voc[i], stage=stage, coef=coef[i], cfirst=first[i])
        assert len(got[i]) == len(ref) and np.all(np.isfinite(ref))
        assert_pcm_close(got[i], same, 240, what=i)
        want = np.stack([O.stage_coefficients(tr[0][t], alpha, beta, False, stage) for t in range(len(tr[0]))])
        assert np.abs(coef[i] - want).max() / np.abs(want).max() <= 1e-6, i
        assert rel_rms(got[i], ref) <= 1e-4, i


# ---- 7. engine level ---------------------------------------------------------------------------------------------

def _engines(base):
    conds = [dict(),
             dict(speed=0.8, half_tone=-3.0, volume=-6.0, beta=0.4),
             dict(speed=1.3, half_tone=4.0, volume=3.0, alpha=0.5),
             dict(alpha=0.5, beta=0.4, volume=-6.0, gv=(0, 0.7)),
             dict(speed=1.0, half_tone=4.0, msd=(1, 0.6), beta=0.4)]
    out = []
    for c in conds:
        e = base.clone()
        k = e.condition
        if "speed" in c:
            k.set_speed(c["speed"])
        if "half_tone" in c:
            k.set_additional_half_tone(c["half_tone"])
        if "volume" in c:
            k.set_volume(c["volume"])
        if "alpha" in c:
            k.set_alpha(c["alpha"])
        if "beta" in c:
            k.set_beta(c["beta"])
        if "gv" in c:
            k.set_gv_weight(*c["gv"])
        if "msd" in c:
            k.set_msd_threshold(*c["msd"])
        out.append((e, c))
    return out


def _check_each(engines, labels, oracle=None):
    got = J.synthesize_batch_each(engines, labels)
    got16 = J.synthesize_batch_each(engines, labels, i16=True)
    for i, (e, lab) in enumerate(zip(engines, labels)):
        alone = e.synthesize(lab)
        assert len(got[i]) == len(alone), i
        if len(alone):
            assert_pcm_close(got[i], alone, 240, what=i)
        want16 = np.clip(got[i], -32768.0, 32767.0).astype(np.int16)
        assert got16[i].dtype == np.int16 and np.array_equal(got16[i], want16), i
        if oracle is not None and oracle[i] is not None:
            ref = oracle[i]()
            assert_pcm_close(got[i], ref, 240, what=i)
    return got


def test_engine_level_each_vs_synthesize_and_oracle(ctx, oracle_voice):
    base = ctx[0]
    ecs = _engines(base)
    labels = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2] + label_pool_utterances(14, seed=17)
    engines, oracle = [], []
    for i, lab in enumerate(labels):
        e, c = ecs[i % len(ecs)]
        engines.append(e)
        if "alpha" in c:
            oracle.append(None)  # the oracle's Voice.synthesize takes the voice's alpha
            continue
        gv = [1.0, 1.0, 1.0]
        msd = [0.5, 0.5, 0.5]
        if "gv" in c:
            gv[c["gv"][0]] = c["gv"][1]
        if "msd" in c:
            msd[c["msd"][0]] = c["msd"][1]
        oracle.append(lambda lab=lab, c=c, gv=gv, msd=msd: oracle_voice.synthesize(
            lab, speed=c.get("speed", 1.0), volume=float(np.exp(c.get("volume", 0.0) * KDB)),
            half_tone=c.get("half_tone", 0.0), beta=c.get("beta", 0.0), gv_weight=gv, msd_threshold=msd))
    _check_each(engines, labels, oracle)


def test_engine_level_two_voice_pair(tmp_path):
    """Engines over nitech + the permuted nitech (one voice set) with different parameter, duration and GV weights."""
    v2 = permuted_voice_path(tmp_path)
    a = J.Engine.load([VOICE, v2])
    b = a.clone()
    a.condition.set_interpolation_duration([0.7, 0.3])
    b.condition.set_interpolation_duration([0.2, 0.8])
    for s in range(3):
        b.condition.set_interpolation_parameter(s, [0.35, 0.65])
        a.condition.set_interpolation_gv(s, [0.9, 0.1])
    b.condition.set_alpha(0.5)
    b.condition.set_volume(2.0)
    labels = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
    got = _check_each([a, b, a, b], labels)
    assert len(got[0]) != len(got[3]) or not np.array_equal(got[0], got[3])

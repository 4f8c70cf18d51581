"""Lengths exactly at the geometry constants, where off-by-one errors live: the default vocoder's checkpoints and its
single-item / chunked boundary, the fast invariant mode's chunk, checkpoint and cap boundaries, the MLPG / GV tiles
and the resident GV kernel's row limit.  The PCM goes through the local gate (tests/helpers.py assert_pcm_close): an
error after one seam shows there at its own size.  Each case asserts that it reaches the path it names (info(),
redo_stats(), kernel_info(), gang_fallbacks()); the vocoder's geometry is also what the host planner
(tests/test_vocoder_plan.py) computes for the same shape."""
import dataclasses

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from jbonsai_amd._ffi import BATCH_INVARIANT, BATCH_LANE_KERNEL, BATCH_WAVE_KERNEL
from oracle import oracle as O
from tests.conftest import VOICE
from tests.helpers import assert_pcm_close
from tests.test_gpu_configs import DMAX, oracle_pcm
from tests.test_vocoder_plan import build_probe, run_probe, summary

pytestmark = pytest.mark.gpu
FP = 240
W = 18  # the default warm-up of a batch with few hand-off positions, and the invariant mode's
# jb_device.h kVocCkpt*: the first checkpoint by chunk length (the need of a chunk is its checkpoint + 8 / + 12
# frames, jb_batch.cpp build_work), the second at 96 frames into chunks of 108 and more
CKPT = {23: 0, 24: 16, 35: 16, 36: 24, 95: 24, 96: 48, 143: 48, 144: 48, 160: 48}
CKPT2 = {144: 96, 160: 96}
GANG_TILE = 3904       # frames a resident-GV workgroup owns (jb_gv_gang.hip kGgBlockOwn)
GANG_MAX_TILES = 64    # tiles a row may have for the resident kernel (kGvGangMaxTiles), in both modes


@pytest.fixture(scope="module")
def ctx():
    assert J.lib().jb_device_count() > 0
    eng = J.Engine.load([VOICE])
    return eng, synth.VoiceTables(eng), eng.voice_info()


_oracle = {}


def oracle(vi, u, key):
    """Oracle PCM and tracks, once per utterance of the module."""
    if key not in _oracle:
        _oracle[key] = oracle_pcm(vi, u)
    return _oracle[key]


def oracle_tracks(vi, u):
    sts = []
    for i, s in enumerate(u.streams):
        si = vi.streams[i]
        msd = s.msd if s.msd is not None else np.full(len(u.durations), DMAX)
        sts.append(O.StreamStates(si.vector_length, len(si.windows), si.is_msd, si.use_gv,
                                  [len(w) for w in si.windows], [c for w in si.windows for c in w],
                                  s.mean, s.var, msd, s.gv_mean, s.gv_var, s.gv_switch, s.gv_weight, s.msd_threshold))
    return [O.mlpg(s, u.durations) for s in sts]


def run(vi, utts, pcm=True, tracks=False, **kw):
    with J.Batch(vi, utts, **kw) as b:
        b.run()
        b.sync()
        out = dict(info=b.info(), redo=b.redo_stats(), kernel=b.kernel_info(), fallbacks=b.gang_fallbacks())
        if pcm:
            out["pcm"] = [b.pcm(i) for i in range(len(utts))]
        if tracks:
            out["tracks"] = [[b.track(i, s) for s in range(3)] for i in range(len(utts))]
    return out


@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("plan"))


def planned(exe, lens, **kw):
    """(info, kernel_info) of a batch of these lengths as the host planner has them (info without n_redo)."""
    s = summary(run_probe(exe, lens, **kw))
    return (dict(chunk_frames=s["chunk"], warmup_frames=s["warmup"], n_items=s["n_items"]),
            ("k_vocoder_lt" if s["lane"] else "k_vocoder", s["waves"]))


def geometry(r):
    return {k: r["info"][k] for k in ("chunk_frames", "warmup_frames", "n_items")}, tuple(r["kernel"])


def _same(a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), what


def items(lens, c, w):
    """Work items of the vocoder: one per utterance of at most c + w frames, else one per chunk."""
    return sum(1 if T <= c + w else -(-T // c) for T in lens if T)


# ---- default mode: checkpoints --------------------------------------------------------------------------------------

def default_lengths(C):
    """Utterances whose last piece is 1 frame, exactly the first checkpoint, exactly the smallest piece that carries
    it (checkpoint + 8 / + 12), exactly the second checkpoint; one of C + W frames (one item) and one of C + W + 1
    (two chunks, the second of W + 1 frames)."""
    k = max(4, 640 // C)
    c1, c2 = CKPT[C], CKPT2.get(C, 0)
    rests = [1] + ([c1, c1 + (8 if c1 < 24 else 12)] if c1 else []) + ([c2] if c2 else [])
    return [k * C + r for r in rests if r < C] + [C + W, C + W + 1]


@pytest.mark.parametrize("kernel", ["wave", "triple"])
@pytest.mark.parametrize("C", sorted(CKPT))
def test_default_checkpoint_lengths(ctx, plan_probe, C, kernel):
    eng, tab, vi = ctx
    lens = default_lengths(C)
    utts = [synth.synth_utterance(tab, T, 9100 + T) for T in lens]
    batch = utts + [utts[0]]  # a duplicate: bitwise equal to its twin
    ser = run(vi, utts, serial=True)
    # the default tolerance: the hand-offs are certified (or redone); where all pass, the serial recursion's PCM
    r = run(vi, batch, chunk_frames=C, kernel=kernel)
    assert r["info"]["chunk_frames"] == C and r["info"]["warmup_frames"] == W, r["info"]
    assert r["info"]["n_items"] == items(lens + lens[:1], C, W), r["info"]
    assert r["kernel"][0] == {"wave": "k_vocoder", "triple": "k_vocoder_lt"}[kernel], r["kernel"]
    assert geometry(r) == planned(plan_probe, lens + lens[:1], chunk=C, first_of_kind=[1] * len(lens) + [0],
                                  flags={"wave": BATCH_WAVE_KERNEL, "triple": BATCH_LANE_KERNEL}[kernel])
    _same(r["pcm"][0], r["pcm"][-1])
    print(f"chunk {C} {kernel}: lengths {lens}, {r['info']}, redo {r['redo']}")
    for i, (u, T) in enumerate(zip(utts, lens)):
        want, _ = oracle(vi, u, T)
        assert_pcm_close(r["pcm"][i], want, FP, what=(C, kernel, T), chunk=C)
        if r["info"]["n_redo"] == 0:
            # (the hand-offs passed: what is left of the warm-up is far below their bound -- measured 1.16e-12 rel RMS,
            # 2.7e-11 in the frame at the seam at 384 frames of 577 with 96-frame chunks; the other cases ~1e-13)
            assert_pcm_close(r["pcm"][i], ser["pcm"][i], FP, tol=1e-11, local=1e-10, what=(C, kernel, T, "serial"), chunk=C)
    # a tolerance and a 2-frame warm-up under which every hand-off fails: chunks with a checkpoint settle there or go
    # on to their end, the short last pieces (no checkpoint) are recomputed to their end
    tol = {0: 1e-12, 16: 1e-9, 24: 1e-10, 48: 1e-12}[CKPT[C]]
    r = run(vi, batch, chunk_frames=C, warmup_frames=2, verify_tol=tol, kernel=kernel)
    n_part, n_full = r["redo"]
    print(f"chunk {C} {kernel} warm-up 2, tol {tol:g}: {r['info']}, settled {n_part}, to the end {n_full}")
    assert r["info"]["chunk_frames"] == C and r["info"]["warmup_frames"] == 2
    assert r["info"]["n_items"] == items(lens + lens[:1], C, 2)
    assert r["info"]["n_redo"] >= 10 and n_part + n_full >= r["info"]["n_redo"]
    assert n_full >= 1
    assert n_part >= 1 if CKPT[C] else n_part == 0
    _same(r["pcm"][0], r["pcm"][-1])
    for i, (u, T) in enumerate(zip(utts, lens)):
        want, _ = oracle(vi, u, T)
        assert_pcm_close(r["pcm"][i], want, FP, what=(C, kernel, T, "redo"), chunk=C)


# ---- fast invariant mode ---------------------------------------------------------------------------------------------

def inv_chunk(T):
    return min(max(-(-T // 96), 16), 153)


INV_LENGTHS = [34, 35, 1536, 1537, 5664, 5665, 10272, 10273, 14592, 14593]


def test_fast_invariant_geometry(ctx, plan_probe):
    """One item or chunked (34 / 35), chunks of 16 / 17, 59 / 60 (the first checkpoint), 107 / 108 (the second),
    152 / 153 (the cap): alone and inside a batch whose longest utterance sets another chunk length, the same bytes."""
    eng, tab, vi = ctx
    assert [inv_chunk(T) for T in INV_LENGTHS] == [16, 16, 16, 17, 59, 60, 107, 108, 152, 153]
    utts = [synth.synth_utterance(tab, T, 9300 + i) for i, T in enumerate(INV_LENGTHS)]
    others = [synth.synth_utterance(tab, T, 9400 + i) for i, T in enumerate((30000, 700, 20000, 3))]
    batch = others[:2] + utts + others[2:]
    inside = run(vi, batch, fast_invariant=True)
    assert inside["info"]["chunk_frames"] == inv_chunk(30000) == 153
    assert inside["info"]["warmup_frames"] == W
    assert inside["info"]["n_items"] == sum(items([T], inv_chunk(T), W) for T in INV_LENGTHS + [30000, 700, 20000, 3])
    assert geometry(inside) == planned(plan_probe, [30000, 700] + INV_LENGTHS + [20000, 3], flags=BATCH_INVARIANT)
    for i, (u, T) in enumerate(zip(utts, INV_LENGTHS)):
        alone = run(vi, [u], fast_invariant=True)
        c = inv_chunk(T)
        assert alone["info"]["chunk_frames"] == c and alone["info"]["warmup_frames"] == W
        assert alone["info"]["n_items"] == items([T], c, W), (T, alone["info"])
        assert alone["kernel"] == inside["kernel"] == ("k_vocoder_lt", 2)
        _same(alone["pcm"][0], inside["pcm"][2 + i], T)
        want, _ = oracle(vi, u, ("inv", T))
        assert_pcm_close(alone["pcm"][0], want, FP, what=T, chunk=c)


def test_fast_invariant_partial_settles(ctx):
    """A tolerance under which hand-offs fail and settle at a checkpoint: chunks of 60 frames carry the first, of 108 the
    second.  The settle decision is the chunk's own: alone and in a batch, the same bytes."""
    eng, tab, vi = ctx
    tol = 1e-12
    others = [synth.synth_utterance(tab, T, 9500 + i) for i, T in enumerate((26000, 1500, 40))]
    for T in (5665, 10273):
        u = synth.synth_utterance(tab, T, 9300 + INV_LENGTHS.index(T))
        alone = run(vi, [u], fast_invariant=True, verify_tol=tol)
        inside = run(vi, others[:1] + [u] + others[1:], fast_invariant=True, verify_tol=tol)
        n_part, n_full = alone["redo"]
        print(f"invariant {T} frames, tol {tol:g}: {alone['info']}, settled {n_part}, to the end {n_full}; "
              f"in the batch {inside['info']}, {inside['redo']}")
        assert alone["info"]["chunk_frames"] == inv_chunk(T) and alone["info"]["n_redo"] >= 1
        assert n_part >= 1 and n_part + n_full >= alone["info"]["n_redo"]
        assert inside["info"]["n_redo"] > alone["info"]["n_redo"] and inside["redo"][0] >= n_part
        _same(alone["pcm"][0], inside["pcm"][1], T)
        want, _ = oracle(vi, u, ("inv", T))
        assert_pcm_close(alone["pcm"][0], want, FP, what=T, chunk=inv_chunk(T))


# ---- the library's own choice of geometry, against the host planner -------------------------------------------------

@pytest.mark.parametrize("case", ["sentences", "4x2000_copies", "4x2000_distinct", "64x2000", "64x2000_invariant"])
def test_planner_matches_batch(ctx, plan_probe, case):
    """Chunk length, warm-up, items, kernel and waves per SIMD as the library chooses them for a batch (copies of one
    utterance count once towards the warm-up rule) are what the host planner computes from the same shape."""
    eng, tab, vi = ctx
    if case == "sentences":
        utts = [synth.synth_utterance(tab, T, 9900 + i) for i, T in enumerate((277, 420, 742))]
    elif case == "4x2000_copies":
        utts = [synth.synth_utterance(tab, 2000, 9910)] * 4
    elif case == "4x2000_distinct":
        utts = [synth.synth_utterance(tab, 2000, 9910 + i) for i in range(4)]
    else:
        utts = [synth.synth_utterance(tab, 2000, 9920 + i) for i in range(64)]
    invariant = case.endswith("_invariant")
    with J.Batch(vi, utts, fast_invariant=invariant) as b:
        lens = [b.num_frames(i) for i in range(len(utts))]
        got = geometry(dict(info=b.info(), kernel=b.kernel_info()))
    first = [1] + [0] * 3 if case == "4x2000_copies" else None
    want = planned(plan_probe, lens, first_of_kind=first, flags=BATCH_INVARIANT if invariant else 0)
    print(case, lens[:4], got)
    assert got == want, (case, got, want)


# ---- MLPG and GV tiles -----------------------------------------------------------------------------------------------

# k_mlpg band solve ring chunks (kFlCT) and build tiles (kBuildTF) of 16 frames, kFrCh 8, GV wave windows of 488 owned
# frames, workgroup tiles of 3,904, k_mlpg_gv_tp tiles of 2,048
TILE_LENGTHS = [1, 2, 3, 8, 9, 16, 17, 23, 24, 25, 487, 488, 489, 976, 977, 2048, 2049, 3903, 3904, 3905, 7808, 7809]


def mcp_close(got, want, what):
    scale = np.abs(want).max(axis=0)
    assert (np.abs(got - want).max(axis=0) <= 1e-12 * scale + 1e-13).all(), what


@pytest.fixture(scope="module")
def tile_utts(ctx):
    eng, tab, vi = ctx
    utts = []
    for i, T in enumerate(TILE_LENGTHS):
        u = synth.synth_utterance(tab, T, 9600 + i)
        if T > 1:  # GV on every frame (synth leaves the first and last phone without: a short row would have none)
            u = J.Utterance(u.durations, [s if s.gv_switch is None else
                                          dataclasses.replace(s, gv_switch=np.ones_like(s.gv_switch)) for s in u.streams])
        utts.append(u)
    return utts, [oracle_tracks(vi, u) for u in utts]


@pytest.mark.parametrize("mode", ["serial_gv", "default", "fast_invariant"])
def test_tile_lengths_tracks(ctx, tile_utts, mode):
    eng, tab, vi = ctx
    utts, refs = tile_utts
    kw = {mode: True} if mode != "default" else {}
    together = run(vi, utts, pcm=False, tracks=True, keep_tracks=True, **kw)["tracks"]
    for i, (u, ref, T) in enumerate(zip(utts, refs, TILE_LENGTHS)):
        alone = run(vi, [u], pcm=False, tracks=True, keep_tracks=True, **kw)["tracks"][0]
        for s in range(3):
            assert together[i][s].shape == ref[s].shape, (T, s)
            _same(together[i][s], alone[s], (mode, T, s))
            if mode == "serial_gv" or s > 0:  # serial-order GV sums; LF0 and LPF keep the reference's order
                _same(together[i][s], ref[s], (mode, T, s))
            else:
                mcp_close(together[i][s], ref[s], (mode, T))
    if mode == "fast_invariant":  # the multi-launch form of the resident GV kernel: the same bits
        swept = run(vi, utts, pcm=False, tracks=True, keep_tracks=True, fast_invariant=True, test_gang_timeout=True)
        assert swept["fallbacks"] == 1
        for i, T in enumerate(TILE_LENGTHS):
            for s in range(3):
                _same(swept["tracks"][i][s], together[i][s], (T, s))


@pytest.mark.parametrize("fast_invariant", [False, True])
def test_resident_gv_row_limit(ctx, fast_invariant):
    """Rows of exactly 64 gang tiles (249,856 frames) take the resident kernel, one frame more the fallback (the
    default's k_mlpg_gv_tp, the invariant mode's k_mlpg_gv_gsweep): gang_fallbacks() under an injected formation
    timeout tells which was planned.  Rows of 900 and 9,500 frames beside them keep the bits they have alone wherever
    the sums keep their shape; beside the default's fallback they stay within the MCP gate."""
    eng, tab, vi = ctx
    short = [synth.synth_utterance(tab, T, 9700 + i) for i, T in enumerate((900, 9500))]
    kw = dict(mlpg_only=True, fast_invariant=fast_invariant)
    lone = [run(vi, [u], pcm=False, tracks=True, **kw)["tracks"][0] for u in short]
    for T in (GANG_MAX_TILES * GANG_TILE, GANG_MAX_TILES * GANG_TILE + 1):
        resident = T <= GANG_MAX_TILES * GANG_TILE
        long = synth.synth_utterance(tab, T, 9702)
        r = run(vi, [long] + short, pcm=False, tracks=True, **kw)
        assert r["fallbacks"] == 0
        probe = run(vi, [long] + short, pcm=False, tracks=False, test_gang_timeout=True, **kw)
        assert probe["fallbacks"] == (1 if resident else 0), (T, probe["fallbacks"])
        for i, T2 in enumerate((900, 9500)):
            for s in range(3):
                if resident or fast_invariant or s > 0:
                    _same(r["tracks"][1 + i][s], lone[i][s], (T, T2, s))
                else:
                    np.testing.assert_allclose(r["tracks"][1 + i][s], lone[i][s], rtol=1e-12, atol=1e-13)
        assert r["tracks"][0][0].shape == (T, 35) and np.isfinite(r["tracks"][0][0]).all()


def voiced_run_utterance(vi, tab, T, start, n, seed):
    """T states of one frame each from a synthetic utterance, voiced exactly on frames [start, start + n)."""
    base = synth.synth_utterance(tab, 16 * T, seed)
    assert len(base.durations) >= T
    sts = []
    for i, s in enumerate(base.streams):
        msd = None
        if s.msd is not None:
            msd = np.full(T, 0.1)
            msd[start:start + n] = 0.9
        gs = None if s.gv_switch is None else s.gv_switch[:T].copy()
        if i == 1 and gs is not None and n < 2:
            gs[:] = 0  # (one voiced frame has zero variance: GV would divide by it)
        sts.append(J.StreamStates(s.mean[:T], s.var[:T], msd, s.gv_mean, s.gv_var, gs, s.gv_weight, s.msd_threshold))
    return J.Utterance(np.ones(T, np.uint32), sts)


def test_lf0_voiced_runs_at_tile_edges(ctx):
    """LF0 voiced runs of 1, 2, 15, 16, 17 frames at frame 0, at the end, and across the 16-frame boundary: the MSD
    stream's tracks bit for bit against the oracle's."""
    eng, tab, vi = ctx
    T = 48
    cases = []
    for n in (1, 2, 15, 16, 17):
        for start in (0, T - n, 16 - max(1, n // 2)):
            cases.append((n, start))
    utts = [voiced_run_utterance(vi, tab, T, start, n, 9800 + k) for k, (n, start) in enumerate(cases)]
    got = run(vi, utts, pcm=False, tracks=True, keep_tracks=True)["tracks"]
    for (n, start), u, g in zip(cases, utts, got):
        ref = oracle_tracks(vi, u)
        voiced = ref[1][:, 0] != O.NODATA
        assert np.flatnonzero(voiced).tolist() == list(range(start, start + n)), (n, start)
        _same(g[1], ref[1], (n, start))

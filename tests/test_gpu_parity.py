"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU
oracle on the same inputs.  Tolerances (f64 device path, sums re-associated):
  * MLPG+GV tracks: bit-exact expected (same order, no FMA); gate rel 1e-12
  * excitation: abs 1e-9 on O(1..30) values; pulse positions exactly equal
  * PCM: relative RMS <= PCM_TOL = 2 x the hand-off certification's tolerance (tests/helpers.py; north_star allows
    1e-4), length exact
"""
import numpy as np
import pytest

import jbonsai_amd as J
from oracle import oracle as O
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.helpers import VERIFY_TOL, assert_pcm_close, oracle_run, oracle_states, rel_rms, to_utt, voice_info

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def have_gpu():
    n = J.lib().jb_device_count()
    assert n > 0, "no HIP device: the product has no CPU path"
    return n


def test_bonsai_tracks_excitation_pcm(oracle_voice, have_gpu):
    v = oracle_voice
    dur, sts = oracle_states(v, SAMPLE_SENTENCE_1)
    tracks, (pcm, exc, pulse) = oracle_run(v, dur, sts, dumps=True)
    with J.Batch(voice_info(v), [to_utt(dur, sts)], keep_tracks=True) as b:
        b.run()
        b.sync()
        assert b.num_samples(0) == 66480
        for si in range(3):
            got = b.track(0, si)
            assert got.shape == tracks[si].shape
            nod = tracks[si] == O.NODATA
            assert np.array_equal(got == O.NODATA, nod)
            np.testing.assert_allclose(got, tracks[si], rtol=1e-12, atol=0)
        gexc = b.excitation(0)
        np.testing.assert_allclose(gexc, exc, rtol=0, atol=1e-9)
        got = b.pcm(0)
    assert_pcm_close(got, pcm, 240)
    # the reference's own goldens (src/lib.rs:44-46), through the GPU
    assert abs(got[2000] - 19.35141137623778) < 1e-6
    assert abs(got[30000] - -980.6757547598129) < 1e-6


def test_is_this_bonsai_and_speed(oracle_voice, have_gpu):
    v = oracle_voice
    utts, refs = [], []
    for speed in (1.0, 1.4):
        dur, sts = oracle_states(v, SAMPLE_SENTENCE_2, speed=speed)
        utts.append(to_utt(dur, sts))
        refs.append(oracle_run(v, dur, sts)[1])
    got = J.paramgen_vocode_batch(voice_info(v), utts)
    assert [len(g) for g in got] == [100800, 72000]
    for g, r in zip(got, refs):
        assert_pcm_close(g, r, 240)
    assert abs(got[0][70000] - -1898.2890228814217) < 1e-6
    assert abs(got[1][71199] - 7.840225089163972) < 1e-6


def test_batch_mixed_and_empty(oracle_voice, have_gpu):
    """Ragged batch: empty utterance, two different sentences, duplicates."""
    v = oracle_voice
    d1, s1 = oracle_states(v, SAMPLE_SENTENCE_1)
    d2, s2 = oracle_states(v, SAMPLE_SENTENCE_2)
    empty = to_utt(np.zeros(0, np.uint32), [type(s)(s.L, s.W, s.is_msd, s.use_gv, s.win_width, s.win_coef,
                                                      np.zeros((0, s.W * s.L)), np.zeros((0, s.W * s.L)),
                                                      np.zeros(0)) for s in s1])
    u1, u2 = to_utt(d1, s1), to_utt(d2, s2)
    got = J.paramgen_vocode_batch(voice_info(v), [u1, empty, u2, u1, u2])
    r1, r2 = oracle_run(v, d1, s1)[1], oracle_run(v, d2, s2)[1]
    assert len(got[1]) == 0
    assert_pcm_close(got[0], r1, 240)
    assert_pcm_close(got[2], r2, 240)
    assert np.array_equal(got[0], got[3]) and np.array_equal(got[2], got[4])


def test_volume_and_gv_weight(oracle_voice, have_gpu):
    v = oracle_voice
    dur, sts = oracle_states(v, SAMPLE_SENTENCE_1, gv_weight=(0.7, 1.3, 1.0), msd_threshold=(0.5, 0.3, 0.5))
    ref = oracle_run(v, dur, sts, volume=0.5)[1]
    got = J.paramgen_vocode_batch(voice_info(v, volume=0.5), [to_utt(dur, sts)])[0]
    assert_pcm_close(got, ref, 240)


def test_fused_mlpg_equals_generic_bitwise(oracle_voice, have_gpu):
    """With the GV sums in the reference's serial order (serial_gv) the chunk-prefetched /
    pass-fused BW=3 solver on the [dim][frame] workspace, the elementwise static-window
    kernel and the state-level prep keep the reference's order of operations: their tracks
    must equal the un-fused generic kernels' bit for bit, and the oracle's within rel 1e-12.
    The default path only changes the SHAPE of the three GV reductions (time-parallel tree
    sums): LF0 and LPF stay bit-identical, MCP agrees to 1e-12 relative."""
    v = oracle_voice
    dur, sts = oracle_states(v, SAMPLE_SENTENCE_2)
    tracks = [O.mlpg(s, dur) for s in sts]
    outs = []
    for kw in (dict(serial_gv=True), dict(generic_mlpg=True), dict()):
        with J.Batch(voice_info(v), [to_utt(dur, sts)], keep_tracks=True, **kw) as b:
            b.run()
            b.sync()
            outs.append([b.track(0, si) for si in range(3)])
    for si in range(3):
        assert np.array_equal(outs[0][si], outs[1][si]), si
        np.testing.assert_allclose(outs[0][si], tracks[si], rtol=1e-12, atol=0)
        print("stream", si, "bit-exact vs oracle:", np.array_equal(outs[0][si], tracks[si]))
        if si != 0:
            assert np.array_equal(outs[2][si], outs[0][si]), si
        np.testing.assert_allclose(outs[2][si], tracks[si], rtol=1e-12, atol=1e-13)
        d = np.abs(outs[2][si] - outs[0][si])
        print("stream", si, "time-parallel GV vs serial order: max abs diff", d.max())


def test_time_parallel_gv_is_deterministic_and_tiled(oracle_voice, have_gpu):
    """The time-parallel GV sweeps: several tiles per utterance (T > 2048 frames for the second one), ragged
    last tile, two utterances of different length in one batch; run-to-run identical bits and
    within 1e-12 of the serial-order kernel."""
    v = oracle_voice
    dur, sts = oracle_states(v, SAMPLE_SENTENCE_2)
    rng = np.random.default_rng(5)
    big = [(np.asarray(dur) * 0 + rng.integers(11, 24, len(dur))).astype(np.uint32) for _ in range(2)]
    big[1] = (big[1] * 2).astype(np.uint32)
    assert int(big[0].sum()) > 1100 and int(big[1].sum()) > 2100
    utts = [to_utt(d, sts) for d in big]
    res = []
    for kw in (dict(), dict(), dict(serial_gv=True)):
        with J.Batch(voice_info(v), utts, keep_tracks=True, **kw) as b:
            b.run()
            b.sync()
            res.append([b.track(i, 0) for i in range(2)])
    for i in range(2):
        assert np.array_equal(res[0][i], res[1][i])
        np.testing.assert_allclose(res[0][i], res[2][i], rtol=1e-12, atol=1e-13)
        ref = O.mlpg(sts[0], big[i])
        np.testing.assert_allclose(res[0][i], ref, rtol=1e-12, atol=1e-13)


@pytest.fixture(scope="module")
def ctx_long():
    """A 6000-frame synthetic utterance (seed 52: it has slowly decaying stretches, tools/warmup_sweep.py)."""
    from jbonsai_amd import synth
    from tests.conftest import VOICE

    eng = J.Engine.load([VOICE])
    return eng.voice_info(), synth.synth_utterance(synth.VoiceTables(eng), 6000, 52)


def _run_vi(vi, utts, **kw):
    with J.Batch(vi, utts, **kw) as b:
        b.run()
        b.sync()
        return [b.pcm(i) for i in range(len(utts))], b.info()


def _run(v, utts, **kw):
    with J.Batch(voice_info(v), utts, **kw) as b:
        b.run()
        b.sync()
        return [b.pcm(i) for i in range(len(utts))], b.info()


def test_chunked_equals_serial(oracle_voice, have_gpu):
    """Time-chunked execution (zero-state start 32 frames early + device-side hand-off
    check) against the one-wave-per-utterance serial recursion and the oracle."""
    v = oracle_voice
    d1, s1 = oracle_states(v, SAMPLE_SENTENCE_1)
    d2, s2 = oracle_states(v, SAMPLE_SENTENCE_2)
    utts = [to_utt(d2, s2), to_utt(d1, s1)]
    ser, info_s = _run(v, utts, serial=True)
    assert info_s["chunk_frames"] == 0 and info_s["n_items"] == 2
    chk, info_c = _run(v, utts, chunk_frames=64, warmup_frames=32)
    assert info_c["chunk_frames"] == 64 and info_c["n_items"] == 7 + 5 and info_c["n_redo"] == 0
    dflt, info_d = _run(v, utts)
    # a batch this small (697 frames) is a latency case: 6-frame chunks (below 1,024 frames; 8 below 8,192; 16
    # above: round 5), 18-frame warm-up (14 from 1000 distinct hand-off positions: tests/test_gpu_benchshapes.py
    # runs such batches)
    assert info_d["chunk_frames"] == 6 and info_d["warmup_frames"] == 18
    ref = [oracle_run(v, d2, s2)[1], oracle_run(v, d1, s1)[1]]
    for i in range(2):
        assert rel_rms(chk[i], ser[i]) <= 1e-12
        assert rel_rms(dflt[i], ser[i]) <= 1e-12
        assert_pcm_close(chk[i], ref[i], 240)
        assert_pcm_close(ser[i], ref[i], 240)
        print("chunked vs serial rel RMS", rel_rms(chk[i], ser[i]), "max abs", np.abs(chk[i] - ser[i]).max())


def test_chunk_handoff_check_triggers_redo(oracle_voice, have_gpu):
    """A 1-frame warm-up cannot pass the hand-off check: every failing chunk must be
    recomputed from its predecessor's end state, which reproduces the serial result."""
    v = oracle_voice
    d2, s2 = oracle_states(v, SAMPLE_SENTENCE_2)
    utts = [to_utt(d2, s2)]
    ser, _ = _run(v, utts, serial=True)
    out, info = _run(v, utts, chunk_frames=64, warmup_frames=1, verify_tol=VERIFY_TOL)
    assert info["n_redo"] >= 3, info
    assert rel_rms(out[0], ser[0]) <= 1e-13
    # and with the check effectively disabled the truncated warm-up is visible
    bad, info2 = _run(v, utts, chunk_frames=64, warmup_frames=1, verify_tol=1e30)
    assert info2["n_redo"] == 0 and rel_rms(bad[0], ser[0]) > 1e-6


def test_partial_redo_at_checkpoint(ctx_long, have_gpu):
    """Chunks of >= 96 frames leave a checkpoint state 48 frames in.  A failing chunk is first
    recomputed only up to it; where the recomputed state meets the checkpoint the rest of the
    chunk stands (certified to the same tolerance as an ordinary hand-off), elsewhere the
    recomputation runs on to the end.  With a 6-frame warm-up most hand-offs fail; both outcomes
    must occur and the PCM must match the serial recursion to the hand-off tolerance."""
    vi, u = ctx_long
    ser, _ = _run_vi(vi, [u], serial=True)
    for kern in ("wave", "triple"):
        with J.Batch(vi, [u, u], chunk_frames=160, warmup_frames=6, verify_tol=VERIFY_TOL, kernel=kern) as b:
            b.run()
            b.sync()
            info, (n_part, n_full) = b.info(), b.redo_stats()
            out = [b.pcm(0), b.pcm(1)]
        assert info["n_redo"] >= 10 and n_part >= 2 and n_part + n_full == info["n_redo"], (info, n_part, n_full)
        assert np.array_equal(out[0], out[1])
        e = rel_rms(out[0], ser[0])
        print(kern, "hand-offs failing", info["n_redo"], "settled at checkpoint", n_part, "to the end", n_full,
              "rel RMS vs serial", e)
        assert_pcm_close(out[0], ser[0], 240, what=kern, chunk=160)
    # the second checkpoint (96 frames into chunks of 144 and more): with a 2-frame warm-up and a tolerance of 1e-12
    # some chunks have not converged 48 frames in and go on to the second checkpoint (JB_REDO_TRACE=1 shows them);
    # with a tolerance below the rounding differences of the two kernels nothing ever settles and every chunk is
    # recomputed to its end through both checkpoints.  Either way the result is the serial recursion's.
    for tol, all_full in ((1e-12, False), (1e-17, True)):
        with J.Batch(vi, [u, u], chunk_frames=160, warmup_frames=2, verify_tol=tol, kernel="triple") as b:
            b.run()
            b.sync()
            info, (n_part, n_full) = b.info(), b.redo_stats()
            e = rel_rms(b.pcm(0), ser[0])
            assert np.array_equal(b.pcm(0), b.pcm(1))
        print("second checkpoint, tol", tol, ": hand-offs failing", info["n_redo"], "settled at a checkpoint", n_part,
              "to the end", n_full, "rel RMS vs serial", e)
        assert info["n_redo"] >= 10 and e <= 1e-11
        assert (n_full >= 10 and n_part == 0) if all_full else n_part >= 10
    # the shorter checkpoints: 24 frames into chunks of 36-95 frames, 16 into chunks of 24-35 (a few long utterances)
    for chunk in (40, 32):
        with J.Batch(vi, [u], chunk_frames=chunk, warmup_frames=10, verify_tol=VERIFY_TOL, kernel="wave") as b:
            b.run()
            b.sync()
            info, (n_part, n_full) = b.info(), b.redo_stats()
            e = rel_rms(b.pcm(0), ser[0])
            assert_pcm_close(b.pcm(0), ser[0], 240, what=chunk, chunk=chunk)
        print("chunk", chunk, "hand-offs failing", info["n_redo"], "settled at checkpoint", n_part, "to the end", n_full,
              "rel RMS vs serial", e)
        assert info["n_redo"] >= 5 and n_part >= 1 and n_part + n_full == info["n_redo"]
    # 32-frame warm-up, the default-like case: whatever fails, the result stays certified
    with J.Batch(vi, [u], chunk_frames=136, warmup_frames=32, kernel="triple") as b:
        b.run()
        b.sync()
        assert_pcm_close(b.pcm(0), ser[0], 240)


def test_pair_kernel_equals_wave_kernel_and_oracle(oracle_voice, have_gpu):
    """The lane-pair throughput kernel (one chunk per lane pair, state in registers) against
    the wave-per-chunk kernel, the serial recursion and the oracle; also through the
    re-do path, which hands its end states to the wave kernel (shared state layout)."""
    v = oracle_voice
    d1, s1 = oracle_states(v, SAMPLE_SENTENCE_1)
    d2, s2 = oracle_states(v, SAMPLE_SENTENCE_2)
    utts = [to_utt(d2, s2), to_utt(d1, s1), to_utt(d2, s2)]
    ser, _ = _run(v, utts, serial=True)
    wav, _ = _run(v, utts, chunk_frames=64, warmup_frames=32, kernel="wave")
    par, info = _run(v, utts, chunk_frames=64, warmup_frames=32, kernel="triple")
    assert info["n_redo"] == 0 and info["n_items"] == 7 + 5 + 7
    ref = [oracle_run(v, d2, s2)[1], oracle_run(v, d1, s1)[1]]
    for i in range(3):
        assert rel_rms(par[i], ser[i]) <= 1e-12, i
        assert rel_rms(par[i], wav[i]) <= 1e-12, i
    assert_pcm_close(par[0], ref[0], 240)
    assert_pcm_close(par[1], ref[1], 240)
    assert np.array_equal(par[0], par[2])
    print("pair vs serial rel RMS", rel_rms(par[0], ser[0]), rel_rms(par[1], ser[1]))
    redo, info2 = _run(v, utts, chunk_frames=64, warmup_frames=1, verify_tol=VERIFY_TOL, kernel="triple")
    assert info2["n_redo"] >= 6
    for i in range(3):
        assert rel_rms(redo[i], ser[i]) <= 1e-12, i


def test_i16_sink_equals_clamped_cast_of_f64(oracle_voice, have_gpu):
    """Fused 16-bit sink (examples/is-bonsai/main.rs:44-48: min/max clamp, `as i16`):
    every vocoder kernel must write exactly clip(f64).astype(int16) of its own f64 output, with a
    volume that makes the clamp bite."""
    v = oracle_voice
    d1, s1 = oracle_states(v, SAMPLE_SENTENCE_1)
    d2, s2 = oracle_states(v, SAMPLE_SENTENCE_2)
    utts = [to_utt(d2, s2), to_utt(d1, s1)] * 4
    for kw in (dict(serial=True), dict(chunk_frames=64, kernel="wave"), dict(chunk_frames=64, kernel="triple"),
               dict(chunk_frames=64)):
        res = []
        for i16 in (False, True):
            with J.Batch(voice_info(v, volume=9.0), utts, pcm_i16=i16, **kw) as b:
                b.run()
                b.sync()
                res.append([b.pcm_i16(i) if i16 else b.pcm(i) for i in range(len(utts))])
                if i16:
                    with pytest.raises(J.JbError):
                        b.pcm(0)
        for f, q in zip(*res):
            want = np.clip(f, -32768.0, 32767.0).astype(np.int16)  # astype truncates toward zero
            assert q.dtype == np.int16 and np.array_equal(q, want)
            assert (np.abs(f) > 32768).any() and (want == 32767).any() and (want == -32768).any()


def test_device_pcm_slab_as_torch_tensor(have_gpu):
    """jb_batch_device_pcm + pcm_offset: the contiguous device slab a caller would hand to an RCCL
    gather, viewed zero-copy as a torch tensor, holds exactly what read_pcm returns.
    Runs in a child process: torch must be imported before the library so that both share one HIP
    runtime (as in bench.py); this pytest process has loaded the library long ago."""
    import subprocess
    import sys
    import textwrap

    pytest.importorskip("torch")
    code = textwrap.dedent("""
        import torch, numpy as np
        assert torch.cuda.is_available()
        import jbonsai_amd as J
        from bench import pcm_slab_tensor
        from oracle import oracle as O
        from tests.conftest import VOICE
        from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
        from tests.helpers import oracle_states, to_utt, voice_info
        v = O.Voice(VOICE)
        d1, s1 = oracle_states(v, SAMPLE_SENTENCE_1)
        d2, s2 = oracle_states(v, SAMPLE_SENTENCE_2)
        utts = [to_utt(d2, s2), to_utt(d1, s1), to_utt(d2, s2)]
        for i16 in (False, True):
            with J.Batch(voice_info(v), utts, pcm_i16=i16) as b:
                b.run(); b.sync()
                t = pcm_slab_tensor(b)
                assert t.is_cuda and t.numel() == b.total_samples
                host = t.cpu().numpy()
                for i in range(3):
                    o, n = b.pcm_offset(i), b.num_samples(i)
                    assert np.array_equal(host[o:o + n], b.pcm_i16(i) if i16 else b.pcm(i))
        print("slab ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       cwd=str(__import__("pathlib").Path(__file__).resolve().parents[1]))
    assert r.returncode == 0 and "slab ok" in r.stdout, r.stdout + r.stderr


def test_removed_cu_partition_field_must_be_zero(oracle_voice, have_gpu):
    """jb_batch_opts.reserved0 was mlpg_cus_per_xcd in rounds 1-3 (a CU partition that lost at every split and
    whose masked streams could not be destroyed reliably; removed in round 4): a caller that still sets it is
    told so instead of silently running unpartitioned."""
    import ctypes as C

    from jbonsai_amd import _ffi as F

    v = oracle_voice
    d1, s1 = oracle_states(v, SAMPLE_SENTENCE_1)
    u = to_utt(d1, s1)
    vd, keep = voice_info(v).c_struct()
    arr = (F.StateUtt * 1)()
    arr[0] = u.c_struct()
    opts = F.BatchOpts()
    opts.device, opts.reserved0 = -1, 8
    h = C.c_void_p()
    assert F.lib().jb_batch_create(C.byref(vd), arr, 1, C.byref(opts), C.byref(h)) == -2  # JB_ERR_UNSUPPORTED
    opts.reserved0 = 0
    assert F.lib().jb_batch_create(C.byref(vd), arr, 1, C.byref(opts), C.byref(h)) == 0
    F.lib().jb_batch_free(h)
    del keep

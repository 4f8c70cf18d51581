"""The shapes bench.py QUOTES numbers on, under the oracle (round 4; VERDICT r3 "next" 3):

  config4 / config5 records: 1024 distinct synthetic utterances x 6,386 frames created from pdf row indices
      (bench.py resident_record, ids 4000+i / 5000+i; config 5 over two different voices 0.5/0.5) -- four
      utterances of each against the oracle;
  config3_job: ONE pass of the 4096-utterance mixed-length list (bench.py config3_shard at N = 1: LPT into
      sub-batches of <= 7 M frames, created from pdf row indices): every utterance's length, eight utterances
      per sub-batch read back and finite, one per sub-batch against the oracle.
Tolerance: relative RMS <= PCM_TOL (tests/helpers.py) per utterance (north_star allows 1e-4), lengths exact."""
import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import shard, synth
from tests.conftest import VOICE
from tests.golden.make_permuted_voice import permuted_voice_path
from tests.helpers import PCM_TOL, assert_pcm_close, rel_rms
from tests.test_gpu_configs import oracle_pcm

pytestmark = pytest.mark.gpu
FRAMES = 6386       # bench.py CONFIG45_FRAMES
PICKS = (0, 341, 682, 1023)
SUB_BATCH_FRAMES = 7_000_000  # bench.py SUB_BATCH_FRAMES


def test_bench_constants_match():
    import bench

    assert bench.CONFIG45_FRAMES == FRAMES and bench.SUB_BATCH_FRAMES == SUB_BATCH_FRAMES


def test_config4_at_the_bench_shape():
    eng = J.Engine.load([VOICE])
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    pset = tab.pdf_set()
    utts = [synth.synth_utterance(tab, FRAMES, 4000 + i, indexed=True) for i in range(1024)]
    with J.Batch(vi, utts, pdf_set=pset) as b:
        b.run()
        b.sync()
        assert all(b.num_samples(i) == FRAMES * 240 for i in range(1024))
        got = {i: b.pcm(i) for i in PICKS}
        info = b.info()
    print("config 4 at the bench shape:", info)
    for i in PICKS:
        ref, _ = oracle_pcm(vi, synth.synth_utterance(tab, FRAMES, 4000 + i))
        assert_pcm_close(got[i], ref, 240, what=i)
    pset.close()


def test_config5_at_the_bench_shape(tmp_path):
    eng = J.Engine.load([VOICE, permuted_voice_path(tmp_path)])
    tabs = [synth.VoiceTables(eng, 0), synth.VoiceTables(eng, 1)]
    half = {"duration": [0.5, 0.5], "parameter": [[0.5, 0.5]] * 3, "gv": [[0.5, 0.5]] * 3}
    vi = eng.voice_info()
    pset = synth.voice_set_pdf_set(tabs)
    utts = [synth.synth_utterance_voices(tabs, half, FRAMES, 5000 + i, indexed=True) for i in range(1024)]
    with J.Batch(vi, utts, pdf_set=pset) as b:
        b.run()
        b.sync()
        assert all(b.num_samples(i) == FRAMES * 240 for i in range(1024))
        got = {i: b.pcm(i) for i in PICKS}
    for i in PICKS:
        ref, _ = oracle_pcm(vi, synth.synth_utterance_voices(tabs, half, FRAMES, 5000 + i))
        assert_pcm_close(got[i], ref, 240, what=i)
    pset.close()


def test_bench_plain_run_prints_the_headline_alone():
    """A run without --full times the headline and nothing else: the line carries the headline's keys, and none of
    the records that only --full measures (CPU baseline, error against the oracle, extras, the config-3 job)."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--batch", "3", "--frames", "600",
                        "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["config"]["samples_per_step_per_gpu"] / (d["ms_per_step"] * 1e-3))
    for key in ("cpu_baseline", "error_vs_oracle", "two_batches_in_flight", "d2h_inclusive", "host_visible",
                "copies_over_seeds", "distinct_64", "labels_to_pcm", "config4", "config5", "order49",
                "batch_invariant", "config3_job", "config3_strong", "config3_job_n1"):
        assert key not in d, key


def test_bench_dump_outputs_are_the_timed_batch_pcm(tmp_path):
    """`bench.py --dump-outputs DIR` writes the PCM a caller of the timed batch reads (all of it for an output this
    small), and the line reports the --steps it timed."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--batch", "3", "--frames", "600",
                        "--steps", "3", "--warmup", "1", "--no-extras", "--no-cpu-baseline", "--dump-outputs",
                        str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    pcm, idx, lens = (np.load(tmp_path / f"{n}.npy") for n in ("pcm", "pcm_index", "pcm_lengths"))
    assert pcm.dtype == idx.dtype == lens.dtype == np.float64
    eng = J.Engine.load([VOICE])
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    vi.beta = 0.0  # bench.py --beta default
    utt = synth.synth_utterance(tab, 600, 0)
    with J.Batch(vi, [utt] * 3) as b:
        b.run()
        b.sync()
        want = [b.pcm(i) for i in range(3)]
    assert lens.tolist() == [len(w) for w in want]
    assert idx.tolist() == [[i, k] for i, w in enumerate(want) for k in range(len(w))]
    for i, w in enumerate(want):
        got = pcm[idx[:, 0] == i]
        # (bench.py's dump against the library's own batch of the same utterances, not the oracle: the plain gate)
        assert np.abs(got).max() > 1.0 and rel_rms(got, w) <= PCM_TOL, i


def test_one_pass_of_the_config3_job():
    eng = J.Engine.load([VOICE])
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    pset = tab.pdf_set()
    lens = synth.mixed_lengths(4096)  # bench.py config3_shard at world size 1
    mine = shard.shard_for_rank(lens, 0, 1)
    assert sorted(mine) == list(range(4096))
    k = max(1, -(-sum(lens) // SUB_BATCH_FRAMES))
    subs = shard.lpt_partition([lens[i] for i in mine], k)
    assert sorted(j for sb in subs for j in sb) == list(range(4096))
    checked = 0
    for sb in subs:
        ids = [mine[j] for j in sb]
        utts = [synth.synth_utterance(tab, lens[i], 2000 + i, indexed=True) for i in ids]
        with J.Batch(vi, utts, pdf_set=pset) as b:
            b.run()
            b.sync()
            assert [b.num_samples(q) for q in range(len(ids))] == [lens[i] * 240 for i in ids]
            order = np.argsort([lens[i] for i in ids])
            look = list(order[:2]) + list(order[len(order) // 2:len(order) // 2 + 3]) + list(order[-3:])
            pcm = {int(q): b.pcm(int(q)) for q in look}
        for q, a in pcm.items():
            assert np.isfinite(a).all() and np.abs(a).max() > 1.0, ids[q]
        q = int(order[1])  # one of the shortest: the oracle takes ~0.15 s per 1000 frames
        ref, _ = oracle_pcm(vi, synth.synth_utterance(tab, lens[ids[q]], 2000 + ids[q]))
        assert_pcm_close(pcm[q], ref, 240, what=ids[q])
        checked += 1
    assert checked == len(subs) >= 8
    pset.close()

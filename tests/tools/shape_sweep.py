"""Shape sweep on the GPU box: seeded random COMBINATIONS of mel-cepstral order (2..64: every taps-per-lane form of
the vocoder kernels), frame period (5..400, any), low-pass order (odd, 1..127), warping alpha, post-filter beta,
volume, kernel choice and chunk length, each on a small ragged batch -- every utterance against the oracle.  The
tests hold ten such combinations (test_random_shape_combinations); this is the wide version.

    python tests/tools/shape_sweep.py [--n 120] > profiles/rNN_shape_sweep.txt
"""
import argparse
import dataclasses
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

DMAX = 1.7976931348623157e308


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=120)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import jbonsai_amd as J
    from jbonsai_amd import synth
    from oracle import oracle as O
    from tests.conftest import VOICE
    from tests.helpers import LOCAL_TOL, PCM_TOL, VERIFY_TOL, frame_err

    eng = J.Engine.load([VOICE])
    tab = synth.VoiceTables(eng)
    vi = eng.voice_info()
    L, W, NL = vi.streams[0].vector_length, len(vi.streams[0].windows), vi.streams[2].vector_length
    worst, fails, t0, above = (0.0, None), [], time.perf_counter(), 0
    hist = {}
    worst_fe, fes, by_cat = (0.0, None), [], {}
    for case in range(a.n):
        rng = np.random.default_rng(50_000 + 1000 * a.seed + case)
        L2 = int(rng.choice([2, 3, 5, 8, 12, 13, 20, 24, 25, 30, 35, 36, 37, 40, 48, 49, 50, 60, 61, 62, 64]))
        fp = int(rng.choice([5, 16, 27, 30, 31, 40, 64, 65, 75, 80, 83, 96, 100, 110, 120, 127, 128, 131, 160, 200, 220,
                             240, 241, 254, 256, 257, 320, 331, 400]))
        fs = int(rng.choice([8000, 16000, 22050, 44100, 48000]))
        nlpf = int(rng.choice([1, 3, 7, 15, 23, 31, 33, 63, 65, 127]))
        alpha = float(rng.choice([0.31, 0.42, 0.5, 0.55, 0.58]))
        beta = float(rng.choice([0.0, 0.0, 0.0, 0.2, 0.5]))
        volume = float(rng.choice([1.0, 0.5, 1.7]))
        kw = [dict(), dict(), dict(serial=True), dict(chunk_frames=32, kernel="triple"), dict(chunk_frames=16, kernel="wave"),
              dict(chunk_frames=24, warmup_frames=6, verify_tol=VERIFY_TOL)][int(rng.integers(0, 6))]
        lens = [int(x) for x in rng.integers(1, 500, size=3)]
        utts = []
        for k, T in enumerate(lens):
            u = synth.synth_utterance(tab, T, 13 * case + k)
            S = len(u.durations)
            m0, s2 = u.streams[0], u.streams[2]
            mean = m0.mean.reshape(S, W, L)
            var = m0.var.reshape(S, W, L)
            gvm, gvv = m0.gv_mean, m0.gv_var
            if L2 <= L:
                mean, var, gvm, gvv = mean[:, :, :L2], var[:, :, :L2], gvm[:L2], gvv[:L2]
            else:  # higher orders: small extra cepstral coefficients behind the voice's 35
                ex = L2 - L
                mean = np.concatenate([mean, rng.normal(0.0, 2e-3, (S, W, ex))], axis=2)
                var = np.concatenate([var, np.tile(var[:, :, -1:], (1, 1, ex))], axis=2)
                gvm = np.concatenate([gvm, np.full(ex, gvm[-1])])
                gvv = np.concatenate([gvv, np.full(ex, gvv[-1])])
            st0 = dataclasses.replace(m0, mean=np.ascontiguousarray(mean.reshape(S, W * L2)),
                                      var=np.ascontiguousarray(var.reshape(S, W * L2)), gv_mean=gvm.copy(), gv_var=gvv.copy())
            if nlpf <= NL:
                lo = (NL - nlpf) // 2
                lm, lv = s2.mean[:, lo:lo + nlpf].copy(), s2.var[:, lo:lo + nlpf].copy()
            else:
                lo = (nlpf - NL) // 2
                lm = rng.normal(0.0, 2e-3, (S, nlpf))
                lv = np.full((S, nlpf), float(s2.var.mean()))
                lm[:, lo:lo + NL] = s2.mean
                lv[:, lo:lo + NL] = s2.var
            utts.append(J.Utterance(u.durations, [st0, u.streams[1], dataclasses.replace(s2, mean=lm, var=lv)]))
        streams = [dataclasses.replace(vi.streams[0], vector_length=L2), vi.streams[1],
                   dataclasses.replace(vi.streams[2], vector_length=nlpf)]
        vi2 = dataclasses.replace(vi, sampling_frequency=fs, fperiod=fp, alpha=alpha, beta=beta, volume=volume, streams=streams)
        desc = f"nmcp {L2} fperiod {fp} nlpf {nlpf} alpha {alpha} beta {beta} volume {volume} {kw} frames {lens}"
        try:
            with J.Batch(vi2, utts, **kw) as b:
                b.run()
                b.sync()
                got = [b.pcm(i) for i in range(len(utts))]
                kern = b.kernel_info()[0]
        except J.JbError as e:
            fails.append((case, desc, "JbError: " + str(e)))
            continue
        hist[kern] = hist.get(kern, 0) + 1
        for u, g, T in zip(utts, got, lens):
            sts = []
            for i, s in enumerate(u.streams):
                si = vi2.streams[i]
                msd = s.msd if s.msd is not None else np.full(len(u.durations), DMAX)
                sts.append(O.StreamStates(si.vector_length, len(si.windows), si.is_msd, si.use_gv,
                                          [len(w) for w in si.windows], [c for w in si.windows for c in w],
                                          s.mean, s.var, msd, s.gv_mean, s.gv_var, s.gv_switch, s.gv_weight, s.msd_threshold))
            tr = [O.mlpg(s, u.durations) for s in sts]
            ref = O.vocoder(fs, fp, alpha, volume, tr[1][:, 0], tr[0], tr[2], beta=beta)
            den = np.sqrt(np.mean(ref * ref))
            e = float(np.sqrt(np.mean((g - ref) ** 2)) / (den if den > 0 else 1.0)) if len(g) == len(ref) else float("inf")
            if not np.isfinite(ref).all():
                continue  # (an unstable filter on both sides says nothing)
            if e > worst[0]:
                worst = (e, desc)
            fe, f = frame_err(g, ref, fp) if len(g) == len(ref) else (float("inf"), -1)
            fes.append(fe)
            cat = "beta > 0" if beta > 0 else "nmcp > 40" if L2 > 40 else "other"
            by_cat[cat] = max(by_cat.get(cat, 0.0), fe)
            if fe > worst_fe[0]:
                worst_fe = (fe, f"{desc}, utterance of {T} frames, frame {f}")
            above += e > VERIFY_TOL
            # what the certification bounds is the filter STATE at a hand-off (VERIFY_TOL, relative); the PCM behind it
            # can carry a little more while the difference decays (strong post-filter, high order): the gate is the
            # tests' own, PCM_TOL = 2 x VERIFY_TOL (tests/helpers.py); the count above VERIFY_TOL itself is printed
            if not e <= PCM_TOL:
                fails.append((case, desc, f"rel RMS {e:.3e} at {T} frames"))
            # (the local gate is reported, not enforced, here: these shapes include the orders and post-filters the
            # tests hold to a per-path constant)
    print(f"{a.n} random shape combinations x 3 utterances against the oracle in {time.perf_counter() - t0:.0f} s; kernels: {hist}")
    print(f"worst relative RMS {worst[0]:.3e}  ({worst[1]})   gate {PCM_TOL:g} (tests/helpers.py); {above} of {3 * a.n} utterances above {VERIFY_TOL:g}")
    fes = np.array(fes)
    print(f"worst frame (frame_err) {worst_fe[0]:.3e}  ({worst_fe[1]})   p99 {np.quantile(fes, 0.99):.3e}  median"
          f" {np.median(fes):.3e}; {int(np.sum(fes > LOCAL_TOL))} of {len(fes)} above LOCAL_TOL {LOCAL_TOL:g}")
    print("worst frame_err by shape:", {k: f"{v:.3e}" for k, v in sorted(by_cat.items())})
    for f in fails[:20]:
        print("FAIL", f)
    print("PARITY GREEN" if not fails else f"PARITY RED: {len(fails)} failures")
    sys.exit(0 if not fails else 1)


if __name__ == "__main__":
    main()

"""Measure what tests/test_vocoder_tv_ref.py gates and write profiles/r26_vocoder_tv.txt:
  * the agreement of the time-varying reference (tests/vocoder_tv_ref.py) with the transfer-function reference
    (tests/mlsa_ref.py) on frozen rows and on the two ramp shapes;
  * the oracle's distance from the reference on every case of tests/vocoder_tv_cases.py, the worst per class and the
    gates (8 x);
  * seven mutations of the oracle's frame loop and excitation, each built from a SCRATCH COPY of oracle/ in a temporary
    directory (the tree is not touched), over the same table: the largest err / gate.

    python -m tests.tools.vocoder_tv_study [profiles/r26_vocoder_tv.txt [gpu_stdout.log [pcm.jsonl]]]

The two logs are those of a GPU run of tests/test_gpu_vocoder_tv.py: pytest -s's output and JB_PCM_LOG's file."""
import json
import re
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

from oracle import oracle as O
from tests import mlsa_cases as C
from tests import mlsa_ref as R
from tests import vocoder_tv_cases as T
from tests import vocoder_tv_ref as V

ROOT = Path(__file__).resolve().parents[2]

INC = "            for (size_t k = 0; k < nmcp; k++)\n                c[k] += cinc[k];\n"
ZERO_DF = "            df1(&f, &x, alpha, c);\n            df2(&f, &x, alpha, c, nmcp);\n"
MGLSA_DF = "            jbo_mglsa_df(d, stage, nmcp, &x, alpha, c);\n"
DEST = "(lpf + (g_i + i < g_left ? (g_i + i) / g_f : (g_left - 1) / g_f) * e->nring)"
# (name, [(old text, new text)]) on oracle/jbo_hot.c; every old text must occur
MUTATIONS = [
    ("the coefficient increment applied before df instead of after",
     [(ZERO_DF + INC, INC + ZERO_DF), (MGLSA_DF + INC, INC + MGLSA_DF)]),
    ("the end-of-frame snap of the coefficients dropped",
     [("        memcpy(c, cc, sizeof(double) * nmcp);\n", "")]),
    ("the first frame taken from the filtered row",
     [("            mc2b(pf, cc, nmcp, alpha);\n",
       "            mc2b(pf, cc, nmcp, alpha);\n            if (t == 0)\n                memcpy(c, cc, sizeof(double) * nmcp);\n")]),
    ("the pitch increment from the new frame's period on both sides",
     [("(pitch - e->pitch_of_curr_point) / (double)fperiod", "(pitch - pitch) / (double)fperiod")]),
    ("the antipode at nlpf / 2",
     [("(e->nring - 1) / 2", "e->nring / 2")]),
    ("the taps of the destination sample's frame instead of the source's",
     [("static double exc_get(", "static size_t g_i, g_f, g_left; /* sample in the frame, frame period, samples left */\nstatic double exc_get("),
      ("e->ring[e->index + i] += c * lpf[i];", "e->ring[e->index + i] += c * %s[i];" % DEST),
      ("e->ring[i] += c * lpf[nright + i];", "e->ring[i] += c * %s[nright + i];" % DEST.replace("g_i + i", "g_i + nright + i")),
      ("            double x = exc_get(&e, lp, &pu);\n",
       "            g_i = i, g_f = fperiod, g_left = (T - t) * fperiod;\n            double x = exc_get(&e, lp, &pu);\n")]),
    ("the noise not drawn on voiced samples (nlpf >= 1)",
     [("        double noise = nrandom(&e->random);\n",
       "        double noise = e->pitch_of_curr_point == 0.0 ? nrandom(&e->random) : 0.0;\n")]),
]


def table_errors():
    """{case name: (class, err, err / gate)} with the oracle library that is bound now."""
    out = {}
    with np.errstate(all="ignore"):
        for s in T.EXC_SHAPES:
            for u in T.exc_cases(s):
                e = T.exc_err(T.oracle_excitation(u), T.expected_excitation(s, u.name.rsplit("-", 1)[1]))
                out[u.name] = ("exc", e)
        for s in T.FILTER_SHAPES:
            for u, want in zip(T.filter_cases(s), T.expected_pcm(s)):
                out[u.name] = (T.filter_class(s), C.err_in_u(T.oracle_pcm(s, u), want))
    return {k: (c, e if np.isfinite(e) else float("inf"), (e if np.isfinite(e) else float("inf")) / T.GATE[c])
            for k, (c, e) in out.items()}


def build_mutant(edits, tmp):
    src = Path(tmp) / "oracle"
    shutil.copytree(ROOT / "oracle", src, ignore=shutil.ignore_patterns("build", "_ref", "__pycache__"))
    f = src / "jbo_hot.c"
    text = f.read_text()
    for old, new in edits:
        assert old in text, old
        text = text.replace(old, new)
    f.write_text(text)
    subprocess.run(["make", "-C", str(src)], check=True, capture_output=True)
    return src / "build" / "libjbo_oracle.so"


def agreement():
    lines = []
    for shape, exc in T.FROZEN:
        case = C.build_case(shape, exc)
        e = V.excitation(case.lf0_track(), case.fs, case.fperiod, np.ones((case.frames, 1)), C.noise())[0]
        if case.stage:
            c = C.oracle_coefficients(case)
            rows, first = np.tile(c, (case.frames, 1)), c
        else:
            rows, first = V.zero_rows(case.mc, case.alpha, 0.0)
        got = V.synthesize([e], [rows], [first], case.fperiod, case.alpha, case.volume, case.stage)[0]
        lines.append("%-34s %9.3f" % (case.name, C.err_in_u(got, C.expected_pcm(case, 1))))
    return lines


def gpu_section(stdout_log, pcm_log=None):
    """What a GPU run of tests/test_gpu_vocoder_tv.py printed (pytest -s) and logged (JB_PCM_LOG), worst per group."""
    from tests.helpers import LOCAL_TOL, PCM_TOL

    lines = ["", "GPU against the same reference (tests/test_gpu_vocoder_tv.py on an MI355X)", "",
             "excitation, worst over the five utterances of a run; the gate is e_gpu <= 4 e_oracle + 64 u of the peak",
             "%-22s %-42s %10s %10s %8s" % ("shape", "family", "e_gpu", "e_oracle", "/ gate")]
    head, rows, kernels = None, {}, {}
    for line in Path(stdout_log).read_text().splitlines():
        m = re.match(r"\.*(\S+)\s+\(\s*\d+,\s*\d+\)\s+bs, nblk \(\d+, \d+\)\s+family (.*?)\s+via", line)
        if m:
            head = (m.group(1), m.group(2))
            rows.setdefault(head, [0.0, 0.0, 0.0])
            continue
        m = re.match(r"\s+\S+\s+e_gpu (\S+)\s+e_oracle (\S+) of the peak", line)
        if m and head:
            g, o = float(m.group(1)), float(m.group(2))
            w = rows[head]
            w[0], w[1], w[2] = max(w[0], g), max(w[1], o), max(w[2], g / (4 * o + 64 * R.U))
            continue
        m = re.match(r"\.*(\S+)\s+(default|wave|triple|serial|fast_invariant|chunk8|redo)\s+(k_vocoder\S*( delay lines in LDS>)?)", line)
        if m:
            kernels.setdefault((m.group(2), m.group(3)), []).append(m.group(1))
    for (shape, fam), w in rows.items():
        lines.append("%-22s %-42s %10.2e %10.2e %8.3f" % (shape, fam, w[0], w[1], w[2]))
    if pcm_log:
        lines += ["", "PCM, worst per schedule; gates: rel RMS %g, frame error %g (tests/helpers.py PCM_TOL, LOCAL_TOL)" % (PCM_TOL, LOCAL_TOL),
                  "%-28s %-12s %12s %12s %12s" % ("schedule", "filter", "comparisons", "rel RMS", "frame error")]
    worst = {}
    for line in (Path(pcm_log).read_text().splitlines() if pcm_log else []):
        r = json.loads(line)
        if "test_gpu_vocoder_tv" not in r["test"]:
            continue
        key = ("ragged batch" if "ragged" in r["test"] else "voc= (two betas)" if "beta_per" in r["test"]
               else "nlpf 0 (vocoder level)" if "vocoder_level" in r["test"] else r["what"].rsplit("'", 2)[-2])
        fam = "MGLSA" if re.search(r"'g\d+_", r["what"]) else "Stage::Zero"
        w = worst.setdefault((key, fam), [0, 0.0, 0.0])
        w[0], w[1], w[2] = w[0] + 1, max(w[1], r["rel_rms"]), max(w[2], r["frame_err"])
    for (key, fam), w in worst.items():
        lines.append("%-28s %-12s %12d %12.2e %12.2e" % (key, fam, w[0], w[1], w[2]))
    lines += ["", "vocoder kernels seen per schedule: " + "; ".join("%s %s x%d" % (s, k, len(v)) for (s, k), v in sorted(kernels.items()))]
    return lines


def main(path, gpu_stdout=None, pcm_log=None):
    assert R.wide_enough()
    t0 = time.time()
    lines = ["The time-varying vocoder path against its extended-precision reference: measured values",
             "(python -m tests.tools.vocoder_tv_study writes this file; tests/test_vocoder_tv_ref.py holds the gates)", "",
             "u = 2^-53.  The reference with ONE repeated row (and the two ramp shapes) against the transfer-function reference",
             "(tests/mlsa_ref.py expected_pcm), max |difference| / (u * peak); asserted under %g u:" % T.AGREE_U,
             "%-34s %9s" % ("case", "agree / u")] + agreement()
    err = table_errors()
    m = T.margins()
    lines += ["", "the oracle against the reference.  excitation: max |error| / peak; PCM: max |error| / (u * peak).",
              "margin: the smallest |counter - period| over the case's pulse decisions, in samples (asserted >= %g)" % T.MARGIN,
              "%-32s %-10s %12s %12s" % ("case", "class", "err", "margin")]
    for k, (c, e, r) in err.items():
        lines.append("%-32s %-10s %12.4g %12.3g" % (k, c, e, m[k]))
    lines += ["", "%-12s %14s %14s %14s" % ("class", "worst", "worst held", "gate (8 x)")]
    for c in ("exc", "zero", "zero_beta", "mglsa"):
        w = max(e for cc, e, _ in err.values() if cc == c)
        lines.append("%-12s %14.4g %14.4g %14.4g%s" % (c, w, T.WORST[c], T.GATE[c], "  of the peak" if c == "exc" else "  u x peak"))
    lines += ["", "mutations of oracle/jbo_hot.c (scratch copies), over the same table: cases over their gate, and the largest",
              "err / gate (the factor by which the mutation misses its gate; below 1: not seen)",
              "%-68s %12s %12s  %s" % ("mutation", "cases over", "max err/gate", "classes over")]
    for name, edits in MUTATIONS:
        with tempfile.TemporaryDirectory() as tmp:
            O.use_library(build_mutant(edits, tmp))
            try:
                e = table_errors()
            finally:
                O.use_library(None)
        over = [k for k, v in e.items() if v[2] > 1]
        lines.append("%-68s %5d of %3d %12.3g  %s" % (name, len(over), len(e), max(v[2] for v in e.values()),
                                                       ", ".join(sorted({e[k][0] for k in over})) or "-"))
    lines += ["", "%.1f s" % (time.time() - t0)]
    if gpu_stdout:
        lines += gpu_section(gpu_stdout, pcm_log)
    Path(path).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "r26_vocoder_tv.txt"), *sys.argv[2:4])

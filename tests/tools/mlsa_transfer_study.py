"""Measures what the gates of tests/test_mlsa_transfer.py are set from, and what they catch:

  * the CPU oracle against the transfer-function reference (tests/mlsa_ref.py) on every case of tests/mlsa_cases.py,
    in units of u * peak, with the reference's own aliasing margins;
  * the oracle's b2en and the b_0 shift of its post-filter against the energy integral;
  * five mutations of the oracle's filter code, each built from a SCRATCH COPY of oracle/ in a temporary directory
    (the tree is not touched) and run over the same table.

    python -m tests.tools.mlsa_transfer_study [report file, default profiles/r20_mlsa_transfer.txt] [PCM log]

No GPU.  PCM log: the JB_PCM_LOG file of a run of tests/test_gpu_mlsa_transfer.py on a GPU (tests/helpers.py
assert_pcm_close writes one line per comparison); its worst values per schedule are appended to the report."""
import json
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
from tests import test_mlsa_transfer as T

ROOT = Path(__file__).resolve().parents[2]

# (name, [(old text, new text)]) on oracle/jbo_hot.c; every old text must occur
MUTATIONS = [
    ("PPADE[3]: last significant digit, 0.01369984 -> 0.01369985",
     [("0.01369984000", "0.01369985000")]),
    ("the (i & 1) sign rule flipped in df1 and df2",
     [("*x += (i & 1) ? v : -v;", "*x += (i & 1) ? -v : v;")]),
    ("the FIR remainder loop one tap short",
     [("for (size_t k = nch * 4; k < m; k++, c++, dd++) {", "for (size_t k = nch * 4; k + 1 < m; k++, c++, dd++) {")]),
    ("MGLSA all-pass step: ds[i - 1] read before its update",
     [("        double y = ds[0] * c[1];\n", "        double y = ds[0] * c[1], before = ds[0];\n"),
      ("            ds[i] += alpha * (ds[i + 1] - ds[i - 1]);\n",
       "            const double keep = ds[i];\n            ds[i] += alpha * (ds[i + 1] - before);\n"
       "            before = keep;\n")]),
    ("the interpolation one sample ahead (i + 1)",
     [("            if (x != 0.0)\n                x *= exp(c[0]);\n",
       "            for (size_t k = 0; k < nmcp; k++)\n                c[k] += cinc[k];\n"
       "            if (x != 0.0)\n                x *= exp(c[0]);\n"),
      ("            df2(&f, &x, alpha, c, nmcp);\n            for (size_t k = 0; k < nmcp; k++)\n"
       "                c[k] += cinc[k];\n", "            df2(&f, &x, alpha, c, nmcp);\n")]),
]


def table_errors():
    """{case name: worst of nlpf 0 / 1, in u * peak} with the oracle library that is bound now."""
    out = {}
    for case in C.all_cases():
        with np.errstate(all="ignore"):
            e = [C.err_in_u(C.oracle_pcm(case, nlpf), C.expected_pcm(case, nlpf)) for nlpf in (0, 1)]
        out[case.name] = max(x if np.isfinite(x) else float("inf") for x in e)
    return out


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


def gpu_section(log):
    """Worst rel RMS and worst frame error per schedule, from the comparisons a GPU run of the table logged."""
    worst = {}
    for line in Path(log).read_text().splitlines():
        r = json.loads(line)
        if "test_gpu_mlsa_transfer" not in r["test"]:
            continue
        what = r["what"]
        key = "nlpf 0 (jb_vocoder_synthesize_batch)" if "nlpf 0" in what else "ragged batch" if "ragged" in r["test"] \
            else what.rsplit("'", 2)[-2]
        fam = "MGLSA" if "mglsa" in what else "Stage::Zero"
        w = worst.setdefault((key, fam), [0, 0.0, 0.0])
        w[0], w[1], w[2] = w[0] + 1, max(w[1], r["rel_rms"]), max(w[2], r["frame_err"])
    tol = "gates: rel RMS %g, frame error %g (tests/helpers.py PCM_TOL, LOCAL_TOL)"
    from tests.helpers import LOCAL_TOL, PCM_TOL
    lines = ["", "GPU against the same reference (tests/test_gpu_mlsa_transfer.py on an MI355X), worst per schedule; "
             + tol % (PCM_TOL, LOCAL_TOL), "%-38s %-12s %12s %12s %12s" % ("schedule", "filter", "comparisons", "rel RMS", "frame error")]
    for (key, fam), w in worst.items():
        lines.append("%-38s %-12s %12d %12.2e %12.2e" % (key, fam, w[0], w[1], w[2]))
    return lines


def main(path, pcm_log=None):
    assert R.wide_enough()
    t0 = time.time()
    lines = ["MLSA / MGLSA synthesis filters against their transfer functions: measured values",
             "(python -m tests.tools.mlsa_transfer_study writes this file; tests/test_mlsa_transfer.py holds the gates)", "",
             "u = 2^-53.  err / u: max |oracle - reference| / (u * max |reference|) over the case's samples, the worse of",
             "nlpf = 0 and nlpf = 1.  N: the grid the impulse response was taken on; agree: |h_N - h_2N| / peak over the first",
             "N samples; tail: max |h_2N| behind N, over the peak (both gated at %g)." % R.ALIAS_TOL, "",
             "%-34s %7s %7s %9s %9s %9s" % ("case", "samples", "N", "agree", "tail", "err / u")]
    err = table_errors()
    for case in C.all_cases():
        m = C.response(case)[2]
        lines.append("%-34s %7d %7d %9.1e %9.1e %9.2f" % (case.name, case.samples, m["N"], m["agree"], m["tail"], err[case.name]))
    zero = max(v for k, v in err.items() if not k.startswith("mglsa"))
    mg = max(v for k, v in err.items() if k.startswith("mglsa"))
    lines += ["", "worst, Stage::Zero: %.2f u (gate %g u = 8 x); worst, MGLSA: %.2f u (gate %g u)"
              % (zero, T.GATE_ZERO_U, mg, T.GATE_MGLSA_U), "",
              "post-filter energy (X1): O.b2en against the integral, relative, in u; the b_0 shift of O.postfilter_mcp",
              "(beta %.1f) against ln(e1 / e2) / 2 of the integral, absolute, in u; grid: |E_M - E_2M| / E" % T.PF_BETA,
              "%-6s %-6s %10s %12s %12s" % ("nmcp", "alpha", "grid", "b2en / u", "shift / u")]
    for nmcp, alpha in T.PF_SHAPES + T.PF_TRUNCATED:
        g, e, s = T.postfilter_errors(nmcp, alpha)
        lines.append("%-6d %-6g %10.1e %12.4g %12.4g%s" % (nmcp, alpha, g, e, s,
                                                       "" if (nmcp, alpha) in T.PF_SHAPES else "   (576-term truncation: not gated)"))
    lines += ["gates: b2en %g u, shift %g u" % (T.GATE_B2EN_U, T.GATE_SHIFT_U), "",
              "mutations of oracle/jbo_hot.c (scratch copies), over the same table: cases over their gate, the smallest",
              "err / gate among those, and the largest", "%-64s %12s %12s %12s" % ("mutation", "cases over", "min over", "max")]
    for name, edits in MUTATIONS:
        with tempfile.TemporaryDirectory() as tmp:
            O.use_library(build_mutant(edits, tmp))
            try:
                e = table_errors()
            finally:
                O.use_library(None)
        ratio = {k: v / (T.GATE_MGLSA_U if k.startswith("mglsa") else T.GATE_ZERO_U) for k, v in e.items()}
        over = [r for r in ratio.values() if r > 1]
        lines.append("%-64s %6d of %2d %12.3g %12.3g" % (name, len(over), len(ratio), min(over) if over else 0.0, max(ratio.values())))
    lines.append("")
    lines.append("%.1f s" % (time.time() - t0))
    if pcm_log:
        lines += gpu_section(pcm_log)
    Path(path).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ROOT / "profiles" / "r20_mlsa_transfer.txt", sys.argv[2] if len(sys.argv) > 2 else None)

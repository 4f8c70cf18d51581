"""Measures what the accuracy gate of tests/test_resample_plan.py sees, per case of tests/resample_ref.py: the path
jb_resample_geometry reports, the lengths the device tests run, and the error of the rule with real FMAs
(tests/plan/resample_probe.cpp) and of a sequential float64 sum, both against the header's formula in long double.

    python -m tests.tools.resample_paths_study [report file, default profiles/r28_resample_paths.txt]

No GPU: the device is held to the probe bit for bit (tests/test_gpu_resample_paths.py), so the probe's error is the
device's."""
import sys
import tempfile
from pathlib import Path

import jbonsai_amd as J
from tests import resample_ref as R

ROOT = Path(__file__).resolve().parents[2]


def main():
    report = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "r28_resample_paths.txt"
    assert R.have_long_double()
    lines = ["== k_resample's paths (jb_resample_geometry) and the rule's error: e = max_k |y - y_ld| / max_k |y_ld|, "
             f"ratio = e(FMA chain) / e(sequential float64 sum), gate {R.GATE:g} ==",
             "   signal: Gaussian, sigma 3000, min(rows, 64) + 1 rows; y_ld: the header's formula and the sum in long "
             "double", ""]
    ratios = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_probe(tmp)
        for c in R.CASES:
            g = J.resample_geometry(c.in_hz, c.out_hz)
            R.check_class(g, c)
            ns = R.lengths(g.L, g.M, g.ntaps, g.rows)
            n = (min(g.rows, 64) + 1) * g.M
            x, = R.signals(c, [n])
            y, = R.run_probe(exe, c.in_hz, c.out_hz, [x], tmp)
            y_ld = R.polyphase_ld(x, c.in_hz, c.out_hz)
            e, e64 = R.err(y, y_ld), R.err(R.polyphase_seq64(x, c.in_hz, c.out_hz), y_ld)
            ratios.append(e / e64)
            lines.append(f"  {c.in_hz:>5} -> {c.out_hz:<5}  L/M {g.L}/{g.M}, ntaps {g.ntaps}: {c.path}, rows {g.rows} "
                         f"(fit {g.fit} of cap {g.cap}), pad {g.pad}, LDS {g.lds_bytes} B; {len(ns)} lengths up to "
                         f"{max(ns)} samples, n_out mod L in {sorted(R.rests(ns[4:], g.L, g.M))}")
            lines.append(f"{'':17}e {e:.3e}  e_seq64 {e64:.3e}  ratio {e / e64:.2f}")
    lines += ["", f"  {len(ratios)} cases, ratios {min(ratios):.2f} .. {max(ratios):.2f}"]
    report.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

"""The tables of the coefficient tests (tests/test_coef_ref.py without a GPU, tests/test_gpu_coef_ref.py with one; the
reference is tests/coef_ref.py).

A CLASS is what one coefficient kernel is configured for and holds 16 rows; a row is one frame, so one utterance of 16
frames carries the class and the kernels see it in one batch with its prefixes of 5, 1 and 0 frames.

Post-filter class: (nmcp, alpha) under two betas.  The orders walk the kernel's lane edges (lane < nm, lane < nm - 1: 3,
4, 63, 64), nitech's 35, and alpha = 0 (mc2b the identity, the all-pass a delay) and a negative alpha; every beta of
{1e-6, 0.1, 0.3, 1.0} occurs at an order <= 7 and at one >= 35.  Rows (PF_KINDS): decaying random cepstra with c0 in
+-8; the all-zero row; c[2] alone; c[nmcp-1] alone; c0 = +-20; strong rows, whose response is still alive at the 576th
sample where b2en cuts it (asserted for (64, 0.77)).

Stage class: (n, stage, use_log_gain, alpha, beta): both parities of n (lsp2lpc's two branches), the post-filter on and
off, one to nine stages.  Rows (STAGE_KINDS): the jittered even grid of tests/test_gpu_stage.py; wide jitter with one
pair closer than the minimum distance 0.25 pi / n; lsp[1] below the minimum; lsp[last] above pi - minimum; three
frequencies bunched within half the minimum (several passes of check_lsp_stability); six (its four passes do not
finish).  The gain slot stays below the first frequency (the reference's lsp2lpc reads it as one).

The oracle's worst error, the e_oracle of the gate, is taken per GATE GROUP of a class (pf_group): the c0 = +-20 rows
apart from the rest.  freqt is fed in ascending order, so c0 is not a gain there: it multiplies the highest power of the
all-pass and reaches all 576 terms, and at c0 = +20 the f64 shift is 1e-13 to 1e-10 off where the other rows are 1e-16
to 3e-15 off.  One group for all would let a 1e-10 row excuse every other row of its class.

What the builders assert (f64 and the reference must take the same branches, and the energies must be numbers):
every comparison of check_lsp_stability and en1 != en2 at least TIE_MARGIN clear of a tie in the reference, d1^2 + d2^2
never zero, e1 and e2 in [1e-200, 1e200], the oracle's vocoder output of every utterance finite (else the next seed, as
tests/test_gpu_stage.py stable_utterance does).  One kind of tie cannot be avoided and is let through (TIE_EXACT): a pass
that has spread a pair to exactly the minimum, or clamped an end to its bound, is followed by a pass that compares the
same two numbers again, at a margin of rounding; whichever way such a comparison goes, it moves a frequency by half that
margin at most.  35 is the highest gated order: the f64 conversion loses 1e-9 there and everything at 64
(tests/test_coef_ref.py records the boundary)."""
from __future__ import annotations

import functools
import zlib

import numpy as np

from tests import coef_ref as R

FS, FPERIOD = 16000, 16
FRAMES = (16, 5, 1, 0)  # the ragged batch of a class
ROWS = 16
TIE_MARGIN = 1e-9
TIE_EXACT = 1e-15  # a comparison that repeats an assignment of the pass before (module docstring)

# name: (nmcp, alpha, (beta, beta))
PF_CLASSES = {
    "n3_a55": (3, 0.55, (1e-6, 0.3)),
    "n4_a0": (4, 0.0, (0.1, 1.0)),
    "n7_a42": (7, 0.42, (0.3, 1.0)),
    "n9_am30": (9, -0.3, (0.3, 1.0)),
    "n25_a42": (25, 0.42, (0.1, 0.3)),
    "n35_a55": (35, 0.55, (0.1, 0.3)),
    "n35_a0": (35, 0.0, (1e-6, 1.0)),
    "n63_a55": (63, 0.55, (0.1, 0.3)),
    "n64_a55": (64, 0.55, (1e-6, 0.3)),
    "n64_a77": (64, 0.77, (0.1, 1.0)),
}
PF_TABLE = [(name, beta) for name, (_, _, betas) in PF_CLASSES.items() for beta in betas]
PF_KINDS = ["random"] * 8 + ["zero", "c2", "clast", "c0_plus_20", "c0_minus_20"] + ["strong"] * 3
STRONG_SCALE = {"n64_a77": 0.2}  # (64, 0.77) rings long as it is; the others: 0.6
ZERO_ROW = PF_KINDS.index("zero")

# name: (n, stage, use_log_gain, alpha, beta)
STAGE_CLASSES = {
    "n3_s1": (3, 1, False, 0.55, 0.5),
    "n4_s4_log": (4, 4, True, 0.0, 0.3),
    "n9_s1": (9, 1, False, 0.42, 0.0),
    "n12_s2_log": (12, 2, True, 0.42, 0.2),
    "n13_s2_log": (13, 2, True, 0.55, 0.0),
    "n34_s2_log": (34, 2, True, 0.55, 0.3),
    "n35_s2": (35, 2, False, 0.55, 0.3),
    "n35_s4_log": (35, 4, True, 0.55, 0.0),
    "n35_s9": (35, 9, False, 0.55, 0.0),  # the generic filter kernel above eight stages
}
STAGE_KINDS = ["grid"] * 4 + ["wide"] * 4 + ["low"] * 2 + ["high"] * 2 + ["three"] * 2 + ["six"] * 2
# one batch with per-utterance alpha and beta: the class's own alpha and another one, beta 0 and 0.3
STAGE_MIXED = ("n12_s2_log", "n35_s2")
OTHER_ALPHA = 0.35

# the mixed-condition batch of the post-filter: (alpha, beta), interleaved over the utterances
MIXED_NMCP, MIXED_ROWS, MIXED_MIN_FRAMES = 7, 32, 8192
MIXED_CONDS = ((0.55, 0.3), (0.42, 0.0), (0.55, 0.0), (0.42, 1.0), (0.0, 0.5))
MIXED_T = (1, 2, 7, 33)
MIXED_KINDS = ["random"] * 20 + ["zero", "c2", "clast", "c0_plus_20", "c0_minus_20"] + ["strong"] * 7


def _rng(name, k=0):
    return np.random.default_rng(zlib.crc32(name.encode()) + k)


def _readonly(a):
    a.setflags(write=False)
    return a


def mc2b_f64(c, alpha):
    """cepstrum.rs:139-149 in f64, the vocoder's own step behind the post-filter (and all of it where beta = 0)."""
    b = np.array(c, dtype=np.float64, copy=True)
    if alpha != 0.0:
        for i in range(len(b) - 2, -1, -1):
            b[i] = c[i] - alpha * b[i + 1]
    return b


# ---- post-filter ---------------------------------------------------------------------------------------------------
def _cepstrum(rng, nmcp, scale, c0=None):
    c = rng.standard_normal(nmcp) * scale / np.sqrt(1.0 + np.arange(nmcp))
    c[0] = rng.uniform(-8.0, 8.0) if c0 is None else c0
    return c


def _pf_rows(name, nmcp, rows=ROWS, kinds=PF_KINDS):
    rng = _rng(name)
    out = np.zeros((rows, nmcp))
    for r in range(rows):
        kind = kinds[r % len(kinds)]
        if kind == "random":
            out[r] = _cepstrum(rng, nmcp, 0.3)
        elif kind == "c2":
            out[r, 2] = 0.7
        elif kind == "clast":
            out[r, nmcp - 1] = 0.5
        elif kind == "c0_plus_20":
            out[r] = _cepstrum(rng, nmcp, 0.3, 20.0)
        elif kind == "c0_minus_20":
            out[r] = _cepstrum(rng, nmcp, 0.3, -20.0)
        elif kind == "strong":
            out[r] = _cepstrum(rng, nmcp, STRONG_SCALE.get(name, 0.6))
    return out


@functools.lru_cache(maxsize=None)
def pf_rows(name):
    """[16][nmcp] f64, the spectrum track of the class."""
    return _readonly(_pf_rows(name, PF_CLASSES[name][0]))


def _pf_reference(rows, alpha, beta, what):
    refs = [R.postfilter(row, alpha, beta) for row in rows]
    for r, ref in enumerate(refs):
        if ref["e1"] is not None:
            assert 1e-200 <= ref["e1"] <= 1e200 and 1e-200 <= ref["e2"] <= 1e200, (what, r, ref["e1"], ref["e2"])
    return dict(b=_readonly(np.stack([x["b"] for x in refs])), plain=_readonly(np.stack([x["plain"] for x in refs])),
                shift=np.array([float(x["shift"]) for x in refs]), tail=np.array([x["tail"] for x in refs]))


@functools.lru_cache(maxsize=None)
def pf_reference(name, beta):
    """The reference of the class under `beta`, computed once per process and read-only: b [16][nmcp] long double (what
    coefficients() reports), plain (mc2b alone, what first_coefficients() reports of a frame), shift, tail [16]."""
    nmcp, alpha, _ = PF_CLASSES[name]
    ref = _pf_reference(pf_rows(name), alpha, beta, (name, beta))
    assert ref["shift"][ZERO_ROW] == 0.0 and not ref["b"][ZERO_ROW].any(), name
    if name == "n64_a77":  # the truncation at 576 samples matters: the strong rows are still ringing there
        assert all(ref["tail"][r] >= 0.05 for r, k in enumerate(PF_KINDS) if k == "strong"), ref["tail"]
    return ref


def pf_group(r, kinds=PF_KINDS):
    """The gate group of row r: the oracle's worst error is taken over the rows of the class in the same group."""
    return "c0_20" if kinds[r % len(kinds)].startswith("c0_") else "ordinary"


def _group_worst(got, ref, kinds):
    worst = {}
    for r, (g, x) in enumerate(zip(got, ref)):
        e = R.pf_errors(g, x)
        w = worst.setdefault(pf_group(r, kinds), [0.0, 0.0])
        w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])
    return worst


@functools.lru_cache(maxsize=None)
def pf_oracle(name, beta):
    """The CPU oracle on the class: (coefficients [16][nmcp] f64, {group: [worst error of b'[0], worst error of
    b'[1:]]})."""
    from oracle import oracle as O

    nmcp, alpha, _ = PF_CLASSES[name]
    got = np.stack([mc2b_f64(O.postfilter_mcp(row, alpha, beta), alpha) for row in pf_rows(name)])
    return _readonly(got), _group_worst(got, pf_reference(name, beta)["b"], PF_KINDS)


@functools.lru_cache(maxsize=None)
def pf_e_oracle(name):
    """The e_oracle of the class's gates: {group: [b'[0], b'[1:]]}, the worst over the class's rows under BOTH its
    betas.  A class is (nmcp, alpha); e1 of a row is the same number under either beta, and at c0 = +20, where the
    shift is 1e3 u or more off, the errors of e1 and e2 can all but cancel under one beta (n7_a42, row 11: 5e-13 at
    beta 0.3, 8e-14 at 1.0) -- one beta's two rows alone would be the lucky figure the gate must not lean on."""
    worst = {}
    for beta in PF_CLASSES[name][2]:
        for group, w in pf_oracle(name, beta)[1].items():
            v = worst.setdefault(group, [0.0, 0.0])
            v[0], v[1] = max(v[0], w[0]), max(v[1], w[1])
    return worst


@functools.lru_cache(maxsize=None)
def mixed_rows():
    """[32][7] f64: the distinct frames of the mixed-condition batch."""
    rows = _pf_rows("mixed", MIXED_NMCP, rows=MIXED_ROWS, kinds=MIXED_KINDS)
    assert len({row.tobytes() for row in rows}) == MIXED_ROWS
    return _readonly(rows)


@functools.lru_cache(maxsize=None)
def mixed_plan():
    """[(T, condition index, row index of each frame)] of the mixed-condition batch: T cycles over 1, 2, 7, 33 and the
    conditions over MIXED_CONDS, with an empty utterance first, in the middle and last; MIXED_MIN_FRAMES frames at
    least, more than one round of the post-filter's persistent grid."""
    plan, frames, k = [], 0, 0
    while frames < MIXED_MIN_FRAMES:
        T = MIXED_T[k % len(MIXED_T)]
        plan.append((T, (k // 3 + k) % len(MIXED_CONDS), (5 * k + np.arange(T)) % MIXED_ROWS))
        frames += T
        k += 1
    empty = lambda c: (0, c, np.zeros(0, dtype=np.int64))
    plan = [empty(0)] + plan[:len(plan) // 2] + [empty(3), empty(1)] + plan[len(plan) // 2:] + [empty(4)]
    for c in range(len(MIXED_CONDS)):  # every condition under every length
        assert {T for T, ci, _ in plan if ci == c} >= set(MIXED_T), c
    return plan


@functools.lru_cache(maxsize=None)
def mixed_reference(cond):
    """The 32 rows under condition `cond`: (reference b [32][7] long double, the oracle's worst errors per group as
    pf_oracle)."""
    from oracle import oracle as O

    alpha, beta = MIXED_CONDS[cond]
    ref = _pf_reference(mixed_rows(), alpha, beta, ("mixed", cond))["b"]
    got = np.stack([mc2b_f64(O.postfilter_mcp(row, alpha, beta), alpha) for row in mixed_rows()])
    return ref, _group_worst(got, ref, MIXED_KINDS)


# ---- Stage::NonZero ------------------------------------------------------------------------------------------------
def _lsp_row(rng, n, kind):
    h = np.pi / n
    mn = 0.25 * h
    jit = 0.45 if kind == "wide" else 0.2
    w = np.sort(h * (np.arange(1, n) + rng.uniform(-jit, jit, n - 1)))
    if kind == "wide":  # one pair for certain under the minimum distance
        j = int(rng.integers(0, n - 2))
        w[j + 1] = w[j] + rng.uniform(0.2, 0.8) * mn
        w = np.sort(w)
    elif kind == "low":
        w[0] = rng.uniform(0.1, 0.6) * mn
    elif kind == "high":
        w[-1] = np.pi - rng.uniform(0.1, 0.6) * mn
    elif kind in ("three", "six"):
        k = min(3 if kind == "three" else 6, n - 1)
        s = int(rng.integers(0, n - k))
        w[s:s + k] = np.sort(h * (s + (k + 1) / 2.0) + rng.uniform(-0.25, 0.25, k) * mn)
    assert (np.diff(w) > 0).all() and w[0] > 0 and w[-1] < np.pi, (n, kind)
    gain = min(rng.uniform(0.02, 0.08), rng.uniform(0.3, 0.7) * w[0])
    return np.concatenate(([gain], w))


def stage_utterance_rows(rows):
    """The row indices of each utterance of a stage class's batch: the ragged four, then every other row alone, so that
    first_coefficients() (the conversion without post-filter and stability check) sees all 16 rows."""
    return [np.arange(T) for T in FRAMES] + [np.arange(r, r + 1) for r in range(1, len(rows))]


def _oracle_pcm_finite(rows, n, stage, log_gain, alpha, beta):
    from oracle import oracle as O

    for idx in stage_utterance_rows(rows):
        T = len(idx)
        if T == 0:
            continue
        with np.errstate(all="ignore"):
            pcm = O.vocoder(FS, FPERIOD, alpha, 1.0, np.full(T, R.M.NODATA), rows[idx], np.ones((T, 1)), beta=beta,
                            stage=stage, use_log_gain=log_gain)
        if not np.isfinite(pcm).all():
            return False
    return True


def _stage_reference(rows, alpha, beta, log_gain, stage, what):
    """Both conversions of every row in long double with the traces, and the builder's conditions on them."""
    out = dict(filtered=[], first=[], trace=[])
    for r, row in enumerate(rows):
        c, tr = R.stage_coefficients(row, alpha, beta, log_gain, stage)
        c0, _ = R.stage_coefficients(row, alpha, beta, log_gain, stage, filtered=False)
        near = [m for *_, m in tr["cmp"] if TIE_EXACT < m < TIE_MARGIN]
        assert not near, (what, r, "a stability comparison within 1e-9 of a tie", near)
        assert tr["en"] is None or tr["en"] >= TIE_MARGIN, (what, r, "en1 within 1e-9 of en2")
        assert tr["den"] is None or tr["den"] > 0.0, (what, r, "d1^2 + d2^2 is zero")
        assert np.isfinite(np.array(c, dtype=np.float64)).all() and np.isfinite(np.array(c0, dtype=np.float64)).all()
        out["filtered"].append(R.as_ld(c))
        out["first"].append(R.as_ld(c0))
        out["trace"].append(tr)
    out["filtered"], out["first"] = _readonly(np.stack(out["filtered"])), _readonly(np.stack(out["first"]))
    return out


@functools.lru_cache(maxsize=None)
def stage_case(name):
    """(rows [16][n] f64, reference) of a stage class: reference = dict(filtered [16][n], first [16][n] long double,
    trace [16]), once per process, read-only."""
    n, stage, log_gain, alpha, beta = STAGE_CLASSES[name]
    for seed in range(10):
        rng = _rng(name, seed)
        rows = np.stack([_lsp_row(rng, n, kind) for kind in STAGE_KINDS])
        if _oracle_pcm_finite(rows, n, stage, log_gain, alpha, beta):
            break
    else:
        raise AssertionError("no table with a finite vocoder output found", name)
    ref = _stage_reference(rows, alpha, beta, log_gain, stage, name)
    # each kind of row reaches the branch it is there for
    fired = lambda r, kind, first_pass=0: any(k == kind and f and p >= first_pass for p, k, _, f, _ in ref["trace"][r]["cmp"])
    for r, kind in enumerate(STAGE_KINDS):
        if kind == "grid":
            assert ref["trace"][r]["passes"] == 1, (name, r)
        elif kind in ("wide", "three", "six"):
            assert fired(r, "gap"), (name, r, kind)
        else:
            assert fired(r, kind), (name, r, kind)
        if kind in ("three", "six") and n >= 9:
            assert fired(r, "gap", 2), (name, r, "one pass was enough")
        if kind == "six" and n >= 9:
            assert ref["trace"][r]["passes"] == 4 and ref["trace"][r]["unfinished"], (name, r, "the four passes finished")
    return _readonly(rows), ref


def stage_oracle_rows(rows, alpha, beta, log_gain, stage, filtered=True):
    from oracle import oracle as O

    return np.stack([O.stage_coefficients(row, alpha, beta, log_gain, stage, filtered=filtered) for row in rows])


@functools.lru_cache(maxsize=None)
def stage_oracle(name):
    """The CPU oracle on the class: (filtered [16][n], first [16][n], worst error filtered, worst error first), the
    errors relative in the inf-norm to the reference row."""
    n, stage, log_gain, alpha, beta = STAGE_CLASSES[name]
    rows, ref = stage_case(name)
    f = stage_oracle_rows(rows, alpha, beta, log_gain, stage)
    f0 = stage_oracle_rows(rows, alpha, beta, log_gain, stage, filtered=False)
    return (f, f0, max(R.rel_inf(g, r) for g, r in zip(f, ref["filtered"])),
            max(R.rel_inf(g, r) for g, r in zip(f0, ref["first"])))


def stage_mixed_conds(name):
    alpha = STAGE_CLASSES[name][3]
    return [(alpha, 0.0), (OTHER_ALPHA, 0.3), (alpha, 0.3), (OTHER_ALPHA, 0.0)]


@functools.lru_cache(maxsize=None)
def stage_mixed_reference(name, cond):
    """The class's rows under condition `cond` of stage_mixed_conds: (reference dict, worst oracle error filtered, worst
    oracle error first)."""
    n, stage, log_gain, _, _ = STAGE_CLASSES[name]
    alpha, beta = stage_mixed_conds(name)[cond]
    rows, _ = stage_case(name)
    assert _oracle_pcm_finite(rows, n, stage, log_gain, alpha, beta), (name, alpha, beta)
    ref = _stage_reference(rows, alpha, beta, log_gain, stage, (name, alpha, beta))
    f = stage_oracle_rows(rows, alpha, beta, log_gain, stage)
    f0 = stage_oracle_rows(rows, alpha, beta, log_gain, stage, filtered=False)
    return (ref, max(R.rel_inf(g, r) for g, r in zip(f, ref["filtered"])),
            max(R.rel_inf(g, r) for g, r in zip(f0, ref["first"])))


# ---- the report ----------------------------------------------------------------------------------------------------
def ratio(e_got, e_oracle, floor):
    """e_got against the gate's right-hand side without its factor: e_oracle + floor / 4."""
    rhs = e_oracle + floor / 4.0
    return e_got / rhs if rhs else (0.0 if e_got == 0.0 else float("inf"))

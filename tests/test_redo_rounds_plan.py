"""The rules of the vocoder's redo rounds (jbonsai_amd/csrc/jb_plan.h: redo_pick_round, redo_stage_a,
redo_second_checkpoint, redo_settle, redo_recertify) on the host, without a GPU.  A small C++ probe
(tests/plan/redo_rounds_probe.cpp) is compiled with g++ against jb_plan.cpp and drives the rules to completion in the
order Batch::finish_verify calls them; what the device would answer -- does a recomputed state meet its checkpoint, its
second checkpoint, the end state of the first pass, does a successor pass re-certification -- is a table this test
supplies, one code per (chunk, attempt).  check_rounds states what the rounds must guarantee and is held against
plans of plan_vocoder_work with random failing hand-offs and random answers; a few small cases are pinned round by
round."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.test_vocoder_plan import SAVE_CKPT, SAVE_CKPT2, SAVE_END, SAVE_WARM
from tests.test_vocoder_plan import build_probe as build_plan_probe
from tests.test_vocoder_plan import run_probe as run_plan_probe

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "jbonsai_amd" / "csrc"
FAIL_FIRST, FAIL_SECOND, FAIL_RECERT = 1, 2, 4  # bits of an outcome code (redo_rounds_probe.cpp)


def build_probe(out_dir, *extra):
    exe = Path(out_dir) / "redo_rounds_probe"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", *extra, "-I", str(CSRC),
           str(ROOT / "tests" / "plan" / "redo_rounds_probe.cpp"), str(CSRC / "jb_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("redo_rounds"))


def run_rounds(exe, items, pending, codes, ckpt2=False):
    """items: (utt, saves) per chunk; pending: the chunks whose hand-off failed; codes: [n][A] outcome codes."""
    n, A = len(items), len(codes[0])
    mask = [int(k in pending) for k in range(n)]
    text = f"{int(ckpt2)} {n} {A}\n" + " ".join(f"{u} {s}" for u, s in items) + "\n" + " ".join(map(str, mask)) + "\n"
    text += " ".join(str(c) for row in codes for c in row) + "\n"
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return json.loads(r.stdout)


def check_rounds(items, pending, codes, out, ckpt2):
    """What the rounds guarantee, from the items, the failing hand-offs and the outcomes alone."""
    n, A = len(items), len(codes[0])
    utt = [u for u, _ in items]
    has = lambda k, bit: bool(items[k][1] & bit)  # noqa: E731
    P = set(pending)
    tries, recerts = [0] * n, [0] * n
    code = lambda k, attempt, bit: bool(codes[k][min(attempt, A - 1)] & bit)  # noqa: E731
    lowest, finals, refused = 0, 0, 0
    assert len(out["rounds"]) <= n - 1
    for r in out["rounds"]:
        ids, final, full = r["ids"], set(r["final"]), set(r["full_ids"])
        spec_end, in_round = set(r["spec_end"]), set(r["ids"])
        assert ids and ids == sorted(in_round) and in_round <= P and 0 not in in_round
        # every round makes the lowest pending chunk final: the loop ends
        assert ids[0] == min(P) > lowest and ids[0] in final
        lowest = ids[0]
        for k in P:
            if k - 1 not in P:
                assert k in in_round  # behind a final chunk: never left waiting
        for k in ids:
            if k - 1 in P:  # speculative: from the first-pass end state of a chunk of this round, same utterance
                assert k - 1 in in_round and utt[k - 1] == utt[k] and has(k - 1, SAVE_END)
        # how far stage A goes, and which recomputed states are compared
        for k in ids:
            spec = not has(k, SAVE_CKPT) and has(k, SAVE_END) and k + 1 in in_round and utt[k + 1] == utt[k]
            assert (k in spec_end) == spec
        assert r["part"] == [k for k in ids if has(k, SAVE_CKPT) or k in spec_end]
        # the outcomes, as the table has them
        first_fails = {k for k in r["part"] if code(k, tries[k], FAIL_FIRST)}
        mid = [k for k in ids if ckpt2 and has(k, SAVE_CKPT) and has(k, SAVE_CKPT2) and k in first_fails]
        assert r["mid"] == mid
        unsettled = (first_fails - set(mid)) | {k for k in mid if code(k, tries[k], FAIL_SECOND)}
        assert set(r["unsettled"]) == unsettled
        # a chunk is final only if it started from a final state: its predecessor was final before the round, or
        # became final in it with a standing end state (settled at a checkpoint, or its speculative end met); one that
        # started from a state that is being replaced stays pending
        for k in ids:
            pred = k - 1
            stands = pred in final and (has(pred, SAVE_CKPT) or pred in spec_end) and pred not in unsettled
            assert (k in final) == (pred not in P or stands), (k, r)
        assert final <= in_round
        # every final chunk is counted once: settled at a checkpoint, or recomputed to its end (stage B from the
        # checkpoint it did not meet, where it has one)
        settled = {k for k in final if has(k, SAVE_CKPT) and k not in unsettled}
        assert full == final - settled and r["full_ids"] == sorted(full)
        assert r["rest"] == sorted(k for k in full if has(k, SAVE_CKPT))
        assert (r["n_partial"], r["n_full"]) == (len(settled), len(full))
        finals += len(final)
        for k in ids:
            tries[k] += 1
        P -= final
        # re-certification: the hand-offs behind chunks recomputed to their end, unless the successor is pending or
        # was recomputed in this round; a failure puts exactly that successor back
        succ = [k + 1 for k in sorted(full) if k + 1 < n and utt[k + 1] == utt[k] and has(k + 1, SAVE_WARM) and
                has(k, SAVE_END) and k + 1 not in P and k + 1 not in in_round]
        assert r["succ"] == succ
        failed = [k for k in succ if code(k, recerts[k], FAIL_RECERT)]
        for k in succ:
            recerts[k] += 1
        assert r["recert_failed"] == failed
        refused += len(failed)
        P |= set(failed)
        assert r["pending"] == sorted(P)
    assert not P, "chunks left pending"
    assert out["n_redo"] == len(pending) + refused and out["n_recert_failed"] == refused
    assert out["n_redo_partial"] + out["n_redo_full"] == finals
    assert out["n_redo_partial"] == sum(r["n_partial"] for r in out["rounds"])


def run_checked(exe, items, pending, codes, ckpt2=False):
    out = run_rounds(exe, items, pending, codes, ckpt2)
    check_rounds(items, pending, codes, out, ckpt2)
    return out


# ---- small cases, round by round -------------------------------------------------------------------------------------

E, EW, EWC, EWC2 = SAVE_END, SAVE_END | SAVE_WARM, SAVE_END | SAVE_WARM | SAVE_CKPT, 15


def one_utt(saves):
    return [(0, s) for s in saves]


def codes_of(n, **at):
    """[n][1] codes: 0 but for chunk k = code (c<k>=code)."""
    return [[at.get(f"c{k}", 0)] for k in range(n)]


def test_a_run_of_failures_whose_speculative_ends_stand_takes_one_round(probe):
    items = one_utt([E] + [EW] * 7)
    out = run_checked(probe, items, {2, 3, 4, 5, 6}, codes_of(8))
    (r,) = out["rounds"]
    assert r["ids"] == r["final"] == r["full_ids"] == [2, 3, 4, 5, 6]
    assert r["spec_end"] == r["part"] == [2, 3, 4, 5] and r["rest"] == [] and r["succ"] == [7]
    assert (out["n_redo"], out["n_redo_partial"], out["n_redo_full"], out["n_recert_failed"]) == (5, 0, 5, 0)


def test_a_speculative_end_that_is_not_met_holds_the_chunks_behind_it_back(probe):
    """Chunk 4's recomputed end state does not meet the first pass's: 5 started from a state that is being replaced, 6
    from one that 5 is yet to leave."""
    items = one_utt([E] + [EW] * 7)
    out = run_checked(probe, items, {2, 3, 4, 5, 6}, codes_of(8, c4=FAIL_FIRST))
    r1, r2 = out["rounds"]
    assert r1["ids"] == [2, 3, 4, 5, 6] and r1["final"] == r1["full_ids"] == [2, 3, 4] and r1["pending"] == [5, 6]
    assert r1["succ"] == []  # 5 is pending: its next attempt starts from 4's exact end state
    assert r2["ids"] == r2["final"] == [5, 6] and r2["spec_end"] == [5] and r2["succ"] == [7]
    assert (out["n_redo"], out["n_redo_full"]) == (5, 5)


def test_checkpoints_settle_continue_and_recertify(probe):
    """1 and 4 settle at their checkpoint, 2 does not and goes on to its end (stage B); 3, behind it, is compared again
    -- and where that fails, redone in a round of its own."""
    items = one_utt([E, EWC, EWC, EWC, EWC, EW])
    out = run_checked(probe, items, {1, 2, 4}, codes_of(6, c2=FAIL_FIRST))
    (r,) = out["rounds"]
    assert r["ids"] == r["part"] == r["final"] == [1, 2, 4] and r["spec_end"] == []
    assert r["rest"] == r["full_ids"] == [2] and r["succ"] == [3] and r["recert_failed"] == []
    assert (out["n_redo"], out["n_redo_partial"], out["n_redo_full"]) == (3, 2, 1)
    out = run_checked(probe, items, {1, 2, 4}, codes_of(6, c2=FAIL_FIRST, c3=FAIL_RECERT))
    r1, r2 = out["rounds"]
    assert r1["recert_failed"] == r1["pending"] == [3] and r2["ids"] == r2["final"] == [3] and r2["full_ids"] == []
    assert (out["n_redo"], out["n_redo_partial"], out["n_redo_full"], out["n_recert_failed"]) == (4, 3, 1, 1)


def test_an_unsettled_checkpoint_holds_the_successor_back(probe):
    items = one_utt([E, EWC, EWC, EW])
    out = run_checked(probe, items, {1, 2}, codes_of(4, c1=FAIL_FIRST))
    r1, r2 = out["rounds"]
    assert r1["ids"] == [1, 2] and r1["final"] == r1["rest"] == [1] and r1["succ"] == [] and r1["pending"] == [2]
    assert r2["ids"] == r2["final"] == [2] and r2["rest"] == []
    assert (out["n_redo_partial"], out["n_redo_full"]) == (1, 1)


def test_second_checkpoint(probe):
    """1 meets its second checkpoint, 2 neither: 1 settles (and its end state stands for 2), 2 goes on from the second."""
    items = one_utt([E, EWC2, EWC2, EW])
    out = run_checked(probe, items, {1, 2}, codes_of(4, c1=FAIL_FIRST, c2=FAIL_FIRST | FAIL_SECOND), ckpt2=True)
    (r,) = out["rounds"]
    assert r["mid"] == [1, 2] and r["unsettled"] == [2] and r["final"] == [1, 2] and r["rest"] == r["full_ids"] == [2]
    assert r["succ"] == [3] and (out["n_redo_partial"], out["n_redo_full"]) == (1, 1)
    # (a plan without second checkpoints: the bits alone do not send a chunk there)
    out = run_checked(probe, items, {1, 2}, codes_of(4, c1=FAIL_FIRST, c2=FAIL_FIRST | FAIL_SECOND), ckpt2=False)
    assert [r["mid"] for r in out["rounds"]] == [[], []] and [r["final"] for r in out["rounds"]] == [[1], [2]]


def test_no_speculation_across_utterances(probe):
    items = [(0, E), (0, EW), (0, EW), (1, E), (1, EW), (1, EW)]
    out = run_checked(probe, items, {2, 3, 4}, codes_of(6))
    r1, r2 = out["rounds"]
    assert r1["ids"] == [2] and r1["spec_end"] == [] and r1["succ"] == []  # 3 belongs to the next utterance
    assert r2["ids"] == r2["final"] == [3, 4] and r2["spec_end"] == [3]


def test_outcomes_go_by_attempt(probe):
    """The second column answers a chunk's second attempt: 3 is held back by 2's end state, then its own is met."""
    items = one_utt([E] + [EW] * 5)
    codes = [[0, 0], [0, 0], [FAIL_FIRST, 0], [FAIL_FIRST, 0], [0, 0], [0, 0]]
    out = run_checked(probe, items, {2, 3, 4}, codes)
    assert [r["ids"] for r in out["rounds"]] == [[2, 3, 4], [3, 4]]
    assert [r["final"] for r in out["rounds"]] == [[2], [3, 4]]


# ---- plans of plan_vocoder_work, random failing hand-offs, random outcomes ----------------------------------------------

# chunk length: no checkpoint (16), the tiny one (24), the short one (64), the first (96), both (144); ragged lengths,
# with single-item utterances and last chunks too short for a checkpoint
SHAPES = {C: [5 * C + 7, C + 10, 3 * C, 30, 2 * C + C // 2, 8 * C + 1] for C in (16, 24, 64, 96, 144)}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = build_plan_probe(tmp_path_factory.mktemp("redo_rounds_plans"))
    return {C: run_plan_probe(exe, T, chunk=C) for C, T in SHAPES.items()}


def test_plans_have_the_checkpoints_they_stand_for(plans):
    got = {C: (p["ckpt_frames"], p["ckpt2_frames"]) for C, p in plans.items()}
    assert got == {16: (0, 0), 24: (16, 0), 64: (24, 0), 96: (48, 0), 144: (48, 96)}
    for C, p in plans.items():
        saves = {it[4] for it in p["items"]}
        assert {0, E, EW} <= saves and (EWC in saves) == (C >= 24) and (EWC2 in saves) == (C == 144)


@pytest.mark.parametrize("C", sorted(SHAPES))
def test_random_failures_on_real_plans(probe, plans, C):
    p = plans[C]
    items = [(it[0], it[4]) for it in p["items"]]
    n, ckpt2 = len(items), p["ckpt2_frames"] != 0
    rng = np.random.default_rng(1000 + C)
    rounds = []
    for trial in range(64):
        density = (0.05, 0.3, 0.7, 1.0)[trial % 4]
        # (any chunk but 0 may be marked, the first of an utterance too: the rules must not lean on the device never
        # reporting those)
        pending = {k for k in range(1, n) if rng.random() < density}
        # each kind of comparison fails rarely, half of the time or nearly always, by attempt
        rates = rng.choice([0.05, 0.5, 0.95], size=3)
        codes = [[sum(bit for bit, q in zip((1, 2, 4), rates) if rng.random() < q) for _ in range(3)] for _ in range(n)]
        out = run_checked(probe, items, pending, codes, ckpt2)
        rounds.append(len(out["rounds"]))
    assert max(rounds) > 1  # (the cases reach held-back and re-certified chunks)


@pytest.mark.parametrize("C", sorted(SHAPES))
def test_everything_fails_everywhere(probe, plans, C):
    """Every hand-off fails, no comparison is ever met, every re-certification fails: the rounds still end, each
    chunk redone to its end."""
    p = plans[C]
    items = [(it[0], it[4]) for it in p["items"]]
    out = run_checked(probe, items, set(range(1, len(items))), [[7]] * len(items), p["ckpt2_frames"] != 0)
    assert out["n_redo_partial"] == 0 and out["n_redo_full"] == len(items) - 1

"""The join stage in the output plan (jbonsai_amd/csrc/jb_output.h: plan_output, mix_layout over join_as_mix, join_closure) on the host,
without a GPU: over every row of the routing table the slab the stage reads and writes, the programmes (`units`), the
members' starts, and the format and ADPCM geometry by programme; the numbering; the refusals; the redo closure; and,
without a request, the plan as it was.  A probe of its own (tests/plan/join_probe.cpp), built the way
tests/test_adpcm_plan.py builds its probes."""
import itertools
import json
import subprocess

import pytest

from tests import adpcm_ref
from tests import join_ref as R
from tests.test_adpcm_plan import build, run_ad
from tests.test_output_plan import ROWS, VOICE_HZ, ceil_div

N6 = [7 * 240, 0, 13 * 240, 240, 3 * 240 + 0, 2 * 240]  # native samples of six utterances (one empty)
REQ6 = [(0, 24000, 3, 240, 240), (1, 1, 0, 0, 7), (0, 0, 5, 0, 0), (1, 7, 9, 3, 0), (0, 0, 11, 5, 5), (None, 2, 4, 1, 1)]


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("join_plan")
    return build(d, "join_probe"), build(d, "adpcm_probe")


def words(req):
    out = []
    for r in req:
        r = tuple(r) + (0,) * (5 - len(r))
        out += [-1 if r[0] is None else r[0], *r[1:5]]
    return out


def call(exe, nums):
    r = subprocess.run([str(exe)], input=" ".join(map(str, nums)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def run_plan(exe, n, req=None, want=None, i16=False, loudness=False, flac=False, fmt_bytes=0, adpcm=False, align=0):
    off = [0] + list(itertools.accumulate(n))[:-1]
    p = call(exe, ["plan", VOICE_HZ, int(i16), int(loudness), int(flac), fmt_bytes, int(adpcm), align, len(n), *n, *off,
                   len(want or []), *(want or []), len(req or []), *words(req or [])])
    p["utt"] = [dict(zip(("hz", "L", "M", "n", "off"), w)) for w in p["utt"]]
    return p


def run_layout(exe, req, n, hz=None, elem=8):
    return call(exe, ["layout", elem, len(n), *words(req), *n, len(hz or []), *(hz or [])])


def run_closure(exe, req, touched, group=None):
    g = [] if group is None else [-1 if x is None else x for x in group]
    return call(exe, ["closure", len(req), *words(req), len(g), *g, *[int(t) for t in touched]])


JOIN_KEYS = ("join_src", "join", "units", "prog_of", "prog_start", "prog_first", "prog_members")


@pytest.mark.parametrize("i16,rate,loudness", sorted(ROWS))
def test_every_row_of_the_routing_table(probes, i16, rate, loudness):
    """The join reads what `final` names and writes a slab of its own in the same type; the encoders read that slab;
    units, starts, fmt and adpcm are laid out from the output plan's n by the rules they use for utterances."""
    want = [44100] * 6 if rate else None  # (odd lengths: 48 kHz -> 44.1 kHz)
    kw = dict(want=want, i16=i16, loudness=loudness, flac=i16, fmt_bytes=0 if i16 else 3, adpcm=True)
    plain = run_plan(probes[0], N6, None, **kw)
    p = run_plan(probes[0], N6, REQ6, **kw)
    slab, ty, elem = ("Join16", "i16", 2) if i16 else ("Join64", "f64", 8)
    assert p["join_src"] == p["final"] == plain["final"] and p["join"] == [slab, ty]
    n = [w["n"] for w in p["utt"]]
    if rate:
        assert n == [ceil_div(k * 147, 160) for k in N6] and any(k % 2 for k in n)
    progs, prog_of, start = R.join([[0] * k for k in n], REQ6)
    assert p["prog_of"] == prog_of == [0, 1, 0, 1, 0, 2] and p["prog_start"] == start
    assert p["prog_first"] == [0, 3, 5, 6] and p["prog_members"] == [0, 2, 4, 1, 3, 5]
    hz = 44100 if rate else VOICE_HZ
    assert [(u[0], u[1]) for u in p["units"]] == [(hz, len(x)) for x in progs]
    # programmes on 16-byte boundaries of the join slab, packed as tightly as that allows
    end = 0
    for _, k, off in p["units"]:
        assert off == ceil_div(end * elem, 16) * 16 // elem
        end = off + k
    assert p["alloc"][slab] == [ceil_div(end * elem, 16) * 16 // elem, elem]
    # the encoders take programmes: P entries, laid out from units
    assert p["flac"] == (slab if i16 else "none") and p["adpcm_src"] == [slab, ty]
    assert p["fmt_src"] == ("none" if i16 else slab) and len(p["fmt"]) == (0 if i16 else 3) and len(p["adpcm"]) == 3
    A = adpcm_ref.block_align(hz)
    at = ft = 0
    for g, (_, k, _) in enumerate(p["units"]):
        assert p["adpcm"][g] == [at, adpcm_ref.geometry(hz, k)[3], A]
        at += ceil_div(p["adpcm"][g][1], 16) * 16
        if not i16:
            assert p["fmt"][g] == [ft, 3 * k]
            ft += ceil_div(3 * k, 16) * 16
    # a join never moves an existing field: everything else is the plan without it
    for key in JOIN_KEYS + ("flac", "fmt_src", "fmt", "adpcm_src", "adpcm"):
        p.pop(key), plain.pop(key)
    assert p["alloc"].pop(slab) and slab not in plain["alloc"]
    for s in ("Fmt", "Adpcm"):
        p["alloc"].pop(s, None), plain["alloc"].pop(s, None)
    assert p == plain


@pytest.mark.parametrize("i16,rate,loudness,flac,fmt_bytes,adpcm",
                         list(itertools.product([False, True], [False, True], [False, True], [False, True], [0, 3],
                                                [False, True])))
def test_no_request_is_the_plan_as_it_was(probes, i16, rate, loudness, flac, fmt_bytes, adpcm):
    """Against the probe of the tree before the stage (tests/plan/adpcm_probe.cpp), field for field."""
    want = [22050] * 6 if rate else None
    kw = dict(want=want, i16=i16, loudness=loudness, flac=flac, fmt_bytes=fmt_bytes, adpcm=adpcm)
    before = run_ad(probes[1], N6, **kw)
    off = run_plan(probes[0], N6, None, **kw)
    assert off.pop("join_src") == ["none", "-"] and off.pop("join") == ["none", "-"]
    assert [off.pop(k) for k in JOIN_KEYS[2:]] == [[], [], [], [], []]
    assert "Join64" not in off["alloc"] and "Join16" not in off["alloc"]
    assert off == before


def test_numbering_by_first_member(probes):
    n = [10, 20, 30, 40, 50]
    req = [(4, 1), (2, 0, 1), (4,), (2,), (4,)]  # the caller's ids 4 and 2: programmes {0, 2, 4} and {1, 3}
    lay = run_layout(probes[0], req, n)
    assert lay["ok"] and lay["prog_of"] == [0, 1, 0, 1, 0]
    assert lay["start"] == [1, 0, 11, 21, 41] and [u[1] for u in lay["units"]] == [91, 61]
    assert [u[2] for u in lay["units"]] == [0, 92] and lay["total"] == 92 + 62  # f64: two samples to 16 bytes
    lay16 = run_layout(probes[0], req, n, elem=2)
    assert [u[2] for u in lay16["units"]] == [0, 96] and lay16["total"] == 96 + 64  # 16 bits: eight


@pytest.mark.parametrize("none", list(itertools.product([False, True], repeat=4)))
def test_every_none_combination(probes, none):
    n = [5, 0, 9, 2]
    req = [(None if none[u] else 1, u, 2 * u, 0, 0) for u in range(4)]
    lay = run_layout(probes[0], req, n)
    progs, prog_of, start = R.join([[0] * k for k in n], req)
    assert lay["ok"] and lay["prog_of"] == prog_of and lay["start"] == start
    assert [u[1] for u in lay["units"]] == [len(x) for x in progs]
    assert len(progs) == sum(none) + (0 if all(none) else 1)
    p = run_plan(probes[0], n, req)
    assert p["prog_of"] == prog_of and [u[1] for u in p["units"]] == [len(x) for x in progs]


def test_refusals_name_the_programme_and_the_field(probes):
    n = [10, 20, 30]
    lay = run_layout(probes[0], [(2,), (None,), (2,)], n, hz=[48000, 8000, 44100])
    assert (lay["ok"], lay["bad"], lay["field"]) == (False, 2, "output rate")
    assert run_layout(probes[0], [(2,), (None,), (2,)], n, hz=[48000, 8000, 48000])["ok"]
    assert run_layout(probes[0], [(2,), (None,), (2,)], n)["ok"]  # (rates not compared)
    lay = run_layout(probes[0], [(0,), (3,), (0,)], n)
    assert (lay["ok"], lay["bad"], lay["field"]) == (False, 3, "programme id")
    # the plan itself (which the chain feeds checked requests only) lists no join for a request that does not lay out
    p = run_plan(probes[0], n, [(0,), (3,), (0,)])
    assert p["join"] == ["none", "-"] and p["units"] == []


def test_closure(probes):
    req = [(0,), (1,), (0,), (1,), (0,), (None,)]  # programmes {0, 2, 4}, {1, 3}, {5}
    for touched, want in (([0] * 6, [0, 0, 0]), ([0, 0, 1, 0, 0, 0], [1, 0, 0]), ([0, 0, 0, 1, 0, 0], [0, 1, 0]),
                          ([0, 0, 0, 0, 0, 1], [0, 0, 1]), ([1, 1, 0, 0, 0, 1], [1, 1, 1])):
        c = run_closure(probes[0], req, touched)
        assert c["post"] == touched and c["programmes"] == want
    # through a loudness group that spans two programmes: a redo of utterance 4 changes the gain of utterance 1,
    # which the vocoder never rewrote, and with it programme 1
    group = [None, 5, None, None, 5, None]
    c = run_closure(probes[0], req, [0, 0, 0, 0, 1, 0], group)
    assert c["post"] == [0, 1, 0, 0, 1, 0] and c["programmes"] == [1, 1, 0]
    c = run_closure(probes[0], req, [1, 0, 0, 0, 0, 0], group)
    assert c["post"] == [1, 0, 0, 0, 0, 0] and c["programmes"] == [1, 0, 0]


def test_empty_batch(probes):
    p = run_plan(probes[0], [], [])
    assert p["join"] == ["none", "-"] and p["units"] == []
    lay = run_layout(probes[0], [], [])
    assert lay["ok"] and lay["units"] == [] and lay["total"] == 0


# ---- the join as the mix it means: one layout serves both (join_as_mix, then mix_layout with the starts chained) ------
def fades_of(n):
    return [0, 1, 2, n, n + 5]


def conversion_cases():
    """(name, request, lengths, elem): every row of the routing table (REQ6 over the lengths and the sample size of that
    row), the LENGTHS x PADS list tests/test_gpu_join.py joins, members of no samples, and no programme ids at all."""
    LENGTHS, PADS = R.LENGTHS, R.PADS
    cases = []
    for i16, rate, loudness in sorted(ROWS):
        n = [ceil_div(k * 147, 160) for k in N6] if rate else list(N6)
        cases.append((f"row-{int(i16)}{int(rate)}{int(loudness)}", REQ6, n, 2 if i16 else 8))
    lengths = LENGTHS + LENGTHS[::-1]
    grid = [(0, PADS[u % 4], PADS[(u // 4) % 4], fades_of(n)[u % 5], fades_of(n)[(u + 2) % 5])
            for u, n in enumerate(lengths)]
    for elem in (8, 2):
        cases.append((f"lengths-pads-{elem}", grid, lengths, elem))
        cases.append((f"lengths-pads-two-{elem}", [(u % 2,) + r[1:] for u, r in enumerate(grid)], lengths, elem))
    cases.append(("empty-members", REQ6, [0] * 6, 8))
    cases.append(("empty-members-no-pads", [(0,), (0,), (1,), (1,)], [0] * 4, 2))
    cases.append(("all-none", [(None,) + r[1:] for r in REQ6], N6, 8))
    cases.append(("all-none-grid", [(None,) + r[1:] for r in grid], lengths, 2))
    return cases


CASES = conversion_cases()


@pytest.fixture(scope="module")
def layouts(probes):
    """Each case through the probe once: the layout, the converted request and the work lists"""
    return {name: run_layout(probes[0], req, n, elem=elem) for name, req, n, elem in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_join_is_the_mix_its_conversion_names(layouts, case):
    """The converted request against the numpy statement (tests/join_ref.py): start = running end + pad_before in
    programme order, 0 dB, fades and pad_after carried over.  jb_mix_geometry of it answers what jb_join_geometry
    answers of the join, with depth at most 1 and no overlap.  (The starts of the converted request are the chained
    layout's own: the conversion has no second loop to disagree with it, so this holds the layout's starts to the numpy
    statement and everything else of the request to the join's fields.)"""
    import jbonsai_amd as J

    name, req, n, elem = case
    lay = layouts[name]
    assert lay["ok"]
    full = [tuple(r) + (0,) * (5 - len(r)) for r in req]
    progs, prog_of, start = R.join([[0] * k for k in n], req)
    conv = [tuple(c) for c in lay["converted"]]
    assert conv == [(-1 if r[0] is None else r[0], start[u], 0.0, r[2], r[3], r[4]) for u, r in enumerate(full)]
    assert lay["prog_of"] == prog_of and [u[1] for u in lay["units"]] == [len(x) for x in progs]
    as_mix = [(None if c[0] < 0 else c[0],) + c[1:] for c in conv]
    jp, js, jn = J.join_geometry(req, n)
    mp, ms, mn, depth, overlap = J.mix_geometry(as_mix, n)
    assert (mp, ms, mn) == (jp, js, jn) == (prog_of, start, [len(x) for x in progs])
    assert all(d <= 1 for d in depth) and overlap == [0] * len(progs)
    assert depth == lay["depth"] and overlap == lay["overlap"]
    assert depth == [int(any(n[u] for u in range(len(n)) if prog_of[u] == p)) for p in range(len(progs))]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_segments_of_a_join_alternate_pad_member_pad(layouts, case):
    """A programme's segments cover [0, n) without a hole; each is one member's own range or the silence between two;
    a member of no samples and a pad of none leave no segment, and never two silences in a row."""
    name, req, n, elem = case
    lay = layouts[name]
    first, segs, lists = lay["seg_first"], lay["segs"], lay["lists"]
    assert len(first) == len(lay["units"]) + 1 and first[0] == 0 and first[-1] == len(segs)
    listed = []
    for p, (_, length, _) in enumerate(lay["units"]):
        mine = segs[first[p]:first[p + 1]]
        members = [u for u in range(len(n)) if lay["prog_of"][u] == p and n[u]]
        k, want = 0, []  # the segments the members' ranges leave, in order
        for u in members:
            if lay["start"][u] > k:
                want.append((k, lay["start"][u], None))
            want.append((lay["start"][u], lay["start"][u] + n[u], u))
            k = lay["start"][u] + n[u]
        if length > k:
            want.append((k, length, None))
        got = []
        for k0, k1, l0, nl in mine:
            assert k0 < k1 and nl <= 1 and l0 + nl <= len(lists)
            got.append((k0, k1, lists[l0] if nl else None))
        assert got == want
        assert not any(a[2] is None and b[2] is None for a, b in zip(got, got[1:]))
        assert (got[0][0], got[-1][1]) == (0, length) if length else got == []
        listed += members
    assert lists == listed


def test_a_join_too_long_to_lay_out_is_refused_by_the_layout(probes):
    """What the one layout adds to the join: pads that carry a programme's length to 2^63 are a refusal naming the
    utterance, not a wrapped length"""
    lay = run_layout(probes[0], [(0, 2 ** 62, 2 ** 62), (0, 0, 0)], [10, 10])
    assert (lay["ok"], lay["bad"], lay["field"]) == (False, 0, "length")
    lay = run_layout(probes[0], [(0, 2 ** 62, 0), (0, 2 ** 62 - 20, 0)], [10, 10])
    assert (lay["ok"], lay["bad"], lay["field"]) == (False, 1, "length")
    assert run_layout(probes[0], [(0, 2 ** 62, 0), (0, 2 ** 62 - 40, 0)], [10, 10])["ok"]  # (the slab rounds up to 16 bytes)

"""Inputs of the tree-search tests (tests/test_tree_search_abi.py, tests/test_gpu_tree_search.py): voices mutated in
memory and labels that make every kind of question pattern answer both ways.

On the GENJI labels the nitech voice exercises `Contains`, `Prefix` and `?`-glob patterns only: no `Suffix`, `Exact`
or `Any` pattern, no `**` and no glob with a `*` inside answers both yes and no there.  So question definitions of
the voice are overwritten in place, byte count kept (the POSITION ranges of the container stay valid), and only
questions that stand at the ROOT of a tree are chosen: a root question is asked for every label.  Every rewritten
question holds its live patterns and fill patterns that match nothing, so each live pattern decides the question's
answer on some input:

  duration tree, root         "*e*N*" (a `*` inside), "QQQQQ" (no `*`: Exact), fill
  MCP trees 2, 3, 6, root     "?^a-*" (`?` first), "*9-23" (Suffix), fill
  LF0 trees 2..6, root        "*-19?" (`?` last), fill
  MCP tree 4, root            "**" (Any) and a fill pattern, in the bytes of one 8-byte pattern
  MCP tree 5, root            a lone "*" (Any) and a fill pattern, in the bytes of one 9-byte pattern

The voice has no one-byte pattern, so the lone `*` takes the place of a longer pattern together with a fill pattern,
quotes and comma counted.  `Any` cannot answer no; every other live pattern is checked to decide both answers.
"""
from __future__ import annotations

import re

from tests.golden.labels import BENCH_LETTER, GENJI

FILL = b"Z"  # a pattern of Z's has no `*`: Exact, and no input equals it


def glob_match(pat: bytes, s: bytes) -> bool:
    """The HTS question glob: `*` any run of bytes, `?` one byte (a restatement, not the library's code)."""
    p = i = 0
    star, mark = -1, 0
    while i < len(s):
        if p < len(pat) and (pat[p:p + 1] == b"?" or (pat[p:p + 1] != b"*" and pat[p] == s[i])):
            p, i = p + 1, i + 1
        elif p < len(pat) and pat[p:p + 1] == b"*":
            star, mark, p = p, i, p + 1
        elif star >= 0:
            mark += 1
            p, i = star + 1, mark
        else:
            return False
    return pat[p:].strip(b"*") == b""


def _section(raw: bytes, key: str):
    """(start, end) in `raw` of the DATA range `key` of the POSITION header (inclusive range -> half-open)."""
    data0 = raw.find(b"[DATA]\n") + len(b"[DATA]\n")
    lo, hi = re.search(re.escape(key.encode()) + rb":(\d+)-(\d+)", raw[:data0]).groups()
    return data0 + int(lo), data0 + int(hi) + 1


def _rewrite_question(raw: bytearray, span, name: bytes, live, split_first=None):
    """Overwrites the patterns of `QS name { ... }` inside span.  live: patterns written into the first slots of
    equal length; every other slot gets FILL.  split_first = (a, ) replaces the FIRST pattern's quoted bytes by
    `"a","ZZ.."` of the same byte count instead."""
    m = re.compile(rb"QS " + re.escape(name) + rb" \{([^}]*)\}").search(raw, span[0], span[1])
    assert m, name
    body_at = m.start(1)
    slots = [(body_at + q.start(), q.group(1)) for q in re.finditer(rb'"([^"]*)"', m.group(1))]
    live = list(live)
    for k, (at, old) in enumerate(slots):  # `at` is the opening quote
        if split_first is not None and k == 0:
            a = split_first[0]
            fill = len(old) + 2 - (len(a) + 2) - 1 - 2  # quotes of a, comma, quotes of the fill
            assert fill >= 1, (old, a)
            new = b'"' + a + b'","' + FILL * fill + b'"'
            assert len(new) == len(old) + 2
            raw[at:at + len(new)] = new
            continue
        pick = next((p for p in live if len(p) == len(old)), None)
        if pick is not None:
            live.remove(pick)
        raw[at + 1:at + 1 + len(old)] = pick if pick is not None else FILL * len(old)
    assert not live, f"no slot of the right length for {live} in {name!r}"


# (question of the root, section, live patterns) -- see the module docstring
MUTATIONS = {
    "inner_star": b"*e*N*", "exact": b"QQQQQ", "q_first": b"?^a-*", "suffix": b"*9-23", "q_last": b"*-19?",
}


def mutated_voice_bytes(raw: bytes) -> bytes:
    out = bytearray(raw)
    dur, mcp, lf0 = _section(raw, "DURATION_TREE"), _section(raw, "STREAM_TREE[MCP]"), _section(raw, "STREAM_TREE[LF0]")
    _rewrite_question(out, dur, b"C-Acc_Fw-Pos-in_Br_Acc<=7", [MUTATIONS["inner_star"], MUTATIONS["exact"]])
    _rewrite_question(out, mcp, b"C-Phone_Yuuseion", [MUTATIONS["q_first"], MUTATIONS["suffix"]])
    _rewrite_question(out, lf0, b"C-Phone_Yuuseion", [MUTATIONS["q_last"]])
    _rewrite_question(out, mcp, b"C-Hinshi_xx", [], split_first=(b"**",))
    _rewrite_question(out, mcp, b"C-Mora_diff_Acc-Type<=9", [], split_first=(b"*",))
    assert len(out) == len(raw)
    return bytes(out)


def _replace_resizing(raw: bytes, at: int, old_len: int, new: bytes) -> bytes:
    """raw with raw[at : at + old_len] (inside DATA) replaced by `new`, the POSITION ranges moved along."""
    data0 = raw.find(b"\n[DATA]\n") + len(b"\n[DATA]\n")
    pos0 = raw.find(b"[POSITION]\n")
    rel, delta = at - data0, len(new) - old_len

    def moved(m):
        lo, hi = int(m.group(1)), int(m.group(2))
        return b"%d-%d" % (lo + delta if lo > rel else lo, hi + delta if hi >= rel else hi)

    head = re.sub(rb"(\d+)-(\d+)", moved, raw[pos0:data0])
    return raw[:pos0] + head + raw[data0:at] + new + raw[at + old_len:]


# Questions larger than the kernel's fast paths (the voice as shipped has none: its largest question holds 23
# patterns and 97 bytes of text): more than 64 patterns, whose records the wave takes in chunks, and more than 256
# bytes of text, which it reads from the pool byte by byte; literals longer than a wave and a glob longer than the
# 16 bytes a lane keeps in registers.
BIG_MANY = [b"ZZ"] * 66 + [b"*e*N*", b"*9-23", b"QQ?QQ", b"*^a-*", b"?", b"*:xx-xx_x?*"]  # duration root: 72 patterns
BIG_LONG = [b"Z" * 40, b"y" * 65, b"x" * 64 + b"*", b"*" + GENJI[7][10:80].encode() + b"*",
            b"*/A:-?+1+*/B:*/C:0?_*", b"*" + b"w" * 66]                          # MCP roots: 6 patterns, ~310 bytes
BIG_LIVE = BIG_MANY[66:] + BIG_LONG[1:]  # ("QQ?QQ", "?": `?` globs without any `*`; the last: a `?` core above 8 bytes)


def big_question_voice_bytes(raw: bytes) -> bytes:
    """The sections grow, so the POSITION ranges are rewritten."""
    for key, name, pats in (("STREAM_TREE[MCP]", b"C-Phone_Yuuseion", BIG_LONG),
                            ("DURATION_TREE", b"C-Acc_Fw-Pos-in_Br_Acc<=7", BIG_MANY)):
        span = _section(raw, key)
        m = re.compile(rb"QS " + re.escape(name) + rb" \{([^}]*)\}").search(raw, span[0], span[1])
        body = b" " + b",".join(b'"' + p + b'"' for p in pats) + b" "
        raw = _replace_resizing(raw, m.start(1), len(m.group(1)), body)
    return raw


def bad_leaf_voice_bytes(raw: bytes, leaf: bytes) -> bytes:
    """`leaf` (e.g. b'"mgc_s2_101"') with its number overwritten by 9s of the same width: out of every tree's range."""
    m = re.fullmatch(rb'"(\D*(?:\d+\D+)*)(\d+)"', leaf)
    assert m and raw.count(leaf) >= 1, leaf
    new = b'"' + m.group(1) + b"9" * len(m.group(2)) + b'"'
    assert int(m.group(2)) < int(b"9" * len(m.group(2)))
    return raw.replace(leaf, new)


def edited_labels():
    """Labels that still pass the engine's shape check, edited by hand so that the mutated patterns (and the voice's own
    Suffix patterns such as `*-23`) are true for some and false for others."""
    base = [GENJI[5], GENJI[40], GENJI[300], BENCH_LETTER[3], BENCH_LETTER[10]]
    out = []
    for lab in base:
        head, tail = lab.rsplit("-", 1)
        out.append(head + "-23")          # Suffix "*-23" and "*9-23"
        out.append(head + "-39")          # Suffix "*-39"
        out.append(head + "-19")          # "*-19?" needs one more byte: no
        out.append(head + "-190")         # "*-19?": yes
        out.append("k^a-" + lab.split("-", 1)[1])   # "?^a-*": yes
        out.append("ky^a-" + lab.split("-", 1)[1])  # two bytes before "^a-": no
    return out


def bare_strings():
    """Strings for the seams only (they take any bytes; the engine's entries would refuse these as labels)."""
    return ["", "Q", "QQQQQ", "QQQQQQ", "ZZZZZ", "*", "?", "-+", "e", "eN", "Ne", "xeyNz", "a^a-", "^a-", "-19", "-199",
            "9-23", "-23", "x" * 64, "y" * 65, "y" * 64, "x" * 64 + "abc", "x" * 63 + "abc", "w" * 66, "vw" + "w" * 66,
            "w" * 65, GENJI[7][:30], GENJI[7][10:]]


def seam_inputs():
    return GENJI[:160] + BENCH_LETTER + edited_labels() + bare_strings()

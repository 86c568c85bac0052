"""The restatement of `reads` (reads_restate.py) on the data of the reference's tests/reads (golden/reads.json), and the
read-name rule of the host code (seq_names_match in mccortex_amd/bin/libmcxhost.so) against the restatement's."""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reads_restate as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "reads.json")))
K = GOLD["k"]
KEYS = S.keys_of([GOLD["genome"]], K)


def test_golden_table():
    exp = GOLD["expected"]
    for what in ("reads", "reads1", "reads2", "singles"):
        assert [int(S.touches(KEYS, K, seq)) for _, seq in GOLD[what]] == exp[what], what
        # the names carry the outcome
        assert [int("hi" in name) for name, _ in GOLD[what]] == exp[what], what
    assert exp["reads"] == [1, 0, 0, 1, 0] and exp["reads1"] == [0, 1, 0, 1, 0] and exp["reads2"] == [1, 1, 0, 0, 0]
    units = S.pair_seq2([(n, s, "") for n, s in GOLD["reads1"]], [(n, s, "") for n, s in GOLD["reads2"]])
    assert [int(any(S.touches(KEYS, K, r[1]) for r in u)) for u in units] == exp["pairs"] == [1, 1, 0, 1, 0]
    assert len(GOLD["singles"][1][1]) < K and exp["singles"] == [1, 0]


def test_touches_rules():
    g = GOLD["genome"]
    keys = S.keys_of([g], K)
    assert len(keys) == len(g) - K + 1
    rc = g[::-1].translate(str.maketrans("ACGT", "TGCA"))
    assert S.touches(keys, K, g[3:3 + K]) and S.touches(keys, K, rc[5:5 + K]) and S.touches(keys, K, g[3:3 + K].lower())
    assert not S.touches(keys, K, g[:K - 1]) and not S.touches(keys, K, "") and not S.touches(keys, K, "N" * 30)
    # a window over an N or over two reads is no k-mer
    assert not S.touches(keys, K, g[:4] + "N" + g[5:K]) and S.touches(keys, K, "NN" + g[:K] + "N")
    assert S.counts(keys, K, [g, "ACGTNACGT", g[:K].lower() + "N" + "T" * K]) == (len(g) - K + 1 + 2, len(g) - K + 1 + 1)


def test_pairing_and_formats():
    i1 = [(n, s, "") for n, s in GOLD["reads1"]]
    i2 = [(n, s, "") for n, s in GOLD["reads2"]]
    inter = [r for pair in zip(i1, i2) for r in pair] + [(n, s, "") for n, s in GOLD["singles"]]
    units = S.pair_seqi(inter)
    assert [len(u) for u in units] == [2, 2, 2, 2, 2, 1, 1]
    out, printed, total = S.filter_units(KEYS, K, units)
    assert (printed, total) == (7, 12)
    assert out[""] == "@hit\nTACCGCCAGGTCAGGGCT\n+\n..................\n"
    assert out["1"].startswith("@r1/1\nGCGAGTGGAACAGACGTTGA\n+\n....................\n@r2/1 hit    |\n")
    inv, printed_inv, _ = S.filter_units(KEYS, K, units, invert=True)
    assert printed + printed_inv == total and inv[""] == "@moo\nACA\n+\n...\n"
    assert S.fmt_read(("n c", "acgT", "IIIIII"), "fq") == "@n c\nacgT\n+\nIIII\n"
    assert S.fmt_read(("n c", "acgT", "II"), "fq") == "@n c\nacgT\n+\nII..\n"
    assert S.fmt_read(("n c", "acgT", "II"), "fa") == ">n c\nacgT\n" and S.fmt_read(("n", "acgT", ""), "plain") == "acgT\n"
    # a shorter second file ends a --seq2 task; an unmatched read of --seqi is tried against the next
    assert len(S.pair_seq2(i1, i2[:3])) == 3
    assert [len(u) for u in S.pair_seqi([("a/1", "A", ""), ("b/1", "C", ""), ("b/2", "G", ""), ("", "T", ""), ("", "T", "")])] == [1, 2, 1, 1]


NAME_CASES = [("r1/1", "r1/2", True), ("r1/2", "r1/1", True), ("r1/1", "r1/1", True), ("r1/1", "r2/2", False), ("a x", "a y", True),
              ("a/1", "a/3", False), ("", "", False), ("ab", "abc", False)]


def test_names_match_restatement():
    for a, b, exp in NAME_CASES:
        assert S.names_match(a, b) is exp, (a, b)


def test_names_match_host(mcx):
    L = C.CDLL(os.path.join(ROOT, "mccortex_amd", "bin", "libmcxhost.so"))
    L.seq_names_match.restype = C.c_bool
    L.seq_names_match.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    extra = [("r1/1 c", "r1/2\td", True), ("x1", "x2", False), ("/1", "/2", True), ("1", "2", False), ("a/2", "a/2 z", True),
             (" a", " a", False)]
    for a, b, _ in NAME_CASES + extra:
        assert L.seq_names_match(a.encode(), len(a), b.encode(), len(b)) is S.names_match(a, b), (a, b)
    for a, b, exp in NAME_CASES:
        assert L.seq_names_match(a.encode(), len(a), b.encode(), len(b)) is exp, (a, b)

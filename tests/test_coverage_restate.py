"""coverage_restate.py pinned on golden/coverage.json: the shape of the reference's tests/coverage/Makefile with fixed
sequences, and one read whose lines were worked out by hand from ctx_coverage.c and db_node.h."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import coverage_restate as V  # noqa: E402
import reads_restate as S  # noqa: E402

CASE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coverage.json")))
K = CASE["k"]


def case_graph():
    seqs = [s for _, s in CASE["seq_fa"]]
    return R.build([[], seqs, seqs * 3], K)  # Wallace: nothing; Gromit: seq.fa; Trousers: --seq seq.fa --seq2 seq.fa:seq.fa


def case_reads():
    return [tuple(r) for r in CASE["rnd_fa"] + CASE["seq_fa"]]


def test_fixture_shape():
    assert K == 5 and CASE["samples"] == ["Wallace", "Gromit", "Trousers"]
    assert all(len(s) == 50 for n, s in CASE["rnd_fa"] + CASE["seq_fa"] if n != "hand")
    g = case_graph()
    assert all(cv[0] == 0 and cv[2] == 3 * cv[1] > 0 and ed[0] == 0 and ed[1] == ed[2] for cv, ed in g.values())


def test_whole_outputs():
    g, reads = case_graph(), case_reads()
    for name, (e, d) in {"plain": (False, False), "e": (True, False), "E": (False, True), "eE": (True, True)}.items():
        assert V.command_text(g, K, 3, reads, e, d) == CASE["expected"][name], name
    plain = CASE["expected"]["plain"].split("\n")
    assert plain[0] == ">rnd" and plain[2] == ">rnd_c0_covgs" and len(plain) == 3 * (2 + 2 * 3) + 1


def test_the_read_worked_out_by_hand():
    hand = dict(map(tuple, CASE["rnd_fa"]))[CASE["by_hand"]["read"]]
    g = case_graph()
    # what the read is there for: two k-mers met in reverse orientation, an absent k-mer, an N
    occ = V.oriented_kmers(K, hand)
    assert [(p, o, key in g) for p, key, o in occ] == [(0, 1, True), (1, 1, True), (7, 0, False)] and "N" in hand
    assert g[S.kmer_int("CCGTA")] == ((0, 1, 3), [0, 0x84, 0x84]) and g[S.kmer_int("ACCGT")] == ((0, 1, 3), [0, 0x01, 0x01])
    lines = V.value_lines(g, K, 3, hand, True, True)
    want = CASE["by_hand"]["lines"]
    for c in range(3):
        assert lines[3 * c] == want["hand_c%d_edges" % c] + "\n"
        assert lines[3 * c + 1] == want["hand_c%d_degree" % c] + "\n"
        assert lines[3 * c + 2] == want["hand_c%d_covgs" % c] + "\n"
    text = CASE["expected"]["eE"]
    for name, line in want.items():
        assert ">%s\n%s\n" % (name, line) in text


def test_formatters():
    assert V.covg_line([]) == "\n" and V.edges_line([]) == "\n" and V.degree_line([]) == "\n"
    assert V.covg_line([0, 9, 10, 99, 100, 2**32 - 1]) == " 0  9 10 99 100 4294967295\n"
    # edges_to_char: "3b" is [AC] k-mer [ACT] in the source's comment -- upper nibble 0xc reversed is 3
    assert V.edges_line([0xcb, 0x12, 0x80]) == "3b 82 10\n"
    assert V.swap_nibbles(0x12) == 0x21 and V.swap_nibbles(0x80) == 0x08
    assert V.degree_line([0x00, 0x01, 0x03, 0x10, 0x11, 0x17, 0x30, 0xf1, 0xff]) == "./[\\-{]}X\n"
    assert V.values({S.kmer_int("AAAAC"): ((2**40,), [0x12])}, 5, 1, "GTTTT")[0] == [[2**32 - 1, 0, 0, 0, 0]]
    assert V.values({S.kmer_int("AAAAC"): ((7,), [0x12])}, 5, 1, "GTTTT")[1] == [[0x21, 0, 0, 0, 0]]

"""correct_restate.py on the CPU: the golden vectors (golden/correct.json: the reference's own unit-test vectors, and the
lines a restatement gives for the reference's tests/correct), one hand-built case per rule, and the random case of
correct_cases.py, which must reach every rule at least three times (test_gpu_correct.py runs it on the device)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_cases as CC  # noqa: E402
import correct_restate as X  # noqa: E402
import reads_restate as S  # noqa: E402

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "correct.json")))
K = 11
A = "ATGCATGTTGACCAAATAAGTCACTGTGGGAGCCACGTAAAGCGTTCGCACCGATTTGTG"  # the unit test's sequence: no 11-mer twice


def sub(s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]


def run(graph, seq, k=K, **kw):
    st = X.new_stats()
    view = X.View(graph, k, kw.pop("colour", 0))
    s, q = X.correct(graph, k, seq, kw.pop("qual", ""), stats=st, view=view, **kw)
    return s, q, st, view.events


def test_golden_file():
    assert GOLDEN["unit_test"]["source"] == "reference" and GOLDEN["tests_correct"]["source"] == "restatement"
    for sec in GOLDEN.values():
        k = sec["k"]
        graph = R.build([sec["graph_seqs"]], k)
        for c in sec["cases"]:
            for two_way in (False, True):
                s, q, st, _ = run(graph, c["read"], k, qual=c.get("qual", ""), two_way=two_way)
                assert s == c["corrected"], (c, two_way)
                assert len(q) == (len(s) if c.get("qual") else 0)
    # the unit test compares contigs (db_nodes_to_str): one contig per read, equal to the corrected read
    sec = GOLDEN["unit_test"]
    graph = R.build([sec["graph_seqs"]], sec["k"])
    for c in sec["cases"]:
        nodes = X.correct_nodes(X.View(graph, sec["k"]), c["read"])
        assert X.contig_str(sec["k"], [n for n, _ in nodes]) == c["corrected"]
    # the qualities of the indel reads: the read's own, '.' where a base was filled
    sec = GOLDEN["tests_correct"]
    graph = R.build([sec["graph_seqs"]], sec["k"])
    by = {c["name"]: c for c in sec["cases"]}
    assert run(graph, by["ins_T>TT"]["read"], 9, qual=by["ins_T>TT"]["qual"])[1] == "abcdefghijklmnopqrstuwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ1"
    assert run(graph, by["del_GG>G_and_extra"]["read"], 9, qual=by["del_GG>G_and_extra"]["qual"])[1] == \
        "abcdefghijklmnopqrs.uwxyzABCDEFGHIJKLMNOPQRSTUVWX...23456789ab"


def test_perfect_short_empty_and_unaligned():
    graph = R.build([[A]], K)
    s, q, st, _ = run(graph, A[5:40].lower(), qual="I" * 35)
    assert s == A[5:40] and q == "I" * 35 and st["num_perfect"] == 1 and st["gaps"] == 0 and st["end_gaps"] == 0
    for seq in (A[:K - 1], "", "N" * 20, CC.rc("TTTTTTTTTTTTTTTTTTTTTTTTTTTTT")):
        s, q, st, _ = run(graph, seq, qual="#" * len(seq))
        assert s == seq.lower() and q == "#" * len(seq) and st["num_no_kmers"] == 1 and st["bases_filled"] == 0
    assert X.fmt_read("r", "acgt", "", "ACGT", "fq", True, "!") == "@r orig=ACGT\nacgt\n+\n!!!!\n"


def test_substitution_gap_bounds_and_fq_zero():
    graph = R.build([[A]], K)
    read = sub(A[3:50], 20)
    s, q, st, _ = run(graph, read, qual="I" * len(read), fq_zero="#")
    assert s == A[3:50] and q == "I" * 20 + "#" + "I" * 26
    assert (st["gaps"], st["gaps_filled"], st["gaps_filled_backward"], st["bases_filled"]) == (1, 1, 0, 1)
    # gap_est = k + 1 = 12, wiggle = (long)(12 * D + d): D = 0.1, d = 5 gives 6
    assert X.wiggle(12, 0.1, 5) == 6 and X.wiggle(12, 0.0, 0.0) == 0 and X.wiggle(30, 0.1, 0.0) == 3 and X.wiggle(9, 0.3, 0.4) == 3
    assert X.wiggle(10, 0.1, 0.0) == 1 and X.wiggle(7, 0.7, 0.1) == 5  # float arithmetic: 4.9999995 + 0.1 rounds to 5.0 in C, too
    # an insertion of three bases: est 14 against 10 nodes seen; d = 3, D = 0 refuses it, d = 4 takes it
    ins = A[3:23] + "CCC" + A[23:50]
    assert run(graph, ins)[0] == A[3:50]
    s, _, st, _ = run(graph, ins, D=0.0, d=3.0)
    assert s != A[3:50] and st["gaps_too_short"] == 1 and st["gaps_filled"] == 0
    s, _, st, _ = run(graph, ins, D=0.0, d=4.0)
    assert s == A[3:50] and st["gaps_filled"] == 1
    # a deletion of three: est 11 against 13 nodes seen; too long for d = 1, fits d = 2
    dele = A[3:23] + A[26:50]
    s, _, st, _ = run(graph, dele, D=0.0, d=1.0)
    assert s != A[3:50] and st["gaps_too_long_or_stopped"] == 1
    s, _, st, _ = run(graph, dele, D=0.0, d=2.0)
    assert s == A[3:50] and len(s) == len(dele) + 3 and st["gaps_filled"] == 1


def test_forks_colour_and_popfwd():
    B = sub(A, 30)  # a second haplotype: a bubble
    read = sub(A[:55], 22)
    # one colour: both branches in the sample, the forward walk stops at the fork behind the error ...
    both = R.build([[A, B]], K)
    s, _, st, ev = run(both, read)
    assert st["stops_fork"] >= 1 and ev["fork_by_colour"] == 0
    # ... two colours with the sample in colour 1: the fork is resolved by colour
    two = R.build([[A, B], [A]], K)
    s, _, st, ev = run(two, read, colour=1)
    assert s == A[:55] and st["stops_fork"] == 0 and ev["fork_by_colour"] >= 1
    # a stretch only colour 0 holds: POPFWD stops the gap walk from both sides, an end extension takes it
    pop = R.build([[A], [A[:25], A[40:]]], K)
    s, _, st, ev = run(pop, A[5:55], colour=1)
    assert st["gaps"] == 1 and st["gaps_filled"] == 0 and st["stops_colour"] == 2 and s == A[5:25] + A[25:40].lower() + A[40:55]
    s, _, st, ev = run(pop, A[5:25] + "TTTTT", colour=1)
    assert s == A[5:30] and st["end_gaps_extended"] == 1 and ev["popfwd_in_extension"] == 5 and st["stops_colour"] == 0


def test_backward_only_and_two_way():
    rng = __import__("random").Random(5)
    P, X1, Y1 = CC.rseq(rng, 40), CC.rseq(rng, 40), CC.rseq(rng, 40)
    graph = R.build([[P + X1, P + Y1]], K)
    read = sub(P[10:] + X1[:30], 30)  # an error on the first base behind the branch point
    s, _, st, _ = run(graph, read)
    assert s == P[10:] + X1[:30] and st["gaps_filled_backward"] == 1 and st["stops_fork"] == 1
    # two sequences share one k-mer: both one-way walks stop at its forks, the two-way walkers meet on it
    M = CC.rseq(rng, K)
    s1, s2 = CC.rseq(rng, 40) + M + CC.rseq(rng, 40), CC.rseq(rng, 40) + M + CC.rseq(rng, 40)
    graph = R.build([[s1, s2]], K)
    read = sub(s1[10:80], 30 + K // 2)
    one, _, st1, _ = run(graph, read)
    two, _, st2, _ = run(graph, read, two_way=True)
    assert one != s1[10:80] and st1["gaps_filled"] == 0 and st1["stops_fork"] == 2
    assert two == s1[10:80] and st2["gaps_filled"] == 1


def test_repeat_missing_edge_and_absent_kmer():
    rng = __import__("random").Random(6)
    cyc = "ACG" * 20
    graph = R.build([[cyc]], K)
    junk = "TTTTTTTTTTTTTTT"
    s, _, st, _ = run(graph, cyc[:K + 6] + junk)
    # round the circle of three nodes: the node after the start is entered at steps 1 and 4, step 7 would be its third
    # entry, so six nodes are kept
    assert st["stops_repeat"] == 1 and s == cyc[:K + 6 + 6] + junk[6:].lower()
    s, _, st, _ = run(graph, junk + cyc[:K + 6])
    assert st["stops_repeat"] == 1 and s.endswith(cyc[:K + 6]) and s[:9] == junk[:9].lower() and s[9:15].isupper()
    # a cleared edge between two aligned neighbours: the read still aligns perfectly, the edge is counted
    graph = {key: (cv, list(ed)) for key, (cv, ed) in R.build([[A]], K).items()}
    occ = {p: (key, o) for p, key, o in X.V.oriented_kmers(K, A)}
    (ka, oa) = occ[20]
    graph[ka][1][0] &= ~(1 << (4 * oa + S.CODE[A[20 + K]])) & 0xff
    s, _, st, _ = run(graph, A[10:45])
    assert s == A[10:45] and st["num_perfect"] == 1 and st["missing_edges"] == 1
    # with an error elsewhere the contig ends at the missing edge; the gap beyond it is still attempted
    s, _, st, _ = run(graph, sub(A[10:58], 35))
    assert st["missing_edges"] == 1 and st["gaps"] == 1 and st["num_perfect"] == 0
    # an edge that names an absent k-mer counts as no edge
    graph = dict(R.build([[A]], K))
    del graph[occ[25][0]]
    s, _, st, ev = run(graph, A[10:50])
    assert ev["absent_edge"] >= 1 and st["gaps"] == 1 and st["gaps_filled"] == 0 and st["stops_fork"] == 0
    assert s.upper() == A[10:50]


@pytest.mark.parametrize("ncols", (1, 3))
@pytest.mark.parametrize("k", CC.KS)
def test_random_case_reaches_every_rule(k, ncols):
    stats, events = CC.check_reach(k, ncols)
    graph, colour, reads, quals, aimed = CC.case(k, ncols)
    assert 440 <= len(reads) <= 480 and len(graph) > 3000
    # the aimed reads do what they are aimed at
    nodes, _, _ = CC.expected(k, ncols)
    two, _, _ = CC.expected(k, ncols, True)
    lo, hi = aimed["shared"]
    assert sum(a != b for a, b in zip(nodes[lo:hi], two[lo:hi])) >= 3  # (at k = 11 a chance k-mer lets one through)
    lo, hi = aimed["long"]
    assert all(len(s) == 600 for s in reads[lo:hi])
    text, off, st = CC.records(k, ncols, True)
    assert len(text) == off[-1] and all((b - a) % 2 == 0 for a, b in zip(off, off[1:]))

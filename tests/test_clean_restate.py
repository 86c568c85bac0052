"""The CPU restatement of `clean` (clean_restate.py) pinned on the reference's own expectations
(tests/clean_graph/clean4/Makefile) and on hand-made graphs with the shapes the unitig walk has to stop at."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402

SEQ4 = "GCTTCTTATTTGGCATAATCCAACTTCCCTACGGAAGCCCAATAGGATTAAATTGAAGCT"


def test_clean4_population():
    # --unitigs=2 --tips=0: a k-mer seen in one sample has coverage 1 (< 2) and goes; in two samples it stays
    k = 31
    pop2 = R.build([["A"], [SEQ4]], k)
    assert len(pop2) == len(SEQ4) - k + 1
    assert R.clean(pop2, k, 2, 0)[0] == {}
    pop3 = R.build([["A"], [SEQ4], [SEQ4]], k)
    assert set(R.clean(pop3, k, 2, 0)[0]) == set(pop3)
    pop3_01 = R.build([["A"], [SEQ4]], k)  # pop3.ctx:0,1
    assert R.clean(pop3_01, k, 2, 0)[0] == {}


def test_closed_cycle():
    k = 5
    s = "ACGGTTCAGATTGC"  # no repeated 5-mer, no 5-mer equal to another's reverse complement
    g = R.build([[s + s[:k]]], k)  # the last k-mer is the first one again
    us = R.unitigs(g, k)
    assert len(us) == 1 and len(us[0]) == len(s)
    assert not R.is_tip(g, us[0])
    out, st, _, _ = R.clean(g, k, 0, 100)  # shorter than the tip length, but a cycle is no tip
    assert set(out) == set(g) and st["num_tips"] == 0


def test_hairpin_and_self_loop():
    k = 5
    # ACGCGT is its own reverse complement: ACGCG -> CGCGT = revcomp(ACGCG), so the walk turns back on itself
    g = R.build([["TTGAC" + "ACGCGT" + "CATTG"]], k)
    us = R.unitigs(g, k)
    key = R.canon(R.kmer_int("ACGCG"), k)
    (u,) = [u for u in us if any(kk == key for kk, _ in u)]
    assert u[0][0] == key or u[-1][0] == key  # the hairpin k-mer ends its unitig
    loop = R.build([["A" * 12]], k)  # AAAAA -> AAAAA
    assert [len(u) for u in R.unitigs(loop, k)] == [1]


def test_even_median_at_threshold():
    # depends on the even-length median assumption (clean_restate.py): coverages 1 and 2 give median 1
    k = 5
    g = R.build([["ACGTTG", "CGTTG"]], k)
    us = R.unitigs(g, k)
    assert len(us) == 1 and len(us[0]) == 2
    assert sorted(R.sum_covg(g, kk) for kk, _ in us[0]) == [1, 2]
    assert R.clean(g, k, 2, 0)[0] == {}
    assert len(R.clean(g, k, 1, 0)[0]) == 2


def test_edge_to_absent_kmer_is_removed():
    k = 5
    g = R.build([["ACGTTG"] * 3], k)
    key = R.canon(R.kmer_int("ACGTT"), k)
    cv, ed = g[key]
    g[key] = (cv, [ed[0] | 1 << 0])  # ACGTT -> CGTTA, which is not in the graph
    out, _, _, _ = R.clean(g, k, 0, 0)
    assert out[key][1] == ed


def test_tips_and_counters():
    # a 40-k-mer trunk with a 3-k-mer spur: the spur is a tip (indeg 1 from the trunk, outdeg 0)
    k = 7
    trunk = "GATTACAGGCTTACCGTAGGCATCCGATTGCAAGTCCTAGCATG"
    spur = trunk[:20] + "TTT"
    g = R.build([[trunk] * 3 + [spur]], k)
    out, st, before, after = R.clean(g, k, 0, 2 * k)
    assert st["num_tips"] == 1 and st["num_tip_kmers"] == 3
    assert len(out) == len(g) - 3
    assert sum(before["unitig_len"]) == sum(after["unitig_len"]) + 1

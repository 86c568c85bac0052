"""The restatement of `bubbles` (bubbles_restate.py) on the cases of bubbles_cases.py against tests/golden/bubbles.json,
on the DNA strings of the reference's own unit test (src/tests/bubble_caller_tests.c, kept in the golden file as data),
and what the case set has to reach.  The golden file was written by the restatement (tests/golden/make_bubbles_golden.py)
and then read through, not worked out by hand: at k = 11 the two calls of `snp` were checked to be the SNP seen from L
(5' flank cut to 5 k-mers, branches of 11 k-mers that differ in their first base) and from R, and the calls of `empty`
to hold a branch of no k-mer beside the inserted one; the other entries were compared with these for shape."""
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bubbles_cases as BC  # noqa: E402
import bubbles_restate as B  # noqa: E402
import clean_restate as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bubbles.json")
EVENTS = ("branch_k_kmers", "branch_empty", "call_three_branches", "branch_multi_unitig", "call_reverse_list", "fork_reverse", "fork_forward",
          "dupes_removed", "3p_first_equal", "3p_prev_equal", "popfwd", "popfrk_colfwd", "flank_cut", "flank_one")
STOPS = ("stop_limit", "stop_nocovg", "stop_nocolcovg", "stop_nolinks", "stop_repeat")


def test_cases_against_golden():
    want = json.load(open(GOLDEN))["cases"]
    assert sorted(want) == sorted(c["name"] for c in BC.cases())
    for c in BC.cases():
        _, text, stats, _ = BC.run(c)
        assert {"text": text, "stats": stats} == want[c["name"]], c["name"]


def test_reference_unit_test_strings():
    ut = json.load(open(GOLDEN))["unit_test"]
    k = ut["k"]
    for call in ut["calls"]:
        seqs = [s.upper() for s in call["seqs"]]
        graph = R.build([[s] for s in seqs], k)  # each sequence in a colour of its own
        got = B.alleles_between(graph, k, len(seqs), call["flank5p"], call["flank3p"], ut["max_allele"])
        assert sorted(got) == sorted(a.upper() for a in call["alleles"]), call
        # the same call is in the file: its flanks end and start as the test's, its branches are the alleles less k - 1 bases
        _, text, _, _ = B.call(graph, k, len(seqs), ut["max_allele"], ut["max_flank"])
        blocks = [b.split("\n") for b in text.split("\n\n") if b]
        hit = [b for b in blocks if b[1].endswith(call["flank5p"]) and call["flank3p"].endswith(b[3])]
        assert len(hit) == 1, call
        assert sorted(hit[0][5::2]) == sorted(a.upper()[k - 1:] for a in call["alleles"])
        assert hit[0][1] == call["flank5p"] and hit[0][3] == call["flank3p"][k - 1:]


def test_records_describe_the_text():
    for c in BC.cases():
        recs, text, stats, _ = BC.run(c)
        assert len(recs) == stats["bubbles"] and sum(r["num_branches"] for r in recs) == stats["branches"]
        at = 0
        for i, r in enumerate(recs):
            assert r["text_off"] == at
            block = text[at:at + r["text_len"]]
            at += r["text_len"]
            lines = block.split("\n")
            assert lines[0] == ">bubble.call%d.5pflank kmers=%d" % (i, r["flank5p_kmers"]) and len(lines[1]) == c["k"] - 1 + r["flank5p_kmers"]
            assert lines[2] == ">bubble.call%d.3pflank kmers=%d" % (i, r["flank3p_kmers"]) and len(lines[3]) == r["flank3p_kmers"]
            assert len(lines) == 4 + 2 * r["num_branches"] + 2 and lines[-2:] == ["", ""]
            assert r["flank5p_kmers"] <= c["params"]["max_flank"]
            fork = B.node_str((r["fork_key"], r["fork_orient"]), c["k"])
            assert lines[1].endswith(fork)
        assert at == len(text)


def test_case_set_reaches_every_rule():
    events, stats, per = collections.Counter(), collections.Counter(), {}
    for c in BC.cases():
        assert 3 <= c["params"]["max_allele"] <= 100 and 3 <= c["params"]["max_flank"] <= 100 and 2 <= c["ncols"] <= 4
        recs, text, st, ev = BC.run(c)
        per[c["name"]] = (recs, text, st, ev)
        events.update(ev)
        stats.update(st)
    assert all(events[e] for e in EVENTS), events
    assert all(stats[s] for s in STOPS), stats
    for k in BC.KS:
        recs, text, st, ev = per["snp_k%d" % k]
        assert st["bubbles"] == 2 and ev["branch_k_kmers"] == 4 and ev["flank_cut"] and ev["3p_first_equal"] and ev["3p_prev_equal"] and ev["dupes_removed"]
        assert len({r["fork_key"] for r in recs}) == 2  # called from both sides
        assert per["snp_limit_k%d" % k][2]["stop_limit"] == per["snp_limit_k%d" % k][2]["paths"] and not per["snp_limit_k%d" % k][2]["bubbles"]
        assert per["indel_k%d" % k][2]["bubbles"] == 2
        assert per["empty_k%d" % k][3]["branch_empty"] == 2
        assert all(r["num_branches"] == 3 for r in per["three_k%d" % k][0])
        assert per["multi_k%d" % k][3]["branch_multi_unitig"]
        assert per["haploid_k%d" % k][2]["haploid_dropped"] == 2 and per["haploid_k%d" % k][2]["bubbles"] == 0
        assert per["haploid_off_k%d" % k][2]["haploid_dropped"] == 0 and per["haploid_off_k%d" % k][2]["bubbles"] == 2
        assert per["haploid_k%d" % k][2]["stop_nolinks"]
        assert per["serial_k%d" % k][2]["serial_dropped"] == 2 and per["serial_k%d" % k][2]["bubbles"] == 4
        assert per["serial_kept_k%d" % k][2]["serial_dropped"] == 0 and per["serial_kept_k%d" % k][2]["bubbles"] == 6
        assert per["nocol_k%d" % k][2]["stop_nocolcovg"] and per["nocol_k%d" % k][3]["popfwd"]
        assert per["loop_k%d" % k][2]["stop_repeat"] == 1
        assert per["cross_k%d" % k][3]["flank_one"]


def test_wide_case_set_reaches_every_rule():
    """the cases at k = 63 .. 127 (keys of two, three and four words), which no golden pins: the conditions that the test
    above asserts per k of KS, per k of WIDE_KS, and its sums over the wide set alone.  The limits that are 100 there are
    max(100, 3 k) here; those of 3, 5 and 7 stay"""
    events, stats, per = collections.Counter(), collections.Counter(), {}
    assert [c["name"] for c in BC.wide_cases()] == ["%s_k%d" % (s[0], k) for k in BC.WIDE_KS for s in BC.SPECS]
    for c, spec in zip(BC.wide_cases(), BC.SPECS * len(BC.WIDE_KS)):
        limits = (3, 5, 7, max(100, 3 * c["k"]))
        assert c["params"]["max_allele"] in limits and c["params"]["max_flank"] in limits and 2 <= c["ncols"] <= 4
        assert (c["params"]["max_allele"] < 100) == (spec[2][0] < 100) and (c["params"]["max_flank"] < 100) == (spec[2][1] < 100)
        recs, text, st, ev = BC.run(c)
        per[c["name"]] = (recs, text, st, ev)
        events.update(ev)
        stats.update(st)
    assert all(events[e] for e in EVENTS), events
    assert all(stats[s] for s in STOPS), stats
    for k in BC.WIDE_KS:
        recs, text, st, ev = per["snp_k%d" % k]
        assert st["bubbles"] == 2 and ev["branch_k_kmers"] == 4 and ev["flank_cut"] and ev["3p_first_equal"] and ev["3p_prev_equal"] and ev["dupes_removed"]
        assert len({r["fork_key"] for r in recs}) == 2  # called from both sides
        assert per["snp_limit_k%d" % k][2]["stop_limit"] == per["snp_limit_k%d" % k][2]["paths"] and not per["snp_limit_k%d" % k][2]["bubbles"]
        assert per["indel_k%d" % k][2]["bubbles"] == 2
        assert per["empty_k%d" % k][3]["branch_empty"] == 2
        assert all(r["num_branches"] == 3 for r in per["three_k%d" % k][0])
        assert per["multi_k%d" % k][3]["branch_multi_unitig"]
        assert per["haploid_k%d" % k][2]["haploid_dropped"] == 2 and per["haploid_k%d" % k][2]["bubbles"] == 0
        assert per["haploid_off_k%d" % k][2]["haploid_dropped"] == 0 and per["haploid_off_k%d" % k][2]["bubbles"] == 2
        assert per["haploid_k%d" % k][2]["stop_nolinks"]
        assert per["serial_k%d" % k][2]["serial_dropped"] == 2 and per["serial_k%d" % k][2]["bubbles"] == 4
        assert per["serial_kept_k%d" % k][2]["serial_dropped"] == 0 and per["serial_kept_k%d" % k][2]["bubbles"] == 6
        assert per["nocol_k%d" % k][2]["stop_nocolcovg"] and per["nocol_k%d" % k][3]["popfwd"]
        assert per["loop_k%d" % k][2]["stop_repeat"] == 1
        assert per["cross_k%d" % k][3]["flank_one"]


def test_a_graph_without_a_fork_gives_nothing():
    graph = R.build([["ACGTTGCATGTCGCATGATGCATGAGAGCT"], ["ACGTTGCATGTCGCATGATGCATGAGAGCT"]], 11)
    recs, text, stats, _ = B.call(graph, 11, 2, 50, 50)
    assert recs == [] and text == "" and not any(stats.values())

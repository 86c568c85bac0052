"""The restatement of `breakpoints` (breakpoints_restate.py) on the cases of breakpoints_cases.py and on the breakpoint1
and breakpoint2 fixtures against tests/golden/breakpoints.json, what the case set has to reach, and a check of every call
that does not depend on the restatement's run logic: each `chr=` entry of a flank names a reference interval that the
flank's sequence, from the entry's offset on, spells out (what the reference's breakpoints-check-ref.pl checks).  The
golden file was written by the restatement (tests/golden/make_breakpoints_golden.py) and then read through: the calls of
the breakpoint1 fixture were compared with the events that the fixture's comment block draws."""
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breakpoints_cases as BC  # noqa: E402
import breakpoints_restate as B  # noqa: E402
import clean_restate as R  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_breakpoints_golden as MG  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "breakpoints.json")
EVENTS = ("key_occurs_twice", "break_forward", "break_reverse", "two_nonref_successors", "fork_has_one_successor", "colour_lacks_successor",
          "one_of_two_runs_ends", "runs_two_chroms_one_qoffset", "sort_tie_on_chrom", "exact_run_dropped_5p", "exact_run_dropped_3p",
          "exact_run_kept_5p", "exact_run_kept_3p", "flank3pidx_below_k1", "flank3pidx_from_k1", "allele_run_minus", "colours_merged",
          "two_calls_one_break", "kept_runs_fell")
STATS = ("occurrences", "ref_keys", "ref_added", "breaks", "flank_walks", "flanks", "flanks_norun", "allele_walks", "alleles", "alleles_norun", "calls",
         "steps", "runs_started", "runs_ended", "stop_runs", "stop_maxref", "stop_flank", "stop_nocovg", "stop_nocolcovg", "stop_nolinks", "stop_repeat")


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def self_check(text, ref, names, k):
    """every run of every flank lies on the reference where it says; returns the parsed calls"""
    chrom = {n: s.upper() for n, s in zip(names, ref)}
    calls = B.parse_calls(text)
    for c in calls:
        for flank, runs in ((c["flank5p"], c["runs5"]), (c["flank3p"], c["runs3"])):
            assert runs
            for name, start, end, strand, offset in runs:
                if strand == "+":
                    assert start <= end
                    want = chrom[name][start - 1:end]
                else:
                    assert start >= end
                    want = rc(chrom[name][end - 1:start])
                assert len(want) >= 1 and offset >= 1
                assert flank[offset - 1:offset - 1 + len(want)] == want, (c["id"], name, start, end, strand, offset)
        assert len(c["flank5p"]) >= k
    return calls


def test_cases_against_golden():
    want = json.load(open(GOLDEN))["cases"]
    assert sorted(want) == sorted(c["name"] for c in BC.cases())
    for c in BC.cases():
        res = BC.run(c)
        assert MG.plain(res) == want[c["name"]], c["name"]
        assert res[2]["stop_bound"] == 0 and res[2]["reruns"] == 0


def test_case_set_reaches_every_rule():
    events, stats, per = collections.Counter(), collections.Counter(), {}
    for c in BC.cases():
        assert len(c["graph"]) <= 400 and 2 <= c["ncols"] <= 3
        res = BC.run(c)
        per[c["name"]] = res
        events.update(res[3])
        stats.update(res[2])
        assert all(res[2].get(n, 0) or res[3].get(n, 0) for n in dict((s[0], s[3]) for s in BC.SPECS)[c["name"].rsplit("_k", 1)[0]]), c["name"]
    assert all(events[e] for e in EVENTS), events
    assert all(stats[s] for s in STATS), stats
    for k in BC.KS:
        st = lambda name: per["%s_k%d" % (name, k)][2]  # noqa: E731
        ev = lambda name: per["%s_k%d" % (name, k)][3]  # noqa: E731
        for name in BC.NO_CALL:
            assert per["%s_k%d" % (name, k)][1] == "" and st(name)["calls"] == 0, name
        for name in BC.NO_BREAK:
            assert st(name)["breaks"] == 0 and st(name)["ref_added"] == 0
        for name in ("snp", "insertion", "deletion", "microhom", "junction", "ends"):
            assert st(name)["calls"] == 2 and st(name)["breaks"] == 2, name  # seen from either side
        assert ev("snp")["flank3pidx_from_k1"] == 2 and all(r["path_kmers"] == 1 for r in per["snp_k%d" % k][0])
        assert all(r["path_kmers"] == 0 for r in per["deletion_k%d" % k][0]) and ev("deletion")["flank3pidx_from_k1"] == 2
        assert ev("microhom")["flank3pidx_below_k1"] == 2 and all(r["path_kmers"] == 0 for r in per["microhom_k%d" % k][0])
        assert st("snp_maxref")["stop_maxref"] == 4
        assert st("twosnps")["stop_runs"] and st("twosnps")["calls"] == 4
        assert ev("inversion")["allele_run_minus"] and st("inversion")["calls"] == 4
        assert st("lost")["stop_flank"] and st("lost")["flanks_norun"] and st("lost")["allele_walks"] < st("lost")["flank_walks"]
        assert st("tail")["alleles_norun"] == 1 and st("loop")["stop_repeat"] == 1
        assert ev("twosucc")["two_nonref_successors"] == 2 and st("twosucc")["calls"] == 4
        assert [r["num_cols"] for r in per["merged_k%d" % k][0]] == [2, 2] and "cols=0,1\n" in per["merged_k%d" % k][1]
        assert ev("twopaths")["two_calls_one_break"] == 1
        assert ev("lacks")["colour_lacks_successor"] and "cols=0\n" in per["lacks_k%d" % k][1] and "cols=1" not in per["lacks_k%d" % k][1]
        assert st("nocol")["stop_nocolcovg"]
        assert st("refn")["ref_added"] and st("refn")["calls"] == 2
        assert ev("exact")["exact_run_kept_5p"] and ev("exact")["exact_run_kept_3p"]
        assert per["exact_k%d" % k][1] != per["exact_edges_k%d" % k][1]  # the reference's edges change the outcome
        assert ev("repeat_exact")["exact_run_dropped_5p"] and ev("repeat_exact")["exact_run_dropped_3p"]
        # a run of exactly min_ref k-mers on a cycle: held at every second step end, gone at the others, held at the end
        assert ev("cycleref")["kept_runs_fell"] and st("cycleref")["stop_repeat"] == 1 and ev("cycleref")["exact_run_kept_3p"]
        assert [r["flank3p_runs"] for r in per["cycleref_k%d" % k][0]] == [1]
        assert ev("repeat")["sort_tie_on_chrom"] and ev("repeat")["one_of_two_runs_ends"]


def test_wide_case_set_reaches_every_rule():
    """the cases at k = 63 .. 127 (keys of two, three and four words), which no golden pins: the conditions that the test
    above asserts per k of KS, per k of WIDE_KS, and its sums over the wide set alone.  The graphs grow with k (675
    k-mers at k = 127), so their bound is 800; every call is checked against the reference as for the narrow set"""
    events, stats, per = collections.Counter(), collections.Counter(), {}
    needs = dict((s[0], s[3]) for s in BC.SPECS)
    assert [c["name"] for c in BC.wide_cases()] == ["%s_k%d" % (s[0], k) for k in BC.WIDE_KS for s in BC.SPECS]
    for c in BC.wide_cases():
        assert len(c["graph"]) <= 800 and 2 <= c["ncols"] <= 3
        res = BC.run(c)
        per[c["name"]] = res
        events.update(res[3])
        stats.update(res[2])
        assert all(res[2].get(n, 0) or res[3].get(n, 0) for n in needs[c["name"].rsplit("_k", 1)[0]]), c["name"]
        assert res[2]["stop_bound"] == 0 and res[2]["reruns"] == 0
        if res[1]:
            self_check(res[1], c["ref"], c["names"], c["k"])
    assert all(events[e] for e in EVENTS), events
    assert all(stats[s] for s in STATS), stats
    for k in BC.WIDE_KS:
        st = lambda name: per["%s_k%d" % (name, k)][2]  # noqa: E731
        ev = lambda name: per["%s_k%d" % (name, k)][3]  # noqa: E731
        for name in BC.NO_CALL:
            assert per["%s_k%d" % (name, k)][1] == "" and st(name)["calls"] == 0, name
        for name in BC.NO_BREAK:
            assert st(name)["breaks"] == 0 and st(name)["ref_added"] == 0
        for name in ("snp", "insertion", "deletion", "microhom", "junction", "ends"):
            assert st(name)["calls"] == 2 and st(name)["breaks"] == 2, name  # seen from either side
        assert ev("snp")["flank3pidx_from_k1"] == 2 and all(r["path_kmers"] == 1 for r in per["snp_k%d" % k][0])
        assert all(r["path_kmers"] == 0 for r in per["deletion_k%d" % k][0]) and ev("deletion")["flank3pidx_from_k1"] == 2
        assert ev("microhom")["flank3pidx_below_k1"] == 2 and all(r["path_kmers"] == 0 for r in per["microhom_k%d" % k][0])
        assert st("snp_maxref")["stop_maxref"] == 4
        assert st("twosnps")["stop_runs"] and st("twosnps")["calls"] == 4
        assert ev("inversion")["allele_run_minus"] and st("inversion")["calls"] == 4
        assert st("lost")["stop_flank"] and st("lost")["flanks_norun"] and st("lost")["allele_walks"] < st("lost")["flank_walks"]
        assert st("tail")["alleles_norun"] == 1 and st("loop")["stop_repeat"] == 1
        assert ev("twosucc")["two_nonref_successors"] == 2 and st("twosucc")["calls"] == 4
        assert [r["num_cols"] for r in per["merged_k%d" % k][0]] == [2, 2] and "cols=0,1\n" in per["merged_k%d" % k][1]
        assert ev("twopaths")["two_calls_one_break"] == 1
        assert ev("lacks")["colour_lacks_successor"] and "cols=0\n" in per["lacks_k%d" % k][1] and "cols=1" not in per["lacks_k%d" % k][1]
        assert st("nocol")["stop_nocolcovg"]
        assert st("refn")["ref_added"] and st("refn")["calls"] == 2
        assert ev("exact")["exact_run_kept_5p"] and ev("exact")["exact_run_kept_3p"]
        assert per["exact_k%d" % k][1] != per["exact_edges_k%d" % k][1]  # the reference's edges change the outcome
        assert ev("repeat_exact")["exact_run_dropped_5p"] and ev("repeat_exact")["exact_run_dropped_3p"]
        assert ev("cycleref")["kept_runs_fell"] and st("cycleref")["stop_repeat"] == 1 and ev("cycleref")["exact_run_kept_3p"]
        assert [r["flank3p_runs"] for r in per["cycleref_k%d" % k][0]] == [1]
        assert ev("repeat")["sort_tie_on_chrom"] and ev("repeat")["one_of_two_runs_ends"]


def test_records_describe_the_text():
    for c in BC.cases():
        recs, text, stats, _, _ = BC.run(c)
        k = c["k"]
        assert len(recs) == stats["calls"]
        calls = B.parse_calls(text) if text else []
        assert len(calls) == len(recs)
        at = 0
        for i, (r, pc) in enumerate(zip(recs, calls)):
            assert r["text_off"] == at and pc["id"] == i
            at += r["text_len"]
            assert len(pc["flank5p"]) == k - 1 + r["flank5p_kmers"] and len(pc["flank3p"]) == r["flank3p_kmers"] and len(pc["path"]) == r["path_kmers"]
            assert len(pc["runs5"]) == r["flank5p_runs"] and len(pc["runs3"]) == r["flank3p_runs"] and len(pc["cols"]) == r["num_cols"]
            assert pc["flank5p"].endswith(B.node_str((r["fork_key"], r["fork_orient"]), k))
            assert (pc["path"] + pc["flank3p"])[0] == "ACGT"[r["succ_base"]]
            assert pc["cols"] == sorted(pc["cols"]) and c["ncols"] - 1 not in pc["cols"]
        assert at == len(text)


def test_every_call_lies_on_the_reference_where_it_says():
    for c in BC.cases():
        res = BC.run(c)
        if res[1]:
            self_check(res[1], c["ref"], c["names"], c["k"])


def test_breakpoint1_fixture():
    want = json.load(open(GOLDEN))["breakpoint1"]
    res = MG.fixture1()
    assert MG.plain(res) == want
    names, ref = MG.fasta("breakpoint1_ref.fa")
    calls = self_check(res[1], ref, names, 11)

    def find(pred):
        hits = [c for c in calls if pred(c)]
        assert hits
        return hits

    def one(c, which):
        return c[which][0]
    # chr4 position 25 C -> T: the flanks on chr4, same strand, either side of position 25
    fw = find(lambda c: one(c, "runs5")[0] == "chr4" and one(c, "runs5")[3] == "+" and one(c, "runs3")[0] == "chr4")
    assert any(one(c, "runs5")[2] == 24 and one(c, "runs3")[1] == 26 and one(c, "runs3")[3] == "+" and c["path"] == "T" for c in fw)
    rv = find(lambda c: one(c, "runs5")[0] == "chr4" and one(c, "runs5")[3] == "-")
    assert any(one(c, "runs5")[2] == 26 and one(c, "runs3")[1] == 24 and one(c, "runs3")[3] == "-" and c["path"] == "A" for c in rv)
    # the chr3 1-bp deletion at 21-22 (CGG -> CG): the flanks on chr3 end and start inside 21 .. 25
    d = find(lambda c: one(c, "runs5")[0] == "chr3" and one(c, "runs3")[0] == "chr3" and one(c, "runs5")[3] == one(c, "runs3")[3])
    assert any(one(c, "runs5")[3] == "+" and 21 <= one(c, "runs5")[2] <= 23 and 22 <= one(c, "runs3")[1] <= 25 for c in d)
    assert any(one(c, "runs5")[3] == "-" and 22 <= one(c, "runs5")[2] <= 25 and 21 <= one(c, "runs3")[1] <= 23 for c in d)
    # the chr1 5-bp insertion after 18 (a tandem copy of AGTGC): both flanks on chr1, overlapping by the copied bases
    ins = find(lambda c: one(c, "runs5")[0] == "chr1" and one(c, "runs3")[0] == "chr1" and one(c, "runs5")[3] == one(c, "runs3")[3])
    assert any(one(c, "runs5")[3] == "+" and 18 <= one(c, "runs5")[2] <= 24 and 19 <= one(c, "runs3")[1] <= 24 for c in ins)
    assert any(one(c, "runs5")[3] == "-" and 19 <= one(c, "runs5")[2] <= 24 and 18 <= one(c, "runs3")[1] <= 24 for c in ins)
    # contig0: the 5' flank on chr1 and chr2, the 3' flank on chr3
    assert find(lambda c: {r[0] for r in c["runs5"]} == {"chr1", "chr2"} and {r[0] for r in c["runs3"]} == {"chr3"})
    assert find(lambda c: {r[0] for r in c["runs3"]} == {"chr1", "chr2"} and {r[0] for r in c["runs5"]} == {"chr3"})


def test_sample_equal_to_reference_gives_empty_text():
    names, ref = MG.fasta("breakpoint1_ref.fa")
    graph = R.build([[s.upper() for s in ref], []], 11)
    recs, text, stats, _, _ = B.call(graph, 11, 2, ref, names, 5, 1000)
    assert recs == [] and text == "" and stats["breaks"] == 0 and stats["ref_added"] == 0 and stats["occurrences"] > stats["ref_keys"]
    # the breakpoint2 reference holds its own SNP bubble: no call
    names, ref = MG.fasta("breakpoint2_ref.fa")
    assert len(ref) == 1 and len(ref[0]) == 200
    for k in (11, 31):
        graph = R.build([[s.upper() for s in ref], []], k)
        recs, text, stats, _, _ = B.call(graph, k, 2, ref, names, 5, 1000)
        assert recs == [] and text == "" and stats["breaks"] == 0


def test_names_are_cleaned_as_the_command_cleans_them():
    assert B.clean_name("chr1 a comment") == "chr1" and B.clean_name("a,b:c\tx") == "a.b;c" and B.clean_name("plain") == "plain"

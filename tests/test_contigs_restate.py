"""The restatement of `contigs` (contigs_restate.py) on the cases of contigs_cases.py against tests/golden/contigs.json,
and what the case set has to reach.  The golden file was written by the restatement (python tests/test_contigs_restate.py
--write) and then read through, not worked out by hand: at k = 5 the contig of `repeat` was checked to be the whole
genome U1 R U2 R U3 (its reverse complement, 45 nodes, two USELINKS steps, both ends StopNoCovg), the contig of `circle`
to be 1 + 45 + 45 nodes (two rounds and the node of the third entry each way, StopHitLoop twice) and the two contigs of
`merge_chain` to be X1 CORE Y1 and the second half of CORE with Y2, the contig of `rho` to be the tail and three rounds
of the loop (59 nodes, three POPFRK_COLFWD steps, StopNoCovg at the tail's start, StopHitLoop in the loop); the other entries were compared with these for
shape (stop causes, step counts, lengths) and no more."""
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contigs_cases as CC  # noqa: E402
import contigs_restate as G  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contigs.json")
STATUSES = (G.COLFWD, G.POPFWD, G.POPFRK_COLFWD, G.USELINKS)
EVENTS = ("choice_age_above_0", "gap_over_several_segments", "counter_link_answers_the_check", "counter_link_filtered",
          "counter_link_past_its_first_base", "link_finished_at_fork", "entered_again", "entered_again_in_another_state",
          "stopped_by_an_equal_state_after_rounds_with_links")


def plain(case):
    recs, seq, st = CC.run(case)
    out = []
    for r in recs:
        r = dict(r)
        r["gap_conf"] = ["%016x" % G.bits(x) for x in r["gap_conf"]]
        r["seed"] = G.kmer_str(r["seed"], case["k"])
        out.append(r)
    st = {k: v for k, v in st.items() if k != "events"}
    return {"records": out, "seq": seq.decode(), "stats": st, "fasta_head": G.fasta(case["k"], recs, seq).split("\n")[0] if recs else ""}


def test_cases_against_golden():
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(c["name"] for c in CC.cases())
    for c in CC.cases():
        assert plain(c) == want[c["name"]], c["name"]


def test_case_set_reaches_every_status_cause_and_rule():
    steps, stops, events, per = collections.Counter(), collections.Counter(), collections.Counter(), {}
    for c in CC.cases():
        _, _, st = CC.run(c)
        per[c["name"]] = st
        for i in range(9):
            steps[i] += st["wlk_steps"][i]
            stops[i] += st["stop_causes"][i]
        events.update(st["events"])
    assert all(steps[s] for s in STATUSES), steps
    assert all(stops[s] for s in range(9)), stops
    assert stops[G.STOP_UNKNOWN] == sum(st["corrupt_links"] for st in per.values())
    assert all(events[e] for e in EVENTS), events
    for k in CC.KS:
        # MISSING_LINKS that -M turns into USELINKS; SPLIT_LINKS at equal age; a corrupt link
        assert per["repeat_missing_k%d" % k]["stop_causes"][G.STOP_MISSING_PATHS] and not per["repeat_missing_k%d" % k]["wlk_steps"][G.USELINKS]
        assert per["repeat_missing_off_k%d" % k]["wlk_steps"][G.USELINKS] and not per["repeat_missing_off_k%d" % k]["stop_causes"][G.STOP_MISSING_PATHS]
        assert per["repeat_split_k%d" % k]["stop_causes"][G.STOP_SPLIT_PATHS] == 1
        assert per["repeat_corrupt_k%d" % k]["corrupt_links"] == 1
        assert per["repeat_low_step_k%d" % k]["stop_causes"][G.STOP_LOW_STEP] and per["repeat_low_cumul_k%d" % k]["stop_causes"][G.STOP_LOW_CUMUL]
        assert per["circle_k%d" % k]["stop_causes"][G.STOP_CYCLE] == 2
        # a cycle walked with different held links round by round and stopped on the entry that repeats a state
        rho = per["rho_k%d" % k]
        assert rho["events"]["stopped_by_an_equal_state_after_rounds_with_links"] == 1 and rho["events"]["link_finished_at_fork"] == 1
        recs = CC.run(next(c for c in CC.cases() if c["name"] == "rho_k%d" % k))[0]
        assert any(G.STOP_CYCLE in r["stop_causes"] and r["num_junc"] > 0 and r["wlk_steps"][G.POPFRK_COLFWD] >= 3 for r in recs)
        assert per["colours_c1_k%d" % k]["contigs"] > 0
        # the filter keeps the hand-made link on P out: the same contigs as without it
        assert per["merge_filtered_k%d" % k]["events"]["counter_link_filtered"]
        assert {k2: v for k2, v in per["merge_filtered_k%d" % k].items() if k2 != "events"} == {k2: v for k2, v in per["merge_k%d" % k].items() if k2 != "events"}
        # the seeding rule: j kills i (so i does not kill l), the seeds given twice go, one seed is no key; -N cuts inside
        chain = per["merge_chain_k%d" % k]
        assert (chain["contigs"], chain["num_reseed_abort"], chain["seeds_not_found"]) == (2, 3, 1)
        assert per["merge_chain_reseed_k%d" % k]["contigs"] == 4
        assert (per["merge_chain_limit_k%d" % k]["contigs"], per["merge_chain_limit_k%d" % k]["num_reseed_abort"]) == (1, 0)
        assert per["repeat_limit_k%d" % k]["contigs"] <= 2 and per["repeat_reseed_k%d" % k]["contigs"] == 7
        assert per["colours_k%d" % k]["wlk_steps"][G.POPFWD] and per["colours_k%d" % k]["stop_causes"][G.STOP_NOCOLCOVG]
    # with reseeding the contig of i holds l, which the contig of j does not: the chain is what keeps l
    for k in CC.KS:
        c = next(c for c in CC.cases() if c["name"] == "merge_chain_reseed_k%d" % k)
        recs, seq, _ = CC.run(c)
        text = [seq[r["seq_off"]:r["seq_off"] + r["len_nodes"] + k - 1].decode() for r in recs]
        sj, si, sl = c["params"]["seeds"][:3]
        has = lambda t, s: s in t or G.kmer_str(G.R.revcomp(G.R.kmer_int(s), k), k) in t  # noqa: E731
        assert has(text[0], si) and not has(text[0], sl) and has(text[1], sl)


def test_wide_case_set_reaches_what_the_narrow_one_does():
    """the cases at k = 63 .. 127 (keys of two, three and four words), which no golden pins: the conditions that the test
    above asserts per k of KS, per k of WIDE_KS, and its sums over the wide set alone"""
    cases = CC.wide_cases()
    assert sorted(c["name"] for c in cases) == sorted(c["name"].rsplit("_k", 1)[0] + "_k%d" % k for c in CC.cases() if c["k"] == CC.KS[0] for k in CC.WIDE_KS)
    steps, stops, events, per, recs_of = collections.Counter(), collections.Counter(), collections.Counter(), {}, {}
    for c in cases:
        recs, seq, st = CC.run(c)
        per[c["name"]], recs_of[c["name"]] = st, (recs, seq)
        for i in range(9):
            steps[i] += st["wlk_steps"][i]
            stops[i] += st["stop_causes"][i]
        events.update(st["events"])
    assert all(steps[s] for s in STATUSES), steps
    assert all(stops[s] for s in range(9)), stops
    assert stops[G.STOP_UNKNOWN] == sum(st["corrupt_links"] for st in per.values())
    assert all(events[e] for e in EVENTS), events
    plain_stats = lambda st: {k2: v for k2, v in st.items() if k2 != "events"}  # noqa: E731
    for k in CC.WIDE_KS:
        st = lambda name: per["%s_k%d" % (name, k)]  # noqa: E731
        assert st("repeat_missing")["stop_causes"][G.STOP_MISSING_PATHS] and not st("repeat_missing")["wlk_steps"][G.USELINKS]
        assert st("repeat_missing_off")["wlk_steps"][G.USELINKS] and not st("repeat_missing_off")["stop_causes"][G.STOP_MISSING_PATHS]
        assert st("repeat_split")["stop_causes"][G.STOP_SPLIT_PATHS] == 1
        assert st("repeat_corrupt")["corrupt_links"] == 1
        assert st("repeat_low_step")["stop_causes"][G.STOP_LOW_STEP] and st("repeat_low_cumul")["stop_causes"][G.STOP_LOW_CUMUL]
        assert st("circle")["stop_causes"][G.STOP_CYCLE] == 2
        rho = st("rho")
        assert rho["events"]["stopped_by_an_equal_state_after_rounds_with_links"] == 1 and rho["events"]["link_finished_at_fork"] == 1
        assert any(G.STOP_CYCLE in r["stop_causes"] and r["num_junc"] > 0 and r["wlk_steps"][G.POPFRK_COLFWD] >= 3 for r in recs_of["rho_k%d" % k][0])
        assert st("colours_c1")["contigs"] > 0
        assert st("merge_filtered")["events"]["counter_link_filtered"]
        assert plain_stats(st("merge_filtered")) == plain_stats(st("merge"))
        chain = st("merge_chain")
        assert (chain["contigs"], chain["num_reseed_abort"], chain["seeds_not_found"]) == (2, 3, 1)
        assert st("merge_chain_reseed")["contigs"] == 4
        assert (st("merge_chain_limit")["contigs"], st("merge_chain_limit")["num_reseed_abort"]) == (1, 0)
        assert st("repeat_limit")["contigs"] <= 2 and st("repeat_reseed")["contigs"] == 7
        assert st("colours")["wlk_steps"][G.POPFWD] and st("colours")["stop_causes"][G.STOP_NOCOLCOVG]
        # with reseeding the contig of i holds l, which the contig of j does not
        c = next(c for c in cases if c["name"] == "merge_chain_reseed_k%d" % k)
        recs, seq = recs_of[c["name"]]
        text = [seq[r["seq_off"]:r["seq_off"] + r["len_nodes"] + k - 1].decode() for r in recs]
        sj, si, sl = c["params"]["seeds"][:3]
        has = lambda t, s: s in t or G.kmer_str(G.R.revcomp(G.R.kmer_int(s), k), k) in t  # noqa: E731
        assert has(text[0], si) and not has(text[0], sl) and has(text[1], sl)


def test_confidence_table_shape():
    t = G.conf_table({}, 100)
    assert t == [] and G.conf_csv(t) == "gap_dist\tconfidence_0\n"
    t = G.conf_table({40: 3, 60: 1}, 1000)
    assert len(t) == 61 and t[0] == 0.0 and all(0.0 <= x <= 1.0 for x in t) and t[1] > t[60]


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    with open(GOLDEN, "w") as f:
        json.dump({c["name"]: plain(c) for c in CC.cases()}, f, indent=0, sort_keys=True)
        f.write("\n")

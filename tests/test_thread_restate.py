"""thread_restate.py on the CPU: it reproduces the vectors of the reference's own unit test (golden/thread.json, from
src/tests/path_tests.c), the random case of thread_cases.py reaches every rule of the restatement at least three times,
and the totals of the header follow from the links."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_restate as C  # noqa: E402
import thread_cases as TC  # noqa: E402
import thread_restate as T  # noqa: E402

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thread.json")))["path_tests"]


def golden_store():
    k = GOLDEN["k"]
    return T.Store(R.build([GOLDEN["graph_seqs"]], k), k)


def test_golden_counts_after_each_call():
    st = golden_store()
    assert [(c["links_total"], c["kmers_total"]) for c in GOLDEN["calls"]] == [(5, 5), (10, 7), (13, 9), (15, 10)]
    for c in GOLDEN["calls"]:
        before = st.info()
        st.thread([c["read"]], two_way=not GOLDEN["one_way"], D=GOLDEN["gap_variance"], d=GOLDEN["gap_wiggle"])
        info = st.info()
        assert (info["num_paths"], info["num_kmers_with_paths"]) == (c["links_total"], c["kmers_total"])
        assert info["num_paths"] - before["num_paths"] == c["links_added"]
        assert info["num_kmers_with_paths"] - before["num_kmers_with_paths"] == c["kmers_added"]
    assert st.stats["links_added"] == 15 and all(n == 1 for n in st.links.values())
    assert st.contig_hist() == [(31, 4)]


def test_golden_traced_sequences():
    st = golden_store().thread([c["read"] for c in GOLDEN["calls"]])
    k = st.k
    got = {}
    for (key, o, bases) in st.links:
        nodes, pos = st.fetch(key, o, bases)
        assert len(pos) == len(bases)
        got.setdefault(C.contig_str(k, nodes)[:k], []).append(C.contig_str(k, nodes))
    assert {a: sorted(b) for a, b in got.items()} == {a: sorted(b) for a, b in GOLDEN["traced"].items()}


def test_golden_text_lines():
    st = golden_store().thread([c["read"] for c in GOLDEN["calls"]])
    lines = st.text().decode().splitlines()
    assert lines[:2] == ["AATCGAATGAC 1", "R 2 1 AG seq=GTCATTCGATTTGGTGTCATTCGCACCCAGG juncpos=13,19"]
    heads = [ln.split()[0] for ln in lines if ln[0] not in "FR" or " " not in ln[:2]]
    assert heads == sorted(heads) and len(heads) == 10
    assert st.text(seq=False).decode().splitlines()[1] == "R 2 1 AG"
    # the same reads again: nothing new, every count doubles; 300 times: the count stays at 255
    st.thread([c["read"] for c in GOLDEN["calls"]])
    assert st.info()["num_paths"] == 15 and set(st.links.values()) == {2}
    st.thread([GOLDEN["calls"][0]["read"]] * 300)
    assert max(st.links.values()) == 255 and min(st.links.values()) == 2


def test_link_order_is_gpath_cmp():
    st = golden_store()
    st.links = {(5, 1, (0,)): 1, (5, 0, (3, 3)): 1, (5, 0, (3,)): 1, (5, 0, (1, 0)): 1, (2, 1, (2,)): 1}
    assert st.by_kmer() == [(2, [(1, (2,), 1)]), (5, [(0, (1, 0), 1), (0, (3,), 1), (0, (3, 3), 1), (1, (0,), 1)])]


@pytest.mark.parametrize("k", TC.KS)
def test_random_case_reaches_every_rule(k):
    st = TC.check_reach(k)
    info = st.info()
    per = st.by_kmer()
    assert info["num_paths"] == sum(len(links) for _, links in per) == len(st.links)
    assert info["num_kmers_with_paths"] == len(per)
    assert info["path_bytes"] == sum((len(b) + 3) // 4 for _, links in per for _, b, _ in links)
    assert sum(n for _, n in st.contig_hist()) == st.stats["contigs"]
    assert sum((length - k + 1) * n for length, n in st.contig_hist()) == st.stats["contig_kmers"]
    assert st.stats["end_gaps"] == st.stats["end_gaps_extended"] == st.stats["bases_filled"] == 0
    # cut to three junctions: links merge behind the cut
    cut = TC.expected(k, False, 3)
    assert max(len(b) for _, _, b in cut.links) == 3 and len(cut.links) < len(st.links)
    assert cut.stats == st.stats

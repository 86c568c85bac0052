"""The restatement of `popbubbles` (pop_restate.py) against expectations worked out by hand (pop_cases.py) and the
reference's own two tests (tests/pop_bubbles/pop_bubbles1 and pop_bubbles2: golden/pop_bubbles.json)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import pop_cases as P  # noqa: E402
import pop_restate as PR  # noqa: E402

CASES = P.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_made(case):
    name, k, graph, args, gone, pops = case
    info = {}
    out, popped, nremoved = PR.pop(graph, k, *args, info=info)
    assert info["removed"] == gone and nremoved == len(gone)
    assert popped == pops
    assert info["fragments"] == 0
    assert set(out) == set(graph) - gone
    for key, (cv, ed) in out.items():
        assert cv == graph[key][0]
        for c, e in enumerate(ed):
            for b in range(8):
                to_gone = R.step(key, b >> 2, b & 3, k)[0] in gone
                assert (e >> b) & 1 == (0 if to_gone else (graph[key][1][c] >> b) & 1)


def test_case_list_covers_the_ground():
    names = {c[0] for c in CASES}
    assert {"three_branches_top_first", "tie", "tie_chain", "snp_C_keeps", "snp_L_keeps", "indel_D_keeps", "hairpin_loop",
            "branch_of_length_1_goes", "one_sided_edge", "snp_zeros_ignore_C_and_L"} <= names
    # the tie chain really is a chain: three ties would be found if A and C were parallel too
    info = {}
    chain = next(c for c in CASES if c[0] == "tie_chain")
    PR.pop(chain[2], chain[1], info=info)
    assert info["pairs"] == 2 and info["ties"] == 2


def test_option_defaults():
    # (!max || x <= max) for -C and -L: -1 (unset) and 0 both ignore; (max < 0 || diff <= max) for -D: 0 counts
    for off in (-1, 0):
        assert PR.passes(10**9, 10**9, 5, 5, off, off, -1)
    assert PR.passes(3, 7, 7, 7, 3, 7, 0) and not PR.passes(4, 7, 7, 7, 3, 7, 0) and not PR.passes(3, 8, 8, 8, 3, 7, 0)
    assert not PR.passes(1, 1, 7, 8, -1, -1, 0) and PR.passes(1, 1, 7, 8, -1, -1, 1) and PR.passes(1, 1, 8, 7, -1, -1, 1)


def oracle_graph(k, colours):
    from oracle import orc
    og = orc.Graph(k, len(colours), 1 << 12)
    for c, seqs in enumerate(colours):
        og.add_reads(c, *orc.pack_reads(seqs))
    return R.parse(og.body_bytes(True), k, len(colours))


@pytest.mark.parametrize("name", ["pop_bubbles1", "pop_bubbles2"])
def test_reference_cases(mcx, name):
    gold = P.golden()
    k, case = gold["kmer_size"], gold[name]
    graph = oracle_graph(k, [inp["seqs"] for inp in case["inputs"]])
    truth = oracle_graph(k, [case["truth"]])
    out, popped, nremoved = PR.pop(graph, k)
    assert set(out) == set(truth) and popped >= 1 and nremoved == len(graph) - len(truth) == k
    assert len(next(iter(out.values()))[0]) == len(case["inputs"])  # the output keeps the input's colours


def test_fragment_of_a_unitig_is_outside_the_restatement():
    # one-sided edges can make an alternative a fragment of a unitig; clean_restate's decomposition is then no partition
    k, graph, _ = P.fragment_case()
    with pytest.raises(AssertionError, match="two unitigs"):
        PR.pop(graph, k)

"""The CPU restatement of `subgraph` (subgraph_restate.py) against the counts the reference pins in tests/subgraph,
tests/subgraph_unitigs and src/tests/subgraph_tests.c (tests/golden/subgraph.json), and hand-made cases."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import subgraph_restate as S  # noqa: E402

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subgraph.json")))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def kept(graph, k, seeds, **kw):
    out, st = S.subgraph(graph, k, seeds, **kw)
    assert st["nkmers_kept"] == len(out) and st["nkmers_kept"] + st["nkmers_removed"] == len(graph)
    return out, st


@pytest.mark.parametrize("colours", [(0,), (0, 2)])
def test_reference_k9(colours):
    c = GOLD["k9"]
    ncols = max(colours) + 1
    graph = R.build([c["graph"] if i in colours else [] for i in range(ncols)], c["k"])
    for dist, n in c["expected"].items():
        out, _ = kept(graph, c["k"], [c["seed"]], dist=int(dist))
        assert len(out) == n
        # the records survive a round trip through the .ctx body
        assert R.parse(R.pack(out, c["k"], ncols), c["k"], ncols) == out


def test_reference_k19():
    c = GOLD["k19"]
    k = c["k"]
    graph = R.build([c["graph"]], k)
    assert len(graph) == c["nkmers"] == 982
    for dist in range(11):
        out, st = kept(graph, k, [c["seed"]], dist=dist)
        assert len(out) == 2 * dist + 2 and st["num_seed_kmers"] == 3 and st["num_seed_found"] == 2 and st["levels"] == dist
    out, st = kept(graph, k, [c["seed2"]], dist=c["seed2_dist"])
    assert len(out) == c["seed2_expected"] == 0 and st["num_seed_kmers"] == 1 and st["num_seed_found"] == 0
    out, st = kept(graph, k, [c["seed"]], dist=c["all_dist"])
    assert len(out) == c["all_expected"] == 982 and out == graph


def test_reference_k11_unitigs():
    c = GOLD["k11"]
    k = c["k"]
    seqs = [s.upper() for s in c["graph"]]  # the lower-case bases count as bases
    graph = R.build([seqs], k)
    for i in c["inner"]:
        assert len(kept(graph, k, [seqs[0][i:i + k]], unitigs=True)[0]) == c["inner_expected"]
    for which, at in c["ends"]:
        assert len(kept(graph, k, [c["graph"][which][at:at + k]], unitigs=True)[0]) == c["end_expected"]
    assert len(kept(graph, k, [c["cli_seed"]], unitigs=True)[0]) == 5


def path_graph(seq, k, ncols=1, col=0):
    return R.build([[seq] if c == col else [] for c in range(ncols)], k)


SEQ = "ACGGTCATTGCAAGTCCGATAGGC"


def test_absent_neighbour_is_passed_over():
    k = 5
    graph = path_graph(SEQ, k)
    gone = R.canon(R.kmer_int(SEQ[4:9]), k)
    del graph[gone]
    out, st = kept(graph, k, [SEQ[:5]], dist=100)
    assert set(out) == {R.canon(R.kmer_int(SEQ[i:i + k]), k) for i in range(4)}
    assert all(R.step(key, b >> 2, b & 3, k)[0] in out for key in out for b in range(8) if (R.union_edges(out, key) >> b) & 1)


def test_closed_cycle():
    k = 5
    cyc = "ACGGTCATTG"
    graph = path_graph(cyc + cyc[:k], k)
    assert len(graph) == len(cyc)
    for dist, n in ((0, 1), (1, 3), (4, 9), (5, 10), (50, 10)):
        out, st = kept(graph, k, [cyc[:k]], dist=dist)
        assert len(out) == n and st["levels"] == min(dist, 5)
    assert len(kept(graph, k, [cyc[:k]], unitigs=True)[0]) == len(cyc)


def test_both_sides_lead_to_the_same_neighbour():
    # ACACA -> CACAC over its forward side (ACACAC) and over its reverse side (TGTGT G = the reverse complement of CACAC)
    k = 5
    graph = R.build([["ACACAC", "TGTGTG", "CACACGGTA"]], k)
    x, y = R.canon(R.kmer_int("ACACA"), k), R.canon(R.kmer_int("CACAC"), k)
    e = R.union_edges(graph, x)
    both = [(b >> 2, R.step(x, b >> 2, b & 3, k)[0]) for b in range(8) if (e >> b) & 1]
    assert (0, y) in both and (1, y) in both
    out, st = kept(graph, k, ["ACACA"], dist=1)
    assert set(out) == {x, y} and st["levels"] == 1 and st["max_frontier"] == 1
    assert len(kept(graph, k, ["ACACA"], dist=9)[0]) == len(graph)


def test_edge_only_in_second_colour():
    k = 7
    a, b = SEQ[:12], SEQ[12:]  # the join between the halves is in colour 1 alone
    graph = R.build([[a, b], [SEQ]], k)
    assert len(graph) == len(SEQ) - k + 1
    out, st = kept(graph, k, [SEQ[:k]], dist=100)
    assert out == graph
    assert S.guards(graph, k, [SEQ[:k]], 100)["only_other_colour"] > 0
    one = R.build([[a, b]], k)
    assert len(kept(one, k, [SEQ[:k]], dist=100)[0]) == len(a) - k + 1


def test_seed_forms():
    k = 5
    graph = path_graph(SEQ, k)
    base, _ = kept(graph, k, [SEQ[3:12]], dist=2)
    assert kept(graph, k, [rc(SEQ[3:12])], dist=2)[0] == base
    assert kept(graph, k, [SEQ[3:12].lower()], dist=2)[0] == base
    out, st = kept(graph, k, [SEQ[3:12], SEQ[3:12], SEQ[5:12]], dist=2)
    assert out == base and st["num_seed_kmers"] == 5 + 5 + 3 and st["num_seed_found"] == 5
    # an N cuts the seed: the k-mers across it are not seeds
    out, st = kept(graph, k, [SEQ[:5] + "N" + SEQ[6:11]], dist=0)
    assert st["num_seed_kmers"] == 2 and len(out) == 2
    assert kept(graph, k, ["ACG"], dist=5)[1]["num_seed_kmers"] == 0  # shorter than k


def test_invert_and_empty():
    k = 5
    graph = R.build([[SEQ], [SEQ[4:]]], k)
    out, st = kept(graph, k, [SEQ[8:14]], dist=1)
    inv, sti = kept(graph, k, [SEQ[8:14]], dist=1, invert=True)
    assert set(inv) == set(graph) - set(out) and inv == S.prune(graph, k, set(graph) - set(out))
    assert 0 < len(out) < len(graph) and sti["nkmers_kept"] == len(graph) - len(out)
    assert any(inv[key][1] != graph[key][1] for key in inv)  # edges into the removed part went
    none, st = kept(graph, k, [], dist=7)
    assert none == {} and st["nkmers_removed"] == len(graph) and st["max_frontier"] == 0
    everything, st = kept(graph, k, [], dist=7, invert=True)
    assert everything == graph

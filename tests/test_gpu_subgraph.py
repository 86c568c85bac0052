"""`subgraph` on the MI355X (Graph.subgraph*, csrc/mcx_subgraph.h) against the CPU restatement in subgraph_restate.py:
the surviving records byte for byte (sorted), the table's k-mer count and checksum, and every field of the stats the
restatement computes.  Every randomised case first asserts, on the restatement alone, that it keeps some but not all
k-mers, that at least three levels add k-mers, that some k-mer is reached only over a reverse-side edge and, with
several colours, that some k-mer is reached only over an edge colour 0 lacks."""
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import subgraph_restate as S  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subgraph.json")))
FOREVER = 2**32 - 1


def rseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def planted(rng, k, ncols, glen, nreads, readlen):
    """reads of a genome and of a second haplotype with a SNP every 3 k bases or so (branches), half of them reverse
    complemented, dealt out over the colours; a second, unrelated genome makes a component the seeds never reach.
    Returns (sequences per colour, the first genome)"""
    g1 = rseq(rng, glen)
    h2 = list(g1)
    for p in range(k, glen, 3 * k + 1):
        h2[p] = rng.choice([b for b in "ACGT" if b != g1[p]])
    h2 = "".join(h2)
    other = rseq(rng, max(k + 2, glen // 3))
    cols = [[] for _ in range(ncols)]
    for i in range(nreads):
        hap = g1 if rng.random() < 0.6 else h2
        p = rng.randrange(0, max(1, len(hap) - readlen))
        r = hap[p:p + readlen]
        cols[rng.randrange(ncols)].append(rc(r) if rng.random() < 0.5 else r)
    cols[-1].append(g1)  # every k-mer of the genome is there; its joins, in colour 0, only where reads cross them
    cols[0].append(other)
    return cols, g1


def load_graph(graph, k, cap=1 << 16):
    ncols = len(next(iter(graph.values()))[0])
    g = mcx.Graph(k, ncols, cap)
    g.add_records(R.pack(graph, k, ncols), ncols, [(c, c) for c in range(ncols)])
    g.sync()
    return g, ncols


def arrays(seeds):
    seqs = [s.encode() for s in seeds]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) or b"\n", dtype=np.uint8), offs


def seed_with(g, seeds, how):
    if how == "reads":
        g.subgraph_seed(*arrays(seeds))
    elif how == "three":
        for part in (seeds[0::3], seeds[1::3], seeds[2::3]):
            g.subgraph_seed(*arrays(part))
    else:
        import torch
        text = ("\n".join(seeds) + "\n").encode()
        d = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        g.subgraph_seed_stream_dev(d, len(text))
        g.sync()  # (the tensor lives until the kernel has read it)


def check(graph, k, seeds, dist=0, invert=False, unitigs=False, how="reads", knobs=(), cap=1 << 16, expect=None):
    exp, est = expect or S.subgraph(graph, k, seeds, dist, invert, unitigs)
    g, ncols = load_graph(graph, k, cap)
    for key, value in knobs:
        g.configure(key, value)
    g.subgraph_begin(unitigs)
    seed_with(g, seeds, how)
    st = g.subgraph_finish(dist, invert, unitigs)
    print("subgraph k=%d cols=%d dist=%d invert=%d unitigs=%d %s %s: %s (expected %s)" % (k, ncols, dist, invert, unitigs, how, knobs, st, est))
    for name, value in est.items():
        assert st[name] == value, name
    out = g.export(True)
    assert out == R.pack(exp, k, ncols)
    assert g.nkmers == len(exp)
    cs, n = g.checksum()
    assert n == len(exp) and cs == mcx.records_checksum(out, k, ncols)
    g.close()
    return st


# (k, colours): generator seeds chosen on the CPU so that the guards below hold
SEEDS = {(3, 1): 3, (5, 2): 5, (31, 1): 0, (33, 3): 0, (63, 2): 0, (65, 1): 0, (127, 2): 5}


def random_case(k, ncols):
    rng = random.Random(9000 + 131 * SEEDS[(k, ncols)] + k)
    glen = {3: 16, 5: 60}.get(k, 1100 + k)
    cols, genome = planted(rng, k, ncols, glen, {3: 3, 5: 12}.get(k, 60), min(glen, 2 * k + 40))
    graph = R.build(cols, k)
    at = len(genome) // 2
    seeds = [genome[at:at + k + 1], rc(genome[at + 2:at + k + 3]), genome[:k - 1]]
    return graph, seeds


def guard(graph, k, seeds, dist, ncols):
    gd = S.guards(graph, k, seeds, dist)
    assert 0 < gd["kept"] < len(graph) and gd["levels"] >= 3 and gd["only_reverse"] > 0, gd
    assert ncols == 1 or gd["only_other_colour"] > 0, gd
    return gd


@pytest.mark.parametrize("k,ncols", sorted(SEEDS))
def test_random_graphs(k, ncols):
    graph, seeds = random_case(k, ncols)
    main = max(k, 3)
    guard(graph, k, seeds, main, ncols)
    guard(graph, k, seeds, FOREVER, ncols)
    for dist in (0, 1, 2, k, 4 * len(graph), FOREVER):
        check(graph, k, seeds, dist)
    check(graph, k, seeds, main, invert=True)
    check(graph, k, seeds, 2, unitigs=True)
    check(graph, k, seeds, 1, invert=True, unitigs=True)


def mid_graph():
    """about 10^4 k-mers at k = 31 in three colours, seeds of more than one tile of stream"""
    rng = random.Random(77)
    k, ncols = 31, 3
    cols, genome = planted(rng, k, ncols, 9000, 700, 100)
    graph = R.build(cols, k)
    seeds = [genome[p:p + 90] for p in range(1000, 7000, 120)] + ["ACGTNNACGT", genome[8000:8040].lower()]
    assert sum(len(s) + 1 for s in seeds) > 4096
    return k, ncols, graph, seeds


def test_grid_and_seed_routes():
    k, ncols, graph, seeds = mid_graph()
    dist = 12
    guard(graph, k, seeds, dist, ncols)
    expect = S.subgraph(graph, k, seeds, dist)
    for grid in (1, 3, 0):
        for how in ("reads", "stream", "three"):
            check(graph, k, seeds, dist, how=how, knobs=(("grid", grid),), expect=expect)
    check(graph, k, seeds, dist, unitigs=True, how="stream", knobs=(("grid", 1),))


def test_decomposition_reused():
    k, ncols, graph, seeds = mid_graph()
    exp, est = S.subgraph(graph, k, seeds, 3, False, True)
    g, _ = load_graph(graph, k)
    g.unitig_stats()
    st = g.subgraph(seeds, 3, unitigs=True)
    assert all(st[name] == value for name, value in est.items())
    assert g.export(True) == R.pack(exp, k, ncols)
    # the pruned table (tombstones, the decomposition gone): once more, plain
    exp2, est2 = S.subgraph(exp, k, seeds[:5], 2)
    st = g.subgraph(seeds[:5], 2)
    assert all(st[name] == value for name, value in est2.items())
    assert g.export(True) == R.pack(exp2, k, ncols) and g.nkmers == len(exp2)
    g.close()


def test_1e5_kmers():
    rng = random.Random(5)
    k = 31
    cols, genome = planted(rng, k, 1, 100000, 800, 100)
    graph = R.build(cols, k)
    assert len(graph) > 100000
    seeds = [genome[p:p + 150] for p in range(20000, 30000, 500)]
    guard(graph, k, seeds, 200, 1)
    st = check(graph, k, seeds, 200, cap=1 << 19)
    assert st["nkmers_kept"] > 10000


def test_table_at_95_percent_load():
    k = 31
    probe = mcx.Graph(k, 1, 1 << 14)
    slots = probe.capacity()[0] * 32 // 33
    probe.close()
    rng = random.Random(35)
    genome = rseq(rng, int(slots * 0.95) + k - 1)
    graph = R.build([[genome]], k)
    assert len(graph) >= 0.94 * slots
    seeds = [genome[5000:5100], rc(genome[9000:9050])]
    gd = S.guards(graph, k, seeds, 40)
    assert 0 < gd["kept"] < len(graph) and gd["levels"] >= 3 and gd["only_reverse"] > 0
    check(graph, k, seeds, 40, cap=1 << 14)
    check(graph, k, seeds, 40, invert=True, cap=1 << 14)


def bushy_graph():
    """a path of 300 k-mers that opens into a tree of 4^5 branches; all but three branches end after 10 k-mers, two after
    200 and one after 400: from the path's far end the frontier is 1, then 1024, then 3, then 1"""
    rng = random.Random(13)
    k = 31
    path = rseq(rng, 300 + k - 1)
    seqs = []
    for i in range(4**5):
        twig = "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(5))
        seqs.append(path[-k:] + twig + rseq(rng, {0: 400, 1: 200, 2: 200}.get(i, 10)))
    graph = R.build([[path] + seqs], k)
    return k, graph, [path[:k]]


def test_narrow_and_wide_alternate():
    k, graph, seeds = bushy_graph()
    marked, _ = S.mark_seeds(graph, k, seeds)
    sizes = []
    S.extend(graph, k, marked, FOREVER, sizes=sizes)
    top = sizes.index(max(sizes))
    assert sizes[0] == 1 and max(sizes) > 256 and 1 < min(sizes[top:top + 150]) <= 256 and sizes[-1] == 1, sizes
    assert any(a <= 256 < b for a, b in zip(sizes, sizes[1:])) and any(a > 256 >= b for a, b in zip(sizes, sizes[1:]))
    assert any(a == 1 < b for a, b in zip(sizes, sizes[1:])) and any(a > 1 == b for a, b in zip(sizes, sizes[1:]))
    for dist in (330, FOREVER):
        expect = S.subgraph(graph, k, seeds, dist)
        assert dist == FOREVER or 0 < expect[1]["nkmers_kept"] < len(graph)
        for narrow in (0, 1, 256, 100000):
            st = check(graph, k, seeds, dist, knobs=(("subgraph_narrow", narrow),), expect=expect)
            assert (st["narrow_launches"] == 0) if narrow == 0 else (st["narrow_launches"] > 0)


def test_reference_k19_through_the_narrow_kernel():
    c = GOLD["k19"]
    k = c["k"]
    graph = R.build([c["graph"]], k)
    narrow = (("subgraph_narrow", 256),)  # (the knob is 0, never, by default)
    st = check(graph, k, [c["seed"]], c["all_dist"], knobs=narrow)
    assert st["nkmers_kept"] == c["all_expected"] == len(graph) and st["narrow_launches"] >= 1 and st["max_frontier"] == 2
    for dist in (0, 3, 10):
        assert check(graph, k, [c["seed"]], dist, knobs=narrow)["nkmers_kept"] == 2 * dist + 2
    assert check(graph, k, [c["seed2"]], c["seed2_dist"], knobs=narrow)["nkmers_kept"] == 0
    assert check(graph, k, [c["seed"]], c["all_dist"])["narrow_launches"] == 0  # the default: chained launches alone


def test_reference_k9_and_k11():
    c = GOLD["k9"]
    for cols in ([c["graph"]], [c["graph"], [], c["graph"]]):
        graph = R.build(cols, c["k"])
        for dist, n in c["expected"].items():
            assert check(graph, c["k"], [c["seed"]], int(dist))["nkmers_kept"] == n
    c = GOLD["k11"]
    graph = R.build([[s.upper() for s in c["graph"]]], c["k"])
    for i in c["inner"]:
        assert check(graph, c["k"], [c["graph"][0][i:i + c["k"]]], unitigs=True)["nkmers_kept"] == c["inner_expected"]
    for which, at in c["ends"]:
        assert check(graph, c["k"], [c["graph"][which][at:at + c["k"]]], unitigs=True)["nkmers_kept"] == c["end_expected"]


def test_empty_seeds_and_empty_graph():
    k, ncols, graph, seeds = mid_graph()
    check(graph, k, [], 5)
    check(graph, k, ["ACGT", "N" * 50], 5, invert=True)
    g = mcx.Graph(31, 1, 1 << 16)
    st = g.subgraph(["ACGT" * 20], 4)
    assert st["nkmers_before"] == 0 and st["nkmers_kept"] == 0 and st["num_seed_found"] == 0 and st["num_seed_kmers"] == 50
    g.close()


def test_state_handling():
    k, ncols, graph, seeds = mid_graph()
    g, _ = load_graph(graph, k)
    with pytest.raises(Exception, match="begin"):
        g.subgraph_finish(1)
    with pytest.raises(Exception, match="begin"):
        g.subgraph_seed(*arrays(seeds))
    before = g.export(True)
    g.subgraph_begin()
    g.subgraph_seed(*arrays(seeds[:3]))
    g.subgraph_begin()  # a second begin starts over: the seeds above are forgotten
    g.subgraph_seed(*arrays(seeds[3:6]))
    with pytest.raises(Exception, match="unitigs flag"):
        g.subgraph_finish(1, unitigs=True)
    g.subgraph_begin()
    g.subgraph_seed(*arrays(seeds[3:6]))
    st = g.subgraph_finish(4)
    exp, est = S.subgraph(graph, k, seeds[3:6], 4)
    assert all(st[name] == value for name, value in est.items()) and g.export(True) == R.pack(exp, k, ncols)
    with pytest.raises(Exception, match="begin"):
        g.subgraph_finish(1)
    g.subgraph_begin()
    g.reset()
    with pytest.raises(Exception, match="begin"):
        g.subgraph_finish(1)
    assert before
    g.close()
    g = mcx.Graph(31, 2, 1 << 16)
    g.configure("intersect", 1)
    with pytest.raises(Exception, match="intersect"):
        g.subgraph_begin()
    g.close()
    g = mcx.Graph(31, 1, 1 << 16, nparts=2, part=0)
    with pytest.raises(Exception, match="split over devices"):
        g.subgraph_begin()
    g.close()

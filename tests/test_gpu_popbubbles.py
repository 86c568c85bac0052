"""`popbubbles` on the MI355X (Graph.pop_bubbles, csrc/mcx_pop.h) against the CPU restatement in pop_restate.py: the
surviving records byte for byte (sorted), num_popped, the removed k-mer count, the table's k-mer count and checksum.
Every randomised case first asserts, on the restatement alone, that its input pops at least one bubble."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import pop_cases as P  # noqa: E402
import pop_restate as PR  # noqa: E402
import unitigs_restate as U  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = P.cases()
rseq, rc = P.rseq, P.rc


def mutate(rng, s, err):
    return "".join(rng.choice("ACGT") if rng.random() < err else ch for ch in s)


def planted(rng, k, ncols, genome_len, nreads, readlen, err):
    """reads of two haplotypes: the second differs from the first by a SNP or a short insertion or deletion every
    3k bases or so; sequencing errors on top"""
    hap1 = rseq(rng, genome_len)
    hap2, i = [], 0
    while i < genome_len:
        j = min(genome_len, i + rng.randrange(2 * k + 2, 4 * k + 4))
        hap2.append(hap1[i:j])
        what = rng.randrange(3)
        if what == 0 and j < genome_len:
            hap2.append(rng.choice([b for b in "ACGT" if b != hap1[j]]))  # a SNP
            j += 1
        elif what == 1:
            hap2.append(rseq(rng, rng.randrange(1, 4)))  # an insertion
        else:
            j += rng.randrange(1, 4)  # a deletion
        i = j
    hap2 = "".join(hap2)
    cols = []
    for c in range(ncols):
        seqs = [hap1] * 3 + [hap2] * (1 + c % 2)  # whole haplotypes: every planted variant is a bubble
        for _ in range(nreads):
            hap = hap1 if rng.random() < 0.6 else hap2
            p = rng.randrange(0, max(1, len(hap) - readlen))
            r = mutate(rng, hap[p:p + readlen], err)
            seqs.append(rc(r) if rng.random() < 0.5 else r)
        cols.append(seqs)
    return cols


def load(k, ncols, cols, cap=1 << 16):
    g = mcx.Graph(k, ncols, cap)
    for c, seqs in enumerate(cols):
        bases = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        g.add_reads(c, bases, offs)
    g.sync()
    return g


def load_graph(graph, k, cap=1 << 16):
    ncols = len(next(iter(graph.values()))[0])
    g = mcx.Graph(k, ncols, cap)
    g.add_records(R.pack(graph, k, ncols), ncols, [(c, c) for c in range(ncols)])
    g.sync()
    return g, ncols


def expect(g, k, ncols, args, min_pops=1, min_ties=0):
    """the restatement's answer for the graph in the table; the guard against a vacuous pass comes before the device"""
    graph = R.parse(g.export(True), k, ncols)
    info = {}
    exp, popped, nremoved = PR.pop(graph, k, *args, info=info)
    assert popped >= min_pops and info["ties"] >= min_ties and info["fragments"] == 0, (popped, info["ties"])
    return graph, exp, popped, nremoved, info


def check(g, k, ncols, args=(-1, -1, -1), min_pops=1, min_ties=0, known=None):
    graph, exp, popped, nremoved, info = known or expect(g, k, ncols, args, min_pops, min_ties)
    st = g.pop_bubbles(*args)
    print("popbubbles k=%d cols=%d args=%s: %d k-mers, popped %d (expected %d), removed %d (%d), pairs %d (%d), rounds %d"
          % (k, ncols, args, len(graph), st["num_popped"], popped, st["nkmers_removed"], nremoved, st["num_pairs"], info["pairs"],
             st["rounds"]))
    assert st["num_popped"] == popped and st["nkmers_removed"] == nremoved and st["nkmers_before"] == len(graph)
    out = g.export(True)
    assert out == R.pack(exp, k, ncols)
    assert g.nkmers == len(exp)
    cs, n = g.checksum()
    assert n == len(exp) and cs == mcx.records_checksum(out, k, ncols)
    return st, exp


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_made(case):
    name, k, graph, args, gone, pops = case
    g, ncols = load_graph(graph, k)
    st, exp = check(g, k, ncols, args, min_pops=0)
    assert st["num_popped"] == pops and set(exp) == set(graph) - gone
    g.close()


# seeds chosen on the CPU so that every (k, colours, options) below pops at least one bubble in the restatement
SEEDS = {3: 7, 5: 3, 33: 1, 127: 3}
ARGS = lambda k, ncols: ((-1, -1, -1), (4 * ncols, -1, -1), (-1, k + 1, -1), (-1, -1, 0), (5 * ncols, k + 2, 1))  # noqa: E731


def random_cols(k, ncols):
    rng = random.Random(7000 + 100 * SEEDS.get(k, 0) + k)
    glen = {3: 14, 5: 90}.get(k, 300 + 10 * k)
    return planted(rng, k, ncols, glen, 20, min(glen, 2 * k + 30), 0.004)


@pytest.mark.parametrize("k,ncols", [(3, 1), (5, 2), (21, 3), (31, 1), (33, 2), (63, 1), (65, 3), (95, 1), (127, 2)])
def test_random_graphs(k, ncols):
    cols = random_cols(k, ncols)
    for args in ARGS(k, ncols):
        g = load(k, ncols, cols)
        check(g, k, ncols, args)
        g.close()


def big_graph():
    """about 10^5 k-mers at k = 31: two haplotypes with a SNP every 400 bases.  The first 60 % is read at random with
    errors; the rest is covered by one copy of each haplotype only, so its bubbles are ties"""
    rng = random.Random(41)
    k, n = 31, 70000
    hap1 = rseq(rng, n)
    h2 = list(hap1)
    for p in range(200, n, 400):
        h2[p] = rng.choice([b for b in "ACGT" if b != hap1[p]])
    hap2 = "".join(h2)
    seqs = []
    for _ in range(6000):
        hap = hap1 if rng.random() < 0.65 else hap2
        p = rng.randrange(0, int(0.6 * n) - 100)
        seqs.append(mutate(rng, hap[p:p + 100], 0.003))
    start = int(0.6 * n) - 100
    seqs += [hap1[start:], hap2[start:]]
    return k, [seqs]


def test_1e5_kmers_with_ties_and_grid():
    k, cols = big_graph()
    known = None
    for grid in (0, 1, 3):
        g = load(k, 1, cols, cap=1 << 19)
        g.configure("grid", grid)
        known = known or expect(g, k, 1, (-1, -1, -1), 100, 1)  # (the same graph each time: one restatement run)
        st, exp = check(g, k, 1, known=known)
        assert st["nkmers_before"] > 90000
        if grid == 0:  # `unitigs` of the popped graph
            assert g.unitigs("fasta") == U.fasta(exp, k)
        g.close()


def test_table_at_95_percent_load():
    k = 31
    probe = mcx.Graph(k, 1, 1 << 14)
    slots = probe.capacity()[0] * 32 // 33
    probe.close()
    rng = random.Random(35)
    genome = rseq(rng, int(slots * 0.93) + k - 1)
    seqs = [genome[i:i + 80 + k] for i in range(0, len(genome) - k, 80)]
    extra = int(slots * 0.02) // k
    for i in range(extra):  # SNP copies of some windows: k more k-mers each
        w = seqs[(i * 7) % len(seqs)]
        m = len(w) // 2
        seqs.append(w[:m] + rng.choice([b for b in "ACGT" if b != w[m]]) + w[m + 1:])
    seqs += seqs[:len(seqs) // 2]
    g = load(k, 1, [seqs], cap=1 << 14)
    assert g.nkmers >= 0.94 * slots
    check(g, k, 1, min_pops=10)
    g.close()


def test_saturated_coverage():
    # sums of a branch's coverage pass 2^32: the means must be taken from 64-bit sums
    rng = random.Random(9)
    k, ncols = 21, 2
    cols = planted(rng, k, ncols, 900, 80, 70, 0.003)
    g = load(k, ncols, cols)
    body = bytearray(g.export(True))
    g.close()
    rs = 8 + 5 * ncols
    for i in range(0, len(body), rs):
        cv = np.frombuffer(bytes(body[i + 8:i + 16]), dtype=np.uint32).astype(np.uint64)
        body[i + 8:i + 16] = np.minimum(cv * np.uint64(2**30), np.uint64(2**32 - 1)).astype(np.uint32).tobytes()
    g = mcx.Graph(k, ncols, 1 << 16)
    g.add_records(bytes(body), ncols, [(0, 0), (1, 1)])
    g.sync()
    graph = R.parse(bytes(body), k, ncols)
    assert max(sum(R.sum_covg(graph, kk) for kk, _ in u) for u in R.unitigs(graph, k)) >= 2**33
    check(g, k, ncols)
    g.close()


def test_decomposition_reused_and_rebuilt():
    rng = random.Random(23)
    k = 31
    cols = planted(rng, k, 1, 3000, 300, 100, 0.004)
    # after unitig_stats(): the kept decomposition is used
    g = load(k, 1, cols)
    g.unitig_stats()
    check(g, k, 1)
    # a second pop of the popped graph (tombstones in the table; the decomposition was dropped by the prune)
    check(g, k, 1, min_pops=0)
    g.close()
    # after a clean: the decomposition is rebuilt for the cleaned graph
    g = load(k, 1, cols)
    g.unitig_stats()
    g.clean(2, 2 * k)
    check(g, k, 1)
    # nothing to pop: the table is left alone
    g2 = load(k, 1, [[rseq(rng, 500)]])
    before = g2.export(True)
    st = g2.pop_bubbles()
    assert st["num_popped"] == 0 and st["nkmers_removed"] == 0 and st["num_pairs"] == 0 and g2.export(True) == before
    g.close()
    g2.close()


def test_refusals():
    g = mcx.Graph(31, 2, 1 << 16)
    g.configure("intersect", 1)
    with pytest.raises(Exception, match="intersect"):
        g.pop_bubbles()
    g.close()
    g = mcx.Graph(31, 1, 1 << 16, nparts=2, part=0)
    with pytest.raises(Exception, match="split over devices"):
        g.pop_bubbles()
    g.close()
    # one-sided edges that would make a branch a fragment of a unitig: refused, the table left as it was
    k, graph, _ = P.fragment_case()
    g, ncols = load_graph(graph, k)
    before = g.export(True)
    with pytest.raises(Exception, match="inside a unitig"):
        g.pop_bubbles()
    assert g.export(True) == before
    g.close()


def test_empty_graph():
    g = mcx.Graph(31, 1, 1 << 16)
    st = g.pop_bubbles()
    assert st == dict(num_popped=0, num_pairs=0, nkmers_before=0, nkmers_removed=0, num_unitigs_removed=0, rounds=0)
    g.close()

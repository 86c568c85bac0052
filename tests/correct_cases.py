"""The random case of the `correct` tests, built on the CPU and shared by test_correct_restate.py (which asserts that it
reaches every rule) and test_gpu_correct.py (which runs it on the device).

A 3 kb random genome carries a planted tandem repeat.  Around it:
  * a second haplotype with three SNPs (bubbles): in three colours it is not in the sample, so a walk's fork at a bubble
    is resolved by colour; in one colour the fork stops the walk;
  * three stretches of the genome that only a colour outside the sample holds (three colours): a walk into one makes
    POPFWD steps, which stop a gap walk and which an end extension takes;
  * three branches that leave the genome (a shared prefix, then their own sequence): a read with an error on the first
    base behind the branch point is bridged by the backward walk only;
  * two pairs of sequences that share exactly one k-mer: a gap over it stops both one-way walks at that k-mer's forks
    and is bridged by the two-way walkers, which meet there;
  * a circular component of period 3: an extension into it goes round until the third entry of a node;
  * three edges cleared between neighbouring k-mers, and three k-mers removed with the edges to them left behind.
The reads: about 400 of 40 to 200 bases (longer where k needs it) from both strands with substitutions, 1-3 base
indels, Ns and soft-clipped random ends, then reads aimed at each structure, reads with a 30-base insertion or
deletion (gaps too short, too long), three reads of 600 bases that a small "reads_chunk" cuts into pieces, reads
shorter than k, empty reads and reads that share nothing with the graph."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_restate as X  # noqa: E402
import reads_restate as S  # noqa: E402

KS = (11, 31, 33, 63, 65, 95, 97, 127)
# what every configuration reaches at least three times (stats of the restatement, one-way) ...
COMMON = ("num_perfect", "num_no_kmers", "gaps_filled", "gaps_filled_backward", "gaps_too_short", "gaps_too_long_or_stopped",
          "stops_fork", "stops_repeat", "missing_edges", "end_gaps_extended", "bases_filled")
# ... and what only a graph with a colour outside the sample can (three colours, the sample in colour 1)
COLOURED = ("stops_colour",)
COLOURED_EVENTS = ("fork_by_colour", "popfwd_in_extension")


def rseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def mutate(rng, s, nsub=0, indel=0, n_at=False):
    """substitutions, one indel of |indel| bases (> 0: insertion) and an N, away from the ends"""
    s = list(s)
    for _ in range(nsub):
        p = rng.randrange(len(s))
        s[p] = rng.choice([c for c in "ACGT" if c != s[p].upper()])
    if indel and len(s) > 20:
        p = rng.randrange(8, len(s) - 8)
        if indel > 0:
            s[p:p] = list(rseq(rng, indel))
        else:
            del s[p:p - indel]
    if n_at:
        s[rng.randrange(len(s))] = "N"
    return "".join(s)


@functools.lru_cache(maxsize=None)
def case(k, ncols):
    """(graph, colour, reads, quals, aimed): aimed names the index ranges of the reads aimed at a structure"""
    assert ncols in (1, 3)
    rng = random.Random(4200 + 10 * k + ncols)
    sample = 1 if ncols == 3 else 0
    unit = "ACCTGAT"
    gen = rseq(rng, 1300) + unit * (k // 7 + 6) + rseq(rng, 1700)
    hap = list(gen)
    for p in (700, 1600 + k, 2400 + k):
        hap[p] = "ACGT"[("ACGT".index(hap[p]) + 1) % 4]
    hap = "".join(hap)
    pops = [(1000, 1030), (2000 + k, 2030 + k), (2700 + k, 2730 + k)]  # the genome's [a, b) outside the sample
    forks = (400, 1800 + k, 2900 + k)
    branches = [gen[p - 100 - k:p] + rseq(rng, 60 + k) for p in forks]
    shared = []
    for _ in range(2):
        m = rseq(rng, k)
        shared.append([rseq(rng, 60 + k) + m + rseq(rng, 60 + k) for _ in range(2)])
    cyc = "ACG" * ((2 * k + 60) // 3)
    inside = [gen] + branches + [s for pair in shared for s in pair] + [cyc]
    if ncols == 1:
        cols = [inside + [hap]]
    else:
        pieces, at = [], 0
        for a, b in pops:
            pieces.append(gen[at:a])
            at = b
        pieces.append(gen[at:])
        cols = [[gen, hap], pieces + inside[1:], [rseq(rng, 300), gen[100:500]]]
    graph = R.build(cols, k)
    graph = {key: (cv, list(ed)) for key, (cv, ed) in graph.items()}
    # three cleared edges and three removed k-mers, away from the other structures
    occ = {p: (key, o) for p, key, o in X.V.oriented_kmers(k, gen)}
    for p in (150, 1150, 2250 + k):
        (ka, oa), (kb, ob) = occ[p], occ[p + 1]
        for c in range(ncols):
            graph[ka][1][c] &= ~(1 << (4 * oa + S.CODE[gen[p + k]])) & 0xff
            graph[kb][1][c] &= ~(1 << (4 * (1 - ob) + 3 - S.CODE[gen[p]])) & 0xff
    for p in (250, 1500 + k, 2550 + k):
        del graph[occ[p][0]]
    view = X.View(graph, k, sample)

    def junk(n):
        for _ in range(10000):
            s = rseq(rng, n)
            if not any(x in graph for x in S.read_kmers(k, s)):
                return s
        raise AssertionError("no junk found")

    reads, aimed = [], {}
    hi = max(200, 3 * k + 20)
    for i in range(400):
        n = rng.randrange(max(40, 2 * k + 10) if i % 3 else 40, hi)  # (a gap is bridged between two aligned k-mers)
        q = rng.randrange(0, len(gen) - n)
        s = mutate(rng, gen[q:q + n], nsub=rng.choice((0, 1, 1, 2, 3)), indel=rng.choice((0, 0, 0, 1, 2, 3, -1, -2, -3)), n_at=i % 9 == 0)
        if i % 6 == 0:
            s = rseq(rng, rng.randrange(5, 20)) + s
        if i % 10 == 0:
            s = s + rseq(rng, rng.randrange(5, 20))
        if i % 7 == 0:
            s = s.lower()
        reads.append(rc(s) if i % 2 else s)

    def aim(name, seqs):
        aimed[name] = (len(reads), len(reads) + len(seqs))
        reads.extend(seqs)

    def sub_at(s, p):
        return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]

    # an error on the first base behind a branch point, read along the genome and along the branch
    aim("branch", [sub_at(src[at - k - 20:at + k + 25], k + 20)
                   for p, br in zip(forks, branches) for src, at in ((gen, p), (br, 100 + k))])
    # a gap over the one k-mer that two sequences share
    aim("shared", [sub_at(s[40:80 + 3 * k], 20 + k + k // 2 + j) for pair in shared for j, s in enumerate(pair)])
    # into the circle: the extension stops at the third entry of a node
    aim("circle", [cyc[j:j + k + 12] + junk(15) for j in range(3)] + [junk(15) + cyc[j:j + k + 12] for j in range(3)])
    # across and into the stretches outside the sample
    aim("pop", [gen[a - k - 20:b + k + 20] for a, b in pops] + [gen[a - k - 25:a + 8] for a, b in pops]
        + [rc(gen[b - 8:b + k + 25]) for a, b in pops])
    # across the bubbles, with an error before each
    aim("bubble", [sub_at(gen[p - 2 * k - 10:p + k + 30], k // 2 + 3) for p in (700, 1600 + k, 2400 + k)])
    # two bases too many and two too few, between flanks that align
    aim("indel", [gen[q:q + k + 6] + "AC" + gen[q + k + 6:q + 2 * k + 12] for q in (420, 450, 720)]
        + [gen[q:q + k + 6] + gen[q + k + 8:q + 2 * k + 14] for q in (430, 460, 740)])
    # thirty bases too many and thirty too few
    aim("insert30", [gen[q:q + k + 20] + junk(30) + gen[q + k + 20:q + 2 * k + 45] for q in (300, 1200 + k, 2150 + k)])
    aim("delete30", [gen[q:q + k + 20] + gen[q + k + 50:q + 2 * k + 75] for q in (500, 1400 + k, 2300 + k)])
    # across the cleared edges and the removed k-mers, with no other error
    aim("edge", [gen[p - 20:p + k + 25] for p in (150, 1150, 2250 + k)] + [rc(gen[p - 10:p + k + 15]) for p in (150, 1150, 2250 + k)])
    aim("absent", [gen[p - 20:p + k + 25] for p in (250, 1500 + k, 2550 + k)])
    # reads that a chunk of 256 bytes cuts: errors every hundred bases or so, one of them over a seam
    aim("long", [mutate(rng, sub_at(sub_at(gen[q:q + 600], 250), 255 + k), nsub=4) for q in (50, 1100, 2200)])
    aim("short", [gen[60:60 + k - 1], "", junk(k + 9), "N" * (k + 3), gen[900:900 + k], ""])
    quals = ["".join(chr(33 + (7 * i + j) % 60) for j in range(len(s))) for i, s in enumerate(reads)]
    return graph, sample, tuple(reads), tuple(quals), aimed


@functools.lru_cache(maxsize=None)
def expected(k, ncols, two_way=False, D=0.1, d=5.0):
    """the restatement over the case, computed once: (node lists, stats without bases_filled, events)"""
    graph, colour, reads, quals, aimed = case(k, ncols)
    view = X.View(graph, k, colour)
    stats = X.new_stats()
    nodes = [X.correct_nodes(view, s, two_way, D, d, stats) for s in reads]
    return nodes, stats, dict(view.events)


def records(k, ncols, with_quals, two_way=False, D=0.1, d=5.0, fq_zero="."):
    """(bytes, out_off, stats) as mcx_graph_correct gives them"""
    graph, colour, reads, quals, aimed = case(k, ncols)
    nodes, stats, _ = expected(k, ncols, two_way, D, d)
    stats = dict(stats)
    parts, off = [], [0]
    for i, s in enumerate(reads):
        seq, q = X.render(k, s, quals[i] if with_quals else "", nodes[i], fq_zero, stats)
        parts.append(seq + q)
        off.append(off[-1] + len(seq) + len(q))
    return "".join(parts).encode(), off, stats


def check_reach(k, ncols):
    """the case reaches every rule at least three times (and says so by name when it does not)"""
    graph, colour, reads, quals, aimed = case(k, ncols)
    nodes, stats, events = expected(k, ncols)
    _, _, stats = records(k, ncols, False)
    for name in COMMON + (COLOURED if ncols == 3 else ()):
        assert stats[name] >= 3, (k, ncols, name, stats)
    for name in ("absent_edge",) + (COLOURED_EVENTS if ncols == 3 else ()):
        assert events.get(name, 0) >= 3, (k, ncols, name, events)
    lens = [sum(len(S_) for S_ in (X.render(k, s, "", n)[0],)) - len(s) for s, n in zip(reads, nodes)]
    assert sum(x > 0 for x in lens) >= 3 and sum(x < 0 for x in lens) >= 3, "indels that change the length"
    two, _, _ = expected(k, ncols, True)
    assert sum(a != b for a, b in zip(nodes, two)) >= 3, "two-way against one-way"
    assert sum(len(s) < k for s in reads) >= 3 and sum(s == "" for s in reads) >= 2
    return stats, events

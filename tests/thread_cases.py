"""The random case of the `thread` tests, built on the CPU and shared by test_thread_restate.py (which asserts that it
reaches every rule) and test_gpu_thread.py (which runs it on the device).  One colour.

A 2 kb random genome with a stretch that occurs three times (repeats: nodes with two ways in and two ways out), a second
haplotype with six SNPs (bubbles), three branches that leave the genome and three that join it, three places where a
branch leaves at one k-mer and another joins at the next (the step back), and three edges cleared between neighbouring
k-mers.  Beside it a "comb": two backbones that share their first 48 out-branches (one every third
base, each a junction) and four in-branches at their start, and then part, so the links of the two on the comb's first
k-mers agree on 48 junction bases and differ behind them: past the first packed word of 32.
The reads: about 200 of 100 to 600 bases (longer where k needs it) from both strands, half of them with one to three
substitutions; reads aimed at the cleared edges; reads with thirty bases too many (a gap that fails); reads that hold
one stretch twice with junk between (the same links twice by one read); reads over an out-branch alone (junctions of
one kind); three reads of 600 bases with an error over base 250, which a "reads_chunk" of 256 cuts at a seam; two reads
over each backbone of the comb; a read shorter than k, an empty one and one that shares nothing with the graph."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_cases as CC  # noqa: E402
import correct_restate as C  # noqa: E402
import reads_restate as S  # noqa: E402
import thread_restate as T  # noqa: E402

KS = (11, 31, 33, 63, 65, 95, 97, 127)
REACH = ("junction_in_filled_gap", "ended_by_missing_edge", "ended_by_failed_gap", "step_back", "reverse_link", "same_link_twice_by_one_read",
         "one_kind_only")
COMB_SHARED = 48


def other(c, by=1):
    return "ACGT"[("ACGT".index(c) + by) % 4]


@functools.lru_cache(maxsize=None)
def case(k):
    """(graph, reads, aimed): aimed names the index ranges of the reads aimed at a structure"""
    rng = random.Random(7700 + k)
    rep = CC.rseq(rng, k + 25)
    gen = CC.rseq(rng, 500) + rep + CC.rseq(rng, 450) + rep + CC.rseq(rng, 450) + rep + CC.rseq(rng, 500)
    hap = list(gen)
    snps = [p for p in (150, 380, 800 + k, 1300 + 2 * k, 1650 + 3 * k, 1900 + 3 * k)]
    for p in snps:
        hap[p] = other(hap[p])
    hap = "".join(hap)
    outs = [gen[p - k - 40:p] + CC.rseq(rng, k + 30) for p in (300, 1000 + k, 1500 + 2 * k)]
    ins = [CC.rseq(rng, k + 30) + gen[p:p + k + 40] for p in (250, 900 + k, 1450 + 2 * k)]
    # an out-branch at a k-mer and an in-branch at the next: the step back of _juncs_to_paths:217
    for p in (420, 700 + k, 1200 + 2 * k):
        outs.append(gen[p - 40:p + k] + other(gen[p + k]) + CC.rseq(rng, k + 30))
        ins.append(CC.rseq(rng, k + 30) + other(gen[p]) + gen[p + 1:p + k + 41])
    # the comb: backbone sites every third base; out-branch i leaves behind base site(i)
    nsite = COMB_SHARED + 24
    blen = 3 * nsite + 2 * k + 40
    b1 = CC.rseq(rng, blen)
    part = k + 12 + 3 * COMB_SHARED  # the two backbones part here
    b2 = b1[:part] + other(b1[part], 2) + CC.rseq(rng, blen - part - 1)
    comb = [b1, b2]
    for b in (b1, b2):
        for i in range(nsite):
            p = k + 12 + 3 * i
            if b is b2 and p <= part:
                continue
            comb.append(b[p - k:p] + other(b[p]) + CC.rseq(rng, k))
    for i in range(4):
        p = 1 + 3 * i
        comb.append(CC.rseq(rng, k) + other(b1[p - 1]) + b1[p:p + k])
    graph = R.build([[gen, hap] + outs + ins + comb], k)
    graph = {key: (cv, list(ed)) for key, (cv, ed) in graph.items()}
    occ = {p: (key, o) for p, key, o in C.V.oriented_kmers(k, gen)}
    cleared = (100, 700 + k, 1800 + 3 * k)
    for p in cleared:
        (ka, oa), (kb, ob) = occ[p], occ[p + 1]
        graph[ka][1][0] &= ~(1 << (4 * oa + S.CODE[gen[p + k]])) & 0xff
        graph[kb][1][0] &= ~(1 << (4 * (1 - ob) + 3 - S.CODE[gen[p]])) & 0xff

    def junk(n):
        for _ in range(10000):
            s = CC.rseq(rng, n)
            if not any(x in graph for x in S.read_kmers(k, s)):
                return s
        raise AssertionError("no junk found")

    reads, aimed = [], {}
    lo = max(100, 2 * k + 20)
    for i in range(200):
        n = rng.randrange(lo, 600)
        src = hap if i % 5 == 0 else gen
        q = rng.randrange(0, len(src) - n)
        s = CC.mutate(rng, src[q:q + n], nsub=rng.choice((0, 1, 2, 3)) if i % 2 else 0)
        if i % 11 == 0:
            s = s.lower()
        reads.append(CC.rc(s) if i % 3 == 0 else s)

    def aim(name, seqs):
        aimed[name] = (len(reads), len(reads) + len(seqs))
        reads.extend(seqs)

    def sub_at(s, p):
        return s[:p] + other(s[p]) + s[p + 1:]

    aim("edge", [gen[max(0, p - 80):p + k + 150] for p in cleared] + [CC.rc(gen[max(0, p - 60):p + k + 120]) for p in cleared])
    aim("insert30", [gen[q:q + k + 60] + junk(30) + gen[q + k + 60:q + 2 * k + 140] for q in (230, 860 + k, 1400 + 2 * k)])
    # (each stretch holds a place where a branch joins and, behind it, one where a branch leaves)
    twice = [gen[q:q + k + 130] + junk(30) + gen[q:q + k + 130] for q in (235, 890 + k, 1440 + 2 * k)]
    aim("twice", twice + [CC.rc(s) for s in twice])
    aim("one_kind", [o[20:k + 40 + 25] for o in outs] + [sub_at(o[20:k + 40 + k + 25], k + 21 + k // 2 + 1) for o in outs])
    aim("branch", [sub_at(o, k + 41) for o in outs] + [sub_at(i_, k + 28) for i_ in ins] + outs + ins)
    aim("long", [CC.mutate(rng, sub_at(sub_at(gen[q:q + 600], 250), 255 + k), nsub=2) for q in (50, 700, 1300)])
    aim("comb", [b1, b2, CC.rc(b1), b2[:part + k + 20]])
    aim("short", [gen[60:60 + k - 1], "", junk(k + 9)])
    return graph, tuple(reads), aimed


@functools.lru_cache(maxsize=None)
def view(k):
    """one view of the case's graph for every restatement run over it"""
    return C.View(case(k)[0], k, 0)


def store(k, max_juncs=0):
    return T.Store(case(k)[0], k, max_juncs, view(k))


@functools.lru_cache(maxsize=None)
def expected(k, two_way=False, max_juncs=0):
    """the restatement over the case, computed once"""
    return store(k, max_juncs).thread(case(k)[1], two_way)


def check_reach(k):
    """the case reaches every rule at least three times (and says so by name when it does not)"""
    graph, reads, aimed = case(k)
    st = expected(k)
    for name in REACH:
        assert st.events[name] >= 3, (k, name, dict(st.events))
    assert st.prefix_pairs() >= 3, (k, "prefix pairs", st.prefix_pairs())
    assert st.stats["gaps_filled"] >= 3 and st.stats["gaps_filled_backward"] >= 1, st.stats
    # the comb: a contig with more than 64 junctions, and two links that agree on 40 bases and differ later
    lo, hi = aimed["comb"]
    nodes = T.contigs(view(k), reads[lo])
    assert len(nodes) == 1 and len(T.junctions(view(k), nodes[0])[0]) > 64
    far = 0
    for key, links in st.by_kmer():
        for a, b in zip(links, links[1:]):
            if a[0] == b[0] and min(len(a[1]), len(b[1])) > 40 and a[1][:40] == b[1][:40] and a[1] != b[1] \
                    and a[1][:min(len(a[1]), len(b[1]))] != b[1][:min(len(a[1]), len(b[1]))]:
                far += 1
    assert far >= 1, (k, "links that differ behind 40 junctions")
    two = expected(k, True)
    assert two.links != st.links or two.stats != st.stats, "two-way against one-way"
    assert len(st.text()) < 4 << 20
    return st

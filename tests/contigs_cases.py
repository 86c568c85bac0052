"""The cases of the `contigs` tests, built on the CPU and shared by test_contigs_restate.py (which asserts that they
reach every status and every stop cause) and test_gpu_contigs.py (which runs them on the device).  Small graphs at
k = 5, 9, 31 and 33 from a few sequences each; the links are those `thread` makes of reads (thread_restate.py) or are put
down by hand where a case needs links that no read makes.  tests/golden/contigs.json pins these by name.  wide_cases() is
the same structures at k = 63, 65, 95, 97 and 127 (keys of two, three and four words, the top word full or holding two
bits), which no golden pins: there the device is compared with the restatement alone.

Structures (upper-case names are random stretches without a repeated k-mer):
  repeat   U1 R U2 R U3: R is entered two ways and left two ways.  The reads U1 R U2 and U2 R U3 give the link that
           takes a walk from U1 through R (USELINKS; it has one junction and finishes exactly at the fork) and the counter
           link that answers the missing-information check.
  merge    X1 CORE Y1, X2 CORE Y2, X2 CORE[:k-1] Z and W CORE[mid:]: CORE is entered three ways (the third in its middle)
           and left two ways; the last k-mer P before CORE on the X2 side has two successors, so its links are counter links
           filtered by the base of the step.
  circle   a circular sequence: no fork, the walk goes round twice and stops at the third entry.
  tandem   U1 X X X U2: a loop walked with a link that holds one junction per round.
  rho      two colours: a tail into a loop that the sample cannot leave; a link held on the first rounds is used up and
           the walk is stopped when it enters the loop again in the state it had the round before.
  colours  two colours: a fork of which one branch is in the sample, a tail that only the other colour has, and an end
           where the population forks and the sample has neither branch."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import contigs_restate as G  # noqa: E402
import thread_restate as T  # noqa: E402

KS = (5, 9, 31, 33)
WIDE_KS = (63, 65, 95, 97, 127)  # a full and a 2-bit top word at keys of two, three and four words


def other(c, by=1):
    return "ACGT"[("ACGT".index(c) + by) % 4]


def node_at(seq, i, k):
    x = R.kmer_int(seq[i:i + k])
    key = R.canon(x, k)
    return (key, 0 if key == x else 1)


def unique(seqs, k):
    """no canonical k-mer twice over the sequences"""
    seen = set()
    for s in seqs:
        for i in range(len(s) - k + 1):
            key = node_at(s, i, k)[0]
            if key in seen:
                return False
            seen.add(key)
    return True


def pieces(k, lens, salt, ok=lambda p: True):
    """random stretches of the given lengths that share no k-mer (also not with their reverse complements)"""
    for attempt in range(20000):
        rng = random.Random(1000 * salt + 17 * k + attempt)
        p = ["".join(rng.choice("ACGT") for _ in range(n)) for n in lens]
        if unique(["".join(p)], k) and ok(p):
            return p
    raise AssertionError("no pieces for k=%d salt=%d" % (k, salt))


def threaded(graph, k, reads):
    """the links `thread` makes of the reads over the one-colour graph: ([(key, orient, bases, nseen)], contig histogram)"""
    st = T.Store(graph, k).thread(reads)
    return [(key, o, b, n) for (key, o, b), n in st.links.items()], dict(st.contig_hist())


def mk(name, k, graph, links, hist=None, ncols=1, **params):
    conf = G.conf_table(hist or {}, len(graph))
    return {"name": "%s_k%d" % (name, k), "k": k, "ncols": ncols, "graph": graph, "links": links, "conf": conf, "params": params}


def repeat_genome(k, salt=1):
    u = 2 * k + 6 if k > 9 else k + 6

    def ok(p):
        return p[1][0] != p[2][0] and p[0][-1] != p[1][-1]
    u1, u2, u3, rep = pieces(k, (u, u, u, k + 3), salt, ok)
    return u1, rep, u2, u3


def merge_seqs(k, salt=2):
    u = 2 * k + 4 if k > 9 else k + 5

    def ok(p):
        x1, x2, core, y1, y2, z, w = p
        mid = len(core) // 2
        return y1[0] != y2[0] and z[0] != core[k - 1] and x1[-1] != x2[-1] and w[-1] != core[mid - 1]
    return pieces(k, (u, u, 2 * k + 8, u, u, k + 3, k + 4), salt, ok)


@functools.lru_cache(maxsize=None)
def cases(ks=KS):
    out = []
    for k in ks:
        # ---- repeat ----
        u1, rep, u2, u3 = repeat_genome(k)
        genome = u1 + rep + u2 + rep + u3
        graph = R.build([[genome]], k)
        reads = [u1 + rep + u2, u2 + rep + u3]
        links, hist = threaded(graph, k, reads)
        out.append(mk("repeat", k, graph, links, hist))
        out.append(mk("repeat_reseed", k, graph, links, hist, flags=G.RESEED, ncontigs=7))
        out.append(mk("repeat_limit", k, graph, links, hist, ncontigs=2))
        out.append(mk("repeat_low_step", k, graph, links, hist, min_step=2.0))
        out.append(mk("repeat_low_cumul", k, graph, links, hist, min_cumul=2.0))
        out.append(mk("repeat_no_links", k, graph, [], hist))
        # one read only: nothing answers for the other branch
        links1, hist1 = threaded(graph, k, reads[:1])
        out.append(mk("repeat_missing", k, graph, links1, hist1))
        out.append(mk("repeat_missing_off", k, graph, links1, hist1, flags=G.NO_MISSING_CHECK))
        # by hand: two links of one age on the last node of U1 that disagree; a link that names a base the fork has not
        n = node_at(genome, len(u1) - 1, k)
        split = [(n[0], n[1], (R.kmer_int(u2[0]),), 1), (n[0], n[1], (R.kmer_int(u3[0]),), 1)]
        out.append(mk("repeat_split", k, graph, split, hist))
        bad = next(b for b in range(4) if "ACGT"[b] not in (u2[0], u3[0]))
        out.append(mk("repeat_corrupt", k, graph, [(n[0], n[1], (bad,), 1)], hist))
        # ---- merge ----
        x1, x2, core, y1, y2, z, w = merge_seqs(k)
        mid = len(core) // 2
        seqs = [x1 + core + y1, x2 + core + y2, x2 + core[:k - 1] + z, w + core[mid:]]
        graph = R.build([seqs], k)
        links, hist = threaded(graph, k, seqs)
        out.append(mk("merge", k, graph, links, hist))
        out.append(mk("merge_no_check", k, graph, links, hist, flags=G.NO_MISSING_CHECK))
        # by hand: an old link on the last node of X1 for Y1, a younger one inside CORE (before its middle) for Y2; the
        # seeds j (in X1), i (in CORE), l (in Y2), i again, and a k-mer that is no key
        a = node_at(seqs[0], len(x1) - 1, k)
        c = node_at(seqs[0], len(x1) + 2, k)
        hand = [(a[0], a[1], (R.kmer_int(y1[0]),), 1), (c[0], c[1], (R.kmer_int(y2[0]),), 1)]
        fw = lambda s, i: T.kmer_str(node_at(s, i, k)[0], k)  # noqa: E731
        sj, si, sl = fw(seqs[0], 2), fw(seqs[0], len(x1) + 1), fw(seqs[1], len(x2) + len(core) + 2)
        nokey = next(s for s in ("A" * k, "C" * (k - 1) + "A", "AC" * (k // 2) + "A") if R.canon(R.kmer_int(s), k) not in graph)
        out.append(mk("merge_chain", k, graph, hand, hist, flags=G.NO_MISSING_CHECK, seeds=[sj, si, sl, si, nokey, sj]))
        out.append(mk("merge_chain_reseed", k, graph, hand, hist, flags=G.NO_MISSING_CHECK | G.RESEED, seeds=[sj, si, sl, si, nokey]))
        out.append(mk("merge_chain_limit", k, graph, hand, hist, flags=G.NO_MISSING_CHECK, seeds=[sj, si, sl, si], ncontigs=1))
        # a counter link on P whose first base is not the step's: the filter drops it (unfiltered it would be corrupt)
        p = node_at(seqs[1], len(x2) - 1, k)
        out.append(mk("merge_filtered", k, graph, links + [(p[0], p[1], (R.kmer_int(z[0]), R.kmer_int(other(y1[0], 2) if other(y1[0], 2) != y2[0] else other(y1[0], 3))), 1)],
                      hist))
        # ---- circle ----
        (circ,) = pieces(k, (3 * k + 7 if k <= 9 else k + 9,), 3, lambda q: unique([q[0] + q[0][:k - 1]], k))
        graph = R.build([[circ + circ[:k]]], k)
        out.append(mk("circle", k, graph, [], {}))
        # ---- tandem ----
        def ok_t(q):
            return q[1][0] != q[2][0]
        t1, x, t2 = pieces(k, (k + 6, k + 4, k + 6), 4, ok_t)
        tand = t1 + x * 3 + t2
        graph = R.build([[tand]], k)
        links, hist = threaded(graph, k, [tand])
        out.append(mk("tandem", k, graph, links, hist))
        # ---- colours ----
        def ok_c(q):
            m, alt, tail, e1, e2 = q
            half = len(m) // 2
            return alt[0] != m[half] and e1[0] != e2[0]
        m, alt, tail, e1, e2 = pieces(k, (3 * k + 8, k + 4, k + 3, k + 2, k + 2), 5, ok_c)
        half = len(m) // 2
        graph = R.build([[m], [m[:half] + alt, m + tail + e1, m + tail + e2]], k)
        g0 = R.build([[m]], k)
        links, hist = threaded(g0, k, [m])
        out.append(mk("colours", k, graph, links, hist, ncols=2))
        out.append(mk("colours_c1", k, graph, [], hist, ncols=2, colour=1))
        # ---- rho ----
        # a tail into a loop whose only way out is in the other colour: the fork F is POPFRK_COLFWD every round.  By hand a
        # link of two junctions on the last node of the tail: it advances at F on the first two rounds and is used up.  The
        # node behind F is entered holding the link the first time, with empty lists the second time, and the third entry,
        # in that same state, stops the walk
        def ok_r(q):
            t, c, x = q
            f = len(c) // 2
            return t[-1] != c[-1] and x[0] != c[f + k] and unique([c + c[:k - 1]], k)
        t, c, x = pieces(k, (k + 5, 2 * k + 9, k + 3), 6, ok_r)
        f = len(c) // 2
        sample = t + c + c[:k]
        graph = R.build([[sample], [c[f:f + k] + x]], k)
        n = node_at(sample, len(t) - 1, k)
        b = R.kmer_int(c[f + k])
        seed = T.kmer_str(node_at(sample, 1, k)[0], k)
        out.append(mk("rho", k, graph, [(n[0], n[1], (b, b), 1)], {}, ncols=2, flags=G.NO_MISSING_CHECK, seeds=[seed]))
    return out


def wide_cases():
    """the same structures at WIDE_KS; no golden pins these, the restatement is the oracle"""
    return cases(WIDE_KS)


def run(case):
    """the restatement on a case: (records, sequence bytes, stats)"""
    p = case["params"]
    return G.assemble(case["graph"], case["k"], case["links"], case["conf"], p.get("colour", 0), p.get("flags", 0), p.get("ncontigs", 0), p.get("min_step", -1.0),
                      p.get("min_cumul", -1.0), p.get("seeds"))


def links_text(case):
    """the links of a case as the body of a .ctp (no seq=, no juncpos=)"""
    per = {}
    for key, o, b, n in case["links"]:
        per.setdefault(key, []).append((o, tuple(b), n))
    out = []
    for key in sorted(per):
        out.append("%s %d\n" % (T.kmer_str(key, case["k"]), len(per[key])))
        for o, b, n in sorted(per[key]):
            out.append("%s %d %d %s\n" % ("FR"[o], len(b), n, "".join("ACGT"[x] for x in b)))
    return "".join(out).encode()

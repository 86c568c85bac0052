"""A CPU restatement of `unitigs` (src/commands/ctx_unitigs.c, src/graph/db_unitig.c, src/graph/unitig_graph.c),
written from the reference's semantics as the expectation of the device tests.  The decomposition is
clean_restate.unitigs(); this adds the normalisation (db_unitig_normalise), the numbering and the three writers
under the project's output contract:

  * every unitig is normalised in all three formats: a chain starts at the end with the lower key, a closed
    cycle at its lowest key read forwards, a single k-mer is forward;
  * unitigs are numbered in ascending order of the key of their first k-mer and appear in that order;
  * an edge that leaves a unitig end is printed when the key of the end k-mer is below the neighbour's, or when
    the two are the same k-mer and not both sides are reverse (_print_edge with `node < next` decided by key);
    the lines are sorted by (source unitig, left end before right end, edge base ACGT).

A graph is clean_restate's: {key: (covgs, edges per colour)}; only the union of the edges is used."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402

ACGT = "ACGT"


def nibble(graph, key, o):
    return (R.union_edges(graph, key) >> (4 * o)) & 15


def is_cycle(graph, u, k):
    """the last node's only edge leads to the first node, which has only that edge in"""
    if len(u) < 2:
        return False
    (k0, o0), (k1, o1) = u[0], u[-1]
    nib = nibble(graph, k1, o1)
    if bin(nib).count("1") != 1 or bin(nibble(graph, k0, 1 - o0)).count("1") != 1:
        return False
    return R.step(k1, o1, nib.bit_length() - 1, k) == (k0, o0)


def flip(u):
    return [(kk, 1 - o) for kk, o in reversed(u)]


def normalise(graph, u, k):
    if len(u) == 1:
        return [(u[0][0], 0)]
    if is_cycle(graph, u, k):
        i = min(range(len(u)), key=lambda j: u[j][0])
        if u[i][1] == 1:  # read the other way round, so that the lowest key is forward
            u = flip(u)
            i = len(u) - 1 - i
        return u[i:] + u[:i]
    return u if u[0][0] < u[-1][0] else flip(u)


def unitigs(graph, k):
    """normalised unitigs in the order of their numbers"""
    return sorted((normalise(graph, u, k) for u in R.unitigs(graph, k)), key=lambda u: u[0][0])


def spell(u, k):
    def s(key, o):
        x = key if o == 0 else R.revcomp(key, k)
        return "".join(ACGT[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))
    return s(*u[0]) + "".join(s(kk, o)[-1] for kk, o in u[1:])


def letters(nib):
    return "".join(ACGT[x] for x in range(4) if (nib >> x) & 1)


def prev_next(graph, u):
    (k0, o0), (k1, o1) = u[0], u[-1]
    back = nibble(graph, k0, 1 - o0)
    prev = sum(1 << (3 - x) for x in range(4) if (back >> x) & 1)  # rev_nibble_lookup
    return letters(prev), letters(nibble(graph, k1, o1))


def links(graph, us, k, rule=True):
    """[(unitig, reverse?, unitig, reverse?)] in output order; rule=False: every edge that leaves an end, from both sides"""
    where = {}
    for i, u in enumerate(us):
        for r, (kk, o) in enumerate(u):
            where[kk] = (i, r, o)
    out = []
    for i, u in enumerate(us):
        for side in (0, 1):  # the left end leaves backwards, the right end forwards
            key, o = (u[0][0], 1 - u[0][1]) if side == 0 else u[-1]
            nib = nibble(graph, key, o)
            for x in range(4):
                if not (nib >> x) & 1:
                    continue
                nk, no = R.step(key, o, x, k)
                if nk not in graph:
                    continue
                j, r, oj = where[nk]
                rev0, rev1 = 1 - side, 0 if (r == 0 and no == oj) else 1
                if not rule or key < nk or (key == nk and not (rev0 and rev1)):
                    out.append((i, rev0, j, rev1))
    return out


def fasta(graph, k):
    parts = []
    for i, u in enumerate(unitigs(graph, k)):
        p, n = prev_next(graph, u)
        parts.append(">unitig%d prev=%s next=%s\n%s\n" % (i, p, n, spell(u, k)))
    return "".join(parts).encode()


def gfa(graph, k):
    us = unitigs(graph, k)
    parts = ["H\tVN:Z:1.0\n"]
    parts += ["S\tnode%d\t%s\n" % (i, spell(u, k)) for i, u in enumerate(us)]
    parts += ["L\tnode%d\t%s\tnode%d\t%s\t%dM\n" % (i, "+-"[a], j, "+-"[b], k - 1) for i, a, j, b in links(graph, us, k)]
    return "".join(parts).encode()


def dot(graph, k, points=False):
    us = unitigs(graph, k)
    parts = ["digraph G {\n", "  edge [dir=both arrowhead=none arrowtail=none color=\"blue\"]\n",
             "  node [%s, fontname=courier, fontsize=9]\n" % ("shape=point, label=none" if points else "shape=none")]
    parts += ["  node%d [label=%s]\n" % (i, spell(u, k)) for i, u in enumerate(us)]
    parts.append("\n")
    parts += ["  node%d:%s -> node%d:%s\n" % (i, "ew"[a], j, "we"[b]) for i, a, j, b in links(graph, us, k)]
    parts.append("}\n")
    return "".join(parts).encode()


def text(graph, k, fmt, points=False):
    return {"fasta": fasta, "gfa": gfa}[fmt](graph, k) if fmt != "dot" else dot(graph, k, points)

"""Pure-Python restatement of `mccortex<K> correct` without link files (src/commands/ctx_correct.c,
src/alignment/db_alignment.c, src/alignment/correct_alignment.c, src/tools/correct_reads.c, src/graph/graph_walker.c,
src/graph/repeat_walker.h), with no device involved.  graph = {canonical key: (covgs, edges)}.

1. Graph view (ctx_correct.c:116-121, 187): every key is walked, a k-mer's edges are the OR of its edge bytes over the
   colours, and a k-mer is in the sample iff its coverage or its edge byte in colour `colour` is non-zero.
2. Alignment (db_alignment_from_read:50-78): the k-mers of the maximal ACGTacgt runs of at least k bases; one aligns iff
   it is a key and in the sample.  r1enderr = len - (last position + k), or len when nothing aligned (:81-82).
3. Segments (db_alignment_next_gap:163-174): aligned k-mers at consecutive positions stay together while the union
   edges of the earlier hold the edge to the later; a missing edge ends the contig with no traversal
   (correct_alignment_nxt:390).  Every boundary between non-consecutive positions is a gap and is attempted once.
4. Walker step (graph_walker_choose:385-433 with no paths): successors over the union edges in nucleotide order; none:
   stop; one: take it, POPFWD if it is not in the sample; several: those in the sample, exactly one: take it, otherwise
   stop.  An edge that names an absent k-mer counts as no edge (the reference asserts there is none).
5. Repeat rule (repeat_walker.h:18-50, graph_walker_hash64 of (node, orient) alone): a walk enters an oriented node at
   most twice, the third entry stops it; the start node is not an entry.  Every walk starts clean: the visited bits the
   reference leaves behind after a POPFWD stop and the false positives of its 22-bit Bloom filter are artefacts of its
   memory layout and are not reproduced.
6. Gap fill (correct_alignment_nxt:402-438, traverse_one_way2, traverse_two_way2:208-236).
7. End extension (correct_aln_read:570-639): POPFWD steps are accepted.  Perfect reads (db_alignment_is_perfect) and
   reads with no aligned k-mer skip 3-7; of a perfect read only the first segment's missing edge is counted
   (correct_alignment_init:81-86).
8. Rendering (handle_read2:106-226, _print_read_kmer).

Stats (mcx_correct_stats): gaps = gaps_filled + gaps_too_short + gaps_too_long_or_stopped, by the walk that decided
the gap (one-way: the backward one when the forward one failed); too short is gap_len < gap_min of that walk
(correct_alignment.c:168, :271).  stops_* count, over every walk of every kind, the reason its last step failed:
fork = several successors and not exactly one in the sample, colour = a POPFWD step inside a gap, repeat = a third
entry.  bases_filled = characters written with fq_zero as their quality."""
import collections
import functools
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import coverage_restate as V  # noqa: E402

STAT_NAMES = ("num_reads", "num_kmers", "num_kmers_found", "num_perfect", "num_no_kmers", "gaps", "gaps_filled",
              "gaps_filled_backward", "gaps_too_short", "gaps_too_long_or_stopped", "stops_fork", "stops_colour",
              "stops_repeat", "missing_edges", "end_gaps", "end_gaps_extended", "bases_filled")
STOP_NONE, STOP_DEAD, STOP_FORK, STOP_COLOUR, STOP_REPEAT = 0, 1, 2, 3, 4


def new_stats():
    return dict.fromkeys(STAT_NAMES, 0)


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def wiggle(est, D, d):
    """(long)(gap_est * gap_variance + gap_wiggle) in float arithmetic (correct_alignment.c:420)"""
    return int(f32(f32(f32(est) * f32(D)) + f32(d)))


def in_sample(graph, key, colour):
    cv, ed = graph[key]
    return cv[colour] != 0 or ed[colour] != 0


@functools.lru_cache(maxsize=1 << 18)
def revcomp(x, k):
    return R.revcomp(x, k)


def rev(node):
    return (node[0], node[1] ^ 1)


def oriented(node, k):
    return node[0] if node[1] == 0 else revcomp(node[0], k)


def last_nuc(node, k):
    return oriented(node, k) & 3


def first_nuc(node, k):
    return (oriented(node, k) >> (2 * (k - 1))) & 3


def step(node, x, k):
    """the node reached from `node` over nucleotide x"""
    s2 = ((oriented(node, k) << 2) | x) & ((1 << (2 * k)) - 1)
    r2 = revcomp(s2, k)
    return (s2, 0) if s2 < r2 else (r2, 1)


class View:
    """the graph as `correct` sees it, with what was worked out for a node kept: the restatement meets the same few
    thousand nodes again and again.  events counts what the stats do not: forks resolved by colour, POPFWD steps taken
    by an end extension, edges that name an absent k-mer (each once per walker step that met it)"""

    def __init__(self, graph, k, colour=0):
        self.graph, self.k, self.colour = graph, k, colour
        self.memo = {}
        self.events = collections.Counter()

    def choose(self, node):
        """(next node or None, POPFWD, stop reason, fork resolved by colour, edges to absent k-mers)"""
        got = self.memo.get(node)
        if got is None:
            got = self.memo[node] = self._choose(node)
        return got

    def _choose(self, node):
        g, k, c = self.graph, self.k, self.colour
        ue = R.union_edges(g, node[0])
        nxt, absent = [], 0
        for x in range(4):
            if (ue >> (4 * node[1] + x)) & 1:
                n = step(node, x, k)
                if n[0] in g:
                    nxt.append(n)
                else:
                    absent += 1
        if not nxt:
            return None, False, STOP_DEAD, False, absent
        if len(nxt) == 1:
            return nxt[0], not in_sample(g, nxt[0][0], c), STOP_NONE, False, absent
        ins = [n for n in nxt if in_sample(g, n[0], c)]
        if len(ins) == 1:
            return ins[0], False, STOP_NONE, True, absent
        return None, False, STOP_FORK, False, absent


def align(view, seq):
    """([(node, position)], k-mer occurrences, occurrences that are keys)"""
    g = view.graph
    occ = V.oriented_kmers(view.k, seq)
    out = [((key, o), p) for p, key, o in occ if key in g and in_sample(g, key, view.colour)]
    return out, len(occ), sum(key in g for _, key, _ in occ)


def has_edge(view, a, b):
    """the union edges of a hold the edge to b (b follows a in the read)"""
    return (R.union_edges(view.graph, a[0]) >> (4 * a[1] + last_nuc(b, view.k))) & 1


class Walker:
    """one GraphWalker with its RepeatWalker: step() moves and says whether the node may be kept"""

    def __init__(self, view, start, only_in_col):
        self.v, self.node, self.only = view, start, only_in_col
        self.path, self.stop = [], STOP_NONE

    def step(self):
        nxt, pop, why, by_colour, absent = self.v.choose(self.node)
        self.v.events["absent_edge"] += absent
        if nxt is None:
            self.stop = why
            return False
        if self.only and pop:
            self.stop = STOP_COLOUR
            return False
        if self.path.count(nxt) >= 2:
            self.stop = STOP_REPEAT
            return False
        self.v.events["fork_by_colour"] += by_colour
        self.v.events["popfwd_in_extension"] += pop
        self.node = nxt
        return True


def count_stop(stats, w):
    if w.stop == STOP_FORK:
        stats["stops_fork"] += 1
    elif w.stop == STOP_COLOUR:
        stats["stops_colour"] += 1
    elif w.stop == STOP_REPEAT:
        stats["stops_repeat"] += 1


def walk_to(view, start, end, gap_min, gap_max, stats):
    """traverse_one_way2: (traversed, nodes walked)"""
    w = Walker(view, start, True)
    ok = False
    while len(w.path) < gap_max + 1 and w.step():
        if w.node == end:
            ok = True
            break
        w.path.append(w.node)
    count_stop(stats, w)
    if len(w.path) < gap_min:
        ok = False
    return ok, w.path


def walk_two_way(view, a, b, gap_min, gap_max, stats):
    """traverse_two_way2: (traversed, fill nodes in read order, gap_len)"""
    w = [Walker(view, a, True), Walker(view, rev(b), True)]
    use, gap_len, ok = [True, True], 0, False
    while gap_len <= gap_max and (use[0] or use[1]):
        for i in (0, 1):
            if not use[i]:
                continue
            if not w[i].step():
                use[i] = False
                if w[i].stop == STOP_REPEAT:
                    use = [False, False]
                    break
                continue
            if w[0].node == rev(w[1].node):
                ok = gap_len <= gap_max
                use = [False, False]
                break
            w[i].path.append(w[i].node)
            gap_len += 1
    count_stop(stats, w[0])
    count_stop(stats, w[1])
    if gap_len < gap_min:
        ok = False
    return ok, w[0].path + [rev(n) for n in reversed(w[1].path)], gap_len


def extend(view, start, limit, stats):
    w = Walker(view, start, False)
    while len(w.path) < limit and w.step():
        w.path.append(w.node)
    count_stop(stats, w)
    return w.path


def correct_nodes(view, seq, two_way=False, D=0.1, d=5.0, stats=None):
    """correct_aln_read: [(node, position or -1)]"""
    stats = new_stats() if stats is None else stats
    k = view.k
    aln, nocc, nkey = align(view, seq)
    stats["num_reads"] += 1
    stats["num_kmers"] += nocc
    stats["num_kmers_found"] += nkey
    if not aln:
        stats["num_no_kmers"] += 1
        return []
    n = len(aln)
    # the boundary between aln[i - 1] and aln[i]: a gap, a missing edge or none
    bound = [None] * (n + 1)
    for i in range(1, n):
        if aln[i - 1][1] + 1 != aln[i][1]:
            bound[i] = "gap"
        elif not has_edge(view, aln[i - 1][0], aln[i][0]):
            bound[i] = "edge"
    left_gap, right_gap = aln[0][1], len(seq) - (aln[-1][1] + k)
    if "gap" not in bound and left_gap == 0 and right_gap == 0:
        stats["num_perfect"] += 1
        stats["missing_edges"] += "edge" in bound
        return list(aln)
    stats["missing_edges"] += bound.count("edge")
    out = [aln[0]]
    for i in range(1, n):
        if bound[i] == "gap":
            a, b = aln[i - 1][0], aln[i][0]
            est = aln[i][1] - aln[i - 1][1]
            wig = wiggle(est, D, d)
            gap_min, gap_max = max(0, est - wig), max(0, est + wig)
            stats["gaps"] += 1
            if two_way:
                ok, fill, gap_len = walk_two_way(view, a, b, gap_min, gap_max, stats)
            else:
                ok, fill = walk_to(view, a, b, gap_min, gap_max, stats)
                if not ok:
                    ok, back = walk_to(view, rev(b), rev(a), gap_min, gap_max, stats)
                    fill = [rev(x) for x in reversed(back)]
                    stats["gaps_filled_backward"] += ok
                gap_len = len(fill)
            if ok:
                stats["gaps_filled"] += 1
                out += [(x, -1) for x in fill]
            elif gap_len < gap_min:
                stats["gaps_too_short"] += 1
            else:
                stats["gaps_too_long_or_stopped"] += 1
        out.append(aln[i])
    if left_gap > 0:
        stats["end_gaps"] += 1
        path = extend(view, rev(aln[0][0]), left_gap, stats)
        stats["end_gaps_extended"] += bool(path)
        out = [(rev(x), -1) for x in reversed(path)] + out
    if right_gap > 0:
        stats["end_gaps"] += 1
        path = extend(view, aln[-1][0], right_gap, stats)
        stats["end_gaps_extended"] += bool(path)
        out += [(x, -1) for x in path]
    return out


def render(k, seq, qual, nodes, fq_zero=".", stats=None):
    """handle_read2: (sequence, qualities or "")"""
    s, q = [], []
    nfill = [0]

    def read(a, b, up):
        s.append(seq[a:b].upper() if up else seq[a:b].lower())
        q.append(qual[a:b])

    def fill(x):
        s.append("ACGT"[x])
        q.append(fq_zero)
        nfill[0] += 1

    if not nodes:
        read(0, len(seq), False)
        return "".join(s), "".join(q) if qual else ""
    pos = [p for _, p in nodes]
    num = len(nodes)
    neg = 0
    while pos[neg] == -1:
        neg += 1
    read(0, pos[neg] - neg, False)
    for j in range(neg):
        fill(first_nuc(nodes[j][0], k))
    i, printed = neg, pos[neg]
    while i < num:
        j = i
        while j < num and pos[j] < 0:
            j += 1
        neg = j - i
        if neg == 0:
            if pos[i] > printed:
                read(printed, pos[i], False)
                printed = pos[i]
            if pos[i] + k > printed:
                read(printed, pos[i] + k, True)
            printed = pos[i] + k
            i += 1
        elif i + neg == num:
            break
        else:
            exp = pos[i + neg] - pos[i - 1] - 1
            nprint = 0
            if neg >= k:
                nprint = neg - k + 1
            if neg > exp:
                nprint = neg - exp
            for j in range(i, i + nprint):
                fill(last_nuc(nodes[j][0], k))
            nextpos = pos[i + neg]
            if neg < k:
                nextpos += k - neg - 1
            printed = max(printed, nextpos)
            i += neg
    if i < num:
        for j in range(i, num):
            fill(last_nuc(nodes[j][0], k))
        printed += num - i
    read(printed, len(seq), False)
    if stats is not None:
        stats["bases_filled"] += nfill[0]
    return "".join(s), "".join(q) if qual else ""


def correct(graph, k, seq, qual="", colour=0, two_way=False, D=0.1, d=5.0, fq_zero=".", stats=None, view=None):
    """(corrected sequence, its qualities or "" when the read has none)"""
    view = view or View(graph, k, colour)
    nodes = correct_nodes(view, seq, two_way, D, d, stats)
    return render(k, seq, qual, nodes, fq_zero, stats)


def contig_str(k, nodes):
    """db_nodes_to_str of a run of nodes"""
    key, o = nodes[0]
    x = oriented((key, o), k)
    s = "".join("ACGT"[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))
    return s + "".join("ACGT"[last_nuc(n, k)] for n in nodes[1:])


def batch(graph, k, reads, quals=None, colour=0, view=None, **kw):
    """what mcx_graph_correct hands out for a batch: (bytes, out_off, stats); record r is the corrected sequence, then
    as many quality bytes when qualities were given"""
    stats = new_stats()
    view = view or View(graph, k, colour)
    parts, off = [], [0]
    for i, seq in enumerate(reads):
        s, q = correct(graph, k, seq, quals[i] if quals else "", stats=stats, view=view, **kw)
        parts.append(s + q)
        off.append(off[-1] + len(s) + len(q))
    return "".join(parts).encode(), off, stats


def fmt_read(name, seq, qual, orig, fmt, print_orig=False, fq_zero="."):
    """handle_read:245-267"""
    head = name + (" orig=" + orig if print_orig else "")
    if fmt == "fa":
        return ">%s\n%s\n" % (head, seq)
    if fmt == "fq":
        return "@%s\n%s\n+\n%s\n" % (head, seq, qual if qual else fq_zero * len(seq))
    return seq + "\n"

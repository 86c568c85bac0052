"""Pure-Python restatement of `mccortex<K> thread` without `-p` and without `-u` (src/commands/ctx_thread.c,
src/alignment/correct_alignment.c, src/tools/generate_paths.c, src/graph_paths/gpath_hash.c, gpath_save.c, gpath_checks.c),
built on correct_restate.py, with no device involved.  graph = {canonical key: (covgs, edges)} of one colour.

1. Graph view: one colour (ctx_thread.c:178); a k-mer is in the sample iff its value word is non-zero; an edge that
   names an absent k-mer counts as no edge, so a degree counts the edges whose k-mer is a key.
2. Contigs (correct_alignment_init, correct_alignment_nxt:361-510): alignment, segments, gaps and their bounds are those
   of `correct`.  A contig is a run of segments joined by filled gaps with the walked nodes in between; a missing edge
   between consecutive aligned k-mers ends it without a walk, a failed gap ends it and the next starts behind the gap.
   No end extensions.  A perfect read is one contig (per missing edge one more).  Every contig adds nodes + k - 1 to the
   contig histogram.
3. Junctions (worker_contig_to_junctions:326-385): forward at i if i + 1 < N and outdegree(n[i]) > 1, base = last base of
   n[i + 1]; reverse at i if i > 0 and indegree(n[i]) > 1, base = first base of n[i - 1].  Nothing is added unless the
   contig has a junction of each kind.
4. Links (_juncs_to_paths:153-298).  Forward: for every reverse junction at i, in ascending order, s = the first forward
   junction at a position >= i; none: stop (:211); if the forward junction before it is at i - 1, it is taken too
   (:217); the link is on n[i - 1] and holds the bases from s on.  Reverse, mirrored: for every forward junction at i,
   in descending order, s = the first reverse junction (descending) at a position <= i; none: stop; the one at i + 1 is
   taken too; the link is on reverse(n[i + 1]) and holds the complements of the reverse bases from s on downwards.
   Cut to max_juncs; nseen += 1 per generated link, saturating at 255.  Two links are the same iff k-mer, orientation,
   length and bases are equal (gpath_hash.c:_find_or_add: orient, num_juncs, then memcmp of the packed bases).
5. Text (gpath_save_sbuf:132-224): per k-mer with links `<kmer> <nlinks>`, the links sorted by gpath_cmp (F before R,
   bases in ACGT order, a prefix before the longer link), each `<F|R> <njuncs> <nseen> <juncs> seq=<bases>
   juncpos=<i,j,..>` with seq and juncpos from gpath_fetch (gpath_checks.c:199-234).  K-MERS COME IN KEY ORDER here.
6. Totals (gpath_store.c:134-136): num_kmers_with_paths, num_paths, path_bytes = sum of (njuncs + 3) / 4.

Stats (mcx_thread_stats): the fields of mcx_correct_stats as `correct` counts them, without the end extensions (end_gaps,
end_gaps_extended and bases_filled stay 0, stops_* count the gap walks only), then contigs, contig_kmers (nodes of all
contigs), juncs_fw and juncs_rv (junctions of all contigs, whether or not links came of them) and links_added (links
generated, equal ones counted every time)."""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_restate as C  # noqa: E402

STAT_NAMES = C.STAT_NAMES + ("contigs", "contig_kmers", "juncs_fw", "juncs_rv", "links_added")
MAX_JUNCS, MAX_SEEN = 32767, 255


def new_stats():
    return dict.fromkeys(STAT_NAMES, 0)


def successors(view, node):
    """[(nucleotide, node)] over the edges of `node` whose k-mer is a key"""
    got = view.memo.get(("succ", node))
    if got is None:
        e = R.union_edges(view.graph, node[0])
        got = []
        for x in range(4):
            if (e >> (4 * node[1] + x)) & 1:
                n = C.step(node, x, view.k)
                if n[0] in view.graph:
                    got.append((x, n))
        view.memo[("succ", node)] = got
    return got


def outdegree(view, node):
    return len(successors(view, node))


def indegree(view, node):
    return len(successors(view, C.rev(node)))


def contigs(view, seq, two_way=False, D=0.1, d=5.0, stats=None, events=None):
    """correct_alignment_nxt until it returns NULL: the contigs of a read, each a list of nodes"""
    stats = new_stats() if stats is None else stats
    events = collections.Counter() if events is None else events
    got = view.memo.get(("align", seq))  # (a case is threaded several times over: one-way, two-way, other bounds)
    if got is None:
        got = view.memo[("align", seq)] = C.align(view, seq)
    aln, nocc, nkey = got
    stats["num_reads"] += 1
    stats["num_kmers"] += nocc
    stats["num_kmers_found"] += nkey
    if not aln:
        stats["num_no_kmers"] += 1
        return []
    n = len(aln)
    bound = [None] * (n + 1)
    for i in range(1, n):
        if aln[i - 1][1] + 1 != aln[i][1]:
            bound[i] = "gap"
        elif not C.has_edge(view, aln[i - 1][0], aln[i][0]):
            bound[i] = "edge"
    if "gap" not in bound and aln[0][1] == 0 and len(seq) == aln[-1][1] + view.k:
        stats["num_perfect"] += 1
        stats["missing_edges"] += "edge" in bound
    else:
        stats["missing_edges"] += bound.count("edge")
    out = [[aln[0][0]]]
    for i in range(1, n):
        if bound[i] == "edge":
            events["ended_by_missing_edge"] += 1
            out.append([])
        elif bound[i] == "gap":
            a, b = aln[i - 1][0], aln[i][0]
            est = aln[i][1] - aln[i - 1][1]
            wig = C.wiggle(est, D, d)
            gap_min, gap_max = max(0, est - wig), max(0, est + wig)
            stats["gaps"] += 1
            if two_way:
                ok, fill, gap_len = C.walk_two_way(view, a, b, gap_min, gap_max, stats)
            else:
                ok, fill = C.walk_to(view, a, b, gap_min, gap_max, stats)
                if not ok:
                    ok, back = C.walk_to(view, C.rev(b), C.rev(a), gap_min, gap_max, stats)
                    fill = [C.rev(x) for x in reversed(back)]
                    stats["gaps_filled_backward"] += ok
                gap_len = len(fill)
            if ok:
                stats["gaps_filled"] += 1
                out[-1] += fill
                if any(outdegree(view, x) > 1 or indegree(view, x) > 1 for x in fill):
                    events["junction_in_filled_gap"] += 1
            else:
                stats["gaps_too_short" if gap_len < gap_min else "gaps_too_long_or_stopped"] += 1
                events["ended_by_failed_gap"] += 1
                out.append([])
        out[-1].append(aln[i][0])
    stats["contigs"] += len(out)
    stats["contig_kmers"] += sum(len(c) for c in out)
    return out


def junctions(view, nodes):
    """([(position, base)] forward, [(position, base)] reverse), both in ascending position"""
    k, fw, rv = view.k, [], []
    for i, n in enumerate(nodes):
        if i + 1 < len(nodes) and outdegree(view, n) > 1:
            fw.append((i, C.last_nuc(nodes[i + 1], k)))
        if i > 0 and indegree(view, n) > 1:
            rv.append((i, C.first_nuc(nodes[i - 1], k)))
    return fw, rv


def contig_links(view, nodes, max_juncs=MAX_JUNCS, stats=None, events=None):
    """the links of one contig in the order they are generated: [(key, orient, (bases))]"""
    events = collections.Counter() if events is None else events
    fw, rv = junctions(view, nodes)
    if stats is not None:
        stats["juncs_fw"] += len(fw)
        stats["juncs_rv"] += len(rv)
    if not fw or not rv:
        events["one_kind_only"] += bool(fw or rv)
        return []
    out = []
    for i, _ in rv:  # forward links
        s = next((j for j, (p, _) in enumerate(fw) if p >= i), None)
        if s is None:
            break
        if s > 0 and fw[s - 1][0] == i - 1:
            s -= 1
            events["step_back"] += 1
        key, o = nodes[i - 1]
        out.append((key, o, tuple(b for _, b in fw[s:][:max_juncs])))
    dn = rv[::-1]
    for i, _ in reversed(fw):  # reverse links
        s = next((j for j, (p, _) in enumerate(dn) if p <= i), None)
        if s is None:
            break
        if s > 0 and dn[s - 1][0] == i + 1:
            s -= 1
            events["step_back"] += 1
        key, o = C.rev(nodes[i + 1])
        out.append((key, o, tuple(3 - b for _, b in dn[s:][:max_juncs])))
        events["reverse_link"] += 1
    events["same_link_twice_in_contig"] += len(out) - len(set(out))
    if stats is not None:
        stats["links_added"] += len(out)
    return out


class Store:
    """the links of a graph: {(key, orient, bases): nseen}, the contig histogram, the stats and what check_reach asks"""

    def __init__(self, graph, k, max_juncs=0, view=None):
        self.view = view or C.View(graph, k, 0)  # (a view may be shared: it keeps what was worked out for a node or a read)
        self.k, self.max_juncs = k, max_juncs or MAX_JUNCS
        self.reset()

    def reset(self):
        self._text = {}
        self.links = {}
        self.hist = collections.Counter()
        self.stats = new_stats()
        self.events = collections.Counter()

    def thread(self, reads, two_way=False, D=0.1, d=5.0):
        self._text = {}
        for seq in reads:
            mine = []
            for nodes in contigs(self.view, seq, two_way, D, d, self.stats, self.events):
                self.hist[len(nodes) + self.k - 1] += 1
                mine += contig_links(self.view, nodes, self.max_juncs, self.stats, self.events)
            self.events["same_link_twice_by_one_read"] += len(mine) > len(set(mine))
            for link in mine:
                self.links[link] = min(MAX_SEEN, self.links.get(link, 0) + 1)
        return self

    def info(self):
        return {"num_kmers_with_paths": len({key for key, _, _ in self.links}), "num_paths": len(self.links),
                "path_bytes": sum((len(b) + 3) // 4 for _, _, b in self.links)}

    def contig_hist(self):
        return sorted(self.hist.items())

    def by_kmer(self):
        """[(key, [(orient, bases, nseen)] in gpath_cmp order)] in key order"""
        per = collections.defaultdict(list)
        for (key, o, bases), n in self.links.items():
            per[key].append((o, bases, n))
        return [(key, sorted(per[key])) for key in sorted(per)]

    def fetch(self, key, o, bases):
        """gpath_fetch: (nodes, juncpos)"""
        node, nodes, pos, nj = (key, o), [(key, o)], [], 0
        while nj < len(bases):
            succ = successors(self.view, node)
            if not succ:
                break
            if len(succ) > 1:
                nxt = [n for x, n in succ if x == bases[nj]]
                if not nxt:
                    break
                pos.append(len(nodes) - 1)
                nj += 1
                node = nxt[0]
            else:
                node = succ[0][1]
            nodes.append(node)
        return nodes, pos

    def text(self, seq=True):
        if seq not in self._text:
            self._text[seq] = self._make_text(seq)
        return self._text[seq]

    def _make_text(self, seq):
        out = []
        for key, links in self.by_kmer():
            out.append("%s %d\n" % (kmer_str(key, self.k), len(links)))
            for o, bases, n in links:
                line = "%s %d %d %s" % ("FR"[o], len(bases), n, "".join("ACGT"[b] for b in bases))
                if seq:
                    nodes, pos = self.fetch(key, o, bases)
                    line += " seq=%s juncpos=%s" % (C.contig_str(self.k, nodes), ",".join(map(str, pos)))
                out.append(line + "\n")
        return "".join(out).encode()

    def prefix_pairs(self):
        """k-mers that hold two links of one orientation of which one is a prefix of the other"""
        n = 0
        for _, links in self.by_kmer():
            n += any(a[0] == b[0] and len(a[1]) < len(b[1]) and b[1][:len(a[1])] == a[1] for a, b in zip(links, links[1:]))
        return n


def kmer_str(key, k):
    return "".join("ACGT"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k))

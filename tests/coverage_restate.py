"""Pure-Python restatement of `mccortex<K> coverage` (src/commands/ctx_coverage.c, src/graph/db_node.h), with no device
involved.

print_read_covg: a read of len bases has klen = max(len - k + 1, 0) values per colour, one per start position.  The
k-mers of a read are those of every maximal run of ACGTacgt that is at least k long (seq_contig_start / seq_contig_end
without cutoffs), looked up by canonical key.  A k-mer that is in the graph gives, per colour, its coverage and its edge
byte; every other position gives 0 and 0x00 (the buffers are zeroed first).

fetch_node_edges: when the read's k-mer is the reverse complement of the key (node.orient == REVERSE) the byte's two
nibbles change places, (e >> 4) | (e << 4) in 8 bits; the bits inside a nibble stay (the line that reversed them is
commented out in the source).

Lines, each ending in a newline:
  _covgs   "%2u" of the first value, " %2u" of every further one; nothing but the newline when klen = 0
  _edges   edges_print per k-mer, separated by one space: edges_to_char gives digits[edges_as_nibble(e, REVERSE)] =
           the upper nibble with its four bits reversed (rev_nibble), then digits[e & 0xf]; lower-case hex
  _degree  one character per k-mer, no separator: "./[" "\\-{" "]}X" [min(indegree, 2)][min(outdegree, 2)], indegree =
           popcount of the upper nibble, outdegree = popcount of the lower (edges_get_indegree / _outdegree, FORWARD)

Output per read: ">name\\nseq\\n" with the sequence as read, then per colour ">name_c<c>_edges\\n" + line (with -e),
">name_c<c>_degree\\n" + line (with -E), ">name_c<c>_covgs\\n" + line."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reads_restate as S  # noqa: E402

COVG_MAX = 2**32 - 1
SYMBOLS = ("./[", "\\-{", "]}X")
DIGITS = "0123456789abcdef"


def oriented_kmers(k, seq):
    """(start position, canonical key, orient) per k-mer occurrence; orient 1 = the key is the reverse complement of
    what the read holds (reads_restate.read_kmers' rolling, with the position and the strand kept)"""
    out, run, fw, rc = [], 0, 0, 0
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    for i, ch in enumerate(seq.upper()):
        c = S.CODE.get(ch)
        if c is None:
            run = 0
            continue
        run += 1
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        if run >= k:
            out.append((i - k + 1, min(fw, rc), 0 if fw < rc else 1))
    return out


def swap_nibbles(e):
    return ((e >> 4) | (e << 4)) & 0xff


def values(graph, k, ncols, seq):
    """(covg[c][p], edges[c][p]) for every position p of seq, with graph = {canonical key: (covgs, edges)}"""
    covg = [[0] * len(seq) for _ in range(ncols)]
    edges = [[0] * len(seq) for _ in range(ncols)]
    for p, key, o in oriented_kmers(k, seq):
        if key in graph:
            cv, ed = graph[key]
            for c in range(ncols):
                covg[c][p] = min(cv[c], COVG_MAX)
                edges[c][p] = swap_nibbles(ed[c]) if o else ed[c]
    return covg, edges


def klen(k, seq):
    return max(len(seq) - k + 1, 0)


def covg_line(vals):
    return " ".join("%2u" % v for v in vals) + "\n"


def rev_nibble(x):
    return ((x & 1) << 3) | ((x & 2) << 1) | ((x & 4) >> 1) | ((x & 8) >> 3)


def edges_line(es):
    return " ".join(DIGITS[rev_nibble(e >> 4)] + DIGITS[e & 15] for e in es) + "\n"


def degree_line(es):
    return "".join(SYMBOLS[min(bin(e >> 4).count("1"), 2)][min(bin(e & 15).count("1"), 2)] for e in es) + "\n"


def value_lines(graph, k, ncols, seq, edges=False, degrees=False):
    """the lines of one read in the order the device writes them: per colour edges?, degree?, coverage"""
    cv, ed = values(graph, k, ncols, seq)
    n, out = klen(k, seq), []
    for c in range(ncols):
        if edges:
            out.append(edges_line(ed[c][:n]))
        if degrees:
            out.append(degree_line(ed[c][:n]))
        out.append(covg_line(cv[c][:n]))
    return out


def counts(graph, k, seqs):
    """(k-mer occurrences in the reads, occurrences whose k-mer is in the graph)"""
    occ = [key for s in seqs for _, key, _ in oriented_kmers(k, s)]
    return len(occ), sum(key in graph for key in occ)


def command_text(graph, k, ncols, reads, edges=False, degrees=False):
    """stdout of `coverage` for reads = [(name, seq)]"""
    out = []
    for name, seq in reads:
        out.append(">%s\n%s\n" % (name, seq))
        lines = iter(value_lines(graph, k, ncols, seq, edges, degrees))
        for c in range(ncols):
            if edges:
                out.append(">%s_c%d_edges\n%s" % (name, c, next(lines)))
            if degrees:
                out.append(">%s_c%d_degree\n%s" % (name, c, next(lines)))
            out.append(">%s_c%d_covgs\n%s" % (name, c, next(lines)))
    return "".join(out)

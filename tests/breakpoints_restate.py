"""A CPU restatement of `breakpoints` without link files (src/commands/ctx_breakpoints.c, src/tools/breakpoint_caller.c,
src/graph/kmer_occur.{c,h}, src/graph/graph_crawler.c), written from the reference's lines as the expectation of the
device tests.

The graph is {key: (covgs, edges)} as in clean_restate; the view is that of `bubbles` / `correct`: union edges, a k-mer
is in a colour iff its value word in that colour is non-zero, an edge that names an absent k-mer counts as no edge.  The
reference colour is the last one.

The deliberate differences:
 1. breaks are taken in ascending key order, FORWARD before REVERSE, successors in ACGT order, and the call ids count up
    in output order (the reference walks its hash table with racing threads);
 2. merged flanks and merged alleles are ordered by their smallest colour, colours ascending inside a set (the reference
    orders them by cache-local unitig ids, graph_crawler.c:232-233);
 3. in the stop rule the lengths of ended runs are taken from the ended runs (breakpoint_caller.c:228-232 reads
    koruns->b[i] while it loops over koruns_ended);
 4. (the command) the header's max_ref_flank_kmers is the real -R (breakpoint_caller.c:649 passes min_ref_nkmers twice).
"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_restate as C  # noqa: E402
from bubbles_restate import successors, node_str  # noqa: E402

ACGT = "ACGT"
STAT_NAMES = ("occurrences", "ref_keys", "ref_added", "breaks", "flank_walks", "flanks", "flanks_norun", "allele_walks", "alleles",
              "alleles_norun", "calls", "steps", "runs_started", "runs_ended", "stop_runs", "stop_maxref", "stop_flank", "stop_nocovg",
              "stop_nocolcovg", "stop_nolinks", "stop_repeat", "stop_bound", "reruns")
FORWARD, REVERSE = 0, 1
PLUS, MINUS = 0, 1
MAX_CHROMS, MAX_LEN = 1 << 30, 1 << 32  # kmer_occur.h:16-17


def clean_name(name):
    """ctx_breakpoints.c: the name up to the first whitespace, then ',' -> '.' and ':' -> ';'"""
    name = name.split()[0] if name.split() else ""
    return name.replace(",", ".").replace(":", ";")


def contigs(seq, k):
    """seq_contig_start / seq_contig_end without cutoffs: (start, bases) of every maximal ACGT run of at least k bases"""
    s = seq.upper()
    i, n = 0, len(s)
    while i < n:
        if s[i] not in ACGT:
            i += 1
            continue
        j = i
        while j < n and s[j] in ACGT:
            j += 1
        if j - i >= k:
            yield i, s[i:j]
        i = j


def add_ref(graph, k, ncols, ref_seqs, ref_edges=True):
    """kograph_create with add_missing_kmers (kmer_occur.c:132-185): the genome goes into the last colour; without
    ref_edges (breakpoint_caller.c:625-626) the k-mers enter with coverage and no edge.  Returns (graph, k-mers added)."""
    ref = R.build([[]] * (ncols - 1) + [[s for q in ref_seqs for _, s in contigs(q, k)]], k)
    out = {key: (list(cv), list(ed)) for key, (cv, ed) in graph.items()}
    added = 0
    for key, (cv, ed) in ref.items():
        if key not in out:
            out[key] = ([0] * ncols, [0] * ncols)
            added += 1
        out[key][0][ncols - 1] = min(out[key][0][ncols - 1] + cv[ncols - 1], R.U32)
        if ref_edges:
            out[key][1][ncols - 1] |= ed[ncols - 1]
    return {key: (tuple(cv), ed) for key, (cv, ed) in out.items()}, added


def occurrences(graph, k, ref_seqs):
    """kograph_create passes 2 and 3 (kmer_occur.c:341-383): per key its (chrom, offset, orient) in genome order"""
    occ = collections.defaultdict(list)
    for chrom, q in enumerate(ref_seqs):
        for start, s in contigs(q, k):
            for i in range(len(s) - k + 1):
                x = R.kmer_int(s[i:i + k])
                key = R.canon(x, k)
                if key in graph:
                    occ[key].append((chrom, start + i, FORWARD if key == x else REVERSE))
    return occ


class Run:
    """KOccurRun (kmer_occur.h:44-51)"""
    __slots__ = ("chrom", "first", "last", "qoffset", "strand", "used")

    def __init__(self, chrom, first, last, qoffset, strand):
        self.chrom, self.first, self.last, self.qoffset, self.strand, self.used = chrom, first, last, qoffset, strand, False

    def __len__(self):  # korun_len
        return abs(self.last - self.first) + 1

    def sort_key(self):  # korun_cmp_qoffset:81-89
        return (self.qoffset, self.chrom, self.first, self.last)

    def tup(self):
        return (self.chrom, self.first, self.last, self.qoffset, self.strand)


def korun_extend(runs, node, kolist, new, qoffset, stats):  # kmer_occur.c:406-475 with pickup
    starti, n = 0, len(runs)
    for chrom, offset, orient in kolist:
        while starti < n and (runs[starti].chrom < chrom or runs[starti].last + 1 < offset):
            starti += 1
        used = False
        strand = PLUS if orient == node[1] else MINUS
        for i in range(starti, n):
            r = runs[i]
            if r.chrom > chrom or r.last > offset + 1:
                break
            nxt = r.last + 1 if strand == PLUS else r.last - 1
            if nxt == offset:
                new.append(Run(r.chrom, r.first, offset, r.qoffset, strand))
                r.used = True
                used = True
        if not used:
            new.append(Run(chrom, offset, offset, qoffset, strand))
            stats["runs_started"] += 1


def filter_extend(occ, nodes, min_ref, qoffset, active, ended, stats, events, is5p):  # kograph_filter_extend:493-524
    for i, node in enumerate(nodes):
        new = []
        korun_extend(active, node, occ.get(node[0], ()), new, qoffset + i, stats)
        for r in active:
            if not r.used:
                if len(r) > min_ref:
                    ended.append(r)
                    stats["runs_ended"] += 1
                elif len(r) == min_ref:
                    events["exact_run_dropped_5p" if is5p else "exact_run_dropped_3p"] += 1
                if any(q.used and q.qoffset == r.qoffset for q in active):
                    events["one_of_two_runs_ends"] += 1
        if len(new) >= 2 and len({r.chrom for r in new}) >= 2 and len({r.qoffset for r in new}) < len(new):
            events["runs_two_chroms_one_qoffset"] += 1
        active = new
    return active


def walk(graph, k, occ, colour, node, is5p, min_ref, max_ref, stats, events):
    """graph_crawler_load_path (graph_crawler.c:30-75) with gcrawler_stop_at_ref_covg (breakpoint_caller.c:195-270) as
    its jmpfunc and gcrawler_finish_ref_covg (:273-299); the walker is graph_walker_choose without links"""
    path, active, ended = [], [], []
    max_kept = 0
    entered = collections.Counter()  # rpt_walker_attempt_traverse; cleared between paths (graph_crawler.c:95-115)
    while True:
        buf = [node]
        R._extend(graph, buf, k)  # gc_create_unitig: forward from the entered node
        stats["steps"] += 1
        qoffset = len(path)
        path.extend(buf)
        active = filter_extend(occ, buf, min_ref, qoffset, active, ended, stats, events, is5p)
        kept = len(ended) + sum(len(r) >= min_ref for r in active)  # what the walk would hand out were it to end here
        if kept < max_kept:
            events["kept_runs_fell"] += 1  # (the device sizes a walk's runs by the largest such number, not the last)
        max_kept = max(max_kept, kept)
        min_run = min((r.qoffset for r in active), default=None)
        min_ended = min((r.qoffset for r in ended), default=None)
        maxlen = max((len(r) for r in active + ended), default=0)  # difference 3
        if min_ended is not None and (min_run is None or min_run > min_ended):
            stats["stop_runs"] += 1
            break
        if max_ref and maxlen >= max_ref:
            stats["stop_maxref"] += 1
            break
        if is5p and not active:
            stats["stop_flank"] += 1
            break
        cand = successors(graph, buf[-1], k)
        if not cand:
            stats["stop_nocovg"] += 1
            break
        if len(cand) == 1:
            node = cand[0]
        else:
            ins = [c for c in cand if C.in_sample(graph, c[0], colour)]
            if not ins:
                stats["stop_nocolcovg"] += 1
                break
            if len(ins) > 1:
                stats["stop_nolinks"] += 1
                break
            node = ins[0]
        entered[node] += 1
        if entered[node] >= 3:
            stats["stop_repeat"] += 1
            break
    for r in active:
        if len(r) == min_ref:
            events["exact_run_kept_5p" if is5p else "exact_run_kept_3p"] += 1
    runs = ended + [r for r in active if len(r) >= min_ref]  # koruns_filter
    return path, runs


def merge(walks):
    """graph_crawler_fetch:228-268 with difference 2: [(colours, path, runs)] in the order of their smallest colour"""
    out = []
    for colour, (path, runs) in walks:
        for m in out:
            if m[1] == path:
                m[0].append(colour)
                break
        else:
            out.append(([colour], path, runs))
    return out


def run_str(r, names, k, first_kmer_idx, kmer_offset):  # korun_gzprint:44-65
    if r.strand == PLUS:
        start, end = r.first + kmer_offset, r.last + k - 1
    else:
        start, end = r.first + k - 1 - kmer_offset, r.last
    return "%s:%d-%d:%s:%d" % (names[r.chrom], start + 1, end + 1, "+-"[r.strand], r.qoffset - first_kmer_idx + 1)


def seq_cont(nodes, k):  # db_nodes_gzprint_cont
    return "".join(ACGT[C.last_nuc(n, k)] for n in nodes)


def breaks(graph, k, occ):
    """breakpoint_caller_node:501-522 and follow_break:376-398 with difference 1"""
    for key in sorted(graph):
        if key not in occ:
            continue
        for o in (FORWARD, REVERSE):
            node = (key, o)
            nxt = successors(graph, node, k)
            nonref = [n for n in nxt if n[0] not in occ]
            if nonref:
                yield node, nxt, nonref


def call(graph, k, ncols, ref_seqs, names, min_ref=5, max_ref=1000, ref_edges=True, ref_loaded=False):
    """(records, text, stats, events, graph with the reference); a record is a dict of the fields of mcx_breakpoint_rec"""
    assert ncols >= 2 and min_ref > 0 and (not max_ref or min_ref <= max_ref)
    assert 0 < len(ref_seqs) <= MAX_CHROMS and all(len(s) <= MAX_LEN for s in ref_seqs)
    stats = dict.fromkeys(STAT_NAMES, 0)
    events = collections.Counter()
    if not ref_loaded:
        graph, stats["ref_added"] = add_ref(graph, k, ncols, ref_seqs, ref_edges)
    occ = occurrences(graph, k, ref_seqs)
    stats["occurrences"] = sum(len(v) for v in occ.values())
    stats["ref_keys"] = len(occ)
    if any(len(v) > 1 for v in occ.values()):
        events["key_occurs_twice"] += 1
    recs, text = [], []
    off = 0
    for node, nxt, nonref in breaks(graph, k, occ):
        if len(nonref) > 1:
            events["two_nonref_successors"] += 1
        if len(nxt) == 1:
            events["fork_has_one_successor"] += 1
        for succ in nonref:
            stats["breaks"] += 1
            events["break_reverse" if node[1] else "break_forward"] += 1
            walks = []
            for colour in range(ncols):  # traverse_5pflank:342-372, graph_crawler_fetch:195-226
                if C.in_sample(graph, node[0], colour) and not C.in_sample(graph, succ[0], colour) and colour < ncols - 1:
                    events["colour_lacks_successor"] += 1
                if not (C.in_sample(graph, node[0], colour) and C.in_sample(graph, succ[0], colour)):
                    continue
                stats["flank_walks"] += 1
                walks.append((colour, walk(graph, k, occ, colour, C.rev(node), True, min_ref, max_ref, stats, events)))
            ncalls_before = len(recs)
            for cols5, path5, runs5 in merge(walks):
                stats["flanks"] += 1
                nf = len(path5)
                runs5 = [Run(*r.tup()) for r in runs5]
                for r in runs5:  # koruns_reverse (kmer_occur.h:124-134)
                    ln = r.last - r.first if r.strand == PLUS else r.first - r.last
                    r.first, r.last = r.last, r.first
                    r.strand ^= 1
                    r.qoffset = nf - 1 - r.qoffset - ln
                runs5.sort(key=Run.sort_key)
                flank = [C.rev(n) for n in reversed(path5)]
                if not runs5:
                    stats["flanks_norun"] += 1
                    continue
                walks3 = []
                for colour in cols5:  # follow_break:453-471
                    stats["allele_walks"] += 1
                    walks3.append((colour, walk(graph, k, occ, colour, succ, False, min_ref, max_ref, stats, events)))
                for cols3, path3, runs3 in merge(walks3):
                    stats["alleles"] += 1
                    runs3 = sorted(runs3, key=Run.sort_key)
                    if not runs3:  # process_contig:151
                        stats["alleles_norun"] += 1
                        continue
                    flank3pidx = runs3[0].qoffset
                    extra = min(k - 1, flank3pidx)
                    path_kmers = flank3pidx - extra
                    kmer3poffset = k - 1 - extra
                    cid = len(recs)
                    t = ">brkpnt.call%d.5pflank chr=%s\n" % (cid, ",".join(run_str(r, names, k, 0, 0) for r in runs5))
                    t += node_str(flank[0], k) + seq_cont(flank[1:], k) + "\n"
                    t += ">brkpnt.call%d.3pflank chr=%s\n" % (cid, ",".join(run_str(r, names, k, flank3pidx, kmer3poffset) for r in runs3))
                    t += seq_cont(path3[path_kmers:], k) + "\n"
                    t += ">brkpnt.call%d.path cols=%s\n" % (cid, ",".join("%d" % c for c in cols3))
                    t += seq_cont(path3[:path_kmers], k) + "\n\n"
                    events["flank3pidx_below_k1" if flank3pidx < k - 1 else "flank3pidx_from_k1"] += 1
                    if any(r.strand == MINUS for r in runs3):
                        events["allele_run_minus"] += 1
                    if len(cols3) > 1:
                        events["colours_merged"] += 1
                    if len(runs3) > 1 and runs3[0].qoffset == runs3[1].qoffset and runs3[0].chrom != runs3[1].chrom:
                        events["sort_tie_on_chrom"] += 1
                    if len(runs5) > 1 and runs5[0].qoffset == runs5[1].qoffset and runs5[0].chrom != runs5[1].chrom:
                        events["sort_tie_on_chrom"] += 1
                    recs.append(dict(fork_key=node[0], fork_orient=node[1], succ_base=C.last_nuc(succ, k), num_cols=len(cols3),
                                     path_kmers=path_kmers, flank5p_kmers=len(flank), flank3p_kmers=len(path3) - path_kmers,
                                     flank5p_runs=len(runs5), flank3p_runs=len(runs3), text_off=off, text_len=len(t)))
                    text.append(t)
                    off += len(t)
                    stats["calls"] += 1
            if len(recs) - ncalls_before >= 2:
                events["two_calls_one_break"] += 1
    return recs, "".join(text), stats, events, graph


def parse_calls(text):
    """the calls of a text: dicts with id, flank5p / flank3p / path sequences, runs5 / runs3 [(name, start, end, strand,
    offset)] and cols"""
    out = []
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) % 7 == 1, len(lines)
    for i in range(0, len(lines) - 1, 7):
        h5, s5, h3, s3, hp, sp, blank = lines[i:i + 7]
        assert blank == ""
        cid = int(h5[len(">brkpnt.call"):h5.index(".5pflank")])
        assert h5.startswith(">brkpnt.call%d.5pflank chr=" % cid) and h3.startswith(">brkpnt.call%d.3pflank chr=" % cid)
        assert hp.startswith(">brkpnt.call%d.path cols=" % cid)

        def runs(h):
            res = []
            for e in h.split("chr=", 1)[1].split(","):
                name, span, strand, offset = e.split(":")
                a, b = span.split("-")
                res.append((name, int(a), int(b), strand, int(offset)))
            return res
        out.append(dict(id=cid, flank5p=s5, flank3p=s3, path=sp, runs5=runs(h5), runs3=runs(h3),
                        cols=[int(c) for c in hp.split("cols=", 1)[1].split(",")]))
    return out

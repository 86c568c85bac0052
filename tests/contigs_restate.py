"""Pure-Python restatement of `mccortex<K> contigs` (src/commands/ctx_contigs.c, src/tools/assemble_contigs.c,
src/graph/graph_walker.c, src/graph/repeat_walker.h, src/graph/contig_confidence.c), written from the reference's lines,
with no device involved.  graph = {canonical key: (covgs, edges)}; links = [(key, orient, (bases), nseen)].

1. Graph view (that of `correct`): the edges of a k-mer are the OR of its edge bytes over all colours; a k-mer is in the
   sample iff its value word in `colour` is non-zero; AN EDGE THAT NAMES AN ABSENT K-MER COUNTS AS NO EDGE.
2. Link store: the links sorted by (key, orientation, bases) with a prefix before its extensions (gpath_cmp inside a
   k-mer, key order across k-mers); a link's id is its index there.
3. Walker (graph_walker.c): held links and counter links oldest first as [id, pos, age]; segments newest first as
   [in_fork, out_fork, num_nodes] (_gw_gseg_init, _gw_gseg_update:97-147); pickup_paths:151-210;
   graph_walker_choose:371-515; _graph_walker_force_jump:525-629.  Where the reference aborts (_corrupt_paths) or would
   read past the segment list (the loop of :482 when no segment up to the oldest link's has in_fork), the walk stops with
   StopUnknown and corrupt_links counts it.
4. Assembly (_assemble_contig:50-153 without a seed link), the repeat rule (repeat_walker.h:18-50 without the Bloom
   filter's false positives: the state is compared through state_hash, which the kernel computes too), the seeding rule
   (sequential: see assemble()), the confidence table (contig_confidence.c:17-64 in numpy.longdouble) and the FASTA
   text (_dump_contig:184-194)."""
import collections
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_restate as C  # noqa: E402
from thread_restate import kmer_str  # noqa: E402

POPFWD, COLFWD, POPFRK_COLFWD, NOCOVG, NOCOLCOVG, NOLINKS, SPLIT_LINKS, MISSING_LINKS, USELINKS = range(9)
CORRUPT = 9  # (not a status of the reference: it aborts)
STATUS_NAMES = ("GoPopForward", "GoColForward", "GoPopForkColForward", "FailNoCovg", "FailNoColCovg", "FailNoLinks",
                "FailSplitLinks", "FailMissingLinks", "GoUseLinks")
STOP_UNKNOWN, STOP_NOCOVG, STOP_NOCOLCOVG, STOP_NOPATHS, STOP_SPLIT_PATHS, STOP_MISSING_PATHS, STOP_CYCLE, STOP_LOW_STEP, STOP_LOW_CUMUL = range(9)
STOP_NAMES = ("StopUnknown", "StopNoCovg", "StopPopForkNoColCovg", "StopForkNoPaths", "StopForkInPaths", "StopMissingPaths",
              "StopHitLoop", "StopLowStepConfidence", "StopLowCumulativeConfidence")
RESEED, NO_MISSING_CHECK = 1, 2
M64 = (1 << 64) - 1


def mix64(x):
    """the finaliser of splitmix64"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


class Links:
    """the store: ids in store order, and per oriented node its ids"""

    def __init__(self, links):
        merged = {}
        for key, o, bases, n in links:
            t = (key, o, tuple(bases))
            merged[t] = min(255, merged.get(t, 0) + n)
        self.all = sorted(merged)
        self.bases = [b for _, _, b in self.all]
        self.per = {}
        for i, (key, o, _) in enumerate(self.all):
            self.per.setdefault((key, o), []).append(i)

    def of(self, node):
        return self.per.get(node, [])


class View:
    def __init__(self, graph, k, colour=0):
        self.graph, self.k, self.colour = graph, k, colour
        self.memo = {}

    def in_sample(self, node):
        return C.in_sample(self.graph, node[0], self.colour)

    def successors(self, node):
        """[(nucleotide, node)] over the union edges, in ACGT order, whose k-mer is a key"""
        got = self.memo.get(node)
        if got is None:
            e = R.union_edges(self.graph, node[0])
            got = []
            for x in range(4):
                if (e >> (4 * node[1] + x)) & 1:
                    n = C.step(node, x, self.k)
                    if n[0] in self.graph:
                        got.append((x, n))
            self.memo[node] = got
        return got

    def outdegree_in_col(self, node):
        return sum(self.in_sample(n) for _, n in self.successors(node))


class Walker:
    def __init__(self, view, links, check=True):
        self.v, self.links, self.check = view, links, check
        self.events = collections.Counter()  # what the case set is asked to reach beside the statuses

    def base(self, f):
        return self.links.bases[f[0]][f[1]]

    def start(self, node):
        self.node = node
        self.held, self.cntr = [], []
        self.segs = [[False, False, 1]]
        self.fork_count = 0
        self.npicked = 0  # links held at any time since the start
        self.pickup(node, False, 0)

    def pickup(self, node, counter, next_base):
        if not self.v.in_sample(self.node):
            return
        buf = self.cntr if counter else self.held
        filt = counter and self.v.outdegree_in_col(node) > 1
        for i in self.links.of(node):
            if not filt:
                buf.append([i, 0, 0])
                self.npicked += not counter
            elif self.links.bases[i][0] == next_base and 1 < len(self.links.bases[i]):
                buf.append([i, 1, 0])
                self.events["counter_link_past_its_first_base"] += 1
            else:
                self.events["counter_link_filtered"] += 1

    def choose(self):
        """(successor or None, status, path_gap)"""
        succ = self.v.successors(self.node)
        if not succ:
            return None, NOCOVG, 0
        if len(succ) == 1:
            return succ[0], (COLFWD if self.v.in_sample(succ[0][1]) else POPFWD), 0
        ins = [s for s in succ if self.v.in_sample(s[1])]
        if len(ins) == 1:
            return ins[0], POPFRK_COLFWD, 0
        if not ins:
            return None, NOCOLCOVG, 0
        if not self.held:
            return None, NOLINKS, 0
        forks = {x for x, _ in ins}
        taken = {self.base(f) for f in self.held + self.cntr}
        if taken - forks:
            return None, CORRUPT, 0
        age, nuc = self.held[0][2], self.base(self.held[0])
        if age == 0:
            return None, NOLINKS, 0
        i = 1
        while i < len(self.held) and self.base(self.held[i]) == nuc:
            i += 1
        if i < len(self.held) and self.held[i][2] == age:
            return None, SPLIT_LINKS, 0
        at = self.held[i][2] if i < len(self.held) else 0
        while at < len(self.segs) and not self.segs[at][0]:
            at += 1
        if at >= len(self.segs):
            return None, CORRUPT, 0
        gap = sum(s[2] for s in self.segs[:at + 1])
        if self.check and len(taken) < len(ins):
            return None, MISSING_LINKS, gap
        self.events["choice_age_above_0"] += i < len(self.held) and self.held[i][2] > 0
        self.events["gap_over_several_segments"] += at > 0
        self.events["counter_link_answers_the_check"] += self.check and len({self.base(f) for f in self.held}) < len(ins)
        return [s for s in ins if s[0] == nuc][0], USELINKS, gap

    def force(self, node, is_fork):
        k = self.v.k
        lost = C.first_nuc(self.node, k)
        self.node = node
        if is_fork:
            b = C.last_nuc(node, k)
            held = []
            for f in self.held:
                if self.base(f) == b:
                    f[1] += 1
                    if f[1] < len(self.links.bases[f[0]]):
                        held.append(f)
                    else:
                        self.events["link_finished_at_fork"] += 1
            self.held = held
            cntr = []
            for f in self.cntr:
                if self.base(f) == b and f[1] + 1 < len(self.links.bases[f[0]]):
                    f[1] += 1
                    cntr.append(f)
            self.cntr = cntr
            self.fork_count += 1
        prevs = []
        if self.v.in_sample(node):
            prevs = [C.rev(n) for x, n in self.v.successors(C.rev(node)) if x != 3 - lost and self.v.in_sample(n)]
            if self.check:
                nb = C.last_nuc(node, k)
                for p in prevs:
                    self.pickup(p, True, nb)
        self.seg_update(is_fork, bool(prevs))
        self.pickup(node, False, 0)

    def seg_update(self, fw_fork, rv_fork):
        self.segs[0][1] |= fw_fork
        if fw_fork or rv_fork:
            self.segs.insert(0, [rv_fork, False, 0])
            for f in self.held + self.cntr:
                f[2] += 1
            keep = 1
            if self.held:
                keep = max(keep, self.held[0][2] + 1)
            if self.cntr:
                keep = max(keep, self.cntr[0][2] + 1)
            del self.segs[keep:]
        self.segs[0][2] += 1

    def next(self):
        """one graph_walker_next: (moved, status, path_gap)"""
        s, status, gap = self.choose()
        if s is None:
            return False, status, gap
        self.force(s[1], status in (POPFRK_COLFWD, USELINKS))
        return True, status, gap

    def state_hash(self):
        h = 0
        for buf in (self.held, self.cntr):
            h = mix64(h ^ len(buf))
            for i, pos, age in buf:
                h = mix64(h ^ i)
                h = mix64(h ^ (pos | (len(self.links.bases[i]) << 32)))
                h = mix64(h ^ age)
        return h


def new_stats():
    return {"contigs": 0, "num_reseed_abort": 0, "seeds_not_found": 0, "stop_causes": [0] * 9, "wlk_steps": [0] * 9,
            "total_nodes": 0, "total_junc": 0, "corrupt_links": 0, "events": collections.Counter()}


def assemble_contig(view, links, key, conf, min_step=-1.0, min_cumul=-1.0, check=True):
    """_assemble_contig for the seed `key`: (record, nodes)"""
    k = view.k
    nodes = [(key, 0)]
    rec = {"seed": key, "num_junc": 0, "paths_held": [0, 0], "paths_cntr": [0, 0], "max_step_gap": [0, 0], "gap_conf": [1.0, 1.0],
           "stop_causes": [0, 0], "wlk_steps": [0] * 9, "corrupt": 0}
    w = Walker(view, links, check)
    for d in (0, 1):
        if d == 1:
            nodes = [C.rev(n) for n in reversed(nodes)]
        w.start(nodes[-1])
        seen_first, seen_states = set(), {}
        cause = None
        while True:
            moved, status, gap = w.next()
            if not moved:
                break
            nodes.append(w.node)
            rec["wlk_steps"][status] += 1
            if status == USELINKS:
                gap_length = gap + k + 1
                confid = float(conf[gap_length]) if gap_length < len(conf) else 0.0
                rec["max_step_gap"][d] = max(rec["max_step_gap"][d], gap_length)
                rec["gap_conf"][d] = float(np.float64(rec["gap_conf"][d]) * np.float64(confid))
                if confid < min_step:
                    cause = STOP_LOW_STEP
                    break
                if rec["gap_conf"][d] < min_cumul:
                    cause = STOP_LOW_CUMUL
                    break
            if w.node not in seen_first:
                seen_first.add(w.node)
            else:
                h = w.state_hash()
                if h in seen_states.setdefault(w.node, set()):
                    cause = STOP_CYCLE
                    w.events["stopped_by_an_equal_state_after_rounds_with_links"] += w.npicked > 0
                    break
                w.events["entered_again_in_another_state" if seen_states[w.node] else "entered_again"] += 1
                seen_states[w.node].add(h)
        rec["num_junc"] += w.fork_count
        rec["paths_held"][d], rec["paths_cntr"][d] = len(w.held), len(w.cntr)
        if cause is None:
            if status == CORRUPT:
                cause = STOP_UNKNOWN
                rec["corrupt"] += 1
            else:
                cause = {NOCOVG: STOP_NOCOVG, NOCOLCOVG: STOP_NOCOLCOVG, NOLINKS: STOP_NOPATHS, SPLIT_LINKS: STOP_SPLIT_PATHS,
                         MISSING_LINKS: STOP_MISSING_PATHS}[status]
        rec["stop_causes"][d] = cause
    rec["outdegree_rv"] = view.outdegree_in_col(C.rev(nodes[0]))
    rec["outdegree_fw"] = view.outdegree_in_col(nodes[-1])
    rec["len_nodes"] = len(nodes)
    rec["events"] = w.events
    return rec, nodes


def assemble(graph, k, links, conf, colour=0, flags=0, ncontigs=0, min_step=-1.0, min_cumul=-1.0, seeds=None):
    """mcx_graph_contigs: (records, sequence bytes, stats).  Seeds in order: every key in the sample ascending, or the
    seed reads (strings of k bases) in input order.  Without RESEED a seed gives a contig iff its k-mer is not among the
    nodes of a contig kept before it.  Only the first `ncontigs` kept contigs exist."""
    view = View(graph, k, colour)
    store = links if isinstance(links, Links) else Links(links)
    st = new_stats()
    if seeds is None:
        cand = [key for key in sorted(graph) if view.in_sample((key, 0))]
    else:
        cand = []
        for s in seeds:
            if len(s) != k or set(s) - set("ACGT"):
                raise ValueError("a seed must be k bases of ACGT")
            key = R.canon(R.kmer_int(s), k)
            if key not in graph:
                st["seeds_not_found"] += 1
            elif view.in_sample((key, 0)):
                cand.append(key)
    visited, recs, text = set(), [], []
    for key in cand:
        if ncontigs and len(recs) >= ncontigs:
            break
        if not (flags & RESEED) and key in visited:
            st["num_reseed_abort"] += 1
            continue
        rec, nodes = assemble_contig(view, store, key, conf, min_step, min_cumul, not (flags & NO_MISSING_CHECK))
        if not (flags & RESEED):
            visited.update(n[0] for n in nodes)
        rec["seq_off"] = sum(len(t) for t in text)
        recs.append(rec)
        text.append(C.contig_str(k, nodes).encode() + b"\n")
        st["contigs"] += 1
        st["total_nodes"] += len(nodes)
        st["total_junc"] += rec["num_junc"]
        st["corrupt_links"] += rec["corrupt"]
        st["events"].update(rec.pop("events"))
        for d in (0, 1):
            st["stop_causes"][rec["stop_causes"][d]] += 1
        for i in range(9):
            st["wlk_steps"][i] += rec["wlk_steps"][i]
    return recs, b"".join(text), st


# ---- the confidence table (contig_confidence.c) ---------------------------------------------------------------------
def calc_confid(covg, read_len, kmer_size):
    """calc_confid:17-27: doubles, with the three exponentials in long double (expl)"""
    ld = np.longdouble
    lam = np.float64(covg) / np.float64(read_len)
    read_kmers = np.float64(float(read_len - kmer_size + 1))
    inner = np.exp(ld(-lam * read_kmers))
    power = (ld(1.0) - inner) * np.exp(ld(-lam) * inner)
    return np.float64(power)


def conf_table(hist, genome_size):
    """conf_table_update_hist over hist = {contig length: count} (or a list indexed by length): the table as a list of
    doubles indexed by gap distance, entry 0 unused"""
    items = sorted(hist.items()) if isinstance(hist, dict) else [(i, n) for i, n in enumerate(hist)]
    table = []
    with np.errstate(all="ignore"):
        for length, num in items:
            if length < 1 or not num:
                continue
            if len(table) < length + 1:
                table += [np.float64(0.0)] * (length + 1 - len(table))
            covg = np.float64(float(length * num)) / np.float64(float(genome_size))
            for i in range(1, length + 1):
                old = table[i]
                table[i] = np.float64(1.0) - ((np.float64(1.0) - old) * (np.float64(1.0) - calc_confid(covg, length, i)))
    return [float(x) for x in table]


def conf_csv(table):
    """conf_table_print of a one-colour table"""
    out = ["gap_dist\tconfidence_0\n"]
    for i in range(1, len(table)):
        out.append("%d\t%.5f\n" % (i, table[i]))
    return "".join(out)


# ---- the FASTA text (_dump_contig) ----------------------------------------------------------------------------------
def fasta(k, recs, seq):
    """the command's output for the records and the sequence bytes of assemble()"""
    out = []
    for i, r in enumerate(recs):
        n = r["len_nodes"] + k - 1
        bases = seq[r["seq_off"]:r["seq_off"] + n].decode()
        out.append(">contig%d len=%d seed=%s seedkmers=1 lf.status=%s lf.paths.held=%d lf.paths.cntr=%d lf.max_gap=%d lf.conf=%f "
                   "rt.status=%s rt.paths.held=%d rt.paths.cntr=%d rf.max_gap=%d rf.conf=%f\n%s\n"
                   % (i, r["len_nodes"], kmer_str(R.revcomp(r["seed"], k), k), STOP_NAMES[r["stop_causes"][0]], r["paths_held"][0],
                      r["paths_cntr"][0], r["max_step_gap"][0], r["gap_conf"][0], STOP_NAMES[r["stop_causes"][1]], r["paths_held"][1],
                      r["paths_cntr"][1], r["max_step_gap"][1], r["gap_conf"][1], bases))
    return "".join(out)


def bits(x):
    """a double as its 64 bits"""
    return struct.unpack("<Q", struct.pack("<d", x))[0]

"""A CPU restatement of `bubbles` without link files (src/commands/ctx_bubbles.c, src/tools/bubble_caller.c,
src/graph/graph_crawler.c, src/graph/graph_cache.c, src/graph/graph_crawler.h:113-121, src/graph/repeat_walker.h:18-50,
src/graph/graph_walker.c:371-515), written from the reference's lines as the expectation of the device tests.

The graph is {key: (covgs, edges)} as in clean_restate; the view is that of `correct`: union edges, a k-mer is in a
sample iff its value word in that colour is non-zero, an edge that names an absent k-mer counts as no edge.

The one deliberate difference: forks are taken in ascending key order, FORWARD before REVERSE (the reference walks its
hash table with racing threads), and the bubble ids count up in that order.
"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_restate as C  # noqa: E402
import unitigs_restate as U  # noqa: E402

ACGT = "ACGT"
STAT_NAMES = ("forks", "paths", "steps", "stop_limit", "stop_nocovg", "stop_nocolcovg", "stop_nolinks", "stop_repeat",
              "candidates", "bubbles", "branches", "haploid_dropped", "serial_dropped")
FORWARD, REVERSE = 0, 1


def successors(graph, node, k):
    """db_graph_next_nodes over the union edges, ACGT order, the k-mers that are keys only"""
    ue = R.union_edges(graph, node[0])
    out = []
    for x in range(4):
        if (ue >> (4 * node[1] + x)) & 1:
            n = C.step(node, x, k)
            if n[0] in graph:
                out.append(n)
    return out


class Cache:
    """graph_cache.c for one fork: unitigs with local ids in the order they are first stepped on, steps, paths"""

    def __init__(self, graph, k):
        self.graph, self.k = graph, k
        self.units = []        # normalised node lists (db_unitig_normalise)
        self.node2unit = {}
        self.unit_steps = []   # per unitig: its step ids, newest first (GCacheUnitig.stepid, GCacheStep.next_step)
        self.steps = []        # (unitig, orient, path)
        self.paths = []        # [first step, number of steps]

    def new_path(self):        # graph_cache_new_path:45-50
        self.paths.append([len(self.steps), 0])

    def new_step(self, node):  # graph_cache_new_step:129-172, gc_create_unitig:55-114
        uid = self.node2unit.get(node)
        if uid is None:
            buf = [node]
            R._extend(self.graph, buf, self.k)
            buf = U.normalise(self.graph, buf, self.k)
            uid = len(self.units)
            self.units.append(buf)
            self.unit_steps.append([])
            self.node2unit[node] = uid
            end = C.rev(buf[-1]) if buf[0] == node else buf[0]  # get_node_at_unitig_end:117-126
            self.node2unit[end] = uid
        orient = FORWARD if self.units[uid][0] == node else REVERSE  # gc_unitig_get_orient:222-228
        sid = len(self.steps)
        self.steps.append((uid, orient, len(self.paths) - 1))
        self.unit_steps[uid].insert(0, sid)
        self.paths[-1][1] += 1
        return sid

    def word(self, sid):       # gc_step_encode_uint32
        return (self.steps[sid][0] << 1) | self.steps[sid][1]

    def first(self, sid):
        return self.paths[self.steps[sid][2]][0]

    def nodes(self, sid):      # gc_db_unitig_fetch_nodes:232-252
        uid, orient, _ = self.steps[sid]
        return self.units[uid] if orient == FORWARD else U.flip(self.units[uid])

    def words_to(self, sid):   # the words of the path up to and including the step
        return tuple(self.word(s) for s in range(self.first(sid), sid + 1))


def walk_paths(graph, k, ncols, fork, max_allele, stats, events):
    """find_bubbles:253-313 with graph_crawler_load_path_limit; the walker is graph_walker_choose without links"""
    cache = Cache(graph, k)
    nxt = successors(graph, fork, k)
    for colour in range(ncols):
        if not C.in_sample(graph, fork[0], colour):
            continue
        for n in nxt:
            if not C.in_sample(graph, n[0], colour):
                continue
            cache.new_path()
            stats["paths"] += 1
            entered = collections.Counter()  # rpt_walker_attempt_traverse; cleared between paths (graph_crawler.c:95-115)
            node, total = n, 0
            while True:
                sid = cache.new_step(node)
                stats["steps"] += 1
                total += len(cache.units[cache.steps[sid][0]])  # gcrawler_load_path_limit_kmer_len
                if total >= max_allele:
                    stats["stop_limit"] += 1
                    break
                cand = successors(graph, cache.nodes(sid)[-1], k)
                if not cand:
                    stats["stop_nocovg"] += 1
                    break
                if len(cand) == 1:
                    node = cand[0]
                    if not C.in_sample(graph, node[0], colour):
                        events["popfwd"] += 1
                else:
                    ins = [c for c in cand if C.in_sample(graph, c[0], colour)]
                    if not ins:
                        stats["stop_nocolcovg"] += 1
                        break
                    if len(ins) > 1:
                        stats["stop_nolinks"] += 1
                        break
                    node = ins[0]
                    events["popfrk_colfwd"] += 1
                entered[node] += 1
                if entered[node] >= 3:  # first entry: marked; second: the state goes into the filter; third: it is there
                    stats["stop_repeat"] += 1
                    break
    return cache


def is_3p_flank(cache, ends, events):  # graph_cache_is_3p_flank:337-381
    if len(ends) <= 1:
        return False
    w0 = cache.word(cache.first(ends[0]))
    if all(cache.word(cache.first(s)) == w0 for s in ends[1:]):
        events["3p_first_equal"] += 1
        return False

    def prev(s):
        return None if s == cache.first(s) else cache.word(s - 1)
    p0 = prev(ends[0])
    if p0 is None:
        ok = any(prev(s) is not None for s in ends[1:])
    else:
        ok = any(prev(s) is None or prev(s) != p0 for s in ends[1:])
    if not ok:
        events["3p_prev_equal"] += 1
    return ok


def remove_dupes(cache, ends, events):  # graph_cache_remove_dupes:384-400, graph_cache_steps_cmp:274-298
    srt = sorted(ends, key=cache.words_to)
    out = [s for i, s in enumerate(srt) if i + 1 == len(srt) or cache.words_to(s) != cache.words_to(srt[i + 1])]
    if len(out) < len(srt):
        events["dupes_removed"] += 1
    return out


def step_has_colour(cache, sid, colour):  # graph_cache_step_has_colour:417-431
    g = cache.graph
    return all(C.in_sample(g, key, colour) for s in range(cache.first(sid), sid + 1) for key, _ in cache.units[cache.steps[s][0]])


def remove_haploid(cache, ends, haploid):  # remove_haploid_paths:354-384
    ends = list(ends)
    n = len(ends)
    seen = [False] * len(haploid)
    p = 0
    while p < n:
        drop = False
        for r, col in enumerate(haploid):
            if step_has_colour(cache, ends[p], col):
                if seen[r]:
                    drop = True
                    break
                seen[r] = True
        if drop:
            ends[p], ends[n - 1] = ends[n - 1], ends[p]
            n -= 1
        else:
            p += 1
    return ends[:n]


def all_share_unitig(cache, ends):  # paths_all_share_unitig:315-350
    cnt = collections.Counter()
    for s in ends:
        for t in range(cache.first(s), s):
            cnt[cache.word(t)] += 1
    return any(v == len(ends) for v in cnt.values())


def filter_bubbles(cache, ends, haploid, keep_serial, stats, events):  # filter_bubbles:387-421
    """the end steps that make a call, in the order of its branches, or None"""
    stats["candidates"] += 1
    if not is_3p_flank(cache, ends, events):
        return None
    ends = remove_dupes(cache, ends, events)
    if len(ends) < 2:
        events["all_dupes"] += 1
        return None
    ends = remove_haploid(cache, ends, haploid)
    if len(ends) < 2:
        stats["haploid_dropped"] += 1
        return None
    if not keep_serial and all_share_unitig(cache, ends):
        stats["serial_dropped"] += 1
        return None
    return ends


def branch_nodes(cache, sid):  # gc_step_fetch_nodes:260-267
    return [n for q in range(cache.first(sid), sid) for n in cache.nodes(q)]


def alleles_between(graph, k, ncols, flank5p, flank3p, max_allele=100):
    """src/tests/bubble_caller_tests.c:_call_bubble: the branches, spelled as db_nodes_to_str does, of the candidate that
    starts with the first k-mer of flank3p, called from the fork at the last k-mer of flank5p"""
    def node_of(s):
        x = R.kmer_int(s)
        key = R.canon(x, k)
        return (key, 0 if key == x else 1)
    fork, node3 = node_of(flank5p[-k:]), node_of(flank3p[:k])
    assert len(successors(graph, fork, k)) > 1
    stats, events = dict.fromkeys(STAT_NAMES, 0), collections.Counter()
    cache = walk_paths(graph, k, ncols, fork, max_allele, stats, events)
    uid = cache.node2unit[node3]
    orient = FORWARD if cache.units[uid][0] == node3 else REVERSE
    ends = [s for s in cache.unit_steps[uid] if cache.steps[s][1] == orient]
    ends = filter_bubbles(cache, ends, (), False, stats, events) or []
    out = []
    for s in ends:
        nodes = branch_nodes(cache, s)
        out.append(node_str(nodes[0], k) + "".join(ACGT[C.last_nuc(n, k)] for n in nodes[1:]))
    return out


def node_str(node, k):
    x = C.oriented(node, k)
    return "".join(ACGT[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def branch_to_str(nodes, k, first_kmer):  # branch_to_str:136-159
    s = node_str(nodes[0], k) if first_kmer else ""
    return s + "".join(ACGT[C.last_nuc(n, k)] for n in nodes[1 if first_kmer else 0:]) + "\n"


def flank5p(graph, k, fork, max_flank):  # print_bubble:170-178
    buf = [C.rev(fork)]
    R._extend(graph, buf, k)
    buf = buf[:max_flank]  # db_unitig_extend adds no node beyond `limit`
    return [C.rev(n) for n in reversed(buf)]


def call(graph, k, ncols, max_allele, max_flank, haploid=(), keep_serial=False):
    """(records, text, stats, events); a record is a dict of the fields of mcx_bubble_rec"""
    stats = dict.fromkeys(STAT_NAMES, 0)
    events = collections.Counter()
    recs, text = [], []
    off = 0
    for key in sorted(graph):
        for o in (FORWARD, REVERSE):
            fork = (key, o)
            if len(successors(graph, fork, k)) <= 1:  # bubble_caller_node:474-487
                continue
            stats["forks"] += 1
            events["fork_reverse" if o else "fork_forward"] += 1
            cache = walk_paths(graph, k, ncols, fork, max_allele, stats, events)
            flank = None
            for uid in range(len(cache.units)):  # write_bubbles_to_file:451-472, find_bubbles_ending_with:425-449
                for orient in (FORWARD, REVERSE):
                    ends = [s for s in cache.unit_steps[uid] if cache.steps[s][1] == orient]
                    if len(ends) < 2:
                        continue
                    ends = filter_bubbles(cache, ends, haploid, keep_serial, stats, events)
                    if ends is None:
                        continue
                    if flank is None:
                        flank = flank5p(graph, k, fork, max_flank)
                    cid = len(recs)
                    f3 = cache.nodes(ends[0])
                    t = ">bubble.call%d.5pflank kmers=%d\n" % (cid, len(flank)) + branch_to_str(flank, k, True)
                    t += ">bubble.call%d.3pflank kmers=%d\n" % (cid, len(f3)) + branch_to_str(f3, k, False)
                    for i, s in enumerate(ends):
                        nodes = branch_nodes(cache, s)
                        t += ">bubble.call%d.branch.%d kmers=%d\n" % (cid, i, len(nodes)) + branch_to_str(nodes, k, False)
                        if not nodes:
                            events["branch_empty"] += 1
                        if s - cache.first(s) > 1:
                            events["branch_multi_unitig"] += 1
                        if len(nodes) == k:
                            events["branch_k_kmers"] += 1
                    t += "\n"
                    if orient == REVERSE:
                        events["call_reverse_list"] += 1
                    if len(ends) >= 3:
                        events["call_three_branches"] += 1
                    if len(flank) == 1:
                        events["flank_one"] += 1
                    if len(flank) == max_flank:
                        full = [C.rev(fork)]
                        R._extend(graph, full, k)
                        if len(full) > max_flank:
                            events["flank_cut"] += 1
                    recs.append(dict(fork_key=key, fork_orient=o, num_branches=len(ends), flank5p_kmers=len(flank),
                                     flank3p_kmers=len(f3), text_off=off, text_len=len(t)))
                    text.append(t)
                    off += len(t)
                    stats["bubbles"] += 1
                    stats["branches"] += len(ends)
    return recs, "".join(text), stats, events

"""A CPU restatement of `popbubbles` (src/commands/ctx_pop_bubbles.c, src/tools/pop_bubbles.c, the unitig iterator
of src/graph/db_unitig.c, db_graph_prev_nodes_with_mask of src/graph/db_graph.c, src/graph/prune_nodes.c), written
from the reference's semantics as the expectation of the device tests.  It is sequential and literal: `visited` and
`rmvbits` are kept per k-mer and every alternative branch is walked with db_unitig_extend from the iterating side,
so nothing is assumed about the parallel relation being symmetric.

Scope: graphs that clean_restate.unitigs() can split, that is, whose unitigs partition the k-mers.  One-sided edges
can break that (db_unitig_extend walks on over an edge whose target has one edge back, wherever that edge leads);
unitigs() then asserts and pop() with it.  On the graphs it accepts, an alternative can still be a fragment of a
unitig; `fragments` counts those, and the device tests require the count to be zero.  The device refuses such
graphs, and somewhat more: it refuses whenever a left sibling of a unitig with siblings at both ends lies inside a
unitig, without looking whether the fragment would have ended at a right sibling (include/mcx_gpu.h).

A graph is clean_restate's: {key: (covgs, edges per colour)}.  All colours count as one: the union of the edges,
db_node_sum_covg for the coverage.

Where the reference leaves the answer to its threads and its hash table, this is the project's choice:

  * every unitig is taken in its normal form (db_unitig_normalise, unitigs_restate.normalise): the end with the
    lower key is its first node, a single k-mer is forward.  The reference's orientation follows the k-mer that
    seeded the unitig; it matters for `num_popped` alone, which counts a sibling once per way it is reached from
    the left end.
  * the unitigs take their turn in ascending order of E(U), the smaller of the keys of U's two end k-mers.
  * the reference skips a unitig when its lock node, the one with the lowest table index, is already visited.  The
    table index is not part of the graph: the lock node here is the k-mer with the lowest key.  (It only matters
    when a fragment of a unitig has been marked, which takes one-sided edges.)

Two places where the reference asserts and this goes on, because such graphs exist (files that have not been
through `inferedges` have one-sided edges):

  * db_graph_prev_nodes_with_mask asserts that the edge back to the node we came from exists; here the bit is
    cleared if present.
  * a neighbour named by an edge but absent from the graph is passed over (as clean_restate does)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import unitigs_restate as U  # noqa: E402


def parallel_nodes(graph, node, k):
    """get_parallel_nodes: one node out over every edge, one node back over every other edge; the siblings come
    oriented as `node` is (heading into the shared neighbour), once per way they are reached"""
    key, o = node
    s = key if o == 0 else R.revcomp(key, k)
    lost = s >> (2 * (k - 1))  # db_node_get_first_nuc
    out = []
    nib = U.nibble(graph, key, o)
    for x in range(4):
        if not (nib >> x) & 1:
            continue
        nk, no = R.step(key, o, x, k)
        if nk not in graph:
            continue
        back = U.nibble(graph, nk, 1 - no) & ~(1 << (3 - lost))  # prev_edge: cleared if present
        for z in range(4):
            if (back >> z) & 1:
                pk, po = R.step(nk, 1 - no, z, k)
                if pk in graph:
                    out.append((pk, 1 - po))
    return out


def passes(covg, klen, n1, n2, max_covg, max_klen, max_kdiff):
    """the three conditions of process_bubble: 0 and -1 both mean "ignore" for -C and -L, D >= 0 is honoured"""
    return ((not max_covg or max_covg < 0 or covg <= max_covg) and (not max_klen or max_klen < 0 or klen <= max_klen) and
            (max_kdiff < 0 or abs(n1 - n2) <= max_kdiff))


def mean_covg(graph, nodes):
    return sum(R.sum_covg(graph, kk) for kk, _ in nodes) // len(nodes)


def end_key(u):
    return min(u[0][0], u[-1][0])


def prune(graph, removed, k):
    """prune_nodes_lacking_flag: removed k-mers go; kept k-mers lose, in every colour, the edges to them (or to
    k-mers that are not in the graph at all)"""
    out = {}
    for key, (cv, ed) in graph.items():
        if key in removed:
            continue
        e = R.union_edges(graph, key)
        mask = e
        for b in range(8):
            if (e >> b) & 1:
                nk, _ = R.step(key, b >> 2, b & 3, k)
                if nk not in graph or nk in removed:
                    mask &= ~(1 << b)
        out[key] = (cv, [x & mask for x in ed])
    return out


def pop(graph, k, max_covg=-1, max_klen=-1, max_kdiff=-1, info=None):
    """pop_bubbles + prune_nodes_lacking_flag: (surviving graph, num_popped, removed k-mer count).
    info (a dict) receives pairs = bubbles examined, ties = those with equal means, fragments = alternatives that
    were not whole unitigs, removed = the removed keys"""
    us = sorted(U.unitigs(graph, k), key=end_key)
    whole = {}
    for u in us:
        whole[u[0]] = len(u)
        whole[(u[-1][0], 1 - u[-1][1])] = len(u)
    visited, rmv = set(), set()
    popped = pairs = ties = fragments = 0
    for u in us:
        keys = [kk for kk, _ in u]
        if min(keys) in visited or all(kk in visited for kk in keys):
            continue
        visited.update(keys)
        node0, node1 = (u[0][0], 1 - u[0][1]), u[-1]
        nodes0, nodes1 = parallel_nodes(graph, node0, k), parallel_nodes(graph, node1, k)
        if not nodes0 or not nodes1:
            continue
        for sk, so in nodes0:
            alt = [(sk, 1 - so)]
            R._extend(graph, alt, k)  # db_unitig_extend
            if alt[-1] not in nodes1:
                continue
            pairs += 1
            fragments += whole.get(alt[0]) != len(alt)
            m1, m2 = mean_covg(graph, u), mean_covg(graph, alt)
            ties += m1 == m2
            n1, n2 = len(u), len(alt)
            first = m1 < m2  # remove s1, else s2
            if not passes(m1 if first else m2, n1 if first else n2, n1, n2, max_covg, max_klen, max_kdiff):
                continue
            if first:
                rmv.update(keys)
            else:
                visited.update(kk for kk, _ in alt)
                rmv.update(kk for kk, _ in alt)
            popped += 1
    if info is not None:
        info.update(pairs=pairs, ties=ties, fragments=fragments, removed=set(rmv))
    return prune(graph, rmv, k), popped, len(rmv)

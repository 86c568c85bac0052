"""A CPU restatement of `subgraph` (src/commands/ctx_subgraph.c, src/tools/subgraph.c, src/graph/prune_nodes.c) over
clean_restate's graph dict, written from the reference's semantics as the expectation of the device tests.

Seeds are cut at every byte that is not a base (lower case counts as upper case) and k-merised; a seed k-mer that is
in the graph is marked, with `unitigs` its whole unitig.  `dist` explicit breadth-first levels follow, over the union
of the colours' edges on both sides; a neighbour that is not in the graph is passed over.  `invert` complements the
marked set.  What is not kept leaves, and kept k-mers lose in every colour the edges to k-mers that are gone or absent.
"""
import functools

import clean_restate as R

step = functools.lru_cache(maxsize=None)(R.step)  # (the tests run many traversals over the same graph)


def seed_kmers(seeds, k):
    """canonical keys of the seeds' k-mer occurrences, in order"""
    out = []
    for s in seeds:
        s = (s.decode() if isinstance(s, (bytes, bytearray)) else s).upper()
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if all(ch in "ACGT" for ch in w):
                out.append(R.canon(R.kmer_int(w), k))
    return out


def mark_seeds(graph, k, seeds, unitigs=False):
    """(marked set, seed k-mer occurrences)"""
    occ = seed_kmers(seeds, k)
    marked = set()
    for key in occ:
        if key in graph and key not in marked:
            marked.update(kk for kk, _ in R.unitig(graph, key, k)) if unitigs else marked.add(key)
    return marked, len(occ)


def extend(graph, k, marked, dist, edges=R.union_edges, sides=(0, 1), sizes=None):
    """`dist` levels from `marked` (which is updated): (levels that added k-mers, largest frontier).  `edges` and
    `sides` exist for the tests' guards: what a traversal over fewer edges would reach; `sizes`, a list, receives
    the size of every frontier"""
    frontier = set(marked)
    levels, maxf, d = 0, len(frontier), 0
    while d < dist and frontier:
        if sizes is not None:
            sizes.append(len(frontier))
        nxt = set()
        for key in frontier:
            e = edges(graph, key)
            for b in range(8):
                if (e >> b) & 1 and (b >> 2) in sides:
                    nk, _ = step(key, b >> 2, b & 3, k)
                    if nk in graph and nk not in marked:
                        nxt.add(nk)
        marked |= nxt
        d += 1
        levels += 1 if nxt else 0
        maxf = max(maxf, len(nxt))
        frontier = nxt
    return levels, maxf


def prune(graph, k, keep):
    """prune_nodes_lacking_flag"""
    out = {}
    for key in keep:
        e = R.union_edges(graph, key)
        mask = e
        for b in range(8):
            if (e >> b) & 1 and step(key, b >> 2, b & 3, k)[0] not in keep:  # gone, or not in the graph at all
                mask &= ~(1 << b)
        cv, ed = graph[key]
        out[key] = (cv, [x & mask for x in ed])
    return out


def subgraph(graph, k, seeds, dist=0, invert=False, unitigs=False):
    """(the pruned graph, stats as mcx_subgraph_stats without narrow_launches)"""
    marked, nocc = mark_seeds(graph, k, seeds, unitigs)
    found = len(marked)
    levels, maxf = extend(graph, k, marked, dist)
    keep = set(graph) - marked if invert else marked
    st = dict(num_seed_kmers=nocc, num_seed_found=found, nkmers_before=len(graph), nkmers_kept=len(keep),
              nkmers_removed=len(graph) - len(keep), levels=levels, max_frontier=maxf)
    return prune(graph, k, keep), st


def guards(graph, k, seeds, dist, unitigs=False):
    """what the tests ask of a randomised case before the device is touched: the number of levels that added k-mers,
    k-mers reached only over a reverse-side edge, k-mers reached only over an edge that colour 0 lacks"""
    full, _ = mark_seeds(graph, k, seeds, unitigs)
    fwd, col0 = set(full), set(full)
    levels, _ = extend(graph, k, full, dist)
    extend(graph, k, fwd, dist, sides=(0,))
    extend(graph, k, col0, dist, edges=lambda g, key: g[key][1][0])
    return dict(kept=len(full), levels=levels, only_reverse=len(full - fwd), only_other_colour=len(full - col0))
